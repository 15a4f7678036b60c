// keys.hip -- the molecule keys of the count stage: the key layout, the key build (one 64-bit key per kept read, compacted, with
// the digit histograms of the sort that follows) and the partition of the keys by owner rank.  dedup.hip counts what is built here.
//
// Replaces UmiInfo::new (umi/src/info.rs:20-37, validity of each UMI) and what DupBuilder::observe
// (tx_annotation/src/mark_dups.rs:128-155) takes from a read.  The key layout is described at the top of dedup.hip.
#include "keys.h"
#include "stage_common.h"
// ------------------------------------------------------------------------------------------------
// key layout
// ------------------------------------------------------------------------------------------------
extern "C" int crgpu_set_key_layout(crgpu_ctx *ctx, uint32_t n_features, uint32_t umi_len, uint32_t n_libs,
                                    uint32_t multiplexing_lib_mask) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, ctx->canon_set, CRGPU_ESTATE, "crgpu_set_key_layout: set the whitelist first");
    CR_REQUIRE(ctx, n_features >= 1, CRGPU_EINVAL, "n_features must be >= 1");
    CR_REQUIRE(ctx, umi_len >= 1 && umi_len <= 16, CRGPU_ERANGE, "umi_len must be 1..16");
    CR_REQUIRE(ctx, n_libs >= 1 && n_libs <= CRGPU_MAX_LIB, CRGPU_EINVAL, "n_libs must be 1..%d", CRGPU_MAX_LIB);
    KeyLayout L;
    L.bits_bc = cr_ceil_log2(ctx->n_canon);
    L.bits_feat = cr_ceil_log2(n_features);
    L.bits_lib = cr_ceil_log2(n_libs);
    L.bits_umi = 2 * umi_len;
    L.n_features = n_features;
    L.umi_len = umi_len;
    L.umi_min_len = umi_len;
    L.n_libs = n_libs;
    L.mux_mask = multiplexing_lib_mask;
    // with CRGPU_OPT_DENSE_BARCODE_KEYS the barcode field shrinks to the columns that occur (known when the first key is built)
    CR_REQUIRE(ctx, L.total_bits() <= 64 || (ctx->dense.on && L.total_bits() - L.bits_bc + 1u <= 64u), CRGPU_ERANGE,
               "molecule key needs %u bits (barcode %u + feature %u + library %u + umi %u + 1) > 64%s", L.total_bits(),
               L.bits_bc, L.bits_feat, L.bits_lib, L.bits_umi,
               ctx->dense.on ? "" : " (CRGPU_OPT_DENSE_BARCODE_KEYS shortens the barcode field to the barcodes that occur)");
    L.set = true;
    cr_dense_drop(ctx);
    ctx->dense.canon_bits = L.bits_bc;
    ctx->layout = L;
    cr_invalidate(ctx);
    return CRGPU_OK;
}

// targeted gene expression: DupBuilder::build(.., targeted_umi_min_read_count) + FeatureReference::target_set
// (mark_dups.rs:156-169,311-320; the threshold comes from _slfe_matrix_computer.mro:122-140).  on_target: n_features bytes
// (host), non-zero = the feature is in the target set; NULL or min_read_count == 0 switches the filter off.
extern "C" int crgpu_set_target_filter(crgpu_ctx *ctx, const uint8_t *on_target, uint32_t n_features, uint64_t min_read_count) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->d_on_target) CR_HIP(ctx, hipFree(ctx->d_on_target));
    ctx->d_on_target = nullptr;
    ctx->n_target_features = 0;
    ctx->target_min_reads = 0;
    if (!on_target || !min_read_count || !n_features) return CRGPU_OK;
    CR_HIP(ctx, hipMalloc((void **)&ctx->d_on_target, n_features));
    CR_HIP(ctx, hipMemcpy(ctx->d_on_target, on_target, n_features, hipMemcpyHostToDevice));
    ctx->n_target_features = n_features;
    ctx->target_min_reads = min_read_count;
    return CRGPU_OK;
}

// Per-read UMI lengths (UmiExtractor::extract_umi, cr_types/src/rna_read.rs:103-138: a read that ends early keeps
// max(min(read_len - offset, length), min_length) bases): UMIs of different lengths are different UmiSeqs, so the length
// becomes part of the key -- a tag (umi_len - length) right above the UMI bits.  Call after crgpu_set_key_layout.
extern "C" int crgpu_set_umi_min_len(crgpu_ctx *ctx, uint32_t umi_min_len) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, ctx->layout.set, CRGPU_ESTATE, "crgpu_set_umi_min_len: call crgpu_set_key_layout first");
    KeyLayout L = ctx->layout;
    CR_REQUIRE(ctx, umi_min_len >= 1 && umi_min_len <= L.umi_len, CRGPU_EINVAL, "umi_min_len must be 1..umi_len (%u)", L.umi_len);
    L.umi_min_len = umi_min_len;
    L.bits_ulen = cr_ceil_log2(L.umi_len - umi_min_len + 1);
    cr_dense_drop(ctx);
    L.bits_bc = ctx->dense.canon_bits;
    CR_REQUIRE(ctx, L.total_bits() <= 64 || (ctx->dense.on && L.total_bits() - L.bits_bc + 1u <= 64u), CRGPU_ERANGE,
               "molecule key needs %u bits with %u bits of UMI length > 64", L.total_bits(), L.bits_ulen);
    ctx->layout = L;
    cr_invalidate(ctx);
    return CRGPU_OK;
}

typedef uint32_t cr_v4u32 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 ld_stream4(const uint4 *p) {  // 16-byte load that does not stay in the caches
    const cr_v4u32 v = __builtin_nontemporal_load(reinterpret_cast<const cr_v4u32 *>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
// CRGPU_OPT_DENSE_BARCODE_KEYS: column of a whitelist rank in the BarcodeIndex, or CRGPU_MISS (DenseIndex::d_fwd)
__device__ __forceinline__ uint32_t dense_column(const uint4 *__restrict__ fwd, uint32_t rank) {
    const uint4 e = fwd[rank >> 6];
    const unsigned long long bits = ((unsigned long long)e.y << 32) | e.x;
    const uint32_t bit = rank & 63u;
    if (!((bits >> bit) & 1ull)) return CRGPU_MISS;
    return e.z + (uint32_t)__popcll(bits & ((1ull << bit) - 1ull));
}

// ------------------------------------------------------------------------------------------------
// build keys (compacting)
// ------------------------------------------------------------------------------------------------
#define KEY_ITEMS 16
#define KEY_BATCH 4  // reads whose loads are issued together: the kernel is bound by load latency, not bandwidth
#define KEY_CHUNK (256ull * KEY_ITEMS)  // reads of one workgroup round
// a row of UMI qualities as LQW dwords (rows of 4k bytes are dword aligned); LQW = 0: byte path
template <int LQW>
struct __attribute__((aligned(4))) QRow {
    uint32_t w[LQW ? LQW : 1];
};

// what a launch of either kernel takes (the host's bundle: launch_build_keys hands the members to the kernel)
struct KeyArgs {
    KL kl;
    const uint32_t *bc_idx, *umi;
    const uint8_t *umi_q;
    const uint32_t *feature;
    const uint8_t *flags;  // nullable: every read is of library 0
    uint64_t n;
    uint64_t *keys_out;
    uint32_t *vals_out;          // nullable: the read ordinal of every key
    unsigned long long *n_out;   // keys written so far
    SweepPlan plan;
    // HIST: the digits of every emitted key are counted for all passes of the sort that follows, which then needs no
    // histogram read of its own (k_global_hist)
    uint32_t *ghist;
    unsigned long long *status;  // ORDERED: one look-back word per chunk
    uint32_t *ticket;            // ORDERED: the chunk counter
    const uint8_t *ulen;         // nullable, byte path (LQW == 0) only: the UMI length of every read, umi_min_len .. umi_len
    const uint4 *dense_fwd;      // nullable: barcode rank -> column of the BarcodeIndex (CRGPU_OPT_DENSE_BARCODE_KEYS)
    uint32_t *n_unknown;         // reads whose barcode has no column
    uint32_t *lb_abort;          // the watchdog word of the ORDERED look-back (block_utils.h)
};

// ---- what a read's key is: the one statement of it ---------------------------------------------------------------------------
// the part of the rule that needs no UMI: a barcode, a feature of the reference, a library of the layout
__device__ __forceinline__ bool read_is_counted(const KL &kl, uint32_t b, uint32_t f, uint32_t fl) {
    return b != CRGPU_MISS && f != CRGPU_NO_FEATURE && f < kl.n_features && (fl & CRGPU_FLAG_LIB_MASK) < kl.n_libs;
}
// UmiInfo::new (umi/src/info.rs:20-37) on four quality bytes: bit 7 marks an N, and a base below UMI_MIN_QV = 10 is the u8
// wrapping subtraction of the offset 33
__device__ __forceinline__ void umi_quality_word(uint32_t w, bool &has_n, bool &low_q) {
    has_n |= (w & 0x80808080u) != 0u;
#pragma unroll
    for (int bb = 0; bb < 4; bb++) low_q |= (uint8_t)(((w >> (8 * bb)) & 0x7Fu) - 33u) < 10u;
}
// b: barcode rank (or column), f: feature, fl: flag byte, u: packed UMI, Lc: its length (1 .. umi_len), has_n / low_q: what its
// qualities say.  *key is written for every read; the return value tells whether the read is kept.
__device__ __forceinline__ bool key_of_read(const KL &kl, uint32_t b, uint32_t f, uint32_t fl, uint32_t u, uint32_t Lc, bool has_n,
                                            bool low_q, uint64_t *key) {
    u &= (uint32_t)lowmask(2u * Lc);
    // is_homopolymer: every adjacent pair equal (true for a 1-base UMI)
    const bool homopolymer = ((u ^ (u >> 2)) & (uint32_t)lowmask(2u * Lc - 2u)) == 0u;
    *key = ((uint64_t)b << kl.sh_bc) | ((uint64_t)f << kl.sh_feat) | ((uint64_t)(fl & CRGPU_FLAG_LIB_MASK) << kl.sh_libid) |
           ((uint64_t)(kl.umi_len - Lc) << kl.sh_lib) | ((uint64_t)u << kl.sh_umi) | ((fl & CRGPU_FLAG_NONTXOMIC) ? 1ull : 0ull);
    return read_is_counted(kl, b, f, fl) && !(has_n || homopolymer || low_q);
}

// ---- the digit histograms of the workgroup, in LDS ---------------------------------------------------------------------------
__device__ __forceinline__ void key_hist_clear(uint32_t *s_hist, const SweepPlan &plan) {
    for (uint32_t x = threadIdx.x; x < plan.n_passes * RADIX_MAX; x += 256) s_hist[x] = 0;
    __syncthreads();
}
__device__ __forceinline__ void key_hist_add(uint32_t *s_hist, const SweepPlan &plan, uint64_t key) {
    for (uint32_t p = 0; p < plan.n_passes; p++)
        atomicAdd(&s_hist[p * RADIX_MAX + ((uint32_t)(key >> plan.shift[p]) & plan.mask[p])], 1u);
}
__device__ __forceinline__ void key_hist_flush(const uint32_t *s_hist, const SweepPlan &plan, uint32_t *__restrict__ ghist) {
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < plan.n_passes * RADIX_MAX; x += 256)
        if (s_hist[x]) atomicAdd(&ghist[x], s_hist[x]);
}

// ---- the unordered compaction of a chunk -------------------------------------------------------------------------------------
// One global atomic per 4096-read chunk (same-address atomics saturate near 88 per microsecond); inside a wave the kept keys
// leave item slot by item slot, so that a store instruction writes consecutive addresses (thread-major order made 64 separate
// 100-byte pieces of every store).  first + j * step is the read ordinal of slot j, for vals_out (nullable).
__device__ __forceinline__ void emit_unordered(const uint64_t (&keys)[KEY_ITEMS], uint32_t mask, uint64_t *__restrict__ keys_out,
                                               uint32_t *__restrict__ vals_out, unsigned long long *__restrict__ n_out,
                                               uint32_t *lds, uint64_t first, uint32_t step) {
    const unsigned long long o = block_reserve_256((uint32_t)__popc(mask), n_out, lds);
    unsigned long long wo = __shfl(o, 0);  // the wave's base = the offset of its first lane
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int j = 0; j < KEY_ITEMS; j++) {
        const bool k = (mask >> j) & 1u;
        const unsigned long long m = __ballot(k);
        if (k) {
            const unsigned long long p = wo + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            keys_out[p] = keys[j];
            if (vals_out) vals_out[p] = (uint32_t)(first + (uint64_t)j * step);
        }
        wo += (uint32_t)__popcll(m);
    }
}

// ORDERED (the keys travel with their read ordinals: the DupInfo paths): the compaction keeps the read order -- chunks
// are handed out by a ticket counter and get their output offset from a decoupled look-back over `status` (one word
// per chunk: flag in the top two bits, 1 = this chunk's count, 2 = inclusive prefix), so equal keys leave in qname
// order.  The sharded path relies on it: the owner of a barcode sees only the position of a key in its receive buffer.
// Without ORDERED a chunk reserves its space with one atomic and the chunks land in arrival order.
#define BK_AGG (1ull << 62)
#define BK_INC (2ull << 62)
template <int LQW, bool HIST, bool ORDERED>
__global__ __launch_bounds__(256) void k_build_keys(const KL kl, const uint32_t *__restrict__ bc_idx,
                                                    const uint32_t *__restrict__ umi, const uint8_t *__restrict__ umi_q,
                                                    const uint32_t *__restrict__ feature, const uint8_t *__restrict__ flags,
                                                    uint64_t n, uint64_t *__restrict__ keys_out,
                                                    uint32_t *__restrict__ vals_out,
                                                    unsigned long long *__restrict__ n_out, const SweepPlan plan,
                                                    uint32_t *__restrict__ ghist, unsigned long long *__restrict__ status,
                                                    uint32_t *__restrict__ ticket, const uint8_t *__restrict__ ulen,
                                                    const uint4 *__restrict__ dense_fwd, uint32_t *__restrict__ n_unknown,
                                                    uint32_t *__restrict__ lb_abort) {  // the members of KeyArgs, one by one
    __shared__ __attribute__((aligned(8))) uint32_t lds[10];
    __shared__ unsigned long long s_c;  // ORDERED: the chunk of this round, then its output offset
    __shared__ uint32_t s_ws[KEY_ITEMS * 4];  // ORDERED: kept keys of (item slot, wave), then their exclusive prefix
    __shared__ uint32_t s_hist[HIST ? OS_MAX_PASSES * RADIX_MAX : 1];
    if (HIST) key_hist_clear(s_hist, plan);
    const uint32_t L = kl.umi_len;
    const uint64_t n_chunks = (n + KEY_CHUNK - 1) / KEY_CHUNK;
    for (uint64_t c = blockIdx.x;; c += gridDim.x) {
      if (ORDERED) {
          if (threadIdx.x == 0) s_c = atomicAdd(ticket, 1u);
          __syncthreads();
          c = s_c;
          __syncthreads();
      }
      if (c >= n_chunks) break;  // uniform
      uint64_t keys[KEY_ITEMS];
      uint32_t mask = 0;
#pragma unroll
      for (int j0 = 0; j0 < KEY_ITEMS; j0 += KEY_BATCH) {
        // every field of KEY_BATCH reads is requested before any is looked at (no load sits behind a branch)
        uint32_t vb[KEY_BATCH], vf[KEY_BATCH], vfl[KEY_BATCH], vu[KEY_BATCH], vl[KEY_BATCH];
        QRow<LQW> vq[KEY_BATCH];
#pragma unroll
        for (int jj = 0; jj < KEY_BATCH; jj++) {
            const uint64_t i = c * KEY_CHUNK + (uint64_t)(j0 + jj) * 256 + threadIdx.x;
            const bool ok = i < n;
            vb[jj] = ok ? bc_idx[i] : CRGPU_MISS;
            vf[jj] = ok ? feature[i] : CRGPU_NO_FEATURE;
            vfl[jj] = (ok && flags) ? flags[i] : 0u;
            vu[jj] = ok ? umi[i] : 0u;
            vl[jj] = (LQW == 0 && ok && ulen) ? ulen[i] : L;
            if (LQW) {
                if (ok) vq[jj] = *reinterpret_cast<const QRow<LQW> *>(umi_q + i * (uint64_t)(4 * LQW));
                else
                    for (int k = 0; k < (LQW ? LQW : 1); k++) vq[jj].w[k] = 0u;
            }
        }
#pragma unroll
        for (int jj = 0; jj < KEY_BATCH; jj++) {
            const int j = j0 + jj;
            const uint64_t i = c * KEY_CHUNK + (uint64_t)j * 256 + threadIdx.x;
            uint32_t b = vb[jj];
            if (dense_fwd && b != CRGPU_MISS) {
                b = dense_column(dense_fwd, b);
                if (b == CRGPU_MISS) atomicAdd(n_unknown, 1u);  // a barcode without reads in the tables: the call fails
            }
            // this read's UMI length (a length outside umi_min_len .. umi_len: the reference's check_range fails, no UMI)
            const uint32_t Li = LQW == 0 ? vl[jj] : L;
            const bool has_umi = LQW != 0 || (Li >= kl.umi_min_len && Li <= L);
            const uint32_t Lc = (LQW == 0 && Li >= 1u && Li <= L) ? Li : L;
            bool has_n = false, low_q = false;
            if (LQW) {
#pragma unroll
                for (int k = 0; k < (LQW ? LQW : 1); k++) umi_quality_word(vq[jj].w[k], has_n, low_q);
            } else if (read_is_counted(kl, b, vf[jj], vfl[jj]) && has_umi) {
                for (uint32_t k = 0; k < Lc; k++) {  // the same test byte by byte
                    const uint32_t q = umi_q[i * L + k];
                    has_n |= (q & 0x80u) != 0u;
                    low_q |= (uint8_t)((q & 0x7Fu) - 33u) < 10u;
                }
            }
            const bool keep = key_of_read(kl, b, vf[jj], vfl[jj], vu[jj], Lc, has_n, low_q, &keys[j]) && has_umi;
            if (keep) mask |= 1u << j;
            if (HIST && keep) key_hist_add(s_hist, plan, keys[j]);
        }
      }
      if (ORDERED) {
          // stable inside the chunk, too: output order = (item slot, wave, lane) = ascending read index
          uint32_t below[KEY_ITEMS];
          const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
          for (int j = 0; j < KEY_ITEMS; j++) {
              const unsigned long long m = __ballot((mask >> j) & 1u);
              below[j] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
              if (lane == 0) s_ws[j * 4 + wave] = (uint32_t)__popcll(m);
          }
          __syncthreads();
          if (threadIdx.x < KEY_ITEMS * 4) {  // one wave: exclusive scan of the 64 (slot, wave) counts + the look-back
              const uint32_t v = s_ws[threadIdx.x];
              const uint32_t x = wave_incl_scan<KEY_ITEMS * 4>(v, threadIdx.x);
              s_ws[threadIdx.x] = x - v;
              const uint32_t total = __shfl(x, 63);
              if (threadIdx.x == 0 && c > 0)
                  __hip_atomic_store(&status[c], BK_AGG | total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              // every lower ticket is held by a workgroup that is running or done: the chain always moves on
              const unsigned long long excl = wave_lookback(status, c, lb_abort);
              if (threadIdx.x == 0) {
                  if (excl != WAVE_LOOKBACK_ABORTED) {
                      __hip_atomic_store(&status[c], BK_INC | (excl + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                      if (c + 1 == n_chunks) *n_out = excl + total;
                  }
                  s_c = excl;
              }
          }
          __syncthreads();
          const unsigned long long base = s_c;
          if (base == WAVE_LOOKBACK_ABORTED) break;  // uniform: the host reports the stall (lb_abort is set)
#pragma unroll
          for (int j = 0; j < KEY_ITEMS; j++)
              if (mask & (1u << j)) {
                  const unsigned long long o = base + s_ws[j * 4 + wave] + below[j];
                  keys_out[o] = keys[j];
                  if (vals_out) vals_out[o] = (uint32_t)(c * KEY_CHUNK + (uint64_t)j * 256 + threadIdx.x);  // read ordinal
              }
          __syncthreads();
      } else {
          emit_unordered(keys, mask, keys_out, vals_out, n_out, lds, c * KEY_CHUNK + threadIdx.x, 256u);
      }
    }
    if (HIST) key_hist_flush(s_hist, plan, ghist);
}

// ---- the same for the common case, four consecutive reads per lane --------------------------------------------------------
// k_build_keys is bound by the number of loads in flight, not by bytes (five loads of 1 to 12 bytes per read).  Here a lane
// takes four consecutive reads with 16-byte loads: barcode ranks, features and UMIs as one uint4 each, the four flag bytes
// as one dword, the four quality rows (4 * LQW dwords) as LQW uint4 -- 1.75 loads per read instead of 5.  Keys only (no
// ordinals, fixed UMI length, dword quality rows), n a multiple of 4, 16-byte aligned arrays; everything else takes
// k_build_keys.  The kept keys leave in thread-major order inside a chunk, as there: the sort does not care.
template <int LQW, bool HIST>
__global__ __launch_bounds__(256) void k_build_keys_v4(const KL kl, const uint32_t *__restrict__ bc_idx, const uint32_t *__restrict__ umi,
                                                       const uint8_t *__restrict__ umi_q, const uint32_t *__restrict__ feature,
                                                       const uint8_t *__restrict__ flags, uint64_t n, uint64_t *__restrict__ keys_out,
                                                       unsigned long long *__restrict__ n_out, const SweepPlan plan,
                                                       uint32_t *__restrict__ ghist, const uint4 *__restrict__ dense_fwd,
                                                       uint32_t *__restrict__ n_unknown) {
    static_assert(LQW >= 1 && LQW <= 4, "dword quality rows");
    __shared__ __attribute__((aligned(8))) uint32_t lds[10];
    __shared__ uint32_t s_hist[HIST ? OS_MAX_PASSES * RADIX_MAX : 1];
    if (HIST) key_hist_clear(s_hist, plan);
    constexpr int NV = KEY_ITEMS / 4;  // vectors of four reads per thread and chunk
    const uint64_t n_chunks = (n + KEY_CHUNK - 1) / KEY_CHUNK;
    const uint64_t n_vec = n / 4;  // n is a multiple of 4
    const uint4 *__restrict__ bc4 = reinterpret_cast<const uint4 *>(bc_idx);
    const uint4 *__restrict__ ft4 = reinterpret_cast<const uint4 *>(feature);
    const uint4 *__restrict__ um4 = reinterpret_cast<const uint4 *>(umi);
    const uint32_t *__restrict__ fl4 = reinterpret_cast<const uint32_t *>(flags);
    const uint4 *__restrict__ q4 = reinterpret_cast<const uint4 *>(umi_q);
    for (uint64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        uint64_t keys[KEY_ITEMS];
        uint32_t mask = 0;
#pragma unroll
        for (int v = 0; v < NV; v++) {
            const uint64_t iv = c * (KEY_CHUNK / 4) + (uint64_t)v * 256 + threadIdx.x;  // index of the vector
            const uint64_t ic = iv < n_vec ? iv : n_vec - 1;                             // loads from a clamped address
            uint4 vb, vf, vu, vq[LQW];
            uint32_t vfl;
            if (dense_fwd) {
                // the rank -> column table has to stay in L2 beside 33 bytes of touch-once input per read: those go past it
                vb = ld_stream4(bc4 + ic);
                vf = ld_stream4(ft4 + ic);
                vu = ld_stream4(um4 + ic);
                vfl = fl4 ? __builtin_nontemporal_load(fl4 + ic) : 0u;
#pragma unroll
                for (int k = 0; k < LQW; k++) vq[k] = ld_stream4(q4 + ic * LQW + k);
            } else {
                vb = bc4[ic];
                vf = ft4[ic];
                vu = um4[ic];
                vfl = fl4 ? fl4[ic] : 0u;
#pragma unroll
                for (int k = 0; k < LQW; k++) vq[k] = q4[ic * LQW + k];
            }
            uint32_t b4[4] = {vb.x, vb.y, vb.z, vb.w};
            if (dense_fwd) {  // rank -> column (four independent gathers from a table that stays in L2)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const uint32_t rk = b4[r];
                    const uint32_t col = dense_column(dense_fwd, rk != CRGPU_MISS ? rk : 0u);
                    if (rk != CRGPU_MISS && col == CRGPU_MISS && iv < n_vec) atomicAdd(n_unknown, 1u);
                    b4[r] = rk != CRGPU_MISS ? col : CRGPU_MISS;
                }
            }
            const uint32_t f4[4] = {vf.x, vf.y, vf.z, vf.w};
            const uint32_t u4[4] = {vu.x, vu.y, vu.z, vu.w};
            uint32_t qw[4 * LQW];
#pragma unroll
            for (int k = 0; k < LQW; k++) {
                qw[4 * k + 0] = vq[k].x;
                qw[4 * k + 1] = vq[k].y;
                qw[4 * k + 2] = vq[k].z;
                qw[4 * k + 3] = vq[k].w;
            }
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = v * 4 + r;
                bool has_n = false, low_q = false;
#pragma unroll
                for (int k = 0; k < LQW; k++) umi_quality_word(qw[r * LQW + k], has_n, low_q);
                const bool keep = key_of_read(kl, b4[r], f4[r], (vfl >> (8 * r)) & 0xFFu, u4[r], kl.umi_len, has_n, low_q, &keys[j]) &&
                                  iv < n_vec;
                if (keep) mask |= 1u << j;
                if (HIST && keep) key_hist_add(s_hist, plan, keys[j]);
            }
        }
        emit_unordered(keys, mask, keys_out, nullptr, n_out, lds, 0, 0u);
    }
    if (HIST) key_hist_flush(s_hist, plan, ghist);
}

// One launch of the key build: the kernels take the members of KeyArgs one by one, because only a pointer parameter can
// be __restrict__ (with the struct as the parameter the compiler split the loads of a read over branches of their own, and
// the ORDERED kernel lost 1 % -- profiles/key_build_refactor_before_after.jsonl, session b).  v4: four reads per lane
// (k_build_keys_v4; dword quality rows, no ordinals).  Histograms when a.ghist is given, read order when a.vals_out is.
template <int LQW>
static void launch_build_keys(crgpu_ctx *ctx, dim3 grid, const KeyArgs &a, bool v4) {
    const bool hist = a.ghist != nullptr, ordered = a.vals_out != nullptr;
    if constexpr (LQW != 0)
        if (v4) {
            auto kernel = hist ? k_build_keys_v4<LQW, true> : k_build_keys_v4<LQW, false>;
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, a.kl, a.bc_idx, a.umi, a.umi_q, a.feature, a.flags, a.n,
                               a.keys_out, a.n_out, a.plan, a.ghist, a.dense_fwd, a.n_unknown);
            return;
        }
    auto kernel = ordered ? (hist ? k_build_keys<LQW, true, true> : k_build_keys<LQW, false, true>)
                          : (hist ? k_build_keys<LQW, true, false> : k_build_keys<LQW, false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ctx->stream, a.kl, a.bc_idx, a.umi, a.umi_q, a.feature, a.flags, a.n, a.keys_out,
                       a.vals_out, a.n_out, a.plan, a.ghist, a.status, a.ticket, a.ulen, a.dense_fwd, a.n_unknown, a.lb_abort);
}
static void launch_build_keys(crgpu_ctx *ctx, uint32_t lqw, dim3 grid, const KeyArgs &a, bool v4) {
    switch (lqw) {
        case 1: launch_build_keys<1>(ctx, grid, a, v4); break;
        case 2: launch_build_keys<2>(ctx, grid, a, v4); break;
        case 3: launch_build_keys<3>(ctx, grid, a, v4); break;
        case 4: launch_build_keys<4>(ctx, grid, a, v4); break;
        default: launch_build_keys<0>(ctx, grid, a, v4); break;
    }
}

// keys only (no read ordinals): the sort's digit histograms are counted on the way, and 1024 workgroups keep their flush at a
// few million atomics
static const uint32_t KEY_GRID_HIST = 1024u;

int build_keys_impl(crgpu_ctx *ctx, const crgpu_records *recs, uint64_t *d_keys_out, uint32_t *d_vals_out,
                    uint64_t *n_keys_out) {
    if (!ctx || !recs || !n_keys_out) return CRGPU_EINVAL;
    CR_REQUIRE(ctx, ctx->layout.set, CRGPU_ESTATE, "crgpu_build_keys: call crgpu_set_key_layout first");
    CR_REQUIRE(ctx, recs->umi_len == ctx->layout.umi_len, CRGPU_EINVAL, "records umi_len %u != layout umi_len %u",
               recs->umi_len, ctx->layout.umi_len);
    *n_keys_out = 0;
    if (recs->n == 0) return CRGPU_OK;
    CR_REQUIRE(ctx, recs->n <= 0x7FFFFFFFull, CRGPU_ERANGE, "crgpu_build_keys: at most 2^31-1 records per call");
    CR_REQUIRE(ctx, recs->d_bc_idx && recs->d_umi && recs->d_umi_qualn && recs->d_feature && d_keys_out, CRGPU_EINVAL,
               "crgpu_build_keys: NULL buffer");
    CR_REQUIRE(ctx, !recs->d_umi_len || ctx->layout.bits_ulen || ctx->layout.umi_min_len == ctx->layout.umi_len, CRGPU_ESTATE,
               "crgpu_build_keys: per-read UMI lengths need crgpu_set_umi_min_len");
    CR_REQUIRE(ctx, (recs->umi_len & 3u) != 0u || (uintptr_t)recs->d_umi_qualn % 4 == 0, CRGPU_EINVAL,
               "crgpu_build_keys: the UMI quality buffer must be 4-byte aligned");
    CR_TRY(cr_dense_ensure(ctx));  // CRGPU_OPT_DENSE_BARCODE_KEYS: the BarcodeIndex of the tables as they stand (else nothing)
    // the histograms of the previous call stop being valid here and those of this call become valid at the very end: every
    // return in between leaves none
    KeyHistograms &gh = ctx->ghist;
    const bool had = gh.valid;
    const uint64_t n_before = gh.n;
    gh.valid = false;
    bool append = false;
    KeyArgs a;
    memset(&a, 0, sizeof(a));
    a.kl = make_kl(ctx->layout);
    a.bc_idx = recs->d_bc_idx;
    a.umi = recs->d_umi;
    a.umi_q = recs->d_umi_qualn;
    a.feature = recs->d_feature;
    a.flags = recs->d_flags;
    a.n = recs->n;
    a.keys_out = d_keys_out;
    a.vals_out = d_vals_out;
    a.n_out = (unsigned long long *)(ctx->d_scalars + CR_SCALAR_KEY_COUNT);
    a.ticket = ctx->d_scalars + CR_SCALAR_KEY_TICKET;
    a.ulen = recs->d_umi_len;
    a.dense_fwd = ctx->dense.valid ? ctx->dense.d_fwd : nullptr;
    a.n_unknown = ctx->d_scalars + CR_SCALAR_BAD_INDEX;
    a.lb_abort = ctx->d_scalars + CR_SCALAR_LOOKBACK_ABORT;
    {
        CrTimer t(ctx, CRGPU_T_KEYS, recs->n);
        CR_HIP(ctx, hipMemsetAsync(a.n_out, 0, sizeof(*a.n_out), ctx->stream));
        CR_HIP(ctx, hipMemsetAsync(a.n_unknown, 0, 2 * sizeof(uint32_t), ctx->stream));
        uint32_t widths[OS_MAX_PASSES];
        if (ctx->trust_buffers && !getenv("CRGPU_NO_KEY_HIST") && cr_sweep_plan(cr_sort_low_bits(ctx->layout.total_bits(), ctx->layout.bits_umi), ctx->layout.total_bits(), &a.plan, widths)) {
            if (!gh.d_hist) CR_TRY(cr_pool_alloc(ctx, (void **)&gh.d_hist, (size_t)OS_MAX_PASSES * RADIX_MAX * sizeof(uint32_t)));
            a.ghist = gh.d_hist;
            // a call that writes its keys right behind the previous call's (the libraries of a well, one after the other, into
            // one buffer) adds to that call's histograms: the sort of the whole buffer then still finds them
            append = had && !d_vals_out && gh.d_keys + gh.n == d_keys_out && memcmp(&gh.plan, &a.plan, sizeof(a.plan)) == 0;
            if (!append) CR_HIP(ctx, hipMemsetAsync(a.ghist, 0, (size_t)OS_MAX_PASSES * RADIX_MAX * sizeof(uint32_t), ctx->stream));
        }
        const dim3 grid(cr_grid(recs->n, 256, a.ghist ? KEY_GRID_HIST : 256u * 8u));
        // with ordinals: order-preserving compaction (tickets + look-back status, one word per 4096-read chunk)
        DevBuf status_b;
        if (d_vals_out) {
            const uint64_t n_chunks = (recs->n + KEY_CHUNK - 1) / KEY_CHUNK;
            CR_TRY(dmalloc(ctx, status_b, n_chunks * sizeof(unsigned long long)));
            a.status = status_b.as<unsigned long long>();
            CR_HIP(ctx, hipMemsetAsync(a.status, 0, n_chunks * sizeof(unsigned long long), ctx->stream));
            CR_HIP(ctx, hipMemsetAsync(a.ticket, 0, sizeof(uint32_t), ctx->stream));
        }
        // four reads per lane with 16-byte loads where the layout allows it (see k_build_keys_v4); the 1 - 3 reads behind the
        // last multiple of four go through the scalar kernel's byte path, appended by the same counter
        const bool aligned16 = ((uintptr_t)recs->d_bc_idx | (uintptr_t)recs->d_umi | (uintptr_t)recs->d_feature |
                                (uintptr_t)recs->d_umi_qualn) % 16 == 0 && (uintptr_t)recs->d_flags % 4 == 0;
        const uint32_t lqw = (recs->umi_len & 3u) == 0u && !recs->d_umi_len ? recs->umi_len / 4u : 0u;  // per-read lengths: the byte path
        if (!d_vals_out && lqw && aligned16 && recs->n >= 4096) {
            const uint64_t n4 = recs->n & ~3ull;
            KeyArgs head = a;
            head.n = n4;
            launch_build_keys(ctx, lqw, grid, head, true);
            if (n4 < recs->n) {
                KeyArgs tail = a;
                tail.bc_idx += n4;
                tail.umi += n4;
                tail.umi_q += n4 * recs->umi_len;
                tail.feature += n4;
                if (tail.flags) tail.flags += n4;
                tail.n = recs->n - n4;
                launch_build_keys(ctx, 0u, dim3(1), tail, false);
            }
        } else
            launch_build_keys(ctx, lqw, grid, a, false);
        CR_HIP(ctx, hipGetLastError());
    }
    unsigned long long h = 0;
    CR_TRY(crgpu_memcpy_d2h(ctx, &h, a.n_out, sizeof(h)));
    if (d_vals_out) {
        uint32_t stalled = 0;
        CR_TRY(crgpu_memcpy_d2h(ctx, &stalled, a.lb_abort, sizeof(stalled)));
        if (stalled)
            return cr_fail(ctx, CRGPU_EHIP, "crgpu_build_keys: the look-back of the order-preserving compaction stalled (watchdog); "
                                            "nothing was hung, the keys of this call are incomplete");
    }
    if (a.dense_fwd) {
        uint32_t unknown = 0;
        CR_TRY(crgpu_memcpy_d2h(ctx, &unknown, a.n_unknown, sizeof(unknown)));
        if (unknown)
            return cr_fail(ctx, CRGPU_ESTATE, "crgpu_build_keys: %u records carry a barcode that has no read in the VALID / CORRECTED tables "
                           "(CRGPU_OPT_DENSE_BARCODE_KEYS needs the tables of the whole well before the first key is built)", unknown);
    }
    *n_keys_out = h;
    gh.n = append ? n_before + h : h;
    if (a.ghist) {
        if (!append) gh.d_keys = d_keys_out;
        gh.plan = a.plan;
        gh.valid = true;
    }
    return CRGPU_OK;
}

extern "C" int crgpu_build_keys_dev(crgpu_ctx *ctx, const crgpu_records *recs, uint64_t *d_keys_out,
                                    uint64_t *n_keys_out) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    return build_keys_impl(ctx, recs, d_keys_out, nullptr, n_keys_out);
}

extern "C" int crgpu_partition_keys_dev(crgpu_ctx *ctx, const uint64_t *d_keys, uint64_t n, uint32_t n_ranks,
                                        const uint32_t *bounds, uint64_t *d_keys_out, uint64_t *counts_out) {
    if (!ctx || !counts_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, ctx->layout.set, CRGPU_ESTATE, "crgpu_partition_keys: call crgpu_set_key_layout first");
    CR_REQUIRE(ctx, n == 0 || (d_keys && d_keys_out), CRGPU_EINVAL, "crgpu_partition_keys: NULL buffer");
    cr_invalidate(ctx);
    CR_TRY(cr_dense_ensure(ctx));
    return cr_partition_by_owner(ctx, d_keys, d_keys_out, n, ctx->layout.sh_bc(), n_ranks, bounds, counts_out);
}

// Histogram-balanced owner ranges: bounds_out[0] = 0, bounds_out[n_ranks] = n_canon, and every range holds
// about the same number of reads according to the VALID + CORRECTED tables of all libraries (call it after the
// tables have been all-reduced so that every rank derives the same bounds).
extern "C" int crgpu_balanced_bounds(crgpu_ctx *ctx, uint32_t n_ranks, uint32_t *bounds_out) {
    if (!ctx || !bounds_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, ctx->canon_set, CRGPU_ESTATE, "crgpu_balanced_bounds: no whitelist set");
    CR_REQUIRE(ctx, n_ranks >= 1 && n_ranks <= 256, CRGPU_EINVAL, "crgpu_balanced_bounds: n_ranks must be 1..256");
    const uint32_t W = ctx->n_canon;
    std::vector<uint64_t> tot(W, 0);
    std::vector<uint32_t> tmp(W);
    for (int l = 0; l < CRGPU_MAX_LIB; l++) {
        if (!ctx->wl[l].set) continue;
        for (int which = 0; which < 2; which++) {
            CR_TRY(crgpu_memcpy_d2h(ctx, tmp.data(), which ? ctx->wl[l].d_corrected : ctx->wl[l].d_valid, sizeof(uint32_t) * W));
            for (uint32_t r = 0; r < W; r++) tot[r] += tmp[r];
        }
    }
    uint64_t total = 0;
    for (uint32_t r = 0; r < W; r++) total += tot[r];
    bounds_out[0] = 0;
    uint64_t acc = 0;
    uint32_t r = 0;
    for (uint32_t k = 1; k < n_ranks; k++) {
        const uint64_t want = total * k / n_ranks;
        while (r < W && acc + tot[r] <= want) acc += tot[r++];
        bounds_out[k] = r;
    }
    bounds_out[n_ranks] = W;
    return CRGPU_OK;
}
