// probe_counts.h -- probe x barcode counts of a Flex / RTL well (part of molecule_stages.hip: it works on crgpu_counts and takes the
// compaction, the pooled temporaries and the device-matrix helpers from stage_common.h).
//
// Replaces, per valid barcode of ALIGN_AND_COUNT (cr_lib/src/stages/align_and_count.rs:311-333):
//   BcUmiInfo::probe_counts            cr_types/src/types.rs:190-204   (histogram of UmiCount::probe_idx, None dropped)
//   ProbeBarcodeCount + its Ord        cr_types/src/types.rs:141-146   (the shard sort key: barcode, then probe_idx)
//   write_probe_matrix_h5_helper       cr_lib/src/probe_barcode_matrix.rs:176-262   (CSC over the sample's barcodes)
//   the two sums of collate_probe_metrics   cr_lib/src/gdna_utils.rs:217-237
//
// The molecule table is ordered by (barcode, feature, library, UMI): the molecules of a barcode are contiguous (a SEGMENT),
// but inside a segment the probe indices follow the features only loosely.  The work is a segmented sort + run-length count:
//   1. segment starts from d_mkeys (one compaction);
//   2. every segment is put in ascending probe order into d_sp (u32 per molecule, CRGPU_NO_PROBE last), by size class:
//        <= 8 / <= 64 molecules   a group of 8 / 64 lanes sorts in registers (shuffles), several segments per wave;
//        <= 4096 / <= 32768       one workgroup of 256 / 1024 threads sorts in LDS (16 / 128 KB);
//        larger                   keys (segment << probe bits | probe) go through the device radix sort and are put back;
//      a segment that already is ascending is copied, not sorted.  Bit 31 of d_sp marks the first molecule of every run of
//      equal probes inside a segment (a BOUNDARY; the first molecule of a segment always is one);
//   3. the boundaries are compacted to (position, probe), and the boundaries with a probe are compacted to the triplets:
//      umi_count = distance to the next boundary.
// Every molecule of a segment is written by exactly one lane to a fixed place, and both compactions are stable: the output
// does not depend on timing.  The only atomics on global memory hand out list slots and count segments per class.

#pragma once

#include "stage_common.h"

#define PC_G8_CAP 8u
#define PC_WAVE_CAP 64u
#define PC_MID_CAP 4096u
#define PC_BIG_CAP 32768u  // 128 KB of the CU's 160 KB of LDS
#define PC_MID_THREADS 256u
#define PC_BIG_THREADS 1024u
#define PC_NONE 0x7FFFFFFFu   // CRGPU_NO_PROBE inside d_sp: after every probe index (n_probes <= 2^31 - 1)
#define PC_BOUND 0x80000000u
#define PC_CHUNK 2048u        // molecules of a globally sorted segment one workgroup turns into keys at a time
// control words of one computation (a pool block of PC_CTL_WORDS u32, zeroed)
#define PC_CTL_BAD 0       // a probe index outside [-1, n_probes)
#define PC_CTL_N_WAVE 1    // segments per route ...
#define PC_CTL_N_MID 2
#define PC_CTL_N_BIG 3
#define PC_CTL_N_GLOB 4
#define PC_CTL_N_CHUNKS 5
#define PC_CTL_GLOB_MOL 6  // u64 (words 6, 7): molecules of the segments that take the global route
#define PC_CTL_WORDS 8

__device__ __forceinline__ uint32_t pc_code(int32_t p, uint32_t n_probes, bool *bad) {
    *bad = p < CRGPU_NO_PROBE || (p >= 0 && (uint32_t)p >= n_probes);
    return p < 0 ? PC_NONE : (uint32_t)p;
}

// One thread per segment: its route.  Segments of the two workgroup classes are appended to lists (their order is of no
// consequence: a segment's place in d_sp is fixed); a segment of the global route gets room for its keys (glob_off) and one
// work item per PC_CHUNK molecules.
__global__ __launch_bounds__(256) void k_pc_classify(const uint32_t *__restrict__ seg_start, uint32_t n_seg, uint32_t cap,
                                                     uint32_t *__restrict__ list_mid, uint32_t *__restrict__ list_big,
                                                     uint32_t *__restrict__ glob_off, uint32_t *__restrict__ chunk_seg,
                                                     uint32_t *__restrict__ chunk_first, uint32_t *__restrict__ ctl) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = s < n_seg;
    const uint32_t size = live ? seg_start[s + 1] - seg_start[s] : 0u;
    const bool lds = live && size <= cap;
    const bool wave = lds && size <= PC_WAVE_CAP, mid = lds && !wave && size <= PC_MID_CAP, big = lds && !wave && !mid;
    const bool glob = live && !lds;
    const unsigned long long mw = __ballot(wave), mg = __ballot(glob);
    if ((threadIdx.x & 63u) == 0) {
        if (mw) atomicAdd(&ctl[PC_CTL_N_WAVE], (uint32_t)__popcll(mw));
        if (mg) atomicAdd(&ctl[PC_CTL_N_GLOB], (uint32_t)__popcll(mg));
    }
    if (mid) list_mid[atomicAdd(&ctl[PC_CTL_N_MID], 1u)] = s;
    if (big) list_big[atomicAdd(&ctl[PC_CTL_N_BIG], 1u)] = s;
    if (glob) {
        glob_off[s] = (uint32_t)atomicAdd(reinterpret_cast<unsigned long long *>(ctl + PC_CTL_GLOB_MOL), (unsigned long long)size);
        const uint32_t nch = (size + PC_CHUNK - 1) / PC_CHUNK;
        const uint32_t c0 = atomicAdd(&ctl[PC_CTL_N_CHUNKS], nch);
        for (uint32_t c = 0; c < nch; c++) {
            chunk_seg[c0 + c] = s;
            chunk_first[c0 + c] = c * PC_CHUNK;
        }
    }
}

// Segments of (lo, hi] molecules, hi <= G: a group of G lanes holds one segment, a molecule per lane, and orders it with a
// bitonic network of shuffles.  Every lane of the wave walks the same number of rounds and executes every shuffle.
template <uint32_t G>
__global__ __launch_bounds__(256) void k_pc_seg_wave(const uint32_t *__restrict__ seg_start, uint32_t n_seg, uint32_t lo, uint32_t hi,
                                                     const int32_t *__restrict__ mprobe, uint32_t n_probes,
                                                     uint32_t *__restrict__ sp, uint32_t *__restrict__ ctl) {
    const uint32_t lane = threadIdx.x & 63u, gl = lane & (G - 1u);
    const uint64_t n_groups = ((uint64_t)gridDim.x * blockDim.x) / G;
    const uint64_t g0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
    const uint64_t rounds = ((uint64_t)n_seg + n_groups - 1) / n_groups;
    for (uint64_t r = 0; r < rounds; r++) {
        const uint64_t s = g0 + r * n_groups;
        uint32_t a = 0, size = 0;
        if (s < n_seg) {
            a = seg_start[s];
            size = seg_start[s + 1] - a;
        }
        const bool mine = size > lo && size <= hi;
        const bool have = mine && gl < size;
        uint32_t v = 0xFFFFFFFFu;  // padding: after PC_NONE
        if (have) {
            bool bad;
            v = pc_code(mprobe[a + gl], n_probes, &bad);
            if (bad) ctl[PC_CTL_BAD] = 1u;
        }
        const uint32_t below = __shfl_up(v, 1);
        if (__any(have && gl > 0 && below > v)) {  // some segment of this wave is out of order
#pragma unroll
            for (uint32_t k = 2; k <= G; k <<= 1) {
#pragma unroll
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    const uint32_t o = __shfl_xor(v, (int)j);
                    const bool up = (gl & k) == 0u, low = (gl & j) == 0u;
                    v = (up == low) ? (v < o ? v : o) : (v > o ? v : o);
                }
            }
        }
        const uint32_t prev = __shfl_up(v, 1);
        if (have) sp[a + gl] = v | ((gl == 0 || prev != v) ? PC_BOUND : 0u);
    }
}

// Segments of a list, at most `cap` molecules each (cap * 4 bytes of dynamic LDS): one workgroup per segment.  The network is
// the bitonic sorter whose compare-exchanges all point upwards (the first step of a stage mirrors inside the block), which
// sorts any n: a partner at or beyond n stands for +infinity and is never exchanged.
template <uint32_t THREADS>
__global__ __launch_bounds__(THREADS) void k_pc_seg_lds(const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ list,
                                                        const uint32_t *__restrict__ n_list, uint32_t cap,
                                                        const int32_t *__restrict__ mprobe, uint32_t n_probes,
                                                        uint32_t *__restrict__ sp, uint32_t *__restrict__ ctl) {
    extern __shared__ uint32_t pc_s[];
    __shared__ uint32_t s_unsorted;
    const uint32_t tid = threadIdx.x, nl = *n_list;
    for (uint32_t e = blockIdx.x; e < nl; e += gridDim.x) {
        const uint32_t seg = list[e], a = seg_start[seg], n = seg_start[seg + 1] - a;
        if (n > cap) continue;  // (uniform) never true for a list k_pc_classify wrote; the LDS window is cap entries
        if (tid == 0) s_unsorted = 0u;
        __syncthreads();
        bool uns = false;
        for (uint32_t j = tid; j < n; j += THREADS) {
            bool bad, bad_prev;
            const uint32_t v = pc_code(mprobe[a + j], n_probes, &bad);
            const uint32_t pv = pc_code(mprobe[a + (j ? j - 1 : 0)], n_probes, &bad_prev);
            if (bad) ctl[PC_CTL_BAD] = 1u;
            uns |= pv > v;
            pc_s[j] = v;
        }
        if (uns) s_unsorted = 1u;
        __syncthreads();
        if (s_unsorted) {  // uniform
            for (uint32_t k = 2; (k >> 1) < n; k <<= 1) {
                for (uint32_t i = tid; i < n; i += THREADS) {
                    const uint32_t l = i ^ (k - 1u);
                    if (l > i && l < n) {
                        const uint32_t x = pc_s[i], y = pc_s[l];
                        if (x > y) {
                            pc_s[i] = y;
                            pc_s[l] = x;
                        }
                    }
                }
                __syncthreads();
                for (uint32_t j = k >> 2; j > 0; j >>= 1) {
                    for (uint32_t i = tid; i < n; i += THREADS) {
                        const uint32_t l = i ^ j;
                        if (l > i && l < n) {
                            const uint32_t x = pc_s[i], y = pc_s[l];
                            if (x > y) {
                                pc_s[i] = y;
                                pc_s[l] = x;
                            }
                        }
                    }
                    __syncthreads();
                }
            }
        }
        for (uint32_t j = tid; j < n; j += THREADS) {
            const uint32_t v = pc_s[j];
            sp[a + j] = v | ((j == 0 || pc_s[j - 1] != v) ? PC_BOUND : 0u);
        }
        __syncthreads();
    }
}

// global route, before the sort: key = segment << pbits | probe code (CRGPU_NO_PROBE -> n_probes, the largest code)
__global__ __launch_bounds__(256) void k_pc_glob_keys(const uint32_t *__restrict__ seg_start, const uint32_t *__restrict__ glob_off,
                                                      const uint32_t *__restrict__ chunk_seg, const uint32_t *__restrict__ chunk_first,
                                                      const uint32_t *__restrict__ ctl_in, const int32_t *__restrict__ mprobe,
                                                      uint32_t n_probes, uint32_t pbits, uint64_t n_glob,
                                                      uint64_t *__restrict__ gkeys, uint32_t *__restrict__ ctl) {
    const uint32_t n_chunks = ctl_in[PC_CTL_N_CHUNKS];
    for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const uint32_t s = chunk_seg[c], first = chunk_first[c];
        const uint32_t a = seg_start[s], size = seg_start[s + 1] - a, off = glob_off[s];
        const uint32_t end = first + PC_CHUNK < size ? first + PC_CHUNK : size;
        for (uint32_t j = first + threadIdx.x; j < end; j += 256) {
            bool bad;
            const uint32_t v = pc_code(mprobe[a + j], n_probes, &bad);
            if (bad) ctl[PC_CTL_BAD] = 1u;
            if ((uint64_t)off + j < n_glob) gkeys[(uint64_t)off + j] = ((uint64_t)s << pbits) | (uint64_t)(v == PC_NONE ? n_probes : v);
        }
    }
}
// after the sort: the place of every segment's first key (the segments follow each other in ascending order) ...
__global__ __launch_bounds__(256) void k_pc_glob_first(const uint64_t *__restrict__ gkeys, uint64_t n_glob, uint32_t pbits,
                                                       uint32_t n_seg, uint32_t *__restrict__ glob_first) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_glob; q += stride) {
        const uint64_t s = gkeys[q] >> pbits, ps = gkeys[q ? q - 1 : 0] >> pbits;
        if ((q == 0 || s != ps) && s < n_seg) glob_first[s] = (uint32_t)q;
    }
}
// ... and every key back to its segment, in sorted order
__global__ __launch_bounds__(256) void k_pc_glob_put(const uint64_t *__restrict__ gkeys, uint64_t n_glob, uint32_t pbits,
                                                     uint32_t n_probes, const uint32_t *__restrict__ seg_start, uint32_t n_seg,
                                                     const uint32_t *__restrict__ glob_first, uint32_t *__restrict__ sp) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t pmask = (1ull << pbits) - 1ull;
    for (uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; q < n_glob; q += stride) {
        const uint64_t k = gkeys[q], pk = gkeys[q ? q - 1 : 0];
        const uint64_t s = k >> pbits;
        if (s >= n_seg) continue;
        const uint32_t p = (uint32_t)(k & pmask);
        const uint32_t a = seg_start[s], size = seg_start[s + 1] - a;
        const uint64_t j = q - glob_first[s];
        if (j < size) sp[a + j] = (p >= n_probes ? PC_NONE : p) | ((q == 0 || k != pk) ? PC_BOUND : 0u);
    }
}

struct BoundFlag {
    const uint32_t *sp;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return (sp[i] & PC_BOUND) != 0u; }
};
struct EmitBound {
    const uint32_t *sp;
    uint32_t *bpos, *bval;
    typedef uint32_t Pre;
    __device__ __forceinline__ Pre pre(uint64_t i) const { return sp[i]; }
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t o, Pre v) const {
        bpos[o] = (uint32_t)i;
        bval[o] = v & ~PC_BOUND;
    }
};
struct ProbedFlag {
    const uint32_t *bval;
    __device__ __forceinline__ bool operator()(uint64_t k) const { return bval[k] != PC_NONE; }
};
struct EmitProbeTriplet {  // ProbeBarcodeCount {barcode, probe_idx, umi_count} (types.rs:141-146)
    const uint32_t *bpos, *bval;
    const uint64_t *mkeys;
    const uint32_t *back;  // dense barcode keys: column -> whitelist rank
    uint32_t sh_bc;
    uint64_t n_bound, n_mol;
    uint32_t *bc, *probe, *count;
    struct Pre {
        uint32_t pos, next, val;
    };
    __device__ __forceinline__ Pre pre(uint64_t k) const {
        Pre p;
        p.pos = bpos[k];
        p.next = k + 1 < n_bound ? bpos[k + 1] : (uint32_t)n_mol;
        p.val = bval[k];
        return p;
    }
    __device__ __forceinline__ void operator()(uint64_t, uint32_t o, Pre p) const {
        const uint32_t b = (uint32_t)(mkeys[p.pos] >> sh_bc);
        bc[o] = back ? back[b] : b;
        probe[o] = p.val;
        count[o] = p.next - p.pos;
    }
};

static void probe_triplets_drop(crgpu_ctx *ctx, crgpu_counts *c) {
    cr_pool_free(ctx, c->d_pt_bc);
    cr_pool_free(ctx, c->d_pt_probe);
    cr_pool_free(ctx, c->d_pt_count);
    c->d_pt_bc = c->d_pt_probe = c->d_pt_count = nullptr;
    c->n_pt = 0;
    c->pt_valid = false;
}

// the triplets of `c` for n_probes, computed on the first request and kept in the counts
static int probe_triplets_ensure(crgpu_ctx *ctx, crgpu_counts *c, uint32_t n_probes, const char *who) {
    if (c->pt_valid && c->pt_n_probes == n_probes) return CRGPU_OK;
    const uint64_t nm = c->n_molecules;
    CR_REQUIRE(ctx, nm == 0 || c->d_mprobe, CRGPU_ESTATE,
               "%s: these counts were made without crgpu_records.d_probe_idx (crgpu_count_records_dev / crgpu_count_host)", who);
    CR_REQUIRE(ctx, n_probes < PC_NONE, CRGPU_ERANGE, "%s: n_probes must be below 2^31 - 1", who);
    CR_REQUIRE(ctx, nm < 0xFFFFFFFFull, CRGPU_ERANGE, "%s: too many molecules", who);
    probe_triplets_drop(ctx, c);
    c->pt_n_probes = n_probes;
    if (nm == 0) {
        c->pt_valid = true;
        return CRGPU_OK;
    }
    const KeyLayout &L = c->layout;
    uint32_t *d_block = ctx->d_sort_hist, *d_total = ctx->d_scalars + CR_SCALAR_TOTAL;
    DevBuf seg_b, ctl_b, sp_b;
    CR_TRY(dmalloc(ctx, ctl_b, PC_CTL_WORDS * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, sp_b, nm * sizeof(uint32_t)));
    uint32_t *ctl = ctl_b.as<uint32_t>(), *sp = sp_b.as<uint32_t>();
    uint32_t n_seg = 0;
    CR_HIP(ctx, hipMemsetAsync(ctl, 0, PC_CTL_WORDS * sizeof(uint32_t), ctx->stream));
    CR_TRY(cr_barcode_segments(ctx, c, who, seg_b, &n_seg));
    uint32_t *seg_start = seg_b.as<uint32_t>();
    const uint32_t cap = ctx->probe_seg_cap < PC_BIG_CAP ? ctx->probe_seg_cap : PC_BIG_CAP;
    // lists: workgroup classes (a segment there has more than PC_WAVE_CAP molecules), global route (chunks of PC_CHUNK)
    const uint64_t list_max = nm / PC_WAVE_CAP + 1, chunk_max = nm / PC_CHUNK + n_seg;
    DevBuf mid_b, big_b, goff_b, cseg_b, cfirst_b;
    CR_TRY(dmalloc(ctx, mid_b, list_max * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, big_b, list_max * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, goff_b, (uint64_t)n_seg * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, cseg_b, chunk_max * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, cfirst_b, chunk_max * sizeof(uint32_t)));
    uint32_t h_ctl[PC_CTL_WORDS];
    {
        CrTimer t(ctx, CRGPU_T_DEDUP);
        hipLaunchKernelGGL(k_pc_classify, dim3((n_seg + 255u) / 256u), dim3(256), 0, ctx->stream, seg_start, n_seg, cap,
                           mid_b.as<uint32_t>(), big_b.as<uint32_t>(), goff_b.as<uint32_t>(), cseg_b.as<uint32_t>(),
                           cfirst_b.as<uint32_t>(), ctl);
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(crgpu_memcpy_d2h(ctx, h_ctl, ctl, sizeof(h_ctl)));
    uint64_t n_glob = 0;
    memcpy(&n_glob, h_ctl + PC_CTL_GLOB_MOL, sizeof(n_glob));
    CR_REQUIRE(ctx, n_glob <= nm && h_ctl[PC_CTL_N_MID] <= list_max && h_ctl[PC_CTL_N_BIG] <= list_max &&
                        h_ctl[PC_CTL_N_CHUNKS] <= chunk_max, CRGPU_EHIP, "%s: inconsistent segment classes", who);
    ctx->probe_segments[0] = h_ctl[PC_CTL_N_WAVE];
    ctx->probe_segments[1] = (uint64_t)h_ctl[PC_CTL_N_MID] + h_ctl[PC_CTL_N_BIG];
    ctx->probe_segments[2] = h_ctl[PC_CTL_N_GLOB];
    {
        CrTimer t(ctx, CRGPU_T_DEDUP, nm - n_glob);
        if (h_ctl[PC_CTL_N_WAVE]) {
            const uint32_t hi8 = cap < PC_G8_CAP ? cap : PC_G8_CAP, hi64 = cap < PC_WAVE_CAP ? cap : PC_WAVE_CAP;
            hipLaunchKernelGGL(k_pc_seg_wave<8>, dim3(cr_grid((uint64_t)n_seg * 8, 256, 8192)), dim3(256), 0, ctx->stream, seg_start,
                               n_seg, 0u, hi8, c->d_mprobe, n_probes, sp, ctl);
            if (hi64 > hi8)
                hipLaunchKernelGGL(k_pc_seg_wave<64>, dim3(cr_grid((uint64_t)n_seg * 64, 256, 8192)), dim3(256), 0, ctx->stream,
                                   seg_start, n_seg, hi8, hi64, c->d_mprobe, n_probes, sp, ctl);
        }
        if (h_ctl[PC_CTL_N_MID]) {
            const uint32_t wcap = cap < PC_MID_CAP ? cap : PC_MID_CAP;
            hipLaunchKernelGGL(k_pc_seg_lds<PC_MID_THREADS>, dim3(cr_grid((uint64_t)h_ctl[PC_CTL_N_MID] * PC_MID_THREADS, PC_MID_THREADS, 4096)),
                               dim3(PC_MID_THREADS), (size_t)wcap * sizeof(uint32_t), ctx->stream, seg_start, mid_b.as<uint32_t>(),
                               ctl + PC_CTL_N_MID, wcap, c->d_mprobe, n_probes, sp, ctl);
        }
        if (h_ctl[PC_CTL_N_BIG]) {
            const size_t lds = (size_t)cap * sizeof(uint32_t);
            cr_allow_lds(ctx, (const void *)k_pc_seg_lds<PC_BIG_THREADS>, lds);
            hipLaunchKernelGGL(k_pc_seg_lds<PC_BIG_THREADS>, dim3(cr_grid((uint64_t)h_ctl[PC_CTL_N_BIG] * PC_BIG_THREADS, PC_BIG_THREADS, 1024)),
                               dim3(PC_BIG_THREADS), lds, ctx->stream, seg_start, big_b.as<uint32_t>(), ctl + PC_CTL_N_BIG, cap,
                               c->d_mprobe, n_probes, sp, ctl);
        }
        CR_HIP(ctx, hipGetLastError());
    }
    if (n_glob) {
        // keys (segment, probe code): the existing device sort (sort.hip), then back to the segments' places
        const uint32_t pbits = cr_ceil_log2((uint64_t)n_probes + 1), sbits = cr_ceil_log2(n_seg);
        DevBuf gk_b, gt_b;
        CR_TRY(dmalloc(ctx, gk_b, n_glob * sizeof(uint64_t)));
        CR_TRY(dmalloc(ctx, gt_b, n_glob * sizeof(uint64_t)));
        {
            CrTimer t(ctx, CRGPU_T_DEDUP, n_glob);
            hipLaunchKernelGGL(k_pc_glob_keys, dim3(cr_grid((uint64_t)h_ctl[PC_CTL_N_CHUNKS] * 256, 256, 4096)), dim3(256), 0, ctx->stream,
                               seg_start, goff_b.as<uint32_t>(), cseg_b.as<uint32_t>(), cfirst_b.as<uint32_t>(), ctl, c->d_mprobe, n_probes,
                               pbits, n_glob, gk_b.as<uint64_t>(), ctl);
            CR_HIP(ctx, hipGetLastError());
        }
        bool in_tmp = false;
        CR_TRY(cr_radix_sort_u64_full(ctx, gk_b.as<uint64_t>(), gt_b.as<uint64_t>(), nullptr, nullptr, n_glob, pbits + (sbits ? sbits : 1u),
                                      &in_tmp));
        const uint64_t *sorted = in_tmp ? gt_b.as<uint64_t>() : gk_b.as<uint64_t>();
        {
            CrTimer t(ctx, CRGPU_T_DEDUP, n_glob);
            hipLaunchKernelGGL(k_pc_glob_first, dim3(cr_grid(n_glob, 256)), dim3(256), 0, ctx->stream, sorted, n_glob, pbits, n_seg,
                               goff_b.as<uint32_t>());
            hipLaunchKernelGGL(k_pc_glob_put, dim3(cr_grid(n_glob, 256)), dim3(256), 0, ctx->stream, sorted, n_glob, pbits, n_probes,
                               seg_start, n_seg, goff_b.as<uint32_t>(), sp);
            CR_HIP(ctx, hipGetLastError());
        }
    }
    // boundaries -> (position, probe); the ones with a probe -> triplets
    DevBuf bpos_b, bval_b;
    CR_TRY(dmalloc(ctx, bpos_b, nm * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, bval_b, nm * sizeof(uint32_t)));
    uint32_t n_bound = 0, n_pt = 0, bad = 0;
    {
        CrTimer t(ctx, CRGPU_T_DEDUP, nm);
        CR_TRY(compact(ctx, BoundFlag{sp}, EmitBound{sp, bpos_b.as<uint32_t>(), bval_b.as<uint32_t>()}, nm, d_block, d_total));
    }
    CR_TRY(read_u32(ctx, d_total, &n_bound));
    CR_TRY(read_u32(ctx, ctl + PC_CTL_BAD, &bad));
    CR_REQUIRE(ctx, !bad, CRGPU_ERANGE, "%s: a molecule carries a probe index outside [-1, %u)", who, n_probes);
    CR_REQUIRE(ctx, n_bound >= n_seg && n_bound <= nm, CRGPU_EHIP, "%s: %u run boundaries in %u segments", who, n_bound, n_seg);
    CR_TRY(cr_pool_alloc(ctx, (void **)&c->d_pt_bc, (uint64_t)n_bound * sizeof(uint32_t)));
    int rc = cr_pool_alloc(ctx, (void **)&c->d_pt_probe, (uint64_t)n_bound * sizeof(uint32_t));
    if (rc == CRGPU_OK) rc = cr_pool_alloc(ctx, (void **)&c->d_pt_count, (uint64_t)n_bound * sizeof(uint32_t));
    if (rc == CRGPU_OK) {
        CrTimer t(ctx, CRGPU_T_DEDUP, n_bound);
        rc = compact(ctx, ProbedFlag{bval_b.as<uint32_t>()},
                     EmitProbeTriplet{bpos_b.as<uint32_t>(), bval_b.as<uint32_t>(), c->d_mkeys, c->d_back, L.sh_bc(), n_bound, nm, c->d_pt_bc,
                                      c->d_pt_probe, c->d_pt_count},
                     n_bound, d_block, d_total);
    }
    if (rc == CRGPU_OK) rc = read_u32(ctx, d_total, &n_pt);
    if (rc != CRGPU_OK) {
        probe_triplets_drop(ctx, c);
        return rc;
    }
    c->n_pt = n_pt;
    c->pt_valid = true;
    return CRGPU_OK;
}

extern "C" int crgpu_counts_probe_triplets_dev(crgpu_ctx *ctx, crgpu_counts *c, uint32_t n_probes, uint32_t **d_bc, uint32_t **d_probe,
                                               uint32_t **d_count, uint64_t *n_out) {
    if (!ctx || !c) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_TRY(probe_triplets_ensure(ctx, c, n_probes, "crgpu_counts_probe_triplets_dev"));
    if (d_bc) *d_bc = c->d_pt_bc;
    if (d_probe) *d_probe = c->d_pt_probe;
    if (d_count) *d_count = c->d_pt_count;
    if (n_out) *n_out = c->n_pt;
    return CRGPU_OK;
}

extern "C" int crgpu_counts_probe_triplets(crgpu_ctx *ctx, crgpu_counts *c, uint32_t n_probes, uint32_t *bc_out, uint32_t *probe_out,
                                           uint32_t *count_out, uint64_t *n_out) {
    if (!ctx || !c) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_TRY(probe_triplets_ensure(ctx, c, n_probes, "crgpu_counts_probe_triplets"));
    const uint64_t b = c->n_pt * sizeof(uint32_t);
    if (bc_out) CR_TRY(crgpu_memcpy_d2h(ctx, bc_out, c->d_pt_bc, b));
    if (probe_out) CR_TRY(crgpu_memcpy_d2h(ctx, probe_out, c->d_pt_probe, b));
    if (count_out) CR_TRY(crgpu_memcpy_d2h(ctx, count_out, c->d_pt_count, b));
    if (n_out) *n_out = c->n_pt;
    return CRGPU_OK;
}

// ---- probe x barcode matrix (write_probe_matrix_h5_helper, probe_barcode_matrix.rs:176-262) ------------------------------
// per column: the range of triplets of its barcode (empty when the barcode has none)
__global__ __launch_bounds__(256) void k_pc_column_ranges(const uint32_t *__restrict__ col_rank, uint64_t n_cols,
                                                          const uint32_t *__restrict__ t_bc, uint64_t nt, uint32_t *__restrict__ first,
                                                          uint32_t *__restrict__ len) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_cols; c += stride) {
        const uint32_t r = col_rank[c];
        const uint64_t lo = cr_lower_bound(t_bc, nt, r);
        first[c] = (uint32_t)lo;
        len[c] = (uint32_t)cr_upper_bound(t_bc + lo, nt - lo, r);
    }
}
// one wave per column: a contiguous copy of its triplets (off = the scanned lengths)
__global__ __launch_bounds__(256) void k_pc_fill_columns(uint64_t n_cols, const uint32_t *__restrict__ first, const uint32_t *__restrict__ off,
                                                         uint32_t total, const uint32_t *__restrict__ t_probe,
                                                         const uint32_t *__restrict__ t_cnt, int32_t *__restrict__ io,
                                                         int32_t *__restrict__ dout) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave0; c < n_cols; c += n_waves) {
        const uint32_t o = off[c], n = (c + 1 < n_cols ? off[c + 1] : total) - o, s = first[c];
        for (uint32_t i = lane; i < n; i += 64) {
            io[o + i] = (int32_t)t_probe[s + i];
            dout[o + i] = (int32_t)t_cnt[s + i];
        }
    }
}

extern "C" int crgpu_assemble_probe_matrix_dev(crgpu_ctx *ctx, crgpu_counts *c, uint32_t n_probes, const uint32_t *d_sample_ranks,
                                               uint64_t n_sample, crgpu_matrix_dev **out) {
    if (!ctx || !c || !out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *out = nullptr;
    CR_REQUIRE(ctx, ctx->canon_set, CRGPU_ESTATE, "crgpu_assemble_probe_matrix_dev: no whitelist set");
    CR_REQUIRE(ctx, d_sample_ranks || n_sample == 0, CRGPU_EINVAL, "crgpu_assemble_probe_matrix_dev: NULL sample ranks");
    CR_REQUIRE(ctx, n_sample < 0xFFFFFFFFull, CRGPU_ERANGE, "crgpu_assemble_probe_matrix_dev: too many barcodes");
    CR_TRY(probe_triplets_ensure(ctx, c, n_probes, "crgpu_assemble_probe_matrix_dev"));
    uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL, *d_flag = ctx->d_scalars + CR_SCALAR_FLAG;
    // the columns: the sample's barcodes (BarcodeIndex::from_iter(sample_bcs), :190-196), or the context's BarcodeIndex
    DevBuf rank_b, first_b, len_b;
    uint64_t V = n_sample;
    if (d_sample_ranks) {
        uint32_t flag = 0;
        CR_TRY(dmalloc(ctx, rank_b, (V ? V : 1) * sizeof(uint32_t)));
        {
            CrTimer t(ctx, CRGPU_T_MATRIX, V);
            CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
            if (V) CR_HIP(ctx, hipMemcpyAsync(rank_b.p, d_sample_ranks, V * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
            cr_check_ranks(ctx, rank_b.as<uint32_t>(), V, d_flag);
            CR_HIP(ctx, hipGetLastError());
        }
        CR_TRY(read_u32(ctx, d_flag, &flag));
        CR_TRY(cr_list_verdict(ctx, flag, "crgpu_assemble_probe_matrix_dev", "sample barcode rank"));
    } else {
        SeenFlag seen;
        seen.ct.n = 0;
        for (int l = 0; l < CRGPU_MAX_LIB; l++)
            if (ctx->wl[l].set) {
                seen.ct.t[seen.ct.n++] = ctx->wl[l].d_valid;
                seen.ct.t[seen.ct.n++] = ctx->wl[l].d_corrected;
            }
        const uint32_t W = ctx->n_canon;
        uint32_t v32 = 0;
        CR_TRY(dmalloc(ctx, rank_b, (uint64_t)(W ? W : 1) * sizeof(uint32_t)));
        {
            CrTimer t(ctx, CRGPU_T_MATRIX, W);
            CR_TRY(compact(ctx, seen, EmitCol{rank_b.as<uint32_t>()}, W, ctx->d_sort_hist, d_total));
        }
        CR_TRY(read_u32(ctx, d_total, &v32));
        V = v32;
    }
    CR_TRY(dmalloc(ctx, first_b, (V ? V : 1) * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, len_b, (V + 1) * sizeof(uint32_t)));
    uint32_t total = 0;
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, V);
        if (V)
            hipLaunchKernelGGL(k_pc_column_ranges, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, rank_b.as<uint32_t>(), V, c->d_pt_bc, c->n_pt,
                               first_b.as<uint32_t>(), len_b.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
        CR_TRY(cr_scan_small(ctx, len_b.as<uint32_t>(), V, d_total));
    }
    CR_TRY(read_u32(ctx, d_total, &total));
    MatrixDevImpl *m = nullptr;
    CR_TRY(cr_new_matrix_dev(ctx, V, total, &m));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, total);
        if (V) {
            CR_HIP(ctx, hipMemcpyAsync(m->d_rank, rank_b.p, V * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
            if (total)
                hipLaunchKernelGGL(k_pc_fill_columns, dim3(cr_grid(V * 64, 256)), dim3(256), 0, ctx->stream, V, first_b.as<uint32_t>(),
                                   len_b.as<uint32_t>(), total, c->d_pt_probe, c->d_pt_count, m->d_indices, m->d_data);
        }
        cr_offsets_to_indptr(ctx, len_b.as<uint32_t>(), V, total, m->d_indptr);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            crgpu_matrix_dev_free(ctx, &m->view);
            return cr_fail(ctx, CRGPU_EHIP, "crgpu_assemble_probe_matrix_dev: kernel failed");
        }
    }
    *out = &m->view;
    return CRGPU_OK;
}

// ---- per-probe UMI sums (collate_probe_metrics, gdna_utils.rs:217-237) ------------------------------------------------------
// one pass over the triplets; integer atomics, so the sums do not depend on the order
__global__ __launch_bounds__(256) void k_pc_probe_sums(const uint32_t *__restrict__ t_bc, const uint32_t *__restrict__ t_probe,
                                                       const uint32_t *__restrict__ t_cnt, uint64_t nt, uint32_t n_probes,
                                                       const uint32_t *__restrict__ cells, uint64_t n_cells,
                                                       unsigned long long *__restrict__ all, unsigned long long *__restrict__ filtered) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nt; i += stride) {
        const uint32_t p = t_probe[i], r = t_bc[i];
        if (p >= n_probes) continue;
        const unsigned long long n = t_cnt[i];
        atomicAdd(&all[p], n);
        const uint64_t lo = cr_lower_bound(cells, n_cells, r);
        if (lo < n_cells && cells[lo] == r) atomicAdd(&filtered[p], n);
    }
}

extern "C" int crgpu_probe_metrics_dev(crgpu_ctx *ctx, crgpu_counts *c, uint32_t n_probes, const uint32_t *d_cell_ranks, uint64_t n_cells,
                                       uint64_t *umis_in_all_barcodes_out, uint64_t *umis_in_filtered_barcodes_out) {
    if (!ctx || !c) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, d_cell_ranks || n_cells == 0, CRGPU_EINVAL, "crgpu_probe_metrics_dev: NULL cell ranks");
    CR_TRY(probe_triplets_ensure(ctx, c, n_probes, "crgpu_probe_metrics_dev"));
    if (!n_probes) return CRGPU_OK;
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    DevBuf sums_b;
    const uint64_t bytes = (uint64_t)n_probes * sizeof(unsigned long long);
    CR_TRY(dmalloc(ctx, sums_b, 2 * bytes));
    unsigned long long *all = sums_b.as<unsigned long long>(), *filtered = all + n_probes;
    {
        CrTimer t(ctx, CRGPU_T_DEDUP, c->n_pt);
        CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
        CR_HIP(ctx, hipMemsetAsync(sums_b.p, 0, 2 * bytes, ctx->stream));
        cr_check_ranks(ctx, d_cell_ranks, n_cells, d_flag);
        if (c->n_pt)
            hipLaunchKernelGGL(k_pc_probe_sums, dim3(cr_grid(c->n_pt, 256)), dim3(256), 0, ctx->stream, c->d_pt_bc, c->d_pt_probe, c->d_pt_count,
                               c->n_pt, n_probes, d_cell_ranks, n_cells, all, filtered);
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_TRY(cr_list_verdict(ctx, flag, "crgpu_probe_metrics_dev", "cell barcode rank"));
    if (umis_in_all_barcodes_out) CR_TRY(crgpu_memcpy_d2h(ctx, umis_in_all_barcodes_out, all, bytes));
    if (umis_in_filtered_barcodes_out) CR_TRY(crgpu_memcpy_d2h(ctx, umis_in_filtered_barcodes_out, filtered, bytes));
    return CRGPU_OK;
}
