// subsample.h -- read subsampling of the molecule table: the tallies behind the saturation curves (part of
// molecule_stages.hip: works on crgpu_counts; the barcode segments and the ascending check are those of stage_common.h).
//
// Replaces run_subsampling / _run_subsample_task (lib/python/cellranger/subsample.py:430-654) for one chunk that holds the whole
// table, compute_target_depths / make_subsamplings / _subsampling_for_depth (:140-309, crgpu_subsample_plan) and the per-task
// numbers of calculate_subsampling_metrics (:719-845, crgpu_subsample_summary).  The reference's np.random.binomial on the serial
// MT19937 stream is replaced: read j of molecule m owns word j of the Philox stream m (philox.h), u = word >> 11, and task t keeps
// the read iff u < T[t][library], T = floor(rate * 2^53).  The words do not depend on the task, so one pass over them serves
// every task of a batch.
//
//   1. prep     one pass over the table: libraries present, any_reads, and the molecules of many reads put on two lists (one
//               buffer of n_molecules words, the wave list from the front, the workgroup list from the back);
//   2. groups   barcode group starts by compaction (cr_barcode_segments); per group the cell index (a search in
//               d_cell_ranks) and the genomes it is a cell of;
//   3. draw     per batch of at most 64 tasks: kept[task][molecule] (u32).  Thresholds of (library, task) sit in LDS; a lane
//               counts per task in 8-bit fields of eight 64-bit registers, at most 63 Philox blocks (252 words) before they are
//               emptied.  k_ss_draw_lane: a molecule per lane (count < wave_min); k_ss_draw_wave: a molecule per wave, lanes
//               stride over the blocks, butterfly sum; k_ss_draw_wg: a molecule per workgroup in rounds of 256 x 63 blocks,
//               summed per wave and then in LDS.  Every kept count has one writer and one place;
//   4. tally    one wave per (barcode group, task) walks the group in tiles of 64 molecules: sums of kept and of kept > 0 per
//               genome, and the (barcode, feature) runs that have a survivor -- the run heads and the survivors of a tile are two
//               ballots, a run that crosses a tile edge carries one bit.  Per-cell entries have one writer; the totals and the
//               per-feature survivor counts are 64-bit integer atomics (exact in any order).
// Nothing depends on timing, on the two thresholds or on the batch.
#pragma once

#include <algorithm>
#include <cmath>

#include "philox.h"
#include "stage_common.h"

#define SS_THREADS 256u
#define SS_MAX_BATCH 64u
#define SS_WAVE_MIN_MAX 256u   // lane path: kept <= count < 256 fits the 8-bit fields
#define SS_WG_MIN_MAX 16128u   // wave path: at most 63 blocks of 4 words per lane
#define SS_LANE_BLOCKS 63u
#define SS_CTL_N_WAVE 0
#define SS_CTL_N_WG 1
#define SS_CTL_N_USED 2        // u64 (words 2, 3)
#define SS_CTL_BAD 4
#define SS_CTL_WORDS 8

struct SsKeys {
    const uint64_t *mkeys;
    const uint32_t *mreads;
    const uint32_t *mpos;   // device position -> position in the table crgpu_counts_molecules lists, NULL: the same
    const uint8_t *fmask;   // per feature, NULL: all
    uint64_t nm;
    uint32_t sh_feat, bits_feat, sh_libid, bits_lib, n_features, n_libs;
};
__device__ __forceinline__ uint32_t ss_feature(const SsKeys &K, uint64_t key) { return (uint32_t)((key >> K.sh_feat) & lowmask(K.bits_feat)); }
__device__ __forceinline__ uint32_t ss_library(const SsKeys &K, uint64_t key) { return (uint32_t)((key >> K.sh_libid) & lowmask(K.bits_lib)); }
// reads of molecule i that take part (0 outside the feature mask), its library
__device__ __forceinline__ uint32_t ss_count(const SsKeys &K, uint64_t i, uint32_t *lib) {
    const uint64_t key = K.mkeys[i];
    const uint32_t f = ss_feature(K, key), l = ss_library(K, key);
    *lib = l < K.n_libs ? l : 0u;
    if (f >= K.n_features || l >= K.n_libs || (K.fmask && !K.fmask[f])) return 0u;
    return K.mreads[i];
}

__global__ __launch_bounds__(256) void k_ss_prep(SsKeys K, const uint8_t *__restrict__ fgen, uint32_t n_genomes, uint32_t wave_min,
                                                 uint32_t wg_min, uint8_t *__restrict__ lib_present, uint8_t *__restrict__ any_reads,
                                                 uint32_t *__restrict__ list, uint32_t *__restrict__ ctl) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < K.nm; i += stride) {
        const uint64_t key = K.mkeys[i];
        const uint32_t f = ss_feature(K, key), lib = ss_library(K, key);
        if (f >= K.n_features || lib >= K.n_libs) {
            ctl[SS_CTL_BAD] = 1u;
            continue;
        }
        if (K.fmask && !K.fmask[f]) continue;
        const uint32_t count = K.mreads[i];
        lib_present[lib] = 1;
        if (count) any_reads[lib * n_genomes + (fgen ? fgen[f] : 0u)] = 1;  // (fgen[f] < n_genomes: checked by the host)
        atomicAdd(reinterpret_cast<unsigned long long *>(ctl + SS_CTL_N_USED), 1ull);
        if (count >= wg_min)
            list[K.nm - 1u - atomicAdd(&ctl[SS_CTL_N_WG], 1u)] = (uint32_t)i;
        else if (count >= wave_min)
            list[atomicAdd(&ctl[SS_CTL_N_WAVE], 1u)] = (uint32_t)i;
    }
}

// ---- the draw -------------------------------------------------------------------------------------------------------------------
struct SsAcc {  // byte (t & 7) of a[t >> 3] = kept words of task t
    unsigned long long a[8];
};
__device__ __forceinline__ void ss_clear(SsAcc &acc) {
#pragma unroll
    for (int g = 0; g < 8; g++) acc.a[g] = 0ull;
}
// Philox block b of stream m: its words that are reads (4 b + k < count) against the thresholds thr[0 .. 8 ng) (LDS; entries
// beyond the batch are 0, which keeps nothing)
__device__ __forceinline__ void ss_block(SsAcc &acc, unsigned long long b, unsigned long long m, unsigned long long seed, uint32_t count,
                                         const unsigned long long *thr, uint32_t ng) {
    unsigned long long w[4];
    cr_philox4x64_10(b + 1ull, m, seed, w);
    const unsigned long long left = (unsigned long long)count - 4ull * b;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned long long u = (unsigned long long)k < left ? (w[k] >> 11) : ~0ull;  // no threshold exceeds 2^53
#pragma unroll
        for (int g = 0; g < 8; g++)
            if ((uint32_t)g < ng) {
                unsigned long long add = 0ull;
#pragma unroll
                for (int j = 0; j < 8; j++) add |= (unsigned long long)(u < thr[8 * g + j]) << (8 * j);
                acc.a[g] += add;
            }
    }
}
// the fields summed over the wave as 16-bit fields (64 lanes x 252 < 2^16): lo = tasks 8 g + 0, 2, 4, 6, hi = the odd ones
__device__ __forceinline__ void ss_wave_sum(const SsAcc &acc, uint32_t ng, unsigned long long lo[8], unsigned long long hi[8]) {
#pragma unroll
    for (int g = 0; g < 8; g++) {
        lo[g] = hi[g] = 0ull;
        if ((uint32_t)g < ng) {
            lo[g] = wave_sum(acc.a[g] & 0x00FF00FF00FF00FFull);
            hi[g] = wave_sum((acc.a[g] >> 8) & 0x00FF00FF00FF00FFull);
        }
    }
}
#define SS_FIELD16(lo, hi, t) ((uint32_t)((((t) & 1) ? (hi)[(t) >> 3] : (lo)[(t) >> 3]) >> (16 * (((t) & 7) >> 1))) & 0xFFFFu)

__device__ __forceinline__ void ss_load_thresholds(unsigned long long *s_thr, const unsigned long long *__restrict__ thr, uint32_t n_libs) {
    for (uint32_t j = threadIdx.x; j < n_libs * SS_MAX_BATCH; j += SS_THREADS) s_thr[j] = thr[j];
    __syncthreads();
}

// thr[lib * 64 + t]; kept[t * nm + i]
__global__ __launch_bounds__(SS_THREADS) void k_ss_draw_lane(SsKeys K, const unsigned long long *__restrict__ thr, uint32_t nb, uint32_t wave_min,
                                                             unsigned long long seed, uint32_t *__restrict__ kept) {
    __shared__ unsigned long long s_thr[CRGPU_MAX_LIB * SS_MAX_BATCH];
    ss_load_thresholds(s_thr, thr, K.n_libs);
    const uint32_t ng = (nb + 7u) >> 3;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < K.nm; i += stride) {
        uint32_t lib;
        const uint32_t count = ss_count(K, i, &lib);
        if (count >= wave_min) continue;  // on a list: k_ss_draw_wave / k_ss_draw_wg write its places
        const unsigned long long m = K.mpos ? K.mpos[i] : i;
        SsAcc acc;
        ss_clear(acc);
        for (uint32_t b = 0; 4u * b < count; b++) ss_block(acc, b, m, seed, count, s_thr + lib * SS_MAX_BATCH, ng);
#pragma unroll
        for (int t = 0; t < (int)SS_MAX_BATCH; t++)
            if ((uint32_t)t < nb) kept[(uint64_t)t * K.nm + i] = (uint32_t)(acc.a[t >> 3] >> (8 * (t & 7))) & 255u;
    }
}

__global__ __launch_bounds__(SS_THREADS) void k_ss_draw_wave(SsKeys K, const uint32_t *__restrict__ list, uint32_t n_list,
                                                             const unsigned long long *__restrict__ thr, uint32_t nb, unsigned long long seed,
                                                             uint32_t *__restrict__ kept) {
    __shared__ unsigned long long s_thr[CRGPU_MAX_LIB * SS_MAX_BATCH];
    ss_load_thresholds(s_thr, thr, K.n_libs);
    const uint32_t ng = (nb + 7u) >> 3, lane = threadIdx.x & 63u;
    const uint32_t wave0 = (blockIdx.x * SS_THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * SS_THREADS) >> 6;
    for (uint32_t e = wave0; e < n_list; e += n_waves) {
        const uint64_t i = list[e];
        if (i >= K.nm) continue;
        uint32_t lib;
        const uint32_t count = ss_count(K, i, &lib);
        const uint32_t nblk = (uint32_t)(((uint64_t)count + 3ull) >> 2);
        if (nblk > 64u * SS_LANE_BLOCKS) continue;  // (uniform) never true for a list k_ss_prep wrote: the fields hold 255
        const unsigned long long m = K.mpos ? K.mpos[i] : i;
        SsAcc acc;
        ss_clear(acc);
        for (uint32_t b = lane; b < nblk; b += 64u) ss_block(acc, b, m, seed, count, s_thr + lib * SS_MAX_BATCH, ng);
        unsigned long long lo[8], hi[8];
        ss_wave_sum(acc, ng, lo, hi);
#pragma unroll
        for (int t = 0; t < (int)SS_MAX_BATCH; t++)
            if ((uint32_t)t < nb && lane == 0) kept[(uint64_t)t * K.nm + i] = SS_FIELD16(lo, hi, t);
    }
}

// list_back points at the LAST word of the list buffer: entry e is list_back[-e]
__global__ __launch_bounds__(SS_THREADS) void k_ss_draw_wg(SsKeys K, const uint32_t *__restrict__ list_back, uint32_t n_list,
                                                           const unsigned long long *__restrict__ thr, uint32_t nb, unsigned long long seed,
                                                           uint32_t *__restrict__ kept) {
    __shared__ unsigned long long s_thr[CRGPU_MAX_LIB * SS_MAX_BATCH];
    __shared__ uint32_t s_sum[SS_MAX_BATCH];
    ss_load_thresholds(s_thr, thr, K.n_libs);
    const uint32_t ng = (nb + 7u) >> 3, tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t e = blockIdx.x; e < n_list; e += gridDim.x) {
        const uint64_t i = *(list_back - e);
        if (i >= K.nm) continue;
        if (tid < SS_MAX_BATCH) s_sum[tid] = 0u;
        __syncthreads();
        uint32_t lib;
        const uint32_t count = ss_count(K, i, &lib);
        const uint64_t nblk = ((uint64_t)count + 3ull) >> 2;
        const unsigned long long m = K.mpos ? K.mpos[i] : i;
        for (uint64_t cb = 0; cb < nblk; cb += (uint64_t)SS_THREADS * SS_LANE_BLOCKS) {
            SsAcc acc;
            ss_clear(acc);
            for (uint32_t j = 0; j < SS_LANE_BLOCKS; j++) {
                const uint64_t b = cb + (uint64_t)j * SS_THREADS + tid;
                if (b < nblk) ss_block(acc, b, m, seed, count, s_thr + lib * SS_MAX_BATCH, ng);
            }
            unsigned long long lo[8], hi[8];
            ss_wave_sum(acc, ng, lo, hi);
#pragma unroll
            for (int t = 0; t < (int)SS_MAX_BATCH; t++)
                if ((uint32_t)t < nb && lane == 0) {
                    const uint32_t v = SS_FIELD16(lo, hi, t);
                    if (v) atomicAdd(&s_sum[t], v);
                }
        }
        __syncthreads();
        if (tid < nb) kept[(uint64_t)tid * K.nm + i] = s_sum[tid];
        __syncthreads();
    }
}

// ---- barcode groups -------------------------------------------------------------------------------------------------------------
// per group: the index of its barcode among the cells (NONE32: not a cell) and the genomes it is a cell of
__global__ __launch_bounds__(256) void k_ss_groups(const uint64_t *__restrict__ mkeys, uint32_t sh_bc, const uint32_t *__restrict__ seg_start,
                                                   uint32_t n_seg, const uint32_t *__restrict__ back, uint32_t n_back,
                                                   const uint32_t *__restrict__ cells, uint64_t n_cells, const uint32_t *__restrict__ cgm,
                                                   uint32_t *__restrict__ seg_cell, uint32_t *__restrict__ seg_gmask) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const uint32_t b = (uint32_t)(mkeys[seg_start[s]] >> sh_bc);
    uint32_t ci = NONE32, gm = 0u;
    if (!back || b < n_back) {
        const uint32_t r = back ? back[b] : b;
        const uint64_t lo = cr_lower_bound(cells, n_cells, r);
        if (lo < n_cells && cells[lo] == r) {
            ci = (uint32_t)lo;
            gm = cgm ? cgm[lo] : 0xFFFFFFFFu;
        }
    }
    seg_cell[s] = ci;
    seg_gmask[s] = gm;
}

struct SsTally {
    SsKeys K;
    const uint32_t *seg_start, *seg_cell, *seg_gmask;
    uint32_t n_seg, G;
    const uint8_t *fgen;    // per feature, NULL: genome 0
    const uint8_t *ttype;   // per task of the batch
    const uint32_t *kept;   // [task][molecule]
    uint64_t n_cells;
    unsigned long long *bc_umis, *bc_rp, *bc_fd;  // [task][genome][cell], zeroed
    unsigned long long *tot_rp, *tot_um;          // [task][genome], zeroed
    unsigned long long *tfd;                      // [task][genome][feature], zeroed
};

// grid (groups, tasks of the batch): one wave per (barcode group, task)
__global__ __launch_bounds__(256) void k_ss_tally(SsTally a) {
    const uint32_t lane = threadIdx.x & 63u, t = blockIdx.y, type = a.ttype[t];
    const uint32_t wave0 = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    const uint32_t *kept = a.kept + (uint64_t)t * a.K.nm;
    const unsigned long long below = lane == 63u ? ~0ull : ((2ull << lane) - 1ull);  // bits 0 .. lane
    const unsigned long long above = lane == 63u ? 0ull : (~0ull << (lane + 1u));    // bits lane + 1 .. 63
    for (uint32_t s = wave0; s < a.n_seg; s += n_waves) {
        const uint32_t s0 = a.seg_start[s], s1 = a.seg_start[s + 1], ci = a.seg_cell[s], gmask = a.seg_gmask[s];
        unsigned long long rp[8];
        uint32_t um[8], fd[8];
#pragma unroll
        for (int g = 0; g < 8; g++) {
            rp[g] = 0ull;
            um[g] = fd[g] = 0u;
        }
        bool carry = false;  // (uniform) the run that reaches into this tile already has a survivor
        for (uint32_t base = s0; base < s1; base += 64u) {
            const uint32_t i = base + lane;
            const bool in = i < s1;
            const uint64_t key = in ? a.K.mkeys[i] : 0ull;
            const uint32_t k = in ? kept[i] : 0u;
            const uint32_t f = ss_feature(a.K, key);
            const bool fok = in && f < a.K.n_features;
            const uint32_t gm = (fok && a.fgen) ? a.fgen[f] : 0u;
            uint64_t pk = __shfl_up(key, 1);
            if (lane == 0 && in && i > s0) pk = a.K.mkeys[i - 1];
            const bool head = in && (i == s0 || (key >> a.K.sh_feat) != (pk >> a.K.sh_feat));  // first molecule of a (barcode, feature) run
            const bool surv = k > 0u;
            const unsigned long long H = __ballot(head), S = __ballot(surv);
            const unsigned long long hb = H & below;  // heads at or before this lane
            const unsigned long long from = hb ? (~0ull << (63 - __clzll((long long)hb))) : ~0ull;  // the run's lanes from its head (or the tile's start)
            const bool first_tile = surv && (S & from & ((1ull << lane) - 1ull)) == 0ull;  // first survivor of its run in this tile
            const bool first_run = first_tile && (hb != 0ull || !carry);
            const unsigned long long ha = H & above;
            const unsigned long long run = ha ? (from & ((1ull << (__ffsll((long long)ha) - 1)) - 1ull)) : from;
#pragma unroll
            for (int g = 0; g < 8; g++) {
                const bool mine = gm == (uint32_t)g;
                rp[g] += mine ? k : 0u;
                um[g] += (mine && surv) ? 1u : 0u;
                fd[g] += (mine && first_run) ? 1u : 0u;
            }
            if (first_tile && fok && gm < a.G && (type == CRGPU_SS_BULK || ((gmask >> gm) & 1u)))
                atomicAdd(&a.tfd[((uint64_t)t * a.G + gm) * a.K.n_features + f], (unsigned long long)__popcll(S & run));
            const unsigned long long last = H ? (~0ull << (63 - __clzll((long long)H))) : ~0ull;
            carry = H ? (S & last) != 0ull : (carry || S != 0ull);
        }
#pragma unroll
        for (int g = 0; g < 8; g++)
            if ((uint32_t)g < a.G) {
                const unsigned long long r = wave_sum(rp[g]);
                const uint32_t u = wave_sum(um[g]), d = wave_sum(fd[g]);
                const bool cell = ci != NONE32 && ((gmask >> g) & 1u);
                if (lane == 0 && !(type == CRGPU_SS_CELLS_ONLY && !cell)) {
                    const uint64_t tg = (uint64_t)t * a.G + g;
                    if (r) atomicAdd(&a.tot_rp[tg], r);
                    if (u) atomicAdd(&a.tot_um[tg], (unsigned long long)u);
                    if (type != CRGPU_SS_BULK && cell && ci < a.n_cells) {
                        a.bc_rp[tg * a.n_cells + ci] = r;
                        a.bc_umis[tg * a.n_cells + ci] = u;
                        a.bc_fd[tg * a.n_cells + ci] = d;
                    }
                }
            }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// position of every device molecule in the table crgpu_counts_molecules lists.  One library and one UMI length: the device
// order is that order (NULL).  Otherwise the host order of cr_molecule_order, inverted, kept in the counts.
static int ss_positions(crgpu_ctx *ctx, crgpu_counts *c, const uint32_t **d_pos) {
    *d_pos = nullptr;
    const KeyLayout &L = c->layout;
    if (L.bits_lib == 0 && L.bits_ulen == 0) return CRGPU_OK;
    if (!c->d_ss_pos) {
        std::vector<uint64_t> keys;
        std::vector<uint32_t> reads, order;
        CR_TRY(cr_molecule_order(ctx, c, keys, reads, order));
        std::vector<uint32_t> pos(order.size());
        for (size_t o = 0; o < order.size(); o++) pos[order[o]] = (uint32_t)o;
        CR_TRY(cr_pool_alloc(ctx, (void **)&c->d_ss_pos, pos.size() * sizeof(uint32_t)));
        const int rc = crgpu_memcpy_h2d(ctx, c->d_ss_pos, pos.data(), pos.size() * sizeof(uint32_t));
        if (rc != CRGPU_OK) {
            cr_pool_free(ctx, c->d_ss_pos);
            c->d_ss_pos = nullptr;
            return rc;
        }
    }
    *d_pos = c->d_ss_pos;
    return CRGPU_OK;
}

static int ss_run(crgpu_ctx *ctx, crgpu_counts *c, const crgpu_subsample_args *a, crgpu_subsample_result *res) {
    const KeyLayout &L = c->layout;
    const uint32_t T = a->n_tasks, G = a->n_genomes, NL = a->n_libs, F = a->n_features;
    const uint64_t nm = c->n_molecules, NC = a->n_cells;
    // outputs start as zeros: the early returns of the reference, barcodes that are not cells, bulk's features_det_per_bc
    for (int64_t *p : {a->umis_per_bc, a->read_pairs_per_bc, a->features_det_per_bc})
        if (p && T && NC) memset(p, 0, (size_t)T * G * NC * sizeof(int64_t));
    for (int64_t *p : {a->read_pairs, a->umis})
        if (p && T) memset(p, 0, (size_t)T * G * sizeof(int64_t));
    if (a->total_features_det && T) memset(a->total_features_det, 0, (size_t)T * G * F * sizeof(int64_t));
    if (a->any_reads) memset(a->any_reads, 0, (size_t)NL * G);

    CR_TRY(cr_require_ascending_ranks(ctx, a->d_cell_ranks, NC, "crgpu_subsample_dev", "cell barcode rank"));
    if (!nm) return CRGPU_OK;

    const uint32_t wave_min = std::min<uint32_t>(std::max<uint32_t>(ctx->ss_wave_min, 1u), SS_WAVE_MIN_MAX);
    const uint32_t wg_min = std::min<uint32_t>(std::max<uint32_t>(ctx->ss_wg_min, wave_min), SS_WG_MIN_MAX);
    const uint32_t *d_pos = nullptr;
    CR_TRY(ss_positions(ctx, c, &d_pos));
    DevBuf fmask_b, fgen_b, cgm_b, small_b, list_b, ctl_b;
    if (a->feature_mask) {
        CR_TRY(dmalloc(ctx, fmask_b, F));
        CR_TRY(crgpu_memcpy_h2d(ctx, fmask_b.p, a->feature_mask, F));
    }
    if (a->feature_genome) {
        CR_TRY(dmalloc(ctx, fgen_b, F));
        CR_TRY(crgpu_memcpy_h2d(ctx, fgen_b.p, a->feature_genome, F));
    }
    if (a->cell_genome_mask && NC) {
        CR_TRY(dmalloc(ctx, cgm_b, NC * sizeof(uint32_t)));
        CR_TRY(crgpu_memcpy_h2d(ctx, cgm_b.p, a->cell_genome_mask, NC * sizeof(uint32_t)));
    }
    const SsKeys K{c->d_mkeys, c->d_mreads, d_pos, fmask_b.as<uint8_t>(), nm, L.sh_feat(), L.bits_feat, L.sh_libid(), L.bits_lib, F, NL};
    const uint8_t *d_fgen = fgen_b.as<uint8_t>();

    // 1. prep
    const uint64_t small_bytes = (uint64_t)NL + (uint64_t)NL * G;  // lib_present, any_reads
    CR_TRY(dmalloc(ctx, small_b, small_bytes));
    CR_TRY(dmalloc(ctx, list_b, nm * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, ctl_b, SS_CTL_WORDS * sizeof(uint32_t)));
    uint8_t *d_present = small_b.as<uint8_t>(), *d_any = d_present + NL;
    uint32_t *list = list_b.as<uint32_t>(), *ctl = ctl_b.as<uint32_t>();
    {
        CrTimer t(ctx, CRGPU_T_DEDUP, nm);
        CR_HIP(ctx, hipMemsetAsync(small_b.p, 0, small_bytes, ctx->stream));
        CR_HIP(ctx, hipMemsetAsync(ctl, 0, SS_CTL_WORDS * sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(k_ss_prep, dim3(cr_grid(nm, 256)), dim3(256), 0, ctx->stream, K, d_fgen, G, wave_min, wg_min, d_present, d_any, list, ctl);
        CR_HIP(ctx, hipGetLastError());
    }
    uint32_t h_ctl[SS_CTL_WORDS];
    std::vector<uint8_t> h_small(small_bytes);
    CR_TRY(crgpu_memcpy_d2h(ctx, h_ctl, ctl, sizeof(h_ctl)));
    CR_TRY(crgpu_memcpy_d2h(ctx, h_small.data(), small_b.p, small_bytes));
    CR_REQUIRE(ctx, !h_ctl[SS_CTL_BAD], CRGPU_ESTATE, "crgpu_subsample_dev: a molecule key holds a feature >= %u or a library >= %u", F, NL);
    const uint32_t n_wave = h_ctl[SS_CTL_N_WAVE], n_wg = h_ctl[SS_CTL_N_WG];
    uint64_t n_used = 0;
    memcpy(&n_used, h_ctl + SS_CTL_N_USED, sizeof(n_used));
    CR_REQUIRE(ctx, (uint64_t)n_wave + n_wg <= nm && n_used <= nm, CRGPU_EHIP, "crgpu_subsample_dev: inconsistent molecule classes");
    if (a->any_reads) memcpy(a->any_reads, h_small.data() + NL, (size_t)NL * G);
    if (res) {
        res->n_molecules = n_used;
        res->n_wave = n_wave;
        res->n_workgroup = n_wg;
        res->n_lane = n_used - n_wave - n_wg;
    }

    // the tasks that draw (subsample.py:598-605), their thresholds
    std::vector<uint32_t> active;
    std::vector<unsigned long long> thr_all((size_t)T * NL, 0ull);
    for (uint32_t t = 0; t < T; t++) {
        bool nonzero = false, nan_present = false;
        for (uint32_t l = 0; l < NL; l++) {
            const double r = a->rates[(size_t)t * NL + l];
            if (std::isnan(r)) {
                nonzero = true;  // (np.count_nonzero counts a NaN)
                nan_present |= h_small[l] != 0;
            } else {
                nonzero |= r != 0.0;
                thr_all[(size_t)t * NL + l] = (unsigned long long)std::floor(std::ldexp(r, 53));  // exact: r in [0, 1]
            }
        }
        if (nonzero && !nan_present) active.push_back(t);
    }
    if (res) res->n_active_tasks = (uint32_t)active.size();
    if (active.empty() || !n_used) return CRGPU_OK;

    // 2. barcode groups
    DevBuf seg_b, scell_b, sgm_b;
    uint32_t n_seg = 0;
    CR_TRY(cr_barcode_segments(ctx, c, "crgpu_subsample_dev", seg_b, &n_seg));
    const uint32_t *seg_start = seg_b.as<uint32_t>();
    if (res) res->n_groups = n_seg;
    CR_TRY(dmalloc(ctx, scell_b, (uint64_t)n_seg * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, sgm_b, (uint64_t)n_seg * sizeof(uint32_t)));
    {
        CrTimer t(ctx, CRGPU_T_DEDUP, n_seg);
        hipLaunchKernelGGL(k_ss_groups, dim3((n_seg + 255u) / 256u), dim3(256), 0, ctx->stream, c->d_mkeys, L.sh_bc(), seg_start, n_seg, c->d_back,
                           c->n_back, a->d_cell_ranks, NC, cgm_b.as<uint32_t>(), scell_b.as<uint32_t>(), sgm_b.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
    }

    // 3./4. batches of tasks: the temporaries of a batch stay below a fixed budget
    const uint64_t per_task = nm * sizeof(uint32_t) + ((uint64_t)3 * G * NC + (uint64_t)G * F + 2ull * G) * sizeof(unsigned long long);
    const uint64_t budget = std::min<uint64_t>(8ull << 30, ctx->pool_budget / 4);
    uint32_t nb_max = (uint32_t)std::min<uint64_t>(SS_MAX_BATCH, std::max<uint64_t>(1, budget / per_task));
    if (ctx->ss_task_batch) nb_max = std::min<uint32_t>(ctx->ss_task_batch, SS_MAX_BATCH);
    nb_max = std::min<uint32_t>(nb_max, (uint32_t)active.size());
    const uint64_t n_bc_words = (uint64_t)G * NC, n_tot = (uint64_t)G, n_tfd = (uint64_t)G * F;
    const uint64_t words_per_task = 3 * n_bc_words + 2 * n_tot + n_tfd;
    DevBuf kept_b, out_b, thr_b, type_b;
    CR_TRY(dmalloc(ctx, kept_b, (uint64_t)nb_max * nm * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, out_b, (uint64_t)nb_max * words_per_task * sizeof(unsigned long long)));
    CR_TRY(dmalloc(ctx, thr_b, (uint64_t)CRGPU_MAX_LIB * SS_MAX_BATCH * sizeof(unsigned long long)));
    CR_TRY(dmalloc(ctx, type_b, SS_MAX_BATCH));
    CrEvents<2> events(ctx);
    const hipEvent_t e0 = events.e[0], e1 = events.e[1];
    CR_REQUIRE(ctx, e0 && e1, CRGPU_EHIP, "crgpu_subsample_dev: no event");
    std::vector<unsigned long long> h_thr((size_t)CRGPU_MAX_LIB * SS_MAX_BATCH), h_tot, h_tfd;
    std::vector<uint8_t> h_type(SS_MAX_BATCH);
    double draw_ms = 0.0;
    uint32_t n_batches = 0;
    for (size_t first = 0; first < active.size(); first += nb_max, n_batches++) {
        const uint32_t nb = (uint32_t)std::min<size_t>(nb_max, active.size() - first);
        std::fill(h_thr.begin(), h_thr.end(), 0ull);
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t t = active[first + k];
            h_type[k] = a->task_type[t];
            for (uint32_t l = 0; l < NL; l++) h_thr[(size_t)l * SS_MAX_BATCH + k] = thr_all[(size_t)t * NL + l];
        }
        CR_TRY(crgpu_memcpy_h2d(ctx, thr_b.p, h_thr.data(), h_thr.size() * sizeof(unsigned long long)));
        CR_TRY(crgpu_memcpy_h2d(ctx, type_b.p, h_type.data(), SS_MAX_BATCH));
        unsigned long long *o = out_b.as<unsigned long long>();
        SsTally ta{K, seg_start, scell_b.as<uint32_t>(), sgm_b.as<uint32_t>(), n_seg, G, d_fgen, type_b.as<uint8_t>(), kept_b.as<uint32_t>(), NC,
                   o, o + (uint64_t)nb * n_bc_words, o + 2ull * nb * n_bc_words, o + 3ull * nb * n_bc_words,
                   o + 3ull * nb * n_bc_words + (uint64_t)nb * n_tot, o + 3ull * nb * n_bc_words + 2ull * nb * n_tot};
        {
            CrTimer t(ctx, CRGPU_T_DEDUP, nm * nb);
            CR_HIP(ctx, hipMemsetAsync(o, 0, (uint64_t)nb * words_per_task * sizeof(unsigned long long), ctx->stream));
            (void)hipEventRecord(e0, ctx->stream);
            hipLaunchKernelGGL(k_ss_draw_lane, dim3(cr_grid(nm, SS_THREADS, 256u * 16u)), dim3(SS_THREADS), 0, ctx->stream, K,
                               thr_b.as<unsigned long long>(), nb, wave_min, (unsigned long long)a->seed, kept_b.as<uint32_t>());
            if (n_wave)
                hipLaunchKernelGGL(k_ss_draw_wave, dim3(cr_grid((uint64_t)n_wave * 64, SS_THREADS, 256u * 16u)), dim3(SS_THREADS), 0, ctx->stream, K,
                                   list, n_wave, thr_b.as<unsigned long long>(), nb, (unsigned long long)a->seed, kept_b.as<uint32_t>());
            if (n_wg)
                hipLaunchKernelGGL(k_ss_draw_wg, dim3(std::min<uint32_t>(n_wg, 256u * 8u)), dim3(SS_THREADS), 0, ctx->stream, K, list + (nm - 1), n_wg,
                                   thr_b.as<unsigned long long>(), nb, (unsigned long long)a->seed, kept_b.as<uint32_t>());
            (void)hipEventRecord(e1, ctx->stream);
            hipLaunchKernelGGL(k_ss_tally, dim3(cr_grid((uint64_t)n_seg * 64, 256, 256u * 8u), nb), dim3(256), 0, ctx->stream, ta);
            CR_HIP(ctx, hipGetLastError());
        }
        // results of the batch (the copies synchronise the stream: the temporaries are free for the next batch)
        h_tot.resize((size_t)2 * nb * n_tot);
        CR_TRY(crgpu_memcpy_d2h(ctx, h_tot.data(), ta.tot_rp, h_tot.size() * sizeof(unsigned long long)));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e0, e1) == hipSuccess) draw_ms += ms;
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t t = active[first + k];
            const bool bulk = a->task_type[t] == CRGPU_SS_BULK;
            const unsigned long long *rp = h_tot.data() + (size_t)k * n_tot, *um = h_tot.data() + (size_t)(nb + k) * n_tot;
            if (a->read_pairs) memcpy(a->read_pairs + (size_t)t * G, rp, n_tot * sizeof(int64_t));
            if (a->umis) memcpy(a->umis + (size_t)t * G, um, n_tot * sizeof(int64_t));
            if (a->total_features_det && n_tfd)
                CR_TRY(crgpu_memcpy_d2h(ctx, a->total_features_det + (size_t)t * n_tfd, ta.tfd + (uint64_t)k * n_tfd, n_tfd * sizeof(int64_t)));
            if (!n_bc_words) continue;
            if (bulk) {  // one group: every cell entry holds the table's total (subsample.py:631-633)
                for (uint32_t g = 0; g < G; g++)
                    for (uint64_t ci = 0; ci < NC; ci++) {
                        if (a->umis_per_bc) a->umis_per_bc[((size_t)t * G + g) * NC + ci] = (int64_t)um[g];
                        if (a->read_pairs_per_bc) a->read_pairs_per_bc[((size_t)t * G + g) * NC + ci] = (int64_t)rp[g];
                    }
                continue;
            }
            if (a->umis_per_bc)
                CR_TRY(crgpu_memcpy_d2h(ctx, a->umis_per_bc + (size_t)t * n_bc_words, ta.bc_umis + (uint64_t)k * n_bc_words, n_bc_words * sizeof(int64_t)));
            if (a->read_pairs_per_bc)
                CR_TRY(crgpu_memcpy_d2h(ctx, a->read_pairs_per_bc + (size_t)t * n_bc_words, ta.bc_rp + (uint64_t)k * n_bc_words, n_bc_words * sizeof(int64_t)));
            if (a->features_det_per_bc)
                CR_TRY(crgpu_memcpy_d2h(ctx, a->features_det_per_bc + (size_t)t * n_bc_words, ta.bc_fd + (uint64_t)k * n_bc_words, n_bc_words * sizeof(int64_t)));
        }
    }
    if (res) {
        res->n_batches = n_batches;
        res->draw_ms = draw_ms;
    }
    return CRGPU_OK;
}

extern "C" int crgpu_subsample_dev(crgpu_ctx *ctx, crgpu_counts *c, const crgpu_subsample_args *a, crgpu_subsample_result *res) {
    if (!ctx || !c || !a) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    if (res) memset(res, 0, sizeof(*res));
    const KeyLayout &L = c->layout;
    CR_REQUIRE(ctx, a->n_genomes >= 1 && a->n_genomes <= 8, CRGPU_EINVAL, "crgpu_subsample_dev: n_genomes must be 1..8");
    CR_REQUIRE(ctx, a->n_libs == L.n_libs && a->n_features == L.n_features, CRGPU_EINVAL,
               "crgpu_subsample_dev: n_libs %u / n_features %u, the counts were made with %u / %u", a->n_libs, a->n_features, L.n_libs, L.n_features);
    CR_REQUIRE(ctx, a->n_tasks == 0 || (a->rates && a->task_type), CRGPU_EINVAL, "crgpu_subsample_dev: NULL rates or task types");
    CR_REQUIRE(ctx, a->n_cells == 0 || a->d_cell_ranks, CRGPU_EINVAL, "crgpu_subsample_dev: NULL cell ranks");
    CR_REQUIRE(ctx, a->n_cells < 0xFFFFFFFFull && c->n_molecules < 0xFFFFFFFFull, CRGPU_ERANGE, "crgpu_subsample_dev: too many cells or molecules");
    for (uint32_t t = 0; t < a->n_tasks; t++) {
        CR_REQUIRE(ctx, a->task_type[t] <= CRGPU_SS_BULK, CRGPU_EINVAL, "crgpu_subsample_dev: task %u has type %u", t, a->task_type[t]);
        for (uint32_t l = 0; l < a->n_libs; l++) {
            const double r = a->rates[(size_t)t * a->n_libs + l];
            CR_REQUIRE(ctx, std::isnan(r) || (r >= 0.0 && r <= 1.0), CRGPU_EINVAL,
                       "crgpu_subsample_dev: subsampling probabilities cannot be < 0 or > 1 (task %u, library %u: %g)", t, l, r);
        }
    }
    for (uint32_t f = 0; a->feature_genome && f < a->n_features; f++)
        CR_REQUIRE(ctx, a->feature_genome[f] < a->n_genomes, CRGPU_EINVAL, "crgpu_subsample_dev: feature %u belongs to genome %u of %u", f,
                   a->feature_genome[f], a->n_genomes);
    const int rc = ss_run(ctx, c, a, res);
    if (rc != CRGPU_OK) (void)hipStreamSynchronize(ctx->stream);  // the temporaries go back to the pool behind this
    return rc;
}

// ---- the plan (subsample.py:140-309), host ---------------------------------------------------------------------------------------
static double ss_np_min(const double *v, const uint32_t *idx, uint32_t n) {  // np.min: a NaN wins
    double m = v[idx[0]];
    for (uint32_t i = 0; i < n; i++) {
        const double x = v[idx[i]];
        if (std::isnan(x)) return x;
        if (x < m) m = x;
    }
    return m;
}

extern "C" int crgpu_subsample_plan(int subsample_type, const uint32_t *lib_indices, uint32_t n_lib_indices, uint32_t n_libs,
                                    const double *num_cells_per_lib, const double *raw_reads_per_lib, const double *usable_reads_per_lib,
                                    const int64_t *fixed_depths, uint32_t n_fixed_depths, uint32_t num_additional_depths, int64_t *depths_out,
                                    double *rates_out, uint32_t cap, uint32_t *n_out) {
    if (n_out) *n_out = 0;
    if (!n_out || !lib_indices || !n_lib_indices || !n_libs || !num_cells_per_lib || !raw_reads_per_lib || !usable_reads_per_lib ||
        (n_fixed_depths && !fixed_depths) || subsample_type < CRGPU_SS_PLAN_RAW || subsample_type > CRGPU_SS_PLAN_BULK)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_subsample_plan: NULL or empty argument, or an unknown subsample type");
    for (uint32_t i = 0; i < n_lib_indices; i++)
        if (lib_indices[i] >= n_libs) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_subsample_plan: library index %u of %u", lib_indices[i], n_libs);
    const bool bulk = subsample_type == CRGPU_SS_PLAN_BULK, mapped = subsample_type == CRGPU_SS_PLAN_MAPPED;
    std::vector<double> raw_rppc(n_libs), usable_rppc(n_libs), usable_frac(n_libs);
    for (uint32_t l = 0; l < n_libs; l++) {
        raw_rppc[l] = raw_reads_per_lib[l] / num_cells_per_lib[l];
        usable_rppc[l] = usable_reads_per_lib[l] / num_cells_per_lib[l];
        usable_frac[l] = usable_reads_per_lib[l] / raw_reads_per_lib[l];
    }
    const double max_target = ss_np_min(bulk ? raw_reads_per_lib : (mapped ? usable_rppc.data() : raw_rppc.data()), lib_indices, n_lib_indices);
    if (!std::isfinite(max_target) || max_target >= 0x1.0p62)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_subsample_plan: the largest feasible depth is %g", max_target);
    // compute_target_depths: unique(linspace(0, max, num + 1, dtype=int)) without the zeros
    std::vector<int64_t> depths;
    if (num_additional_depths >= 1) {
        const double step = max_target / (double)num_additional_depths;
        for (uint32_t i = 0; i <= num_additional_depths; i++) {
            const double y = i == num_additional_depths ? max_target : (double)i * step;
            depths.push_back((int64_t)y);  // truncation, as astype(int)
        }
    }
    std::sort(depths.begin(), depths.end());
    depths.erase(std::unique(depths.begin(), depths.end()), depths.end());
    depths.erase(std::remove_if(depths.begin(), depths.end(), [](int64_t d) { return d <= 0; }), depths.end());
    const bool have_max = !depths.empty();
    const int64_t max_computed = have_max ? depths.back() : 0;
    depths.insert(depths.end(), fixed_depths, fixed_depths + n_fixed_depths);
    std::sort(depths.begin(), depths.end());
    depths.erase(std::unique(depths.begin(), depths.end()), depths.end());
    *n_out = (uint32_t)depths.size();
    if (!depths_out && !rates_out) return CRGPU_OK;
    if (depths.size() > cap) return cr_fail(nullptr, CRGPU_ERANGE, "crgpu_subsample_plan: %zu depths, room for %u", depths.size(), cap);
    std::vector<double> rates(n_libs);
    for (size_t d = 0; d < depths.size(); d++) {
        const double depth = (double)depths[d];
        std::fill(rates.begin(), rates.end(), 0.0);
        const double *den = bulk ? raw_reads_per_lib : usable_reads_per_lib;
        for (uint32_t i = 0; i < n_lib_indices; i++) {
            const uint32_t l = lib_indices[i];
            const double target = bulk ? depth : (mapped ? depth * num_cells_per_lib[l] : depth * num_cells_per_lib[l] * usable_frac[l]);
            if (den[l] != 0.0) rates[l] = target / den[l];
        }
        if (have_max && depths[d] == max_computed) {  // the smallest library is subsampled at rate 1
            double mx = rates[0];
            for (double r : rates) {
                if (std::isnan(r)) {
                    mx = r;
                    break;
                }
                if (r > mx) mx = r;
            }
            if (mx != 0.0)
                for (double &r : rates) r = r / mx;
        }
        for (double &r : rates)
            if (r > 1.0) r = 0.0;
        if (depths_out) depths_out[d] = depths[d];
        if (rates_out) memcpy(rates_out + d * n_libs, rates.data(), n_libs * sizeof(double));
    }
    return CRGPU_OK;
}

// ---- the summary (subsample.py:719-845), host ------------------------------------------------------------------------------------
static void ss_mean_median(std::vector<int64_t> &v, double *mean, double *median) {
    const size_t n = v.size();
    if (!n) {
        *mean = *median = NAN;
        return;
    }
    double sum = 0.0;
    for (int64_t x : v) sum += (double)x;  // (exact below 2^53, whatever the order)
    *mean = sum / (double)n;
    std::sort(v.begin(), v.end());
    *median = cr_median_sorted(v);
}

extern "C" int crgpu_subsample_summary(uint32_t n_tasks, uint32_t n_genomes, uint64_t n_cells, uint32_t n_features, const uint8_t *task_type,
                                       const uint32_t *cell_genome_mask, const int64_t *umis_per_bc, const int64_t *read_pairs_per_bc,
                                       const int64_t *features_det_per_bc, const int64_t *read_pairs, const int64_t *umis,
                                       const int64_t *total_features_det, double *out, double *dup_frac_all_out) {
    if (!out || !task_type || !read_pairs || !umis || n_genomes < 1 || n_genomes > 8 ||
        (n_cells && (!umis_per_bc || !read_pairs_per_bc || !features_det_per_bc)))
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_subsample_summary: NULL argument or n_genomes outside 1..8");
    auto dup = [](int64_t rp, int64_t um) { return rp > 0 ? (double)(rp - um) / (double)rp : 0.0; };
    std::vector<int64_t> v;
    for (uint32_t t = 0; t < n_tasks; t++) {
        const bool bulk = task_type[t] == CRGPU_SS_BULK;
        if (bulk && !total_features_det) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_subsample_summary: a bulk task needs total_features_det");
        int64_t all_rp = 0, all_um = 0;
        for (uint32_t g = 0; g < n_genomes; g++) {
            const size_t tg = (size_t)t * n_genomes + g;
            double *o = out + tg * CRGPU_SS_SUMMARY_COLS;
            const int64_t *src[3] = {read_pairs_per_bc, umis_per_bc, features_det_per_bc};
            for (int k = 0; k < 3; k++) {
                v.clear();
                for (uint64_t ci = 0; ci < n_cells; ci++)
                    if (!cell_genome_mask || ((cell_genome_mask[ci] >> g) & 1u)) v.push_back(src[k][tg * n_cells + ci]);
                ss_mean_median(v, &o[2 * k], &o[2 * k + 1]);
            }
            if (bulk) {
                uint64_t nz = 0;
                for (uint32_t f = 0; f < n_features; f++) nz += total_features_det[tg * n_features + f] != 0;
                o[CRGPU_SS_MEAN_FEATURES] = o[CRGPU_SS_MEDIAN_FEATURES] = (double)nz;
            }
            o[CRGPU_SS_DUP_FRAC] = dup(read_pairs[tg], umis[tg]);
            all_rp += read_pairs[tg];
            all_um += umis[tg];
        }
        if (dup_frac_all_out) dup_frac_all_out[t] = dup(all_rp, all_um);
    }
    return CRGPU_OK;
}
