// matrix_summary.h -- the summary metrics of the filtered matrix on the device (part of matrix_stages.hip).
//
// Replaces the matrix arithmetic of report_genomes -> _report / _report_genome_agnostic_metrics
// (lib/python/cellranger/rna/report_matrix.py:76-387): sum_masked / count_ge_masked of the views (feature mask x barcode mask) of
// the RAW matrix (cellranger/sparse.py:36-168) and top_n (matrix.py:55-67).  A class is one (feature type, genome) pair.
//
//   1. cr_check_columns with MarkPlace: cellidx[c] = k + 1 for the k-th listed cell (0: not a cell); the list is checked on the way.
//   2. k_ms_pass, ONE pass over all columns, one wave per column (the loads of MS_UNROLL rounds of 64 entries are issued together, the
//      bounds of the wave's next column one column ahead: the pass waits for loads, not for the LDS): per class the column's sum and its entries >= 1 (static
//      accumulators per lane, a wave reduction per class the column holds) feed the class totals (lane k keeps class k, one LDS
//      add per wave, one global add per workgroup) and the per-cell arrays; every entry of a cell of its feature's class is added
//      to the feature's counters.  Those live in a SLICE of the workgroup's LDS (u32 sum, u32 count of entries >= 2 and the class
//      byte per feature); workgroup (s, w) owns slice s of the rows and every G-th group of 16 columns.  Rows ascend inside a
//      column, so a wave finds its slice by a 64-ary search (columns of at most 64 entries are read whole and filtered).  A u32
//      sum that wraps carries 2^32 into a u64 per feature in device memory.  At the end a workgroup stores its slice to the slab
//      [w][feature] with plain coalesced stores.
//   3. k_ms_slab_sum adds the slab up per feature: no global atomic on a hot row, integer sums in any order.
//   4. k_ms_finish: the per-cell sums as u32 (CRGPU_ERANGE beyond), their moments (the sum of squares in 128 bits) and the keys
//      ((2 class + which) << 32) | value; ONE radix sort serves every class and both arrays; the six order statistics per array
//      are gathered from it.  Top features and genes detected are host work over the per-feature arrays.
// With ctx->ms_lds_features == 0 the per-feature counters are u64 atomics in device memory (the A/B of the slice form).
// The floats of _report come from the integers on the host (crgpu_matrix_summary_stats): f64, unfused.
#pragma once

#include <algorithm>
#include <cmath>

#include "stage_common.h"

#define MS_NONE 0xFFu
#define MS_WG 1024u                                 // threads of a pass workgroup: 16 waves, one column each
#define MS_WAVES (MS_WG / 64u)
#define MS_UNROLL 4                                 // rounds of 64 entries whose loads a wave issues together
#define MS_LDS_BYTES (160u * 1024u - 64u)
#define MS_STATIC_BYTES 2048u                       // room for the pass's static LDS (the class totals)
#define MS_SLICE_MAX ((MS_LDS_BYTES - MS_STATIC_BYTES) / 9u)  // u32 sum + u32 count + class byte per feature
#define MS_T_RAW 0u
#define MS_T_UNION 1u
#define MS_T_UNION_NNZ 2u
#define MS_T_CELLS 3u
#define MS_T_CELLS_NNZ 4u
#define MS_T_WORDS 5u
#define MS_T_SEEN (CRGPU_MS_MAX_CLASSES * MS_T_WORDS)  // entries the pass looked at: == nnz when the rows ascend
#define MS_T_TOTAL (MS_T_SEEN + 1u)

template <int NC, bool LDS>
__global__ __launch_bounds__(MS_WG) void k_ms_pass(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                   const int32_t *__restrict__ data, uint64_t V, const uint8_t *__restrict__ fclass,
                                                   uint32_t n_features, uint32_t n_classes, const uint32_t *__restrict__ cellidx,
                                                   const uint32_t *__restrict__ cellmask, uint64_t n_cells, uint32_t slice, uint32_t G,
                                                   uint2 *__restrict__ slab, unsigned long long *__restrict__ carry,
                                                   unsigned long long *__restrict__ gsum, unsigned long long *__restrict__ gcnt,
                                                   unsigned long long *__restrict__ cell_sum, uint32_t *__restrict__ cell_genes,
                                                   unsigned long long *__restrict__ tot, uint32_t *__restrict__ flag) {
    extern __shared__ uint32_t s_dyn[];  // LDS: sum[slice], count[slice], class byte [slice]
    __shared__ unsigned long long s_tot[MS_T_TOTAL];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t w = LDS ? blockIdx.x % G : blockIdx.x, n_wg = LDS ? G : gridDim.x;
    const uint32_t lo = LDS ? (blockIdx.x / G) * slice : 0u;
    const uint32_t hi = LDS ? (n_features - lo < slice ? n_features : lo + slice) : n_features;
    uint32_t *s_sum = s_dyn, *s_cnt = s_dyn + slice;
    uint8_t *s_cls = (uint8_t *)(s_dyn + 2 * (size_t)slice);
    if (LDS)
        for (uint32_t i = tid; i < hi - lo; i += MS_WG) s_sum[i] = 0u, s_cnt[i] = 0u, s_cls[i] = fclass[lo + i];
    for (uint32_t i = tid; i < MS_T_TOTAL; i += MS_WG) s_tot[i] = 0ull;
    __syncthreads();
    unsigned long long t_raw = 0, t_union = 0, t_union_nnz = 0, t_cells = 0, t_cells_nnz = 0;  // lane k: class k
    uint32_t seen = 0;
    bool bad = false;
    const uint64_t c_step = (uint64_t)n_wg * MS_WAVES;
    uint64_t c = (uint64_t)w * MS_WAVES + wave;
    long long nb = 0, ne = 0;  // the bounds of the wave's next column, loaded one column ahead
    uint32_t nci = 0;
    if (c < V) nb = indptr[c], ne = indptr[c + 1], nci = cellidx[c];
    for (; c < V; c += c_step) {  // uniform in the wave
        long long b = nb, e = ne;
        const uint32_t ci = nci;
        if (c + c_step < V) nb = indptr[c + c_step], ne = indptr[c + c_step + 1], nci = cellidx[c + c_step];
        if (b >= e) continue;
        const uint32_t mask = ci ? cellmask[ci - 1u] : 0u;
        if (LDS && e - b > 64) {
            if (lo > 0u) b = wave_lower_bound(indices, b, e, lo, lane);
            if (hi < n_features) e = wave_lower_bound(indices, b, e, hi, lane);
        }
        unsigned long long acc[NC];
        uint32_t nz[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) acc[k] = 0ull, nz[k] = 0u;
        for (long long i0 = b + lane; i0 - lane < e; i0 += 64 * MS_UNROLL) {
            // the loads of MS_UNROLL rounds are issued before the first entry is counted: a wave keeps 2 x MS_UNROLL loads in flight
            uint32_t fs[MS_UNROLL], ds[MS_UNROLL];
#pragma unroll
            for (int u = 0; u < MS_UNROLL; u++) {
                const long long i = i0 + 64 * u;
                fs[u] = i < e ? (uint32_t)indices[i] : 0xFFFFFFFFu;
                ds[u] = i < e ? (uint32_t)data[i] : 0u;
            }
#pragma unroll
            for (int u = 0; u < MS_UNROLL; u++) {
                const uint32_t f = fs[u], d = ds[u];
                if (i0 + 64 * u >= e) continue;
                if (f >= n_features) {
                    bad = true;
                    continue;
                }
                if (f < lo || f >= hi) continue;  // another slice's (a short column is not searched)
                seen++;
                const uint32_t fc = LDS ? s_cls[f - lo] : fclass[f];
                if (fc >= n_classes) continue;  // in no class
#pragma unroll
                for (int k = 0; k < NC; k++) acc[k] += fc == (uint32_t)k ? d : 0u, nz[k] += (fc == (uint32_t)k && d) ? 1u : 0u;
                if (!((mask >> fc) & 1u)) continue;
                if (LDS) {
                    const uint32_t old = atomicAdd(&s_sum[f - lo], d);
                    if (old + d < old) atomicAdd(&carry[f], 1ull << 32);  // the u32 counter wrapped
                    if (d >= 2u) atomicAdd(&s_cnt[f - lo], 1u);
                } else {
                    atomicAdd(&gsum[f], (unsigned long long)d);
                    if (d >= 2u) atomicAdd(&gcnt[f], 1ull);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NC; k++) {
            if ((uint32_t)k >= n_classes || !__ballot(acc[k] != 0ull || nz[k] != 0u)) continue;  // uniform
            const unsigned long long sum = wave_sum(acc[k]);
            const uint32_t n = wave_sum(nz[k]);
            const bool own = (mask >> k) & 1u;
            if (lane == (uint32_t)k) {
                t_raw += sum;
                if (ci) t_union += sum, t_union_nnz += n;
                if (own) t_cells += sum, t_cells_nnz += n;
            }
            if (lane == 0u && own) {  // one address per (cell, class): the slices of a column add up here
                atomicAdd(&cell_sum[(uint64_t)k * n_cells + (ci - 1u)], sum);
                atomicAdd(&cell_genes[(uint64_t)k * n_cells + (ci - 1u)], n);
            }
        }
    }
    if (bad) atomicOr(flag, 1u);
    seen = wave_sum(seen);
    if (lane == 0u && seen) atomicAdd(&s_tot[MS_T_SEEN], (unsigned long long)seen);
    if (lane < n_classes) {
        unsigned long long *t = s_tot + lane * MS_T_WORDS;
        if (t_raw) atomicAdd(&t[MS_T_RAW], t_raw);
        if (t_union) atomicAdd(&t[MS_T_UNION], t_union);
        if (t_union_nnz) atomicAdd(&t[MS_T_UNION_NNZ], t_union_nnz);
        if (t_cells) atomicAdd(&t[MS_T_CELLS], t_cells);
        if (t_cells_nnz) atomicAdd(&t[MS_T_CELLS_NNZ], t_cells_nnz);
    }
    __syncthreads();
    for (uint32_t i = tid; i < MS_T_TOTAL; i += MS_WG)
        if (s_tot[i]) atomicAdd(&tot[i], s_tot[i]);
    if (LDS) {
        uint2 *row = slab + (size_t)w * n_features + lo;
        for (uint32_t i = tid; i < hi - lo; i += MS_WG) row[i] = make_uint2(s_sum[i], s_cnt[i]);
    }
}

__global__ __launch_bounds__(256) void k_ms_slab_sum(const uint2 *__restrict__ slab, uint32_t G, uint32_t n_features,
                                                     const unsigned long long *__restrict__ carry, unsigned long long *__restrict__ sum_out,
                                                     unsigned long long *__restrict__ cnt_out) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < n_features; f += stride) {
        unsigned long long s = carry[f], n = 0ull;
        for (uint32_t g = 0; g < G; g++) {
            const uint2 v = slab[(size_t)g * n_features + f];
            s += v.x, n += v.y;
        }
        sum_out[f] = s, cnt_out[f] = n;
    }
}

// out[0] = every column, out[1] = every listed cell, out[2 + k] = the cells of class k
__global__ __launch_bounds__(256) void k_ms_reads(const uint32_t *__restrict__ reads, uint64_t V, const uint32_t *__restrict__ cellidx,
                                                  const uint32_t *__restrict__ cellmask, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long s_out[2 + CRGPU_MS_MAX_CLASSES];
    if (threadIdx.x < 2 + CRGPU_MS_MAX_CLASSES) s_out[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long all = 0, listed = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < V; c += stride) {
        const uint32_t r = reads[c], ci = cellidx[c];
        all += r;
        if (!ci) continue;
        listed += r;
        for (uint32_t mk = cellmask[ci - 1u]; mk && r; mk &= mk - 1u) atomicAdd(&s_out[2 + __builtin_ctz(mk)], (unsigned long long)r);
    }
    all = wave_sum(all), listed = wave_sum(listed);
    if ((threadIdx.x & 63u) == 0u) {
        if (all) atomicAdd(&s_out[0], all);
        if (listed) atomicAdd(&s_out[1], listed);
    }
    __syncthreads();
    if (threadIdx.x < 2 + CRGPU_MS_MAX_CLASSES && s_out[threadIdx.x]) atomicAdd(&out[threadIdx.x], s_out[threadIdx.x]);
}

// a 128-bit sum as two u64 words, added with integer atomics: hi takes the carries of lo
__device__ __forceinline__ void ms_add128(unsigned long long *hi, unsigned long long *lo, unsigned long long vhi, unsigned long long vlo) {
    if (vlo) {
        const unsigned long long old = atomicAdd(lo, vlo);
        if (old + vlo < old) vhi++;
    }
    if (vhi) atomicAdd(hi, vhi);
}

// grid (x, class).  keys[(2 k + which) * n_cells + j] = ((2 k + which) << 32) | value for a cell of the class, (2 n_classes) << 32 else;
// mom[k * 6 ..] = sum, sumsq hi, sumsq lo of the counts, then of the genes; flag: a per-cell sum above 2^32 - 1
__global__ __launch_bounds__(256) void k_ms_finish(const unsigned long long *__restrict__ cell_sum, const uint32_t *__restrict__ cell_genes,
                                                   const uint32_t *__restrict__ cellmask, uint64_t n_cells, uint32_t n_classes,
                                                   uint64_t *__restrict__ keys, uint32_t *__restrict__ counts_out, uint32_t *__restrict__ genes_out,
                                                   unsigned long long *__restrict__ mom, uint32_t *__restrict__ flag) {
    __shared__ unsigned long long s_m[6];
    if (threadIdx.x < 6) s_m[threadIdx.x] = 0ull;
    __syncthreads();
    const uint32_t k = blockIdx.y;
    const uint64_t none = (uint64_t)(2u * n_classes) << 32, row = (uint64_t)k * n_cells;
    unsigned long long cs = 0, cq_hi = 0, cq_lo = 0, gs = 0, gq_hi = 0, gq_lo = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_cells; j += stride) {
        const bool own = (cellmask[j] >> k) & 1u;
        uint64_t key0 = none, key1 = none;
        uint32_t x = 0, g = 0;
        if (own) {
            const unsigned long long s = cell_sum[row + j];
            if (s > 0xFFFFFFFFull) atomicOr(flag, 1u);
            x = (uint32_t)s, g = cell_genes[row + j];
            key0 = ((uint64_t)(2u * k) << 32) | x, key1 = ((uint64_t)(2u * k + 1u) << 32) | g;
            const unsigned long long x2 = (unsigned long long)x * x, g2 = (unsigned long long)g * g;
            cs += x, gs += g;
            cq_lo += x2, cq_hi += cq_lo < x2;
            gq_lo += g2, gq_hi += gq_lo < g2;
        }
        keys[(uint64_t)(2u * k) * n_cells + j] = key0;
        keys[(uint64_t)(2u * k + 1u) * n_cells + j] = key1;
        if (counts_out) counts_out[row + j] = x;
        if (genes_out) genes_out[row + j] = g;
    }
    if (cs) atomicAdd(&s_m[0], cs);
    ms_add128(&s_m[1], &s_m[2], cq_hi, cq_lo);
    if (gs) atomicAdd(&s_m[3], gs);
    ms_add128(&s_m[4], &s_m[5], gq_hi, gq_lo);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long *o = mom + k * 6u;
        if (s_m[0]) atomicAdd(&o[0], s_m[0]);
        ms_add128(&o[1], &o[2], s_m[1], s_m[2]);
        if (s_m[3]) atomicAdd(&o[3], s_m[3]);
        ms_add128(&o[4], &o[5], s_m[4], s_m[5]);
    }
}

__global__ __launch_bounds__(256) void k_ms_gather(const uint64_t *__restrict__ sorted, const uint64_t *__restrict__ pos, uint32_t n, uint64_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sorted[pos[i]];
}

template <int NC>
static void ms_launch_pass(crgpu_ctx *ctx, bool lds, uint32_t grid, size_t dyn, const crgpu_matrix_dev *m, const uint8_t *fclass, uint32_t n_features,
                           uint32_t n_classes, const uint32_t *cellidx, const uint32_t *cellmask, uint64_t n_cells, uint32_t slice, uint32_t G,
                           uint2 *slab, unsigned long long *carry, unsigned long long *gsum, unsigned long long *gcnt, unsigned long long *cell_sum,
                           uint32_t *cell_genes, unsigned long long *tot, uint32_t *flag) {
    if (lds) {
        cr_allow_lds(ctx, (const void *)k_ms_pass<NC, true>, dyn);
        hipLaunchKernelGGL((k_ms_pass<NC, true>), dim3(grid), dim3(MS_WG), dyn, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data,
                           m->n_barcodes, fclass, n_features, n_classes, cellidx, cellmask, n_cells, slice, G, slab, carry, gsum, gcnt, cell_sum,
                           cell_genes, tot, flag);
    } else {
        hipLaunchKernelGGL((k_ms_pass<NC, false>), dim3(grid), dim3(MS_WG), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data,
                           m->n_barcodes, fclass, n_features, n_classes, cellidx, cellmask, n_cells, slice, G, slab, carry, gsum, gcnt, cell_sum,
                           cell_genes, tot, flag);
    }
}

// the `n_top` largest values among the features of class k: by value descending, then by feature index ascending
static void ms_top(const std::vector<uint64_t> &v, const std::vector<uint32_t> &feat, uint32_t n_top, uint32_t *feature_out, uint64_t *value_out) {
    std::vector<uint32_t> idx(feat);
    std::partial_sort(idx.begin(), idx.begin() + n_top, idx.end(), [&](uint32_t a, uint32_t b) { return v[a] != v[b] ? v[a] > v[b] : a < b; });
    for (uint32_t i = 0; i < n_top; i++) feature_out[i] = idx[i], value_out[i] = v[idx[i]];
}

extern "C" int crgpu_matrix_summary_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, uint32_t n_features, uint32_t n_classes, const uint8_t *feature_class,
                                        const uint64_t *d_cell_cols, uint64_t n_cells, const uint32_t *cell_class_mask,
                                        const uint32_t *d_reads_per_col, uint64_t *counts_per_feature_out, uint64_t *cells_ge2_per_feature_out,
                                        crgpu_matrix_summary_class *classes_out, uint64_t *reads_all_out, uint64_t *reads_union_out,
                                        uint32_t *d_counts_per_cell_out, uint32_t *d_genes_per_cell_out) {
    if (!ctx || !m) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, n_classes >= 1 && n_classes <= CRGPU_MS_MAX_CLASSES, CRGPU_EINVAL, "crgpu_matrix_summary_dev: 1 .. %d classes", CRGPU_MS_MAX_CLASSES);
    const uint64_t V = m->n_barcodes;
    CR_REQUIRE(ctx, V < 0xFFFFFFFFull, CRGPU_ERANGE, "crgpu_matrix_summary_dev: fewer than 2^32 - 1 columns");
    CR_REQUIRE(ctx, n_cells <= V && (d_cell_cols || !n_cells), CRGPU_EINVAL, "crgpu_matrix_summary_dev: the cell call does not fit the matrix");
    const uint32_t all_mask = n_classes == 32u ? 0xFFFFFFFFu : (1u << n_classes) - 1u;
    std::vector<uint64_t> cls_features(n_classes, 0), cls_cells(n_classes, 0);
    for (uint32_t f = 0; f < n_features; f++) {
        const uint32_t fc = feature_class ? feature_class[f] : 0u;
        CR_REQUIRE(ctx, fc < n_classes || fc == MS_NONE, CRGPU_EINVAL, "crgpu_matrix_summary_dev: feature_class[%u] = %u with %u classes", f, fc, n_classes);
        if (fc < n_classes) cls_features[fc]++;
    }
    std::vector<uint32_t> h_mask(n_cells ? n_cells : 1, all_mask);
    for (uint64_t j = 0; j < n_cells; j++) {
        if (cell_class_mask) h_mask[j] = cell_class_mask[j] & all_mask;
        for (uint32_t mk = h_mask[j]; mk; mk &= mk - 1u) cls_cells[__builtin_ctz(mk)]++;
    }
    if (counts_per_feature_out) memset(counts_per_feature_out, 0, n_features * sizeof(uint64_t));
    if (cells_ge2_per_feature_out) memset(cells_ge2_per_feature_out, 0, n_features * sizeof(uint64_t));
    if (reads_all_out) *reads_all_out = 0;
    if (reads_union_out) *reads_union_out = 0;
    if (classes_out) {
        memset(classes_out, 0, n_classes * sizeof(*classes_out));
        for (uint32_t k = 0; k < n_classes; k++) {
            classes_out[k].n_features_class = cls_features[k];
            classes_out[k].n_cells = cls_cells[k];
            classes_out[k].n_top = (uint32_t)std::min<uint64_t>(CRGPU_MS_TOP_N, cls_features[k]);
        }
    }
    if (V) {
        // ---- the tables of the pass ----
        DevBuf fc_b, idx_b, mask_b, tot_b, csum_b, cgen_b, fsum_b, fcnt_b, slab_b, carry_b;
        CR_TRY(dmalloc(ctx, fc_b, n_features ? n_features : 1));
        if (n_features) {
            if (feature_class) CR_TRY(crgpu_memcpy_h2d(ctx, fc_b.p, feature_class, n_features));
            else CR_HIP(ctx, hipMemsetAsync(fc_b.p, 0, n_features, ctx->stream));
        }
        CR_TRY(dmalloc(ctx, idx_b, V * sizeof(uint32_t)));
        CR_HIP(ctx, hipMemsetAsync(idx_b.p, 0, V * sizeof(uint32_t), ctx->stream));
        CR_TRY(dmalloc(ctx, mask_b, h_mask.size() * sizeof(uint32_t)));
        CR_TRY(crgpu_memcpy_h2d(ctx, mask_b.p, h_mask.data(), h_mask.size() * sizeof(uint32_t)));
        uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag[3] = {0, 0, 0};  // the list, the pass, the per-cell sums
        CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(flag), ctx->stream));
        cr_check_columns<true>(ctx, d_cell_cols, n_cells, V, MarkPlace{idx_b.as<uint32_t>()}, d_flag);
        CR_HIP(ctx, hipGetLastError());
        CR_TRY(read_u32(ctx, d_flag, &flag[0]));
        CR_TRY(cr_list_verdict(ctx, flag[0], "crgpu_matrix_summary_dev", "cell column"));
        const uint64_t n_pc = (uint64_t)n_classes * (n_cells ? n_cells : 1);
        const uint64_t nf1 = n_features ? n_features : 1;
        CR_TRY(dmalloc(ctx, tot_b, (MS_T_TOTAL + 2 + CRGPU_MS_MAX_CLASSES + 6 * CRGPU_MS_MAX_CLASSES) * sizeof(unsigned long long)));
        CR_HIP(ctx, hipMemsetAsync(tot_b.p, 0, (MS_T_TOTAL + 2 + CRGPU_MS_MAX_CLASSES + 6 * CRGPU_MS_MAX_CLASSES) * sizeof(unsigned long long), ctx->stream));
        unsigned long long *d_tot = tot_b.as<unsigned long long>(), *d_reads = d_tot + MS_T_TOTAL, *d_mom = d_reads + 2 + CRGPU_MS_MAX_CLASSES;
        CR_TRY(dmalloc(ctx, csum_b, n_pc * sizeof(unsigned long long)));
        CR_TRY(dmalloc(ctx, cgen_b, n_pc * sizeof(uint32_t)));
        CR_HIP(ctx, hipMemsetAsync(csum_b.p, 0, n_pc * sizeof(unsigned long long), ctx->stream));
        CR_HIP(ctx, hipMemsetAsync(cgen_b.p, 0, n_pc * sizeof(uint32_t), ctx->stream));
        CR_TRY(dmalloc(ctx, fsum_b, nf1 * sizeof(unsigned long long)));
        CR_TRY(dmalloc(ctx, fcnt_b, nf1 * sizeof(unsigned long long)));
        // ---- the pass ----
        const bool lds = ctx->ms_lds_features != 0u && n_features != 0u;
        uint32_t slice = 0, G = 0, grid = cr_grid(V * 64, MS_WG);
        size_t dyn = 0;
        if (lds) {
            slice = std::min(std::min(ctx->ms_lds_features, (uint32_t)MS_SLICE_MAX), n_features);
            const uint32_t n_slices = (n_features + slice - 1) / slice;
            dyn = (size_t)slice * 8 + ((slice + 3u) & ~3u);
            int n_cu = 0;
            if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n_cu < 1) n_cu = 256;
            // one workgroup of 1024 threads per CU, two where two slices fit its LDS: the slab stays at a few workgroups per CU
            const uint32_t per_cu = 2u * (dyn + MS_STATIC_BYTES) <= MS_LDS_BYTES ? 2u : 1u;
            G = std::max<uint32_t>(1u, std::min<uint64_t>((uint32_t)n_cu * per_cu / n_slices, (V + MS_WAVES - 1) / MS_WAVES));
            grid = n_slices * G;
            CR_TRY(dmalloc(ctx, slab_b, (uint64_t)G * n_features * sizeof(uint2)));
            CR_TRY(dmalloc(ctx, carry_b, nf1 * sizeof(unsigned long long)));
            CR_HIP(ctx, hipMemsetAsync(carry_b.p, 0, nf1 * sizeof(unsigned long long), ctx->stream));
        } else {
            CR_HIP(ctx, hipMemsetAsync(fsum_b.p, 0, nf1 * sizeof(unsigned long long), ctx->stream));
            CR_HIP(ctx, hipMemsetAsync(fcnt_b.p, 0, nf1 * sizeof(unsigned long long), ctx->stream));
        }
        {
            CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
            auto launch = n_classes == 1u ? ms_launch_pass<1> : n_classes <= 4u ? ms_launch_pass<4> : ms_launch_pass<CRGPU_MS_MAX_CLASSES>;
            launch(ctx, lds, grid, dyn, m, fc_b.as<uint8_t>(), n_features, n_classes, idx_b.as<uint32_t>(), mask_b.as<uint32_t>(), n_cells ? n_cells : 1, slice, G,
                   slab_b.as<uint2>(), carry_b.as<unsigned long long>(), fsum_b.as<unsigned long long>(), fcnt_b.as<unsigned long long>(),
                   csum_b.as<unsigned long long>(), cgen_b.as<uint32_t>(), d_tot, d_flag + 1);
            CR_HIP(ctx, hipGetLastError());
            if (lds) {
                hipLaunchKernelGGL(k_ms_slab_sum, dim3(cr_grid(n_features, 256)), dim3(256), 0, ctx->stream, slab_b.as<uint2>(), G, n_features,
                                   carry_b.as<unsigned long long>(), fsum_b.as<unsigned long long>(), fcnt_b.as<unsigned long long>());
                CR_HIP(ctx, hipGetLastError());
            }
            if (d_reads_per_col) {
                hipLaunchKernelGGL(k_ms_reads, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, d_reads_per_col, V, idx_b.as<uint32_t>(), mask_b.as<uint32_t>(), d_reads);
                CR_HIP(ctx, hipGetLastError());
            }
        }
        // ---- per cell: u32 values, moments, order statistics ----
        DevBuf key_b, keyt_b, pos_b, got_b;
        std::vector<uint64_t> h_pos, h_got;
        if (n_cells) {
            const uint64_t n_keys = 2ull * n_classes * n_cells;
            CR_TRY(dmalloc(ctx, key_b, n_keys * sizeof(uint64_t)));
            CR_TRY(dmalloc(ctx, keyt_b, n_keys * sizeof(uint64_t)));
            CrTimer t(ctx, CRGPU_T_MATRIX, n_keys);
            hipLaunchKernelGGL(k_ms_finish, dim3(cr_grid(n_cells, 256, 256), n_classes), dim3(256), 0, ctx->stream, csum_b.as<unsigned long long>(), cgen_b.as<uint32_t>(),
                               mask_b.as<uint32_t>(), n_cells, n_classes, key_b.as<uint64_t>(), d_counts_per_cell_out, d_genes_per_cell_out, d_mom, d_flag + 2);
            CR_HIP(ctx, hipGetLastError());
            bool in_tmp = false;
            CR_TRY(cr_radix_sort_u64(ctx, key_b.as<uint64_t>(), keyt_b.as<uint64_t>(), nullptr, nullptr, n_keys, 0, 32 + cr_ceil_log2(2ull * n_classes + 1), &in_tmp));
            // the six places of every (class, array): x[floor((n - 1) q)] and its right neighbour, q = 1/4, 2/4, 3/4
            uint64_t off = 0;
            for (uint32_t g = 0; g < 2u * n_classes; g++) {
                const uint64_t n = cls_cells[g / 2];
                for (uint64_t q = 1; n && q <= 3; q++) {
                    const uint64_t p = (n - 1) * q / 4;
                    h_pos.push_back(off + p);
                    h_pos.push_back(off + std::min(p + 1, n - 1));
                }
                off += n;
            }
            if (!h_pos.empty()) {
                h_got.resize(h_pos.size());
                CR_TRY(dmalloc(ctx, pos_b, h_pos.size() * sizeof(uint64_t)));
                CR_TRY(dmalloc(ctx, got_b, h_pos.size() * sizeof(uint64_t)));
                CR_TRY(crgpu_memcpy_h2d(ctx, pos_b.p, h_pos.data(), h_pos.size() * sizeof(uint64_t)));
                hipLaunchKernelGGL(k_ms_gather, dim3(cr_grid(h_pos.size(), 256)), dim3(256), 0, ctx->stream, in_tmp ? keyt_b.as<uint64_t>() : key_b.as<uint64_t>(),
                                   pos_b.as<uint64_t>(), (uint32_t)h_pos.size(), got_b.as<uint64_t>());
                CR_HIP(ctx, hipGetLastError());
                CR_TRY(crgpu_memcpy_d2h(ctx, h_got.data(), got_b.p, h_got.size() * sizeof(uint64_t)));  // (synchronises: h_pos was read)
            }
        }
        CR_TRY(crgpu_memcpy_d2h(ctx, flag, d_flag, sizeof(flag)));
        CR_REQUIRE(ctx, !flag[1], CRGPU_EINVAL, "crgpu_matrix_summary_dev: the matrix holds a row >= n_features (%u)", n_features);
        std::vector<uint64_t> h_tot(MS_T_TOTAL + 2 + CRGPU_MS_MAX_CLASSES + 6 * CRGPU_MS_MAX_CLASSES);
        static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
        CR_TRY(crgpu_memcpy_d2h(ctx, h_tot.data(), d_tot, h_tot.size() * sizeof(uint64_t)));
        CR_REQUIRE(ctx, h_tot[MS_T_SEEN] == m->nnz, CRGPU_EINVAL, "crgpu_matrix_summary_dev: the rows of a column do not ascend (%llu of %llu entries found)",
                   (unsigned long long)h_tot[MS_T_SEEN], (unsigned long long)m->nnz);
        CR_REQUIRE(ctx, !flag[2], CRGPU_ERANGE, "crgpu_matrix_summary_dev: a per-cell sum does not fit 32 bits");
        // ---- per feature: the sums, then host statistics over them ----
        std::vector<uint64_t> h_sum(n_features), h_cnt(n_features);
        if (n_features) {
            CR_TRY(crgpu_memcpy_d2h(ctx, h_sum.data(), fsum_b.p, n_features * sizeof(uint64_t)));
            CR_TRY(crgpu_memcpy_d2h(ctx, h_cnt.data(), fcnt_b.p, n_features * sizeof(uint64_t)));
            if (counts_per_feature_out) std::copy(h_sum.begin(), h_sum.end(), counts_per_feature_out);
            if (cells_ge2_per_feature_out) std::copy(h_cnt.begin(), h_cnt.end(), cells_ge2_per_feature_out);
        }
        if (reads_all_out) *reads_all_out = h_tot[MS_T_TOTAL];
        if (reads_union_out) *reads_union_out = h_tot[MS_T_TOTAL + 1];
        if (classes_out) {
            std::vector<std::vector<uint32_t>> feat(n_classes);
            for (uint32_t f = 0; f < n_features; f++) {
                const uint32_t fc = feature_class ? feature_class[f] : 0u;
                if (fc < n_classes) feat[fc].push_back(f);
            }
            size_t at = 0;
            for (uint32_t k = 0; k < n_classes; k++) {
                crgpu_matrix_summary_class &c = classes_out[k];
                const uint64_t *t = h_tot.data() + k * MS_T_WORDS, *mo = h_tot.data() + MS_T_TOTAL + 2 + CRGPU_MS_MAX_CLASSES + 6 * k;
                c.raw_total_counts = t[MS_T_RAW], c.union_total_counts = t[MS_T_UNION], c.union_nnz = t[MS_T_UNION_NNZ];
                c.cells_total_counts = t[MS_T_CELLS], c.cells_nnz = t[MS_T_CELLS_NNZ];
                c.reads_cells = h_tot[MS_T_TOTAL + 2 + k];
                c.counts_sum = mo[0], c.counts_sumsq_hi = mo[1], c.counts_sumsq_lo = mo[2];
                c.genes_sum = mo[3], c.genes_sumsq_hi = mo[4], c.genes_sumsq_lo = mo[5];
                for (uint32_t f : feat[k]) c.genes_detected += h_sum[f] != 0;
                ms_top(h_sum, feat[k], c.n_top, c.top_counts_feature, c.top_counts_value);
                ms_top(h_cnt, feat[k], c.n_top, c.top_cells_feature, c.top_cells_value);
                for (uint32_t which = 0; which < 2 && c.n_cells; which++) {
                    uint32_t *q = which ? c.genes_q : c.counts_q;
                    for (uint32_t i = 0; i < 6; i++, at++) {
                        CR_REQUIRE(ctx, (h_got[at] >> 32) == 2u * k + which, CRGPU_EHIP, "crgpu_matrix_summary_dev: the sorted per-cell keys are out of place");
                        q[i] = (uint32_t)h_got[at];
                    }
                }
            }
        }
    } else if (classes_out) {  // no column: every value is 0, the top features follow the tie rule as for a matrix without cells
        const std::vector<uint64_t> zero(n_features, 0);
        for (uint32_t k = 0; k < n_classes; k++) {
            std::vector<uint32_t> feat;
            for (uint32_t f = 0; f < n_features; f++)
                if ((feature_class ? feature_class[f] : 0u) == k) feat.push_back(f);
            crgpu_matrix_summary_class &c = classes_out[k];
            ms_top(zero, feat, c.n_top, c.top_counts_feature, c.top_counts_value);
            ms_top(zero, feat, c.n_top, c.top_cells_feature, c.top_cells_value);
        }
    }
    return CRGPU_OK;
}

// ---- the reads of every column -------------------------------------------------------------------------------------------------
struct MsReadTables {
    const uint32_t *t[2 * CRGPU_MAX_LIB];
    uint32_t n;
};
// flag bit 0: a sum above 2^32 - 1, bit 1: a rank outside the whitelist
__global__ __launch_bounds__(256) void k_ms_reads_per_column(const uint32_t *__restrict__ rank, uint64_t V, uint32_t n_canon, MsReadTables tabs,
                                                             uint32_t *__restrict__ out, uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < V; c += stride) {
        const uint32_t r = rank[c];
        unsigned long long s = 0;
        if (r >= n_canon) {
            atomicOr(flag, 2u);
        } else {
            for (uint32_t i = 0; i < tabs.n; i++) s += tabs.t[i][r];
            if (s > 0xFFFFFFFFull) atomicOr(flag, 1u);
        }
        out[c] = (uint32_t)s;
    }
}

extern "C" int crgpu_matrix_dev_reads_per_column(crgpu_ctx *ctx, const crgpu_matrix_dev *m, uint32_t lib_mask, uint32_t *d_out) {
    if (!ctx || !m) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, ctx->canon_set, CRGPU_ESTATE, "crgpu_matrix_dev_reads_per_column: no whitelist set");
    CR_REQUIRE(ctx, lib_mask != 0u, CRGPU_EINVAL, "crgpu_matrix_dev_reads_per_column: an empty library mask");
    MsReadTables tabs;
    tabs.n = 0;
    for (uint32_t l = 0; l < 32; l++) {
        if (!((lib_mask >> l) & 1u)) continue;
        CR_REQUIRE(ctx, l < CRGPU_MAX_LIB && ctx->wl[l].set && (!ctx->layout.set || l < ctx->layout.n_libs), CRGPU_EINVAL,
                   "crgpu_matrix_dev_reads_per_column: library %u has no whitelist or lies outside the key layout", l);
        tabs.t[tabs.n++] = ctx->wl[l].d_valid;
        tabs.t[tabs.n++] = ctx->wl[l].d_corrected;
    }
    const uint64_t V = m->n_barcodes;
    if (!V) return CRGPU_OK;
    CR_REQUIRE(ctx, d_out != nullptr, CRGPU_EINVAL, "crgpu_matrix_dev_reads_per_column: NULL output");
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, V);
        hipLaunchKernelGGL(k_ms_reads_per_column, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, m->d_barcode_rank, V, ctx->n_canon, tabs, d_out, d_flag);
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !(flag & 2u), CRGPU_EINVAL, "crgpu_matrix_dev_reads_per_column: a column's barcode rank is not on the whitelist");
    CR_REQUIRE(ctx, !(flag & 1u), CRGPU_ERANGE, "crgpu_matrix_dev_reads_per_column: a column's reads do not fit 32 bits");
    return CRGPU_OK;
}

// ---- the floats of _report (host, f64, unfused; no context) -----------------------------------------------------------------------
// np.percentile(x, 25 i) of n sorted values from x[floor((n - 1) i / 4)] = a and its right neighbour b: the fraction in integers
static inline double ms_percentile(uint64_t n, uint32_t i, uint32_t a, uint32_t b) {
    return cr_lerp((double)a, (double)b, (double)((n - 1) * i % 4) / 4.0);
}
static void ms_summarize(uint64_t n, uint64_t sum, uint64_t sq_hi, uint64_t sq_lo, const uint32_t *q, double *mean, double *median, double *cv, double *iqr,
                         double *stddev) {
    const double nan = std::nan("");
    *mean = *median = *cv = *iqr = *stddev = nan;
    if (!n) return;
    *mean = (double)sum / (double)n;
    *median = ms_percentile(n, 2, q[2], q[3]);
    *iqr = ms_percentile(n, 3, q[4], q[5]) - ms_percentile(n, 1, q[0], q[1]);
    const unsigned __int128 sq = ((unsigned __int128)sq_hi << 64) | sq_lo, s2 = (unsigned __int128)sum * sum;
    const unsigned __int128 num = (unsigned __int128)n * sq - s2;  // n sum(x^2) - (sum x)^2 >= 0, exact: n < 2^32, sum(x^2) < 2^96
    *stddev = std::sqrt((double)num / ((double)n * (double)n));
    *cv = cr_robust_divide(*stddev, *mean);
}

extern "C" int crgpu_matrix_summary_stats(const crgpu_matrix_summary_class *c, uint64_t reads_cells, uint64_t reads_all, crgpu_matrix_summary_floats *out) {
    if (!c || !out) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_matrix_summary_stats: NULL argument");
    if (c->n_cells > 0xFFFFFFFFull || c->counts_sumsq_hi > 0xFFFFFFFFull || c->genes_sumsq_hi > 0xFFFFFFFFull)
        return cr_fail(nullptr, CRGPU_ERANGE, "crgpu_matrix_summary_stats: more than 2^32 - 1 cells or a sum of squares of 96 bits or more");
    ms_summarize(c->n_cells, c->counts_sum, c->counts_sumsq_hi, c->counts_sumsq_lo, c->counts_q, &out->counts_mean, &out->counts_median, &out->counts_cv,
                 &out->counts_iqr, &out->counts_std);
    ms_summarize(c->n_cells, c->genes_sum, c->genes_sumsq_hi, c->genes_sumsq_lo, c->genes_q, &out->genes_mean, &out->genes_median, &out->genes_cv,
                 &out->genes_iqr, &out->genes_std);
    // (the products of the reference are Python integers, rounded once by float())
    out->density = cr_robust_divide((double)c->cells_nnz, (double)((unsigned __int128)c->n_features_class * c->n_cells));
    out->cum_frac = cr_robust_divide((double)c->cells_total_counts, (double)c->raw_total_counts);
    out->dupe_frac = 1.0 - cr_robust_divide((double)c->cells_total_counts, (double)reads_cells);
    out->reads_per_cell = cr_robust_divide((double)reads_cells, (double)c->n_cells);
    out->reads_cum_frac = cr_robust_divide((double)reads_cells, (double)reads_all);
    return CRGPU_OK;
}
