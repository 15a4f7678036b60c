// aggregates.h -- protein aggregates of an antibody / antigen well and the two closing cell filters on the device (part of
// matrix_stages.hip).
//
// Replaces remove_antibody_antigen_aggregates (lib/python/cellranger/cell_calling_helpers.py:188-270) with detect_aggregate_barcodes,
// detect_highly_corrected_bcs and detect_outlier_umis_bcs (cellranger/feature/antibody/analysis.py:77-185), which FILTER_BARCODES runs
// on the RAW matrix before the cell call, and apply_global_minimum_umis_threshold / apply_mitochondrial_threshold
// (lib/python/cellranger/cell_calling_helpers.py:671-785; called from the stage's __init__.py:551-575), which close it.
//
// The reference builds a dense barcodes x antibodies table and sorts every column of it.  A candidate only matters through its place
// from the top of a row, so here
//   1. k_ag_row_sums, one pass over all columns (a wave per column): per antibody row the sum and the entries >= 1, collected in the
//      workgroup's LDS; the rows of every column are checked (strictly ascending, < n_features) on the way.  The signal antibodies
//      (sum >= 1000) and the rows with fewer than K positive entries follow on the host.
//   2. the column sums over the signal rows (crgpu_matrix_dev_column_sums) and ONE radix sort of the keys (sum << column bits) | column: the
//      candidates are the last Kc = min(K, V) keys.  Every order in this file is the order of such pairs (value, column), ascending;
//      the top K are the K largest pairs: np.argsort(x, kind="stable")[-K:].
//   3. k_ag_gather (a wave per candidate) reads the candidates' Kc x n_signal counts, k_ag_sort_rows orders the pairs of every row
//      (a rank sort in LDS: Kc <= 1024).
//   4. k_ag_rank, ONE pass over the signal-antibody entries: workgroup (s, w) holds the sorted pairs of slice s of the signal rows and
//      one u32 counter per (row, place) in LDS and takes every G-th group of 16 columns.  Rows ascend inside a column, so a wave
//      narrows a long column to the features of its slice by a 64-ary search.  An entry >= 1 finds by binary search the number p of
//      the row's candidate pairs below its own pair and bumps counter p (an entry below the row's lowest candidate with a count is
//      not counted: that is nearly every entry of a well).  The counters are added to device memory at the end.  With 0 rows per
//      slice the pairs are read from and the counters bumped in device memory: the A/B of the slice form, and what a table that
//      does not fit ONE slice takes by default (several slices walk the columns once each; measured slower).
//   5. k_ag_decide: the entries above the candidate at place q of a row are the counters p > q.  A candidate whose count in the
//      row is ZERO ranks among the implicit zeros: above it are the row's nnz positive entries and the zeros of a higher column,
//      (V - 1 - col) - #{positive entries of the row with a column > col}.  That last count is only needed for a row with nnz < K
//      (otherwise nnz >= K decides); such rows bump a second set of counters by column (device memory: fewer than K entries each).
//      A candidate passes a row with fewer than K pairs above it; votes[j] = rows passed.
// Integer work throughout; the two thresholds are f64 on the host.
#pragma once

#include <algorithm>
#include <cmath>

#include "stage_common.h"

#define AG_NONE 0xFFFFFFFFu
#define AG_MAX_ANTIBODIES 4096u                      // rows whose sums a workgroup of pass 1 keeps in LDS (12 bytes each)
#define AG_MAX_K 1024u                               // candidates: 25 x at most 40 probe barcodes
#define AG_WG 1024u                                  // threads of a rank-pass workgroup: 16 waves, one column each
#define AG_WAVES (AG_WG / 64u)
#define AG_LDS_BYTES (160u * 1024u - 64u)
#define AG_SIGNAL_UMIS 1000ull                       // BACKGROUND_ANTIBODY_UMI_THRESHOLD
#define AG_TOP_UMI_BCS 25u                           // TOP_UMI_BCS
#define AG_ANTIGEN_TOP 100u
#define AG_ANTIGEN_MIN 1000.0

// ---- host: the two thresholds --------------------------------------------------------------------------------------------------
// int(np.round(n * _calculate_fraction_to_use(n))): f64, unfused, half to even
extern "C" int crgpu_aggregate_min_antibodies(uint32_t n_signal, uint32_t *out) {
    if (!out) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_aggregate_min_antibodies: NULL output");
    const double n = (double)n_signal;
    double frac = 0.6;
    if (n_signal <= 26u) {
        const double mn = -0.02 * n;
        frac = mn + 1.1;
    }
    const double prod = n * frac;
    *out = (uint32_t)std::nearbyint(prod);
    return CRGPU_OK;
}

extern "C" int crgpu_antigen_outlier_threshold(const uint32_t *top_counts, uint32_t n, double *q1_out, double *q3_out, double *threshold_out) {
    if (!top_counts || !n || !threshold_out) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_antigen_outlier_threshold: at least one count and an output");
    std::vector<uint32_t> x(top_counts, top_counts + n);
    std::sort(x.begin(), x.end());
    const double q3 = cr_quantile_sorted(x, 0.75), q1 = cr_quantile_sorted(x, 0.25);
    const double iqr = q3 - q1, spread = iqr * 3.0;
    if (q1_out) *q1_out = q1;
    if (q3_out) *q3_out = q3;
    *threshold_out = q3 + spread;
    return CRGPU_OK;
}

// ---- pass 1: the antibody rows' sums ---------------------------------------------------------------------------------------------
// flag bit 0: a row >= n_features, bit 1: the rows of a column do not ascend strictly
__global__ __launch_bounds__(256) void k_ag_row_sums(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                     const int32_t *__restrict__ data, uint64_t V, const uint32_t *__restrict__ abidx,
                                                     uint32_t n_features, uint32_t n_ab, unsigned long long *__restrict__ gsum,
                                                     uint32_t *__restrict__ gnnz, uint32_t *__restrict__ flag) {
    extern __shared__ unsigned long long s_ag_sum[];  // sum[n_ab], then u32 nnz[n_ab]
    uint32_t *s_nnz = (uint32_t *)(s_ag_sum + n_ab);
    for (uint32_t i = threadIdx.x; i < n_ab; i += 256) s_ag_sum[i] = 0ull, s_nnz[i] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    uint32_t bad = 0;
    for (uint64_t c = wave0; c < V; c += n_waves) {
        const long long s = indptr[c], e = indptr[c + 1];
        for (long long i = s + lane; i < e; i += 64) {
            const uint32_t f = (uint32_t)indices[i];
            if (i > s && (uint32_t)indices[i - 1] >= f) bad |= 2u;
            if (f >= n_features) {
                bad |= 1u;
                continue;
            }
            const uint32_t a = abidx[f];
            if (a == AG_NONE) continue;
            const uint32_t d = (uint32_t)data[i];
            if (!d) continue;
            atomicAdd(&s_ag_sum[a], (unsigned long long)d);
            atomicAdd(&s_nnz[a], 1u);
        }
    }
    if (bad) atomicOr(flag, bad);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_ab; i += 256) {
        if (s_ag_sum[i]) atomicAdd(&gsum[i], s_ag_sum[i]);
        if (s_nnz[i]) atomicAdd(&gnnz[i], s_nnz[i]);
    }
}

// ---- the candidates ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ag_pair_keys(const uint32_t *__restrict__ sums, uint64_t V, uint32_t col_bits, uint64_t *__restrict__ keys) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < V; c += stride) keys[c] = ((uint64_t)sums[c] << col_bits) | c;
}

// the n largest pairs (sum, column) of all columns -> host, ascending, as (sum << 32) | column.  One radix sort of the keys
// (sum << bits of a column) | column: 32 + ceil(log2 V) bits
static int ag_top_pairs(crgpu_ctx *ctx, const uint32_t *d_sums, uint64_t V, uint32_t n, std::vector<uint64_t> &top) {
    top.assign(n, 0);
    if (!n) return CRGPU_OK;
    const uint32_t col_bits = std::max(1u, cr_ceil_log2(V));
    DevBuf key_b, keyt_b;
    CR_TRY(dmalloc(ctx, key_b, V * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, keyt_b, V * sizeof(uint64_t)));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, V);
        hipLaunchKernelGGL(k_ag_pair_keys, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, d_sums, V, col_bits, key_b.as<uint64_t>());
        CR_HIP(ctx, hipGetLastError());
        bool in_tmp = false;
        CR_TRY(cr_radix_sort_u64(ctx, key_b.as<uint64_t>(), keyt_b.as<uint64_t>(), nullptr, nullptr, V, 0, 32 + col_bits, &in_tmp));
        CR_TRY(crgpu_memcpy_d2h(ctx, top.data(), (in_tmp ? keyt_b.as<uint64_t>() : key_b.as<uint64_t>()) + (V - n), (size_t)n * sizeof(uint64_t)));
    }
    for (uint64_t &k : top) k = ((k >> col_bits) << 32) | (k & ((1ull << col_bits) - 1ull));
    return CRGPU_OK;
}

// vals[s * Kc + j] = the count of signal row s in candidate j (the table is zeroed first); a wave per candidate
__global__ __launch_bounds__(256) void k_ag_gather(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                   const int32_t *__restrict__ data, const uint32_t *__restrict__ cand_cols, uint32_t Kc,
                                                   const uint32_t *__restrict__ sigidx, uint32_t *__restrict__ vals) {
    const uint32_t lane = threadIdx.x & 63u, j = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (j >= Kc) return;
    const uint32_t c = cand_cols[j];
    const long long s = indptr[c], e = indptr[c + 1];
    for (long long i = s + lane; i < e; i += 64) {
        const uint32_t r = sigidx[(uint32_t)indices[i]];  // rows < n_features: pass 1 checked
        if (r != AG_NONE) vals[(size_t)r * Kc + j] = (uint32_t)data[i];
    }
}

// one workgroup per signal row: keys[s][.] = the row's pairs (count << 32) | column ascending, place[s][j] = where candidate j went,
// zeros[s] (zeroed first) = its candidates with a count of zero
__global__ __launch_bounds__(256) void k_ag_sort_rows(const uint32_t *__restrict__ vals, const uint32_t *__restrict__ cand_cols, uint32_t Kc,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ place, uint32_t *__restrict__ zeros) {
    __shared__ uint64_t s_k[AG_MAX_K];
    const size_t row = (size_t)blockIdx.x * Kc;
    for (uint32_t j = threadIdx.x; j < Kc; j += 256) {
        const uint32_t v = vals[row + j];
        s_k[j] = ((uint64_t)v << 32) | cand_cols[j];
        if (!v) atomicAdd(&zeros[blockIdx.x], 1u);  // the row's candidates without a count: the first places of its order
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < Kc; j += 256) {
        const uint64_t k = s_k[j];
        uint32_t below = 0;
        for (uint32_t i = 0; i < Kc; i++) below += s_k[i] < k ? 1u : 0u;  // the columns differ: the pairs are distinct
        keys[row + below] = k;
        place[row + j] = below;
    }
}

// ---- pass 2: the place of every signal-antibody entry among the candidates of its row -------------------------------------------------
// LDS: workgroup blockIdx.x = s * G + w holds the signal rows [s * rows, min(n_signal, (s + 1) * rows)); bounds[2 s], bounds[2 s + 1]
// = the features of the first of them and one past the last.  !LDS: every workgroup takes all rows from device memory.
template <bool LDS>
__global__ __launch_bounds__(AG_WG) void k_ag_rank(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                   const int32_t *__restrict__ data, uint64_t V, const uint32_t *__restrict__ sigidx,
                                                   uint32_t n_features, uint32_t n_signal, uint32_t Kc, const uint64_t *__restrict__ keys,
                                                   const uint32_t *__restrict__ zeros, const uint8_t *__restrict__ sparse,
                                                   const uint32_t *__restrict__ cols_sorted, uint32_t rows,
                                                   uint32_t G, const uint32_t *__restrict__ bounds, uint32_t *__restrict__ cnt,
                                                   uint32_t *__restrict__ cnt2) {
    extern __shared__ uint64_t s_ag_keys[];  // LDS: u64 pairs[rows * Kc], then u32 counters[rows * (Kc + 1)]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t slice = LDS ? blockIdx.x / G : 0u, w = LDS ? blockIdx.x % G : blockIdx.x, n_wg = LDS ? G : gridDim.x;
    const uint32_t r0 = LDS ? slice * rows : 0u, r1 = LDS ? (n_signal - r0 < rows ? n_signal : r0 + rows) : n_signal;
    const uint32_t flo = bounds[2u * slice], fhi = bounds[2u * slice + 1u];
    const uint32_t K1 = Kc + 1u;
    uint32_t *s_cnt = (uint32_t *)(s_ag_keys + (size_t)rows * Kc);
    if (LDS) {
        for (uint32_t i = tid; i < (r1 - r0) * Kc; i += AG_WG) s_ag_keys[i] = keys[(size_t)r0 * Kc + i];
        for (uint32_t i = tid; i < (r1 - r0) * K1; i += AG_WG) s_cnt[i] = 0u;
        __syncthreads();
    }
    const uint64_t c_step = (uint64_t)n_wg * AG_WAVES;
    for (uint64_t c = (uint64_t)w * AG_WAVES + wave; c < V; c += c_step) {  // uniform in the wave
        long long b = indptr[c], e = indptr[c + 1];
        if (e - b > 64) {
            if (flo > 0u) b = wave_lower_bound(indices, b, e, flo, lane);
            if (fhi < n_features) e = wave_lower_bound(indices, b, e, fhi, lane);
        }
        for (long long i = b + lane; i < e; i += 64) {
            const uint32_t f = (uint32_t)indices[i], d = (uint32_t)data[i];
            if (f < flo || f >= fhi || !d) continue;  // a short column is not searched
            const uint32_t r = sigidx[f];
            if (r == AG_NONE || r < r0 || r >= r1) continue;
            const uint64_t key = ((uint64_t)d << 32) | (uint32_t)c;
            const uint64_t *k = LDS ? s_ag_keys + (size_t)(r - r0) * Kc : keys + (size_t)r * Kc;
            // the counters up to place z (the candidates without a count come first) are never read: such a candidate is decided by
            // the row's nnz and the column counters.  Nearly every entry of a well lies below the lowest counted candidate.
            const uint32_t z = zeros[r];
            if (z < Kc && key > k[z]) {
                const uint32_t p = z + 1u + cr_lower_bound(k + z + 1u, Kc - z - 1u, key);  // the pairs of the row below this entry
                atomicAdd(LDS ? &s_cnt[(r - r0) * K1 + p] : &cnt[(size_t)r * K1 + p], 1u);
            }
            if (sparse[r]) atomicAdd(&cnt2[(size_t)r * K1 + cr_lower_bound(cols_sorted, Kc, (uint32_t)c)], 1u);
        }
    }
    if (LDS) {
        __syncthreads();
        for (uint32_t i = tid; i < (r1 - r0) * K1; i += AG_WG)
            if (s_cnt[i]) atomicAdd(&cnt[(size_t)r0 * K1 + i], s_cnt[i]);
    }
}

// one workgroup per signal row; votes[j] += 1 when fewer than K pairs of the row lie above candidate j
__global__ __launch_bounds__(256) void k_ag_decide(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ place,
                                                   const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ cnt2,
                                                   const uint32_t *__restrict__ colrank, const uint32_t *__restrict__ nnz, uint64_t V, uint32_t K,
                                                   uint32_t Kc, uint32_t *__restrict__ votes) {
    const uint32_t r = blockIdx.x, K1 = Kc + 1u;
    for (uint32_t j = threadIdx.x; j < Kc; j += 256) {
        const uint32_t q = place[(size_t)r * Kc + j];
        const uint64_t key = keys[(size_t)r * Kc + q];
        unsigned long long above = 0;
        if (key >> 32) {
            for (uint32_t p = q + 1u; p <= Kc; p++) above += cnt[(size_t)r * K1 + p];
        } else {
            // a zero: every positive entry of the row, and the zeros of a higher column
            unsigned long long right = 0;  // positive entries of the row with a column beyond the candidate's
            for (uint32_t p = colrank[j] + 1u; p <= Kc; p++) right += cnt2[(size_t)r * K1 + p];
            above = (unsigned long long)nnz[r] + (V - 1ull - (uint32_t)key) - right;
        }
        if (above < K) atomicAdd(&votes[j], 1u);
    }
}

__global__ __launch_bounds__(256) void k_ag_mark(const uint64_t *__restrict__ cols, uint32_t n, uint64_t V, uint8_t bit, uint8_t *__restrict__ reason) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && cols[i] < V) reason[cols[i]] |= bit;  // the columns of a list differ: one writer per byte
}

// the listed columns (host, distinct) get `bit` in d_reason
static int ag_mark(crgpu_ctx *ctx, const std::vector<uint64_t> &cols, uint64_t V, uint8_t bit, uint8_t *d_reason) {
    if (cols.empty() || !d_reason) return CRGPU_OK;
    DevBuf b;
    CR_TRY(dmalloc(ctx, b, cols.size() * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, b.p, cols.data(), cols.size() * sizeof(uint64_t)));
    hipLaunchKernelGGL(k_ag_mark, dim3(cr_grid(cols.size(), 256)), dim3(256), 0, ctx->stream, b.as<uint64_t>(), (uint32_t)cols.size(), V, bit, d_reason);
    CR_HIP(ctx, hipGetLastError());
    return crgpu_synchronize(ctx);  // the list is a temporary of this call
}

static int ag_check_kinds(crgpu_ctx *ctx, const char *who, const crgpu_matrix_dev *m, const uint8_t *feature_kind, uint32_t n_features) {
    CR_REQUIRE(ctx, feature_kind || !n_features, CRGPU_EINVAL, "%s: NULL feature kinds", who);
    CR_REQUIRE(ctx, m->n_barcodes < 0xFFFFFFFFull, CRGPU_ERANGE, "%s: fewer than 2^32 - 1 columns", who);
    for (uint32_t f = 0; f < n_features; f++)
        CR_REQUIRE(ctx, feature_kind[f] <= CRGPU_AGG_KIND_ANTIGEN, CRGPU_EINVAL, "%s: feature_kind[%u] = %u", who, f, feature_kind[f]);
    return CRGPU_OK;
}

extern "C" int crgpu_aggregates_by_counts_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint8_t *feature_kind, uint32_t n_features,
                                              uint32_t num_probe_barcodes, uint8_t *d_reason_inout, uint64_t *cols_out, uint32_t cap,
                                              uint32_t *n_cols_out, crgpu_aggregates_info *info) {
    if (!ctx || !m || !n_cols_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *n_cols_out = 0;
    crgpu_aggregates_info nfo;
    memset(&nfo, 0, sizeof(nfo));
    if (info) *info = nfo;
    CR_TRY(ag_check_kinds(ctx, "crgpu_aggregates_by_counts_dev", m, feature_kind, n_features));
    const uint64_t npb = num_probe_barcodes ? num_probe_barcodes : 1u;
    CR_REQUIRE(ctx, npb * AG_TOP_UMI_BCS <= AG_MAX_K, CRGPU_ERANGE, "crgpu_aggregates_by_counts_dev: at most %u probe barcodes", AG_MAX_K / AG_TOP_UMI_BCS);
    const uint32_t K = (uint32_t)npb * AG_TOP_UMI_BCS;
    const uint64_t V = m->n_barcodes;
    std::vector<uint32_t> abidx(n_features ? n_features : 1, AG_NONE), ab_feature;
    for (uint32_t f = 0; f < n_features; f++)
        if (feature_kind[f] == CRGPU_AGG_KIND_ANTIBODY) abidx[f] = (uint32_t)ab_feature.size(), ab_feature.push_back(f);
    const uint32_t n_ab = (uint32_t)ab_feature.size();
    CR_REQUIRE(ctx, n_ab <= AG_MAX_ANTIBODIES, CRGPU_ERANGE, "crgpu_aggregates_by_counts_dev: %u antibody features, at most %u", n_ab, AG_MAX_ANTIBODIES);
    nfo.n_antibodies = n_ab, nfo.top_k = K;
    if (info) *info = nfo;
    if (!V) return CRGPU_OK;

    // 1. the antibody rows' sums (and the check of every column's rows)
    const uint32_t nab1 = n_ab ? n_ab : 1u;
    DevBuf idx_b, sum_b, nnz_b;
    CR_TRY(dmalloc(ctx, idx_b, abidx.size() * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, idx_b.p, abidx.data(), abidx.size() * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, sum_b, nab1 * sizeof(unsigned long long)));
    CR_TRY(dmalloc(ctx, nnz_b, nab1 * sizeof(uint32_t)));
    CR_HIP(ctx, hipMemsetAsync(sum_b.p, 0, nab1 * sizeof(unsigned long long), ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(nnz_b.p, 0, nab1 * sizeof(uint32_t), ctx->stream));
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
        const size_t dyn = (size_t)nab1 * 12;
        cr_allow_lds(ctx, (const void *)k_ag_row_sums, dyn);
        hipLaunchKernelGGL(k_ag_row_sums, dim3(cr_grid(V * 64, 256)), dim3(256), dyn, ctx->stream, (const long long *)m->d_indptr, m->d_indices,
                           m->d_data, V, idx_b.as<uint32_t>(), n_features, n_ab, sum_b.as<unsigned long long>(), nnz_b.as<uint32_t>(), d_flag);
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !(flag & 1u), CRGPU_EINVAL, "crgpu_aggregates_by_counts_dev: the matrix holds a row >= n_features (%u)", n_features);
    CR_REQUIRE(ctx, !(flag & 2u), CRGPU_EINVAL, "crgpu_aggregates_by_counts_dev: the rows of a column do not ascend");
    std::vector<uint64_t> h_sum(nab1);
    std::vector<uint32_t> h_nnz(nab1);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
    CR_TRY(crgpu_memcpy_d2h(ctx, h_sum.data(), sum_b.p, nab1 * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, h_nnz.data(), nnz_b.p, nab1 * sizeof(uint32_t)));
    std::vector<uint32_t> sigidx(abidx.size(), AG_NONE), sig_feature, sig_nnz;
    std::vector<uint8_t> mask(n_features ? n_features : 1, 0), sparse;
    for (uint32_t a = 0; a < n_ab; a++) {
        if (h_sum[a] < AG_SIGNAL_UMIS) continue;
        sigidx[ab_feature[a]] = (uint32_t)sig_feature.size();
        mask[ab_feature[a]] = 1;
        sig_feature.push_back(ab_feature[a]);
        sig_nnz.push_back(h_nnz[a]);
        sparse.push_back(h_nnz[a] < K);
    }
    const uint32_t n_signal = (uint32_t)sig_feature.size();
    nfo.n_signal = n_signal;
    CR_TRY(crgpu_aggregate_min_antibodies(n_signal, &nfo.min_antibodies));
    if (info) *info = nfo;
    if (n_signal < 5u) return CRGPU_OK;  // "cannot reliably differentiate low-order multiplets from aggregates"

    // 2. the candidates: the Kc columns with the largest sums over the signal rows
    const uint32_t Kc = (uint32_t)std::min<uint64_t>(K, V), K1 = Kc + 1u;
    nfo.n_candidates = Kc;
    std::vector<uint64_t> top;
    {
        DevBuf colsum_b;
        CR_TRY(dmalloc(ctx, colsum_b, V * sizeof(uint32_t)));
        CR_TRY(crgpu_matrix_dev_column_sums(ctx, m, mask.data(), n_features, colsum_b.as<uint32_t>()));
        CR_TRY(ag_top_pairs(ctx, colsum_b.as<uint32_t>(), V, Kc, top));
    }
    std::vector<uint32_t> cand(Kc), cols_sorted(Kc), colrank(Kc);
    for (uint32_t j = 0; j < Kc; j++) cand[j] = cols_sorted[j] = (uint32_t)top[j];
    std::sort(cols_sorted.begin(), cols_sorted.end());
    for (uint32_t j = 0; j < Kc; j++) colrank[j] = (uint32_t)(std::lower_bound(cols_sorted.begin(), cols_sorted.end(), cand[j]) - cols_sorted.begin());

    // 3. their counts in every signal row, ordered per row
    DevBuf sig_b, cand_b, csort_b, crank_b, snnz_b, sparse_b, vals_b, keys_b, place_b, cnt_b, votes_b, bounds_b, zeros_b;
    CR_TRY(dmalloc(ctx, sig_b, sigidx.size() * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, sig_b.p, sigidx.data(), sigidx.size() * sizeof(uint32_t)));
    for (auto pr : {std::make_pair(&cand_b, &cand), std::make_pair(&csort_b, &cols_sorted), std::make_pair(&crank_b, &colrank)}) {
        CR_TRY(dmalloc(ctx, *pr.first, Kc * sizeof(uint32_t)));
        CR_TRY(crgpu_memcpy_h2d(ctx, pr.first->p, pr.second->data(), Kc * sizeof(uint32_t)));
    }
    CR_TRY(dmalloc(ctx, snnz_b, n_signal * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, snnz_b.p, sig_nnz.data(), n_signal * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, sparse_b, n_signal));
    CR_TRY(crgpu_memcpy_h2d(ctx, sparse_b.p, sparse.data(), n_signal));
    const size_t n_tab = (size_t)n_signal * Kc, n_cnt = (size_t)n_signal * K1;
    CR_TRY(dmalloc(ctx, vals_b, n_tab * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, keys_b, n_tab * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, place_b, n_tab * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, cnt_b, 2 * n_cnt * sizeof(uint32_t)));  // by pair, then by column
    CR_TRY(dmalloc(ctx, votes_b, Kc * sizeof(uint32_t)));
    CR_HIP(ctx, hipMemsetAsync(vals_b.p, 0, n_tab * sizeof(uint32_t), ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(cnt_b.p, 0, 2 * n_cnt * sizeof(uint32_t), ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(votes_b.p, 0, Kc * sizeof(uint32_t), ctx->stream));
    CR_TRY(dmalloc(ctx, zeros_b, n_signal * sizeof(uint32_t)));
    CR_HIP(ctx, hipMemsetAsync(zeros_b.p, 0, n_signal * sizeof(uint32_t), ctx->stream));
    uint32_t *d_cnt = cnt_b.as<uint32_t>(), *d_cnt2 = d_cnt + n_cnt;
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, n_tab);
        hipLaunchKernelGGL(k_ag_gather, dim3(cr_grid((uint64_t)Kc * 64, 256)), dim3(256), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices,
                           m->d_data, cand_b.as<uint32_t>(), Kc, sig_b.as<uint32_t>(), vals_b.as<uint32_t>());
        hipLaunchKernelGGL(k_ag_sort_rows, dim3(n_signal), dim3(256), 0, ctx->stream, vals_b.as<uint32_t>(), cand_b.as<uint32_t>(), Kc,
                           keys_b.as<uint64_t>(), place_b.as<uint32_t>(), zeros_b.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
    }

    // 4. the rank pass: the rows in slices of the LDS, or everything in device memory
    const uint32_t row_bytes = Kc * 8u + K1 * 4u;
    // By default the LDS form is taken when ONE slice holds every row; several slices walk the columns once each and lose to the
    // device-memory form (profiles/aggregates_throughput.txt).  CRGPU_AGG_LDS_ROWS=<n> asks for slices of at most n rows.
    const uint32_t fit = AG_LDS_BYTES / row_bytes;
    const uint32_t rows = ctx->agg_lds_rows == 0xFFFFFFFFu ? (fit >= n_signal ? n_signal : 0u) : std::min(std::min(ctx->agg_lds_rows, fit), n_signal);
    const bool lds = rows != 0u;
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n_cu < 1) n_cu = 256;
    const uint64_t col_groups = (V + AG_WAVES - 1) / AG_WAVES;
    uint32_t n_slices = 1, G = 0, grid = 0;
    size_t dyn = 0;
    std::vector<uint32_t> bounds;
    if (lds) {
        n_slices = (n_signal + rows - 1) / rows;
        dyn = (size_t)rows * row_bytes;
        const uint32_t per_cu = 2u * dyn <= AG_LDS_BYTES ? 2u : 1u;  // one workgroup of 1024 threads per CU, two where two slices fit its LDS
        G = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)n_cu * per_cu / n_slices, col_groups));
        grid = n_slices * G;
        for (uint32_t s = 0; s < n_slices; s++) {
            bounds.push_back(sig_feature[s * rows]);
            bounds.push_back(sig_feature[std::min(n_signal, (s + 1) * rows) - 1] + 1u);
        }
    } else {
        grid = (uint32_t)std::min<uint64_t>((uint64_t)n_cu * 2, col_groups);
        bounds = {sig_feature.front(), sig_feature.back() + 1u};
    }
    CR_TRY(dmalloc(ctx, bounds_b, bounds.size() * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, bounds_b.p, bounds.data(), bounds.size() * sizeof(uint32_t)));
    nfo.n_slices = n_slices, nfo.rows_per_slice = rows, nfo.in_lds = lds;
    {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        CR_HIP(ctx, hipEventCreate(&e0));
        if (hipEventCreate(&e1) != hipSuccess) {
            (void)hipEventDestroy(e0);
            return cr_fail(ctx, CRGPU_EHIP, "crgpu_aggregates_by_counts_dev: no event");
        }
        (void)hipEventRecord(e0, ctx->stream);
        {
            CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
            if (lds) {
                cr_allow_lds(ctx, (const void *)k_ag_rank<true>, dyn);
                hipLaunchKernelGGL(k_ag_rank<true>, dim3(grid), dim3(AG_WG), dyn, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data, V,
                                   sig_b.as<uint32_t>(), n_features, n_signal, Kc, keys_b.as<uint64_t>(), zeros_b.as<uint32_t>(), sparse_b.as<uint8_t>(), csort_b.as<uint32_t>(),
                                   rows, G, bounds_b.as<uint32_t>(), d_cnt, d_cnt2);
            } else {
                hipLaunchKernelGGL(k_ag_rank<false>, dim3(grid), dim3(AG_WG), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data, V,
                                   sig_b.as<uint32_t>(), n_features, n_signal, Kc, keys_b.as<uint64_t>(), zeros_b.as<uint32_t>(), sparse_b.as<uint8_t>(), csort_b.as<uint32_t>(),
                                   rows, G, bounds_b.as<uint32_t>(), d_cnt, d_cnt2);
            }
        }
        (void)hipEventRecord(e1, ctx->stream);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        if (e != hipSuccess) return cr_fail(ctx, CRGPU_EHIP, "crgpu_aggregates_by_counts_dev: the rank pass failed: %s", hipGetErrorString(e));
        nfo.rank_ms = ms;
    }

    // 5. the votes
    hipLaunchKernelGGL(k_ag_decide, dim3(n_signal), dim3(256), 0, ctx->stream, keys_b.as<uint64_t>(), place_b.as<uint32_t>(), d_cnt, d_cnt2,
                       crank_b.as<uint32_t>(), snnz_b.as<uint32_t>(), V, K, Kc, votes_b.as<uint32_t>());
    CR_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> votes(Kc);
    CR_TRY(crgpu_memcpy_d2h(ctx, votes.data(), votes_b.p, Kc * sizeof(uint32_t)));
    std::vector<uint64_t> found;
    for (uint32_t j = 0; j < Kc; j++)
        if (votes[j] >= nfo.min_antibodies) found.push_back(cand[j]);
    std::sort(found.begin(), found.end());
    nfo.n_aggregates = (uint32_t)found.size();
    if (info) *info = nfo;
    *n_cols_out = nfo.n_aggregates;
    CR_REQUIRE(ctx, !cols_out || found.size() <= cap, CRGPU_ERANGE, "crgpu_aggregates_by_counts_dev: %zu columns, room for %u", found.size(), cap);
    if (cols_out) std::copy(found.begin(), found.end(), cols_out);
    return ag_mark(ctx, found, V, CRGPU_AGG_COUNTS, d_reason_inout);
}

// ---- highly corrected barcodes ------------------------------------------------------------------------------------------------------
// corrected / reads > 0.5 in f64 is 2 * corrected > reads in integers for reads < 2^50: the quotient of two integers below 2^53 is
// rounded once; it is monotone in the exact quotient, and 0.5 is a f64, so a quotient above (at or below) 1/2 rounds to a value >=
// (<=) 0.5; it can only round TO 0.5 from above when it lies within 2^-54 of it, but the exact distance (2 corrected - reads) /
// (2 reads) is at least 1 / (2 reads) > 2^-51.
__global__ __launch_bounds__(256) void k_ag_highly_corrected(const uint32_t *__restrict__ reads, const uint32_t *__restrict__ corrected, uint64_t V,
                                                             uint8_t *__restrict__ reason, uint32_t *__restrict__ n_found) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < V; c += stride) {
        const uint64_t r = reads[c], k = corrected[c];
        if (r > 10000ull && 2ull * k > r) {  // NUM_READS_THRESHOLD, HIGH_UMI_CORRECTION_THRESHOLD
            reason[c] |= CRGPU_AGG_HIGHLY_CORRECTED;
            atomicAdd(n_found, 1u);
        }
    }
}

extern "C" int crgpu_aggregates_highly_corrected_dev(crgpu_ctx *ctx, const uint32_t *d_reads, const uint32_t *d_corrected_reads, uint64_t V,
                                                     uint8_t *d_reason_inout, uint64_t *n_found_out) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    if (n_found_out) *n_found_out = 0;
    if (!V) return CRGPU_OK;
    CR_REQUIRE(ctx, d_reads && d_corrected_reads && d_reason_inout, CRGPU_EINVAL, "crgpu_aggregates_highly_corrected_dev: NULL argument");
    uint32_t *d_n = ctx->d_scalars + CR_SCALAR_FLAG, n = 0;
    CR_HIP(ctx, hipMemsetAsync(d_n, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_ag_highly_corrected, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, d_reads, d_corrected_reads, V, d_reason_inout, d_n);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_n, &n));
    if (n_found_out) *n_found_out = n;
    return CRGPU_OK;
}

// the umi_corrected_reads of every column, the masked libraries added up (the counterpart of crgpu_matrix_dev_reads_per_column)
// flag bit 0: a sum above 2^32 - 1, bit 1: a rank outside the whitelist
__global__ __launch_bounds__(256) void k_ag_corrected_per_column(const uint32_t *__restrict__ rank, uint64_t V, uint32_t n_canon,
                                                                 const uint32_t *__restrict__ corr, uint32_t lib_mask, uint32_t *__restrict__ out,
                                                                 uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < V; c += stride) {
        const uint32_t r = rank[c];
        unsigned long long s = 0;
        if (r >= n_canon) {
            atomicOr(flag, 2u);
        } else if (corr) {
            for (uint32_t mk = lib_mask; mk; mk &= mk - 1u) s += corr[(size_t)__builtin_ctz(mk) * n_canon + r];
            if (s > 0xFFFFFFFFull) atomicOr(flag, 1u);
        }
        out[c] = (uint32_t)s;
    }
}

extern "C" int crgpu_counts_corrected_reads_per_column(crgpu_ctx *ctx, const crgpu_counts *c, const crgpu_matrix_dev *m, uint32_t lib_mask,
                                                       uint32_t *d_out) {
    if (!ctx || !c || !m) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const char *who = "crgpu_counts_corrected_reads_per_column";
    CR_REQUIRE(ctx, ctx->canon_set, CRGPU_ESTATE, "%s: no whitelist set", who);
    CR_REQUIRE(ctx, c->n_canon == ctx->n_canon, CRGPU_ESTATE, "%s: the whitelist changed since the counts were made", who);
    CR_REQUIRE(ctx, c->n_molecules == 0 || c->d_corr_reads, CRGPU_ESTATE,
               "%s: these counts carry no corrected-read table (crgpu_enable_barcode_summary before crgpu_count_keys_dev, or use crgpu_count_records_dev)", who);
    const uint32_t slots = 1u << c->layout.bits_lib;
    CR_REQUIRE(ctx, lib_mask != 0u && (slots >= 32u || !(lib_mask >> slots)), CRGPU_EINVAL, "%s: the library mask is empty or names a library beyond the %u of the key layout",
               who, slots);
    const uint64_t V = m->n_barcodes;
    if (!V) return CRGPU_OK;
    CR_REQUIRE(ctx, d_out != nullptr, CRGPU_EINVAL, "%s: NULL output", who);
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, V);
        hipLaunchKernelGGL(k_ag_corrected_per_column, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, m->d_barcode_rank, V, ctx->n_canon,
                           (const uint32_t *)c->d_corr_reads, lib_mask, d_out, d_flag);
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !(flag & 2u), CRGPU_EINVAL, "%s: a column's barcode rank is not on the whitelist", who);
    CR_REQUIRE(ctx, !(flag & 1u), CRGPU_ERANGE, "%s: a column's corrected reads do not fit 32 bits", who);
    return CRGPU_OK;
}

// ---- antigen outliers ----------------------------------------------------------------------------------------------------------------
extern "C" int crgpu_aggregates_antigen_outliers_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint8_t *feature_kind, uint32_t n_features,
                                                     uint8_t *d_reason_inout, uint64_t *cols_out, uint32_t cap, uint32_t *n_cols_out,
                                                     double *threshold_out) {
    if (!ctx || !m || !n_cols_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *n_cols_out = 0;
    if (threshold_out) *threshold_out = std::nan("");
    CR_TRY(ag_check_kinds(ctx, "crgpu_aggregates_antigen_outliers_dev", m, feature_kind, n_features));
    const uint64_t V = m->n_barcodes;
    if (!V) return CRGPU_OK;
    std::vector<uint8_t> mask(n_features ? n_features : 1, 0);
    for (uint32_t f = 0; f < n_features; f++) mask[f] = feature_kind[f] == CRGPU_AGG_KIND_ANTIGEN;
    const uint32_t n = (uint32_t)std::min<uint64_t>(AG_ANTIGEN_TOP, V);
    std::vector<uint64_t> top;
    {
        DevBuf colsum_b;
        CR_TRY(dmalloc(ctx, colsum_b, V * sizeof(uint32_t)));
        CR_TRY(crgpu_matrix_dev_column_sums(ctx, m, mask.data(), n_features, colsum_b.as<uint32_t>()));
        CR_TRY(ag_top_pairs(ctx, colsum_b.as<uint32_t>(), V, n, top));
    }
    std::vector<uint32_t> x(n);
    for (uint32_t i = 0; i < n; i++) x[i] = (uint32_t)(top[i] >> 32);
    double threshold = 0.0;
    CR_TRY(crgpu_antigen_outlier_threshold(x.data(), n, nullptr, nullptr, &threshold));
    if (threshold_out) *threshold_out = threshold;
    if (threshold < AG_ANTIGEN_MIN) return CRGPU_OK;  // "min cutoff=1000 umis to be labeled as aggregate"
    std::vector<uint64_t> found;
    for (uint32_t i = 0; i < n; i++)
        if ((double)x[i] >= threshold) found.push_back((uint32_t)top[i]);
    std::sort(found.begin(), found.end());
    *n_cols_out = (uint32_t)found.size();
    CR_REQUIRE(ctx, !cols_out || found.size() <= cap, CRGPU_ERANGE, "crgpu_aggregates_antigen_outliers_dev: %zu columns, room for %u", found.size(), cap);
    if (cols_out) std::copy(found.begin(), found.end(), cols_out);
    return ag_mark(ctx, found, V, CRGPU_AGG_ANTIGEN, d_reason_inout);
}

// ---- the union: removed and kept columns ----------------------------------------------------------------------------------------------
struct AgReasonFlag {
    const uint8_t *reason;
    bool removed;
    __device__ __forceinline__ bool operator()(uint64_t c) const { return (reason[c] != 0) == removed; }
};
struct AgColEmit {
    uint64_t *out;
    struct Pre {};
    __device__ __forceinline__ Pre pre(uint64_t) const { return Pre(); }
    __device__ __forceinline__ void operator()(uint64_t c, uint32_t o, Pre) const { out[o] = c; }
};

// a pool block with the columns c in [0, V) that flag(c) keeps, ascending (the caller's, released with crgpu_free)
template <typename Flag>
static int ag_list(crgpu_ctx *ctx, Flag flag, uint64_t V, uint64_t **d_out, uint64_t *n_out) {
    uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL, n = 0;
    DevBuf tmp;
    CR_TRY(dmalloc(ctx, tmp, (V ? V : 1) * sizeof(uint64_t)));
    if (V) {
        CR_TRY(compact(ctx, flag, AgColEmit{tmp.as<uint64_t>()}, V, ctx->d_sort_hist, d_total));
        CR_TRY(read_u32(ctx, d_total, &n));
    }
    uint64_t *d = nullptr;
    CR_TRY(cr_pool_alloc(ctx, (void **)&d, (n ? n : 1) * sizeof(uint64_t)));
    hipError_t e = n ? hipMemcpyAsync(d, tmp.p, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        cr_pool_free(ctx, d);
        return cr_fail(ctx, CRGPU_EHIP, "column list: %s", hipGetErrorString(e));
    }
    *d_out = d;
    *n_out = n;
    return CRGPU_OK;
}

extern "C" int crgpu_aggregates_partition_dev(crgpu_ctx *ctx, const uint8_t *d_reason, uint64_t V, uint64_t **d_kept_cols_out, uint64_t *n_kept_out,
                                              uint64_t **d_removed_cols_out, uint64_t *n_removed_out) {
    if (!ctx || !d_kept_cols_out || !n_kept_out || !d_removed_cols_out || !n_removed_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *d_kept_cols_out = *d_removed_cols_out = nullptr;
    *n_kept_out = *n_removed_out = 0;
    CR_REQUIRE(ctx, d_reason || !V, CRGPU_EINVAL, "crgpu_aggregates_partition_dev: NULL reasons");
    CR_REQUIRE(ctx, V < 0xFFFFFFFFull, CRGPU_ERANGE, "crgpu_aggregates_partition_dev: fewer than 2^32 - 1 columns");
    CR_TRY(ag_list(ctx, AgReasonFlag{d_reason, false}, V, d_kept_cols_out, n_kept_out));
    const int rc = ag_list(ctx, AgReasonFlag{d_reason, true}, V, d_removed_cols_out, n_removed_out);
    if (rc != CRGPU_OK) {
        cr_pool_free(ctx, *d_kept_cols_out);
        *d_kept_cols_out = nullptr;
        *n_kept_out = 0;
    }
    return rc;
}

// out[i] = src[cols[i]] (elements of 1 or 4 bytes); flag: a column >= V
template <typename T>
__global__ __launch_bounds__(256) void k_ag_take(const T *__restrict__ src, uint64_t V, const uint64_t *__restrict__ cols, uint64_t n, T *__restrict__ out,
                                                 uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t c = cols[i];
        if (c < V) out[i] = src[c]; else atomicOr(flag, 1u);
    }
}

extern "C" int crgpu_take_columns_dev(crgpu_ctx *ctx, const void *d_src, uint32_t elem_bytes, uint64_t V, const uint64_t *d_cols, uint64_t n,
                                      void *d_out) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, elem_bytes == 1u || elem_bytes == 4u, CRGPU_EINVAL, "crgpu_take_columns_dev: elements of 1 or 4 bytes");
    if (!n) return CRGPU_OK;
    CR_REQUIRE(ctx, d_src && d_cols && d_out, CRGPU_EINVAL, "crgpu_take_columns_dev: NULL argument");
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    if (elem_bytes == 1u)
        hipLaunchKernelGGL(k_ag_take<uint8_t>, dim3(cr_grid(n, 256)), dim3(256), 0, ctx->stream, (const uint8_t *)d_src, V, d_cols, n, (uint8_t *)d_out, d_flag);
    else
        hipLaunchKernelGGL(k_ag_take<uint32_t>, dim3(cr_grid(n, 256)), dim3(256), 0, ctx->stream, (const uint32_t *)d_src, V, d_cols, n, (uint32_t *)d_out, d_flag);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !flag, CRGPU_EINVAL, "crgpu_take_columns_dev: a column is out of range");
    return CRGPU_OK;
}

__global__ __launch_bounds__(256) void k_ag_sum_u32(const uint32_t *__restrict__ x, uint64_t n, unsigned long long *__restrict__ out) {
    unsigned long long s = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) s += x[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(out, s);
}

extern "C" int crgpu_sum_u32_dev(crgpu_ctx *ctx, const uint32_t *d_values, uint64_t n, uint64_t *sum_out) {
    if (!ctx || !sum_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *sum_out = 0;
    if (!n) return CRGPU_OK;
    CR_REQUIRE(ctx, d_values != nullptr, CRGPU_EINVAL, "crgpu_sum_u32_dev: NULL values");
    DevBuf b;
    CR_TRY(dmalloc(ctx, b, sizeof(unsigned long long)));
    CR_HIP(ctx, hipMemsetAsync(b.p, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_ag_sum_u32, dim3(cr_grid(n, 256)), dim3(256), 0, ctx->stream, d_values, n, b.as<unsigned long long>());
    CR_HIP(ctx, hipGetLastError());
    return crgpu_memcpy_d2h(ctx, sum_out, b.p, sizeof(uint64_t));
}

// ---- the closing filters of a cell call ------------------------------------------------------------------------------------------------
// cell k of the list stays (keep) or leaves (!keep): the ONE compaction of both filters, the order of the list preserved
struct AgCellFlag {
    const uint64_t *cols;
    const uint32_t *total, *part;  // per column of the matrix; part == NULL: the minimum-UMI filter
    unsigned long long minimum;
    double max_pct;
    bool keep;
    __device__ __forceinline__ bool stays(uint64_t k) const {
        const uint64_t c = cols[k];
        if (!part) return (unsigned long long)total[c] >= minimum;
        const double pct = 100.0 * (double)part[c] / (double)total[c];  // 0 / 0 = NaN: not above the threshold, the cell stays
        return !(pct > max_pct);
    }
    __device__ __forceinline__ bool operator()(uint64_t k) const { return stays(k) == keep; }
};
struct AgCellEmit {
    const uint64_t *cols;
    uint64_t *out;
    struct Pre {
        uint64_t c;
    };
    __device__ __forceinline__ Pre pre(uint64_t k) const { return Pre{cols[k]}; }
    __device__ __forceinline__ void operator()(uint64_t, uint32_t o, Pre p) const { out[o] = p.c; }
};

static int ag_filter_cells(crgpu_ctx *ctx, const char *who, AgCellFlag flag, uint64_t V, uint64_t n_cells, uint64_t **d_kept, uint64_t *n_kept,
                           uint64_t **d_removed, uint64_t *n_removed) {
    *d_kept = nullptr, *n_kept = 0;
    if (d_removed) *d_removed = nullptr, *n_removed = 0;
    CR_REQUIRE(ctx, flag.total || !n_cells, CRGPU_EINVAL, "%s: NULL counts", who);
    CR_REQUIRE(ctx, n_cells <= V && (flag.cols || !n_cells), CRGPU_EINVAL, "%s: the cell call does not fit the %llu columns", who, (unsigned long long)V);
    CR_REQUIRE(ctx, V < 0xFFFFFFFFull, CRGPU_ERANGE, "%s: fewer than 2^32 - 1 columns", who);
    uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL, *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, bad = 0;
    if (n_cells) {  // the list: in range, strictly ascending
        CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
        cr_check_columns<true>(ctx, flag.cols, n_cells, V, MarkNone{}, d_flag);
        CR_HIP(ctx, hipGetLastError());
        CR_TRY(read_u32(ctx, d_flag, &bad));
        CR_TRY(cr_list_verdict(ctx, bad, who, "cell column"));
    }
    for (int pass = 0; pass < (d_removed ? 2 : 1); pass++) {
        flag.keep = pass == 0;
        uint64_t *d = nullptr;
        uint32_t n = 0;
        int rc = cr_pool_alloc(ctx, (void **)&d, (n_cells ? n_cells : 1) * sizeof(uint64_t));
        if (rc == CRGPU_OK && n_cells) {
            rc = compact(ctx, flag, AgCellEmit{flag.cols, d}, n_cells, ctx->d_sort_hist, d_total);
            if (rc == CRGPU_OK) rc = read_u32(ctx, d_total, &n);
        }
        if (rc != CRGPU_OK) {
            cr_pool_free(ctx, d);
            if (pass) cr_pool_free(ctx, *d_kept), *d_kept = nullptr, *n_kept = 0;
            return rc;
        }
        if (pass) *d_removed = d, *n_removed = n; else *d_kept = d, *n_kept = n;
    }
    return CRGPU_OK;
}

extern "C" int crgpu_filter_cells_min_umis_dev(crgpu_ctx *ctx, const uint32_t *d_umis_per_col, uint64_t V, const uint64_t *d_cell_cols,
                                               uint64_t n_cells, uint64_t minimum_umis, uint64_t **d_kept_cols_out, uint64_t *n_kept_out) {
    if (!ctx || !d_kept_cols_out || !n_kept_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    return ag_filter_cells(ctx, "crgpu_filter_cells_min_umis_dev", AgCellFlag{d_cell_cols, d_umis_per_col, nullptr, minimum_umis, 0.0, true}, V, n_cells,
                           d_kept_cols_out, n_kept_out, nullptr, nullptr);
}

extern "C" int crgpu_filter_cells_mito_dev(crgpu_ctx *ctx, const uint32_t *d_mito_umis_per_col, const uint32_t *d_total_umis_per_col, uint64_t V,
                                           const uint64_t *d_cell_cols, uint64_t n_cells, double max_mito_percent, uint64_t **d_kept_cols_out,
                                           uint64_t *n_kept_out, uint64_t **d_removed_cols_out, uint64_t *n_removed_out) {
    if (!ctx || !d_kept_cols_out || !n_kept_out || !d_removed_cols_out || !n_removed_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, d_mito_umis_per_col || !n_cells, CRGPU_EINVAL, "crgpu_filter_cells_mito_dev: NULL counts");
    CR_REQUIRE(ctx, max_mito_percent == max_mito_percent, CRGPU_EINVAL, "crgpu_filter_cells_mito_dev: the threshold is NaN");
    return ag_filter_cells(ctx, "crgpu_filter_cells_mito_dev", AgCellFlag{d_cell_cols, d_total_umis_per_col, d_mito_umis_per_col, 0ull, max_mito_percent, true},
                           V, n_cells, d_kept_cols_out, n_kept_out, d_removed_cols_out, n_removed_out);
}
