// graph_common.h -- what the stages on the kNN graph (tsne.hip, umap.hip, louvain.hip) share on top of stage_common.h: the path from
// pair keys i * n + j to a CSR (the keys of a neighbour list, the sort, the merge of the runs of equal keys, indptr by search), the
// ordered column sum, and the host checks of a caller's neighbour lists and of a caller's CSR.  As in stage_common.h a kernel defined
// here is a template: the header is part of several units.  The kernels and the run-head flag also sit in an unnamed namespace, so that
// every unit compiles, registers and launches its own copy, as it did when each wrote its own: one shared definition would be served
// by the code object of whichever unit registered it first, and that code object is loaded on first use (0.7 ms on the first
// affinities call of a process, measured).
#pragma once

#include <algorithm>
#include <vector>

#include "stage_common.h"

#define GRAPH_WG 256u
#define GRAPH_PART_ROWS 256u  // rows of a partial of the ordered column sum: fixed, no seam moves it

namespace {
// ---- pair keys to a CSR --------------------------------------------------------------------------------------------------------------
// two keys per neighbour pair of a list of n rows and k columns, i * n + j and j * n + i, and the identity permutation: the pair's
// number is the payload >> 1
template <typename P>
__global__ __launch_bounds__(GRAPH_WG) void k_pair_keys(const int32_t *__restrict__ nn, uint32_t n, uint32_t k, uint64_t *__restrict__ keys,
                                                        P *__restrict__ perm) {
    const uint64_t total = (uint64_t)n * k;
    for (uint64_t e = (uint64_t)blockIdx.x * GRAPH_WG + threadIdx.x; e < total; e += (uint64_t)gridDim.x * GRAPH_WG) {
        const uint64_t i = e / k, j = (uint64_t)(uint32_t)nn[e];
        keys[2 * e] = i * n + j, keys[2 * e + 1] = j * n + i;
        perm[2 * e] = (P)(2 * e), perm[2 * e + 1] = (P)(2 * e + 1);
    }
}
static inline void cr_pair_keys(crgpu_ctx *ctx, const int32_t *d_nn, uint32_t n, uint32_t k, uint64_t *d_keys, uint32_t *d_perm) {
    hipLaunchKernelGGL(k_pair_keys<uint32_t>, dim3(cr_grid((uint64_t)n * k, GRAPH_WG)), dim3(GRAPH_WG), 0, ctx->stream, d_nn, n, k, d_keys, d_perm);
}
struct KeyHeadFlag {  // the first of a run of equal keys
    const uint64_t *keys;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return (i == 0) | (keys[i] != keys[i ? i - 1 : 0]); }
};
// the CSR of sorted distinct keys i * n + j; weights (or NULL) = 1
template <typename W>
__global__ __launch_bounds__(GRAPH_WG) void k_keys_to_csr(const uint64_t *__restrict__ ckeys, uint64_t nnz, uint32_t n, long long *__restrict__ indptr,
                                                          int32_t *__restrict__ indices, W *__restrict__ weights) {
    const uint64_t stride = (uint64_t)gridDim.x * GRAPH_WG, t0 = (uint64_t)blockIdx.x * GRAPH_WG + threadIdx.x;
    for (uint64_t r = t0; r <= n; r += stride) indptr[r] = (long long)cr_lower_bound(ckeys, nnz, r * (uint64_t)n);
    for (uint64_t e = t0; e < nnz; e += stride) {
        indices[e] = (int32_t)(ckeys[e] % n);
        if (weights) weights[e] = 1u;
    }
}
static inline void cr_keys_to_csr(crgpu_ctx *ctx, const uint64_t *d_ckeys, uint64_t nnz, uint32_t n, long long *d_indptr, int32_t *d_indices,
                                  uint32_t *d_weights) {
    hipLaunchKernelGGL(k_keys_to_csr<uint32_t>, dim3(cr_grid(std::max<uint64_t>(nnz, (uint64_t)n + 1u), GRAPH_WG)), dim3(GRAPH_WG), 0, ctx->stream, d_ckeys,
                       nnz, n, d_indptr, d_indices, d_weights);
}

// The library's radix sort of `count` keys of `bits` bits with their payload (perm and perm_tmp, or both NULL) and the buffers it ended in
struct SortedKeys {
    const uint64_t *keys;
    const uint32_t *perm;
    uint64_t *spare;  // the key buffer the sort did not end in
};
static int cr_sort_keys(crgpu_ctx *ctx, uint64_t *d_keys, uint64_t *d_tmp, uint32_t *d_perm, uint32_t *d_perm_tmp, uint64_t count, uint32_t bits,
                        SortedKeys *out) {
    bool in_tmp = false;
    CR_TRY(cr_radix_sort_u64(ctx, d_keys, d_tmp, d_perm, d_perm_tmp, count, 0, std::max(1u, bits), &in_tmp));
    out->keys = in_tmp ? d_tmp : d_keys, out->perm = in_tmp ? d_perm_tmp : d_perm, out->spare = in_tmp ? d_keys : d_tmp;
    return CRGPU_OK;
}
// One emit per run of equal sorted keys (the stage's own functor, called at the run's head), *runs = their number, lo <= *runs <= hi or
// CRGPU_EHIP.  d_block: workspace of 4097 u32
template <typename Emit>
static int cr_merge_runs(crgpu_ctx *ctx, const uint64_t *d_sorted, Emit emit, uint64_t count, uint32_t *d_block, uint64_t lo, uint64_t hi, const char *who,
                         const char *what, uint32_t *runs) {
    CR_TRY(compact(ctx, KeyHeadFlag{d_sorted}, emit, count, d_block, d_block + 4096));
    CR_TRY(read_u32(ctx, d_block + 4096, runs));
    CR_REQUIRE(ctx, *runs >= lo && *runs <= hi, CRGPU_EHIP, "%s: %u %s of %llu keys, %llu to %llu", who, *runs, what, (unsigned long long)count,
               (unsigned long long)lo, (unsigned long long)hi);
    return CRGPU_OK;
}

// ---- the ordered column sum ----------------------------------------------------------------------------------------------------------
// parts[part * ncols + c] = a[r * ld + c] over the rows r of the partial, left to right from 0.0
template <typename T>
__global__ __launch_bounds__(GRAPH_WG) void k_colparts(const T *__restrict__ a, uint64_t n, uint32_t ld, uint32_t ncols, uint64_t n_parts,
                                                       T *__restrict__ parts) {
    const uint64_t total = n_parts * ncols;
    for (uint64_t e = (uint64_t)blockIdx.x * GRAPH_WG + threadIdx.x; e < total; e += (uint64_t)gridDim.x * GRAPH_WG) {
        const uint64_t part = e / ncols, r0 = part * GRAPH_PART_ROWS, r1 = r0 + GRAPH_PART_ROWS < n ? r0 + GRAPH_PART_ROWS : n;
        const uint32_t c = (uint32_t)(e % ncols);
        T s = 0.0;
        for (uint64_t r = r0; r < r1; r++) s += a[r * ld + c];
        parts[e] = s;
    }
}
// out[c] = the partials ascending
template <typename T>
__global__ __launch_bounds__(64) void k_colfinal(const T *__restrict__ parts, uint64_t n_parts, uint32_t ncols, T *__restrict__ out) {
    const uint32_t c = threadIdx.x;
    if (c >= ncols) return;
    T s = 0.0;
    for (uint64_t p = 0; p < n_parts; p++) s += parts[p * ncols + c];
    out[c] = s;
}
// the column sums of a (n rows of ld doubles, the first ncols <= 64 of each) into out (device, ncols doubles); parts: room for
// ceil(n / GRAPH_PART_ROWS) * ncols partials
static inline void cr_colsums(crgpu_ctx *ctx, const double *a, uint64_t n, uint32_t ld, uint32_t ncols, double *parts, double *out) {
    const uint64_t n_parts = (n + GRAPH_PART_ROWS - 1u) / GRAPH_PART_ROWS;
    hipLaunchKernelGGL(k_colparts<double>, dim3(cr_grid(n_parts * ncols, GRAPH_WG)), dim3(GRAPH_WG), 0, ctx->stream, a, n, ld, ncols, n_parts, parts);
    hipLaunchKernelGGL(k_colfinal<double>, dim3(1), dim3(64), 0, ctx->stream, (const double *)parts, n_parts, ncols, out);
}

}  // namespace

// ---- a caller's input, checked on the host -------------------------------------------------------------------------------------------
// Neighbour lists of n rows and k columns: indices inside the rows, no row names a row twice, finite distances that are not negative
static int cr_check_knn_lists(crgpu_ctx *ctx, const char *who, const int32_t *nn_indices, const double *nn_distances, uint64_t n, uint32_t k) {
    std::vector<uint32_t> stamp(n, 0u);
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t m = 0; m < k; m++) {
            const int32_t j = nn_indices[i * k + m];
            const double d = nn_distances[i * k + m];
            CR_REQUIRE(ctx, j >= 0 && (uint64_t)j < n, CRGPU_EINVAL, "%s: nn_indices[%llu, %u] = %d outside the rows", who, (unsigned long long)i, m, j);
            CR_REQUIRE(ctx, stamp[j] != (uint32_t)i + 1u, CRGPU_EINVAL, "%s: row %llu names row %d twice", who, (unsigned long long)i, j);
            stamp[j] = (uint32_t)i + 1u;
            CR_REQUIRE(ctx, std::isfinite(d) && d >= 0.0, CRGPU_EINVAL, "%s: nn_distances[%llu, %u] = %g, finite and not negative", who,
                       (unsigned long long)i, m, d);
        }
    return CRGPU_OK;
}
// The first structural fault of a CSR of n rows: indptr[0] != 0, an indptr that shrinks or reaches 2^limit_log2 entries (at = its
// place), an index outside the rows (at = the entry), with `ascending` an index not above its predecessor in the row (at = the row)
enum CsrFaultKind { CSR_FINE = 0, CSR_FIRST, CSR_INDPTR, CSR_INDEX, CSR_ORDER };
struct CsrFault {
    CsrFaultKind kind;
    uint64_t at;
};
static CsrFault cr_csr_fault(const int64_t *indptr, const int32_t *indices, uint64_t n, uint32_t limit_log2, bool ascending) {
    if (indptr[0] != 0) return {CSR_FIRST, 0};
    for (uint64_t i = 0; i < n; i++)
        if (indptr[i + 1] < indptr[i] || indptr[i + 1] >= (1ll << limit_log2)) return {CSR_INDPTR, i + 1};
    for (uint64_t i = 0; i < n; i++)
        for (int64_t e = indptr[i]; e < indptr[i + 1]; e++) {
            if (indices[e] < 0 || (uint64_t)indices[e] >= n) return {CSR_INDEX, (uint64_t)e};
            if (ascending && e > indptr[i] && indices[e] <= indices[e - 1]) return {CSR_ORDER, i};
        }
    return {CSR_FINE, 0};
}
static int cr_check_csr(crgpu_ctx *ctx, const char *who, const int64_t *indptr, const int32_t *indices, uint64_t n, uint32_t limit_log2, bool ascending) {
    const CsrFault f = cr_csr_fault(indptr, indices, n, limit_log2, ascending);
    CR_REQUIRE(ctx, f.kind != CSR_FIRST, CRGPU_EINVAL, "%s: indptr[0] = %lld", who, (long long)indptr[0]);
    CR_REQUIRE(ctx, f.kind != CSR_INDPTR, CRGPU_EINVAL, "%s: indptr[%llu] = %lld after %lld: rows do not shrink and hold fewer than 2^%u entries", who,
               (unsigned long long)f.at, (long long)indptr[f.at], (long long)indptr[f.at ? f.at - 1 : 0], limit_log2);
    CR_REQUIRE(ctx, f.kind != CSR_INDEX, CRGPU_EINVAL, "%s: indices[%llu] = %d outside the rows", who, (unsigned long long)f.at, indices[f.at]);
    CR_REQUIRE(ctx, f.kind != CSR_ORDER, CRGPU_EINVAL, "%s: the indices of row %llu must be strictly ascending", who, (unsigned long long)f.at);
    return CRGPU_OK;
}
