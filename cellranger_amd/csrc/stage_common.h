// stage_common.h -- what the count stage (keys.hip, dedup.hip), the device matrix (matrix_dev.hip) and the analysis stages behind
// them (molecule_stages.hip on a crgpu_counts, matrix_stages.hip on a crgpu_matrix_dev) share: the two opaque result types, the
// stream compaction, the barcode segments of the molecule table, the search in an ascending array, the checks of a caller's column
// or rank list, numpy's percentile, and the few host functions one of these units defines for the others.  A kernel defined here is
// a template: the header is part of several units.
// graph_common.h builds on this header for the stages on the kNN graph (tsne.hip, umap.hip, louvain.hip): the pair keys of a neighbour
// list, the run-head flag of equal keys, the sort and the merge of the runs, the CSR from the merged keys, the ordered column sum, and
// the host checks of a caller's neighbour lists and CSR.
#pragma once

#include <cmath>

#include "block_utils.h"
#include "common.h"

int cr_scan_small(crgpu_ctx *ctx, uint32_t *d_data, uint64_t n, uint32_t *d_total_out);  // sort.hip
int cr_partition_by_owner(crgpu_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, uint64_t n, uint32_t sh_bc,
                          uint32_t n_ranks, const uint32_t *bounds, uint64_t *counts_out);  // sort.hip

#define NONE32 0xFFFFFFFFu

struct crgpu_counts {
    uint64_t n_triplets = 0, n_molecules = 0;
    uint32_t *d_bc = nullptr, *d_feature = nullptr, *d_count = nullptr;  // triplets
    uint64_t *d_mkeys = nullptr;    // molecule keys (primary layout), n_molecules
    uint32_t *d_mreads = nullptr;   // read_count of each molecule
    uint32_t *d_corr_reads = nullptr;  // [library][barcode rank] reads whose UMI was corrected (BarcodeSummary), or NULL
    uint32_t *d_filt_reads = nullptr;  // [library][barcode rank] reads of molecules the targeted-panel filter removed, or NULL
    int32_t *d_mprobe = nullptr;    // probe_idx of each molecule's representative read (crgpu_records.d_probe_idx given), or NULL
    uint32_t *d_back = nullptr;     // CRGPU_OPT_DENSE_BARCODE_KEYS: column -> whitelist rank of the barcode field of d_mkeys (n_back), else NULL
    uint32_t n_back = 0;
    uint32_t n_canon = 0;
    KeyLayout layout;
    // (barcode rank, probe_idx, umi_count) triplets, made on the first request (probe_counts.h) for pt_n_probes probes
    bool pt_valid = false;
    uint32_t pt_n_probes = 0;
    uint64_t n_pt = 0;
    uint32_t *d_pt_bc = nullptr, *d_pt_probe = nullptr, *d_pt_count = nullptr;
    // device position -> position in the table crgpu_counts_molecules lists, made on the first subsampling of counts with
    // several libraries or UMI lengths (subsample.h), else NULL
    uint32_t *d_ss_pos = nullptr;
    bool sharded = false;  // one rank's share of a well counted over several ranks (crgpu_count_records_sharded_dev)
};

struct MatrixDevImpl {
    crgpu_matrix_dev view;
    uint32_t *d_rank = nullptr;
    long long *d_indptr = nullptr;
    int32_t *d_indices = nullptr, *d_data = nullptr;
};

// Defined in one unit for the stage units as well: a kernel that is not a template has one definition in one unit, and
// another unit reaches it through a host function.
// matrix_dev.hip: a matrix of V columns and nnz entries with nothing in it yet
int cr_new_matrix_dev(crgpu_ctx *ctx, uint64_t V, uint64_t nnz, MatrixDevImpl **out);
// matrix_dev.hip, launch only: indptr[i] = off[i] for i < n, indptr[n] = total
void cr_offsets_to_indptr(crgpu_ctx *ctx, const uint32_t *d_off, uint64_t n, uint32_t total, long long *d_indptr);
// dedup.hip: the molecule table on the host in the order ALIGN_AND_COUNT emits it: order[o] = device position of the o-th UmiCount
int cr_molecule_order(crgpu_ctx *ctx, const crgpu_counts *c, std::vector<uint64_t> &keys, std::vector<uint32_t> &reads,
                      std::vector<uint32_t> &order);

// robust_divide of the reference's metrics: NaN for a zero denominator
static inline double cr_robust_divide(double a, double b) { return b == 0.0 ? std::nan("") : a / b; }

// np.sum of a contiguous f64 array: numpy's pairwise sum (blocks of at most 128 values, eight interleaved partial sums)
static double cr_pairwise_sum(const double *a, size_t n) {
    if (n < 8) {
        double r = 0.0;
        for (size_t i = 0; i < n; i++) r += a[i];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; j++) r[j] = a[j];
        size_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; j++) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; i++) res += a[i];
        return res;
    }
    size_t n2 = n / 2;
    n2 -= n2 % 8;
    return cr_pairwise_sum(a, n2) + cr_pairwise_sum(a + n2, n - n2);
}
// numpy's _lerp: a + (b - a) t, taken from b's side for t >= 0.5
__host__ __device__ __forceinline__ double cr_lerp(double a, double b, double t) {
    const double d = b - a;
    return t >= 0.5 ? b - d * (1.0 - t) : a + d * t;
}
// np.percentile(sorted x, 100 q) with the linear rule: virtual index (n - 1) q; x is not empty, its elements are taken as f64
template <typename T>
static inline double cr_quantile_sorted(const std::vector<T> &x, double q) {
    const size_t n = x.size();
    const double vi = (double)(n - 1) * q, fl = std::floor(vi);
    const size_t p = (size_t)fl, nx = p + 1 < n ? p + 1 : n - 1;
    return cr_lerp((double)x[p], (double)x[nx], vi - fl);
}
// np.median of sorted x: the mean of the two middle values; x is not empty
template <typename T>
static inline double cr_median_sorted(const std::vector<T> &x) {
    const size_t n = x.size();
    return n % 2 ? (double)x[n / 2] : ((double)x[n / 2 - 1] + (double)x[n / 2]) / 2.0;
}

// scikit-learn's GaussianMixture EM for two 1-D components, as rpu_gmm.h (molecule_stages.hip) and marginal_calls.h
// (matrix_stages.hip) both run it: max_iter, tol, reg_covar, log(2 pi) and the logsumexp of the two weighted log probabilities
#define GMM_MAX_ITER 100u
#define GMM_TOL 1e-3
#define GMM_REG 1e-6
#define GMM_LOG_2PI 1.8378770664093453  // np.log(2 * np.pi)
__device__ __forceinline__ double gmm_logsumexp(double a0, double a1) {
    const double m = a0 > a1 ? a0 : a1;
    return log(exp(a0 - m) + exp(a1 - m)) + m;
}

__device__ __forceinline__ uint64_t lowmask(uint32_t bits) { return bits >= 64 ? ~0ull : ((1ull << bits) - 1ull); }

// x[0 .. n) ascending: the first index with x[i] >= v (cr_lower_bound) or x[i] > v (cr_upper_bound), else n = the number of elements
// below v / not above v.  The index type is that of n.
template <typename T, typename I>
__device__ __forceinline__ I cr_lower_bound(const T *x, I n, T v) {
    I lo = 0, hi = n;
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (x[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
template <typename T, typename I>
__device__ __forceinline__ I cr_upper_bound(const T *x, I n, T v) {
    I lo = 0, hi = n;
    while (lo < hi) {
        const I mid = lo + ((hi - lo) >> 1);
        if (x[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

static inline int read_u32(crgpu_ctx *ctx, const uint32_t *d, uint32_t *h) {
    return crgpu_memcpy_d2h(ctx, h, d, sizeof(uint32_t));
}

// ------------------------------------------------------------------------------------------------
// generic two-pass stream compaction driven by a flag functor: out position of every flagged item
// ------------------------------------------------------------------------------------------------
#define CP_BLOCK 256
#ifndef CP_ITEMS
#define CP_ITEMS 8  // items per thread per round: their flag loads are all issued before the first compare
#endif
#define CP_ROUND (CP_BLOCK * CP_ITEMS)
#define CP_WAVES (CP_BLOCK / 64)

// Flags are evaluated at clamped indices and masked afterwards, so that the loads of a round are not chained
// behind `i < hi` branches (one load in flight per wave left these passes at ~2 TB/s).
template <typename Flag>
__global__ __launch_bounds__(CP_BLOCK) void k_cp_count(Flag flag, uint64_t n, uint64_t tile, uint32_t *__restrict__ block_counts) {
    __shared__ uint32_t ws[CP_WAVES];
    const uint64_t lo = (uint64_t)blockIdx.x * tile;
    const uint64_t hi = lo + tile < n ? lo + tile : n;
    uint32_t c = 0;
    for (uint64_t base = lo; base < hi; base += CP_ROUND) {
        bool f[CP_ITEMS];
#pragma unroll
        for (int j = 0; j < CP_ITEMS; j++) {
            const uint64_t i = base + (uint64_t)j * CP_BLOCK + threadIdx.x;
            f[j] = flag(i < hi ? i : hi - 1);
        }
#pragma unroll
        for (int j = 0; j < CP_ITEMS; j++) {
            const uint64_t i = base + (uint64_t)j * CP_BLOCK + threadIdx.x;
            c += (f[j] && i < hi) ? 1u : 0u;
        }
    }
    block_sum_to_first<CP_WAVES>(c, ws, &block_counts[blockIdx.x]);
}

// Stable: inside a round the output order is (item slot, wave, lane) == ascending input index.
template <typename Flag, typename Emit>
__global__ __launch_bounds__(CP_BLOCK) void k_cp_write(Flag flag, Emit emit, uint64_t n, uint64_t tile,
                                                       const uint32_t *__restrict__ block_offs) {
    __shared__ uint32_t ws[CP_ITEMS * CP_WAVES];  // flagged items of (item slot, wave), then their exclusive prefix
    __shared__ uint32_t round_total;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t lo = (uint64_t)blockIdx.x * tile;
    const uint64_t hi = lo + tile < n ? lo + tile : n;
    uint32_t run = block_offs[blockIdx.x];
    for (uint64_t base = lo; base < hi; base += CP_ROUND) {
        bool f[CP_ITEMS];
        typename Emit::Pre pre[CP_ITEMS];  // what the emit needs from memory, requested together with the flags
#pragma unroll
        for (int j = 0; j < CP_ITEMS; j++) {
            const uint64_t i = base + (uint64_t)j * CP_BLOCK + threadIdx.x;
            f[j] = flag(i < hi ? i : hi - 1);
            pre[j] = emit.pre(i < hi ? i : hi - 1);
        }
        uint32_t below[CP_ITEMS];
#pragma unroll
        for (int j = 0; j < CP_ITEMS; j++) {
            const uint64_t i = base + (uint64_t)j * CP_BLOCK + threadIdx.x;
            f[j] = f[j] && i < hi;
            const unsigned long long m = __ballot(f[j]);
            below[j] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) ws[j * CP_WAVES + wave] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        block_scan_words<CP_ITEMS * CP_WAVES>(ws, &round_total);  // 32 lanes of wave 0: exclusive scan in (slot, wave) order
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CP_ITEMS; j++) {
            const uint64_t i = base + (uint64_t)j * CP_BLOCK + threadIdx.x;
            if (f[j]) emit(i, run + ws[j * CP_WAVES + wave] + below[j], pre[j]);
        }
        run += round_total;
        __syncthreads();
    }
}

static inline uint32_t cp_blocks(uint64_t n, uint64_t *tile_out) {
    uint64_t nb = (n + CP_ROUND * 4 - 1) / (CP_ROUND * 4);
    if (nb < 1) nb = 1;
    if (nb > 4096) nb = 4096;
    uint64_t tile = (n + nb - 1) / nb;
    tile = (tile + CP_ROUND - 1) / CP_ROUND * CP_ROUND;
    nb = (n + tile - 1) / tile;
    if (nb < 1) nb = 1;
    *tile_out = tile;
    return (uint32_t)nb;
}

// d_block: workspace of >= 4096 u32.  *total_out (device u32) receives the number of flagged items.
template <typename Flag, typename Emit>
static int compact(crgpu_ctx *ctx, Flag flag, Emit emit, uint64_t n, uint32_t *d_block, uint32_t *d_total_out) {
    uint64_t tile;
    const uint32_t nb = cp_blocks(n, &tile);
    hipLaunchKernelGGL(k_cp_count<Flag>, dim3(nb), dim3(CP_BLOCK), 0, ctx->stream, flag, n, tile, d_block);
    CR_TRY(cr_scan_small(ctx, d_block, nb, d_total_out));
    hipLaunchKernelGGL((k_cp_write<Flag, Emit>), dim3(nb), dim3(CP_BLOCK), 0, ctx->stream, flag, emit, n, tile, d_block);
    CR_HIP(ctx, hipGetLastError());
    return CRGPU_OK;
}

struct CandFlag {
    const uint8_t *cand;
    __device__ __forceinline__ bool operator()(uint64_t k) const { return cand[k] != 0; }
};
struct SegHeadFlag {  // first molecule of a barcode
    const uint64_t *keys;
    uint32_t shift;
    __device__ __forceinline__ bool operator()(uint64_t i) const {
        const uint64_t prev = keys[i ? i - 1 : 0];
        return (i == 0) | ((keys[i] >> shift) != (prev >> shift));
    }
};
struct EmitSegStart {
    uint32_t *start;
    struct Pre {};
    __device__ __forceinline__ Pre pre(uint64_t) const { return Pre(); }
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t o, Pre) const { start[o] = (uint32_t)i; }
};

// The barcode segments of the molecule table (ordered by barcode first; 1 <= n_molecules < 2^32 - 1): seg_b[s] = the first molecule
// of the s-th barcode with a molecule, seg_b[*n_seg] = n_molecules.  One compaction and one read-back.
static int cr_barcode_segments(crgpu_ctx *ctx, const crgpu_counts *c, const char *who, DevBuf &seg_b, uint32_t *n_seg) {
    const uint64_t nm = c->n_molecules, n_bc = c->d_back ? c->n_back : c->n_canon;
    const uint64_t seg_max = nm < n_bc ? nm : n_bc;
    uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL;
    CR_TRY(dmalloc(ctx, seg_b, (seg_max + 1) * sizeof(uint32_t)));
    {
        CrTimer t(ctx, CRGPU_T_DEDUP, nm);
        CR_TRY(compact(ctx, SegHeadFlag{c->d_mkeys, c->layout.sh_bc()}, EmitSegStart{seg_b.as<uint32_t>()}, nm, ctx->d_sort_hist, d_total));
    }
    CR_TRY(read_u32(ctx, d_total, n_seg));
    CR_REQUIRE(ctx, *n_seg >= 1 && *n_seg <= seg_max, CRGPU_EHIP, "%s: %u barcode segments for at most %llu barcodes", who, *n_seg,
               (unsigned long long)seg_max);
    CR_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)(seg_b.as<uint32_t>() + *n_seg), (int)(uint32_t)nm, 1, ctx->stream));  // the end of the last segment
    return CRGPU_OK;
}

// ---- a caller's list, checked on the device ----------------------------------------------------------------------------------
// Column list: flag bit 0 for a column >= V, with ASCEND bit 1 for a column that is not above its predecessor; every column < V goes
// to the mark functor with its place in the list.
#define CR_LIST_RANGE 1u
#define CR_LIST_ORDER 2u
struct MarkNone {
    __device__ __forceinline__ void operator()(uint64_t, uint64_t) const {}
};
struct MarkByte {  // flag[c] = 1
    uint8_t *flag;
    __device__ __forceinline__ void operator()(uint64_t, uint64_t c) const { flag[c] = 1u; }
};
struct MarkPlace {  // idx[c] = place + 1 (0: not listed)
    uint32_t *idx;
    __device__ __forceinline__ void operator()(uint64_t k, uint64_t c) const { idx[c] = (uint32_t)k + 1u; }
};
template <bool ASCEND, typename Mark>
__global__ __launch_bounds__(256) void k_check_columns(const uint64_t *__restrict__ cols, uint64_t n, uint64_t V, Mark mark, uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const uint64_t c = cols[k];
        if (ASCEND && k && cols[k - 1] >= c) atomicOr(flag, CR_LIST_ORDER);
        if (c >= V) atomicOr(flag, CR_LIST_RANGE);
        else mark(k, c);
    }
}
// Rank list: CR_LIST_ORDER for a rank that is not above its predecessor.  A template only for the one-definition rule.
template <typename T>
__global__ __launch_bounds__(256) void k_check_ranks(const T *__restrict__ r, uint64_t n, uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 1 < n; i += stride)
        if (r[i] >= r[i + 1]) atomicOr(flag, CR_LIST_ORDER);
}
// launch only; *d_flag was zeroed on the stream.  n == 0 launches nothing
template <bool ASCEND, typename Mark>
static inline void cr_check_columns(crgpu_ctx *ctx, const uint64_t *d_cols, uint64_t n, uint64_t V, Mark mark, uint32_t *d_flag) {
    if (n) hipLaunchKernelGGL((k_check_columns<ASCEND, Mark>), dim3(cr_grid(n, 256)), dim3(256), 0, ctx->stream, d_cols, n, V, mark, d_flag);
}
static inline void cr_check_ranks(crgpu_ctx *ctx, const uint32_t *d_ranks, uint64_t n, uint32_t *d_flag) {
    if (n > 1) hipLaunchKernelGGL(k_check_ranks<uint32_t>, dim3(cr_grid(n, 256)), dim3(256), 0, ctx->stream, d_ranks, n, d_flag);
}
// the verdict on the flag word read back: `what` names an element of the list ("cell column", "cell barcode rank")
static inline int cr_list_verdict(crgpu_ctx *ctx, uint32_t flag, const char *who, const char *what) {
    CR_REQUIRE(ctx, !(flag & CR_LIST_RANGE), CRGPU_EINVAL, "%s: a %s is out of range", who, what);
    CR_REQUIRE(ctx, !(flag & CR_LIST_ORDER), CRGPU_EINVAL, "%s: the %ss must be strictly ascending", who, what);
    return CRGPU_OK;
}
// a rank list checked on its own: zero the flag, launch, read back, verdict
static int cr_require_ascending_ranks(crgpu_ctx *ctx, const uint32_t *d_ranks, uint64_t n, const char *who, const char *what) {
    if (n < 2) return CRGPU_OK;
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    cr_check_ranks(ctx, d_ranks, n, d_flag);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_flag, &flag));
    return cr_list_verdict(ctx, flag, who, what);
}

// ---- the barcode index: the canonical barcodes with a count in some library (barcode_index.rs:20-53) ----
struct CountTables {
    const uint32_t *t[2 * CRGPU_MAX_LIB];
    uint32_t n;
};
struct SeenFlag {  // barcode has a non-zero valid or corrected count in some library
    CountTables ct;
    __device__ __forceinline__ bool operator()(uint64_t r) const {
        uint32_t any = 0;
        for (uint32_t k = 0; k < ct.n; k++) any |= ct.t[k][r];
        return any != 0u;
    }
};
struct EmitCol {
    uint32_t *rank;
    struct Pre {};
    __device__ __forceinline__ Pre pre(uint64_t) const { return Pre(); }
    __device__ __forceinline__ void operator()(uint64_t r, uint32_t o, Pre) const { rank[o] = (uint32_t)r; }
};
