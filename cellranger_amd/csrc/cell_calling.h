// cell_calling.h -- the initial cell call on the device (part of matrix_stages.hip: works on crgpu_matrix_dev).
//
// Replaces filter_cellular_barcodes_ordmag with estimate_recovered_cells_ordmag, find_within_ordmag and
// summarize_bootstrapped_top_n (lib/python/cellranger/cell_calling_helpers.py:832-955) and
// filter_cellular_barcodes_fixed_cutoff (:958-964), get_counts_per_bc of a feature sub-matrix, and
// CountMatrix.select_barcodes with the called columns.
//
// The reference draws 100 (200 with the estimate) bootstrap samples of the N non-zero barcode totals with
// np.random.RandomState(0).choice and sorts every one of them.  A sample only matters through order statistics, so here
//   1. the N totals are sorted ONCE, descending (pos[i] = place of barcode i, sorted[p] = the total at place p);
//   2. k_mt19937 produces the generator's raw stream (one workgroup: the recurrence is serial, see below), a compaction that
//      keeps the stream order applies numpy's mask-and-reject, and accepted draw j lands in the histogram of sample j / N at
//      pos[index]: h[sample][p] = how often the barcode at place p was drawn;
//   3. C = inclusive scan of h along p: C[p] = sampled barcodes whose total is >= sorted[p] (ties in place order).  The k-th
//      largest of the sample is sorted[min p : C[p] >= k], the number of sampled totals >= cutoff is C[last p : sorted[p] >= cutoff]:
//      two binary searches per (sample, baseline), and the estimate scores all <= 1414 grid values against the same C;
//   4. the summary of the 100 integers and the tie extension run on the host; the selection is a compaction of pos[i] < top_n.
// Integer work except rint(0.1 * baseline) and the loss divide (f64, -ffp-contract=off like the rest of the library).
#pragma once

#include <algorithm>
#include <cmath>
#include <optional>

#include "stage_common.h"

// ---- MT19937 (the raw stream of np.random.RandomState) -----------------------------------------------------------------------
// x[n] = x[n - 227] ^ twist(x[n - 624], x[n - 623]): 227 consecutive words depend on older ones only.  ONE workgroup keeps a
// window of the sequence in LDS and extends it by 227 words per barrier; after MT_CHUNK words the last 624 move to the front.
// The 624 words that precede the next output are the carried state (device memory, between launches).
// Measured: 1.68 Gword/s, 98 - 99 % of a call (profiles/cell_calling_throughput.txt).
#define MT_N 624
#define MT_STEP 227
#define MT_STEPS 16
#define MT_CHUNK (MT_STEP * MT_STEPS)  // words per chunk; every launch produces whole chunks

__host__ __device__ __forceinline__ uint32_t mt_temper(uint32_t y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

static void mt_init_genrand(uint32_t seed, uint32_t *mt) {
    mt[0] = seed;
    for (uint32_t i = 1; i < MT_N; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i;
}

// out[0 .. n_chunks * MT_CHUNK): the next words of the sequence (TEMPER: the generator's outputs, else the untempered words
// for a consumer that tempers them itself); state[0 .. 624) is read and left at the position after the last word.
template <bool TEMPER>
__global__ __launch_bounds__(256) void k_mt19937(uint32_t *__restrict__ state, uint32_t *__restrict__ out, uint64_t n_chunks) {
    __shared__ uint32_t w[MT_N + MT_CHUNK];
    const uint32_t tid = threadIdx.x;
    for (uint32_t t = tid; t < MT_N; t += 256) w[t] = state[t];
    __syncthreads();
    for (uint64_t c = 0; c < n_chunks; c++) {
        uint32_t *o = out + c * MT_CHUNK;
        for (uint32_t s = 0; s < MT_STEPS; s++) {
            if (tid < MT_STEP) {
                const uint32_t k = MT_N + s * MT_STEP + tid;  // reads reach back to k - 227 at the nearest: words of earlier steps
                const uint32_t y = (w[k - 624] & 0x80000000u) | (w[k - 623] & 0x7fffffffu);
                const uint32_t x = w[k - 227] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
                w[k] = x;
                o[s * MT_STEP + tid] = TEMPER ? mt_temper(x) : x;
            }
            __syncthreads();
        }
        uint32_t keep[3];
#pragma unroll
        for (uint32_t r = 0; r < 3; r++) {
            const uint32_t t = tid + r * 256;
            keep[r] = t < MT_N ? w[MT_CHUNK + t] : 0u;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t r = 0; r < 3; r++) {
            const uint32_t t = tid + r * 256;
            if (t < MT_N) w[t] = keep[r];
        }
        __syncthreads();
    }
    for (uint32_t t = tid; t < MT_N; t += 256) state[t] = w[t];
}

extern "C" int crgpu_mt19937_stream_dev(crgpu_ctx *ctx, uint32_t seed, uint64_t n_words, uint32_t *d_out, uint64_t *n_written_out,
                                        double *ms_out) {
    if (!ctx || !n_written_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *n_written_out = 0;
    if (ms_out) *ms_out = 0.0;
    const uint64_t chunks = n_words / MT_CHUNK;
    if (!chunks) return CRGPU_OK;
    CR_REQUIRE(ctx, d_out != nullptr, CRGPU_EINVAL, "crgpu_mt19937_stream_dev: NULL output");
    uint32_t mt[MT_N];
    mt_init_genrand(seed, mt);
    DevBuf st;
    CR_TRY(dmalloc(ctx, st, sizeof(mt)));
    CR_TRY(crgpu_memcpy_h2d(ctx, st.p, mt, sizeof(mt)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    CR_HIP(ctx, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        return cr_fail(ctx, CRGPU_EHIP, "crgpu_mt19937_stream_dev: no event");
    }
    (void)hipEventRecord(e0, ctx->stream);
    hipLaunchKernelGGL(k_mt19937<true>, dim3(1), dim3(256), 0, ctx->stream, st.as<uint32_t>(), d_out, chunks);
    (void)hipEventRecord(e1, ctx->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (e != hipSuccess) return cr_fail(ctx, CRGPU_EHIP, "crgpu_mt19937_stream_dev: %s", hipGetErrorString(e));
    if (ms_out) *ms_out = ms;
    *n_written_out = chunks * MT_CHUNK;
    return CRGPU_OK;
}

// ---- the candidate grid of the estimate (host) -------------------------------------------------------------------------------
static void om_candidates(int64_t max_expected_cells, std::vector<int64_t> &rc) {
    // np.linspace(1, log2(max), 2000): i * step + 1 with the end point set exactly; then unique(round(2 ^ .))
    const double stop = std::log2((double)max_expected_cells), step = (stop - 1.0) / 1999.0;
    rc.clear();
    for (int i = 0; i < 2000; i++) {
        const double x = i == 1999 ? stop : (double)i * step + 1.0;
        const int64_t v = (int64_t)std::nearbyint(std::pow(2.0, x));
        if (rc.empty() || v > rc.back()) rc.push_back(v);  // the values ascend: unique == drop repeats
    }
}

extern "C" int crgpu_ordmag_candidates(int64_t max_expected_cells, int64_t *out, uint32_t cap, uint32_t *n_out) {
    if (!n_out || max_expected_cells < 2) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_ordmag_candidates: max_expected_cells >= 2 and n_out");
    std::vector<int64_t> rc;
    om_candidates(max_expected_cells, rc);
    *n_out = (uint32_t)rc.size();
    if (!out) return CRGPU_OK;
    if (cap < rc.size()) return cr_fail(nullptr, CRGPU_ERANGE, "crgpu_ordmag_candidates: %zu values, room for %u", rc.size(), cap);
    std::copy(rc.begin(), rc.end(), out);
    return CRGPU_OK;
}

// ---- column sums -------------------------------------------------------------------------------------------------------------
// one wave per column; flag bit 0: a sum above 2^32 - 1, bit 1: a row outside the mask
__global__ __launch_bounds__(256) void k_column_sums(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                     const int32_t *__restrict__ data, uint64_t V, const uint8_t *__restrict__ mask,
                                                     uint32_t n_features, uint32_t *__restrict__ sums, uint32_t *__restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave0; c < V; c += n_waves) {
        const long long s = indptr[c], e = indptr[c + 1];
        unsigned long long acc = 0;
        uint32_t bad = 0;
        for (long long i = s + lane; i < e; i += 64) {
            bool take = true;
            if (mask) {
                const uint32_t f = (uint32_t)indices[i];
                if (f >= n_features) {
                    bad = 2u;
                    take = false;
                } else {
                    take = mask[f] != 0;
                }
            }
            if (take) acc += (uint32_t)data[i];
        }
        acc = wave_sum(acc);
        bad = wave_or(bad);
        if (lane == 0) {
            if (acc > 0xFFFFFFFFull) bad |= 1u;
            sums[c] = (uint32_t)acc;
            if (bad) atomicOr(flag, bad);
        }
    }
}

extern "C" int crgpu_matrix_dev_column_sums(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint8_t *feature_mask, uint32_t n_features,
                                            uint32_t *d_sums_out) {
    if (!ctx || !m) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const uint64_t V = m->n_barcodes;
    if (!V) return CRGPU_OK;
    CR_REQUIRE(ctx, d_sums_out != nullptr, CRGPU_EINVAL, "crgpu_matrix_dev_column_sums: NULL output");
    DevBuf mask_b;
    if (feature_mask) {
        CR_TRY(dmalloc(ctx, mask_b, n_features ? n_features : 1));
        if (n_features) CR_TRY(crgpu_memcpy_h2d(ctx, mask_b.p, feature_mask, n_features));
    }
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
        hipLaunchKernelGGL(k_column_sums, dim3(cr_grid(V * 64, 256)), dim3(256), 0, ctx->stream, (const long long *)m->d_indptr,
                           m->d_indices, m->d_data, V, feature_mask ? mask_b.as<uint8_t>() : (const uint8_t *)nullptr, n_features,
                           d_sums_out, d_flag);
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !(flag & 2u), CRGPU_EINVAL, "crgpu_matrix_dev_column_sums: the matrix holds a row >= n_features (%u)", n_features);
    CR_REQUIRE(ctx, !(flag & 1u), CRGPU_ERANGE, "crgpu_matrix_dev_column_sums: a column sum does not fit 32 bits");
    return CRGPU_OK;
}

// ---- the non-zero totals, their descending order -----------------------------------------------------------------------------
struct OmNzFlag {
    const uint32_t *counts;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return counts[i] != 0u; }
};
struct OmNzEmit {
    const uint32_t *counts;
    uint32_t *val, *col;
    struct Pre {
        uint32_t c;
    };
    __device__ __forceinline__ Pre pre(uint64_t i) const { return Pre{counts[i]}; }
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t o, Pre p) const {
        val[o] = p.c;
        col[o] = (uint32_t)i;
    }
};
// keys of a stable ASCENDING sort that yields the totals descending with the LARGER column first among equal ones (the
// reverse of a stable ascending argsort): the complement of the total, fed in reversed column order
__global__ __launch_bounds__(256) void k_om_keys(const uint32_t *__restrict__ nz, uint32_t N, uint32_t *__restrict__ key,
                                                 uint32_t *__restrict__ val) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += stride) {
        key[j] = ~nz[N - 1u - j];
        val[j] = N - 1u - j;
    }
}
__global__ __launch_bounds__(256) void k_om_places(const uint32_t *__restrict__ key, const uint32_t *__restrict__ val, uint32_t N,
                                                   uint32_t *__restrict__ sorted, uint32_t *__restrict__ pos) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < N; p += stride) {
        sorted[p] = ~key[p];
        pos[val[p]] = p;  // val is a permutation of 0 .. N-1
    }
}

// ---- draws -> per-sample histograms ------------------------------------------------------------------------------------------
// numpy's bounded draw: the 32-bit output ANDed with the smallest 2^k - 1 >= N - 1, values above N - 1 dropped
struct OmDrawFlag {
    const uint32_t *raw;
    uint32_t mask, nm1;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return (mt_temper(raw[i]) & mask) <= nm1; }
};
// accepted draw number base + o of the whole call; the window [0, span) of (that number - the window's first draw) is the
// batch in hand: sample (rel / N) of the batch, element pos[index]
struct OmDrawEmit {
    const uint32_t *raw, *pos;
    uint32_t *hist;
    uint32_t mask, N;
    long long base;
    unsigned long long span;
    struct Pre {
        uint32_t v;
    };
    __device__ __forceinline__ Pre pre(uint64_t i) const { return Pre{mt_temper(raw[i]) & mask}; }
    __device__ __forceinline__ void operator()(uint64_t, uint32_t o, Pre p) const {
        const long long rel = base + (long long)o;
        if (rel < 0 || (unsigned long long)rel >= span) return;
        const uint32_t r = (uint32_t)rel;  // span = samples * N of one batch < 2^32
        atomicAdd(&hist[r - r % N + pos[p.v]], 1u);
    }
};
__global__ __launch_bounds__(256) void k_om_fill(uint32_t *__restrict__ a, uint64_t n, uint32_t v) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) a[i] = v;
}

// in-place inclusive scan of every row of h[rows][N]; one workgroup per row, 8 consecutive elements per thread and round
#define OM_SCAN_ITEMS 8
__global__ __launch_bounds__(256) void k_om_row_scan(uint32_t *__restrict__ h, uint32_t N) {
    __shared__ uint32_t ws[4];
    __shared__ uint32_t carry_s;
    uint32_t *row = h + (uint64_t)blockIdx.x * N;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint64_t base = 0; base < N; base += 256 * OM_SCAN_ITEMS) {
        const uint64_t i0 = base + (uint64_t)tid * OM_SCAN_ITEMS;
        uint32_t v[OM_SCAN_ITEMS];
        uint32_t sum = 0;
#pragma unroll
        for (int j = 0; j < OM_SCAN_ITEMS; j++) {
            v[j] = i0 + j < N ? row[i0 + j] : 0u;
            sum += v[j];
            v[j] = sum;
        }
        const uint32_t x = wave_incl_scan(sum, lane);
        if (lane == 63) ws[wave] = x;
        __syncthreads();
        uint32_t pre = carry_s + x - sum, tot = 0;
        for (uint32_t k = 0; k < 4; k++) {
            if (k < wave) pre += ws[k];
            tot += ws[k];
        }
#pragma unroll
        for (int j = 0; j < OM_SCAN_ITEMS; j++)
            if (i0 + j < N) row[i0 + j] = pre + v[j];
        __syncthreads();
        if (tid == 0) carry_s += tot;
        __syncthreads();
    }
}

// find_within_ordmag (:864-870) of the sample whose scanned histogram is C: baseline = its (b + 1)-th largest total,
// cutoff = max(1, round_half_even(0.1 * baseline)), result = sampled totals >= cutoff.  b <= N - 1 and C[N - 1] == N.
__device__ __forceinline__ uint32_t om_within(const uint32_t *__restrict__ C, const uint32_t *__restrict__ sorted, uint32_t N, uint32_t b) {
    uint32_t lo = 0, hi = N - 1u;
    while (lo < hi) {  // the first place with C >= b + 1
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (C[mid] > b) hi = mid; else lo = mid + 1u;
    }
    const double c = rint(0.1 * (double)sorted[lo]);
    const uint32_t cutoff = c < 1.0 ? 1u : (uint32_t)c;
    hi = N - 1u;  // the last place with sorted >= cutoff; cutoff <= baseline, so `lo` already qualifies
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (sorted[mid] >= cutoff) lo = mid; else hi = mid - 1u;
    }
    return C[lo];
}

__global__ __launch_bounds__(256) void k_om_top_n(const uint32_t *__restrict__ C, const uint32_t *__restrict__ sorted, uint32_t N,
                                                  uint32_t b, uint32_t rows, long long *__restrict__ top_n) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < rows) top_n[s] = (long long)om_within(C + (uint64_t)s * N, sorted, N, b);
}

// estimate_recovered_cells_ordmag (:873-886) of one sample per workgroup: loss = (filtered - rc)^2 / rc over the grid, its FIRST
// minimum.  bidx[k] = min(round(rc[k] * (1 - 0.99)), N - 1), made on the host.
__global__ __launch_bounds__(256) void k_om_estimate(const uint32_t *__restrict__ C, const uint32_t *__restrict__ sorted, uint32_t N,
                                                     const long long *__restrict__ rc, const uint32_t *__restrict__ bidx, uint32_t n_rc,
                                                     long long *__restrict__ rec_out, double *__restrict__ loss_out) {
    __shared__ double s_loss[256];
    __shared__ uint32_t s_k[256];
    const uint32_t *row = C + (uint64_t)blockIdx.x * N;
    double best = 0.0;
    uint32_t best_k = 0xFFFFFFFFu;
    for (uint32_t k = threadIdx.x; k < n_rc; k += 256) {
        const long long d = (long long)om_within(row, sorted, N, bidx[k]) - rc[k];  // |d| < 2^31 (N < 2^31, rc <= 2^30): the square fits
        const double loss = (double)(d * d) / (double)rc[k];
        if (best_k == 0xFFFFFFFFu || loss < best) {  // k ascends: ties keep the earlier one
            best = loss;
            best_k = k;
        }
    }
    s_loss[threadIdx.x] = best;
    s_k[threadIdx.x] = best_k;
    __syncthreads();
    for (uint32_t d = 128; d >= 1; d >>= 1) {
        if (threadIdx.x < d) {
            const double ol = s_loss[threadIdx.x + d];
            const uint32_t ok = s_k[threadIdx.x + d], mk = s_k[threadIdx.x];
            if (ok != 0xFFFFFFFFu && (mk == 0xFFFFFFFFu || ol < s_loss[threadIdx.x] || (ol == s_loss[threadIdx.x] && ok < mk))) {
                s_loss[threadIdx.x] = ol;
                s_k[threadIdx.x] = ok;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        rec_out[blockIdx.x] = rc[s_k[0]];
        loss_out[blockIdx.x] = s_loss[0];
    }
}

// ---- the bootstrap: stream rounds and sample batches ---------------------------------------------------------------------------
// Accepted draws are numbered through the whole call (sample s owns [s * N, (s + 1) * N)).  A round is one launch of the
// generator into d_raw; the draws it holds may straddle two batches, so a batch first looks at the round in hand again.
struct OmBootstrap {
    crgpu_ctx *ctx;
    uint32_t N = 0, mask = 0, B = 1;
    const uint32_t *d_pos = nullptr, *d_sorted = nullptr;
    DevBuf state, raw, hist;
    uint64_t raw_words = 0, total = 0;                          // room of d_raw; accepted draws the whole call needs
    uint64_t acc_before = 0, acc_round = 0, round_words = 0;  // accepted draws before / in the round in hand, its raw words
    // samples per batch: at most batch_cap; batch_forced >= 0 replaces CRGPU_ORDMAG_BATCH (the multi-genome bootstrap, multigenome.h)
    uint32_t batch_cap = CRGPU_ORDMAG_SAMPLES;
    long long batch_forced = -1;
    uint64_t words_made = 0;  // raw words the generator produced for this call
    // ledger spans of the generator, the compaction and the scan: off for the cell call, whose ledger slots stay as they were
    bool timed = false;
    const char *who = "cell call";  // the caller, for the error text

    uint64_t words_wanted(uint64_t draws) const {
        const double w = (double)draws * ((double)mask + 1.0) / (double)N * 1.001 + (double)MT_CHUNK;
        return ((uint64_t)w + MT_CHUNK - 1) / MT_CHUNK * MT_CHUNK;
    }
    int init(uint32_t n, uint32_t n_samples, const uint32_t *pos, const uint32_t *sorted) {
        N = n;
        d_pos = pos;
        d_sorted = sorted;
        total = (uint64_t)n_samples * N;
        for (mask = 0; mask < N - 1u; mask = (mask << 1) | 1u) {}
        const uint32_t forced = batch_forced >= 0 ? (uint32_t)batch_forced : ctx->ordmag_batch;
        if (forced) {
            B = forced;
        } else {  // histograms of one batch: at most 256 MB
            const uint64_t fit = (64ull << 20) / N;
            B = (uint32_t)(fit < 1 ? 1 : fit > batch_cap ? batch_cap : fit);
        }
        if (B > batch_cap) B = batch_cap;
        if (B > n_samples) B = n_samples;  // no rows beyond the call's samples (n_samples >= 1)
        if ((uint64_t)B * N > 0xFFFFFFFFull) B = (uint32_t)(0xFFFFFFFFull / N);  // OmDrawEmit counts inside a batch in 32 bits
        CR_TRY(dmalloc(ctx, hist, (uint64_t)B * N * sizeof(uint32_t)));
        if (N == 1) return CRGPU_OK;  // choice() of one element consumes no generator output
        const uint64_t cap = ((1ull << 24) / MT_CHUNK) * MT_CHUNK;
        raw_words = std::min(words_wanted(total), cap);
        CR_TRY(dmalloc(ctx, raw, raw_words * sizeof(uint32_t)));
        uint32_t mt[MT_N];
        mt_init_genrand(0u, mt);
        CR_TRY(dmalloc(ctx, state, sizeof(mt)));
        return crgpu_memcpy_h2d(ctx, state.p, mt, sizeof(mt));
    }
    // the round in hand -> the histograms of the draws [w0, w1); acc_round = what the round holds
    // Every batch that overlaps a round tempers and compacts the WHOLE round again.  With the default batches that is at most one
    // extra pass per batch seam; with CRGPU_ORDMAG_BATCH=1 and a small N (one round holds all samples) it is one pass per
    // sample, which only the tests pay.  Measured with everything else but the generator: <= 2.7 of 127 ms at N = 2^20.
    int consume(uint64_t w0, uint64_t w1) {
        uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL, t = 0;
        OmDrawFlag flag{raw.as<uint32_t>(), mask, N - 1u};
        OmDrawEmit emit{raw.as<uint32_t>(), d_pos, hist.as<uint32_t>(), mask, N, (long long)acc_before - (long long)w0, w1 - w0};
        {
            std::optional<CrTimer> tm;
            if (timed) tm.emplace(ctx, CRGPU_T_KEYS, round_words);
            CR_TRY(compact(ctx, flag, emit, round_words, ctx->d_sort_hist, d_total));
        }
        CR_TRY(read_u32(ctx, d_total, &t));
        acc_round = t;
        return CRGPU_OK;
    }
    // scanned histograms of samples [s0, s1) of the call (s1 - s0 <= B) in hist
    int fill(uint32_t s0, uint32_t s1) {
        const uint64_t w0 = (uint64_t)s0 * N, w1 = (uint64_t)s1 * N;
        if (N == 1) {
            hipLaunchKernelGGL(k_om_fill, dim3(1), dim3(256), 0, ctx->stream, hist.as<uint32_t>(), w1 - w0, 1u);
            CR_HIP(ctx, hipGetLastError());
            return CRGPU_OK;
        }
        CR_HIP(ctx, hipMemsetAsync(hist.p, 0, (w1 - w0) * sizeof(uint32_t), ctx->stream));
        if (round_words && acc_before + acc_round > w0) CR_TRY(consume(w0, w1));
        while (acc_before + acc_round < w1) {
            acc_before += acc_round;
            acc_round = 0;
            round_words = std::min(words_wanted(total - acc_before), raw_words);
            {
                std::optional<CrTimer> tm;
                if (timed) tm.emplace(ctx, CRGPU_T_SYNTH, round_words);
                hipLaunchKernelGGL(k_mt19937<false>, dim3(1), dim3(256), 0, ctx->stream, state.as<uint32_t>(), raw.as<uint32_t>(),
                                   round_words / MT_CHUNK);
                CR_HIP(ctx, hipGetLastError());
            }
            words_made += round_words;
            CR_TRY(consume(w0, w1));
            CR_REQUIRE(ctx, acc_round > 0, CRGPU_EHIP, "%s: a generator round of %llu words held no draw", who,
                       (unsigned long long)round_words);
        }
        std::optional<CrTimer> tm;
        if (timed) tm.emplace(ctx, CRGPU_T_SCAN, w1 - w0);
        hipLaunchKernelGGL(k_om_row_scan, dim3(s1 - s0), dim3(256), 0, ctx->stream, hist.as<uint32_t>(), N);
        CR_HIP(ctx, hipGetLastError());
        return CRGPU_OK;
    }
};

struct OmSelFlag {
    const uint32_t *pos;
    uint32_t top_n;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return pos[i] < top_n; }
};
struct OmSelEmit {
    const uint32_t *col;
    uint64_t *out;
    struct Pre {
        uint32_t c;
    };
    __device__ __forceinline__ Pre pre(uint64_t i) const { return Pre{col[i]}; }
    __device__ __forceinline__ void operator()(uint64_t, uint32_t o, Pre p) const { out[o] = p.c; }
};

static inline int64_t om_round_i64(double x) { return (int64_t)std::nearbyint(x); }  // np.round: half to even

// summarize_bootstrapped_top_n (:832-861) on the host; sorted totals are read from the device where the loop looks at them
static int om_summarize(crgpu_ctx *ctx, crgpu_ordmag_result *res, const uint32_t *d_sorted, uint64_t N) {
    const int S = CRGPU_ORDMAG_SAMPLES;
    double sum = 0.0;
    for (int i = 0; i < S; i++) sum += (double)res->top_n_boot[i];
    const double mean = sum / S;
    double sq = 0.0;
    for (int i = 0; i < S; i++) {
        const double d = (double)res->top_n_boot[i] - mean;
        sq += d * d;
    }
    const double var = sq / S, sd = std::sqrt(var);
    res->filtered_bcs_mean = mean;
    res->filtered_bcs_var = var;
    res->filtered_bcs_cv = mean == 0.0 ? 0.0 : sd / mean;
    // scipy's norm.ppf(q, loc, scale) = loc + scale * ppf(q), NaN for scale == 0
    const double nan = std::nan("");
    res->filtered_bcs_lb = sd > 0.0 ? std::nearbyint(mean + sd * -1.9599639845400545) : nan;
    res->filtered_bcs_ub = sd > 0.0 ? std::nearbyint(mean + sd * 1.959963984540054) : nan;
    const int64_t nbcs = om_round_i64(mean);
    res->filtered_bcs = nbcs;
    if (nbcs <= 0) return CRGPU_OK;
    // the loop steps from place nbcs - 1 while the total there equals the cutoff, and gives up once it took more than
    // 0.20 * nbcs: it never looks beyond place nbcs - 1 + floor(0.2 * nbcs) + 1
    const uint64_t first = (uint64_t)nbcs - 1;
    const uint64_t last = std::min<uint64_t>(N, (uint64_t)nbcs + (uint64_t)(0.20 * (double)nbcs) + 2);
    std::vector<uint32_t> win(last - first);
    CR_TRY(crgpu_memcpy_d2h(ctx, win.data(), d_sorted + first, win.size() * sizeof(uint32_t)));
    const uint32_t cutoff = win[0];
    uint64_t index = first;
    while (index + 1 < N && win[index - first] == cutoff) {
        index++;
        if ((double)(index + 1 - (uint64_t)nbcs) > 0.20 * (double)nbcs) return CRGPU_OK;
        res->filtered_bcs = (int64_t)(index + 1);
        res->filtered_bcs_cutoff = cutoff;
        res->filtered_bcs_cutoff_set = 1;
    }
    return CRGPU_OK;
}

extern "C" int crgpu_call_cells_ordmag_dev(crgpu_ctx *ctx, const uint32_t *d_bc_counts, uint64_t V, int64_t recovered_cells,
                                           int64_t max_expected_cells, int64_t force_cells, crgpu_ordmag_result *res,
                                           uint64_t **d_cell_cols, uint64_t *n_cells) {
    if (!ctx || !res || !d_cell_cols || !n_cells) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    memset(res, 0, sizeof(*res));
    *d_cell_cols = nullptr;
    *n_cells = 0;
    CR_REQUIRE(ctx, V == 0 || d_bc_counts, CRGPU_EINVAL, "crgpu_call_cells_ordmag_dev: NULL counts");
    CR_REQUIRE(ctx, V < 0x80000000ull, CRGPU_ERANGE, "crgpu_call_cells_ordmag_dev: at most 2^31 - 1 columns");
    const bool estimate = force_cells <= 0 && recovered_cells <= 0;
    CR_REQUIRE(ctx, !estimate || (max_expected_cells >= 2 && max_expected_cells <= (1ll << 30)), CRGPU_EINVAL,
               "crgpu_call_cells_ordmag_dev: max_expected_cells must be 2 .. 2^30 to estimate the recovered cells");
    if (!V) return CRGPU_OK;
    const int S = CRGPU_ORDMAG_SAMPLES;
    uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL;

    // 1. nonzero_bc_counts with their columns
    DevBuf nzv_b, nzc_b;
    CR_TRY(dmalloc(ctx, nzv_b, V * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, nzc_b, V * sizeof(uint32_t)));
    uint32_t *nzv = nzv_b.as<uint32_t>(), *nzc = nzc_b.as<uint32_t>(), N = 0;
    CR_TRY(compact(ctx, OmNzFlag{d_bc_counts}, OmNzEmit{d_bc_counts, nzv, nzc}, V, ctx->d_sort_hist, d_total));
    CR_TRY(read_u32(ctx, d_total, &N));
    res->n_nonzero = N;
    if (!N) return CRGPU_OK;  // "allowing no bcs through": metrics stay zero

    // 2. one descending sort: sorted[p], pos[i]
    DevBuf key_b, keyt_b, val_b, valt_b, sorted_b, pos_b;
    for (DevBuf *b : {&key_b, &keyt_b, &val_b, &valt_b, &sorted_b, &pos_b}) CR_TRY(dmalloc(ctx, *b, (uint64_t)N * sizeof(uint32_t)));
    uint32_t *sorted = sorted_b.as<uint32_t>(), *pos = pos_b.as<uint32_t>();
    {
        hipLaunchKernelGGL(k_om_keys, dim3(cr_grid(N, 256)), dim3(256), 0, ctx->stream, nzv, N, key_b.as<uint32_t>(), val_b.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
        bool in_tmp = false;
        CR_TRY(cr_radix_sort_u32(ctx, key_b.as<uint32_t>(), keyt_b.as<uint32_t>(), val_b.as<uint32_t>(), valt_b.as<uint32_t>(), N, 0, 32,
                                 &in_tmp));
        hipLaunchKernelGGL(k_om_places, dim3(cr_grid(N, 256)), dim3(256), 0, ctx->stream,
                           in_tmp ? keyt_b.as<uint32_t>() : key_b.as<uint32_t>(), in_tmp ? valt_b.as<uint32_t>() : val_b.as<uint32_t>(), N,
                           sorted, pos);
        CR_HIP(ctx, hipGetLastError());
    }

    uint64_t top_n = 0;
    if (force_cells > 0) {
        // filter_cellular_barcodes_fixed_cutoff: the cutoff is the total at descending place top_n of ALL columns
        top_n = std::min<uint64_t>((uint64_t)force_cells, N);
        res->filtered_bcs = (int64_t)top_n;
        res->filtered_bcs_mean = res->filtered_bcs_lb = res->filtered_bcs_ub = (double)top_n;
        if (top_n < N) {
            uint32_t c = 0;
            CR_TRY(read_u32(ctx, sorted + top_n, &c));
            res->filtered_bcs_cutoff = c;
        }
        res->filtered_bcs_cutoff_set = top_n < V;  // places N .. V-1 hold the zeros
    } else {
        OmBootstrap boot{ctx};
        CR_TRY(boot.init(N, estimate ? 2 * S : S, pos, sorted));
        DevBuf out_i_b, out_d_b;
        CR_TRY(dmalloc(ctx, out_i_b, S * sizeof(long long)));
        CR_TRY(dmalloc(ctx, out_d_b, S * sizeof(double)));
        long long *out_i = out_i_b.as<long long>();
        double *out_d = out_d_b.as<double>();
        const double one_minus_q = 1 - 0.99;  // ORDMAG_RECOVERED_CELLS_QUANTILE; not 0.01
        uint32_t s_base = 0;
        if (estimate) {
            std::vector<int64_t> rc;
            om_candidates(max_expected_cells, rc);
            std::vector<uint32_t> bidx(rc.size());
            for (size_t k = 0; k < rc.size(); k++)
                bidx[k] = (uint32_t)std::min<int64_t>(om_round_i64((double)rc[k] * one_minus_q), (int64_t)N - 1);
            DevBuf rc_b, bidx_b;
            CR_TRY(dmalloc(ctx, rc_b, rc.size() * sizeof(int64_t)));
            CR_TRY(dmalloc(ctx, bidx_b, rc.size() * sizeof(uint32_t)));
            CR_TRY(crgpu_memcpy_h2d(ctx, rc_b.p, rc.data(), rc.size() * sizeof(int64_t)));
            CR_TRY(crgpu_memcpy_h2d(ctx, bidx_b.p, bidx.data(), bidx.size() * sizeof(uint32_t)));
            for (uint32_t s0 = 0; s0 < (uint32_t)S; s0 += boot.B) {
                const uint32_t s1 = std::min<uint32_t>(S, s0 + boot.B);
                CR_TRY(boot.fill(s0, s1));
                hipLaunchKernelGGL(k_om_estimate, dim3(s1 - s0), dim3(256), 0, ctx->stream, boot.hist.as<uint32_t>(), sorted, N,
                                   rc_b.as<long long>(), bidx_b.as<uint32_t>(), (uint32_t)rc.size(), out_i + s0, out_d + s0);
                CR_HIP(ctx, hipGetLastError());
            }
            static_assert(sizeof(long long) == sizeof(int64_t), "");
            CR_TRY(crgpu_memcpy_d2h(ctx, res->recovered_boot, out_i, S * sizeof(int64_t)));
            CR_TRY(crgpu_memcpy_d2h(ctx, res->loss_boot, out_d, S * sizeof(double)));
            double sum = 0.0;
            for (int i = 0; i < S; i++) sum += (double)res->recovered_boot[i];
            recovered_cells = om_round_i64(sum / S);
            res->estimated = 1;
            s_base = S;
        }
        recovered_cells = std::max<int64_t>(recovered_cells, 50);  // MIN_RECOVERED_CELLS_PER_GEM_GROUP
        res->recovered_cells = recovered_cells;
        const int64_t b = std::min<int64_t>(om_round_i64((double)recovered_cells * one_minus_q), (int64_t)N - 1);
        res->baseline_bc_idx = b;
        for (uint32_t s0 = 0; s0 < (uint32_t)S; s0 += boot.B) {
            const uint32_t s1 = std::min<uint32_t>(S, s0 + boot.B);
            CR_TRY(boot.fill(s_base + s0, s_base + s1));
            hipLaunchKernelGGL(k_om_top_n, dim3(1), dim3(256), 0, ctx->stream, boot.hist.as<uint32_t>(), sorted, N, (uint32_t)b, s1 - s0,
                               out_i + s0);
            CR_HIP(ctx, hipGetLastError());
        }
        CR_TRY(crgpu_memcpy_d2h(ctx, res->top_n_boot, out_i, S * sizeof(int64_t)));
        CR_TRY(om_summarize(ctx, res, sorted, N));
        top_n = (uint64_t)res->filtered_bcs;
        CR_REQUIRE(ctx, top_n <= N, CRGPU_EHIP, "cell call: %llu barcodes called of %u non-zero ones", (unsigned long long)top_n, N);
    }

    // 3. the called columns, ascending
    uint64_t *d_cols = nullptr;
    CR_TRY(cr_pool_alloc(ctx, (void **)&d_cols, (top_n ? top_n : 1) * sizeof(uint64_t)));
    int rc = compact(ctx, OmSelFlag{pos, (uint32_t)top_n}, OmSelEmit{nzc, d_cols}, N, ctx->d_sort_hist, d_total);
    if (rc == CRGPU_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = cr_fail(ctx, CRGPU_EHIP, "cell call: selection failed");
    if (rc != CRGPU_OK) {
        cr_pool_free(ctx, d_cols);
        return rc;
    }
    *d_cell_cols = d_cols;
    *n_cells = top_n;
    return CRGPU_OK;
}

__global__ __launch_bounds__(256) void k_cell_ranks(const uint32_t *__restrict__ rank, uint64_t V, const uint64_t *__restrict__ cols,
                                                    uint64_t n, uint32_t *__restrict__ out, uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const uint64_t c = cols[k];
        if (c < V) out[k] = rank[c]; else *flag = 1u;
    }
}

extern "C" int crgpu_cell_ranks_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint64_t *d_cell_cols, uint64_t n_cells,
                                    uint32_t *d_ranks_out) {
    if (!ctx || !m) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    if (!n_cells) return CRGPU_OK;
    CR_REQUIRE(ctx, d_cell_cols && d_ranks_out, CRGPU_EINVAL, "crgpu_cell_ranks_dev: NULL argument");
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_cell_ranks, dim3(cr_grid(n_cells, 256)), dim3(256), 0, ctx->stream, m->d_barcode_rank, m->n_barcodes, d_cell_cols,
                       n_cells, d_ranks_out, d_flag);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !flag, CRGPU_EINVAL, "crgpu_cell_ranks_dev: a column is out of range");
    return CRGPU_OK;
}
