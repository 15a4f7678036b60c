// batch_correction.hip -- CORRECT_CHEMISTRY_BATCH on the device: the mutual nearest neighbours of a batch pair (host) and the
// Gaussian-kernel-weighted correction of the rows of a merged panorama, a whole merge schedule per call (the hot path).
//
// Replaces correction_vector (lib/python/cellranger/analysis/batch_correction.py:162-200) and the loop of join() around it
// (mro/rna/stages/analyzer/correct_chemistry_batch/__init__.py:277-355).  The neighbour query of the stage is crgpu_knn_cross_dev
// (knn.hip).  For a cur row c and a pair p of a step, with gamma = 0.5 * sigma as the reference has it:
//     y_p = x[mnn_cur[p]],  b_p = x[mnn_ref[p]] - y_p,  w_cp = exp((-gamma) * d2(x_c, y_p)),
//     d2 = the sum over t = 0 .. d - 1 of (x_t - y_t) * (x_t - y_t), in that order, f64, unfused (knn.hip's),
//     num_ct = the sum over p of w_cp * b_pt,  den_c = the sum over p of w_cp,  corr_ct = num_ct / den_c.
// The pairs are cut into chunks of CRGPU_BC_PAIR_CHUNK consecutive pairs: within a chunk both sums run left to right from 0.0, the
// chunks' partials are then added left to right.  No tile, no seam, no other row and no run moves a bit of corr.
// QUIRK kept (it is numpy's): a row whose weights all underflow gets 0 / 0 = NaN; no maximum is subtracted in the exponent.
//
// Launch structure, per step.
//   k_bc_gather      Y[p] = x[mnn_cur[p]], B[p] = x[mnn_ref[p]] - Y[p], n_mnn x d each.
//   k_bc_accumulate  a workgroup per (tile of R cur rows, pair chunk).  The tile's rows sit transposed in LDS.  Tiles of P pairs: Y
//                    goes to LDS; phase 1: a thread takes one row and BC_PP pairs at a time, so that one read of a row's coordinate
//                    serves BC_PP pairs, and writes the weights to LDS; B goes to LDS over Y; phase 2: a thread owns BC_RR rows
//                    by up to BC_TD dimensions (t = dg, dg + 1024 / R, ...) in registers and walks the tile's pairs in ascending
//                    order: one read of b_pt serves BC_RR rows, the 32 or more lanes of a row group read consecutive doubles, the
//                    weights are a broadcast.  The chunk's partial num[d] and den go to a slab with plain stores.
//                    LDS: (R d + P d + P R) doubles <= 72 KiB, two workgroups per CU at d = 128 (R = 32, P = 32).
//   k_bc_finish      a thread per (row, dimension): the chunks in order, the division.
//   k_bc_apply       x[cur_rows] += corr, after every corr of the step is there.
// No floating-point atomic anywhere; the only atomic counts the rows with den == 0 (u64).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "common.h"

#define BC_WG 256u
#define BC_PP 4u               // pairs of a thread per read of a coordinate (phase 1)
#define BC_RR 4u               // rows of a thread (phase 2)
#define BC_TD 8u               // dimensions of a thread at the most (phase 2): d <= 128 over 1024 / R >= 16 groups
#define BC_LDS_BYTES 73728u    // 72 KiB: two workgroups in the CU's 160 KiB
#define BC_MAX_PAIR_TILE 64u
#define BC_SLAB_BYTES (1ull << 30)

struct BcShape {
    uint32_t d, R, P, n_rows, n_mnn, n_tiles;
    double neg_gamma;
};

// ---- host: the mutual nearest neighbours of a batch pair -------------------------------------------------------------------------
extern "C" int crgpu_mnn_pairs(const int32_t *a, uint64_t n_i, uint64_t start_i, const int32_t *b, uint64_t n_j, uint64_t start_j, uint32_t k,
                               int32_t *pairs_out, uint64_t capacity, uint64_t *n_pairs_out, uint64_t *n_first_out, uint64_t *n_second_out) {
    if (!a || !b || !n_pairs_out || !n_first_out || !n_second_out || k == 0 || n_i == 0 || n_j == 0) return CRGPU_EINVAL;
    if (start_i + n_i > (1ull << 31) || start_j + n_j > (1ull << 31) || start_i >= (1ull << 31) || start_j >= (1ull << 31)) return CRGPU_EINVAL;
    const int64_t lo_i = (int64_t)start_i, hi_i = lo_i + (int64_t)n_i, lo_j = (int64_t)start_j, hi_j = lo_j + (int64_t)n_j;
    for (uint64_t e = 0; e < n_i * k; e++)
        if (a[e] < lo_j || a[e] >= hi_j) return CRGPU_EINVAL;
    for (uint64_t e = 0; e < n_j * k; e++)
        if (b[e] < lo_i || b[e] >= hi_i) return CRGPU_EINVAL;
    std::vector<uint8_t> second(n_j, 0);
    std::vector<int32_t> qs;
    uint64_t n_pairs = 0, n_first = 0, n_second = 0;
    for (uint64_t p = 0; p < n_i; p++) {
        const int32_t gp = (int32_t)(lo_i + (int64_t)p);
        qs.clear();
        for (uint32_t e = 0; e < k; e++) {
            const int32_t q = a[p * k + e];
            const int32_t *back = b + (uint64_t)(q - lo_j) * k;
            if (std::find(back, back + k, gp) != back + k) qs.push_back(q);
        }
        std::sort(qs.begin(), qs.end());
        qs.erase(std::unique(qs.begin(), qs.end()), qs.end());  // the reference's pairs are a set
        n_first += qs.empty() ? 0 : 1;
        for (int32_t q : qs) {
            if (pairs_out && n_pairs < capacity) pairs_out[2 * n_pairs] = gp, pairs_out[2 * n_pairs + 1] = q;
            n_pairs++;
            uint8_t &seen = second[(uint64_t)(q - lo_j)];
            n_second += seen ? 0 : 1;
            seen = 1;
        }
    }
    *n_pairs_out = n_pairs, *n_first_out = n_first, *n_second_out = n_second;
    return pairs_out && n_pairs > capacity ? CRGPU_EINVAL : CRGPU_OK;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BC_WG) void k_bc_gather(const double *__restrict__ x, const int32_t *__restrict__ mnn_cur, const int32_t *__restrict__ mnn_ref,
                                                     uint32_t n_mnn, uint32_t d, double *__restrict__ Y, double *__restrict__ B) {
    const uint64_t total = (uint64_t)n_mnn * d;
    for (uint64_t e = (uint64_t)blockIdx.x * BC_WG + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BC_WG) {
        const uint32_t p = (uint32_t)(e / d), t = (uint32_t)(e % d);
        const double y = x[(size_t)mnn_cur[p] * d + t];
        Y[e] = y;
        B[e] = x[(size_t)mnn_ref[p] * d + t] - y;
    }
}

// Dynamic LDS, in this order: the cur rows transposed (d * R doubles), the pair tile (P * d: Y, then B), the weights (P * R).
// cur_rows: the n_rows rows of this launch; slab_num [chunk][n_rows][d], slab_den [chunk][n_rows].
__global__ __launch_bounds__(BC_WG) void k_bc_accumulate(const double *__restrict__ x, const int32_t *__restrict__ cur_rows, const double *__restrict__ Y,
                                                         const double *__restrict__ B, BcShape s, double *__restrict__ slab_num,
                                                         double *__restrict__ slab_den) {
    extern __shared__ double bc_lds[];
    const uint32_t tid = threadIdx.x, d = s.d, R = s.R, P = s.P;
    double *s_x = bc_lds;
    double *s_yb = s_x + (size_t)R * d;
    double *s_w = s_yb + (size_t)P * d;
    const uint32_t tile = blockIdx.x % s.n_tiles, chunk = blockIdx.x / s.n_tiles, r0 = tile * R;
    for (uint32_t e = tid; e < R * d; e += BC_WG) {
        const uint32_t rl = e / d, t = e % d;
        const uint32_t c = r0 + rl < s.n_rows ? r0 + rl : s.n_rows - 1u;  // a row beyond the list computes on the last one and stores nothing
        s_x[t * R + rl] = x[(size_t)cur_rows[c] * d + t];
    }
    // phase 1: row1, and the pairs g1 * BC_PP .. + BC_PP - 1, then G * BC_PP further on
    const uint32_t G = BC_WG / R, row1 = tid % R, g1 = tid / R;
    // phase 2: the rows rg * BC_RR .. + BC_RR - 1, the dimensions dg, dg + dgn, ...
    const uint32_t dgn = BC_RR * BC_WG / R, dg = tid % dgn, rg = tid / dgn, ntd = (d + dgn - 1u) / dgn;
    double num[BC_RR][BC_TD], den[BC_RR];
#pragma unroll
    for (uint32_t r = 0; r < BC_RR; r++) {
        den[r] = 0.0;
#pragma unroll
        for (uint32_t j = 0; j < BC_TD; j++) num[r][j] = 0.0;
    }
    const uint32_t p_lo = chunk * CRGPU_BC_PAIR_CHUNK, p_hi = s.n_mnn - p_lo < CRGPU_BC_PAIR_CHUNK ? s.n_mnn : p_lo + CRGPU_BC_PAIR_CHUNK;
    for (uint32_t p0 = p_lo; p0 < p_hi; p0 += P) {
        const uint32_t m = p_hi - p0 < P ? p_hi - p0 : P;
        __syncthreads();  // the rows are there; the previous tile is done with
        for (uint32_t e = tid; e < m * d; e += BC_WG) s_yb[e] = Y[(size_t)p0 * d + e];
        __syncthreads();
        for (uint32_t pb = g1 * BC_PP; pb < m; pb += G * BC_PP) {
            double a[BC_PP];
            uint32_t off[BC_PP];
#pragma unroll
            for (uint32_t u = 0; u < BC_PP; u++) a[u] = 0.0, off[u] = (pb + u < m ? pb + u : m - 1u) * d;
            for (uint32_t t = 0; t < d; t++) {
                const double xv = s_x[t * R + row1];
#pragma unroll
                for (uint32_t u = 0; u < BC_PP; u++) {
                    const double v = xv - s_yb[off[u] + t];
                    a[u] += v * v;
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < BC_PP; u++)
                if (pb + u < m) s_w[(pb + u) * R + row1] = exp(s.neg_gamma * a[u]);
        }
        __syncthreads();  // the weights are there, Y is done with
        for (uint32_t e = tid; e < m * d; e += BC_WG) s_yb[e] = B[(size_t)p0 * d + e];
        __syncthreads();
        for (uint32_t p = 0; p < m; p++) {
            double w[BC_RR];
#pragma unroll
            for (uint32_t r = 0; r < BC_RR; r++) w[r] = s_w[p * R + rg * BC_RR + r], den[r] += w[r];
#pragma unroll
            for (uint32_t j = 0; j < BC_TD; j++)
                if (j < ntd) {
                    const uint32_t t = dg + j * dgn;
                    const double bv = s_yb[p * d + (t < d ? t : d - 1u)];
#pragma unroll
                    for (uint32_t r = 0; r < BC_RR; r++) num[r][j] += w[r] * bv;
                }
        }
    }
#pragma unroll
    for (uint32_t r = 0; r < BC_RR; r++) {
        const uint32_t c = r0 + rg * BC_RR + r;
        if (c >= s.n_rows) continue;
        const size_t at = (size_t)chunk * s.n_rows + c;
#pragma unroll
        for (uint32_t j = 0; j < BC_TD; j++) {
            const uint32_t t = dg + j * dgn;
            if (j < ntd && t < d) slab_num[at * d + t] = num[r][j];
        }
        if (dg == 0u) slab_den[at] = den[r];
    }
}

__global__ __launch_bounds__(BC_WG) void k_bc_finish(const double *__restrict__ slab_num, const double *__restrict__ slab_den, uint32_t n_rows, uint32_t d,
                                                     uint32_t n_chunks, double *__restrict__ corr, unsigned long long *__restrict__ zero_den) {
    const uint64_t total = (uint64_t)n_rows * d;
    for (uint64_t e = (uint64_t)blockIdx.x * BC_WG + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BC_WG) {
        const uint32_t c = (uint32_t)(e / d), t = (uint32_t)(e % d);
        double num = 0.0, den = 0.0;
        for (uint32_t ch = 0; ch < n_chunks; ch++) {
            const size_t at = (size_t)ch * n_rows + c;
            num += slab_num[at * d + t];
            den += slab_den[at];
        }
        corr[e] = num / den;
        if (t == 0u && den == 0.0) atomicAdd(zero_den, 1ull);
    }
}

__global__ __launch_bounds__(BC_WG) void k_bc_apply(double *__restrict__ x, const int32_t *__restrict__ cur_rows, uint32_t n_cur, uint32_t d,
                                                    const double *__restrict__ corr) {
    const uint64_t total = (uint64_t)n_cur * d;
    for (uint64_t e = (uint64_t)blockIdx.x * BC_WG + threadIdx.x; e < total; e += (uint64_t)gridDim.x * BC_WG) {
        const uint32_t c = (uint32_t)(e / d), t = (uint32_t)(e % d);
        x[(size_t)cur_rows[c] * d + t] += corr[e];
    }
}

// ---- the entry point -------------------------------------------------------------------------------------------------------------
// device time of what was enqueued since BC_BEGIN, added to *acc; waits for it
#define BC_BEGIN(ctx, ev) CR_HIP(ctx, hipEventRecord((ev)[0], (ctx)->stream))
#define BC_END(ctx, ev, acc)                                         \
    do {                                                             \
        float _ms = 0.0f;                                            \
        CR_HIP(ctx, hipGetLastError());                              \
        CR_HIP(ctx, hipEventRecord((ev)[1], (ctx)->stream));         \
        CR_HIP(ctx, hipEventSynchronize((ev)[1]));                   \
        CR_HIP(ctx, hipEventElapsedTime(&_ms, (ev)[0], (ev)[1]));    \
        (acc) += _ms;                                                \
    } while (0)

// the largest pair tile, a multiple of 8 up to BC_MAX_PAIR_TILE, that fits BC_LDS_BYTES beside R rows; 0 = none
static uint32_t bc_pair_tile_max(uint32_t d, uint32_t R) {
    const uint32_t have = BC_LDS_BYTES / 8u, rows = R * d;
    if (rows >= have) return 0u;
    return std::min(BC_MAX_PAIR_TILE, ((have - rows) / (d + R)) & ~7u);
}

extern "C" int crgpu_batch_correct_dev(crgpu_ctx *ctx, const double *x, uint64_t n, uint32_t d, uint64_t ld, double sigma, const crgpu_bc_step *steps,
                                       uint32_t n_steps, double *x_out, const crgpu_bc_args *a, crgpu_bc_result *res) {
    if (!ctx || !x || !x_out || !a || !res || (n_steps && !steps)) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    // every refusal below comes before the device is touched
    CR_REQUIRE(ctx, n >= 1 && n < (1ull << 31), CRGPU_EINVAL, "crgpu_batch_correct_dev: %llu rows, 1 to 2^31 - 1", (unsigned long long)n);
    CR_REQUIRE(ctx, d >= 1 && d <= CRGPU_KM_MAX_D && ld >= d, CRGPU_EINVAL, "crgpu_batch_correct_dev: %u dimensions (1 to %u) in rows of %llu", d,
               CRGPU_KM_MAX_D, (unsigned long long)ld);
    CR_REQUIRE(ctx, std::isfinite(sigma) && sigma >= 0.0, CRGPU_EINVAL, "crgpu_batch_correct_dev: sigma = %g, finite and not negative", sigma);
    const uint32_t R = a->row_tile ? a->row_tile : 32u;
    CR_REQUIRE(ctx, R == 16u || R == 32u || R == 64u, CRGPU_EINVAL, "crgpu_batch_correct_dev: a row tile of %u rows, 16, 32 or 64", R);
    const uint32_t tile_max = bc_pair_tile_max(d, R);
    const uint32_t P = a->pair_tile ? a->pair_tile : tile_max;
    CR_REQUIRE(ctx, tile_max >= 8u && P >= 8u && P <= tile_max && P % 8u == 0u, CRGPU_EINVAL,
               "crgpu_batch_correct_dev: a pair tile of %u pairs, a multiple of 8 up to %u for %u dimensions and %u rows", P, tile_max, d, R);
    CR_REQUIRE(ctx, a->slab_rows % R == 0u && a->reserved == 0u, CRGPU_EINVAL, "crgpu_batch_correct_dev: slab_rows is a multiple of the row tile, reserved 0");
    uint64_t sum_cur = 0, sum_mnn = 0, max_cur = 0, max_mnn = 0, pairs_evaluated = 0, chunks = 0;
    {
        std::vector<uint32_t> stamp(n, 0u);
        for (uint32_t st = 0; st < n_steps; st++) {
            const crgpu_bc_step &q = steps[st];
            CR_REQUIRE(ctx, q.cur_rows && q.mnn_cur && q.mnn_ref, CRGPU_EINVAL, "crgpu_batch_correct_dev: step %u lacks a list", st);
            CR_REQUIRE(ctx, q.n_cur >= 1 && q.n_cur <= n && q.n_mnn >= 1 && q.n_mnn < (1ull << 31), CRGPU_EINVAL,
                       "crgpu_batch_correct_dev: step %u has %llu cur rows and %llu pairs", st, (unsigned long long)q.n_cur, (unsigned long long)q.n_mnn);
            for (uint64_t i = 0; i < q.n_cur; i++) {
                const int32_t r = q.cur_rows[i];
                CR_REQUIRE(ctx, r >= 0 && (uint64_t)r < n, CRGPU_EINVAL, "crgpu_batch_correct_dev: step %u, cur_rows[%llu] = %d outside the rows", st,
                           (unsigned long long)i, r);
                CR_REQUIRE(ctx, stamp[r] != st + 1u, CRGPU_EINVAL, "crgpu_batch_correct_dev: step %u, row %d twice in cur_rows", st, r);
                stamp[r] = st + 1u;
            }
            for (uint64_t i = 0; i < q.n_mnn; i++)
                CR_REQUIRE(ctx, q.mnn_cur[i] >= 0 && (uint64_t)q.mnn_cur[i] < n && q.mnn_ref[i] >= 0 && (uint64_t)q.mnn_ref[i] < n, CRGPU_EINVAL,
                           "crgpu_batch_correct_dev: step %u, pair %llu outside the rows", st, (unsigned long long)i);
            sum_cur += q.n_cur, sum_mnn += q.n_mnn;
            max_cur = std::max(max_cur, q.n_cur), max_mnn = std::max(max_mnn, q.n_mnn);
            pairs_evaluated += q.n_cur * q.n_mnn;
            chunks += (q.n_mnn + CRGPU_BC_PAIR_CHUNK - 1u) / CRGPU_BC_PAIR_CHUNK;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<double> xp((size_t)n * d);  // the first d columns, packed; an infinity or a NaN is refused
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t t = 0; t < d; t++) {
            const double v = x[i * ld + t];
            CR_REQUIRE(ctx, std::isfinite(v), CRGPU_EINVAL, "crgpu_batch_correct_dev: x[%llu, %u] is not finite", (unsigned long long)i, t);
            xp[i * d + t] = v;
        }
    res->fit_ms = res->upload_ms = res->download_ms = res->gather_ms = res->accumulate_ms = res->finish_ms = res->apply_ms = 0.0;
    res->pairs_evaluated = pairs_evaluated, res->chunks = chunks, res->zero_den_rows = 0, res->pair_tile = P, res->row_tile = R;
    if (n_steps == 0) {  // nothing moves: the matrix as it came
        std::memcpy(x_out, xp.data(), xp.size() * sizeof(double));
        res->fit_ms = cr_ms_since(t0);
        return CRGPU_OK;
    }
    // the lists of all steps, one behind the other
    std::vector<int32_t> h_cur(sum_cur), h_mc(sum_mnn), h_mr(sum_mnn);
    {
        uint64_t ac = 0, am = 0;
        for (uint32_t st = 0; st < n_steps; st++) {
            const crgpu_bc_step &q = steps[st];
            std::copy(q.cur_rows, q.cur_rows + q.n_cur, h_cur.begin() + ac);
            std::copy(q.mnn_cur, q.mnn_cur + q.n_mnn, h_mc.begin() + am);
            std::copy(q.mnn_ref, q.mnn_ref + q.n_mnn, h_mr.begin() + am);
            ac += q.n_cur, am += q.n_mnn;
        }
    }
    // rows whose partials a launch keeps: what BC_SLAB_BYTES hold for the step with the most chunks, whole row tiles, at least one
    const uint64_t max_chunks = (max_mnn + CRGPU_BC_PAIR_CHUNK - 1u) / CRGPU_BC_PAIR_CHUNK;
    uint64_t slab_rows = a->slab_rows ? a->slab_rows : std::max<uint64_t>(R, BC_SLAB_BYTES / (max_chunks * (d + 1u) * sizeof(double)) / R * R);
    slab_rows = std::min<uint64_t>(slab_rows, (max_cur + R - 1u) / R * R);
    const size_t lds = ((size_t)R * d + (size_t)P * d + (size_t)P * R) * sizeof(double);

    DevBuf x_b, cur_b, mc_b, mr_b, y_b, b_b, corr_b, num_b, den_b, ctr_b;
    CR_TRY(dmalloc(ctx, x_b, xp.size() * sizeof(double)));
    CR_TRY(dmalloc(ctx, cur_b, sum_cur * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, mc_b, sum_mnn * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, mr_b, sum_mnn * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, y_b, max_mnn * d * sizeof(double)));
    CR_TRY(dmalloc(ctx, b_b, max_mnn * d * sizeof(double)));
    CR_TRY(dmalloc(ctx, corr_b, max_cur * d * sizeof(double)));
    CR_TRY(dmalloc(ctx, num_b, max_chunks * slab_rows * d * sizeof(double)));
    CR_TRY(dmalloc(ctx, den_b, max_chunks * slab_rows * sizeof(double)));
    CR_TRY(dmalloc(ctx, ctr_b, sizeof(uint64_t)));
    const auto t_up = std::chrono::steady_clock::now();
    CR_TRY(crgpu_memcpy_h2d(ctx, x_b.p, xp.data(), xp.size() * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, cur_b.p, h_cur.data(), sum_cur * sizeof(int32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, mc_b.p, h_mc.data(), sum_mnn * sizeof(int32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, mr_b.p, h_mr.data(), sum_mnn * sizeof(int32_t)));
    CR_HIP(ctx, hipMemsetAsync(ctr_b.p, 0, sizeof(uint64_t), ctx->stream));
    res->upload_ms = cr_ms_since(t_up);

    CrEvents<2> events(ctx);
    hipEvent_t *ev = events.e;
    cr_allow_lds(ctx, (const void *)k_bc_accumulate, lds);
    uint64_t ac = 0, am = 0;
    for (uint32_t st = 0; st < n_steps; st++) {
        const crgpu_bc_step &q = steps[st];
        const uint32_t n_cur = (uint32_t)q.n_cur, n_mnn = (uint32_t)q.n_mnn, n_chunks = (n_mnn + CRGPU_BC_PAIR_CHUNK - 1u) / CRGPU_BC_PAIR_CHUNK;
        const int32_t *d_cur = cur_b.as<int32_t>() + ac;
        double ms[4] = {0.0, 0.0, 0.0, 0.0};
        BC_BEGIN(ctx, ev);
        hipLaunchKernelGGL(k_bc_gather, dim3(cr_grid((uint64_t)n_mnn * d, BC_WG)), dim3(BC_WG), 0, ctx->stream, x_b.as<double>(), mc_b.as<int32_t>() + am,
                           mr_b.as<int32_t>() + am, n_mnn, d, y_b.as<double>(), b_b.as<double>());
        BC_END(ctx, ev, ms[0]);
        for (uint64_t row0 = 0; row0 < n_cur; row0 += slab_rows) {
            BcShape s;
            s.d = d, s.R = R, s.P = P, s.n_rows = (uint32_t)std::min<uint64_t>(slab_rows, n_cur - row0), s.n_mnn = n_mnn;
            s.n_tiles = (s.n_rows + R - 1u) / R, s.neg_gamma = -(0.5 * sigma);
            BC_BEGIN(ctx, ev);
            hipLaunchKernelGGL(k_bc_accumulate, dim3(s.n_tiles * n_chunks), dim3(BC_WG), lds, ctx->stream, x_b.as<double>(), d_cur + row0, y_b.as<double>(),
                               b_b.as<double>(), s, num_b.as<double>(), den_b.as<double>());
            BC_END(ctx, ev, ms[1]);
            BC_BEGIN(ctx, ev);
            hipLaunchKernelGGL(k_bc_finish, dim3(cr_grid((uint64_t)s.n_rows * d, BC_WG)), dim3(BC_WG), 0, ctx->stream, num_b.as<double>(), den_b.as<double>(),
                               s.n_rows, d, n_chunks, corr_b.as<double>() + row0 * d, ctr_b.as<unsigned long long>());
            BC_END(ctx, ev, ms[2]);
        }
        BC_BEGIN(ctx, ev);  // every corr of the step comes from the matrix as it stood: the rows move only now
        hipLaunchKernelGGL(k_bc_apply, dim3(cr_grid((uint64_t)n_cur * d, BC_WG)), dim3(BC_WG), 0, ctx->stream, x_b.as<double>(), d_cur, n_cur, d,
                           corr_b.as<double>());
        BC_END(ctx, ev, ms[3]);
        if (q.corr_out) {
            const auto t_dn = std::chrono::steady_clock::now();
            CR_TRY(crgpu_memcpy_d2h(ctx, q.corr_out, corr_b.p, (uint64_t)n_cur * d * sizeof(double)));
            res->download_ms += cr_ms_since(t_dn);
        }
        res->gather_ms += ms[0], res->accumulate_ms += ms[1], res->finish_ms += ms[2], res->apply_ms += ms[3];
        if (res->step_ms_out) std::copy(ms, ms + 4, res->step_ms_out + 4 * (size_t)st);
        ac += q.n_cur, am += q.n_mnn;
    }
    const auto t_dn = std::chrono::steady_clock::now();
    uint64_t zero_den = 0;
    CR_TRY(crgpu_memcpy_d2h(ctx, &zero_den, ctr_b.p, sizeof(zero_den)));
    CR_TRY(crgpu_memcpy_d2h(ctx, x_out, x_b.p, xp.size() * sizeof(double)));
    res->download_ms += cr_ms_since(t_dn);
    res->zero_den_rows = zero_den;
    res->fit_ms = cr_ms_since(t0);
    return CRGPU_OK;
}
