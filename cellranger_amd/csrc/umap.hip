// umap.hip -- RUN_UMAP on the device: the fuzzy kNN graph (rho, the sigma search, the union of both directions, the prune) and the
// sampled epochs of the layout; on the host the fit of the curve 1 / (1 + a x^(2b)).
//
// The stage (lib/rust/cr_ana/src/stages/umap.rs, mro/rna/sc_rna_analyzer.mro) calls the crate umap-rs, whose source the reference does
// not carry; what is here is the published algorithm (McInnes et al., as umap-learn states it) with the layout in a per-epoch batch
// form, restated in include/crgpu.h and in tests/umap_numpy.py.  All of it f64, unfused.
//
// Launch structure.
//   k_umap_rows        a lane per row: the row's distance sum left to right over the ranks, rho = the first distance > 0
//   k_colparts / k_colfinal   (graph_common.h) the total of the row sums over partials of 256 rows, left to right, then the partials
//                      ascending
//   k_umap_search      a lane per row: the search for sigma over the row's k distances, the floor, the k memberships
//   k_pair_keys        (graph_common.h) two keys per neighbour pair, i * n + j and j * n + i, the pair's number as payload; one radix sort
//   compaction         the first of a run of equal keys is emitted: (a + b) - a * b with the other direction's membership or 0
//   k_umap_maxparts / k_umap_maxfinal   wmax and the prune threshold wmax / n_epochs (a maximum has no order)
//   compaction         the entries at or above the threshold; k_keys_to_csr (graph_common.h) by search
//   k_umap_schedule    epoch 0: eps = wmax / w, the two states start at eps and eps / rate
//   k_umap_epoch       one epoch: walks a row's CSR entries left to right, adds the terms of the active ones (the attraction, then the
//                      negative samples in ascending order) and writes y + alpha * delta into a second Y; a lane per row below
//                      wave_row_len entries, a wave per row from it on (the lanes compute 64 terms, which are then added in term order)
// An epoch is the two launches of k_umap_epoch and nothing else: every term is taken from Y as it stood at the epoch's start (Jacobi
// over vertices), so the step is a pure function (Y, state, epoch) -> (Y', state').  No scatter, no atomic, no graph capture, no
// cooperative launch, and the host reads nothing inside the loop.
// QUIRK kept: a row that is its own neighbour (Context.knn keeps a row whose exact duplicate of lower index took the first place) gives
// the entry (i, i), which is scheduled and draws its negative samples like any other and whose attraction is 0.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "graph_common.h"
#include "philox.h"

#define UMAP_WG 256u
#define UMAP_MAX_STEPS 64u    // steps of the search at the most
#define UMAP_TOL 1e-5
#define UMAP_FLOOR 1e-3       // umap-learn's MIN_K_DIST_SCALE
#define UMAP_SLOTS CRGPU_UMAP_SLOTS

// ---- the fuzzy graph -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(UMAP_WG) void k_umap_rows(const double *__restrict__ dist, uint32_t n, uint32_t k, double *__restrict__ rho_out,
                                                       double *__restrict__ rowsum) {
    const uint32_t i = blockIdx.x * UMAP_WG + threadIdx.x;
    if (i >= n) return;
    const double *d = dist + (size_t)i * k;
    double s = 0.0, rho = 0.0;
    for (uint32_t m = 0; m < k; m++) {
        s += d[m];
        rho = (rho == 0.0 && d[m] > 0.0) ? d[m] : rho;  // the first distance > 0 by rank
    }
    rho_out[i] = rho, rowsum[i] = s;
}
// sigma_out[i] = max(the search's mid, 1e-3 * m), steps_out[i] = evaluations of psum, memb[i * k + m] = the membership of rank m.
// den_row = k + 1, den_all = n (k + 1), both exact in f64
__global__ __launch_bounds__(UMAP_WG) void k_umap_search(const double *__restrict__ dist, const double *__restrict__ rho_in, const double *__restrict__ rowsum,
                                                         const double *__restrict__ total, uint32_t n, uint32_t k, double target, double den_row,
                                                         double den_all, double *__restrict__ sigma_out, uint32_t *__restrict__ steps_out,
                                                         double *__restrict__ memb) {
    const uint32_t i = blockIdx.x * UMAP_WG + threadIdx.x;
    if (i >= n) return;
    const double *d = dist + (size_t)i * k;
    const double rho = rho_in[i];
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    uint32_t steps = 0;
    while (steps < UMAP_MAX_STEPS) {
        double psum = 0.0;
        for (uint32_t m = 0; m < k; m++) {
            const double x = d[m] - rho;
            psum += x > 0.0 ? exp(-(x / mid)) : 1.0;
        }
        steps++;
        if (fabs(psum - target) < UMAP_TOL) break;
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            mid = hi == INFINITY ? mid * 2.0 : (lo + hi) / 2.0;
        }
    }
    const double m = rho > 0.0 ? rowsum[i] / den_row : total[0] / den_all, floor_at = UMAP_FLOOR * m;
    const double sigma = mid < floor_at ? floor_at : mid;
    sigma_out[i] = sigma;
    steps_out[i] = steps;
    for (uint32_t r = 0; r < k; r++) {
        const double x = d[r] - rho;
        memb[(size_t)i * k + r] = (x <= 0.0 || sigma == 0.0) ? 1.0 : exp(-(x / sigma));
    }
}

// A key occurs once per direction at the most (a row's neighbours are distinct), so a run has one or two members; (a + b) - a * b is
// commutative, so the order of the two does not reach the value and (i, j) and (j, i) carry the same bits.
struct UmapEmitUnion {
    const uint64_t *keys;
    const uint32_t *perm;
    const double *memb;
    uint64_t n2;
    uint64_t *ckeys;
    double *values;
    struct Pre {};
    __device__ __forceinline__ Pre pre(uint64_t) const { return Pre(); }
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t o, Pre) const {
        const uint64_t key = keys[i];
        const double a = memb[perm[i] >> 1];
        const double b = (i + 1 < n2 && keys[i + 1] == key) ? memb[perm[i + 1] >> 1] : 0.0;
        ckeys[o] = key;
        values[o] = (a + b) - a * b;
    }
};
// parts[block] = the largest of the block's share of v
__global__ __launch_bounds__(UMAP_WG) void k_umap_maxparts(const double *__restrict__ v, uint64_t nnz, double *__restrict__ parts) {
    __shared__ double ws[UMAP_WG / 64u];
    double m = 0.0;
    for (uint64_t e = (uint64_t)blockIdx.x * UMAP_WG + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * UMAP_WG) m = fmax(m, v[e]);
    m = wave_max(m);
    if ((threadIdx.x & 63u) == 0u) ws[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < UMAP_WG / 64u; w++) m = fmax(m, ws[w]);
        parts[blockIdx.x] = m;
    }
}
// out[0] = wmax, out[1] = wmax / n_epochs: the prune threshold
__global__ __launch_bounds__(64) void k_umap_maxfinal(const double *__restrict__ parts, uint32_t n_parts, double n_epochs, double *__restrict__ out) {
    if (threadIdx.x) return;
    double m = 0.0;
    for (uint32_t p = 0; p < n_parts; p++) m = fmax(m, parts[p]);
    out[0] = m, out[1] = m / n_epochs;
}
struct UmapKeepFlag {  // an entry at or above the threshold stays
    const double *values, *scal;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return values[i] >= scal[1]; }
};
struct UmapEmitKept {
    const uint64_t *ckeys;
    const double *values;
    uint64_t *keys_out;
    double *values_out;
    struct Pre {};
    __device__ __forceinline__ Pre pre(uint64_t) const { return Pre(); }
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t o, Pre) const { keys_out[o] = ckeys[i], values_out[o] = values[i]; }
};

// ---- the epochs ----------------------------------------------------------------------------------------------------------------------
struct UmapStep {
    double a, b, m2ab, g2b;  // m2ab = (-2.0 * a) * b, g2b = (2.0 * gamma) * b, the host's products
    double alpha, wmax, rate, nd;  // nd = the absolute epoch as f64
    uint64_t seed, epoch;
    uint32_t n, thr;
};
__global__ __launch_bounds__(UMAP_WG) void k_umap_schedule(const double *__restrict__ values, uint64_t nnz, double wmax, double rate,
                                                           double *__restrict__ eons, double *__restrict__ eonns) {
    for (uint64_t e = (uint64_t)blockIdx.x * UMAP_WG + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * UMAP_WG) {
        const double eps = wmax / values[e];
        eons[e] = eps, eonns[e] = eps / rate;
    }
}
// The entry's turn in epoch s.nd: 0 when it is not active, else 1 + n_neg; both states move on.
// n_neg <= 2 rate - 1 <= 15 < UMAP_SLOTS.  The first activation is at the first n >= eps, so n < eps + 1 and, with eonns = epns =
// eps / rate, (n - epns) / epns < rate + rate / eps - 1 <= 2 rate - 1 (eps >= 1).  Afterwards eonns is the largest multiple of epns
// not above the epoch of the last activation, eons a multiple of epns not above it either, so eonns >= eons - eps; the next
// activation is at n' < eons + 1, and (n' - eonns) / epns < (eps + 1) / epns = rate + rate / eps <= 2 rate.  A caller's state that
// asks for more takes UMAP_SLOTS, the words the entry owns in the epoch's stream.
__device__ __forceinline__ uint32_t umap_turn(double *__restrict__ eons, double *__restrict__ eonns, const double *__restrict__ values, uint64_t e,
                                              const UmapStep &s) {
    const double eo = eons[e];
    if (!(eo <= s.nd)) return 0u;
    const double eps = s.wmax / values[e], epns = eps / s.rate, en = eonns[e];
    const double f = floor((s.nd - en) / epns);
    const uint32_t n_neg = f >= (double)UMAP_SLOTS ? UMAP_SLOTS : (f > 0.0 ? (uint32_t)f : 0u);
    eons[e] = eo + eps;
    eonns[e] = en + (double)n_neg * epns;
    return 1u + n_neg;
}
__device__ __forceinline__ double umap_clip(double x) { return x > 4.0 ? 4.0 : (x < -4.0 ? -4.0 : x); }
// word q of the epoch's stream (philox.h's numbering) modulo n
__device__ __forceinline__ uint32_t umap_sample(const UmapStep &s, uint64_t q) {
    unsigned long long w[4];
    cr_philox4x64_10(1ull + (q >> 2), s.epoch, s.seed, w);
    const uint32_t r = (uint32_t)(q & 3ull);
    const unsigned long long word = r == 0u ? w[0] : (r == 1u ? w[1] : (r == 2u ? w[2] : w[3]));
    return (uint32_t)(word % (unsigned long long)s.n);
}
// The term of row i (at yi) against the vertex `other`: the attraction of an entry, doubled for the tail-side move of its twin, or a
// negative sample.  A sample of the row itself has v = 0 and adds +0.0, which moves no bit: it contributes nothing.
template <uint32_t DIMS>
__device__ __forceinline__ void umap_term(const double *__restrict__ Y, const double *yi, uint32_t other, bool attract, const UmapStep &s, double *term) {
    double v[DIMS], d2 = 0.0;
#pragma unroll
    for (uint32_t t = 0; t < DIMS; t++) {
        v[t] = yi[t] - Y[(size_t)other * DIMS + t];
        d2 += v[t] * v[t];
    }
    double c = 0.0;
    if (d2 > 0.0) {
        const double p = pow(d2, s.b), den = s.a * p + 1.0;
        c = attract ? (s.m2ab * (p / d2)) / den : s.g2b / ((0.001 + d2) * den);
    }
#pragma unroll
    for (uint32_t t = 0; t < DIMS; t++) {
        const double x = umap_clip(c * v[t]);
        term[t] = attract ? 2.0 * x : x;
    }
}
// counts[2 i], counts[2 i + 1] += the active entries and the negative samples of row i; delta_out (or NULL) = the row's delta.
// A row belongs to the launch with WAVE = (its entries >= s.thr).
template <uint32_t DIMS, bool WAVE>
__global__ __launch_bounds__(UMAP_WG) void k_umap_epoch(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                        const double *__restrict__ values, const double *__restrict__ Y, UmapStep s,
                                                        double *__restrict__ eons, double *__restrict__ eonns, double *__restrict__ Ynew,
                                                        double *__restrict__ delta_out, unsigned long long *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t gtid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, gsize = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t first = WAVE ? gtid >> 6 : gtid, stride = WAVE ? gsize >> 6 : gsize;
    for (uint64_t i = first; i < s.n; i += stride) {
        const uint64_t a = (uint64_t)indptr[i], b = (uint64_t)indptr[i + 1];
        if (((b - a) >= s.thr) != WAVE) continue;  // uniform in a wave when WAVE
        double yi[DIMS], delta[DIMS], term[DIMS];
#pragma unroll
        for (uint32_t t = 0; t < DIMS; t++) yi[t] = Y[i * DIMS + t], delta[t] = 0.0;
        unsigned long long n_act = 0, n_neg = 0;
        if (WAVE) {
            for (uint64_t e0 = a; e0 < b; e0 += 64u) {
                const uint64_t e = e0 + lane;
                const uint32_t cnt = e < b ? umap_turn(eons, eonns, values, e, s) : 0u;
                const uint32_t incl = wave_incl_scan(cnt, lane), excl = incl - cnt, T = (uint32_t)__shfl((int)incl, 63);
                n_act += cnt ? 1u : 0u, n_neg += cnt ? cnt - 1u : 0u;
                // the terms of the 64 entries in (entry, attraction, then sample) order, 64 at a time, a lane a term
                for (uint32_t q0 = 0; q0 < T; q0 += 64u) {
                    const uint32_t q = q0 + lane;
                    uint32_t owner = 0;  // the last lane whose terms start at or before q: an entry without a term starts where the next does
#pragma unroll
                    for (uint32_t step = 32u; step; step >>= 1) {
                        const uint32_t at = (uint32_t)__shfl((int)excl, (int)(owner + step));
                        owner = at <= q ? owner + step : owner;
                    }
                    const uint32_t slot = q - (uint32_t)__shfl((int)excl, (int)owner);
#pragma unroll
                    for (uint32_t t = 0; t < DIMS; t++) term[t] = 0.0;  // a lane past the end adds +0.0, which moves no bit
                    if (q < T) {
                        const uint64_t eo = e0 + owner;
                        const uint32_t other = slot == 0u ? (uint32_t)indices[eo] : umap_sample(s, eo * UMAP_SLOTS + (slot - 1u));
                        umap_term<DIMS>(Y, yi, other, slot == 0u, s, term);
                    }
                    const int m = (int)(T - q0 < 64u ? T - q0 : 64u);
                    for (int l = 0; l < m; l++) {
#pragma unroll
                        for (uint32_t t = 0; t < DIMS; t++) delta[t] += __shfl(term[t], l);
                    }
                }
            }
            n_act = wave_sum(n_act), n_neg = wave_sum(n_neg);
            if (lane != 0u) continue;
        } else {
            for (uint64_t e = a; e < b; e++) {
                const uint32_t cnt = umap_turn(eons, eonns, values, e, s);
                if (!cnt) continue;
                n_act += 1u, n_neg += cnt - 1u;
                umap_term<DIMS>(Y, yi, (uint32_t)indices[e], true, s, term);
#pragma unroll
                for (uint32_t t = 0; t < DIMS; t++) delta[t] += term[t];
                for (uint32_t k = 0; k + 1u < cnt; k++) {
                    umap_term<DIMS>(Y, yi, umap_sample(s, e * UMAP_SLOTS + k), false, s, term);
#pragma unroll
                    for (uint32_t t = 0; t < DIMS; t++) delta[t] += term[t];
                }
            }
        }
#pragma unroll
        for (uint32_t t = 0; t < DIMS; t++) {
            Ynew[i * DIMS + t] = yi[t] + s.alpha * delta[t];
            if (delta_out) delta_out[i * DIMS + t] = delta[t];
        }
        counts[2 * i] += n_act, counts[2 * i + 1] += n_neg;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
static void umap_clear(crgpu_umap_result *r) {
    r->wmax = r->fit_ms = r->search_ms = r->csr_ms = r->loop_ms = 0.0;
    r->nnz = r->n_active = r->n_negative = 0;
    r->wave_row_len = r->rows_per_wg = r->max_steps = r->reserved = 0;
}
template <uint32_t DIMS>
static void umap_launch_epoch(crgpu_ctx *ctx, uint32_t wg, const long long *indptr, const int32_t *indices, const double *values, const double *Y,
                              const UmapStep &st, double *eons, double *eonns, double *Ynew, double *delta, unsigned long long *counts) {
    hipLaunchKernelGGL((k_umap_epoch<DIMS, false>), dim3(cr_grid(st.n, wg)), dim3(wg), 0, ctx->stream, indptr, indices, values, Y, st, eons, eonns, Ynew,
                       delta, counts);
    hipLaunchKernelGGL((k_umap_epoch<DIMS, true>), dim3(cr_grid((uint64_t)st.n * 64u, wg)), dim3(wg), 0, ctx->stream, indptr, indices, values, Y, st, eons,
                       eonns, Ynew, delta, counts);
}

// ---- the entry points ----------------------------------------------------------------------------------------------------------------
// The least-squares fit of 1 / (1 + a x^(2b)) to umap-learn's curve at linspace(0, 3 spread, 300): Levenberg-Marquardt from (1, 1) with
// the 2 x 2 normal equations solved directly.  A step is taken when the cost does not rise by more than its own rounding (near the
// minimum the cost is flat to second order, so a strict comparison would stop at the square root of the precision); it ends when a
// taken step is below 1e-12 of the parameters.
extern "C" int crgpu_umap_ab(double min_dist, double spread, double *a_out, double *b_out) {
    if (!a_out || !b_out || !std::isfinite(min_dist) || !std::isfinite(spread) || min_dist < 0.0 || !(spread > 0.0)) return CRGPU_EINVAL;
    const int M = 300;
    double x[M], y[M], lx[M];
    const double stop = 3.0 * spread, step = stop / (double)(M - 1);
    for (int i = 0; i < M; i++) {
        x[i] = i == M - 1 ? stop : (double)i * step;  // numpy's linspace
        y[i] = x[i] < min_dist ? 1.0 : std::exp(-(x[i] - min_dist) / spread);
        lx[i] = x[i] > 0.0 ? std::log(x[i]) : 0.0;
    }
    auto cost_of = [&](double a, double b) {
        double c = 0.0;
        for (int i = 0; i < M; i++) {
            const double r = 1.0 / (1.0 + a * std::pow(x[i], 2.0 * b)) - y[i];
            c += r * r;
        }
        return c;
    };
    double a = 1.0, b = 1.0, lambda = 1e-3, cost = cost_of(a, b);
    for (int it = 0; it < 500; it++) {
        double A00 = 0.0, A01 = 0.0, A11 = 0.0, g0 = 0.0, g1 = 0.0;
        for (int i = 0; i < M; i++) {
            const double p = std::pow(x[i], 2.0 * b), f = 1.0 / (1.0 + a * p), r = f - y[i];
            const double ja = -(p * (f * f)), jb = x[i] > 0.0 ? -((a * p) * (2.0 * lx[i]) * (f * f)) : 0.0;
            A00 += ja * ja, A01 += ja * jb, A11 += jb * jb, g0 += ja * r, g1 += jb * r;
        }
        bool taken = false;
        double da = 0.0, db = 0.0, cn = cost;
        for (int tries = 0; tries < 60 && !taken; tries++) {
            const double B00 = A00 + lambda * A00, B11 = A11 + lambda * A11, det = B00 * B11 - A01 * A01;
            da = (-g0 * B11 + g1 * A01) / det, db = (-g1 * B00 + g0 * A01) / det;
            if (det > 0.0 && std::isfinite(da) && std::isfinite(db) && a + da > 0.0 && b + db > 0.0) {
                cn = cost_of(a + da, b + db);
                taken = cn <= cost + 1e-14 * cost;
            }
            lambda = taken ? std::max(lambda / 10.0, 1e-15) : lambda * 10.0;
        }
        if (!taken) break;
        const double rel = std::sqrt(da * da + db * db) / std::sqrt(a * a + b * b);
        a += da, b += db, cost = cn;
        if (rel < 1e-12) break;
    }
    *a_out = a, *b_out = b;
    return CRGPU_OK;
}

extern "C" int crgpu_umap_graph_dev(crgpu_ctx *ctx, const int32_t *nn_indices, const double *nn_distances, uint64_t n, uint32_t k, uint32_t n_epochs,
                                    crgpu_umap_result *res) {
    if (!ctx || !nn_indices || !nn_distances || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const char *who = "crgpu_umap_graph_dev";
    // every refusal below comes before the device is touched
    CR_REQUIRE(ctx, n >= 2 && n < (1ull << 31), CRGPU_EINVAL, "%s: %llu rows, 2 to 2^31 - 1", who, (unsigned long long)n);
    CR_REQUIRE(ctx, k >= 1 && k <= CRGPU_KNN_MAX_K && k < n, CRGPU_EINVAL, "%s: k = %u, 1 to min(%u, the %llu rows - 1)", who, k, CRGPU_KNN_MAX_K,
               (unsigned long long)n);
    CR_REQUIRE(ctx, n_epochs >= 1, CRGPU_EINVAL, "%s: %u epochs, at least 1", who, n_epochs);
    CR_REQUIRE(ctx, 2 * n * k < (1ull << 32), CRGPU_ERANGE, "%s: %llu neighbour pairs, fewer than 2^31", who, (unsigned long long)(n * k));
    CR_TRY(cr_check_knn_lists(ctx, who, nn_indices, nn_distances, n, k));
    const auto t0 = std::chrono::steady_clock::now();
    umap_clear(res);
    const uint64_t nk = n * k, n2 = 2 * nk, n_parts = (n + GRAPH_PART_ROWS - 1u) / GRAPH_PART_ROWS;
    const uint32_t max_blocks = 1024u;
    DevBuf nn_b, dist_b, rho_b, rowsum_b, sigma_b, steps_b, memb_b, keys_b, keyt_b, perm_b, permt_b, ckeys_b, val_b, kept_b, ind_b, ptr_b, block_b, parts_b, scal_b;
    CR_TRY(dmalloc(ctx, nn_b, nk * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, dist_b, nk * sizeof(double)));
    CR_TRY(dmalloc(ctx, rho_b, n * sizeof(double)));
    CR_TRY(dmalloc(ctx, rowsum_b, n * sizeof(double)));
    CR_TRY(dmalloc(ctx, sigma_b, n * sizeof(double)));
    CR_TRY(dmalloc(ctx, steps_b, n * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, memb_b, nk * sizeof(double)));
    CR_TRY(dmalloc(ctx, keys_b, n2 * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, keyt_b, n2 * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, perm_b, n2 * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, permt_b, n2 * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, ckeys_b, n2 * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, val_b, n2 * sizeof(double)));
    CR_TRY(dmalloc(ctx, kept_b, n2 * sizeof(double)));
    CR_TRY(dmalloc(ctx, ind_b, n2 * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, ptr_b, (n + 1) * sizeof(int64_t)));
    CR_TRY(dmalloc(ctx, block_b, 4100 * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, parts_b, std::max<uint64_t>(n_parts, max_blocks) * sizeof(double)));
    CR_TRY(dmalloc(ctx, scal_b, 4 * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, nn_b.p, nn_indices, nk * sizeof(int32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, dist_b.p, nn_distances, nk * sizeof(double)));
    double *d_total = scal_b.as<double>(), *d_wmax = scal_b.as<double>() + 2;  // d_wmax[0] = wmax, [1] = the threshold

    CrEvents<3> events(ctx);
    hipEvent_t *ev = events.e;
    const uint32_t row_grid = (uint32_t)((n + UMAP_WG - 1u) / UMAP_WG);
    CR_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    hipLaunchKernelGGL(k_umap_rows, dim3(row_grid), dim3(UMAP_WG), 0, ctx->stream, dist_b.as<double>(), (uint32_t)n, k, rho_b.as<double>(),
                       rowsum_b.as<double>());
    cr_colsums(ctx, rowsum_b.as<double>(), n, 1u, 1u, parts_b.as<double>(), d_total);
    hipLaunchKernelGGL(k_umap_search, dim3(row_grid), dim3(UMAP_WG), 0, ctx->stream, dist_b.as<double>(), rho_b.as<double>(), rowsum_b.as<double>(), d_total,
                       (uint32_t)n, k, std::log2((double)(k + 1u)), (double)(k + 1u), (double)n * (double)(k + 1u), sigma_b.as<double>(),
                       steps_b.as<uint32_t>(), memb_b.as<double>());
    CR_HIP(ctx, hipGetLastError());
    CR_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    cr_pair_keys(ctx, nn_b.as<int32_t>(), (uint32_t)n, k, keys_b.as<uint64_t>(), perm_b.as<uint32_t>());
    CR_HIP(ctx, hipGetLastError());
    SortedKeys sk;
    CR_TRY(cr_sort_keys(ctx, keys_b.as<uint64_t>(), keyt_b.as<uint64_t>(), perm_b.as<uint32_t>(), permt_b.as<uint32_t>(), n2, cr_ceil_log2(n * n), &sk));
    uint32_t merged32 = 0;
    CR_TRY(cr_merge_runs(ctx, sk.keys, UmapEmitUnion{sk.keys, sk.perm, memb_b.as<double>(), n2, ckeys_b.as<uint64_t>(), val_b.as<double>()}, n2,
                         block_b.as<uint32_t>(), nk, n2, who, "merged entries", &merged32));
    const uint64_t merged = merged32;
    uint32_t *d_count = block_b.as<uint32_t>() + 4096;
    const uint32_t max_grid = cr_grid(merged, UMAP_WG, max_blocks);
    hipLaunchKernelGGL(k_umap_maxparts, dim3(max_grid), dim3(UMAP_WG), 0, ctx->stream, val_b.as<double>(), merged, parts_b.as<double>());
    hipLaunchKernelGGL(k_umap_maxfinal, dim3(1), dim3(64), 0, ctx->stream, parts_b.as<double>(), max_grid, (double)n_epochs, d_wmax);
    CR_HIP(ctx, hipGetLastError());
    // the kept entries: their keys into the sort's spare buffer
    CR_TRY(compact(ctx, UmapKeepFlag{val_b.as<double>(), d_wmax}, UmapEmitKept{ckeys_b.as<uint64_t>(), val_b.as<double>(), sk.spare, kept_b.as<double>()},
                   merged, block_b.as<uint32_t>(), d_count));
    uint32_t nnz32 = 0;
    CR_TRY(read_u32(ctx, d_count, &nnz32));
    const uint64_t nnz = nnz32;
    CR_REQUIRE(ctx, nnz >= 1 && nnz <= merged, CRGPU_EHIP, "%s: %llu kept entries of %llu", who, (unsigned long long)nnz, (unsigned long long)merged);
    cr_keys_to_csr(ctx, sk.spare, nnz, (uint32_t)n, ptr_b.as<long long>(), ind_b.as<int32_t>(), nullptr);
    CR_HIP(ctx, hipGetLastError());
    CR_HIP(ctx, hipEventRecord(ev[2], ctx->stream));

    std::vector<uint32_t> steps(n);
    CR_TRY(crgpu_memcpy_d2h(ctx, steps.data(), steps_b.p, n * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, &res->wmax, d_wmax, sizeof(double)));
    if (res->rho_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->rho_out, rho_b.p, n * sizeof(double)));
    if (res->sigma_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->sigma_out, sigma_b.p, n * sizeof(double)));
    if (res->steps_out) std::copy(steps.begin(), steps.end(), res->steps_out);
    if (res->indptr_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->indptr_out, ptr_b.p, (n + 1) * sizeof(int64_t)));
    if (res->indices_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->indices_out, ind_b.p, nnz * sizeof(int32_t)));
    if (res->values_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->values_out, kept_b.p, nnz * sizeof(double)));
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms_a = 0.0f, ms_b = 0.0f;
    CR_HIP(ctx, hipEventElapsedTime(&ms_a, ev[0], ev[1]));
    CR_HIP(ctx, hipEventElapsedTime(&ms_b, ev[1], ev[2]));
    res->search_ms = ms_a, res->csr_ms = ms_b, res->nnz = nnz;
    res->max_steps = *std::max_element(steps.begin(), steps.end());
    res->fit_ms = cr_ms_since(t0);
    return CRGPU_OK;
}

extern "C" int crgpu_umap_epochs_dev(crgpu_ctx *ctx, const int64_t *indptr, const int32_t *indices, const double *values, uint64_t n, uint32_t dims,
                                     double *y, double *epoch_of_next_sample, double *epoch_of_next_negative_sample, const crgpu_umap_args *a,
                                     crgpu_umap_result *res) {
    if (!ctx || !indptr || !indices || !values || !y || !epoch_of_next_sample || !epoch_of_next_negative_sample || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const char *who = "crgpu_umap_epochs_dev";
    CR_REQUIRE(ctx, n >= 2 && n < (1ull << 31), CRGPU_EINVAL, "%s: %llu rows, 2 to 2^31 - 1", who, (unsigned long long)n);
    CR_REQUIRE(ctx, dims == 2u || dims == 3u, CRGPU_EINVAL, "%s: %u dimensions, 2 or 3", who, dims);
    CR_REQUIRE(ctx, std::isfinite(a->a) && a->a > 0.0 && std::isfinite(a->b) && a->b > 0.0, CRGPU_EINVAL, "%s: a = %g, b = %g, finite and positive", who, a->a,
               a->b);
    const double gamma = a->gamma == 0.0 ? 1.0 : a->gamma, alpha0 = a->initial_alpha == 0.0 ? 1.0 : a->initial_alpha;
    const uint32_t rate = a->negative_sample_rate ? a->negative_sample_rate : 5u, wg = a->rows_per_wg ? a->rows_per_wg : UMAP_WG;
    const uint32_t thr = a->wave_row_len ? a->wave_row_len : 32u;
    CR_REQUIRE(ctx, std::isfinite(gamma) && gamma > 0.0 && std::isfinite(alpha0) && alpha0 > 0.0, CRGPU_EINVAL,
               "%s: gamma = %g, initial_alpha = %g, finite and positive (0 = 1)", who, a->gamma, a->initial_alpha);
    CR_REQUIRE(ctx, rate >= 1u && rate <= CRGPU_UMAP_MAX_RATE, CRGPU_EINVAL, "%s: a negative sample rate of %u, 1 to %u (0 = 5)", who, rate, CRGPU_UMAP_MAX_RATE);
    CR_REQUIRE(ctx, a->n_epochs >= 1u && (uint64_t)a->first_epoch + a->n_run <= a->n_epochs, CRGPU_EINVAL, "%s: epochs %u + %u of %u", who, a->first_epoch,
               a->n_run, a->n_epochs);
    CR_REQUIRE(ctx, wg == 64u || wg == 128u || wg == 256u, CRGPU_EINVAL, "%s: %u rows of a workgroup, 64, 128 or 256", who, wg);
    CR_REQUIRE(ctx, a->reserved0 == 0u && a->reserved1 == 0u, CRGPU_EINVAL, "%s: reserved is 0", who);
    CR_TRY(cr_check_csr(ctx, who, indptr, indices, n, 59u, true));  // nnz * 16 < 2^63
    const uint64_t nnz = (uint64_t)indptr[n];
    double wmax = 0.0;
    for (uint64_t e = 0; e < nnz; e++) {
        CR_REQUIRE(ctx, std::isfinite(values[e]) && values[e] > 0.0, CRGPU_EINVAL, "%s: values[%llu] = %g, finite and positive", who, (unsigned long long)e,
                   values[e]);
        wmax = std::max(wmax, values[e]);
    }
    for (uint64_t e = 0; e < n * dims; e++) CR_REQUIRE(ctx, std::isfinite(y[e]), CRGPU_EINVAL, "%s: y[%llu] is not finite", who, (unsigned long long)e);
    if (a->first_epoch)
        for (uint64_t e = 0; e < nnz; e++)
            CR_REQUIRE(ctx, std::isfinite(epoch_of_next_sample[e]) && std::isfinite(epoch_of_next_negative_sample[e]), CRGPU_EINVAL,
                       "%s: the schedule state of entry %llu is not finite", who, (unsigned long long)e);
    const auto t0 = std::chrono::steady_clock::now();
    umap_clear(res);
    res->wmax = wmax, res->nnz = nnz, res->wave_row_len = thr, res->rows_per_wg = wg;

    const uint64_t yb = n * dims * sizeof(double), eb = std::max<uint64_t>(1, nnz) * sizeof(double);
    DevBuf ptr_b, ind_b, val_b, y0_b, y1_b, eons_b, eonns_b, delta_b, counts_b;
    CR_TRY(dmalloc(ctx, ptr_b, (n + 1) * sizeof(int64_t)));
    CR_TRY(dmalloc(ctx, ind_b, std::max<uint64_t>(1, nnz) * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, val_b, eb));
    CR_TRY(dmalloc(ctx, y0_b, yb));
    CR_TRY(dmalloc(ctx, y1_b, yb));
    CR_TRY(dmalloc(ctx, eons_b, eb));
    CR_TRY(dmalloc(ctx, eonns_b, eb));
    CR_TRY(dmalloc(ctx, delta_b, yb));
    CR_TRY(dmalloc(ctx, counts_b, 2 * n * sizeof(unsigned long long)));
    CR_TRY(crgpu_memcpy_h2d(ctx, ptr_b.p, indptr, (n + 1) * sizeof(int64_t)));
    if (nnz) {
        CR_TRY(crgpu_memcpy_h2d(ctx, ind_b.p, indices, nnz * sizeof(int32_t)));
        CR_TRY(crgpu_memcpy_h2d(ctx, val_b.p, values, nnz * sizeof(double)));
        if (a->first_epoch) {
            CR_TRY(crgpu_memcpy_h2d(ctx, eons_b.p, epoch_of_next_sample, nnz * sizeof(double)));
            CR_TRY(crgpu_memcpy_h2d(ctx, eonns_b.p, epoch_of_next_negative_sample, nnz * sizeof(double)));
        }
    }
    CR_TRY(crgpu_memcpy_h2d(ctx, y0_b.p, y, yb));
    CR_HIP(ctx, hipMemsetAsync(counts_b.p, 0, 2 * n * sizeof(unsigned long long), ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(delta_b.p, 0, yb, ctx->stream));

    CrEvents<3> events(ctx);
    CR_HIP(ctx, hipEventRecord(events.e[0], ctx->stream));
    if (nnz && !a->first_epoch)
        hipLaunchKernelGGL(k_umap_schedule, dim3(cr_grid(nnz, UMAP_WG)), dim3(UMAP_WG), 0, ctx->stream, val_b.as<double>(), nnz, wmax, (double)rate,
                           eons_b.as<double>(), eonns_b.as<double>());
    double *Y = y0_b.as<double>(), *Ynew = y1_b.as<double>();
    UmapStep st = {a->a, a->b, (-2.0 * a->a) * a->b, (2.0 * gamma) * a->b, 0.0, wmax, (double)rate, 0.0, a->seed, 0, (uint32_t)n, thr};
    for (uint32_t r = 0; r < a->n_run; r++) {
        st.epoch = (uint64_t)a->first_epoch + r, st.nd = (double)st.epoch;
        st.alpha = alpha0 * (1.0 - st.nd / (double)a->n_epochs);
        double *delta = res->delta_out && r + 1u == a->n_run ? delta_b.as<double>() : nullptr;
        if (dims == 2u)
            umap_launch_epoch<2>(ctx, wg, ptr_b.as<long long>(), ind_b.as<int32_t>(), val_b.as<double>(), Y, st, eons_b.as<double>(), eonns_b.as<double>(), Ynew,
                                 delta, counts_b.as<unsigned long long>());
        else
            umap_launch_epoch<3>(ctx, wg, ptr_b.as<long long>(), ind_b.as<int32_t>(), val_b.as<double>(), Y, st, eons_b.as<double>(), eonns_b.as<double>(), Ynew,
                                 delta, counts_b.as<unsigned long long>());
        std::swap(Y, Ynew);
    }
    CR_HIP(ctx, hipGetLastError());
    CR_HIP(ctx, hipEventRecord(events.e[1], ctx->stream));

    std::vector<unsigned long long> counts(2 * n);
    CR_TRY(crgpu_memcpy_d2h(ctx, y, Y, yb));
    if (nnz) {
        CR_TRY(crgpu_memcpy_d2h(ctx, epoch_of_next_sample, eons_b.p, nnz * sizeof(double)));
        CR_TRY(crgpu_memcpy_d2h(ctx, epoch_of_next_negative_sample, eonns_b.p, nnz * sizeof(double)));
    }
    if (res->delta_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->delta_out, delta_b.p, yb));
    CR_TRY(crgpu_memcpy_d2h(ctx, counts.data(), counts_b.p, 2 * n * sizeof(unsigned long long)));
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (uint64_t i = 0; i < n; i++) res->n_active += counts[2 * i], res->n_negative += counts[2 * i + 1];
    float ms = 0.0f;
    CR_HIP(ctx, hipEventElapsedTime(&ms, events.e[0], events.e[1]));
    res->loop_ms = ms;
    res->fit_ms = cr_ms_since(t0);
    return CRGPU_OK;
}
