// sseq.h -- sSeq differential expression of clusters: RUN_DIFFERENTIAL_EXPRESSION on the device (part of matrix_stages.hip).
//
// Replaces compute_sseq_params and sseq_differential_expression as the stage calls them (lib/rust/cr_ana/src/stages/diff_exp_stage.rs,
// lib/python/cellranger/analysis/diffexp.py): every cluster of a labelling against all other cells.  The reference takes its numerics
// from the external diff_exp crate, whose source is NOT in the reference tree; this file follows the published algorithm (Yu et al.
// 2013, Bioinformatics 29:1275) as the pure-Python diffexp.py of open-source Cell Ranger 3 had it, restated in include/crgpu.h and
// tests/sseq_numpy.py.  No parity with the crate is claimed.  What the reference tree does give is kept: estimate_size_factors,
// adjust_pvalue_bh, big_count = 900, the zeta quantile 0.995, the G x 3K layout.
//
// Parameters (once per matrix)   crgpu_matrix_dev_column_sums, the radix sort for the median; the entries keyed row * N + column and
//                                sorted (the transpose), then k_sq_row_sums: a wave per gene, lane l adds the gene's entries l, l + 64,
//                                ... in column order, the lanes are joined by a fixed tree -- an order that depends on the matrix alone,
//                                no floating-point atomic.  The G-vectors (phi_mm, the quantile, delta, phi) are host f64.
// Group sums (per labelling)     k_sq_group_sums: a wave per cell, u64 atomics into [cluster][gene]: integers, exact in any order.
// Exact tests (the hot path)     the terms of a test are w_i = exp(d_i), d_i = g(i, r_a) + g(T - i, r_b), g(k, r) = lgamma(r + k) -
//                                lgamma(k + 1): what lp(i; ...) + lp(T - i; ...) leaves when the factors that do not depend on i are
//                                dropped (log(m / (r + m)) is the same for both groups, the r log(r / (r + m)) and lgamma(r) are
//                                constants).  g is a pure function of (k, r), so d_i == d_(T - i) bit for bit when r_a == r_b.
//                                sq_lgdiff takes the difference of the two log-gammas analytically (Stirling with the large terms
//                                cancelled on paper), so its error scales with |g|, not with lgamma(70 000).
//                                ONE order of summation for every test: term i belongs to slot i % 256; a slot adds its terms in
//                                ascending i (a running maximum, both sums rescaled when it moves); the slots are joined as
//                                ((s, s + 64), (s + 128, s + 192)) and then by the tree 32, 16, 8, 4, 2, 1 over s.  Three kernels
//                                walk that one order: k_sq_exact_short (up to 16 terms: 16 lanes a test, four tests a wave),
//                                k_sq_exact_wave (a wave a test, four slots a lane), k_sq_exact_wg (a workgroup a test, a slot a
//                                thread).  So the class thresholds of crgpu_sseq_args change no bit of any result.
// Asymptotic tests               a lane per test: the regularised incomplete beta by its continued fraction (modified Lentz, the
//                                complement from x >= (a + 1) / (a + b + 2)), the prefactor with its large terms cancelled on paper,
//                                the median by bisection on the same function.
// Benjamini-Hochberg             per cluster the used genes' p-values (their bit patterns ascend with them) through the radix sort with
//                                the gene as payload, k_sq_bh_close: the running minimum from the largest p downwards, scattered back.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <vector>

#include "stage_common.h"

#define SQ_WG 256u
#define SQ_SHORT 16u           // terms of the short class at the most
#define SQ_WG_MIN_DEFAULT 4096u
#define SQ_BIG_COUNT 900ull
#define SQ_ZETA_QUANTILE 0.995
#define SQ_NOT_ASYMPTOTIC 255u

struct crgpu_sseq_params {
    uint64_t n_cells = 0;
    uint32_t n_features = 0, n_used = 0;
    double zeta_hat = 0.0, delta = 0.0;
    std::vector<double> sf, mean, var, phi_mm, phi;
    std::vector<uint8_t> use;
    double *d_sf = nullptr, *d_mean = nullptr, *d_phi = nullptr;  // the parameters stay on the device
};

struct SqTest {
    double ra, rb;       // s_a / phi, s_b / phi; with phi == 0 log(s_a), log(s_b)
    uint32_t xa, T, out, poisson;
};
struct SqBig {
    double alpha, beta;
    uint64_t xa, xb;
    uint32_t out, reserved;
};
struct SqAcc {
    double m, sn, sd;    // the largest d so far; the sums of exp(d - m) over the terms with d <= d_obs, over all terms
};

// ---- host: Benjamini-Hochberg ----------------------------------------------------------------------------------------------------------
extern "C" int crgpu_sseq_adjust_bh(const double *p, uint64_t n, double *q_out) {
    if ((!p || !q_out) && n) return CRGPU_EINVAL;
    std::vector<uint64_t> order(n);
    for (uint64_t i = 0; i < n; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return p[a] < p[b] || (p[a] == p[b] && a < b); });
    double run = INFINITY;
    for (uint64_t k = n; k >= 1; k--) {  // scale = float(n) / rank; np.minimum.accumulate from the largest p downwards
        const double v = ((double)n / (double)k) * p[order[k - 1]];
        run = v < run ? v : run;
        q_out[order[k - 1]] = run < 1.0 ? run : 1.0;
    }
    return CRGPU_OK;
}

// ---- device: log-gamma differences ----------------------------------------------------------------------------------------------------
// the tail of Stirling's series in 1 / z, z >= 16: the first term left out is 1 / (156 z^13) < 2e-18
__device__ __forceinline__ double sq_stirling(double iz) {
    const double w = iz * iz;
    return iz * (1.0 / 12.0 + w * (-1.0 / 360.0 + w * (1.0 / 1260.0 + w * (-1.0 / 1680.0 + w * (1.0 / 1188.0 + w * (-691.0 / 360360.0))))));
}
// lgamma(z1) - lgamma(z2) for z1, z2 > 0.  Arguments below 16 are raised by the recurrence (a product of at most 16 factors, one log).
// (z1 - 1/2) log z1 - (z2 - 1/2) log z2 - (z1 - z2) is taken as D log z1 + ((z2 - 1/2) log1p(D / z2) - D) with D = z1 - z2.
__device__ __forceinline__ double sq_lgdiff(double z1, double z2) {
    double p1 = 1.0, p2 = 1.0;
    for (uint32_t it = 0; it < 16u && z1 < 16.0; it++) p1 *= z1, z1 += 1.0;  // 16 steps at the most for an argument above 0
    for (uint32_t it = 0; it < 16u && z2 < 16.0; it++) p2 *= z2, z2 += 1.0;
    const double D = z1 - z2, i1 = 1.0 / z1, i2 = 1.0 / z2;
    double r = D * log(z1) + ((z2 - 0.5) * log1p(D * i2) - D) + (sq_stirling(i1) - sq_stirling(i2));
    if (p1 != 1.0 || p2 != 1.0) r += log(p2 / p1);
    return r;
}
// lgamma(z), z > 0
__device__ __forceinline__ double sq_lgamma(double z) {
    double p = 1.0;
    for (uint32_t it = 0; it < 16u && z < 16.0; it++) p *= z, z += 1.0;
    double r = (z - 0.5) * log(z) - z + 0.91893853320467274178 + sq_stirling(1.0 / z);
    if (p != 1.0) r -= log(p);
    return r;
}
// d_i up to what does not depend on i
__device__ __forceinline__ double sq_term(const SqTest &t, uint32_t i) {
    const double k = (double)i, j = (double)(t.T - i);
    if (t.poisson) return (k * t.ra - sq_lgamma(k + 1.0)) + (j * t.rb - sq_lgamma(j + 1.0));
    return sq_lgdiff(t.ra + k, k + 1.0) + sq_lgdiff(t.rb + j, j + 1.0);
}
__device__ __forceinline__ void sq_add_term(SqAcc &a, double d, double d_obs) {
    const double f = d <= d_obs ? 1.0 : 0.0;
    if (d <= a.m) {
        const double e = exp(d - a.m);
        a.sn += f * e, a.sd += e;
    } else {  // a.m == -inf on the first term: e == 0
        const double e = exp(a.m - d);
        a.sn = a.sn * e + f, a.sd = a.sd * e + 1.0, a.m = d;
    }
}
// a's terms come before b's; a state without terms (m == -inf) changes nothing
__device__ __forceinline__ SqAcc sq_merge(SqAcc a, SqAcc b) {
    if (b.m == -INFINITY) return a;
    if (a.m == -INFINITY) return b;
    if (b.m <= a.m) {
        const double e = exp(b.m - a.m);
        a.sn += b.sn * e, a.sd += b.sd * e;
        return a;
    }
    const double e = exp(a.m - b.m);
    b.sn = a.sn * e + b.sn, b.sd = a.sd * e + b.sd;
    return b;
}
// the tree over the lanes of a group of `width` lanes (64 or 16): lane l takes lane l + off, off = width / 2 .. 1; lane 0 holds the result
template <uint32_t WIDTH>
__device__ __forceinline__ SqAcc sq_lane_tree(SqAcc t, uint32_t lane_in_group) {
#pragma unroll
    for (uint32_t off = WIDTH / 2u; off >= 1u; off >>= 1) {
        SqAcc o;
        o.m = __shfl_down(t.m, off, WIDTH), o.sn = __shfl_down(t.sn, off, WIDTH), o.sd = __shfl_down(t.sd, off, WIDTH);
        if (lane_in_group + off < WIDTH) t = sq_merge(t, o);
    }
    return t;
}

// ---- exact tests ---------------------------------------------------------------------------------------------------------------------------
// up to 16 terms: slot l holds term l alone, every other slot is empty, the steps 32 and 16 of the tree join empty states
__global__ __launch_bounds__(SQ_WG) void k_sq_exact_short(const SqTest *__restrict__ tests, uint32_t n, double *__restrict__ p) {
    const uint32_t gid = (blockIdx.x * SQ_WG + threadIdx.x) / SQ_SHORT, l = threadIdx.x % SQ_SHORT;
    const bool live = gid < n;  // uniform over the 16 lanes
    SqTest t = tests[live ? gid : 0u];
    SqAcc a = {-INFINITY, 0.0, 0.0};
    if (live && l <= t.T) sq_add_term(a, sq_term(t, l), sq_term(t, t.xa));
    a = sq_lane_tree<SQ_SHORT>(a, l);
    if (live && l == 0u) p[t.out] = a.sn / a.sd;
}
// a wave a test: lane l holds the slots l, l + 64, l + 128, l + 192
__global__ __launch_bounds__(SQ_WG) void k_sq_exact_wave(const SqTest *__restrict__ tests, uint32_t n, double *__restrict__ p) {
    const uint32_t w = (blockIdx.x * SQ_WG + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (w >= n) return;  // uniform over the wave
    const SqTest t = tests[w];
    const double d_obs = sq_term(t, t.xa);
    SqAcc a[4];
#pragma unroll
    for (uint32_t u = 0; u < 4u; u++) a[u] = SqAcc{-INFINITY, 0.0, 0.0};
    for (uint64_t base = 0; base <= t.T; base += 256u) {
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) {
            const uint64_t i = base + 64u * u + lane;
            if (i <= t.T) sq_add_term(a[u], sq_term(t, (uint32_t)i), d_obs);
        }
    }
    SqAcc r = sq_lane_tree<64u>(sq_merge(sq_merge(a[0], a[1]), sq_merge(a[2], a[3])), lane);
    if (lane == 0u) p[t.out] = r.sn / r.sd;
}
// a workgroup a test: thread s holds slot s
__global__ __launch_bounds__(SQ_WG) void k_sq_exact_wg(const SqTest *__restrict__ tests, uint32_t n, double *__restrict__ p) {
    __shared__ SqAcc s_acc[SQ_WG];
    if (blockIdx.x >= n) return;
    const SqTest t = tests[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const double d_obs = sq_term(t, t.xa);
    SqAcc a = {-INFINITY, 0.0, 0.0};
    for (uint64_t i = tid; i <= t.T; i += SQ_WG) sq_add_term(a, sq_term(t, (uint32_t)i), d_obs);
    s_acc[tid] = a;
    __syncthreads();
    if (tid < 64u) {
        SqAcc r = sq_lane_tree<64u>(sq_merge(sq_merge(s_acc[tid], s_acc[tid + 64u]), sq_merge(s_acc[tid + 128u], s_acc[tid + 192u])), tid);
        if (tid == 0u) p[t.out] = r.sn / r.sd;
    }
}

// ---- asymptotic tests --------------------------------------------------------------------------------------------------------------------
// the continued fraction of the incomplete beta function, modified Lentz
__device__ double sq_betacf(double a, double b, double x) {
    const double tiny = 1e-300, qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (uint32_t m = 1; m <= 20000u; m++) {
        const double fm = (double)m, m2 = 2.0 * fm;
        double aa = fm * (b - fm) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + fm) * (qab + fm) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < 2e-16) break;
    }
    return h;
}
// log(x^a y^b / B(a, b)), y = 1 - x.  With a, b >= 16 Stirling's large terms are cancelled on paper: with x0 = a / (a + b)
// a log(x / x0) + b log(y / (1 - x0)) + log(a b / (2 pi (a + b))) / 2 + the series' tails
__device__ double sq_beta_log_prefix(double a, double b, double x, double y) {
    if (a < 16.0 || b < 16.0) return a * log(x) + b * log(y) - ((sq_lgamma(a) + sq_lgamma(b)) - sq_lgamma(a + b));
    const double s = a + b, x0 = a / s, y0 = b / s;
    const double dx = x - x0;
    const double main = a * log1p(dx / x0) + b * log1p(-dx / y0);
    return main + 0.5 * log(a * b / (6.283185307179586476925 * s)) + ((sq_stirling(1.0 / s) - sq_stirling(1.0 / a)) - sq_stirling(1.0 / b));
}
// I_x(a, b) with y = 1 - x given
__device__ double sq_betainc(double a, double b, double x, double y) {
    if (x <= 0.0) return 0.0;
    if (y <= 0.0) return 1.0;
    const double pre = exp(sq_beta_log_prefix(a, b, x, y));
    if (x < (a + 1.0) / (a + b + 2.0)) return pre * sq_betacf(a, b, x) / a;
    return 1.0 - pre * sq_betacf(b, a, y) / b;
}
__global__ __launch_bounds__(64) void k_sq_asymptotic(const SqBig *__restrict__ tests, uint32_t n, double *__restrict__ p, uint8_t *__restrict__ side) {
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const SqBig t = tests[i];
    const double T = (double)(t.xa + t.xb);
    double lo = 0.0, hi = 1.0;  // the median of Beta(alpha, beta)
    for (uint32_t it = 0; it < 60u; it++) {
        const double mid = 0.5 * (lo + hi);
        if (sq_betainc(t.alpha, t.beta, mid, 1.0 - mid) < 0.5) lo = mid; else hi = mid;
    }
    const double med = 0.5 * (lo + hi);
    const bool left = ((double)t.xa + 0.5) / T < med;
    // 1 - X ~ Beta(beta, alpha): the right side is the left side of the mirrored variable
    const double v = left ? sq_betainc(t.alpha, t.beta, ((double)t.xa + 0.5) / T, ((double)t.xb - 0.5) / T)
                          : sq_betainc(t.beta, t.alpha, ((double)t.xb + 0.5) / T, ((double)t.xa - 0.5) / T);
    p[t.out] = 2.0 * v;
    side[t.out] = left ? 1u : 0u;
}

// ---- the matrix passes ---------------------------------------------------------------------------------------------------------------
// key = row * N + column, value = the count; flag: a row >= G
__global__ __launch_bounds__(SQ_WG) void k_sq_keys(const long long *__restrict__ indptr, const int32_t *__restrict__ indices, const int32_t *__restrict__ data,
                                                   uint64_t N, uint32_t G, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t *__restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave0; c < N; c += n_waves) {
        const long long s = indptr[c], e = indptr[c + 1];
        for (long long i = s + lane; i < e; i += 64) {
            const uint32_t r = (uint32_t)indices[i];
            if (r >= G) {
                atomicOr(flag, 1u);
                keys[i] = 0ull, vals[i] = 0u;
            } else {
                keys[i] = (uint64_t)r * N + c, vals[i] = (uint32_t)data[i];
            }
        }
    }
}
// a wave per gene over its entries in column order: sum x / sf and sum (x / sf)^2
__global__ __launch_bounds__(SQ_WG) void k_sq_row_sums(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t nnz, uint64_t N, uint32_t G,
                                                       const double *__restrict__ sf, double *__restrict__ s1_out, double *__restrict__ s2_out) {
    const uint32_t g = (blockIdx.x * SQ_WG + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (g >= G) return;
    const uint64_t lo = cr_lower_bound(keys, nnz, (uint64_t)g * N), hi = cr_lower_bound(keys, nnz, ((uint64_t)g + 1u) * N);
    double s1 = 0.0, s2 = 0.0;
    for (uint64_t i = lo + lane; i < hi; i += 64u) {
        const double v = (double)vals[i] / sf[keys[i] - (uint64_t)g * N];
        s1 += v, s2 += v * v;
    }
    s1 = wave_sum(s1), s2 = wave_sum(s2);  // lane 0 of the butterfly adds what a __shfl_down tree adds, in its order
    if (lane == 0u) s1_out[g] = s1, s2_out[g] = s2;
}
// sums[label - 1][row] += count: a wave per cell
__global__ __launch_bounds__(SQ_WG) void k_sq_group_sums(const long long *__restrict__ indptr, const int32_t *__restrict__ indices, const int32_t *__restrict__ data,
                                                         uint64_t N, uint32_t G, const int32_t *__restrict__ labels, unsigned long long *__restrict__ sums) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave0; c < N; c += n_waves) {
        const long long s = indptr[c], e = indptr[c + 1];
        unsigned long long *row = sums + (size_t)(labels[c] - 1) * G;
        for (long long i = s + lane; i < e; i += 64) {
            const uint32_t r = (uint32_t)indices[i];
            if (r < G) atomicAdd(row + r, (unsigned long long)(uint32_t)data[i]);
        }
    }
}

// ---- Benjamini-Hochberg ---------------------------------------------------------------------------------------------------------------
// the used genes' p-values of cluster blockIdx.y as sort keys (a non-negative double's bit pattern ascends with it), the gene as payload
__global__ __launch_bounds__(SQ_WG) void k_sq_bh_keys(const double *__restrict__ p, uint32_t G, const uint32_t *__restrict__ used, uint32_t n_used,
                                                      uint64_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const uint32_t j = blockIdx.x * SQ_WG + threadIdx.x, c = blockIdx.y;
    if (j >= n_used) return;
    const uint32_t g = used[j];
    keys[(size_t)c * n_used + j] = (uint64_t)__double_as_longlong(p[(size_t)c * G + g]);
    vals[(size_t)c * n_used + j] = g;
}
// one workgroup per cluster: q[rank k] = min(1, min over the ranks j >= k of (n / j) p_j).  A minimum is the same in any order.
__global__ __launch_bounds__(SQ_WG) void k_sq_bh_close(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint32_t n_used, uint32_t G,
                                                       double *__restrict__ adj) {
    __shared__ double s_min[SQ_WG];
    const uint32_t tid = threadIdx.x;
    const uint64_t *k = keys + (size_t)blockIdx.x * n_used;
    const uint32_t *v = vals + (size_t)blockIdx.x * n_used;
    double *out = adj + (size_t)blockIdx.x * G;
    const uint32_t per = (n_used + SQ_WG - 1u) / SQ_WG, lo = tid * per < n_used ? tid * per : n_used, hi = lo + per < n_used ? lo + per : n_used;
    const double n = (double)n_used;
    double mn = INFINITY;
    for (uint32_t j = lo; j < hi; j++) {
        const double q = (n / (double)(j + 1u)) * __longlong_as_double((long long)k[j]);
        mn = q < mn ? q : mn;
    }
    s_min[tid] = mn;
    __syncthreads();
    double run = INFINITY;  // the minimum over the chunks behind this one
    for (uint32_t t = tid + 1u; t < SQ_WG; t++) run = s_min[t] < run ? s_min[t] : run;
    for (uint32_t j = hi; j > lo; j--) {
        const double q = (n / (double)j) * __longlong_as_double((long long)k[j - 1u]);
        run = q < run ? q : run;
        out[v[j - 1u]] = run < 1.0 ? run : 1.0;
    }
}

// ---- the host arithmetic of the parameters: crgpu_sseq_params_dev and crgpu_sseq_pair_dev (sseq_pair.h) share it, so that a pair of
// groups gets the bits the sub-matrix of its cells gets ----
// sf[c] = cnt[c] / median; returns S = sum 1 / sf in the order of cnt
static double sq_size_factors(const uint32_t *cnt, uint64_t N, double median, std::vector<double> &sf) {
    sf.resize(N);
    double S = 0.0;
    for (uint64_t c = 0; c < N; c++) {
        sf[c] = (double)cnt[c] / median;
        S += 1.0 / sf[c];
    }
    return S;
}
// the G-vectors (mean, var, use, phi_mm, the quantile, delta, phi) from the per-gene sums s1 = sum x / sf, s2 = sum (x / sf)^2;
// P.n_cells and P.n_features are set
static int sq_gene_params(crgpu_ctx *ctx, const char *who, crgpu_sseq_params &P, const std::vector<double> &s1, const std::vector<double> &s2, double S) {
    const uint32_t G = P.n_features;
    P.mean.resize(G), P.var.resize(G), P.phi_mm.assign(G, 0.0), P.phi.assign(G, std::nan("")), P.use.assign(G, 0);
    std::vector<double> pm;
    const double n = (double)P.n_cells;
    bool any_pos = false;
    for (uint32_t g = 0; g < G; g++) {
        const double mean = s1[g] / n, mean_sq = s2[g] / n, var = mean_sq - mean * mean;
        P.mean[g] = mean, P.var[g] = var;
        if (!(var > 0.0)) continue;
        P.use[g] = 1;
        const double v = (n * var - mean * S) / (mean * mean * S);
        P.phi_mm[g] = v > 0.0 ? v : 0.0;
        any_pos = any_pos || P.phi_mm[g] > 0.0;
        pm.push_back(P.phi_mm[g]);
    }
    P.n_used = (uint32_t)pm.size();
    CR_REQUIRE(ctx, !pm.empty(), CRGPU_EINVAL, "%s: no gene varies over the cells", who);
    std::vector<double> srt(pm);
    std::sort(srt.begin(), srt.end());
    P.zeta_hat = cr_quantile_sorted(srt, SQ_ZETA_QUANTILE);
    const double pm_mean = cr_pairwise_sum(pm.data(), pm.size()) / (double)pm.size();
    std::vector<double> q1(pm.size()), q2(pm.size());
    for (size_t i = 0; i < pm.size(); i++) q1[i] = (pm[i] - pm_mean) * (pm[i] - pm_mean), q2[i] = (pm[i] - P.zeta_hat) * (pm[i] - P.zeta_hat);
    const double num = cr_pairwise_sum(q1.data(), q1.size()) / (double)(G - 1u), den = cr_pairwise_sum(q2.data(), q2.size()) / (double)(G - 2u);
    // every phi_mm 0: the Python leaves delta 0 / 0 and sets phi to 0 (the Poisson limit); otherwise a zero denominator is refused
    CR_REQUIRE(ctx, !any_pos || den > 0.0, CRGPU_EINVAL, "%s: every moment dispersion equals the shrinkage target, delta is x / 0", who);
    P.delta = any_pos ? num / den : std::nan("");
    for (uint32_t g = 0; g < G; g++)
        if (P.use[g]) {
            P.phi[g] = any_pos ? (1.0 - P.delta) * P.phi_mm[g] + P.delta * P.zeta_hat : 0.0;
            // delta above 1 can push a gene below 0, where the negative binomial has no meaning (the Python goes on to NaN)
            CR_REQUIRE(ctx, P.phi[g] >= 0.0, CRGPU_EINVAL, "%s: the shrunken dispersion of gene %u is %g (delta = %g)", who, g, P.phi[g], P.delta);
        }
    return CRGPU_OK;
}

// ---- the entry points ----------------------------------------------------------------------------------------------------------------------
extern "C" void crgpu_sseq_params_free(crgpu_ctx *ctx, crgpu_sseq_params *p) {
    if (!p) return;
    if (ctx) {
        CR_ENTER(ctx);
        cr_pool_free(ctx, p->d_sf), cr_pool_free(ctx, p->d_mean), cr_pool_free(ctx, p->d_phi);
    }
    delete p;
}

extern "C" int crgpu_sseq_params_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const crgpu_sseq_args *a, crgpu_sseq_params **out) {
    if (!ctx || !m || !a || !out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *out = nullptr;
    const uint64_t N = m->n_barcodes, nnz = m->nnz;
    const uint32_t G = a->n_features;
    CR_REQUIRE(ctx, G >= 3, CRGPU_EINVAL, "crgpu_sseq_params_dev: %u features, at least 3", G);
    CR_REQUIRE(ctx, N >= 2 && N < (1ull << 31), CRGPU_EINVAL, "crgpu_sseq_params_dev: %llu cells, 2 to 2^31 - 1", (unsigned long long)N);
    CR_REQUIRE(ctx, nnz >= 1, CRGPU_EINVAL, "crgpu_sseq_params_dev: the matrix is empty, every size factor would be 0 / 0");

    // counts_per_cell, their median through the sort, the size factors
    DevBuf cnt_b, key_b, keyt_b;
    CR_TRY(dmalloc(ctx, cnt_b, N * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, key_b, N * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, keyt_b, N * sizeof(uint32_t)));
    CR_TRY(crgpu_matrix_dev_column_sums(ctx, m, nullptr, 0, cnt_b.as<uint32_t>()));
    CR_HIP(ctx, hipMemcpyAsync(key_b.p, cnt_b.p, N * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    bool in_tmp = false;
    CR_TRY(cr_radix_sort_u32(ctx, key_b.as<uint32_t>(), keyt_b.as<uint32_t>(), nullptr, nullptr, N, 0, 32, &in_tmp));
    std::vector<uint32_t> cnt(N), sorted(N);
    CR_TRY(crgpu_memcpy_d2h(ctx, cnt.data(), cnt_b.p, N * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, sorted.data(), in_tmp ? keyt_b.p : key_b.p, N * sizeof(uint32_t)));
    CR_REQUIRE(ctx, sorted[0] > 0, CRGPU_EINVAL, "crgpu_sseq_params_dev: a cell without counts (its size factor would be 0)");
    const double median = cr_median_sorted(sorted);
    std::unique_ptr<crgpu_sseq_params> P(new crgpu_sseq_params);
    P->n_cells = N, P->n_features = G;
    const double S = sq_size_factors(cnt.data(), N, median, P->sf);

    // the transpose by one sort, then a wave per gene
    DevBuf sf_b, k_b, kt_b, v_b, vt_b, s1_b, s2_b;
    CR_TRY(dmalloc(ctx, sf_b, N * sizeof(double)));
    CR_TRY(dmalloc(ctx, k_b, nnz * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, kt_b, nnz * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, v_b, nnz * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, vt_b, nnz * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, s1_b, G * sizeof(double)));
    CR_TRY(dmalloc(ctx, s2_b, G * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, sf_b.p, P->sf.data(), N * sizeof(double)));
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, nnz);
        hipLaunchKernelGGL(k_sq_keys, dim3(cr_grid(N * 64, SQ_WG)), dim3(SQ_WG), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data, N, G,
                           k_b.as<uint64_t>(), v_b.as<uint32_t>(), d_flag);
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !flag, CRGPU_EINVAL, "crgpu_sseq_params_dev: the matrix holds a row >= n_features (%u)", G);
    const uint32_t key_bits = std::max(1u, cr_ceil_log2((uint64_t)G * N));
    CR_TRY(cr_radix_sort_u64(ctx, k_b.as<uint64_t>(), kt_b.as<uint64_t>(), v_b.as<uint32_t>(), vt_b.as<uint32_t>(), nnz, 0, key_bits, &in_tmp));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, nnz);
        hipLaunchKernelGGL(k_sq_row_sums, dim3((G + 3u) / 4u), dim3(SQ_WG), 0, ctx->stream, in_tmp ? kt_b.as<uint64_t>() : k_b.as<uint64_t>(),
                           in_tmp ? vt_b.as<uint32_t>() : v_b.as<uint32_t>(), nnz, N, G, sf_b.as<double>(), s1_b.as<double>(), s2_b.as<double>());
        CR_HIP(ctx, hipGetLastError());
    }
    std::vector<double> s1(G), s2(G);
    CR_TRY(crgpu_memcpy_d2h(ctx, s1.data(), s1_b.p, G * sizeof(double)));
    CR_TRY(crgpu_memcpy_d2h(ctx, s2.data(), s2_b.p, G * sizeof(double)));

    CR_TRY(sq_gene_params(ctx, "crgpu_sseq_params_dev", *P, s1, s2, S));

    CR_TRY(cr_pool_alloc(ctx, (void **)&P->d_sf, N * sizeof(double)));
    crgpu_sseq_params *raw = P.release();
    int rc = cr_pool_alloc(ctx, (void **)&raw->d_mean, G * sizeof(double));
    if (rc == CRGPU_OK) rc = cr_pool_alloc(ctx, (void **)&raw->d_phi, G * sizeof(double));
    if (rc == CRGPU_OK) rc = crgpu_memcpy_h2d(ctx, raw->d_sf, raw->sf.data(), N * sizeof(double));
    if (rc == CRGPU_OK) rc = crgpu_memcpy_h2d(ctx, raw->d_mean, raw->mean.data(), G * sizeof(double));
    if (rc == CRGPU_OK) rc = crgpu_memcpy_h2d(ctx, raw->d_phi, raw->phi.data(), G * sizeof(double));
    if (rc != CRGPU_OK) {
        crgpu_sseq_params_free(ctx, raw);
        return rc;
    }
    *out = raw;
    return CRGPU_OK;
}

extern "C" int crgpu_sseq_params_get(crgpu_ctx *ctx, const crgpu_sseq_params *p, crgpu_sseq_params_info *info) {
    if (!ctx || !p || !info) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const uint64_t N = p->n_cells;
    const uint32_t G = p->n_features;
    // the vectors the tests read come from the device copies
    if (info->size_factors_out) CR_TRY(crgpu_memcpy_d2h(ctx, info->size_factors_out, p->d_sf, N * sizeof(double)));
    if (info->mean_out) CR_TRY(crgpu_memcpy_d2h(ctx, info->mean_out, p->d_mean, G * sizeof(double)));
    if (info->phi_out) CR_TRY(crgpu_memcpy_d2h(ctx, info->phi_out, p->d_phi, G * sizeof(double)));
    if (info->var_out) std::copy(p->var.begin(), p->var.end(), info->var_out);
    if (info->phi_mm_out) std::copy(p->phi_mm.begin(), p->phi_mm.end(), info->phi_mm_out);
    if (info->use_out) std::copy(p->use.begin(), p->use.end(), info->use_out);
    info->zeta_hat = p->zeta_hat, info->delta = p->delta;
    info->n_cells = N, info->n_features = G, info->n_used = p->n_used;
    return CRGPU_OK;
}

// the results of sq_run_tests that stay on the device: [K][G] each
struct SqTested {
    DevBuf p_b, adj_b, side_b;
    std::vector<uint64_t> n_exact, n_big;
};
// The exact and asymptotic tests of K clusters and Benjamini-Hochberg over the used genes of each: xin [K][G] = x_a, total [G] = x_a + x_b,
// s_a / s_b [K].  Fills res->ms_exact, ms_asymptotic, ms_bh, n_terms and the kernel classes.  crgpu_sseq_diffexp_dev and
// crgpu_sseq_pair_dev (sseq_pair.h, K = 1) share it.
static int sq_run_tests(crgpu_ctx *ctx, const char *who, const crgpu_sseq_params &P, uint32_t K, const std::vector<uint64_t> &xin,
                        const std::vector<uint64_t> &total, const std::vector<double> &s_a, const std::vector<double> &s_b, const crgpu_sseq_args *a,
                        crgpu_sseq_result *res, SqTested &T) {
    const uint32_t G = P.n_features;
    const uint32_t short_max = a->wave_min == 0u ? SQ_SHORT : std::min(a->wave_min - 1u, SQ_SHORT);  // terms of the short class at the most
    const uint64_t wg_min = a->wg_min ? a->wg_min : SQ_WG_MIN_DEFAULT;
    const size_t KG = (size_t)K * G;

    // the work lists
    std::vector<SqTest> t_short, t_wave, t_wg;
    std::vector<SqBig> t_big;
    std::vector<uint32_t> used;
    std::vector<uint64_t> &n_exact = T.n_exact, &n_big = T.n_big;
    n_exact.assign(K, 0), n_big.assign(K, 0);
    uint64_t n_terms = 0;
    for (uint32_t g = 0; g < G; g++)
        if (P.use[g]) used.push_back(g);
    for (uint32_t c = 0; c < K; c++)
        for (uint32_t g : used) {
            const uint64_t xa = xin[(size_t)c * G + g], xb = total[g] - xa;
            const double mu = P.mean[g], phi = P.phi[g];
            const uint32_t out = (uint32_t)((size_t)c * G + g);
            if (xa > SQ_BIG_COUNT && xb > SQ_BIG_COUNT) {
                SqBig b;
                b.alpha = s_a[c] * mu / (1.0 + phi * mu), b.beta = (s_b[c] / s_a[c]) * b.alpha;
                b.xa = xa, b.xb = xb, b.out = out, b.reserved = 0;
                t_big.push_back(b), n_big[c]++;
                continue;
            }
            CR_REQUIRE(ctx, total[g] < 0xFFFFFFFFull, CRGPU_ERANGE, "%s: an exact test of %llu terms (gene %u)", who, (unsigned long long)total[g] + 1ull, g);
            SqTest t;
            t.poisson = phi == 0.0 ? 1u : 0u;
            t.ra = t.poisson ? std::log(s_a[c]) : s_a[c] / phi, t.rb = t.poisson ? std::log(s_b[c]) : s_b[c] / phi;
            t.xa = (uint32_t)xa, t.T = (uint32_t)total[g], t.out = out;
            const uint64_t terms = total[g] + 1ull;
            (terms <= short_max ? t_short : terms >= wg_min ? t_wg : t_wave).push_back(t);
            n_exact[c]++, n_terms += terms;
        }
    CR_REQUIRE(ctx, KG < 0xFFFFFFFFull, CRGPU_ERANGE, "%s: %u clusters x %u genes", who, K, G);

    DevBuf &p_b = T.p_b, &adj_b = T.adj_b, &side_b = T.side_b;
    DevBuf ts_b, tw_b, tg_b, tb_b;
    std::vector<double> ones(KG, 1.0);
    CR_TRY(dmalloc(ctx, p_b, KG * sizeof(double)));
    CR_TRY(dmalloc(ctx, adj_b, KG * sizeof(double)));
    CR_TRY(dmalloc(ctx, side_b, KG));
    CR_TRY(crgpu_memcpy_h2d(ctx, p_b.p, ones.data(), KG * sizeof(double)));   // a gene that is not used: p = adjusted p = 1
    CR_TRY(crgpu_memcpy_h2d(ctx, adj_b.p, ones.data(), KG * sizeof(double)));
    CR_HIP(ctx, hipMemsetAsync(side_b.p, (int)SQ_NOT_ASYMPTOTIC, KG, ctx->stream));
    auto upload = [&](DevBuf &b, const void *src, size_t bytes) -> int {
        CR_TRY(dmalloc(ctx, b, bytes ? bytes : 8));
        if (bytes) CR_TRY(crgpu_memcpy_h2d(ctx, b.p, src, bytes));
        return CRGPU_OK;
    };
    CR_TRY(upload(ts_b, t_short.data(), t_short.size() * sizeof(SqTest)));
    CR_TRY(upload(tw_b, t_wave.data(), t_wave.size() * sizeof(SqTest)));
    CR_TRY(upload(tg_b, t_wg.data(), t_wg.size() * sizeof(SqTest)));
    CR_TRY(upload(tb_b, t_big.data(), t_big.size() * sizeof(SqBig)));
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));

    auto t0 = std::chrono::steady_clock::now();
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, n_terms);
        const uint32_t ns = (uint32_t)t_short.size(), nw = (uint32_t)t_wave.size(), ng = (uint32_t)t_wg.size();
        if (ng) hipLaunchKernelGGL(k_sq_exact_wg, dim3(ng), dim3(SQ_WG), 0, ctx->stream, tg_b.as<SqTest>(), ng, p_b.as<double>());
        if (nw) hipLaunchKernelGGL(k_sq_exact_wave, dim3((nw + 3u) / 4u), dim3(SQ_WG), 0, ctx->stream, tw_b.as<SqTest>(), nw, p_b.as<double>());
        if (ns) hipLaunchKernelGGL(k_sq_exact_short, dim3((ns + 15u) / 16u), dim3(SQ_WG), 0, ctx->stream, ts_b.as<SqTest>(), ns, p_b.as<double>());
        CR_HIP(ctx, hipGetLastError());
    }
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    res->ms_exact = cr_ms_since(t0);

    t0 = std::chrono::steady_clock::now();
    if (!t_big.empty()) {
        CrTimer t(ctx, CRGPU_T_MATRIX, t_big.size());
        const uint32_t nb = (uint32_t)t_big.size();
        hipLaunchKernelGGL(k_sq_asymptotic, dim3((nb + 63u) / 64u), dim3(64), 0, ctx->stream, tb_b.as<SqBig>(), nb, p_b.as<double>(), side_b.as<uint8_t>());
        CR_HIP(ctx, hipGetLastError());
    }
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    res->ms_asymptotic = cr_ms_since(t0);

    // Benjamini-Hochberg over the used genes of every cluster
    t0 = std::chrono::steady_clock::now();
    const uint32_t n_used = (uint32_t)used.size();
    {
        DevBuf used_b, k_b, kt_b, v_b, vt_b, ks_b, vs_b;
        CR_TRY(upload(used_b, used.data(), (size_t)n_used * sizeof(uint32_t)));
        CR_TRY(dmalloc(ctx, k_b, (size_t)K * n_used * sizeof(uint64_t)));
        CR_TRY(dmalloc(ctx, kt_b, (size_t)n_used * sizeof(uint64_t)));
        CR_TRY(dmalloc(ctx, v_b, (size_t)K * n_used * sizeof(uint32_t)));
        CR_TRY(dmalloc(ctx, vt_b, (size_t)n_used * sizeof(uint32_t)));
        CrTimer t(ctx, CRGPU_T_MATRIX, (uint64_t)K * n_used);
        hipLaunchKernelGGL(k_sq_bh_keys, dim3((n_used + SQ_WG - 1u) / SQ_WG, K), dim3(SQ_WG), 0, ctx->stream, p_b.as<double>(), G, used_b.as<uint32_t>(), n_used,
                           k_b.as<uint64_t>(), v_b.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
        for (uint32_t c = 0; c < K; c++) {  // the sorted keys of every cluster end in its own part of k_b / v_b
            uint64_t *kc = k_b.as<uint64_t>() + (size_t)c * n_used;
            uint32_t *vc = v_b.as<uint32_t>() + (size_t)c * n_used;
            bool in_tmp = false;
            CR_TRY(cr_radix_sort_u64(ctx, kc, kt_b.as<uint64_t>(), vc, vt_b.as<uint32_t>(), n_used, 0, 63, &in_tmp));
            if (in_tmp) {
                CR_HIP(ctx, hipMemcpyAsync(kc, kt_b.p, (size_t)n_used * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
                CR_HIP(ctx, hipMemcpyAsync(vc, vt_b.p, (size_t)n_used * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
            }
        }
        hipLaunchKernelGGL(k_sq_bh_close, dim3(K), dim3(SQ_WG), 0, ctx->stream, k_b.as<uint64_t>(), v_b.as<uint32_t>(), n_used, G, adj_b.as<double>());
        CR_HIP(ctx, hipGetLastError());
        CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    res->ms_bh = cr_ms_since(t0);
    res->n_terms = n_terms;
    res->n_short = t_short.size(), res->n_wave = t_wave.size(), res->n_workgroup = t_wg.size();
    return CRGPU_OK;
}

// what the caller set a pointer for, [K][G] and [K]
static int sq_write_results(crgpu_ctx *ctx, uint32_t G, uint32_t K, const std::vector<uint64_t> &xin, const std::vector<uint64_t> &total,
                            const std::vector<double> &s_a, const std::vector<double> &s_b, SqTested &T, crgpu_sseq_result *res) {
    const size_t KG = (size_t)K * G;
    const std::vector<uint64_t> &n_exact = T.n_exact, &n_big = T.n_big;
    DevBuf &p_b = T.p_b, &adj_b = T.adj_b, &side_b = T.side_b;
    if (res->p_values_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->p_values_out, p_b.p, KG * sizeof(double)));
    if (res->adjusted_p_values_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->adjusted_p_values_out, adj_b.p, KG * sizeof(double)));
    if (res->below_median_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->below_median_out, side_b.p, KG));
    for (uint32_t c = 0; c < K; c++) {
        for (uint32_t g = 0; g < G; g++) {
            const size_t e = (size_t)c * G + g;
            const uint64_t xa = xin[e], xb = total[g] - xa;
            if (res->sums_in_out) res->sums_in_out[e] = xa;
            if (res->sums_out_out) res->sums_out_out[e] = xb;
            if (res->norm_mean_in_out) res->norm_mean_in_out[e] = (double)xa / s_a[c];
            if (res->norm_mean_out_out) res->norm_mean_out_out[e] = (double)xb / s_b[c];
            if (res->log2_fold_change_out)
                res->log2_fold_change_out[e] = std::log2((1.0 + (double)xa) / (1.0 + s_a[c])) - std::log2((1.0 + (double)xb) / (1.0 + s_b[c]));
        }
        if (res->s_a_out) res->s_a_out[c] = s_a[c];
        if (res->s_b_out) res->s_b_out[c] = s_b[c];
        if (res->n_exact_out) res->n_exact_out[c] = n_exact[c];
        if (res->n_asymptotic_out) res->n_asymptotic_out[c] = n_big[c];
    }
    return CRGPU_OK;
}

extern "C" int crgpu_sseq_diffexp_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const crgpu_sseq_params *P, const int32_t *labels, uint32_t K,
                                      const crgpu_sseq_args *a, crgpu_sseq_result *res) {
    if (!ctx || !m || !P || !labels || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const uint64_t N = m->n_barcodes;
    const uint32_t G = P->n_features;
    CR_REQUIRE(ctx, G >= 3 && N >= 2, CRGPU_EINVAL, "crgpu_sseq_diffexp_dev: %u features and %llu cells, at least 3 and 2", G, (unsigned long long)N);
    CR_REQUIRE(ctx, K >= 2 && K <= CRGPU_SSEQ_MAX_K, CRGPU_EINVAL, "crgpu_sseq_diffexp_dev: %u clusters, 2 to %u", K, CRGPU_SSEQ_MAX_K);
    CR_REQUIRE(ctx, P->n_cells == N && (a->n_features == 0 || a->n_features == G), CRGPU_EINVAL,
               "crgpu_sseq_diffexp_dev: the parameters are those of a %u x %llu matrix, this one is %u x %llu", G, (unsigned long long)P->n_cells,
               a->n_features ? a->n_features : G, (unsigned long long)N);
    std::vector<uint64_t> size(K, 0);
    for (uint64_t c = 0; c < N; c++) {
        CR_REQUIRE(ctx, labels[c] >= 1 && (uint32_t)labels[c] <= K, CRGPU_EINVAL, "crgpu_sseq_diffexp_dev: label %d of cell %llu, 1 to %u", labels[c],
                   (unsigned long long)c, K);
        size[labels[c] - 1]++;
    }
    for (uint32_t c = 0; c < K; c++) CR_REQUIRE(ctx, size[c] > 0, CRGPU_EINVAL, "crgpu_sseq_diffexp_dev: cluster %u is empty", c + 1u);
    const size_t KG = (size_t)K * G;

    // the group sums
    auto t0 = std::chrono::steady_clock::now();
    DevBuf lab_b, sums_b;
    CR_TRY(dmalloc(ctx, lab_b, N * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, sums_b, KG * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, lab_b.p, labels, N * sizeof(int32_t)));
    CR_HIP(ctx, hipMemsetAsync(sums_b.p, 0, KG * sizeof(uint64_t), ctx->stream));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
        hipLaunchKernelGGL(k_sq_group_sums, dim3(cr_grid(N * 64, SQ_WG)), dim3(SQ_WG), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data, N,
                           G, lab_b.as<int32_t>(), sums_b.as<unsigned long long>());
        CR_HIP(ctx, hipGetLastError());
    }
    std::vector<uint64_t> xin(KG);
    CR_TRY(crgpu_memcpy_d2h(ctx, xin.data(), sums_b.p, KG * sizeof(uint64_t)));
    res->ms_sums = cr_ms_since(t0);

    // per cluster the sums of the size factors, in cell order; per gene the total
    std::vector<double> s_a(K, 0.0), s_b(K, 0.0);
    for (uint32_t c = 0; c < K; c++)
        for (uint64_t i = 0; i < N; i++) {
            if ((uint32_t)labels[i] == c + 1u) s_a[c] += P->sf[i]; else s_b[c] += P->sf[i];
        }
    std::vector<uint64_t> total(G, 0);
    for (uint32_t c = 0; c < K; c++)
        for (uint32_t g = 0; g < G; g++) total[g] += xin[(size_t)c * G + g];

    SqTested T;
    CR_TRY(sq_run_tests(ctx, "crgpu_sseq_diffexp_dev", *P, K, xin, total, s_a, s_b, a, res, T));
    CR_TRY(sq_write_results(ctx, G, K, xin, total, s_a, s_b, T, res));
    return CRGPU_OK;
}
