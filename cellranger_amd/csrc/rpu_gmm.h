// rpu_gmm.h -- the enrichment call of a targeted well: fit_enrichments(..., method = BOTH_TIED) on the device (part of
// molecule_stages.hip; it shares nothing with the other stages but the pooled temporaries).
//
// Replaces lib/python/cellranger/targeted/gmm.py: fit_enrichments (:116-183) with its guards (:145-169) and fit_2comp_gmm (:26-112)
// for covariance_type = TIED, i.e. 1 + 5151 independent runs of scikit-learn's GaussianMixture EM on 1-D data:
//   start 0        the label medians; then every pair (a, b), a >= b, of np.linspace(0, max(values), 101) in the reference's order
//   initial values weights = the label counts / n, ONE tied precision 1 / max(iqr(off-target values) / 1.35, 1e-2)^2
//   an iteration   e-step (weighted log probabilities, logsumexp, responsibilities), m-step (nk + 10 eps, means, the tied covariance
//                  + reg_covar 1e-6, weights), lower bound = mean logsumexp under the PREVIOUS parameters; stop at |change| < 1e-3
//                  or after 100 iterations
//   the winner     lk > max_lk in start order, lk = sum of score_samples under the final parameters
//   afterwards     the posterior, threshold = min value whose high-mean posterior is > 0.5 (NaN unless both components get members),
//                  ClassStats from values >= threshold.
// QUIRK kept: sd_high and sd_low are what the reference reports for the tied model, the PRECISION, twice (gmm.py:86-90).
//
// k_gmm_fit: one workgroup of 256 threads per start; the 100-iteration loop never leaves the kernel.  The values sit in LDS where
// n <= ctx->gmm_lds_values (CRGPU_GMM_LDS_VALUES, default 8192 = 64 KB, which leaves room for two workgroups per CU; at 128 KB the
// fit was 17 % slower than from L2), else they are read from device memory (36 601 doubles are 286 KB: more than one LDS, resident
// in L2).  Every sum of an iteration is reduced in ONE order that depends on n alone: thread t
// adds the values t, t + 256, ... in ascending order, a wave adds its lanes by the xor butterfly, lane 0 of wave 0 adds the four
// waves in ascending order.  A start reads nothing another start writes: its result does not depend on the grid, on the other
// starts or on the run.  f64 throughout, unfused (-ffp-contract=off).
// Not covered: BOTH_SPHERICAL and OFFTARGETS_ONLY (the stage uses neither).
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>

#include "stage_common.h"

#define GMM_WG 256u
#define GMM_MIN_OFFTARGET_GENES 30u
#define GMM_NSUM 5u
#define GMM_OUT 6u  // per start: w0, w1, mu0, mu1, precision, lk

// sums of GMM_NSUM doubles over the workgroup, the same value in every thread; s_red: GMM_NSUM * 4 doubles
__device__ __forceinline__ void gmm_block_sum(double *v, double *s_red, double *s_tot) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < GMM_NSUM; k++) {
        v[k] = wave_sum(v[k]);
        if (lane == 0u) s_red[k * 4u + wave] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < GMM_NSUM) {
        const double *r = s_red + threadIdx.x * 4u;
        s_tot[threadIdx.x] = ((r[0] + r[1]) + r[2]) + r[3];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < GMM_NSUM; k++) v[k] = s_tot[k];
    __syncthreads();
}

// gmm_logsumexp and the constants of the EM iteration: stage_common.h (the marginal caller runs the same iteration)

template <bool LDS>
__global__ __launch_bounds__(GMM_WG) void k_gmm_fit(const double *__restrict__ values, uint32_t n, const double *__restrict__ start_means, uint32_t n_starts,
                                                    double w0_init, double w1_init, double prec_init, double xx, double *__restrict__ out,
                                                    uint32_t *__restrict__ iters_out) {
    extern __shared__ double gmm_x[];  // LDS: the values (n doubles)
    __shared__ double s_red[GMM_NSUM * 4u], s_tot[GMM_NSUM];
    const uint32_t tid = threadIdx.x, s = blockIdx.x;
    if (s >= n_starts) return;  // uniform
    if (LDS) {
        for (uint32_t i = tid; i < n; i += GMM_WG) gmm_x[i] = values[i];
        __syncthreads();
    }
    const double *x = LDS ? gmm_x : values;
    double w0 = w0_init, w1 = w1_init, mu0 = start_means[2u * s], mu1 = start_means[2u * s + 1u], pc = sqrt(prec_init);
    double lb = -INFINITY;
    uint32_t it = 0;
    for (it = 1; it <= GMM_MAX_ITER; it++) {  // uniform: every thread holds the same parameters
        const double prev = lb;
        // -0.5 (log 2 pi + y^2) + log pc + log w: the restatement's order of the three terms
        const double lp = log(pc), l0 = log(w0), l1 = log(w1);
        double v[GMM_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint32_t i = tid; i < n; i += GMM_WG) {
            const double xi = x[i];
            const double y0 = xi * pc - mu0 * pc, y1 = xi * pc - mu1 * pc;
            const double a0 = -0.5 * (GMM_LOG_2PI + y0 * y0) + lp + l0, a1 = -0.5 * (GMM_LOG_2PI + y1 * y1) + lp + l1;
            const double lpn = gmm_logsumexp(a0, a1);
            const double r0 = exp(a0 - lpn), r1 = exp(a1 - lpn);
            v[0] += r0, v[1] += r1, v[2] += r0 * xi, v[3] += r1 * xi, v[4] += lpn;
        }
        gmm_block_sum(v, s_red, s_tot);
        const double nk0 = v[0] + 10.0 * 2.220446049250313e-16, nk1 = v[1] + 10.0 * 2.220446049250313e-16;
        mu0 = v[2] / nk0, mu1 = v[3] / nk1;
        const double nks = nk0 + nk1;
        const double cov = (xx - ((nk0 * mu0) * mu0 + (nk1 * mu1) * mu1)) / nks + GMM_REG;
        w0 = nk0 / nks, w1 = nk1 / nks;
        const double ws = w0 + w1;
        w0 = w0 / ws, w1 = w1 / ws;
        pc = 1.0 / sqrt(cov);
        lb = v[4] / (double)n;
        if (fabs(lb - prev) < GMM_TOL) break;
    }
    if (it > GMM_MAX_ITER) it = GMM_MAX_ITER;
    // lk = sum of score_samples under the final parameters
    const double lp = log(pc), l0 = log(w0), l1 = log(w1);
    double v[GMM_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t i = tid; i < n; i += GMM_WG) {
        const double xi = x[i];
        const double y0 = xi * pc - mu0 * pc, y1 = xi * pc - mu1 * pc;
        v[4] += gmm_logsumexp(-0.5 * (GMM_LOG_2PI + y0 * y0) + lp + l0, -0.5 * (GMM_LOG_2PI + y1 * y1) + lp + l1);
    }
    gmm_block_sum(v, s_red, s_tot);
    if (tid == 0u) {
        double *o = out + (size_t)s * GMM_OUT;
        o[0] = w0, o[1] = w1, o[2] = mu0, o[3] = mu1, o[4] = pc * pc, o[5] = v[4];
        iters_out[s] = it;
    }
}

// predict_proba under the winner's parameters: bit 0 = posterior of component `hi` > 0.5, bit 1 = posterior of component `lo` >= 0.5
__global__ __launch_bounds__(256) void k_gmm_posterior(const double *__restrict__ values, uint32_t n, double w0, double w1, double mu0, double mu1, double prec,
                                                       uint32_t hi, uint32_t lo, uint8_t *__restrict__ member) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double pc = sqrt(prec), lp = log(pc), l0 = log(w0), l1 = log(w1), xi = values[i];
    const double y0 = xi * pc - mu0 * pc, y1 = xi * pc - mu1 * pc;
    const double a0 = -0.5 * (GMM_LOG_2PI + y0 * y0) + lp + l0, a1 = -0.5 * (GMM_LOG_2PI + y1 * y1) + lp + l1;
    const double lpn = gmm_logsumexp(a0, a1);
    const double p[2] = {exp(a0 - lpn), exp(a1 - lpn)};
    member[i] = (uint8_t)((p[hi] > 0.5 ? 1u : 0u) | (p[lo] >= 0.5 ? 2u : 0u));
}

static void gmm_class_stats(const double *values, const uint8_t *labels, uint32_t n, double thr, crgpu_rpu_gmm_result *res, uint8_t *enriched_out) {
    uint64_t te = 0, tn = 0, oe = 0, on = 0;
    for (uint32_t i = 0; i < n; i++) {
        const bool e = values[i] >= thr;  // false for a NaN threshold
        if (enriched_out) enriched_out[i] = e;
        if (labels[i]) (e ? te : tn)++; else (e ? oe : on)++;
    }
    res->n_targeted_enriched = (double)te, res->n_targeted_not_enriched = (double)tn;
    res->n_offtgt_enriched = (double)oe, res->n_offtgt_not_enriched = (double)on;
}

extern "C" int crgpu_rpu_gmm_dev(crgpu_ctx *ctx, const double *values, const uint8_t *labels, uint32_t n, const crgpu_rpu_gmm_args *args,
                                 crgpu_rpu_gmm_result *res) {
    if (!ctx || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, (values && labels) || n == 0, CRGPU_EINVAL, "crgpu_rpu_gmm_dev: NULL values or labels");
    const double nan = std::nan("");
    memset(res, 0, sizeof(*res));
    res->log_rpu_threshold = res->mu_high = res->mu_low = res->sd_high = res->sd_low = res->alpha_high = res->alpha_low = nan;
    res->n_targeted_enriched = res->n_targeted_not_enriched = res->n_offtgt_enriched = res->n_offtgt_not_enriched = nan;
    res->max_lk = nan;
    res->winner = NONE32;
    double *lk_out = args ? args->start_lk_out : nullptr;
    uint32_t *it_out = args ? args->start_iters_out : nullptr;
    uint8_t *enriched_out = args ? args->enriched_out : nullptr;
    for (uint32_t s = 0; s < CRGPU_GMM_STARTS; s++) {
        if (lk_out) lk_out[s] = nan;
        if (it_out) it_out[s] = 0;
    }
    if (enriched_out && n) memset(enriched_out, 0, n);
    uint32_t nt = 0;
    for (uint32_t i = 0; i < n; i++) {
        CR_REQUIRE(ctx, std::isfinite(values[i]), CRGPU_EINVAL, "crgpu_rpu_gmm_dev: values[%u] is not finite", i);
        nt += labels[i] != 0;
    }
    const uint32_t no = n - nt;
    // ---- the guards of fit_enrichments (gmm.py:145-169): no launch ----
    if (nt == 0 && no == 0) return CRGPU_OK;  // nothing to do
    if (no == 0) {                            // no off-target genes: completely enriched
        res->log_rpu_threshold = 0.0;
        gmm_class_stats(values, labels, n, 0.0, res, enriched_out);
        return CRGPU_OK;
    }
    if (std::max(no, nt) < GMM_MIN_OFFTARGET_GENES || std::min(nt, no) == 0) return CRGPU_OK;
    // ---- initial values (fit_2comp_gmm :36-65) ----
    std::vector<double> on_v, off_v;
    double vmax = values[0], xx = 0.0;
    for (uint32_t i = 0; i < n; i++) {
        (labels[i] ? on_v : off_v).push_back(values[i]);
        vmax = std::max(vmax, values[i]);
    }
    std::sort(on_v.begin(), on_v.end());
    std::sort(off_v.begin(), off_v.end());
    const double w0 = (double)nt / (double)(nt + no), w1 = (double)no / (double)(nt + no);
    const double sd_off = std::max((cr_quantile_sorted(off_v, 0.75) - cr_quantile_sorted(off_v, 0.25)) / 1.35, 1e-2);
    const double prec0 = 1.0 / (sd_off * sd_off);
    std::vector<double> grid(101), starts;
    const double step = (vmax - 0.0) / 100.0;  // np.linspace: arange(101) * step + start, the last point set to stop
    for (uint32_t i = 0; i < 101; i++) grid[i] = step == 0.0 ? (double)i / 100.0 * vmax : (double)i * step;
    grid[100] = vmax;
    starts.push_back(cr_median_sorted(on_v));
    starts.push_back(cr_median_sorted(off_v));
    for (uint32_t a = 0; a < 101; a++)
        for (uint32_t b = 0; b < 101; b++) {
            if (grid[a] < grid[b]) continue;
            starts.push_back(grid[a]);
            starts.push_back(grid[b]);
        }
    const uint32_t n_starts = (uint32_t)(starts.size() / 2);
    // x @ x: the tied covariance's constant; added in the order of gmm_block_sum so that it, too, depends on n alone
    {
        double part[GMM_WG];
        for (uint32_t t = 0; t < GMM_WG; t++) {
            part[t] = 0.0;
            for (uint32_t i = t; i < n; i += GMM_WG) part[t] += values[i] * values[i];
        }
        double wsum[4];
        for (uint32_t w = 0; w < 4; w++) {
            double lane[64];
            for (uint32_t l = 0; l < 64; l++) lane[l] = part[w * 64 + l];
            for (uint32_t d = 32; d >= 1; d >>= 1)
                for (uint32_t l = 0; l < d; l++) lane[l] += lane[l + d];
            wsum[w] = lane[0];
        }
        xx = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    }
    // ---- the fit ----
    DevBuf val_b, st_b, out_b, it_b, mem_b;
    CR_TRY(dmalloc(ctx, val_b, (uint64_t)n * sizeof(double)));
    CR_TRY(dmalloc(ctx, st_b, starts.size() * sizeof(double)));
    CR_TRY(dmalloc(ctx, out_b, (uint64_t)n_starts * GMM_OUT * sizeof(double)));
    CR_TRY(dmalloc(ctx, it_b, (uint64_t)n_starts * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, mem_b, n));
    CR_TRY(crgpu_memcpy_h2d(ctx, val_b.p, values, (uint64_t)n * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, st_b.p, starts.data(), starts.size() * sizeof(double)));
    const bool lds = n <= ctx->gmm_lds_values && (uint64_t)n * sizeof(double) <= 128u * 1024u;
    const auto t0 = std::chrono::steady_clock::now();
    {
        CrTimer t(ctx, CRGPU_T_DEDUP, (uint64_t)n_starts * n);
        if (lds) {
            const size_t dyn = (size_t)n * sizeof(double);
            cr_allow_lds(ctx, (const void *)k_gmm_fit<true>, dyn);
            hipLaunchKernelGGL(k_gmm_fit<true>, dim3(n_starts), dim3(GMM_WG), dyn, ctx->stream, val_b.as<double>(), n, st_b.as<double>(), n_starts, w0, w1, prec0,
                               xx, out_b.as<double>(), it_b.as<uint32_t>());
        } else {
            hipLaunchKernelGGL(k_gmm_fit<false>, dim3(n_starts), dim3(GMM_WG), 0, ctx->stream, val_b.as<double>(), n, st_b.as<double>(), n_starts, w0, w1, prec0,
                               xx, out_b.as<double>(), it_b.as<uint32_t>());
        }
        CR_HIP(ctx, hipGetLastError());
    }
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    res->fit_ms = cr_ms_since(t0);
    std::vector<double> h_out((size_t)n_starts * GMM_OUT);
    std::vector<uint32_t> h_it(n_starts);
    CR_TRY(crgpu_memcpy_d2h(ctx, h_out.data(), out_b.p, h_out.size() * sizeof(double)));
    CR_TRY(crgpu_memcpy_d2h(ctx, h_it.data(), it_b.p, h_it.size() * sizeof(uint32_t)));
    // ---- the winner: lk > max_lk in start order ----
    double max_lk = -INFINITY;
    uint32_t win = NONE32;
    for (uint32_t s = 0; s < n_starts; s++) {
        const double lk = h_out[(size_t)s * GMM_OUT + 5];
        if (s < CRGPU_GMM_STARTS) {
            if (lk_out) lk_out[s] = lk;
            if (it_out) it_out[s] = h_it[s];
        }
        if (lk > max_lk) max_lk = lk, win = s;
    }
    res->n_starts = n_starts, res->fitted = 1u, res->in_lds = lds ? 1u : 0u;
    CR_REQUIRE(ctx, win != NONE32, CRGPU_ERANGE, "crgpu_rpu_gmm_dev: no start has a likelihood (a NaN in every fit)");
    const double *o = h_out.data() + (size_t)win * GMM_OUT;
    // np.argmax / np.argmin of the two means: the first of equal values
    const uint32_t hi = o[3] > o[2] ? 1u : 0u, lo = o[3] < o[2] ? 1u : 0u;
    res->winner = win, res->max_lk = max_lk;
    res->mu_high = o[2 + hi], res->mu_low = o[2 + lo];
    res->sd_high = res->sd_low = o[4];  // the quirk: the precision, twice
    res->alpha_high = o[hi], res->alpha_low = o[lo];
    // ---- the posterior and the threshold ----
    {
        CrTimer t(ctx, CRGPU_T_DEDUP, n);
        hipLaunchKernelGGL(k_gmm_posterior, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, val_b.as<double>(), n, o[0], o[1], o[2], o[3], o[4], hi, lo,
                           mem_b.as<uint8_t>());
        CR_HIP(ctx, hipGetLastError());
    }
    std::vector<uint8_t> member(n);
    CR_TRY(crgpu_memcpy_d2h(ctx, member.data(), mem_b.p, n));
    uint64_t n_hi = 0, n_lo = 0;
    double thr = INFINITY;
    for (uint32_t i = 0; i < n; i++) {
        if (member[i] & 1u) n_hi++, thr = std::min(thr, values[i]);
        if (member[i] & 2u) n_lo++;
    }
    res->log_rpu_threshold = n_hi && n_lo ? thr : nan;
    gmm_class_stats(values, labels, n, res->log_rpu_threshold, res, enriched_out);
    return CRGPU_OK;
}
