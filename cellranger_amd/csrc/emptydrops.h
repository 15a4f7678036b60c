// emptydrops.h -- the non-ambient ("EmptyDrops") barcodes behind the initial cell call (part of matrix_stages.hip: the sort
// keys are those of cell_calling.h).
//
// Replaces find_nonambient_barcodes (lib/python/cellranger/cell_calling.py:144-263) with est_background_profile_sgt /
// estimate_profile_sgt (:47-102), sgt_proportions / simple_good_turing (sgt.py:24-132), eval_multinomial_loglikelihoods
// (stats.py:24-46), simulate_multinomial_loglikelihoods (stats.py:81-202), compute_ambient_pvalues (stats.py:205-231) and
// adjust_pvalue_bh (analysis/diffexp.py:88-97), as called from call_additional_cells (cell_calling_helpers.py:575-668) for ONE
// genome / GEM group.  `low` and `high` are arguments: get_empty_drops_range (cell_calling.py:122-141) gives
// (N_PARTITIONS / 2, N_PARTITIONS) with N_PARTITIONS = 9 000 for the LT chip, 160 000 (80 000 x probe barcodes when
// multiplexed) for the chips with doubled GEM count and 90 000 (45 000 x probe barcodes) otherwise.
//
//   1. ambient set      all V totals are sorted once, descending with the LARGER column first among equal totals (a stable
//                       ascending argsort, reversed: k_om_keys of the OrdMag call); places [low, high) with a non-zero total;
//   2. profile counts   u64 atomics per row over the ambient columns (exact), a flag per row that is non-zero anywhere;
//   3. SGT              host, f64 (crgpu_sgt_proportions); profile_p over eval_features, its cdf by a sequential running sum;
//   4. candidates       a compaction of total >= max(minimum, 1 + max_background) && not an initial cell: ascending columns;
//   5. observed loglk   one wave per candidate, lane-strided partial sums joined by a butterfly: one fixed order.  lgamma(c + 1)
//                       comes from a host-built table (c <= the largest candidate total), log p from a host-built array;
//   6. simulation       k_ed_simulate, below;
//   7. p-values, BH     n_lower (integers, from the device) -> (1 + n_lower) / (1 + S); p takes at most S + 1 values, so BH is
//                       a histogram of n_lower and a running minimum over its S + 1 levels: host, O(candidates + S);
//   8. merge            initial cells and non-ambient candidates are both ascending and disjoint: one merge on the host.
#pragma once

#include <algorithm>
#include <cmath>

#include "cell_calling.h"
#include "philox.h"
#include "stage_common.h"

#define ED_SIM_THREADS 1024
#define ED_LDS_BYTES (160u * 1024u - 64u)  // dynamic LDS a workgroup of k_ed_simulate may take (its static part is 24 bytes)
#define ED_FIXED_BITS 40                   // fraction bits of the fixed-point log terms (fewer when the sum would not fit 2^62)

// ---- Simple Good-Turing (sgt.py:24-132), host ---------------------------------------------------------------------------------
static int ed_sgt(const uint64_t *freq, uint64_t n, double *pstar, double *p0_out, double *slope_out) {
    std::vector<uint64_t> s(freq, freq + n);
    std::sort(s.begin(), s.end());
    std::vector<double> xr, xnr;  // use_freqs, freqfreqs[use_freqs]
    for (uint64_t i = 0; i < n;) {
        uint64_t j = i;
        while (j < n && s[j] == s[i]) j++;
        xr.push_back((double)s[i]);
        xnr.push_back((double)(j - i));
        i = j;
    }
    const size_t R = xr.size();
    if (R < 10) return CRGPU_SGT_TOO_FEW;
    double xN = 0.0;
    for (size_t i = 0; i < R; i++) xN += xr[i] * xnr[i];
    // _averaging_transform: d = [1, diff(r)], dr = [0.5 * (d[1:] + d[:-1]), d[-1]]
    std::vector<double> d(R), lx(R), ly(R);
    d[0] = 1.0;
    for (size_t i = 1; i < R; i++) d[i] = xr[i] - xr[i - 1];
    for (size_t i = 0; i < R; i++) {
        const double dr = i + 1 < R ? 0.5 * (d[i + 1] + d[i]) : d[R - 1];
        lx[i] = std::log(xr[i]);
        ly[i] = std::log(xnr[i] / dr);
    }
    // linregress: slope = mean((x - mx)(y - my)) / mean((x - mx)^2)
    double mx = 0.0, my = 0.0;
    for (size_t i = 0; i < R; i++) {
        mx += lx[i];
        my += ly[i];
    }
    mx /= (double)R;
    my /= (double)R;
    double sxy = 0.0, sxx = 0.0;
    for (size_t i = 0; i < R; i++) {
        sxy += (lx[i] - mx) * (ly[i] - my);
        sxx += (lx[i] - mx) * (lx[i] - mx);
    }
    const double slope = (sxy / (double)R) / (sxx / (double)R);
    if (slope_out) *slope_out = slope;
    if (slope > -1.0) return CRGPU_SGT_SLOPE;
    std::vector<double> rel(R), star(R, 0.0), tursd(R, 1.0), cmb(R, 0.0);
    for (size_t i = 0; i < R; i++) {
        rel[i] = xr[i] * std::pow(1.0 + 1.0 / xr[i], 1.0 + slope) / xr[i];
        const bool turing = i + 1 < R && xr[i] == xr[i + 1] - 1.0;
        if (turing) {
            star[i] = (xr[i] + 1.0) / xr[i] * xnr[i + 1] / xnr[i];
            tursd[i] = (double)(i + 2) / xnr[i] * std::sqrt(xnr[i + 1] * (1.0 + xnr[i + 1] / xnr[i]));
        }
    }
    bool useturing = true;
    for (size_t r = 0; r < R; r++) {
        if (useturing && std::fabs(rel[r] - star[r]) * (double)(1 + r) / tursd[r] > 1.65) {
            cmb[r] = star[r];
        } else {
            useturing = false;
            cmb[r] = rel[r];
        }
    }
    double sumpraw = 0.0;
    for (size_t i = 0; i < R; i++) sumpraw += cmb[i] * xr[i] * xnr[i] / xN;
    const double p0 = xnr[0] / xN;
    std::vector<double> rstar(R);
    double rstar_sum = 0.0;
    for (size_t i = 0; i < R; i++) {
        rstar[i] = xr[i] * (cmb[i] * (1.0 - xnr[0] / xN) / sumpraw);
        rstar_sum += xnr[i] * rstar[i];
    }
    if (p0_out) *p0_out = p0;
    if (pstar)
        for (uint64_t i = 0; i < n; i++) {
            const size_t k = (size_t)(std::lower_bound(xr.begin(), xr.end(), (double)freq[i]) - xr.begin());
            pstar[i] = (1.0 - p0) * (rstar[k] / rstar_sum);
        }
    return CRGPU_OK;
}

extern "C" int crgpu_sgt_proportions(const uint64_t *freq, uint64_t n, double *pstar, double *p0, double *slope) {
    if (!freq || !n) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_sgt_proportions: the frequency vector is empty");
    for (uint64_t i = 0; i < n; i++)
        if (!freq[i]) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_sgt_proportions: frequencies must be greater than zero");
    return ed_sgt(freq, n, pstar, p0, slope);
}

// ---- small kernels -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_ed_max_row(const int32_t *__restrict__ indices, uint64_t nnz, uint32_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t m = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += stride) m = max(m, (uint32_t)indices[i] + 1u);
    if (m) atomicMax(out, m);
}

// any[f] = 1 for the rows with a positive entry (inside the mask); flag: a row >= n_features
__global__ __launch_bounds__(256) void k_ed_rows_present(const int32_t *__restrict__ indices, const int32_t *__restrict__ data, uint64_t nnz,
                                                         const uint8_t *__restrict__ mask, uint32_t n_features, uint8_t *__restrict__ any,
                                                         uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += stride) {
        const uint32_t f = (uint32_t)indices[i];
        if (f >= n_features) {
            *flag = 1u;
            continue;
        }
        if (data[i] > 0 && (!mask || mask[f])) any[f] = 1;
    }
}

// places [p0, p1) of the descending order (key = ~total, val = column): row sums of the columns with a non-zero total, their number
__global__ __launch_bounds__(256) void k_ed_ambient_rows(const uint32_t *__restrict__ key, const uint32_t *__restrict__ val, uint64_t p0,
                                                         uint64_t p1, const long long *__restrict__ indptr,
                                                         const int32_t *__restrict__ indices, const int32_t *__restrict__ data,
                                                         const uint8_t *__restrict__ mask, uint32_t n_features,
                                                         unsigned long long *__restrict__ rowsum, uint32_t *__restrict__ n_used) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t p = p0 + wave0; p < p1; p += n_waves) {
        if (key[p] == 0xFFFFFFFFu) continue;  // total 0
        const uint32_t c = val[p];
        if (lane == 0) atomicAdd(n_used, 1u);
        for (long long i = indptr[c] + lane, e = indptr[c + 1]; i < e; i += 64) {
            const uint32_t f = (uint32_t)indices[i];
            if (f < n_features && data[i] > 0 && (!mask || mask[f])) atomicAdd(&rowsum[f], (unsigned long long)data[i]);
        }
    }
}

struct EdCandFlag {
    const uint32_t *counts;
    const uint8_t *is_cell;
    uint32_t thr;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return counts[i] >= thr && !is_cell[i]; }
};
struct EdCandEmit {
    const uint32_t *counts;
    uint64_t *col;
    uint32_t *umis;
    struct Pre {
        uint32_t c;
    };
    __device__ __forceinline__ Pre pre(uint64_t i) const { return Pre{counts[i]}; }
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t o, Pre p) const {
        col[o] = i;
        umis[o] = p.c;
    }
};

// eval_multinomial_loglikelihoods (stats.py:24-46): lgamma(N + 1) + sum_j (c_j * log p_j - lgamma(c_j + 1)) of one candidate column
// per wave.  logp[f] is indexed by the ROW (0 outside eval_features), lgam[c] = lgamma(c + 1) for c <= nmax.  flag: umis[k] is not the
// sum of the column under the mask (N and the c_j must come from the same counts), or a count above nmax.
__global__ __launch_bounds__(256) void k_ed_observed(const uint64_t *__restrict__ cols, const uint32_t *__restrict__ umis, uint64_t n,
                                                     const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                     const int32_t *__restrict__ data, const uint8_t *__restrict__ mask, uint32_t n_features,
                                                     const double *__restrict__ logp, const double *__restrict__ lgam, uint32_t nmax,
                                                     double *__restrict__ out, uint32_t *__restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t k = wave0; k < n; k += n_waves) {
        const uint64_t c = cols[k];
        double acc = 0.0;
        unsigned long long total = 0;
        for (long long i = indptr[c] + lane, e = indptr[c + 1]; i < e; i += 64) {
            const uint32_t f = (uint32_t)indices[i];
            const int32_t x = data[i];
            if (f >= n_features || x <= 0 || (mask && !mask[f])) continue;
            total += (uint32_t)x;
            if ((uint32_t)x > nmax) continue;  // total then differs from umis[k] <= nmax, or umis[k] > nmax: flagged below
            acc += (double)x * logp[f] - lgam[x];
        }
        acc = wave_sum(acc), total = wave_sum(total);
        if (lane == 0) {
            const uint32_t N = umis[k];
            if (N > nmax || total != N) *flag = 1u; else out[k] = lgam[N] + acc;
        }
    }
}

// ---- the simulation -------------------------------------------------------------------------------------------------------------
// Draw t of simulation s is word t & 3 (philox.h) of Philox4x64-10(counter = (1 + (t >> 2), s, 0, 0), key = (seed, 0)): element t of
// np.random.Philox(counter=[0, s, 0, 0], key=[seed, 0]).random_raw().  u = (word >> 11) * 2^-53, feature = searchsorted(cdf, u,
// side="right").  The counts after N draws are the first N draws (nested, as stats.py:143-197 extends one sample).
struct EdSimArgs {
    const double *cdf;        // n_feat, last == 1.0
    const uint32_t *guide;    // (1 << guide_bits) + 1: guide[b] = #{cdf <= b * 2^-guide_bits}
    uint32_t guide_bits, n_feat;
    const long long *lp;      // n_feat: round(log p_j * 2^fixed_bits)
    const long long *lc;      // dn[D - 1]: round(log(c + 1) * 2^fixed_bits)
    const uint32_t *dn;       // D distinct N, ascending, all > 0
    const double *lgn;        // D: lgamma(N + 1)
    uint32_t D, S;
    double scale;             // 2^-fixed_bits
    const uint32_t *cand_start;  // D + 1: the candidates with N == dn[i] are order[cand_start[i] .. cand_start[i + 1])
    const uint32_t *order;
    const double *obs;        // observed log-likelihoods (candidate order)
    uint32_t *n_lower;        // ... simulated values strictly below them (zeroed by the caller)
    double *table;            // D x S or NULL
    unsigned long long seed;
    uint32_t *gcounters;      // !LDS: gridDim.x * n_feat
};

// One workgroup runs whole simulations (s = blockIdx.x, += gridDim.x).  The feature counters live in LDS (LDS) or in the
// workgroup's slice of gcounters.  A segment = the draws between two distinct N: its draws are taken by the threads in any order,
// each returning atomic gives the count c before the draw, the draw adds log p_j - log(c + 1).  The SET of terms of a segment
// does not depend on the order of its atomics, and the terms are integers (fixed point), so their sum is one value whatever the
// order, the path and the run.  s_acc[3]: the segment sums, rotating, so that a segment needs one barrier: segment i adds into
// s_acc[i % 3], everybody reads it behind the barrier, and thread 0 clears s_acc[(i + 2) % 3], which nobody touches before the
// next barrier.
template <bool LDS>
__global__ __launch_bounds__(ED_SIM_THREADS) void k_ed_simulate(EdSimArgs a) {
    extern __shared__ uint32_t s_cnt[];
    __shared__ unsigned long long s_acc[3];
    uint32_t *cnt = LDS ? s_cnt : a.gcounters + (uint64_t)blockIdx.x * a.n_feat;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, shift = 64u - a.guide_bits;
    for (uint32_t s = blockIdx.x; s < a.S; s += gridDim.x) {
        for (uint32_t j = tid; j < a.n_feat; j += ED_SIM_THREADS) cnt[j] = 0u;
        if (tid < 3) s_acc[tid] = 0ull;
        if (!LDS) __threadfence();
        __syncthreads();
        long long running = 0;
        for (uint32_t i = 0; i < a.D; i++) {
            const uint32_t lo = i ? a.dn[i - 1] : 0u, hi = a.dn[i];
            long long acc = 0;
            for (uint32_t b = (lo >> 2) + tid; b <= ((hi - 1u) >> 2); b += ED_SIM_THREADS) {
                unsigned long long w[4];
                cr_philox4x64_10((unsigned long long)b + 1ull, s, a.seed, w);
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) {
                    const unsigned long long t = 4ull * b + k;
                    if (t < lo || t >= hi) continue;
                    const double u = (double)(w[k] >> 11) * 0x1.0p-53;
                    uint32_t l = a.guide[w[k] >> shift], h = a.guide[(w[k] >> shift) + 1u];
                    while (l < h) {  // #{cdf <= u}
                        const uint32_t mid = (l + h) >> 1;
                        if (a.cdf[mid] <= u) l = mid + 1u; else h = mid;
                    }
                    const uint32_t j = min(l, a.n_feat - 1u);  // cdf[n_feat - 1] == 1 > u: l < n_feat already
                    const uint32_t c = atomicAdd(&cnt[j], 1u);
                    acc += a.lp[j] - a.lc[c];  // c < hi <= dn[D - 1]
                }
            }
            acc = wave_sum(acc);
            if (lane == 0 && acc != 0) atomicAdd(&s_acc[i % 3u], (unsigned long long)acc);
            __syncthreads();
            running += (long long)s_acc[i % 3u];
            if (tid == 0) s_acc[(i + 2u) % 3u] = 0ull;
            const double val = a.lgn[i] + (double)running * a.scale;
            for (uint32_t q = a.cand_start[i] + tid; q < a.cand_start[i + 1]; q += ED_SIM_THREADS) {
                const uint32_t c = a.order[q];
                if (val < a.obs[c]) atomicAdd(&a.n_lower[c], 1u);
            }
            if (a.table && tid == 0) a.table[(uint64_t)i * a.S + s] = val;
        }
        __syncthreads();
    }
}

// compute_ambient_pvalues (stats.py:205-231) against a table: n_lower[c] = #{s : table[row[c]][s] < obs[c]}; one wave per candidate
__global__ __launch_bounds__(256) void k_ed_count_lower(const double *__restrict__ table, uint32_t S, const uint32_t *__restrict__ row,
                                                        const double *__restrict__ obs, uint64_t n, uint32_t *__restrict__ n_lower) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave0; c < n; c += n_waves) {
        const double *t = table + (uint64_t)row[c] * S;
        const double o = obs[c];
        uint32_t k = 0;
        for (uint32_t s = lane; s < S; s += 64) k += t[s] < o ? 1u : 0u;
        k = wave_sum(k);
        if (lane == 0) n_lower[c] = k;
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// (1 + n_lower) / (1 + S), adjust_pvalue_bh (diffexp.py:88-97) and the calls.  The reference scales the p-values in descending
// order by n / k (k = n .. 1) and takes a running minimum: equal p-values meet their largest k first, so all of them get
// min(minimum so far, p * n / (number of p-values <= p)), whatever the argsort does with the ties.
static uint64_t ed_pvalues_bh(const std::vector<uint32_t> &n_lower, uint32_t S, double max_adj, std::vector<double> &p, std::vector<double> &adj,
                              std::vector<uint8_t> &call) {
    const size_t n = n_lower.size();
    std::vector<uint64_t> le((size_t)S + 2, 0);
    for (uint32_t v : n_lower) le[std::min<uint32_t>(v, S)]++;
    for (size_t v = 1; v <= S; v++) le[v] += le[v - 1];  // candidates with n_lower <= v
    std::vector<double> q((size_t)S + 1, 1.0);
    double run = INFINITY;
    for (size_t v = (size_t)S + 1; v-- > 0;) {
        if (le[v] == (v ? le[v - 1] : 0)) continue;  // no candidate at this level
        const double pv = (double)(1 + v) / (double)(1 + (uint64_t)S);
        run = std::min(run, (double)n / (double)le[v] * pv);
        q[v] = std::min(1.0, run);
    }
    p.resize(n);
    adj.resize(n);
    call.resize(n);
    uint64_t called = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t v = std::min<uint32_t>(n_lower[i], S);
        p[i] = (double)(1 + (uint64_t)v) / (double)(1 + (uint64_t)S);
        adj[i] = q[v];
        call[i] = adj[i] <= max_adj;
        called += call[i];
    }
    return called;
}

template <typename T>
static int ed_upload(crgpu_ctx *ctx, DevBuf &b, const std::vector<T> &h) {
    CR_TRY(dmalloc(ctx, b, std::max<size_t>(h.size(), 1) * sizeof(T)));
    if (!h.empty()) CR_TRY(crgpu_memcpy_h2d(ctx, b.p, h.data(), h.size() * sizeof(T)));
    return CRGPU_OK;
}
template <typename T>
static int ed_keep(crgpu_ctx *ctx, T **out, const T *h, size_t n) {  // a library-owned result array
    CR_TRY(cr_pool_alloc(ctx, (void **)out, std::max<size_t>(n, 1) * sizeof(T)));
    if (n) CR_TRY(crgpu_memcpy_h2d(ctx, *out, h, n * sizeof(T)));
    return CRGPU_OK;
}

extern "C" void crgpu_emptydrops_arrays_free(crgpu_ctx *ctx, crgpu_emptydrops_arrays *a) {
    if (!ctx || !a) return;
    CR_ENTER(ctx);
    void *ps[] = {a->d_eval_cols, a->d_umis, a->d_obs_loglk, a->d_n_lower, a->d_pvalues, a->d_pvalues_adj, a->d_is_nonambient,
                  a->d_called_cols, a->d_eval_features, a->d_profile_p, a->d_sim_n, a->d_sim_loglk};
    for (void *p : ps)
        if (p) cr_pool_free(ctx, p);
    memset(a, 0, sizeof(*a));
}

// n_lower -> p-values, BH, calls (device arrays of the caller, any may be NULL)
static int ed_finish(crgpu_ctx *ctx, const uint32_t *d_n_lower, uint64_t n, uint32_t S, double max_adj, double *d_p, double *d_adj,
                     uint8_t *d_call, std::vector<uint8_t> &call, uint64_t *n_called) {
    std::vector<uint32_t> nl(n);
    if (n) CR_TRY(crgpu_memcpy_d2h(ctx, nl.data(), d_n_lower, n * sizeof(uint32_t)));
    std::vector<double> p, adj;
    *n_called = ed_pvalues_bh(nl, S, max_adj, p, adj, call);
    if (n && d_p) CR_TRY(crgpu_memcpy_h2d(ctx, d_p, p.data(), n * sizeof(double)));
    if (n && d_adj) CR_TRY(crgpu_memcpy_h2d(ctx, d_adj, adj.data(), n * sizeof(double)));
    if (n && d_call) CR_TRY(crgpu_memcpy_h2d(ctx, d_call, call.data(), n));
    return CRGPU_OK;
}

// rows of a supplied table for the candidates' N (np.searchsorted(sim_n, umis), stats.py:221); a missing N is refused
static int ed_table_rows(crgpu_ctx *ctx, const int64_t *sim_n, uint32_t n_sim_n, const std::vector<uint32_t> &umis, std::vector<uint32_t> &row,
                         const char *who) {
    row.resize(umis.size());
    for (size_t i = 0; i < umis.size(); i++) {
        const int64_t *it = std::lower_bound(sim_n, sim_n + n_sim_n, (int64_t)umis[i]);
        CR_REQUIRE(ctx, it != sim_n + n_sim_n && *it == (int64_t)umis[i], CRGPU_EINVAL, "%s: the table has no row for N = %u", who, umis[i]);
        row[i] = (uint32_t)(it - sim_n);
    }
    return CRGPU_OK;
}

extern "C" int crgpu_ambient_pvalues_dev(crgpu_ctx *ctx, const uint32_t *d_umis, const double *d_obs_loglk, uint64_t n, const int64_t *sim_n,
                                         uint32_t n_sim_n, const double *d_sim_loglk, uint32_t num_sims, double max_adj_pvalue,
                                         uint32_t *d_n_lower_out, double *d_pvalues_out, double *d_pvalues_adj_out,
                                         uint8_t *d_is_nonambient_out, uint64_t *n_nonambient_out) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    if (n_nonambient_out) *n_nonambient_out = 0;
    if (!n) return CRGPU_OK;
    CR_REQUIRE(ctx, d_umis && d_obs_loglk && sim_n && n_sim_n && d_sim_loglk && num_sims && n < 0x80000000ull, CRGPU_EINVAL,
               "crgpu_ambient_pvalues_dev: NULL or empty argument");
    for (uint32_t i = 1; i < n_sim_n; i++)
        CR_REQUIRE(ctx, sim_n[i - 1] < sim_n[i], CRGPU_EINVAL, "crgpu_ambient_pvalues_dev: sim_n must ascend strictly");
    std::vector<uint32_t> umis(n), row;
    CR_TRY(crgpu_memcpy_d2h(ctx, umis.data(), d_umis, n * sizeof(uint32_t)));
    CR_TRY(ed_table_rows(ctx, sim_n, n_sim_n, umis, row, "crgpu_ambient_pvalues_dev"));
    DevBuf row_b, nl_b;
    CR_TRY(ed_upload(ctx, row_b, row));
    uint32_t *d_nl = d_n_lower_out;
    if (!d_nl) {
        CR_TRY(dmalloc(ctx, nl_b, n * sizeof(uint32_t)));
        d_nl = nl_b.as<uint32_t>();
    }
    hipLaunchKernelGGL(k_ed_count_lower, dim3(cr_grid(n * 64, 256)), dim3(256), 0, ctx->stream, d_sim_loglk, num_sims, row_b.as<uint32_t>(),
                       d_obs_loglk, n, d_nl);
    CR_HIP(ctx, hipGetLastError());
    std::vector<uint8_t> call;
    uint64_t called = 0;
    CR_TRY(ed_finish(ctx, d_nl, n, num_sims, max_adj_pvalue, d_pvalues_out, d_pvalues_adj_out, d_is_nonambient_out, call, &called));
    if (n_nonambient_out) *n_nonambient_out = called;
    return CRGPU_OK;
}

// simulate_multinomial_loglikelihoods' replacement for the candidates' totals `umis` (all > 0): d_n_lower[c] = simulations whose
// value at N = umis[c] is strictly below d_obs[c] (d_obs == NULL: nothing is compared, d_n_lower may be NULL), d_table
// (nullable) = the values, (distinct N ascending) x S
static int ed_simulate(crgpu_ctx *ctx, const std::vector<double> &profile_p, const std::vector<uint32_t> &umis, const double *d_obs, uint32_t S,
                       uint64_t seed, uint32_t *d_n_lower, double *d_table, float *ms_out, bool *lds_out) {
    const size_t F = profile_p.size();
    const uint32_t n_cand = (uint32_t)umis.size();
    std::vector<uint32_t> order(n_cand), dn, cand_start;
    for (uint32_t i = 0; i < n_cand; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return umis[x] < umis[y]; });
    for (uint32_t q = 0; q < n_cand; q++)
        if (!q || umis[order[q]] != dn.back()) {
            dn.push_back(umis[order[q]]);
            cand_start.push_back(q);
        }
    cand_start.push_back(n_cand);
    if (!d_obs) std::fill(cand_start.begin(), cand_start.end(), 0u);  // no candidate is compared
    const uint32_t D = (uint32_t)dn.size(), nmax = dn.back();
    double max_abs_logp = 0.0;
    for (double p : profile_p) max_abs_logp = std::max(max_abs_logp, std::fabs(std::log(p)));
    // fixed point: every term is rounded to 2^-bits (<= 2^-(bits + 1) off), two terms per draw: the value at N is within
    // N * 2^-bits of the f64 sum.  |sum| <= N * (max |log p| + log N) must stay below 2^62.
    const double bound = (double)nmax * (max_abs_logp + std::log((double)nmax + 1.0)) + 1.0;
    int bits = ED_FIXED_BITS;
    while (bits > 0 && std::ldexp(bound, bits) >= 0x1.0p62) bits--;
    CR_REQUIRE(ctx, bits >= 20, CRGPU_ERANGE, "EmptyDrops simulation: log-likelihoods of %u draws do not fit the fixed-point sum", nmax);
    std::vector<long long> lp(F), lc(nmax);
    for (size_t j = 0; j < F; j++) lp[j] = std::llrint(std::ldexp(std::log(profile_p[j]), bits));
    for (uint32_t c = 0; c < nmax; c++) lc[c] = std::llrint(std::ldexp(std::log((double)c + 1.0), bits));
    std::vector<double> cdf(F), lgn(D);
    double run = 0.0;
    for (size_t j = 0; j < F; j++) cdf[j] = run += profile_p[j];  // np.cumsum: sequential
    for (size_t j = 0; j < F; j++) cdf[j] /= run;
    for (uint32_t i = 0; i < D; i++) lgn[i] = std::lgamma((double)dn[i] + 1.0);
    const uint32_t gbits = std::min<uint32_t>(20, std::max<uint32_t>(8, cr_ceil_log2(F) + 2));
    std::vector<uint32_t> guide(((size_t)1 << gbits) + 1);
    {
        size_t k = 0;
        for (size_t b = 0; b < guide.size(); b++) {
            const double edge = std::ldexp((double)b, -(int)gbits);
            while (k < F && cdf[k] <= edge) k++;
            guide[b] = (uint32_t)k;
        }
    }
    DevBuf cdf_b, guide_b, lp_b, lc_b, dn_b, lgn_b, cs_b, ord_b, gcnt_b;
    CR_TRY(ed_upload(ctx, cdf_b, cdf));
    CR_TRY(ed_upload(ctx, guide_b, guide));
    CR_TRY(ed_upload(ctx, lp_b, lp));
    CR_TRY(ed_upload(ctx, lc_b, lc));
    CR_TRY(ed_upload(ctx, dn_b, dn));
    CR_TRY(ed_upload(ctx, lgn_b, lgn));
    CR_TRY(ed_upload(ctx, cs_b, cand_start));
    CR_TRY(ed_upload(ctx, ord_b, order));
    if (d_n_lower) CR_HIP(ctx, hipMemsetAsync(d_n_lower, 0, (uint64_t)n_cand * sizeof(uint32_t), ctx->stream));
    const uint32_t lds_cap = std::min<uint32_t>(ctx->ed_lds_features, ED_LDS_BYTES / sizeof(uint32_t));
    const bool lds = F <= lds_cap;
    const uint32_t grid = std::min<uint32_t>(S, lds ? 1024u : 512u);
    if (!lds) CR_TRY(dmalloc(ctx, gcnt_b, (uint64_t)grid * F * sizeof(uint32_t)));
    EdSimArgs a{cdf_b.as<double>(), guide_b.as<uint32_t>(), gbits, (uint32_t)F, lp_b.as<long long>(), lc_b.as<long long>(),
                dn_b.as<uint32_t>(), lgn_b.as<double>(), D, S, std::ldexp(1.0, -bits), cs_b.as<uint32_t>(), ord_b.as<uint32_t>(),
                d_obs, d_n_lower, d_table, (unsigned long long)seed, lds ? nullptr : gcnt_b.as<uint32_t>()};
    hipEvent_t e0 = nullptr, e1 = nullptr;
    CR_HIP(ctx, hipEventCreate(&e0));
    if (hipEventCreate(&e1) != hipSuccess) {
        (void)hipEventDestroy(e0);
        return cr_fail(ctx, CRGPU_EHIP, "EmptyDrops simulation: no event");
    }
    (void)hipEventRecord(e0, ctx->stream);
    if (lds) {
        const size_t bytes = F * sizeof(uint32_t);
        cr_allow_lds(ctx, (const void *)k_ed_simulate<true>, bytes);
        hipLaunchKernelGGL(k_ed_simulate<true>, dim3(grid), dim3(ED_SIM_THREADS), bytes, ctx->stream, a);
    } else {
        hipLaunchKernelGGL(k_ed_simulate<false>, dim3(grid), dim3(ED_SIM_THREADS), 0, ctx->stream, a);
    }
    (void)hipEventRecord(e1, ctx->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventSynchronize(e1);  // the temporaries above go back to the pool behind this
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (e != hipSuccess) return cr_fail(ctx, CRGPU_EHIP, "EmptyDrops simulation: %s", hipGetErrorString(e));
    *ms_out = ms;
    *lds_out = lds;
    return CRGPU_OK;
}

// Test and measurement hook (crgpu.h): the simulation on a given profile
extern "C" int crgpu_emptydrops_simulate_dev(crgpu_ctx *ctx, const double *profile_p, uint32_t n_features, const uint32_t *umis,
                                             const double *obs_loglk, uint64_t n, uint32_t num_sims, uint64_t seed, int64_t *sim_n_out,
                                             uint32_t *n_distinct_out, double *sim_loglk_out, uint32_t *n_lower_out, double *ms_out) {
    if (!ctx || !n_distinct_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *n_distinct_out = 0;
    CR_REQUIRE(ctx, profile_p && n_features && umis && n && n < 0x80000000ull && num_sims >= 1 && num_sims <= (1u << 24), CRGPU_EINVAL,
               "crgpu_emptydrops_simulate_dev: NULL or empty argument");
    std::vector<double> p(profile_p, profile_p + n_features);
    std::vector<uint32_t> u(umis, umis + n), dn(umis, umis + n);
    for (double x : p) CR_REQUIRE(ctx, x > 0.0 && x <= 1.0, CRGPU_EINVAL, "crgpu_emptydrops_simulate_dev: probabilities must be in (0, 1]");
    for (uint32_t x : u) CR_REQUIRE(ctx, x > 0, CRGPU_EINVAL, "crgpu_emptydrops_simulate_dev: totals must be positive");
    std::sort(dn.begin(), dn.end());
    dn.erase(std::unique(dn.begin(), dn.end()), dn.end());
    const uint32_t D = (uint32_t)dn.size();
    *n_distinct_out = D;
    for (uint32_t i = 0; sim_n_out && i < D; i++) sim_n_out[i] = dn[i];
    DevBuf obs_b, nl_b, tab_b;
    if (obs_loglk) {
        CR_TRY(dmalloc(ctx, obs_b, n * sizeof(double)));
        CR_TRY(crgpu_memcpy_h2d(ctx, obs_b.p, obs_loglk, n * sizeof(double)));
        CR_TRY(dmalloc(ctx, nl_b, n * sizeof(uint32_t)));
    }
    if (sim_loglk_out) {
        CR_REQUIRE(ctx, (uint64_t)D * num_sims <= (1ull << 27), CRGPU_ERANGE, "crgpu_emptydrops_simulate_dev: a table of at most 2^27 values");
        CR_TRY(dmalloc(ctx, tab_b, (uint64_t)D * num_sims * sizeof(double)));
    }
    float ms = 0.f;
    bool lds = false;
    CR_TRY(ed_simulate(ctx, p, u, obs_loglk ? obs_b.as<double>() : nullptr, num_sims, seed, obs_loglk ? nl_b.as<uint32_t>() : nullptr,
                       sim_loglk_out ? tab_b.as<double>() : nullptr, &ms, &lds));
    if (sim_loglk_out) CR_TRY(crgpu_memcpy_d2h(ctx, sim_loglk_out, tab_b.p, (uint64_t)D * num_sims * sizeof(double)));
    if (obs_loglk && n_lower_out) CR_TRY(crgpu_memcpy_d2h(ctx, n_lower_out, nl_b.p, n * sizeof(uint32_t)));
    if (ms_out) *ms_out = ms;
    return CRGPU_OK;
}

static int ed_run(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint8_t *feature_mask, uint32_t n_features, const uint32_t *d_bc_counts,
                  const uint64_t *d_cell_cols, uint64_t n_cells, uint64_t low, uint64_t high, uint64_t min_umis, uint32_t S, double max_adj,
                  uint64_t seed, const int64_t *sim_n, uint32_t n_sim_n, const double *sim_loglk, uint32_t flags,
                  crgpu_emptydrops_result *res, crgpu_emptydrops_arrays *out) {
    const uint64_t V = m->n_barcodes;
    const long long *indptr = (const long long *)m->d_indptr;
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, *d_total = ctx->d_scalars + CR_SCALAR_TOTAL, *d_aux = ctx->d_scalars + CR_SCALAR_FLAG_AUX, flag = 0;
    std::vector<uint64_t> cells(n_cells);
    if (n_cells) CR_TRY(crgpu_memcpy_d2h(ctx, cells.data(), d_cell_cols, n_cells * sizeof(uint64_t)));
    for (uint64_t i = 0; i < n_cells; i++)
        CR_REQUIRE(ctx, cells[i] < V && (!i || cells[i - 1] < cells[i]), CRGPU_EINVAL,
                   "crgpu_emptydrops_dev: the initial cells must be ascending columns of the matrix");
    // every way out without additional cells: the merged list is the initial one
    auto no_cells = [&](int status) -> int {
        res->status = status;
        out->n_called = n_cells;
        return ed_keep(ctx, &out->d_called_cols, cells.data(), (size_t)n_cells);
    };
    res->emptydrops_minimum_umis = min_umis;
    if (!V) return no_cells(CRGPU_ED_NO_AMBIENT);

    DevBuf mask_b;
    if (feature_mask) {
        CR_TRY(dmalloc(ctx, mask_b, n_features));
        CR_TRY(crgpu_memcpy_h2d(ctx, mask_b.p, feature_mask, n_features));
    } else if (!n_features) {  // the rows the matrix uses
        CR_HIP(ctx, hipMemsetAsync(d_aux, 0, sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(k_ed_max_row, dim3(cr_grid(m->nnz, 256)), dim3(256), 0, ctx->stream, m->d_indices, m->nnz, d_aux);
        CR_HIP(ctx, hipGetLastError());
        CR_TRY(read_u32(ctx, d_aux, &n_features));
        if (!n_features) n_features = 1;
    }
    const uint8_t *d_mask = feature_mask ? mask_b.as<uint8_t>() : nullptr;

    // 1. the descending order of ALL columns (np.argsort(kind="stable")[::-1]) and its places [low, high)
    const uint64_t p0 = std::min<uint64_t>(low, V), p1 = std::min<uint64_t>(std::max(high, low), V);
    DevBuf key_b, keyt_b, val_b, valt_b, rowsum_b, any_b;
    for (DevBuf *b : {&key_b, &keyt_b, &val_b, &valt_b}) CR_TRY(dmalloc(ctx, *b, V * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, rowsum_b, (uint64_t)n_features * sizeof(unsigned long long)));
    CR_TRY(dmalloc(ctx, any_b, n_features));
    CR_HIP(ctx, hipMemsetAsync(rowsum_b.p, 0, (uint64_t)n_features * sizeof(unsigned long long), ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(any_b.p, 0, n_features, ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, 2 * sizeof(uint32_t), ctx->stream));  // d_flag, d_aux
    uint32_t max_bg = 0, n_used = 0;
    if (p1 > p0) {
        hipLaunchKernelGGL(k_om_keys, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, d_bc_counts, (uint32_t)V, key_b.as<uint32_t>(),
                           val_b.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
        bool in_tmp = false;
        CR_TRY(cr_radix_sort_u32(ctx, key_b.as<uint32_t>(), keyt_b.as<uint32_t>(), val_b.as<uint32_t>(), valt_b.as<uint32_t>(), V, 0, 32, &in_tmp));
        const uint32_t *key = in_tmp ? keyt_b.as<uint32_t>() : key_b.as<uint32_t>(), *val = in_tmp ? valt_b.as<uint32_t>() : val_b.as<uint32_t>();
        CR_TRY(read_u32(ctx, key + p0, &max_bg));
        max_bg = ~max_bg;  // the first place of the slice holds its largest total
        hipLaunchKernelGGL(k_ed_ambient_rows, dim3(cr_grid((p1 - p0) * 64, 256)), dim3(256), 0, ctx->stream, key, val, p0, p1, indptr,
                           m->d_indices, m->d_data, d_mask, n_features, rowsum_b.as<unsigned long long>(), d_aux);
        CR_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_ed_rows_present, dim3(cr_grid(m->nnz, 256)), dim3(256), 0, ctx->stream, m->d_indices, m->d_data, m->nnz, d_mask,
                       n_features, any_b.as<uint8_t>(), d_flag);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !flag, CRGPU_EINVAL, "crgpu_emptydrops_dev: the matrix holds a row >= n_features (%u)", n_features);
    CR_TRY(read_u32(ctx, d_aux, &n_used));
    res->n_ambient_used = n_used;
    res->max_background_umis = max_bg;
    const uint64_t thr = std::max<uint64_t>(min_umis, 1ull + max_bg);
    res->emptydrops_minimum_umis = thr;

    // 2./3. the profile over eval_features, smoothed
    std::vector<unsigned long long> rowsum(n_features);
    std::vector<uint8_t> any(n_features);
    CR_TRY(crgpu_memcpy_d2h(ctx, rowsum.data(), rowsum_b.p, (uint64_t)n_features * sizeof(unsigned long long)));
    CR_TRY(crgpu_memcpy_d2h(ctx, any.data(), any_b.p, n_features));
    std::vector<uint32_t> eval_features;
    for (uint32_t f = 0; f < n_features; f++)
        if (any[f]) eval_features.push_back(f);
    const size_t F = eval_features.size();
    res->n_eval_features = F;
    if (!n_used || !F) return no_cells(CRGPU_ED_NO_AMBIENT);
    std::vector<double> profile_p(F);
    {
        std::vector<uint64_t> freq;
        for (uint32_t f : eval_features)
            if (rowsum[f]) freq.push_back(rowsum[f]);
        std::vector<double> pstar(freq.size());
        const int st = ed_sgt(freq.data(), freq.size(), pstar.data(), &res->sgt_p0, &res->sgt_slope);
        if (st != CRGPU_OK) return no_cells(CRGPU_ED_SGT_NOT_APPLICABLE);
        const size_t n0 = F - freq.size();
        double sum = 0.0;
        for (double x : pstar) sum += x;
        size_t k = 0;
        for (size_t j = 0; j < F; j++) {
            if (rowsum[eval_features[j]])
                profile_p[j] = n0 ? pstar[k++] : pstar[k++] / sum;  // no zero class: renormalised (cell_calling.py:68-70)
            else
                profile_p[j] = res->sgt_p0 / (double)n0;
        }
    }
    if (flags & CRGPU_ED_KEEP_PROFILE) {
        out->n_eval_features = F;
        CR_TRY(ed_keep(ctx, &out->d_eval_features, eval_features.data(), F));
        CR_TRY(ed_keep(ctx, &out->d_profile_p, profile_p.data(), F));
    }
    if (!n_cells) return no_cells(CRGPU_ED_NO_CELLS);

    // 4. candidates
    uint32_t n_cand = 0;
    DevBuf cell_b;
    CR_TRY(dmalloc(ctx, cell_b, V));
    CR_HIP(ctx, hipMemsetAsync(cell_b.p, 0, V, ctx->stream));
    cr_check_columns<false>(ctx, d_cell_cols, n_cells, V, MarkByte{cell_b.as<uint8_t>()}, d_flag);
    CR_HIP(ctx, hipGetLastError());
    if (thr <= 0xFFFFFFFFull) {
        CR_TRY(cr_pool_alloc(ctx, (void **)&out->d_eval_cols, V * sizeof(uint64_t)));
        CR_TRY(cr_pool_alloc(ctx, (void **)&out->d_umis, V * sizeof(uint32_t)));
        CR_TRY(compact(ctx, EdCandFlag{d_bc_counts, cell_b.as<uint8_t>(), (uint32_t)thr}, EdCandEmit{d_bc_counts, out->d_eval_cols, out->d_umis}, V,
                       ctx->d_sort_hist, d_total));
        CR_TRY(read_u32(ctx, d_total, &n_cand));
    }
    res->n_candidates = n_cand;
    if (!n_cand) return no_cells(CRGPU_ED_NO_CANDIDATES);
    out->n_candidates = n_cand;
    std::vector<uint32_t> umis(n_cand);
    CR_TRY(crgpu_memcpy_d2h(ctx, umis.data(), out->d_umis, (uint64_t)n_cand * sizeof(uint32_t)));
    std::vector<uint32_t> dn(umis);
    std::sort(dn.begin(), dn.end());
    dn.erase(std::unique(dn.begin(), dn.end()), dn.end());
    const uint32_t D = (uint32_t)dn.size(), nmax = dn.back();
    res->n_distinct_n = D;

    // 5. observed log-likelihoods
    std::vector<double> logp_rows(n_features, 0.0), lgam((size_t)nmax + 1);
    for (size_t j = 0; j < F; j++) logp_rows[eval_features[j]] = std::log(profile_p[j]);
    for (uint32_t c = 0; c <= nmax; c++) lgam[c] = std::lgamma((double)c + 1.0);
    DevBuf logp_b, lgam_b;
    CR_TRY(ed_upload(ctx, logp_b, logp_rows));
    CR_TRY(ed_upload(ctx, lgam_b, lgam));
    CR_TRY(cr_pool_alloc(ctx, (void **)&out->d_obs_loglk, (uint64_t)n_cand * sizeof(double)));
    hipLaunchKernelGGL(k_ed_observed, dim3(cr_grid((uint64_t)n_cand * 64, 256)), dim3(256), 0, ctx->stream, out->d_eval_cols, out->d_umis,
                       (uint64_t)n_cand, indptr, m->d_indices, m->d_data, d_mask, n_features, logp_b.as<double>(), lgam_b.as<double>(), nmax,
                       out->d_obs_loglk, d_flag);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !flag, CRGPU_EINVAL, "crgpu_emptydrops_dev: the counts are not the column sums of the matrix, or a cell column is out of range");

    // 6. n_lower: from the supplied table, or from the simulation
    CR_TRY(cr_pool_alloc(ctx, (void **)&out->d_n_lower, (uint64_t)n_cand * sizeof(uint32_t)));
    out->num_sims = S;
    if (sim_n) {
        std::vector<uint32_t> row;
        CR_TRY(ed_table_rows(ctx, sim_n, n_sim_n, umis, row, "crgpu_emptydrops_dev"));
        DevBuf row_b, tab_b;
        CR_TRY(ed_upload(ctx, row_b, row));
        CR_TRY(dmalloc(ctx, tab_b, (uint64_t)n_sim_n * S * sizeof(double)));
        CR_TRY(crgpu_memcpy_h2d(ctx, tab_b.p, sim_loglk, (uint64_t)n_sim_n * S * sizeof(double)));
        hipLaunchKernelGGL(k_ed_count_lower, dim3(cr_grid((uint64_t)n_cand * 64, 256)), dim3(256), 0, ctx->stream, tab_b.as<double>(), S,
                           row_b.as<uint32_t>(), out->d_obs_loglk, (uint64_t)n_cand, out->d_n_lower);
        CR_HIP(ctx, hipGetLastError());
        CR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // tab_b and row_b go back to the pool
    } else {
        if (flags & CRGPU_ED_KEEP_SIM_TABLE) {
            CR_REQUIRE(ctx, (uint64_t)D * S <= (1ull << 27), CRGPU_ERANGE,
                       "crgpu_emptydrops_dev: a simulated table of %u x %u values is not kept (at most 2^27)", D, S);
            std::vector<int64_t> dn64(dn.begin(), dn.end());
            out->n_distinct_n = D;
            CR_TRY(ed_keep(ctx, &out->d_sim_n, dn64.data(), (size_t)D));
            CR_TRY(cr_pool_alloc(ctx, (void **)&out->d_sim_loglk, (uint64_t)D * S * sizeof(double)));
        }
        float ms = 0.f;
        bool lds = false;
        CR_TRY(ed_simulate(ctx, profile_p, umis, out->d_obs_loglk, S, seed, out->d_n_lower, out->d_sim_loglk, &ms, &lds));
        res->sim_ms = ms;
        res->sim_in_lds = lds;
    }

    // 7. p-values, BH, calls   8. merge
    CR_TRY(cr_pool_alloc(ctx, (void **)&out->d_pvalues, (uint64_t)n_cand * sizeof(double)));
    CR_TRY(cr_pool_alloc(ctx, (void **)&out->d_pvalues_adj, (uint64_t)n_cand * sizeof(double)));
    CR_TRY(cr_pool_alloc(ctx, (void **)&out->d_is_nonambient, n_cand));
    std::vector<uint8_t> call;
    uint64_t called = 0;
    CR_TRY(ed_finish(ctx, out->d_n_lower, n_cand, S, max_adj, out->d_pvalues, out->d_pvalues_adj, out->d_is_nonambient, call, &called));
    res->n_nonambient = called;
    std::vector<uint64_t> eval_cols(n_cand), merged;
    CR_TRY(crgpu_memcpy_d2h(ctx, eval_cols.data(), out->d_eval_cols, (uint64_t)n_cand * sizeof(uint64_t)));
    merged.reserve(n_cells + called);
    size_t ci = 0;
    for (uint32_t i = 0; i < n_cand; i++) {
        if (!call[i]) continue;
        while (ci < n_cells && cells[ci] < eval_cols[i]) merged.push_back(cells[ci++]);
        merged.push_back(eval_cols[i]);
    }
    while (ci < n_cells) merged.push_back(cells[ci++]);
    out->n_called = merged.size();
    return ed_keep(ctx, &out->d_called_cols, merged.data(), merged.size());
}

extern "C" int crgpu_emptydrops_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint8_t *feature_mask, uint32_t n_features,
                                    const uint32_t *d_bc_counts, const uint64_t *d_cell_cols, uint64_t n_cells, uint64_t low, uint64_t high,
                                    uint64_t emptydrops_minimum_umis, uint32_t num_sims, double max_adj_pvalue, uint64_t seed,
                                    const int64_t *sim_n, uint32_t n_sim_n, const double *sim_loglk, uint32_t flags,
                                    crgpu_emptydrops_result *res, crgpu_emptydrops_arrays *out) {
    if (!ctx || !m || !res || !out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    memset(res, 0, sizeof(*res));
    memset(out, 0, sizeof(*out));
    CR_REQUIRE(ctx, m->n_barcodes == 0 || d_bc_counts, CRGPU_EINVAL, "crgpu_emptydrops_dev: NULL counts");
    CR_REQUIRE(ctx, m->n_barcodes < 0x80000000ull, CRGPU_ERANGE, "crgpu_emptydrops_dev: at most 2^31 - 1 columns");
    CR_REQUIRE(ctx, n_cells == 0 || d_cell_cols, CRGPU_EINVAL, "crgpu_emptydrops_dev: NULL cell columns");
    CR_REQUIRE(ctx, !feature_mask || n_features, CRGPU_EINVAL, "crgpu_emptydrops_dev: a feature mask needs n_features");
    CR_REQUIRE(ctx, num_sims >= 1 && num_sims <= (1u << 24), CRGPU_EINVAL, "crgpu_emptydrops_dev: num_sims must be 1 .. 2^24");
    CR_REQUIRE(ctx, !sim_n == !sim_loglk && (!sim_n || n_sim_n), CRGPU_EINVAL, "crgpu_emptydrops_dev: a supplied table needs sim_n and sim_loglk");
    for (uint32_t i = 1; sim_n && i < n_sim_n; i++)
        CR_REQUIRE(ctx, sim_n[i - 1] < sim_n[i], CRGPU_EINVAL, "crgpu_emptydrops_dev: sim_n must ascend strictly");
    const int rc = ed_run(ctx, m, feature_mask, n_features, d_bc_counts, d_cell_cols, n_cells, low, high, emptydrops_minimum_umis, num_sims,
                          max_adj_pvalue, seed, sim_n, n_sim_n, sim_loglk, flags, res, out);
    if (rc != CRGPU_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        crgpu_emptydrops_arrays_free(ctx, out);
    }
    return rc;
}
