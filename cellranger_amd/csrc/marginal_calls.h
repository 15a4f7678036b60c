// marginal_calls.h -- "is this feature present in this cell, above background": the marginal caller of guides, tags and antibodies
// on the device (part of matrix_stages.hip).
//
// Replaces call_presence_with_gmm_ab (lib/python/cellranger/feature/feature_assigner.py:213-230) under GuideAssigner,
// AntibodyOrAntigenAssigner and TagAssigner: per feature row a tied two-component Gaussian mixture on log10(1 + count) over ALL
// cells, scikit-learn 1.7.2's GaussianMixture(n_components = 2, n_init = 10, covariance_type = "tied", random_state = 0), then
// predict.  Everything after the k-means++ seeding sees the counts only through the histogram of the row's distinct values (the
// zeros are one bin of V - nnz(row)); the seeding needs the cumulative squared distance in CELL order, which a sparse row gives
// with its zero gaps in closed form.
//   guards kept   a row whose maximum is 0, or V < 2, is not fitted and has no calls (CRGPU_MC_SKIPPED)
//   QUIRK kept    a row of one distinct value is fitted: the second cluster stays empty (mean 0, weight of a few eps) and every
//                 cell whose count meets the threshold is called
//   the stream    RandomState(0) anew per feature: init j draws one double for choice(V, p = uniform) and two for the trial
//                 candidates; the 30 doubles and the 10 first cells depend on V alone (mc_seed_draws, host)
//
// Launch structure.
//   k_mc_count / k_mc_scatter   a thread per column: its entries in listed rows -> keys (place << 32 | column) with the count as
//                               payload, in CSC order behind an exclusive scan; the library's radix sort orders them by (row,
//                               column): CSR over the listed rows, columns ascending.  A second sort of (place << 32 | count)
//                               gives the values of a row ascending.  Keys are unique or ordered whole, so the order is fixed.
//   k_mc_rowptr                 the first key of every listed row (binary search)
//   k_mc_hist                   a workgroup per row: the heads of the runs of equal counts, compacted in order -> (value,
//                               multiplicity, x); x = log10(1 + value) from a HOST table (numpy's own values through the C
//                               library) for value < 65536, the device's log10 above
//   k_mc_fit<NW, LDS>           a workgroup of NW waves per (row, init): seeding, Lloyd, EM.  NW = 1 for a row of at most
//                               MC_WAVE_VALUES distinct values and MC_WAVE_ENTRIES entries, else 4: it depends on the row alone.  The histogram (x, multiplicity
//                               as f64) sits in LDS up to ctx->mc_lds_values values (CRGPU_MC_LDS_VALUES), else it is read from
//                               device memory; nothing else differs.
//   k_mc_assign                 a workgroup per row: the winner (the first init with the strictly largest lower bound), predict per
//                               distinct value, the positive component, the row's tallies
//   k_mc_emit                   a workgroup per row: the assigned columns in order behind the scan of the rows' tallies
//   k_mc_cells                  a thread per column: features_per_cell and the four cell tallies (integer sums)
// Every floating-point sum has ONE order that depends on the row alone: thread t adds the items t, t + 64 NW, ... ascending, a wave
// adds its lanes by the xor butterfly, lane 0 adds the waves ascending.  The cell-order scan takes tiles of 64 NW entries: an
// inclusive scan by shuffles inside a wave, the waves ascending, the carry of the tiles before.  No floating-point atomic, no
// global atomic on a row; a (row, init) reads nothing another one writes: a row's result does not depend on the grid, on the other
// rows of the call or on the run.  f64 throughout, unfused (-ffp-contract=off).
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "cell_calling.h"
#include "stage_common.h"

#define MC_INITS CRGPU_MC_INITS
#define MC_WAVE_VALUES 256u   // a row of at most this many distinct values and at most MC_WAVE_ENTRIES entries is fitted by one wave,
#define MC_WAVE_ENTRIES 4096u // any other by four: the Lloyd / EM sums run over the values, the cell-order scan over the entries
#define MC_LOG_TABLE 65536u   // counts below this take log10(1 + count) from the host table
#define MC_KM_MAX_ITER 300u
#define MC_KM_TOL 1e-4
#define MC_EPS10 (10.0 * 2.220446049250313e-16)
#define MC_OUT 6u  // per (row, init): w0, w1, mu0, mu1, covariance, lower bound

struct crgpu_marginal_calls_impl {
    crgpu_marginal_calls view;
    std::vector<crgpu_marginal_row> rows;
    void *d_indptr = nullptr, *d_columns = nullptr, *d_fpc = nullptr, *d_hoff = nullptr, *d_hval = nullptr, *d_hmul = nullptr;
};

// ---- the random stream (host) --------------------------------------------------------------------------------------------------------
struct McMt {
    uint32_t mt[MT_N];
    uint32_t pos = MT_N;
    explicit McMt(uint32_t seed) { mt_init_genrand(seed, mt); }
    uint32_t next() {
        if (pos >= MT_N) {
            for (uint32_t k = 0; k < MT_N; k++) {
                const uint32_t y = (mt[k] & 0x80000000u) | (mt[(k + 1) % MT_N] & 0x7fffffffu);
                mt[k] = mt[(k + 397) % MT_N] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            pos = 0;
        }
        return mt_temper(mt[pos++]);
    }
    double random_sample() {  // genrand_res53
        const uint32_t a = next() >> 5, b = next() >> 6;
        return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    }
};

// u_out[3 j .. 3 j + 3): the double of init j's choice and the two of its trial candidates; first_cell_out[j]: the reference's own
// p.cumsum(), cdf /= cdf[-1], searchsorted(side = "right"), done sequentially
static void mc_seed_draws(uint64_t V, double *u_out, uint64_t *first_cell_out) {
    McMt g(0u);
    for (uint32_t i = 0; i < 3u * MC_INITS; i++) u_out[i] = g.random_sample();
    if (!V) {
        for (uint32_t j = 0; j < MC_INITS; j++) first_cell_out[j] = 0;
        return;
    }
    const double p = 1.0 / (double)V;
    std::vector<double> cdf(V);
    double s = 0.0;
    for (uint64_t i = 0; i < V; i++) s += p, cdf[i] = s;
    const double last = cdf[V - 1];
    for (uint64_t i = 0; i < V; i++) cdf[i] /= last;
    for (uint32_t j = 0; j < MC_INITS; j++) {
        const uint64_t c = (uint64_t)(std::upper_bound(cdf.begin(), cdf.end(), u_out[3u * j]) - cdf.begin());
        first_cell_out[j] = c < V ? c : V - 1;
    }
}

extern "C" int crgpu_marginal_seed_draws(uint64_t V, double *u_out, uint64_t *first_cell_out) {
    if (!u_out || !first_cell_out || !V) return CRGPU_EINVAL;
    mc_seed_draws(V, u_out, first_cell_out);
    return CRGPU_OK;
}

// ---- row extraction --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_mc_count(const long long *__restrict__ indptr, const int32_t *__restrict__ indices, uint64_t V,
                                                  const uint32_t *__restrict__ place, uint32_t n_features, uint32_t *__restrict__ cnt,
                                                  uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < V; c += stride) {
        uint32_t n = 0;
        for (long long e = indptr[c]; e < indptr[c + 1]; e++) {
            const uint32_t f = (uint32_t)indices[e];
            if (f >= n_features) atomicOr(flag, 4u);
            else if (place[f]) n++;
        }
        cnt[c] = n;
    }
}
__global__ __launch_bounds__(256) void k_mc_scatter(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    const int32_t *__restrict__ data, uint64_t V, const uint32_t *__restrict__ place,
                                                    uint32_t n_features, const uint32_t *__restrict__ off, uint64_t n_ent,
                                                    uint64_t *__restrict__ key_col, uint32_t *__restrict__ val, uint64_t *__restrict__ key_cnt,
                                                    uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < V; c += stride) {
        uint64_t o = off[c];
        for (long long e = indptr[c]; e < indptr[c + 1]; e++) {
            const uint32_t f = (uint32_t)indices[e];
            if (f >= n_features) continue;
            const uint32_t p = place[f];
            if (!p) continue;
            const int32_t d = data[e];
            if (d <= 0) {  // a stored zero or a negative count: not a count matrix
                atomicOr(flag, 8u);
                continue;
            }
            if (o >= n_ent) break;  // cannot happen: off is the scan of the same walk
            key_col[o] = ((uint64_t)(p - 1u) << 32) | (uint64_t)c;
            key_cnt[o] = ((uint64_t)(p - 1u) << 32) | (uint64_t)(uint32_t)d;
            val[o] = (uint32_t)d;
            o++;
        }
    }
}
// rowptr[p] = the first sorted key of row p or a later one; rowptr[n_rows] = n_ent
__global__ __launch_bounds__(256) void k_mc_rowptr(const uint64_t *__restrict__ keys, uint64_t n_ent, uint32_t n_rows, uint32_t *__restrict__ rowptr) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > n_rows) return;
    rowptr[p] = (uint32_t)cr_lower_bound(keys, n_ent, (uint64_t)p << 32);
}

// ---- the distinct-value histogram -------------------------------------------------------------------------------------------------------
// Row p owns the slots [rowptr[p] + p, rowptr[p + 1] + p + 1) of hval / hmul / hx; nd[p] of them are used.  keys: (place << 32 | count)
// ascending.  The zeros come first: one bin of V - nnz(row).  total[p] = the row's UMIs.
__global__ __launch_bounds__(256) void k_mc_hist(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ rowptr, uint64_t V,
                                                 const double *__restrict__ log_table, int32_t *__restrict__ hval, uint32_t *__restrict__ hmul,
                                                 double *__restrict__ hx, uint32_t *__restrict__ hpos, uint32_t *__restrict__ nd_out,
                                                 unsigned long long *__restrict__ total_out) {
    __shared__ uint32_t s_wave[4];
    __shared__ unsigned long long s_sum[4];
    const uint32_t p = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t lo = rowptr[p], hi = rowptr[p + 1], n = hi - lo;
    const size_t base = (size_t)lo + p;
    const uint32_t zeros = (uint64_t)n < V ? 1u : 0u;
    uint32_t run = zeros;  // slots used so far
    unsigned long long sum = 0ull;
    for (uint32_t t0 = 0; t0 < n; t0 += 256u) {  // uniform trip count
        const uint32_t i = t0 + tid;
        bool head = false;
        uint32_t v = 0;
        if (i < n) {
            v = (uint32_t)keys[lo + i];
            head = i == 0u || (uint32_t)keys[lo + i - 1u] != v;
            sum += v;
        }
        const unsigned long long m = __ballot(head);
        if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < 4u; w++) {
            if (w < wave) before += s_wave[w];
            all += s_wave[w];
        }
        if (head) {
            const size_t k = base + run + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            hval[k] = (int32_t)v;
            hpos[k] = i;
            hx[k] = v < MC_LOG_TABLE ? log_table[v] : log10(1.0 + (double)v);
        }
        run += all;
        __syncthreads();
    }
    sum = wave_sum(sum);
    if (lane == 0u) s_sum[wave] = sum;
    __syncthreads();  // also: every hpos of the row is written
    if (zeros && tid == 0u) hval[base] = 0, hx[base] = 0.0, hmul[base] = (uint32_t)(V - n);
    for (uint32_t k = zeros + tid; k < run; k += 256u) hmul[base + k] = (k + 1u < run ? hpos[base + k + 1u] : n) - hpos[base + k];
    if (tid == 0u) nd_out[p] = run, total_out[p] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

// ---- the fit ---------------------------------------------------------------------------------------------------------------------------
// sums of N doubles over the workgroup in the one order of this file, the same values in every thread
template <uint32_t NW, uint32_t N>
__device__ __forceinline__ void mc_block_sum(double *v, double *s_red) {
#pragma unroll
    for (uint32_t k = 0; k < N; k++) v[k] = wave_sum(v[k]);
    if (NW == 1u) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    __syncthreads();  // s_red of the sum before is read by now
    if (lane == 0u)
        for (uint32_t k = 0; k < N; k++) s_red[k * NW + wave] = v[k];
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < N; k++) {
        double a = s_red[k * NW];
        for (uint32_t w = 1; w < NW; w++) a += s_red[k * NW + w];
        v[k] = a;
    }
}
// the smallest code over the workgroup (NONE32: none)
template <uint32_t NW>
__device__ __forceinline__ uint32_t mc_block_min(uint32_t c, uint32_t *s_min) {
    c = wave_min(c);
    if (NW == 1u) return c;
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) s_min[threadIdx.x >> 6] = c;
    __syncthreads();
    uint32_t a = s_min[0];
    for (uint32_t w = 1; w < NW; w++) a = s_min[w] < a ? s_min[w] : a;
    return a;
}
__device__ __forceinline__ double mc_x_of(uint32_t v, const double *log_table) {
    return v < MC_LOG_TABLE ? log_table[v] : log10(1.0 + (double)v);
}

struct McFitArgs {
    const uint64_t *keys;      // (place << 32 | column) ascending
    const uint32_t *counts;    // the count of every key
    const uint32_t *rowptr;
    const uint32_t *nd;
    const double *hx;
    const uint32_t *hmul;
    const double *log_table;
    const uint32_t *fit_rows;  // the rows this launch fits
    uint64_t V;
    double u[3u * MC_INITS];
    uint32_t first_cell[MC_INITS];
    double *out;               // [row][init][MC_OUT]
    uint32_t *iters;           // [row][init]
};

// The cell-order search of one trial draw: the first cell whose cumulative squared distance to the first centre reaches r.  Entry e
// of the row stands behind gap_e zeros, each d0 away: G_e = S_(e-1) + gap_e d0, S_e = G_e + d_e.  Returns the VALUE of that cell
// (0 for a zero), the last cell's when r is beyond the total.
template <uint32_t NW>
__device__ __forceinline__ uint32_t mc_locate(const McFitArgs &a, uint32_t lo, uint32_t n, double r, double c0, double d0, double mean,
                                              double *s_scan, uint32_t *s_min) {
    constexpr uint32_t WG = 64u * NW;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    double carry = 0.0;
    for (uint32_t t0 = 0; t0 < n; t0 += WG) {  // uniform
        const uint32_t e = t0 + tid;
        double gapd = 0.0, de = 0.0;
        uint32_t gap = 0, v = 0;
        if (e < n) {
            const uint32_t col = (uint32_t)a.keys[lo + e], prev = e ? (uint32_t)a.keys[lo + e - 1u] + 1u : 0u;
            gap = col - prev;
            v = a.counts[lo + e];
            const double xe = mc_x_of(v, a.log_table) - mean;
            de = (xe - c0) * (xe - c0);
            gapd = (double)gap * d0;
        }
        double s = wave_incl_scan(gapd + de, lane);  // inclusive scan: lanes, then the waves before, then the tiles before
        if (NW > 1u) {
            __syncthreads();
            if (lane == 63u) s_scan[wave] = s;
            __syncthreads();
            double before = 0.0;
            for (uint32_t w = 0; w < wave; w++) before += s_scan[w];
            s = before + s;
        }
        s = carry + s;
        uint32_t code = NONE32;
        if (e < n) {
            if (gap && r <= s - de) code = 2u * tid;  // a zero of the gap in front of e
            else if (r <= s) code = 2u * tid + 1u;
        }
        const uint32_t first = mc_block_min<NW>(code, s_min);
        if (first != NONE32) return (first & 1u) ? a.counts[lo + t0 + (first >> 1)] : 0u;
        // the tile's total: the last thread's s
        if (NW > 1u) {
            __syncthreads();
            if (tid == WG - 1u) s_scan[NW] = s;
            __syncthreads();
            carry = s_scan[NW];
        } else {
            carry = __shfl(s, 63);
        }
    }
    const uint32_t last_col = n ? (uint32_t)a.keys[lo + n - 1u] : 0u;
    if (!n || (uint64_t)last_col + 1u < a.V) return 0u;  // a trailing zero (inside the gap, or the clip to the last cell)
    return a.counts[lo + n - 1u];
}

template <uint32_t NW, bool LDS>
__global__ __launch_bounds__(64 * NW) void k_mc_fit(McFitArgs a) {
    constexpr uint32_t WG = 64u * NW;
    extern __shared__ double mc_lds[];  // LDS: x (nd doubles), the multiplicities as doubles (nd)
    __shared__ double s_red[5u * NW + 1u];
    __shared__ double s_scan[NW + 1u];
    __shared__ uint32_t s_min[NW];
    const uint32_t tid = threadIdx.x, p = a.fit_rows[blockIdx.x / MC_INITS], init = blockIdx.x % MC_INITS;
    const uint32_t lo = a.rowptr[p], n_ent = a.rowptr[p + 1] - lo, nd = a.nd[p];
    const size_t base = (size_t)lo + p;
    const double *gx = a.hx + base;
    const uint32_t *gm = a.hmul + base;
    if (LDS) {
        for (uint32_t k = tid; k < nd; k += WG) mc_lds[k] = gx[k], mc_lds[nd + k] = (double)gm[k];
        __syncthreads();
    }
#define MC_X(k) (LDS ? mc_lds[k] : gx[k])
#define MC_M(k) (LDS ? mc_lds[nd + (k)] : (double)gm[k])
    const double n = (double)a.V;
    // the mean, x @ x and the variance of the row
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t k = tid; k < nd; k += WG) {
        const double x = MC_X(k), m = MC_M(k);
        v[0] += m * x, v[1] += (m * x) * x;
    }
    mc_block_sum<NW, 2>(v, s_red);
    const double mean = v[0] / n, xx = v[1];
    v[0] = 0.0;
    for (uint32_t k = tid; k < nd; k += WG) {
        const double d = MC_X(k) - mean;
        v[0] += MC_M(k) * (d * d);
    }
    mc_block_sum<NW, 1>(v, s_red);
    const double tol = MC_KM_TOL * (v[0] / n);
    // ---- k-means++ for two centres, on the centred values ----
    double c0, c1;
    {
        const uint64_t cell = a.first_cell[init];
        const uint64_t at = cr_lower_bound(a.keys + lo, (uint64_t)n_ent, ((uint64_t)p << 32) | cell);
        const uint32_t v0 = at < n_ent && a.keys[lo + at] == (((uint64_t)p << 32) | cell) ? a.counts[lo + at] : 0u;
        c0 = mc_x_of(v0, a.log_table) - mean;
        v[0] = 0.0;
        for (uint32_t k = tid; k < nd; k += WG) {
            const double d = (MC_X(k) - mean) - c0;
            v[0] += MC_M(k) * (d * d);
        }
        mc_block_sum<NW, 1>(v, s_red);
        const double pot = v[0], d0 = (0.0 - mean - c0) * (0.0 - mean - c0);
        const uint32_t va = mc_locate<NW>(a, lo, n_ent, a.u[3u * init + 1u] * pot, c0, d0, mean, s_scan, s_min);
        const uint32_t vb = mc_locate<NW>(a, lo, n_ent, a.u[3u * init + 2u] * pot, c0, d0, mean, s_scan, s_min);
        const double ca = mc_x_of(va, a.log_table) - mean, cb = mc_x_of(vb, a.log_table) - mean;
        v[0] = v[1] = 0.0;
        for (uint32_t k = tid; k < nd; k += WG) {
            const double x = MC_X(k) - mean, m = MC_M(k);
            const double dc = (x - c0) * (x - c0), da = (x - ca) * (x - ca), db = (x - cb) * (x - cb);
            v[0] += m * (da < dc ? da : dc), v[1] += m * (db < dc ? db : dc);
        }
        mc_block_sum<NW, 2>(v, s_red);
        c1 = v[1] < v[0] ? cb : ca;  // the smaller potential, the first on a tie
    }
    // ---- Lloyd: the labels of a round come from the centres before it; (f0, f1) are the centres the final labels come from ----
    double f0 = c0, f1 = c1;
    {
        double p0 = 0.0, p1 = 0.0;  // the centres of the round before
        bool repeat = false;
        for (uint32_t it = 0; it < MC_KM_MAX_ITER; it++) {
            v[0] = v[1] = v[2] = v[3] = v[4] = 0.0;
            for (uint32_t k = tid; k < nd; k += WG) {
                const double x = MC_X(k) - mean, m = MC_M(k);
                const bool l1 = fabs(x - c1) < fabs(x - c0);
                if (l1) v[1] += m, v[3] += m * x; else v[0] += m, v[2] += m * x;
                if (it && l1 != (fabs(x - p1) < fabs(x - p0))) v[4] += 1.0;
            }
            mc_block_sum<NW, 5>(v, s_red);
            const double n0 = v[0] > 0.0 ? v[2] / v[0] : c0, n1 = v[1] > 0.0 ? v[3] / v[1] : c1;  // an empty cluster keeps its centre
            const double shift = (n0 - c0) * (n0 - c0) + (n1 - c1) * (n1 - c1);
            f0 = c0, f1 = c1;
            p0 = c0, p1 = c1;
            c0 = n0, c1 = n1;
            if (it && v[4] == 0.0) {  // the labels repeat: they stand
                repeat = true;
                break;
            }
            if (shift <= tol) break;
        }
        if (!repeat) f0 = c0, f1 = c1;  // one relabel under the last centres (also after 300 rounds)
    }
    // ---- EM on the histogram: the iteration of rpu_gmm.h, weighted by the multiplicities ----
    double w0, w1, mu0, mu1, cov, pc;
    {
        v[0] = v[1] = v[2] = v[3] = 0.0;
        for (uint32_t k = tid; k < nd; k += WG) {
            const double x = MC_X(k), m = MC_M(k), xc = x - mean;
            if (fabs(xc - f1) < fabs(xc - f0)) v[1] += m, v[3] += m * x; else v[0] += m, v[2] += m * x;
        }
        mc_block_sum<NW, 4>(v, s_red);
        const double nk0 = v[0] + MC_EPS10, nk1 = v[1] + MC_EPS10;
        mu0 = v[2] / nk0, mu1 = v[3] / nk1;
        cov = (xx - ((nk0 * mu0) * mu0 + (nk1 * mu1) * mu1)) / (nk0 + nk1) + GMM_REG;
        w0 = nk0 / n, w1 = nk1 / n;  // _initialize: not renormalised
        pc = 1.0 / sqrt(cov);
    }
    double lb = -INFINITY;
    uint32_t it = 0;
    for (it = 1; it <= GMM_MAX_ITER; it++) {
        const double prev = lb;
        const double lp = log(pc), l0 = log(w0), l1 = log(w1);
        v[0] = v[1] = v[2] = v[3] = v[4] = 0.0;
        for (uint32_t k = tid; k < nd; k += WG) {
            const double xi = MC_X(k), m = MC_M(k);
            const double y0 = xi * pc - mu0 * pc, y1 = xi * pc - mu1 * pc;
            const double a0 = -0.5 * (GMM_LOG_2PI + y0 * y0) + lp + l0, a1 = -0.5 * (GMM_LOG_2PI + y1 * y1) + lp + l1;
            const double lpn = gmm_logsumexp(a0, a1);
            const double r0 = m * exp(a0 - lpn), r1 = m * exp(a1 - lpn);
            v[0] += r0, v[1] += r1, v[2] += r0 * xi, v[3] += r1 * xi, v[4] += m * lpn;
        }
        mc_block_sum<NW, 5>(v, s_red);
        const double nk0 = v[0] + MC_EPS10, nk1 = v[1] + MC_EPS10;
        mu0 = v[2] / nk0, mu1 = v[3] / nk1;
        const double nks = nk0 + nk1;
        cov = (xx - ((nk0 * mu0) * mu0 + (nk1 * mu1) * mu1)) / nks + GMM_REG;
        w0 = nk0 / nks, w1 = nk1 / nks;
        const double ws = w0 + w1;
        w0 = w0 / ws, w1 = w1 / ws;
        pc = 1.0 / sqrt(cov);
        lb = v[4] / n;
        if (fabs(lb - prev) < GMM_TOL) break;
    }
    if (it > GMM_MAX_ITER) it = GMM_MAX_ITER;
    if (tid == 0u) {
        double *o = a.out + ((size_t)p * MC_INITS + init) * MC_OUT;
        o[0] = w0, o[1] = w1, o[2] = mu0, o[3] = mu1, o[4] = cov, o[5] = lb;
        a.iters[(size_t)p * MC_INITS + init] = it;
    }
#undef MC_X
#undef MC_M
}

// ---- predict and assign ----------------------------------------------------------------------------------------------------------------
struct McRowDev {  // what k_mc_assign leaves per row
    double w[2], mu[2], cov, lb;
    uint32_t winner, n_iter, assigned, min_count;  // min_count NONE32: no cell assigned
};

// A workgroup per fitted row.  hpos[slot] = 1 where the distinct value is predicted into the positive component AND meets the
// threshold: what an entry (and k_mc_cells) looks up.
__global__ __launch_bounds__(256) void k_mc_assign(const uint32_t *__restrict__ fit_rows, const uint32_t *__restrict__ rowptr,
                                                   const uint32_t *__restrict__ nd_arr, const double *__restrict__ hx,
                                                   const int32_t *__restrict__ hval, const uint32_t *__restrict__ hmul, uint32_t *__restrict__ hpos,
                                                   const double *__restrict__ fit_out, const uint32_t *__restrict__ iters, uint32_t umi_threshold,
                                                   McRowDev *__restrict__ rows) {
    __shared__ uint32_t s_cnt[4], s_mn[4];
    const uint32_t p = fit_rows[blockIdx.x], tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const size_t base = (size_t)rowptr[p] + p;
    const uint32_t nd = nd_arr[p];
    uint32_t win = 0;
    double best = -INFINITY;
    for (uint32_t j = 0; j < MC_INITS; j++) {  // uniform: every thread reads the same ten numbers
        const double lb = fit_out[((size_t)p * MC_INITS + j) * MC_OUT + 5u];
        if (j == 0u || lb > best) best = lb, win = j;  // the first init always, a later one with a strictly larger bound
    }
    const double *o = fit_out + ((size_t)p * MC_INITS + win) * MC_OUT;
    const double w0 = o[0], w1 = o[1], mu0 = o[2], mu1 = o[3], cov = o[4];
    const double pc = 1.0 / sqrt(cov), lp = log(pc), l0 = log(w0), l1 = log(w1);
    const uint32_t pos = mu1 > mu0 ? 1u : 0u;  // np.argmax: the first of equal means
    uint32_t cnt = 0, mn = NONE32;
    for (uint32_t k = tid; k < nd; k += 256u) {
        const double xi = hx[base + k];
        const double y0 = xi * pc - mu0 * pc, y1 = xi * pc - mu1 * pc;
        const double a0 = -0.5 * (GMM_LOG_2PI + y0 * y0) + lp + l0, a1 = -0.5 * (GMM_LOG_2PI + y1 * y1) + lp + l1;
        const uint32_t pred = a1 > a0 ? 1u : 0u;  // argmax: a tie goes to component 0
        const uint32_t v = (uint32_t)hval[base + k];
        const bool on = pred == pos && v >= umi_threshold;  // umi_threshold >= 1: the zeros are never assigned
        hpos[base + k] = on ? 1u : 0u;
        if (on) cnt += hmul[base + k], mn = v < mn ? v : mn;
    }
    cnt = wave_sum(cnt), mn = wave_min(mn);
    if (lane == 0u) s_cnt[wave] = cnt, s_mn[wave] = mn;
    __syncthreads();
    if (tid == 0u) {
        McRowDev r;
        r.w[0] = w0, r.w[1] = w1, r.mu[0] = mu0, r.mu[1] = mu1, r.cov = cov, r.lb = best;
        r.winner = win, r.n_iter = iters[(size_t)p * MC_INITS + win];
        r.assigned = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        r.min_count = min(min(s_mn[0], s_mn[1]), min(s_mn[2], s_mn[3]));
        rows[p] = r;
    }
}

// the slot of count v among the row's distinct values (it is there)
__device__ __forceinline__ uint32_t mc_slot_of(const int32_t *hval, uint32_t nd, int32_t v) {
    const uint32_t k = cr_lower_bound(hval, nd, v);
    return k < nd ? k : nd - 1u;
}

// A workgroup per fitted row: its assigned columns, ascending, at out_ptr[p]
__global__ __launch_bounds__(256) void k_mc_emit(const uint32_t *__restrict__ fit_rows, const uint64_t *__restrict__ keys,
                                                 const uint32_t *__restrict__ counts, const uint32_t *__restrict__ rowptr,
                                                 const uint32_t *__restrict__ nd_arr, const int32_t *__restrict__ hval,
                                                 const uint32_t *__restrict__ hpos, const long long *__restrict__ out_ptr,
                                                 uint32_t *__restrict__ out_cols) {
    __shared__ uint32_t s_wave[4];
    const uint32_t p = fit_rows[blockIdx.x], tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t lo = rowptr[p], n = rowptr[p + 1] - lo, nd = nd_arr[p];
    const size_t base = (size_t)lo + p;
    const long long end = out_ptr[p + 1];
    long long run = out_ptr[p];
    for (uint32_t t0 = 0; t0 < n; t0 += 256u) {  // uniform
        const uint32_t e = t0 + tid;
        bool on = false;
        if (e < n) on = hpos[base + mc_slot_of(hval + base, nd, (int32_t)counts[lo + e])] != 0u;
        const unsigned long long m = __ballot(on);
        if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < 4u; w++) {
            if (w < wave) before += s_wave[w];
            all += s_wave[w];
        }
        const long long at = run + before + (long long)__popcll(m & ((1ull << lane) - 1ull));
        if (on && at < end) out_cols[at] = (uint32_t)keys[lo + e];
        run += all;
        __syncthreads();
    }
}

// A thread per column: the number of listed rows assigned to it, and the tallies tally[0 .. 4): cells with 0 / 1 / > 1 assigned
// features, cells without a UMI in any listed row
__global__ __launch_bounds__(256) void k_mc_cells(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                  const int32_t *__restrict__ data, uint64_t V, const uint32_t *__restrict__ place,
                                                  const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ nd_arr,
                                                  const uint8_t *__restrict__ fitted, const int32_t *__restrict__ hval,
                                                  const uint32_t *__restrict__ hpos, uint32_t *__restrict__ fpc,
                                                  unsigned long long *__restrict__ tally) {
    __shared__ uint32_t s_t[4][4];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t t[4] = {0u, 0u, 0u, 0u};
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < V; c += stride) {
        uint32_t n = 0, umis = 0;
        for (long long e = indptr[c]; e < indptr[c + 1]; e++) {
            const uint32_t pl = place[(uint32_t)indices[e]];
            if (!pl) continue;
            const uint32_t p = pl - 1u;
            umis = 1u;
            if (!fitted[p]) continue;
            const size_t base = (size_t)rowptr[p] + p;
            n += hpos[base + mc_slot_of(hval + base, nd_arr[p], data[e])] != 0u;
        }
        fpc[c] = n;
        t[n > 2u ? 2u : n]++;
        t[3] += umis ? 0u : 1u;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        t[k] = wave_sum(t[k]);
        if (lane == 0u) s_t[k][wave] = t[k];
    }
    __syncthreads();
    if (threadIdx.x < 4u) {  // one integer atomic per workgroup and tally: the sum does not depend on the order
        const uint32_t k = threadIdx.x;
        atomicAdd(tally + k, (unsigned long long)(s_t[k][0] + s_t[k][1] + s_t[k][2] + s_t[k][3]));
    }
}

extern "C" void crgpu_marginal_calls_free(crgpu_ctx *ctx, crgpu_marginal_calls *r) {
    if (!r) return;
    crgpu_marginal_calls_impl *im = (crgpu_marginal_calls_impl *)r;
    if (ctx) {
        CR_ENTER(ctx);
        for (void *p : {im->d_indptr, im->d_columns, im->d_fpc, im->d_hoff, im->d_hval, im->d_hmul})
            if (p) cr_pool_free(ctx, p);
    }
    delete im;
}

static int mc_run(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint32_t *feature_rows, uint32_t n_rows, uint32_t n_features, uint32_t umi_threshold,
                  bool want_hist, crgpu_marginal_calls_impl *im) {
    const uint64_t V = m->n_barcodes;
    CR_REQUIRE(ctx, V < 0x7FFFFFFFull, CRGPU_ERANGE, "crgpu_marginal_calls_dev: %llu barcodes, at most 2^31 - 2", (unsigned long long)V);
    im->rows.assign(n_rows, crgpu_marginal_row{});
    for (auto &r : im->rows) r.umi_threshold_observed = -1, r.winner = NONE32;
    im->view.n_rows = n_rows, im->view.n_barcodes = V;
    const auto clk = [] { return std::chrono::steady_clock::now(); };
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL;
    // ---- extraction ----
    auto t0 = clk();
    DevBuf rows_b, place_b, cnt_b;
    std::vector<uint64_t> rows64(feature_rows, feature_rows + n_rows);
    CR_TRY(dmalloc(ctx, rows_b, (uint64_t)n_rows * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, place_b, (uint64_t)n_features * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, cnt_b, (V + 1) * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, rows_b.p, rows64.data(), (uint64_t)n_rows * sizeof(uint64_t)));
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(place_b.p, 0, (uint64_t)n_features * sizeof(uint32_t), ctx->stream));
    cr_check_columns<true>(ctx, rows_b.as<uint64_t>(), n_rows, n_features, MarkPlace{place_b.as<uint32_t>()}, d_flag);
    uint32_t n_ent = 0;
    if (V) {
        CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
        hipLaunchKernelGGL(k_mc_count, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, V,
                           place_b.as<uint32_t>(), n_features, cnt_b.as<uint32_t>(), d_flag);
        CR_HIP(ctx, hipGetLastError());
        CR_TRY(cr_scan_small(ctx, cnt_b.as<uint32_t>(), V, d_total));
        CR_TRY(read_u32(ctx, d_total, &n_ent));
    }
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_TRY(cr_list_verdict(ctx, flag, "crgpu_marginal_calls_dev", "feature row"));
    CR_REQUIRE(ctx, !(flag & 4u), CRGPU_EINVAL, "crgpu_marginal_calls_dev: the matrix holds a row >= n_features (%u)", n_features);
    CR_REQUIRE(ctx, (uint64_t)n_ent + n_rows + 1u < 0xFFFFFFFFull, CRGPU_ERANGE, "crgpu_marginal_calls_dev: too many entries in the listed rows");
    const uint64_t n_slots = (uint64_t)n_ent + n_rows;  // histogram slots: a row's entries + 1
    DevBuf kc_b, kct_b, kv_b, kvt_b, val_b, valt_b, rp_b, nd_b, tot_b, hx_b, hval_b, hmul_b, hpos_b, tab_b;
    CR_TRY(dmalloc(ctx, kc_b, std::max<uint64_t>(n_ent, 1) * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, kct_b, std::max<uint64_t>(n_ent, 1) * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, kv_b, std::max<uint64_t>(n_ent, 1) * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, kvt_b, std::max<uint64_t>(n_ent, 1) * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, val_b, std::max<uint64_t>(n_ent, 1) * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, valt_b, std::max<uint64_t>(n_ent, 1) * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, rp_b, ((uint64_t)n_rows + 1) * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, nd_b, (uint64_t)n_rows * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, tot_b, (uint64_t)n_rows * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, hx_b, n_slots * sizeof(double)));
    CR_TRY(dmalloc(ctx, hval_b, n_slots * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, hmul_b, n_slots * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, hpos_b, n_slots * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, tab_b, (uint64_t)MC_LOG_TABLE * sizeof(double)));
    const uint64_t *keys_col = kc_b.as<uint64_t>(), *keys_cnt = kv_b.as<uint64_t>();
    const uint32_t *counts = val_b.as<uint32_t>();
    if (n_ent) {
        CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
        {
            CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
            hipLaunchKernelGGL(k_mc_scatter, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data, V,
                               place_b.as<uint32_t>(), n_features, cnt_b.as<uint32_t>(), (uint64_t)n_ent, kc_b.as<uint64_t>(), val_b.as<uint32_t>(),
                               kv_b.as<uint64_t>(), d_flag);
            CR_HIP(ctx, hipGetLastError());
        }
        CR_TRY(read_u32(ctx, d_flag, &flag));
        CR_REQUIRE(ctx, !(flag & 8u), CRGPU_EINVAL, "crgpu_marginal_calls_dev: a listed row holds a stored count <= 0");
        const uint32_t row_bits = std::max(cr_ceil_log2(n_rows), 1u);
        bool in_tmp = false;
        CR_TRY(cr_radix_sort_u64(ctx, kc_b.as<uint64_t>(), kct_b.as<uint64_t>(), val_b.as<uint32_t>(), valt_b.as<uint32_t>(), n_ent, 0, 32u + row_bits, &in_tmp));
        if (in_tmp) keys_col = kct_b.as<uint64_t>(), counts = valt_b.as<uint32_t>();
        in_tmp = false;
        CR_TRY(cr_radix_sort_u64(ctx, kv_b.as<uint64_t>(), kvt_b.as<uint64_t>(), nullptr, nullptr, n_ent, 0, 32u + row_bits, &in_tmp));
        if (in_tmp) keys_cnt = kvt_b.as<uint64_t>();
    }
    hipLaunchKernelGGL(k_mc_rowptr, dim3((n_rows + 256u) / 256u), dim3(256), 0, ctx->stream, keys_col, (uint64_t)n_ent, n_rows, rp_b.as<uint32_t>());
    CR_HIP(ctx, hipGetLastError());
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    im->view.ms_extract = cr_ms_since(t0);
    // ---- histograms ----
    t0 = clk();
    {
        static const std::vector<double> tab = [] {  // made once: 65 536 logarithms cost a millisecond
            std::vector<double> t(MC_LOG_TABLE);
            for (uint32_t v = 0; v < MC_LOG_TABLE; v++) t[v] = std::log10(1.0 + (double)v);
            return t;
        }();
        CR_TRY(crgpu_memcpy_h2d(ctx, tab_b.p, tab.data(), tab.size() * sizeof(double)));
    }
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, n_ent);
        hipLaunchKernelGGL(k_mc_hist, dim3(n_rows), dim3(256), 0, ctx->stream, keys_cnt, rp_b.as<uint32_t>(), V, tab_b.as<double>(), hval_b.as<int32_t>(),
                           hmul_b.as<uint32_t>(), hx_b.as<double>(), hpos_b.as<uint32_t>(), nd_b.as<uint32_t>(), tot_b.as<unsigned long long>());
        CR_HIP(ctx, hipGetLastError());
    }
    std::vector<uint32_t> rowptr(n_rows + 1u), nd(n_rows);
    std::vector<uint64_t> total(n_rows);
    CR_TRY(crgpu_memcpy_d2h(ctx, rowptr.data(), rp_b.p, rowptr.size() * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, nd.data(), nd_b.p, nd.size() * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, total.data(), tot_b.p, total.size() * sizeof(uint64_t)));
    im->view.ms_histogram = cr_ms_since(t0);
    // ---- the fit: the rows in four classes (one wave or four, LDS or device memory) ----
    t0 = clk();
    std::vector<uint32_t> cls[4], fit_rows;
    std::vector<uint8_t> fitted(n_rows, 0);
    for (uint32_t p = 0; p < n_rows; p++) {
        im->rows[p].total_umis = total[p], im->rows[p].n_distinct = nd[p];
        CR_REQUIRE(ctx, rowptr[p] <= rowptr[p + 1] && rowptr[p + 1] <= n_ent && nd[p] <= rowptr[p + 1] - rowptr[p] + 1u, CRGPU_EHIP,
                   "crgpu_marginal_calls_dev: row %u has an impossible extent", p);
        if (rowptr[p + 1] == rowptr[p] || V < 2) continue;  // np.max == 0, or fewer than two cells: SKIPPED
        const bool lds = nd[p] <= ctx->mc_lds_values && (uint64_t)nd[p] * 16u <= 96u * 1024u;
        const bool wide = nd[p] > MC_WAVE_VALUES || rowptr[p + 1] - rowptr[p] > MC_WAVE_ENTRIES;
        cls[(wide ? 2u : 0u) + (lds ? 0u : 1u)].push_back(p);
        fitted[p] = 1u, fit_rows.push_back(p);
        im->rows[p].status = CRGPU_MC_FITTED, im->rows[p].in_lds = lds ? 1u : 0u;
    }
    DevBuf out_b, it_b, fr_b, rowdev_b, fitted_b, tally_b, fpc_b;
    CR_TRY(dmalloc(ctx, out_b, (uint64_t)n_rows * MC_INITS * MC_OUT * sizeof(double)));
    CR_TRY(dmalloc(ctx, it_b, (uint64_t)n_rows * MC_INITS * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, fr_b, std::max<uint64_t>(fit_rows.size(), 1) * 2u * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, rowdev_b, (uint64_t)n_rows * sizeof(McRowDev)));
    CR_TRY(dmalloc(ctx, fitted_b, n_rows));
    CR_TRY(dmalloc(ctx, tally_b, 4u * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, fitted_b.p, fitted.data(), n_rows));
    McFitArgs fa;
    fa.keys = keys_col, fa.counts = counts, fa.rowptr = rp_b.as<uint32_t>(), fa.nd = nd_b.as<uint32_t>(), fa.hx = hx_b.as<double>();
    fa.hmul = hmul_b.as<uint32_t>(), fa.log_table = tab_b.as<double>(), fa.V = V, fa.out = out_b.as<double>(), fa.iters = it_b.as<uint32_t>();
    if (!fit_rows.empty()) {
        uint64_t fc[MC_INITS];
        mc_seed_draws(V, fa.u, fc);
        for (uint32_t j = 0; j < MC_INITS; j++) fa.first_cell[j] = (uint32_t)fc[j];
        std::vector<uint32_t> order;  // the classes one after the other, then the whole list for the assign kernels
        for (auto &c : cls) order.insert(order.end(), c.begin(), c.end());
        order.insert(order.end(), fit_rows.begin(), fit_rows.end());
        CR_TRY(crgpu_memcpy_h2d(ctx, fr_b.p, order.data(), order.size() * sizeof(uint32_t)));
        CrTimer t(ctx, CRGPU_T_MATRIX, (uint64_t)fit_rows.size() * MC_INITS);
        uint32_t at = 0;
        for (uint32_t c = 0; c < 4u; c++) {
            const uint32_t nc = (uint32_t)cls[c].size();
            if (!nc) continue;
            fa.fit_rows = fr_b.as<uint32_t>() + at;
            at += nc;
            uint32_t nd_max = 0;
            for (uint32_t p : cls[c]) nd_max = std::max(nd_max, nd[p]);
            const size_t dyn = (size_t)nd_max * 2u * sizeof(double);
            switch (c) {
            case 0:
                cr_allow_lds(ctx, (const void *)k_mc_fit<1, true>, dyn);
                hipLaunchKernelGGL((k_mc_fit<1, true>), dim3(nc * MC_INITS), dim3(64), dyn, ctx->stream, fa);
                break;
            case 1: hipLaunchKernelGGL((k_mc_fit<1, false>), dim3(nc * MC_INITS), dim3(64), 0, ctx->stream, fa); break;
            case 2:
                cr_allow_lds(ctx, (const void *)k_mc_fit<4, true>, dyn);
                hipLaunchKernelGGL((k_mc_fit<4, true>), dim3(nc * MC_INITS), dim3(256), dyn, ctx->stream, fa);
                break;
            default: hipLaunchKernelGGL((k_mc_fit<4, false>), dim3(nc * MC_INITS), dim3(256), 0, ctx->stream, fa); break;
            }
            CR_HIP(ctx, hipGetLastError());
        }
    }
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    im->view.ms_fit = cr_ms_since(t0);
    // ---- predict and assign ----
    t0 = clk();
    const uint32_t n_fit = (uint32_t)fit_rows.size();
    const uint32_t *d_fit_rows = fr_b.as<uint32_t>() + n_fit;
    std::vector<long long> out_ptr(n_rows + 1u, 0);
    if (n_fit) {
        hipLaunchKernelGGL(k_mc_assign, dim3(n_fit), dim3(256), 0, ctx->stream, d_fit_rows, rp_b.as<uint32_t>(), nd_b.as<uint32_t>(), hx_b.as<double>(),
                           hval_b.as<int32_t>(), hmul_b.as<uint32_t>(), hpos_b.as<uint32_t>(), out_b.as<double>(), it_b.as<uint32_t>(), umi_threshold,
                           rowdev_b.as<McRowDev>());
        CR_HIP(ctx, hipGetLastError());
        std::vector<McRowDev> rd(n_rows);
        CR_TRY(crgpu_memcpy_d2h(ctx, rd.data(), rowdev_b.p, (uint64_t)n_rows * sizeof(McRowDev)));
        for (uint32_t p : fit_rows) {
            crgpu_marginal_row &r = im->rows[p];
            const McRowDev &d = rd[p];
            const uint32_t hi = d.mu[1] > d.mu[0] ? 1u : 0u, lo = 1u - hi;
            r.mean_low = d.mu[lo], r.mean_high = d.mu[hi], r.weight_low = d.w[lo], r.weight_high = d.w[hi];
            r.covariance = d.cov, r.lower_bound = d.lb, r.winner = d.winner, r.n_iter = d.n_iter;
            CR_REQUIRE(ctx, d.assigned <= rowptr[p + 1] - rowptr[p], CRGPU_EHIP, "crgpu_marginal_calls_dev: row %u assigns more cells than it has entries", p);
            r.cells_assigned = d.assigned;
            r.umi_threshold_observed = d.min_count == NONE32 ? -1 : (int64_t)d.min_count;
        }
    }
    for (uint32_t p = 0; p < n_rows; p++) out_ptr[p + 1] = out_ptr[p] + (long long)im->rows[p].cells_assigned;
    const uint64_t n_asg = (uint64_t)out_ptr[n_rows];
    im->view.n_assigned = n_asg;
    CR_TRY(cr_pool_alloc(ctx, &im->d_indptr, ((uint64_t)n_rows + 1) * sizeof(long long)));
    CR_TRY(cr_pool_alloc(ctx, &im->d_columns, std::max<uint64_t>(n_asg, 1) * sizeof(uint32_t)));
    CR_TRY(cr_pool_alloc(ctx, &im->d_fpc, std::max<uint64_t>(V, 1) * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, im->d_indptr, out_ptr.data(), out_ptr.size() * sizeof(long long)));
    CR_HIP(ctx, hipMemsetAsync(tally_b.p, 0, 4u * sizeof(uint64_t), ctx->stream));
    if (n_fit && n_asg) {
        hipLaunchKernelGGL(k_mc_emit, dim3(n_fit), dim3(256), 0, ctx->stream, d_fit_rows, keys_col, counts, rp_b.as<uint32_t>(), nd_b.as<uint32_t>(),
                           hval_b.as<int32_t>(), hpos_b.as<uint32_t>(), (const long long *)im->d_indptr, (uint32_t *)im->d_columns);
        CR_HIP(ctx, hipGetLastError());
    }
    if (V) {
        CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
        hipLaunchKernelGGL(k_mc_cells, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data, V,
                           place_b.as<uint32_t>(), rp_b.as<uint32_t>(), nd_b.as<uint32_t>(), fitted_b.as<uint8_t>(), hval_b.as<int32_t>(),
                           hpos_b.as<uint32_t>(), (uint32_t *)im->d_fpc, tally_b.as<unsigned long long>());
        CR_HIP(ctx, hipGetLastError());
    }
    uint64_t tally[4];
    CR_TRY(crgpu_memcpy_d2h(ctx, tally, tally_b.p, sizeof(tally)));
    im->view.cells_with_0 = tally[0], im->view.cells_with_1 = tally[1], im->view.cells_with_many = tally[2], im->view.cells_without_umis = tally[3];
    if (want_hist) {
        std::vector<long long> hoff(n_rows + 1u);
        for (uint32_t p = 0; p <= n_rows; p++) hoff[p] = (long long)rowptr[p] + p;
        CR_TRY(cr_pool_alloc(ctx, &im->d_hoff, hoff.size() * sizeof(long long)));
        CR_TRY(cr_pool_alloc(ctx, &im->d_hval, std::max<uint64_t>(n_slots, 1) * sizeof(int32_t)));
        CR_TRY(cr_pool_alloc(ctx, &im->d_hmul, std::max<uint64_t>(n_slots, 1) * sizeof(uint32_t)));
        CR_TRY(crgpu_memcpy_h2d(ctx, im->d_hoff, hoff.data(), hoff.size() * sizeof(long long)));
        CR_HIP(ctx, hipMemcpyAsync(im->d_hval, hval_b.p, n_slots * sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
        CR_HIP(ctx, hipMemcpyAsync(im->d_hmul, hmul_b.p, n_slots * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
        im->view.n_hist_slots = n_slots;
    }
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    im->view.ms_assign = cr_ms_since(t0);
    im->view.rows = im->rows.data();
    im->view.d_indptr = (const int64_t *)im->d_indptr, im->view.d_columns = (const uint32_t *)im->d_columns;
    im->view.d_features_per_cell = (const uint32_t *)im->d_fpc;
    im->view.d_hist_offsets = (const int64_t *)im->d_hoff, im->view.d_hist_values = (const int32_t *)im->d_hval;
    im->view.d_hist_counts = (const uint32_t *)im->d_hmul;
    return CRGPU_OK;
}

extern "C" int crgpu_marginal_calls_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint32_t *feature_rows, uint32_t n_rows, uint32_t n_features,
                                        uint32_t umi_threshold, uint32_t want_histograms, crgpu_marginal_calls **out) {
    if (!ctx || !m || !out) return CRGPU_EINVAL;
    *out = nullptr;
    crgpu_marginal_calls_impl *im = nullptr;
    int rc;
    {
        CR_ENTER(ctx);
        CR_REQUIRE(ctx, feature_rows && n_rows && n_features, CRGPU_EINVAL, "crgpu_marginal_calls_dev: no feature rows or no features");
        CR_REQUIRE(ctx, umi_threshold >= 1u, CRGPU_EINVAL, "crgpu_marginal_calls_dev: umi_threshold must be at least 1");
        im = new crgpu_marginal_calls_impl();
        memset(&im->view, 0, sizeof(im->view));
        rc = mc_run(ctx, m, feature_rows, n_rows, n_features, umi_threshold, want_histograms != 0u, im);
    }
    if (rc != CRGPU_OK) {
        crgpu_marginal_calls_free(ctx, &im->view);
        return rc;
    }
    *out = &im->view;
    return CRGPU_OK;
}

// ---- the tag moments and the contaminant rule ----------------------------------------------------------------------------------------
// A thread per column walks its tag entries pairwise; the sums are integers, so their order does not matter: LDS atomics per
// workgroup, then one global atomic per workgroup and sum.  mom[0 .. 16): sum x; mom[16 + 16 i + j), i <= j: sum x_i x_j.
__global__ __launch_bounds__(256) void k_mc_moments(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    const int32_t *__restrict__ data, uint64_t V, const uint32_t *__restrict__ place,
                                                    uint32_t n_features, unsigned long long *__restrict__ mom) {
    __shared__ unsigned long long s_m[JB_MAXK + JB_MAXK * JB_MAXK];
    for (uint32_t i = threadIdx.x; i < JB_MAXK + JB_MAXK * JB_MAXK; i += 256u) s_m[i] = 0ull;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < V; c += stride) {
        const long long e1 = indptr[c + 1];
        for (long long e = indptr[c]; e < e1; e++) {
            const uint32_t f = (uint32_t)indices[e];
            const uint32_t p = f < n_features ? place[f] : 0u;
            if (!p) continue;
            const unsigned long long d = (unsigned long long)(uint32_t)data[e];
            atomicAdd(&s_m[p - 1u], d);
            for (long long g = e; g < e1; g++) {  // rows ascend inside a column and the list ascends: q >= p
                const uint32_t f2 = (uint32_t)indices[g];
                const uint32_t q = f2 < n_features ? place[f2] : 0u;
                if (q) atomicAdd(&s_m[JB_MAXK + (p - 1u) * JB_MAXK + (q - 1u)], d * (unsigned long long)(uint32_t)data[g]);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < JB_MAXK + JB_MAXK * JB_MAXK; i += 256u)
        if (s_m[i]) atomicAdd(mom + i, s_m[i]);
}

extern "C" int crgpu_tag_moments_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint32_t *tag_rows, uint32_t n_rows, uint32_t n_features,
                                     uint64_t *sum_x_out, uint64_t *sum_xx_out, uint64_t *sum_xy_out) {
    if (!ctx || !m) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, tag_rows && n_rows && n_features && sum_x_out && sum_xx_out && sum_xy_out, CRGPU_EINVAL, "crgpu_tag_moments_dev: no tag rows, no features or a NULL output");
    CR_REQUIRE(ctx, n_rows <= JB_MAXK, CRGPU_ERANGE, "crgpu_tag_moments_dev: %u tags, at most %u", n_rows, JB_MAXK);
    const uint64_t V = m->n_barcodes;
    constexpr uint32_t NM = JB_MAXK + JB_MAXK * JB_MAXK;
    DevBuf rows_b, place_b, mom_b;
    std::vector<uint64_t> rows64(tag_rows, tag_rows + n_rows);
    CR_TRY(dmalloc(ctx, rows_b, (uint64_t)n_rows * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, place_b, (uint64_t)n_features * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, mom_b, NM * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, rows_b.p, rows64.data(), (uint64_t)n_rows * sizeof(uint64_t)));
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(place_b.p, 0, (uint64_t)n_features * sizeof(uint32_t), ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(mom_b.p, 0, NM * sizeof(uint64_t), ctx->stream));
    cr_check_columns<true>(ctx, rows_b.as<uint64_t>(), n_rows, n_features, MarkPlace{place_b.as<uint32_t>()}, d_flag);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_flag, &flag));  // before the walk: a list out of range marked nothing
    CR_TRY(cr_list_verdict(ctx, flag, "crgpu_tag_moments_dev", "tag row"));
    if (V) {
        CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
        hipLaunchKernelGGL(k_mc_moments, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data, V,
                           place_b.as<uint32_t>(), n_features, mom_b.as<unsigned long long>());
        CR_HIP(ctx, hipGetLastError());
    }
    uint64_t mom[NM];
    CR_TRY(crgpu_memcpy_d2h(ctx, mom, mom_b.p, sizeof(mom)));
    for (uint32_t i = 0; i < n_rows; i++) {
        sum_x_out[i] = mom[i], sum_xx_out[i] = mom[JB_MAXK + i * JB_MAXK + i];
        for (uint32_t j = i; j < n_rows; j++) sum_xy_out[i * n_rows + j] = sum_xy_out[j * n_rows + i] = mom[JB_MAXK + i * JB_MAXK + j];
    }
    return CRGPU_OK;
}

// Pearson's r from the integer sums; the two factors under the root and the numerator are exact in 128-bit integers
static double mc_pearson(uint64_t n, uint64_t sx, uint64_t sy, uint64_t sxx, uint64_t syy, uint64_t sxy) {
    const __int128 vx = (__int128)n * sxx - (__int128)sx * sx, vy = (__int128)n * syy - (__int128)sy * sy;
    const __int128 cxy = (__int128)n * sxy - (__int128)sx * sy;
    if (vx <= 0 || vy <= 0) return std::nan("");
    return (double)((long double)cxy / (sqrtl((long double)vx) * sqrtl((long double)vy)));
}

extern "C" int crgpu_tag_contaminants(uint32_t n_tags, uint64_t n_cells, const uint64_t *sum_x, const uint64_t *sum_xx, const uint64_t *sum_xy,
                                      const uint32_t *order, uint64_t min_counts, double dynamic_range, double max_cor, uint8_t *flags_out,
                                      int32_t *sources_out) {
    if (!n_tags || !sum_x || !sum_xx || !sum_xy || !order || !flags_out || !sources_out) return CRGPU_EINVAL;
    if (n_tags > JB_MAXK) return CRGPU_ERANGE;
    uint32_t seen = 0;
    for (uint32_t i = 0; i < n_tags; i++) {
        if (order[i] >= n_tags || (seen >> order[i] & 1u)) return CRGPU_EINVAL;  // not a permutation
        seen |= 1u << order[i];
    }
    uint64_t max_count = 0;
    for (uint32_t t = 0; t < n_tags; t++) max_count = std::max(max_count, sum_x[t]);
    uint32_t n_src[JB_MAXK] = {0};
    for (uint32_t i = 0; i < n_tags * n_tags; i++) sources_out[i] = -1;
    for (uint32_t t = 0; t < n_tags; t++) {
        const uint64_t c = sum_x[t];
        flags_out[t] = c == 0 ? 2u : (c < min_counts || (double)c * dynamic_range < (double)max_count) ? 1u : 0u;
    }
    for (uint32_t a = 0; a + 1 < n_tags; a++) {
        const uint32_t i = order[a];
        if (flags_out[i] == 2u) continue;
        for (uint32_t b = a + 1; b < n_tags; b++) {
            const uint32_t j = order[b];
            if (flags_out[j] == 2u) continue;
            const double r = mc_pearson(n_cells, sum_x[i], sum_x[j], sum_xx[i], sum_xx[j], sum_xy[i * n_tags + j]);
            if (std::isnan(r) || r < max_cor) continue;
            const uint32_t loser = sum_x[i] < sum_x[j] ? i : j, other = loser == i ? j : i;
            flags_out[loser] = 1u;
            sources_out[loser * n_tags + n_src[loser]++] = (int32_t)other;
        }
    }
    return CRGPU_OK;
}
