// jibes.h -- the tag caller of a cell-multiplexed (CMO) well: CALL_TAGS_JIBES on the device (part of matrix_stages.hip).
//
// Replaces cellranger.feature.jibes_tag_assigner over the EM fit of lib/rust/jibes_o3/src/lib.rs (the Rust is what runs in
// production; lib/python/cellranger/analysis/jibes_py.py is its original).  QUIRKS kept:
//   * with k <= max_k_lets and a limited model the last k-let probability is an empty sum: its states have a prior of -inf and a
//     posterior of exactly 0 (exp(-inf) = 0; nothing on the way multiplies an infinity by zero);
//   * the stop comparisons are strict and never taken against the initial -inf; rep > max_reps is looked at first;
//   * the slope clamp at 0.01 re-estimates the intercept; the residual variance is over elem_11, under the OLD posterior and the
//     NEW coefficients; the sd floor is 1e-4.
// Beyond the reference: it has 14 Poisson counts (NUM_TOTAL_TAGS), so with 15 or 16 tags and a limited model its unit-vector
// state indexes past them; here the counts run to max(14, k).
//
// Launch structure.  A state is 2 bits per tag in one word; the words, the prior and one row of states per wave sit in LDS.  A
// workgroup of four waves takes one chunk of JB_CHUNK barcodes, wave w the barcodes w, w + 4, ... of it.  Per barcode the k x 4
// distinct log densities are computed once (lane 4 t + c: tag t, count c); a lane then adds them to the prior in TAG order for its
// states lane, lane + 64, ...: the reference's own sequence of additions.  The row never reaches device memory.
//   k_jb_pass<KP, 0>   posterior under the current model; the sums of the M step and of LL
//   k_jb_close_a       adds the chunks, LL, the stop rule and its latch, the new coefficients
//   k_jb_pass<KP, 1>   the same posterior again (bit for bit), the residual sums under the new coefficients
//   k_jb_close_b       the new sd; the model of the next round
//   k_jb_pass<KP, 2>   after the stop: the per-barcode outputs
// KP = k rounded up to 2, 4, 8, 12 or 16: the loops over the tags unroll and a lane's sums stay in registers; a tag beyond k adds
// +0.0 to a state's log posterior, which changes no bit.  Every cross-barcode sum is reduced in ONE order that depends on (n, z,
// k) alone: a lane over its (barcode, state) pairs in ascending order, the xor butterfly, the four waves ascending, then the
// chunks ascending out of a slab of plain stores (k_jb_close_*, which bring the slab through LDS a tile at a time and add from
// there): no floating-point atomic, nothing depends on the grid (a chunk IS a workgroup) or on the run.  tag_cnt * row.sum() and
// elem_11 take the whole row's sum, as the reference does (one more butterfly per barcode): with per-lane partial rows the n = 1
// fixture, whose residual cancels to 0.005 of y, was 4e-14 off in sd; now it is equal bit for bit.
// No kernel waits for another workgroup.  The host does not synchronise per iteration:
// k_jb_close_a latches "stopped at round r" with the model and LL of that round, every later launch returns at once, and the
// host reads the latch after each batch of ctx->jibes_batch rounds (CRGPU_JIBES_BATCH).  f64 throughout, unfused.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "stage_common.h"

#define JB_WG 256u
#define JB_WAVES 4u
#define JB_CHUNK 64u
#define JB_MAXK CRGPU_JIBES_MAX_TAGS
#define JB_NSTAT_A (3u + 4u * JB_MAXK)  // sum ln(marginal), sum max, elem_11, then per tag first, second, elem_12, elem_22
#define JB_NSTAT_B JB_MAXK              // per tag the residual sum
#define JB_CLOSE_ROWS_A 32u             // chunks a closing kernel brings through LDS at a time
#define JB_CLOSE_ROWS_B 128u
#define JB_LN_SQRT_2PI 0.91893853320467274178
#define JB_CORR_FACTOR 1.54
#define JB_NUM_TOTAL_TAGS 14u
#define JB_MIN_FOREGROUND_DELTA 0.01
#define JB_SD_FLOOR 0.0001

struct JbState {
    double bg[JB_MAXK], fg[JB_MAXK], sd[JB_MAXK], lnsd[JB_MAXK];  // the current model
    double c0[JB_MAXK], c1[JB_MAXK];                               // the new coefficients, between the two closing kernels
    double e11, ll, last_ll;
    uint32_t round, stopped, converged, iterations;
};
struct JbOut {
    double *probs, *aprob, *post;
    int32_t *asst;
    uint32_t *ml;
    double confidence;
    uint32_t flags;
};

// ---- host: the Poisson loading, the latent states, the prior, the initial parameters ---------------------------------------------
static void jb_multiplet_counts(double obs_cells, uint32_t n_gems, uint32_t n_entries, double *out) {
    const double mu = JB_CORR_FACTOR * obs_cells / (double)n_gems;
    for (uint32_t j = 1; j <= n_entries; j++)
        out[j - 1] = mu <= 0.0 ? 0.0 : std::exp((double)j * std::log(mu) - std::lgamma((double)j + 1.0) - mu) * (double)n_gems / JB_CORR_FACTOR;
}
static double jb_count_excess(double x, uint32_t n_gems, double n) {
    double c[JB_NUM_TOTAL_TAGS];
    jb_multiplet_counts(x, n_gems, JB_NUM_TOTAL_TAGS, c);
    return cr_pairwise_sum(c, JB_NUM_TOTAL_TAGS) - n;
}

extern "C" int crgpu_jibes_expected_cells(uint64_t n, uint32_t n_gems, double *out) {
    if (!out || !n_gems) return CRGPU_EINVAL;
    *out = 0.0;
    if (!n) return CRGPU_OK;
    // the rising branch ends where d/d mu P(1 <= J <= 14) = pmf(0) - pmf(14) = 0: mu^14 = 14!
    double lo = 0.0, hi = std::exp(std::lgamma(15.0) / 14.0) * (double)n_gems / JB_CORR_FACTOR;
    const double top = jb_count_excess(hi, n_gems, (double)n);
    if (top < 0.0) {
        if (top * top > 2.0) return CRGPU_JIBES_CANT_CONVERGE;
        *out = hi;
        return CRGPU_OK;
    }
    for (int it = 0; it < 200; it++) {
        const double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi) break;
        if (jb_count_excess(mid, n_gems, (double)n) < 0.0) lo = mid; else hi = mid;
    }
    *out = hi;
    return CRGPU_OK;
}

static void jb_solutions(uint32_t elements, uint32_t total, std::vector<uint8_t> &cur, std::vector<uint8_t> &out) {
    if (elements == 1) {
        out.insert(out.end(), cur.begin(), cur.end());
        out.push_back((uint8_t)total);
        return;
    }
    for (uint32_t i = 0; i <= total; i++) {
        cur.push_back((uint8_t)i);
        jb_solutions(elements - 1, total - i, cur, out);
        cur.pop_back();
    }
}
static int jb_setup(uint64_t n, uint32_t k, uint32_t n_gems, uint32_t max_k_lets, double estimated_cells, std::vector<uint8_t> &states,
                    crgpu_jibes_setup *out) {
    if (!k || !max_k_lets || !n_gems) return CRGPU_EINVAL;
    if (k > JB_MAXK || max_k_lets > CRGPU_JIBES_MAX_K_LETS) return CRGPU_ERANGE;
    double c[JB_NUM_TOTAL_TAGS];
    jb_multiplet_counts(estimated_cells, n_gems, JB_NUM_TOTAL_TAGS, c);
    int last = -1;
    for (uint32_t j = 0; j < JB_NUM_TOTAL_TAGS; j++)
        if (std::nearbyint(c[j]) > 0.0) last = (int)j;
    uint32_t mm = last < 0 ? 4u : std::max((uint32_t)last + 1u, 2u);
    const bool limited = mm > max_k_lets;
    if (limited) mm = max_k_lets;
    states.clear();
    std::vector<uint8_t> cur;
    for (uint32_t j = 0; j <= mm; j++) jb_solutions(k, j, cur, states);
    if (limited) states.insert(states.end(), k, (uint8_t)1);
    out->estimated_cells = estimated_cells;
    out->n_states = (uint32_t)(states.size() / k), out->k_let_limited = limited ? 1u : 0u;
    out->max_multiplets = mm, out->max_modeled_k_let = std::max(k, mm);
    (void)n;
    return CRGPU_OK;
}
extern "C" int crgpu_jibes_latent_states(uint64_t n, uint32_t k, uint32_t n_gems, uint32_t max_k_lets, double estimated_cells, uint8_t *states_out,
                                         crgpu_jibes_setup *out) {
    if (!out) return CRGPU_EINVAL;
    std::vector<uint8_t> st;
    const int rc = jb_setup(n, k, n_gems, max_k_lets, estimated_cells, st, out);
    if (rc != CRGPU_OK) return rc;
    if (states_out) std::copy(st.begin(), st.end(), states_out);
    return CRGPU_OK;
}

extern "C" int crgpu_jibes_log_prior(const uint8_t *states, uint32_t n_states, uint32_t k, double estimated_cells, uint32_t n_gems, uint32_t max_k_lets,
                                     uint32_t k_let_limited, uint32_t max_modeled_k_let, double blank_prob, const double *freqs, double *prior_out) {
    if (!states || !prior_out || !n_states || !k || !n_gems) return CRGPU_EINVAL;
    if (k > JB_MAXK || max_k_lets > CRGPU_JIBES_MAX_K_LETS) return CRGPU_ERANGE;
    const uint32_t n_entries = std::max(JB_NUM_TOTAL_TAGS, k);
    double c[JB_MAXK], p[JB_MAXK], pis[JB_MAXK], lfact[4 * JB_MAXK + 1];
    jb_multiplet_counts(estimated_cells, n_gems, n_entries, c);
    const uint32_t m = std::min(max_modeled_k_let, n_entries);
    if (!m) return CRGPU_EINVAL;
    const double total = cr_pairwise_sum(c, m);
    for (uint32_t j = 0; j < m; j++) p[j] = c[j] / total;
    if (k_let_limited) p[m - 1] = max_k_lets < m ? cr_pairwise_sum(p + max_k_lets, m - max_k_lets) : 0.0;
    for (uint32_t t = 0; t < k; t++) pis[t] = std::log(freqs ? freqs[t] : 1.0 / (double)k);
    double f = 1.0;
    lfact[0] = 0.0;
    for (uint32_t j = 1; j <= 4 * JB_MAXK; j++) f *= (double)j, lfact[j] = std::log(f);  // statrs ln_factorial: ln of the cached factorial
    prior_out[0] = std::log(blank_prob);
    const double log_not_blank = std::log(1.0 - blank_prob);
    for (uint32_t s = 1; s < n_states; s++) {
        const uint8_t *x = states + (size_t)s * k;
        uint32_t sum = 0;
        double den = 0.0, pl = 0.0;
        for (uint32_t t = 0; t < k; t++) {
            if (!x[t]) continue;
            if (x[t] > 3) return CRGPU_EINVAL;
            sum += x[t], den += lfact[x[t]], pl += (double)x[t] * pis[t];
        }
        if (!sum || sum > m) return CRGPU_EINVAL;
        prior_out[s] = pl + (lfact[sum] - den) + std::log(p[sum - 1]) + log_not_blank;
    }
    return CRGPU_OK;
}

// np.mean / np.std of a gathered column in numpy's pairwise order
static double jb_mean(const std::vector<double> &v) { return cr_pairwise_sum(v.data(), v.size()) / (double)v.size(); }
extern "C" int crgpu_jibes_initial_parameters(const double *y, uint64_t n, uint32_t k, const int32_t *calls, double *bg, double *fg, double *sd) {
    if (!bg || !fg || !sd || !k || (n && (!y || !calls))) return CRGPU_EINVAL;
    if (k > JB_MAXK) return CRGPU_ERANGE;
    std::vector<uint32_t> bad, good;
    std::vector<double> own, other, all;
    for (uint32_t t = 0; t < k; t++) {
        own.clear(), other.clear(), all.clear();
        for (uint64_t i = 0; i < n; i++) {
            const double v = y[i * k + t];
            all.push_back(v);
            if (calls[i] == (int32_t)t) own.push_back(v);
            else if (calls[i] >= 0 && calls[i] < (int32_t)k) other.push_back(v);
        }
        if (own.size() < 2) {
            bg[t] = fg[t] = sd[t] = std::nan("");
            bad.push_back(t);
            continue;
        }
        good.push_back(t);
        bg[t] = jb_mean(other.empty() ? all : other);
        const double mean = jb_mean(own);
        fg[t] = std::max(0.6 + bg[t], mean) - bg[t];
        for (double &v : own) v = (v - mean) * (v - mean);  // np.std: sqrt(mean(abs(x - mean)^2))
        sd[t] = std::sqrt(jb_mean(own));
    }
    if (!bad.empty()) {
        double fm = 1.0, bm = 0.5, vm = 0.3;
        if (!good.empty()) {
            std::vector<double> a, b, c;
            for (uint32_t t : good) a.push_back(fg[t]), b.push_back(bg[t]), c.push_back(sd[t]);
            fm = jb_mean(a), bm = jb_mean(b), vm = jb_mean(c);
        }
        for (uint32_t t : bad) fg[t] = fm, bg[t] = bm, sd[t] = vm;
    }
    for (uint32_t t = 0; t < k; t++)
        if (sd[t] == 0.0) sd[t] = 0.2;
    return CRGPU_OK;
}

// ---- the tag table -------------------------------------------------------------------------------------------------------------------
// one thread per column: the dense counts of the listed rows (place[row] = position + 1, 0 = not a tag row) and their sum
__global__ __launch_bounds__(256) void k_jb_tag_counts(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                       const int32_t *__restrict__ data, uint64_t V, const uint32_t *__restrict__ place,
                                                       uint32_t n_features, uint32_t n_rows, int32_t *__restrict__ counts,
                                                       unsigned long long *__restrict__ sums, uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < V; c += stride) {
        unsigned long long sum = 0ull;
        for (long long e = indptr[c]; e < indptr[c + 1]; e++) {
            const uint32_t f = (uint32_t)indices[e];
            if (f >= n_features) {
                atomicOr(flag, 4u);
                continue;
            }
            const uint32_t p = place[f];
            if (!p) continue;
            counts[c * n_rows + (p - 1u)] = data[e];
            sum += (unsigned long long)(uint32_t)data[e];
        }
        sums[c] = sum;
    }
}

extern "C" int crgpu_jibes_tag_counts_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint32_t *tag_rows, uint32_t n_rows, uint32_t n_features,
                                          int32_t *counts_out, uint64_t *row_sums_out, uint64_t *near_zero_out, uint64_t *n_near_zero_out,
                                          uint64_t *kept_out) {
    if (!ctx || !m) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, tag_rows && n_rows && n_features, CRGPU_EINVAL, "crgpu_jibes_tag_counts_dev: no tag rows or no features");
    const uint64_t V = m->n_barcodes;
    if (n_near_zero_out) *n_near_zero_out = 0;
    DevBuf rows_b, place_b, cnt_b, sum_b;
    std::vector<uint64_t> rows64(tag_rows, tag_rows + n_rows);
    CR_TRY(dmalloc(ctx, rows_b, (uint64_t)n_rows * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, place_b, (uint64_t)n_features * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, cnt_b, std::max<uint64_t>(V * n_rows, 1) * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, sum_b, std::max<uint64_t>(V, 1) * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, rows_b.p, rows64.data(), (uint64_t)n_rows * sizeof(uint64_t)));
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(place_b.p, 0, (uint64_t)n_features * sizeof(uint32_t), ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(cnt_b.p, 0, std::max<uint64_t>(V * n_rows, 1) * sizeof(int32_t), ctx->stream));
    cr_check_columns<true>(ctx, rows_b.as<uint64_t>(), n_rows, n_features, MarkPlace{place_b.as<uint32_t>()}, d_flag);
    if (V) {
        CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
        hipLaunchKernelGGL(k_jb_tag_counts, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data, V,
                           place_b.as<uint32_t>(), n_features, n_rows, cnt_b.as<int32_t>(), sum_b.as<unsigned long long>(), d_flag);
    }
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_TRY(cr_list_verdict(ctx, flag, "crgpu_jibes_tag_counts_dev", "tag row"));
    CR_REQUIRE(ctx, !(flag & 4u), CRGPU_EINVAL, "crgpu_jibes_tag_counts_dev: the matrix holds a row >= n_features (%u)", n_features);
    if (!V) return CRGPU_OK;
    std::vector<uint64_t> sums(V);
    CR_TRY(crgpu_memcpy_d2h(ctx, sums.data(), sum_b.p, V * sizeof(uint64_t)));
    if (counts_out) CR_TRY(crgpu_memcpy_d2h(ctx, counts_out, cnt_b.p, V * n_rows * sizeof(int32_t)));
    uint64_t nz = 0, nk = 0;
    for (uint64_t c = 0; c < V; c++) {
        if (row_sums_out) row_sums_out[c] = sums[c];
        if (sums[c] <= CRGPU_JIBES_NEAR_ZERO) {
            if (near_zero_out) near_zero_out[nz] = c;
            nz++;
        } else {
            if (kept_out) kept_out[nk] = c;
            nk++;
        }
    }
    if (n_near_zero_out) *n_near_zero_out = nz;
    return CRGPU_OK;
}

// ---- the fit -------------------------------------------------------------------------------------------------------------------------
__global__ void k_jb_init(JbState *st) {
    const uint32_t t = threadIdx.x;
    if (t < JB_MAXK) st->lnsd[t] = log(st->sd[t]);
}

// MODE 0: the sums of the M step and of LL; 1: the residual sums under the new coefficients; 2: the outputs.
// Dynamic LDS: prior (z doubles), one row per wave (4 z doubles), the state words (z u32), the state classes (z bytes).
template <uint32_t KP, int MODE>
__global__ __launch_bounds__(JB_WG) void k_jb_pass(const double *__restrict__ y, uint32_t n, uint32_t k, uint32_t z, const uint32_t *__restrict__ words,
                                                   const double *__restrict__ prior, const uint8_t *__restrict__ cls, const JbState *__restrict__ st,
                                                   double *__restrict__ slab, JbOut out) {
    extern __shared__ double jb_lds[];
    __shared__ double s_bg[JB_MAXK], s_fg[JB_MAXK], s_sd[JB_MAXK], s_lnsd[JB_MAXK], s_c0[JB_MAXK], s_c1[JB_MAXK];
    __shared__ double s_tab[JB_WAVES][64];
    __shared__ double s_red[JB_WAVES][JB_NSTAT_A];
    if (MODE != 2 && st->stopped) return;  // uniform: the latch
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    double *s_prior = jb_lds, *s_row = jb_lds + z + (size_t)wave * z;
    uint32_t *s_words = (uint32_t *)(jb_lds + 5u * (size_t)z);
    uint8_t *s_cls = (uint8_t *)(s_words + z);
    for (uint32_t s = tid; s < z; s += JB_WG) {
        s_prior[s] = prior[s], s_words[s] = words[s];
        if (MODE == 2) s_cls[s] = cls[s];
    }
    if (tid < JB_MAXK) {
        s_bg[tid] = st->bg[tid], s_fg[tid] = st->fg[tid], s_sd[tid] = st->sd[tid], s_lnsd[tid] = st->lnsd[tid];
        s_c0[tid] = st->c0[tid], s_c1[tid] = st->c1[tid];
    }
    __syncthreads();
    double a_first[KP], a_second[KP], a_12[KP], a_22[KP];  // MODE 0; a_first doubles as the residual sums of MODE 1
    double a_11 = 0.0, a_lnm = 0.0, a_max = 0.0;
#pragma unroll
    for (uint32_t t = 0; t < KP; t++) a_first[t] = a_second[t] = a_12[t] = a_22[t] = 0.0;
    const uint32_t i0 = blockIdx.x * JB_CHUNK;
    for (uint32_t j = wave; j < JB_CHUNK; j += JB_WAVES) {  // the same trip count in every wave: the barriers below are uniform
        const uint32_t i = i0 + j;
        const bool live = i < n;  // uniform in the wave
        const double *yr = y + (size_t)(live ? i : 0u) * k;
        {  // the k x 4 distinct log densities of this barcode: statrs' ln_pdf
            const uint32_t t = lane >> 2, c = lane & 3u;
            double v = 0.0;
            if (t < k) {
                const double mu = s_bg[t] + s_fg[t] * (double)c;
                const double d = (yr[t] - mu) / s_sd[t];
                v = (-0.5 * d * d) - JB_LN_SQRT_2PI - s_lnsd[t];
            }
            s_tab[wave][lane] = v;
        }
        __syncthreads();
        const double *tab = s_tab[wave];
        double mx = -INFINITY;
        for (uint32_t s = lane; s < z; s += 64u) {
            const uint32_t w = s_words[s];
            double v = s_prior[s];
#pragma unroll
            for (uint32_t t = 0; t < KP; t++) v += tab[4u * t + ((w >> (2u * t)) & 3u)];
            s_row[s] = v;
            mx = fmax(mx, v);
        }
        mx = wave_max(mx);
        double sum = 0.0;
        for (uint32_t s = lane; s < z; s += 64u) {
            const double e = exp(s_row[s] - mx);
            s_row[s] = e;
            sum += e;
        }
        const double marg = wave_sum(sum);
        if (MODE == 0) {
            if (live) a_lnm += log(marg), a_max += mx;
            double r = 0.0, pa[KP], pb[KP];
#pragma unroll
            for (uint32_t t = 0; t < KP; t++) pa[t] = pb[t] = 0.0;
            for (uint32_t s = lane; s < z; s += 64u) {
                const uint32_t w = s_words[s];
                const double p = s_row[s] / marg;
                r += p;
#pragma unroll
                for (uint32_t t = 0; t < KP; t++) {
                    const double x = (double)((w >> (2u * t)) & 3u), px = p * x;
                    pa[t] += px, pb[t] += px * x;
                }
            }
            const double row_sum = wave_sum(r);  // the reference's tag_cnt * row.sum(): the whole row, the same value in every lane
            if (live) {
                a_11 += row_sum;
#pragma unroll
                for (uint32_t t = 0; t < KP; t++) {
                    const double yt = t < k ? yr[t] : 0.0;
                    a_first[t] += yt * row_sum, a_second[t] += yt * pa[t], a_12[t] += pa[t], a_22[t] += pb[t];
                }
            }
        } else if (MODE == 1) {
            double res[KP];
#pragma unroll
            for (uint32_t t = 0; t < KP; t++) res[t] = 0.0;
            for (uint32_t s = lane; s < z; s += 64u) {
                const uint32_t w = s_words[s];
                const double p = s_row[s] / marg;
#pragma unroll
                for (uint32_t t = 0; t < KP; t++) {
                    const double x = (double)((w >> (2u * t)) & 3u);
                    const double r = (s_c1[t] * x + s_c0[t]) - (t < k ? yr[t] : 0.0);
                    res[t] += r * r * p;
                }
            }
            if (live) {
#pragma unroll
                for (uint32_t t = 0; t < KP; t++) a_first[t] += res[t];
            }
        } else {
            // the outputs of one barcode: class c (0 .. k - 1 only that tag, k Multiplet, k + 1 Blank) ends in lane c
            double mine = 0.0, best = -1.0;
            uint32_t best_s = 0xFFFFFFFFu;
            for (uint32_t s = lane; s < z; s += 64u) {
                const double p = s_row[s] / marg;
                s_row[s] = p;
                if (s_cls[s] == k && p > best) best = p, best_s = s;  // ascending s: the first maximum of the lane
                if (live && out.post) out.post[(size_t)i * z + s] = p;
            }
            for (uint32_t c = 0; c < k + 2u; c++) {
                double part = 0.0;
                for (uint32_t s = lane; s < z; s += 64u) part += s_cls[s] == c ? s_row[s] : 0.0;
                part = wave_sum(part);
                if (lane == c) mine = part;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {  // the first maximum over the Multiplet states: the larger value, then the smaller index
                const double ob = __shfl_xor(best, d);
                const uint32_t os = __shfl_xor(best_s, d);
                if (ob > best || (ob == best && os < best_s)) best = ob, best_s = os;
            }
            double top = lane < k + 2u ? mine : -1.0;
            uint32_t top_c = lane < k + 2u ? lane : 0xFFFFFFFFu;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {  // the first maximum in the order tags, Multiplet, Blank
                const double ob = __shfl_xor(top, d);
                const uint32_t oc = __shfl_xor(top_c, d);
                if (ob > top || (ob == top && oc < top_c)) top = ob, top_c = oc;
            }
            const double blank = __shfl(mine, (int)(k + 1u));
            if (live) {
                if (lane < k + 2u) out.probs[(size_t)i * (k + 2u) + lane] = mine;
                if (lane == 0u) {
                    double pr = top;
                    if ((out.flags & CRGPU_JIBES_EXCLUDE_BLANKS) && top_c != k + 1u) pr = pr / (1.0 - blank);
                    const bool unassigned = !(out.flags & CRGPU_JIBES_NO_CONFIDENCE) && pr < out.confidence;
                    out.asst[i] = (int32_t)(unassigned ? k + 2u : top_c);
                    out.aprob[i] = top;
                    out.ml[i] = best_s == 0xFFFFFFFFu ? 0u : best_s;
                }
            }
        }
        __syncthreads();  // the table and the row are rewritten by the next barcode
    }
    if (MODE == 2) return;
    // the chunk's sums: the butterfly, then the four waves in ascending order
    const uint32_t n_stat = MODE == 0 ? 3u + 4u * KP : KP;
    if (MODE == 0) {  // a_lnm, a_max, a_11 and a_first hold whole-row values: the wave's barcodes in ascending order, no butterfly
        if (lane == 0u) s_red[wave][0] = a_lnm, s_red[wave][1] = a_max, s_red[wave][2] = a_11;
#pragma unroll
        for (uint32_t t = 0; t < KP; t++) {
            const double f = a_first[t], sc = wave_sum(a_second[t]), e12 = wave_sum(a_12[t]), e22 = wave_sum(a_22[t]);
            if (lane == 0u) s_red[wave][3u + 4u * t] = f, s_red[wave][4u + 4u * t] = sc, s_red[wave][5u + 4u * t] = e12, s_red[wave][6u + 4u * t] = e22;
        }
    } else {
#pragma unroll
        for (uint32_t t = 0; t < KP; t++) {
            const double f = wave_sum(a_first[t]);
            if (lane == 0u) s_red[wave][t] = f;
        }
    }
    __syncthreads();
    if (tid < n_stat)
        slab[(size_t)blockIdx.x * (MODE == 0 ? JB_NSTAT_A : JB_NSTAT_B) + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

// the chunks in ascending order, LL, the stop rule (perform_EM) and its latch, the new coefficients (maximize_parameters)
__global__ __launch_bounds__(JB_WG) void k_jb_close_a(const double *__restrict__ slab, uint32_t n_chunks, uint32_t k, JbState *st, double abs_tol,
                                                      double rel_tol, uint32_t max_reps) {
    __shared__ double s_tile[JB_CLOSE_ROWS_A * JB_NSTAT_A];
    __shared__ double s[JB_NSTAT_A];
    if (st->stopped) return;
    const uint32_t tid = threadIdx.x;
    {  // the workgroup brings the slab through LDS a tile of chunks at a time; thread t adds statistic t in ascending chunk order
        double a = 0.0;
        for (uint32_t c0 = 0; c0 < n_chunks; c0 += JB_CLOSE_ROWS_A) {
            const uint32_t m = n_chunks - c0 < JB_CLOSE_ROWS_A ? n_chunks - c0 : JB_CLOSE_ROWS_A;
            for (uint32_t i = tid; i < m * JB_NSTAT_A; i += JB_WG) s_tile[i] = slab[(size_t)c0 * JB_NSTAT_A + i];
            __syncthreads();
            if (tid < 3u + 4u * k)
                for (uint32_t j = 0; j < m; j++) a += s_tile[j * JB_NSTAT_A + tid];
            __syncthreads();
        }
        if (tid < 3u + 4u * k) s[tid] = a;
    }
    __syncthreads();
    if (tid != 0u) return;
    const double ll = s[0] + s[1], last = st->last_ll;
    const uint32_t round = st->round;
    st->ll = ll;
    if (round >= 1u) {  // rep = round: one_EM_step has run `round` times
        const double rel_change = 1.0 - ll / last, abs_change = ll - last;
        bool stop = false, conv = false;
        if (round > max_reps) stop = true;
        else if (!(last == -INFINITY) && ((abs_change < abs_tol) || (rel_change < rel_tol))) stop = conv = true;
        if (stop) {
            st->iterations = round, st->converged = conv ? 1u : 0u;
            st->stopped = 1u;
            return;
        }
        st->last_ll = ll;
    }
    const double e11 = s[2];
    st->e11 = e11;
    for (uint32_t t = 0; t < k; t++) {
        const double first = s[3u + 4u * t], second = s[4u + 4u * t], e12 = s[5u + 4u * t], e22 = s[6u + 4u * t];
        const double det = 1.0 / (e11 * e22 - e12 * e12);
        double c0 = (det * e22) * first + (det * -e12) * second;
        double c1 = (det * -e12) * first + (det * e11) * second;
        if (c1 < JB_MIN_FOREGROUND_DELTA) {
            c1 = JB_MIN_FOREGROUND_DELTA;
            c0 = first / e11 - JB_MIN_FOREGROUND_DELTA * (e12 / e11);
        }
        st->c0[t] = c0, st->c1[t] = c1;
    }
}

// the residual sums in chunk order, the new sd: the model of the next round
__global__ __launch_bounds__(JB_WG) void k_jb_close_b(const double *__restrict__ slab, uint32_t n_chunks, uint32_t k, JbState *st) {
    __shared__ double s_tile[JB_CLOSE_ROWS_B * JB_NSTAT_B];
    if (st->stopped) return;
    const uint32_t t = threadIdx.x;
    double a = 0.0;
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += JB_CLOSE_ROWS_B) {
        const uint32_t m = n_chunks - c0 < JB_CLOSE_ROWS_B ? n_chunks - c0 : JB_CLOSE_ROWS_B;
        for (uint32_t i = t; i < m * JB_NSTAT_B; i += JB_WG) s_tile[i] = slab[(size_t)c0 * JB_NSTAT_B + i];
        __syncthreads();
        if (t < k)
            for (uint32_t j = 0; j < m; j++) a += s_tile[j * JB_NSTAT_B + t];
        __syncthreads();
    }
    if (t < k) {
        const double sd = fmax(sqrt(a / st->e11), JB_SD_FLOOR);
        st->bg[t] = st->c0[t], st->fg[t] = st->c1[t], st->sd[t] = sd, st->lnsd[t] = log(sd);
    }
    if (t == 0u) st->round = st->round + 1u;
}

template <int MODE>
static void jb_launch_pass(crgpu_ctx *ctx, uint32_t kp, uint32_t n_chunks, size_t dyn, const double *y, uint32_t n, uint32_t k, uint32_t z,
                           const uint32_t *words, const double *prior, const uint8_t *cls, const JbState *st, double *slab, const JbOut &out) {
#define JB_LAUNCH(KP)                                                                                                                          \
    hipLaunchKernelGGL((k_jb_pass<KP, MODE>), dim3(n_chunks), dim3(JB_WG), dyn, ctx->stream, y, n, k, z, words, prior, cls, st, slab, out)
    switch (kp) {
    case 2: JB_LAUNCH(2); break;
    case 4: JB_LAUNCH(4); break;
    case 8: JB_LAUNCH(8); break;
    case 12: JB_LAUNCH(12); break;
    default: JB_LAUNCH(16); break;
    }
#undef JB_LAUNCH
}

extern "C" int crgpu_jibes_fit_dev(crgpu_ctx *ctx, const double *y, uint64_t n, uint32_t k, const crgpu_jibes_fit_args *a, crgpu_jibes_fit_result *res) {
    if (!ctx || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    memset(res, 0, sizeof(*res));
    CR_REQUIRE(ctx, k >= 1 && a->max_k_lets >= 1, CRGPU_EINVAL, "crgpu_jibes_fit_dev: no tag or max_k_lets 0");
    CR_REQUIRE(ctx, k <= JB_MAXK, CRGPU_ERANGE, "crgpu_jibes_fit_dev: %u tags, at most %u", k, JB_MAXK);
    CR_REQUIRE(ctx, a->max_k_lets <= CRGPU_JIBES_MAX_K_LETS, CRGPU_ERANGE, "crgpu_jibes_fit_dev: max_k_lets %u, at most %u", a->max_k_lets,
               CRGPU_JIBES_MAX_K_LETS);
    CR_REQUIRE(ctx, a->bg && a->fg && a->sd && (y || !n) && a->n_gems, CRGPU_EINVAL, "crgpu_jibes_fit_dev: NULL model or data, or n_gems 0");
    CR_REQUIRE(ctx, n < 0xFFFFFFFFull - JB_CHUNK, CRGPU_ERANGE, "crgpu_jibes_fit_dev: too many barcodes");
    for (uint32_t t = 0; t < k; t++) {
        CR_REQUIRE(ctx, a->fg[t] >= JB_MIN_FOREGROUND_DELTA, CRGPU_EINVAL, "crgpu_jibes_fit_dev: cannot initialize with foreground value %g less than %g",
                   a->fg[t], JB_MIN_FOREGROUND_DELTA);
        CR_REQUIRE(ctx, a->sd[t] > 0.0 && std::isfinite(a->bg[t]) && std::isfinite(a->sd[t]), CRGPU_EINVAL,
                   "crgpu_jibes_fit_dev: the initial model of tag %u is not finite or its sd is not positive", t);
        res->bg[t] = a->bg[t], res->fg[t] = a->fg[t], res->sd[t] = a->sd[t];
    }
    for (uint64_t i = 0; i < n * k; i++) CR_REQUIRE(ctx, std::isfinite(y[i]), CRGPU_EINVAL, "crgpu_jibes_fit_dev: y[%llu] is not finite", (unsigned long long)i);
    std::vector<uint8_t> states;
    crgpu_jibes_setup su;
    CR_REQUIRE(ctx, jb_setup(n, k, a->n_gems, a->max_k_lets, a->estimated_cells, states, &su) == CRGPU_OK, CRGPU_EINVAL, "crgpu_jibes_fit_dev: no latent states");
    const uint32_t z = su.n_states;
    res->n_states = z, res->k_let_limited = su.k_let_limited;
    CR_REQUIRE(ctx, z <= CRGPU_JIBES_MAX_STATES, CRGPU_ERANGE, "crgpu_jibes_fit_dev: %u latent states", z);
    if (n == 0) {  // perform_EM: no cells, no EM
        res->ll = 0.0, res->converged = 1u;
        for (uint32_t t = 0; t < k; t++) res->fg[t] = 0.0;
        return CRGPU_OK;
    }
    std::vector<double> prior(z);
    CR_REQUIRE(ctx, crgpu_jibes_log_prior(states.data(), z, k, a->estimated_cells, a->n_gems, a->max_k_lets, su.k_let_limited, su.max_modeled_k_let,
                                          a->blank_prob, a->freqs, prior.data()) == CRGPU_OK, CRGPU_EINVAL, "crgpu_jibes_fit_dev: the prior cannot be formed");
    std::vector<uint32_t> words(z);
    std::vector<uint8_t> cls(z);
    for (uint32_t s = 0; s < z; s++) {
        uint32_t w = 0, sum = 0, only = k;  // get_cols_associated_with_assignments: only tag t, Multiplet (k), Blank (k + 1)
        for (uint32_t t = 0; t < k; t++) w |= (uint32_t)states[(size_t)s * k + t] << (2u * t), sum += states[(size_t)s * k + t];
        for (uint32_t t = 0; t < k; t++)
            if (sum && states[(size_t)s * k + t] == sum) only = t;
        words[s] = w, cls[s] = (uint8_t)(sum ? only : k + 1u);
    }
    const uint32_t n32 = (uint32_t)n, n_chunks = (n32 + JB_CHUNK - 1u) / JB_CHUNK;
    const uint32_t kp = k <= 2 ? 2u : k <= 4 ? 4u : k <= 8 ? 8u : k <= 12 ? 12u : 16u;
    const size_t dyn = (size_t)z * (5u * sizeof(double) + sizeof(uint32_t) + 1u) + 8u;
    DevBuf y_b, w_b, p_b, c_b, st_b, slab_a, slab_b, probs_b, asst_b, aprob_b, ml_b, post_b;
    CR_TRY(dmalloc(ctx, y_b, n * k * sizeof(double)));
    CR_TRY(dmalloc(ctx, w_b, z * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, p_b, z * sizeof(double)));
    CR_TRY(dmalloc(ctx, c_b, z));
    CR_TRY(dmalloc(ctx, st_b, sizeof(JbState)));
    CR_TRY(dmalloc(ctx, slab_a, (uint64_t)n_chunks * JB_NSTAT_A * sizeof(double)));
    CR_TRY(dmalloc(ctx, slab_b, (uint64_t)n_chunks * JB_NSTAT_B * sizeof(double)));
    CR_TRY(dmalloc(ctx, probs_b, n * (k + 2u) * sizeof(double)));
    CR_TRY(dmalloc(ctx, asst_b, n * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, aprob_b, n * sizeof(double)));
    CR_TRY(dmalloc(ctx, ml_b, n * sizeof(uint32_t)));
    if (a->posterior_out) CR_TRY(dmalloc(ctx, post_b, n * z * sizeof(double)));
    JbState h = {};
    for (uint32_t t = 0; t < JB_MAXK; t++) h.bg[t] = 0.0, h.fg[t] = 1.0, h.sd[t] = 1.0;
    for (uint32_t t = 0; t < k; t++) h.bg[t] = a->bg[t], h.fg[t] = a->fg[t], h.sd[t] = a->sd[t];
    h.last_ll = -INFINITY, h.ll = -INFINITY;
    CR_TRY(crgpu_memcpy_h2d(ctx, y_b.p, y, n * k * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, w_b.p, words.data(), z * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, p_b.p, prior.data(), z * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, c_b.p, cls.data(), z));
    CR_TRY(crgpu_memcpy_h2d(ctx, st_b.p, &h, sizeof(h)));
    JbState *d_st = st_b.as<JbState>();
    JbOut out = {probs_b.as<double>(), aprob_b.as<double>(), a->posterior_out ? post_b.as<double>() : nullptr, asst_b.as<int32_t>(), ml_b.as<uint32_t>(),
                 a->confidence, a->flags};
    const uint32_t batch = ctx->jibes_batch ? ctx->jibes_batch : 8u;
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(k_jb_init, dim3(1), dim3(64), 0, ctx->stream, d_st);
    uint64_t rounds = 0;
    const uint64_t rounds_max = (uint64_t)a->max_reps + 2u;  // round max_reps + 1 stops at the latest
    while (true) {
        {
            CrTimer t(ctx, CRGPU_T_MATRIX, (uint64_t)batch * n * z);
            for (uint32_t b = 0; b < batch && rounds < rounds_max; b++, rounds++) {
                jb_launch_pass<0>(ctx, kp, n_chunks, dyn, y_b.as<double>(), n32, k, z, w_b.as<uint32_t>(), p_b.as<double>(), c_b.as<uint8_t>(), d_st,
                                  slab_a.as<double>(), out);
                hipLaunchKernelGGL(k_jb_close_a, dim3(1), dim3(JB_WG), 0, ctx->stream, slab_a.as<double>(), n_chunks, k, d_st, a->abs_tol, a->rel_tol,
                                   a->max_reps);
                jb_launch_pass<1>(ctx, kp, n_chunks, dyn, y_b.as<double>(), n32, k, z, w_b.as<uint32_t>(), p_b.as<double>(), c_b.as<uint8_t>(), d_st,
                                  slab_b.as<double>(), out);
                hipLaunchKernelGGL(k_jb_close_b, dim3(1), dim3(JB_WG), 0, ctx->stream, slab_b.as<double>(), n_chunks, k, d_st);
            }
            CR_HIP(ctx, hipGetLastError());
        }
        CR_TRY(crgpu_memcpy_d2h(ctx, &h, d_st, sizeof(h)));  // the latch: the one synchronisation of a batch
        if (h.stopped) break;
        CR_REQUIRE(ctx, rounds < rounds_max, CRGPU_EHIP, "crgpu_jibes_fit_dev: no stop after %llu rounds", (unsigned long long)rounds);
    }
    res->fit_ms = cr_ms_since(t0);
    res->ll = h.ll, res->iterations = h.iterations, res->converged = h.converged;
    for (uint32_t t = 0; t < k; t++) res->bg[t] = h.bg[t], res->fg[t] = h.fg[t], res->sd[t] = h.sd[t];
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, n * z);
        jb_launch_pass<2>(ctx, kp, n_chunks, dyn, y_b.as<double>(), n32, k, z, w_b.as<uint32_t>(), p_b.as<double>(), c_b.as<uint8_t>(), d_st, nullptr, out);
        CR_HIP(ctx, hipGetLastError());
    }
    if (a->probs_out) CR_TRY(crgpu_memcpy_d2h(ctx, a->probs_out, probs_b.p, n * (k + 2u) * sizeof(double)));
    if (a->assignment_out) CR_TRY(crgpu_memcpy_d2h(ctx, a->assignment_out, asst_b.p, n * sizeof(int32_t)));
    if (a->assignment_prob_out) CR_TRY(crgpu_memcpy_d2h(ctx, a->assignment_prob_out, aprob_b.p, n * sizeof(double)));
    if (a->ml_state_out) CR_TRY(crgpu_memcpy_d2h(ctx, a->ml_state_out, ml_b.p, n * sizeof(uint32_t)));
    if (a->posterior_out) CR_TRY(crgpu_memcpy_d2h(ctx, a->posterior_out, post_b.p, n * z * sizeof(double)));
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRGPU_OK;
}
