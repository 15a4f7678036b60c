// test_umap_kernels.hip -- the kernels of cellranger_amd/csrc/umap.hip by direct launch into guarded buffers, at constructed shapes.
// What holds + - * /, floor and integers only has an ORDER MODEL on the host whose bits the device must give: rho, the row sums and
// their total, the steps and the mid of the search, the keys, the CSR structure, the union values from the device's own memberships,
// wmax, the prune; in an epoch the active set and n_neg (through both schedule states and the two counters) and the sampled vertices
// (umap_sample through a probe kernel).  Which branch a term took shows in its value: d2 = 0 and a sample of the row itself give a
// term of exactly 0, a clipped term is exactly 4 (8 for an attraction); the model counts how often each occurred.
// What holds exp or pow is compared against long double with a bound derived here (u = 2^-53):
//     OCML's f64 exp and pow are documented at 1 ulp = 2 u (ROCm device libraries, doc/OCML.md, the table of function accuracies: the
//     figure is read there; the document is not part of this repository).
//     d2: D differences (u each, 2 u on a square), D products (u), D - 1 additions of positive terms: e_d2 = (D + 2) u
//     p = pow(d2, b): b e_d2 + 2 u = e_p
//     attraction c v: p / d2 (e_p + e_d2 + u), the product with the host's (-2 a b) (u), a p + 1 (e_p + 2 u), the division (u), c v
//                 (u for v, u for the product): e_att = 2 e_p + e_d2 + 7 u = ((2 b + 1)(D + 2) + 11) u
//     a negative sample's c v: 0.001 + d2 (e_d2 + u), the denominator (e_p + 2 u), their product (u), the division (u), c v (2 u):
//                 ((b + 1)(D + 2) + 9) u <= e_att
//     the clip is 1-Lipschitz and continuous at +-4, so a clipped term adds nothing; the factor 2 is exact
//     delta: m terms added in one order: gamma(m) sum |terms| (Higham, Accuracy and Stability, 3.1), gamma(k) = k u / (1 - k u)
//     y' = y + alpha delta: u on the product, u on the sum
//     psum at the device's own sigma: x = d - rho (u), x / sigma (u), so the argument t of exp is off by 2 u t and exp by 2 u t of itself
//                 (t exp(-t) <= 1 / e), plus exp's 2 u; k terms, then gamma(k) on the sum (each term <= 1)
// The order model of delta uses the host's pow: it is within the same bound of the reference (--host-only checks that) and not bit-equal.
//
// umap.hip is compiled here inside a namespace: the same text under the same flags (cellranger_amd.build.FLAGS), not the library's
// object code.  The context, the pool, the scan and the radix sort come from libcrgpu.so.
//
//   test_umap_kernels --host-only              every case without a device: the order model within the bound of the reference
//   test_umap_kernels --group graph|epoch
// One line per case, "all tests passed" at the end; the first mismatch or HIP error ends the program with status 1.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "graph_common.h"
#include "kernel_test.h"
#include "philox.h"

namespace umap_under_test {
#include "umap.hip"
}
using namespace umap_under_test;

typedef long double ld_t;
static double g_worst_delta = 0.0, g_worst_y = 0.0, g_worst_exp = 0.0, g_worst_psum = 0.0;  // the device's, or with --host-only the order model's
static double g_model[4] = {0.0, 0.0, 0.0, 0.0};                                        // the order model's beside a device
static uint64_t g_zero_d2 = 0, g_self = 0, g_clipped = 0, g_neg0 = 0, g_neg15 = 0, g_neg16 = 0;
static void within(double *worst, const char *what, uint64_t at, double got, ld_t ref, double bound) {
    const double dev = (double)fabsl((ld_t)got - ref);
    if (!(dev <= bound)) die("%s[%llu]: %.17g against %.21Lg, off by %.3g, bound %.3g", what, (unsigned long long)at, got, ref, dev, bound);
    if (bound > 0.0) *worst = std::max(*worst, dev / bound);
}
// ---- the order model: the stream -----------------------------------------------------------------------------------------------------
static void host_philox(uint64_t c0, uint64_t c1, uint64_t k0, uint64_t w[4]) {
    uint64_t c2 = 0, c3 = 0, k1 = 0;
    for (int r = 0; r < 10; r++) {
        const unsigned __int128 m0 = (unsigned __int128)0xD2E7470EE14C6C93ull * c0, m1 = (unsigned __int128)0xCA5A826395121157ull * c2;
        const uint64_t hi0 = (uint64_t)(m0 >> 64), lo0 = (uint64_t)m0, hi1 = (uint64_t)(m1 >> 64), lo1 = (uint64_t)m1;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += 0x9E3779B97F4A7C15ull, k1 += 0xBB67AE8584CAA73Bull;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}
static uint32_t model_sample(uint64_t seed, uint64_t epoch, uint64_t q, uint32_t n) {
    uint64_t w[4];
    host_philox(1ull + (q >> 2), epoch, seed, w);
    return (uint32_t)(w[q & 3] % n);
}
__global__ void k_probe_sample(UmapStep s, const uint64_t *__restrict__ q, uint32_t m, uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) out[i] = umap_sample(s, q[i]);
}

// ---- the epoch -----------------------------------------------------------------------------------------------------------------------
struct Graph {
    uint32_t n = 0;
    std::vector<long long> indptr;
    std::vector<int32_t> indices;
    std::vector<double> values;
};
static Graph make_graph(uint32_t n, const std::map<std::pair<uint32_t, uint32_t>, double> &edges) {
    std::vector<std::map<uint32_t, double>> rows(n);
    for (const auto &e : edges) rows[e.first.first][e.first.second] = e.second, rows[e.first.second][e.first.first] = e.second;
    Graph g;
    g.n = n;
    g.indptr.push_back(0);
    for (uint32_t i = 0; i < n; i++) {
        for (const auto &c : rows[i]) g.indices.push_back((int32_t)c.first), g.values.push_back(c.second);
        g.indptr.push_back((long long)g.indices.size());
    }
    return g;
}
// row 0 is a hub of n - 1 entries, the others form a chain: rows of 2 and 3 entries; (3, 4) is an entry
static Graph hub_graph(uint32_t n, uint64_t seed) {
    Rng rng(seed);
    std::map<std::pair<uint32_t, uint32_t>, double> e;
    for (uint32_t j = 1; j < n; j++) e[{0u, j}] = j == 1 ? 1.0 : 0.05 + 0.95 * rng.unit();
    for (uint32_t j = 1; j + 1 < n; j++) e[{j, j + 1}] = 0.05 + 0.95 * rng.unit();
    return make_graph(n, e);
}
// row n - 1 has no entry, rows n - 2 and n - 3 one (each other); rows 1, 2, 3 have T - 1, T, T + 1; (3, 4) is an entry
static Graph lengths_graph(uint32_t n, uint32_t T, uint64_t seed) {
    Rng rng(seed);
    std::map<std::pair<uint32_t, uint32_t>, double> e;
    e[{n - 3, n - 2}] = 1.0;
    for (uint32_t m = 0; m + 1 < T; m++) e[{1u, 10u + m}] = 0.05 + 0.95 * rng.unit();
    for (uint32_t m = 0; m < T; m++) e[{2u, 10u + m}] = 0.05 + 0.95 * rng.unit();
    e[{3u, 4u}] = 0.05 + 0.95 * rng.unit();
    for (uint32_t m = 0; m < T; m++) e[{3u, 10u + m}] = 0.05 + 0.95 * rng.unit();
    return make_graph(n, e);
}
struct Epoch {
    std::vector<double> eons, eonns, delta, ynew;                  // the order model
    std::vector<unsigned long long> counts;
    std::vector<ld_t> delta_ref, abs_ref;                          // the reference and sum |terms| per coordinate
    std::vector<uint32_t> n_terms;
};
static double clip4(double x) { return x > 4.0 ? 4.0 : (x < -4.0 ? -4.0 : x); }
static ld_t clip4l(ld_t x) { return x > 4.0L ? 4.0L : (x < -4.0L ? -4.0L : x); }
static Epoch model_epoch(const Graph &g, uint32_t D, const std::vector<double> &Y, const std::vector<double> &eons, const std::vector<double> &eonns,
                         const UmapStep &s) {
    Epoch o;
    const uint32_t n = g.n;
    o.eons = eons, o.eonns = eonns;
    o.delta.assign((size_t)n * D, 0.0), o.ynew.assign((size_t)n * D, 0.0), o.counts.assign(2 * (size_t)n, 0);
    o.delta_ref.assign((size_t)n * D, 0.0L), o.abs_ref.assign((size_t)n * D, 0.0L), o.n_terms.assign(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        auto add_term = [&](uint32_t other, bool attract, bool self) {
            double v[3], d2 = 0.0;
            ld_t vl[3], d2l = 0.0L;
            for (uint32_t t = 0; t < D; t++) {
                v[t] = Y[(size_t)i * D + t] - Y[(size_t)other * D + t], d2 += v[t] * v[t];
                vl[t] = (ld_t)Y[(size_t)i * D + t] - (ld_t)Y[(size_t)other * D + t], d2l += vl[t] * vl[t];
            }
            double c = 0.0;
            ld_t cl = 0.0L;
            if (d2 > 0.0) {
                const double p = std::pow(d2, s.b), den = s.a * p + 1.0;
                c = attract ? (s.m2ab * (p / d2)) / den : s.g2b / ((0.001 + d2) * den);
                const ld_t pl = powl(d2l, (ld_t)s.b), denl = (ld_t)s.a * pl + 1.0L;
                cl = attract ? ((ld_t)s.m2ab * (pl / d2l)) / denl : (ld_t)s.g2b / ((0.001L + d2l) * denl);
            } else {
                g_zero_d2 += self ? 0u : 1u;
            }
            g_self += self ? 1u : 0u;
            bool clipped = false;
            for (uint32_t t = 0; t < D; t++) {
                const double x = clip4(c * v[t]);
                clipped |= x != c * v[t];
                o.delta[(size_t)i * D + t] += attract ? 2.0 * x : x;
                const ld_t xl = clip4l(cl * vl[t]), tl = attract ? 2.0L * xl : xl;
                o.delta_ref[(size_t)i * D + t] += tl, o.abs_ref[(size_t)i * D + t] += fabsl(tl);
            }
            g_clipped += clipped ? 1u : 0u;
            o.n_terms[i]++;
        };
        for (long long e = g.indptr[i]; e < g.indptr[i + 1]; e++) {
            if (!(eons[e] <= s.nd)) continue;
            const double eps = s.wmax / g.values[e], epns = eps / s.rate;
            const double f = std::floor((s.nd - eonns[e]) / epns);
            const uint32_t n_neg = f >= 16.0 ? 16u : (f > 0.0 ? (uint32_t)f : 0u);
            g_neg0 += n_neg == 0u, g_neg15 += n_neg == 15u, g_neg16 += n_neg == 16u;
            o.eons[e] = eons[e] + eps, o.eonns[e] = eonns[e] + (double)n_neg * epns;
            o.counts[2 * (size_t)i] += 1, o.counts[2 * (size_t)i + 1] += n_neg;
            add_term((uint32_t)g.indices[e], true, false);
            for (uint32_t k = 0; k < n_neg; k++) {
                const uint32_t kk = model_sample(s.seed, s.epoch, (uint64_t)e * 16u + k, n);
                add_term(kk, false, kk == i);
            }
        }
        for (uint32_t t = 0; t < D; t++) o.ynew[(size_t)i * D + t] = Y[(size_t)i * D + t] + s.alpha * o.delta[(size_t)i * D + t];
    }
    return o;
}
// delta and y' (the device's or the order model's) against the reference
static void check_epoch_ld(const Epoch &m, uint32_t n, uint32_t D, const std::vector<double> &Y, const UmapStep &s, const std::vector<double> &delta,
                           const std::vector<double> &ynew, double *worst_delta, double *worst_y) {
    const double e_att = ((2.0 * s.b + 1.0) * (D + 2.0) + 11.0) * U, e_term = e_att / (1.0 - e_att);
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t t = 0; t < D; t++) {
            const size_t at = (size_t)i * D + t;
            const double sum_abs = (double)m.abs_ref[at];
            const double d_bound = (e_term + gamma_k(m.n_terms[i]) * (1.0 + e_term) + (m.n_terms[i] + 8.0) * 0x1.0p-64) * sum_abs;
            within(worst_delta, "delta", at, delta[at], m.delta_ref[at], d_bound);
            const ld_t yref = (ld_t)Y[at] + (ld_t)s.alpha * m.delta_ref[at];
            within(worst_y, "y'", at, ynew[at], yref, s.alpha * d_bound * (1.0 + 2.0 * U) + U * std::fabs(s.alpha * (double)m.delta_ref[at]) * 1.01 +
                                                                 U * (double)fabsl(yref) * 1.01);
        }
}
template <uint32_t D>
static void epoch_case(const char *name, const Graph &g, uint64_t seed, const std::vector<std::pair<uint32_t, uint32_t>> &settings) {
    const uint32_t n = g.n;
    const uint64_t nnz = g.values.size();
    Rng rng(seed);
    std::vector<double> Y((size_t)n * D);
    for (auto &y : Y) y = 10.0 * rng.unit();
    for (uint32_t t = 0; t < D; t++) Y[4 * D + t] = Y[3 * D + t];  // coincident rows with an entry between them: d2 = 0
    for (uint32_t t = 0; t < D; t++) Y[6 * D + t] = Y[5 * D + t] + 1e-3;  // a pair this near is clipped
    const double a = 0.9921756240062863, b = 1.112253375992829, rate = 8.0;
    UmapStep s = {a, b, (-2.0 * a) * b, (2.0 * 1.0) * b, 0.0, 1.0, rate, 10.0, 12345u + seed, 10u, n, 0u};
    s.alpha = 1.0 * (1.0 - s.nd / 100.0);
    // a crafted state at epoch 10: by entry, not active; active with n_neg 0, 1, 15, more than the 16 words it owns, 5
    std::vector<double> eons(nnz), eonns(nnz);
    static const double back[6] = {0.0, 0.5, 1.5, 15.5, 20.5, 5.5};
    for (uint64_t e = 0; e < nnz; e++) {
        const double eps = 1.0 / g.values[e], epns = eps / rate;
        eons[e] = e % 6u == 0u ? 10.5 : 9.25, eonns[e] = 10.0 - back[e % 6u] * epns;
    }
    const Epoch m = model_epoch(g, D, Y, eons, eonns, s);
    check_epoch_ld(m, n, D, Y, s, m.delta, m.ynew, g_host_only ? &g_worst_delta : &g_model[0], g_host_only ? &g_worst_y : &g_model[1]);
    if (!g_host_only) {
        GBuf<long long> d_ptr(g.indptr);
        GBuf<int32_t> d_ind(g.indices);
        GBuf<double> d_val(g.values), d_Y(Y);
        std::vector<double> first_y, first_delta;
        for (const auto &set : settings) {
            GBuf<double> d_eons(eons), d_eonns(eonns), d_new((uint64_t)n * D), d_delta((uint64_t)n * D);
            GBuf<unsigned long long> d_counts(std::vector<unsigned long long>(2 * (size_t)n, 0ull));
            UmapStep st = s;
            st.thr = set.first;
            umap_launch_epoch<D>(g_gpu->ctx, set.second, d_ptr.d, d_ind.d, d_val.d, d_Y.d, st, d_eons.d, d_eonns.d, d_new.d, d_delta.d, d_counts.d);
            g_gpu->launched("k_umap_epoch");
            const std::vector<double> ynew = d_new.get("Ynew"), delta = d_delta.get("delta");
            same("epoch_of_next_sample", d_eons.get("eons"), m.eons);
            same("epoch_of_next_negative_sample", d_eonns.get("eonns"), m.eonns);
            same("counts", d_counts.get("counts"), m.counts);
            (void)d_Y.get("Y"), (void)d_val.get("values");
            check_epoch_ld(m, n, D, Y, s, delta, ynew, &g_worst_delta, &g_worst_y);
            for (uint32_t i = 0; i < n; i++)  // the branches show in the values: a row without an active entry does not move
                if (m.n_terms[i] == 0)
                    for (uint32_t t = 0; t < D; t++)
                        if (delta[(size_t)i * D + t] != 0.0 || ynew[(size_t)i * D + t] != Y[(size_t)i * D + t]) die("%s: row %u without a term moved", name, i);
            if (first_y.empty()) first_y = ynew, first_delta = delta;
            same("Ynew under a seam", ynew, first_y);
            same("delta under a seam", delta, first_delta);
        }
    }
    case_done("epoch %-8s n %4u dims %u nnz %5llu: %zu settings equal bit for bit", name, n, D, (unsigned long long)nnz, settings.size());
}
static void group_epoch() {
    const uint32_t T = 6;
    // (wave_row_len, threads of a workgroup): every row a lane; the threshold one below, at and above the rows of T - 1, T, T + 1 entries;
    // every row with an entry a wave; the hub alone
    const std::vector<std::pair<uint32_t, uint32_t>> settings = {{1u << 30, 256u}, {T - 1u, 64u}, {T, 128u}, {T + 1u, 256u}, {T + 2u, 64u}, {1u, 128u},
                                                                 {1u, 64u}, {32u, 256u}};
    for (uint32_t n : {63u, 64u, 65u, 255u, 257u}) {
        epoch_case<2>("hub", hub_graph(n, 100 + n), 200 + n, settings);
        epoch_case<3>("hub", hub_graph(n, 300 + n), 400 + n, settings);
        epoch_case<2>("lengths", lengths_graph(n, T, 500 + n), 600 + n, settings);
        epoch_case<3>("lengths", lengths_graph(n, T, 700 + n), 800 + n, settings);
    }
    if (!(g_zero_d2 && g_self && g_clipped && g_neg0 && g_neg15 && g_neg16))
        die("a branch was never taken: d2 = 0 %llu, self-sample %llu, clipped %llu, n_neg 0 %llu, 15 %llu, 16 %llu", (unsigned long long)g_zero_d2,
            (unsigned long long)g_self, (unsigned long long)g_clipped, (unsigned long long)g_neg0, (unsigned long long)g_neg15, (unsigned long long)g_neg16);
    std::printf("branches: d2 = 0 %llu, self-sample %llu, clipped terms %llu, n_neg 0 %llu, 15 %llu, held to 16 %llu\n", (unsigned long long)g_zero_d2,
                (unsigned long long)g_self, (unsigned long long)g_clipped, (unsigned long long)g_neg0, (unsigned long long)g_neg15, (unsigned long long)g_neg16);
    // the stream and the schedule's start
    const uint32_t m = 1000;
    std::vector<uint64_t> q(m);
    std::vector<uint32_t> want(m);
    Rng rng(7);
    UmapStep s = {};
    s.seed = 0xFFFFFFFF12345678ull, s.epoch = 499, s.n = 2147483647u;
    for (uint32_t i = 0; i < m; i++) q[i] = i < 40 ? i : rng.next() >> 2, want[i] = model_sample(s.seed, s.epoch, q[i], s.n);
    if (!g_host_only) {
        GBuf<uint64_t> d_q(q);
        GBuf<uint32_t> d_out((uint64_t)m);
        hipLaunchKernelGGL(k_probe_sample, dim3((m + 255) / 256), dim3(256), 0, g_gpu->ctx->stream, s, (const uint64_t *)d_q.d, m, d_out.d);
        g_gpu->launched("k_probe_sample");
        same("umap_sample", d_out.get("samples"), want);
        const Graph g = hub_graph(257, 9);
        std::vector<double> eps(g.values.size()), epns(g.values.size());
        for (size_t e = 0; e < eps.size(); e++) eps[e] = 1.0 / g.values[e], epns[e] = eps[e] / 5.0;
        GBuf<double> d_val(g.values), d_eons((uint64_t)eps.size()), d_eonns((uint64_t)eps.size());
        hipLaunchKernelGGL(k_umap_schedule, dim3(2), dim3(UMAP_WG), 0, g_gpu->ctx->stream, (const double *)d_val.d, (uint64_t)eps.size(), 1.0, 5.0, d_eons.d,
                           d_eonns.d);
        g_gpu->launched("k_umap_schedule");
        same("the schedule's start", d_eons.get("eons"), eps);
        same("the negative schedule's start", d_eonns.get("eonns"), epns);
    }
    case_done("the stream: %u words of epoch 499 modulo 2^31 - 1; the schedule's start", m);
}

// ---- the graph -----------------------------------------------------------------------------------------------------------------------
static void graph_case(uint32_t n, uint32_t k, uint32_t n_epochs, uint64_t seed) {
    Rng rng(seed);
    const uint64_t nk = (uint64_t)n * k, n2 = 2 * nk;
    std::vector<int32_t> nn(nk);
    std::vector<double> dist(nk);
    for (uint32_t i = 0; i < n; i++) {
        double d = 0.0;
        for (uint32_t m = 0; m < k; m++) {
            // row i names i + 1 .. i + k (so rows name each other in part), row 7 names the rows before it: one direction only
            nn[(size_t)i * k + m] = (int32_t)(i == 7u ? (i + n - 1u - m) % n : (i + 1u + m) % n);
            d += (i == 5u || (i == 6u && m < 2u)) ? 0.0 : 0.05 + rng.unit() * (i % 3u == 0u ? 5.0 : 0.5);  // row 5 all zeros, row 6 two leading zeros
            dist[(size_t)i * k + m] = d;
        }
    }
    // the order model
    std::vector<double> rho(n), rowsum(n), sigma(n), memb(nk);
    std::vector<uint32_t> steps(n);
    for (uint32_t i = 0; i < n; i++) {
        double s = 0.0, r = 0.0;
        for (uint32_t m = 0; m < k; m++) s += dist[(size_t)i * k + m], r = (r == 0.0 && dist[(size_t)i * k + m] > 0.0) ? dist[(size_t)i * k + m] : r;
        rho[i] = r, rowsum[i] = s;
    }
    double total = 0.0;
    for (uint32_t r0 = 0; r0 < n; r0 += GRAPH_PART_ROWS) {
        double s = 0.0;
        for (uint32_t r = r0; r < std::min(n, r0 + GRAPH_PART_ROWS); r++) s += rowsum[r];
        total += s;
    }
    const double target = std::log2((double)(k + 1u)), den_row = (double)(k + 1u), den_all = (double)n * (double)(k + 1u);
    std::vector<bool> floored(n);
    for (uint32_t i = 0; i < n; i++) {
        const double *d = &dist[(size_t)i * k];
        double lo = 0.0, hi = INFINITY, mid = 1.0;
        uint32_t st = 0;
        while (st < UMAP_MAX_STEPS) {
            double psum = 0.0;
            for (uint32_t m = 0; m < k; m++) psum += d[m] - rho[i] > 0.0 ? std::exp(-((d[m] - rho[i]) / mid)) : 1.0;
            st++;
            if (std::fabs(psum - target) < UMAP_TOL) break;
            if (psum > target) hi = mid, mid = (lo + hi) / 2.0;
            else lo = mid, mid = hi == INFINITY ? mid * 2.0 : (lo + hi) / 2.0;
        }
        const double mm = rho[i] > 0.0 ? rowsum[i] / den_row : total / den_all;
        floored[i] = mid < UMAP_FLOOR * mm;
        sigma[i] = floored[i] ? UMAP_FLOOR * mm : mid, steps[i] = st;
        for (uint32_t m = 0; m < k; m++) memb[(size_t)i * k + m] = (d[m] - rho[i] <= 0.0 || sigma[i] == 0.0) ? 1.0 : std::exp(-((d[m] - rho[i]) / sigma[i]));
    }
    if (rho[5] != 0.0 || steps[5] != 64u || !floored[5] || rho[6] != dist[6 * (size_t)k + 2]) die("the constructed rows are not what they were built to be");
    // psum and the memberships at a given sigma against long double
    auto check_ld = [&](const std::vector<double> &sg, const std::vector<uint32_t> &stp, const std::vector<double> &mb, double *worst_exp, double *worst_psum) {
        for (uint32_t i = 0; i < n; i++) {
            ld_t psum = 0.0L;
            for (uint32_t m = 0; m < k; m++) {
                const ld_t x = (ld_t)dist[(size_t)i * k + m] - (ld_t)rho[i], t = x > 0.0L ? x / (ld_t)sg[i] : 0.0L;  // x <= 0: exactly 1
                const ld_t ref = x > 0.0L ? expl(-t) : 1.0L;
                psum += ref;
                within(worst_exp, "membership", (uint64_t)i * k + m, mb[(size_t)i * k + m], ref, (double)((2.0L + 2.0L * t) * ref) * U * 1.01 + 0x1.0p-1074 + 0x1.0p-60 * (double)ref);
            }
            if (stp[i] < UMAP_MAX_STEPS && !floored[i])
                within(worst_psum, "psum at sigma", i, (double)psum, (ld_t)target, UMAP_TOL + k * (2.0 + 2.0 / 2.718281828) * U + gamma_k(k) * k + 4.0 * U * target);
        }
    };
    check_ld(sigma, steps, memb, g_host_only ? &g_worst_exp : &g_model[2], g_host_only ? &g_worst_psum : &g_model[3]);
    if (!g_host_only) {
        crgpu_ctx *ctx = g_gpu->ctx;
        GBuf<int32_t> d_nn(nn);
        GBuf<double> d_dist(dist), d_rho((uint64_t)n), d_rowsum((uint64_t)n), d_sigma((uint64_t)n), d_memb(nk), d_parts((uint64_t)1024), d_scal((uint64_t)4);
        GBuf<uint32_t> d_steps((uint64_t)n);
        const uint32_t row_grid = (n + UMAP_WG - 1u) / UMAP_WG;
        const uint64_t n_parts = (n + GRAPH_PART_ROWS - 1u) / GRAPH_PART_ROWS;
        hipLaunchKernelGGL(k_umap_rows, dim3(row_grid), dim3(UMAP_WG), 0, ctx->stream, (const double *)d_dist.d, n, k, d_rho.d, d_rowsum.d);
        hipLaunchKernelGGL(k_colparts<double>, dim3(1), dim3(GRAPH_WG), 0, ctx->stream, (const double *)d_rowsum.d, (uint64_t)n, 1u, 1u, n_parts, d_parts.d);
        hipLaunchKernelGGL(k_colfinal<double>, dim3(1), dim3(64), 0, ctx->stream, (const double *)d_parts.d, n_parts, 1u, d_scal.d);
        hipLaunchKernelGGL(k_umap_search, dim3(row_grid), dim3(UMAP_WG), 0, ctx->stream, (const double *)d_dist.d, (const double *)d_rho.d,
                           (const double *)d_rowsum.d, (const double *)d_scal.d, n, k, target, den_row, den_all, d_sigma.d, d_steps.d, d_memb.d);
        g_gpu->launched("k_umap_search");
        same("rho", d_rho.get("rho"), rho);
        same("rowsum", d_rowsum.get("rowsum"), rowsum);
        if (d_scal.get("total")[0] != total) die("the total of all distances: %.17g against %.17g", d_scal.get("total")[0], total);
        same("steps", d_steps.get("steps"), steps);
        same("sigma", d_sigma.get("sigma"), sigma);  // the decisions given, + - * / only
        const std::vector<double> dmemb = d_memb.get("memb");
        check_ld(sigma, steps, dmemb, &g_worst_exp, &g_worst_psum);
        // the union, wmax, the prune and the CSR from the device's own memberships
        GBuf<uint64_t> d_keys(n2), d_keyt(n2), d_ckeys(n2);
        GBuf<uint32_t> d_perm(n2), d_permt(n2), d_block((uint64_t)4100);
        GBuf<double> d_val(n2), d_kept(n2);
        GBuf<int32_t> d_ind(n2);
        GBuf<long long> d_ptr((uint64_t)n + 1);
        hipLaunchKernelGGL(k_pair_keys<uint32_t>, dim3(cr_grid(nk, GRAPH_WG)), dim3(GRAPH_WG), 0, ctx->stream, (const int32_t *)d_nn.d, n, k, d_keys.d, d_perm.d);
        g_gpu->launched("k_pair_keys");
        std::vector<uint64_t> keys(n2);
        for (uint64_t e = 0; e < nk; e++) keys[2 * e] = (e / k) * n + (uint32_t)nn[e], keys[2 * e + 1] = (uint64_t)(uint32_t)nn[e] * n + e / k;
        same("keys", d_keys.get("keys"), keys);
        bool in_tmp = false;
        GOK(cr_radix_sort_u64(ctx, d_keys.d, d_keyt.d, d_perm.d, d_permt.d, n2, 0, std::max(1u, cr_ceil_log2((uint64_t)n * n)), &in_tmp));
        const uint64_t *sk = in_tmp ? d_keyt.d : d_keys.d;
        uint64_t *spare = in_tmp ? d_keys.d : d_keyt.d;
        const uint32_t *sp = in_tmp ? d_permt.d : d_perm.d;
        uint32_t *d_count = d_block.d + 4096;
        GOK(compact(ctx, KeyHeadFlag{sk}, UmapEmitUnion{sk, sp, d_memb.d, n2, d_ckeys.d, d_val.d}, n2, d_block.d, d_count));
        uint32_t merged = 0;
        GOK(read_u32(ctx, d_count, &merged));
        std::map<uint64_t, std::pair<double, double>> runs;
        for (uint64_t e = 0; e < n2; e++) {
            auto it = runs.find(keys[e]);
            if (it == runs.end()) runs[keys[e]] = {dmemb[e >> 1], 0.0};
            else it->second.second = dmemb[e >> 1];
        }
        std::vector<uint64_t> ukeys, kkeys;
        std::vector<double> uval, kval;
        double wmax = 0.0;
        for (const auto &r : runs) ukeys.push_back(r.first), uval.push_back((r.second.first + r.second.second) - r.second.first * r.second.second), wmax = std::max(wmax, uval.back());
        if (merged != ukeys.size()) die("%u merged entries against %zu", merged, ukeys.size());
        std::vector<uint64_t> got_keys = d_ckeys.get("ckeys");
        std::vector<double> got_val = d_val.get("values");
        got_keys.resize(merged), got_val.resize(merged);
        same("the union's keys", got_keys, ukeys);
        same("the union's values", got_val, uval);
        const uint32_t max_grid = cr_grid(merged, UMAP_WG, 1024u);
        hipLaunchKernelGGL(k_umap_maxparts, dim3(max_grid), dim3(UMAP_WG), 0, ctx->stream, (const double *)d_val.d, (uint64_t)merged, d_parts.d);
        hipLaunchKernelGGL(k_umap_maxfinal, dim3(1), dim3(64), 0, ctx->stream, (const double *)d_parts.d, max_grid, (double)n_epochs, d_scal.d + 2);
        g_gpu->launched("k_umap_maxfinal");
        GOK(compact(ctx, UmapKeepFlag{d_val.d, d_scal.d + 2}, UmapEmitKept{d_ckeys.d, d_val.d, spare, d_kept.d}, merged, d_block.d, d_count));
        uint32_t nnz = 0;
        GOK(read_u32(ctx, d_count, &nnz));
        const std::vector<double> scal = d_scal.get("scalars");
        if (scal[2] != wmax || scal[3] != wmax / (double)n_epochs) die("wmax %.17g, the threshold %.17g against %.17g, %.17g", scal[2], scal[3], wmax, wmax / (double)n_epochs);
        for (size_t e = 0; e < ukeys.size(); e++)
            if (uval[e] >= wmax / (double)n_epochs) kkeys.push_back(ukeys[e]), kval.push_back(uval[e]);
        if (nnz != kkeys.size() || nnz == merged) die("%u kept entries of %u against %zu (the case is meant to prune)", nnz, merged, kkeys.size());
        hipLaunchKernelGGL(k_keys_to_csr<uint32_t>, dim3(cr_grid(std::max<uint64_t>(nnz, n + 1), GRAPH_WG)), dim3(GRAPH_WG), 0, ctx->stream, (const uint64_t *)spare,
                           (uint64_t)nnz, n, d_ptr.d, d_ind.d, (uint32_t *)nullptr);
        g_gpu->launched("k_keys_to_csr");
        std::vector<double> got_kept = d_kept.get("kept values");
        std::vector<int32_t> got_ind = d_ind.get("indices"), want_ind;
        got_kept.resize(nnz), got_ind.resize(nnz);
        std::vector<long long> want_ptr(n + 1, 0);
        for (uint64_t key : kkeys) want_ind.push_back((int32_t)(key % n)), want_ptr[key / n + 1]++;
        for (uint32_t i = 0; i < n; i++) want_ptr[i + 1] += want_ptr[i];
        same("the kept values", got_kept, kval);
        same("indices", got_ind, want_ind);
        same("indptr", d_ptr.get("indptr"), want_ptr);
        (void)d_keyt.get("keyt"), (void)d_perm.get("perm"), (void)d_permt.get("permt"), (void)d_block.get("block"), (void)d_nn.get("nn"), (void)d_dist.get("dist");
    }
    case_done("graph n %4u k %4u: rho, the search, the union, the prune at wmax / %u, the CSR", n, k, n_epochs);
}
static void group_graph() {
    for (uint32_t n : {63u, 64u, 65u, 255u, 257u}) graph_case(n, 3, 2, 1000 + n);
    graph_case(257, 29, 3, 2001);
    graph_case(1100, 1024, 2, 2002);
}

int main(int argc, char **argv) {
    std::string group;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--host-only")) g_host_only = true;
        else if (!std::strcmp(argv[i], "--group") && i + 1 < argc) group = argv[++i];
        else die("usage: test_umap_kernels --host-only | --group graph|epoch");
    }
    if (!g_host_only && group != "graph" && group != "epoch") die("usage: test_umap_kernels --host-only | --group graph|epoch");
    Gpu *gpu = nullptr;
    if (!g_host_only) g_gpu = gpu = new Gpu();
    if (g_host_only || group == "graph") group_graph();
    if (g_host_only || group == "epoch") group_epoch();
    std::printf("worst ratio to the bound against long double: delta %.3f, y' %.3f, a membership %.3f, psum at sigma %.3f (1e-5 is part of its bound)\n",
                g_worst_delta, g_worst_y, g_worst_exp, g_worst_psum);
    delete gpu;
    std::printf("all tests passed (%d cases)\n", g_cases);
    return 0;
}
