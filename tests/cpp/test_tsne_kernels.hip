// test_tsne_kernels.hip -- the kernels of cellranger_amd/csrc/tsne.hip by direct launch into guarded buffers, at constructed shapes.
// Every f64 output of the descent has two references: an ORDER MODEL (a host loop that takes the device's steps in its order: the
// candidates of a chunk left to right, the chunk partials left to right, 256-row partials ascending, CSR entries left to right;
// both sides are unfused f64 and hold + - * / only, so the bits must agree) and a PLAIN REFERENCE in long double, from which the device
// may differ by a bound derived here:
//     a sum of n terms, each carrying r roundings of its own, whose longest path holds d additions:
//         |dev - ref| <= gamma(r + d) * sum |terms|,  gamma(k) = k u / (1 - k u), u = 2^-53   (Higham, Accuracy and Stability, 3.1)
//     plus the reference's own (n + r + 2) * 2^-64 * sum |terms|.
//     z_i:    r = 2 D + 2 (D differences, D products, D - 1 additions, 1 + d2, the division), d = min(n, CHUNK) + chunks
//     neg_it: r = 4 D + 7 (q twice, q q, the difference, the product),                        d as z
//     Z:      the error of every z_i plus d = 256 + partials
//     pos_it: r = 2 D + 6 (q, e p, (e p) q, the difference, the product),                     d = the row's entries
// exp (the conditional rows) and log (the cost) are OCML's on the device: they are compared against long double at the device's own
// beta / P / Y with a bound from OCML's documented 1 ulp (derived beside each check); the worst ratio is printed.
//
// tsne.hip is compiled here inside a namespace: the same text under the same flags (cellranger_amd.build.FLAGS), not the library's
// object code.  The context, the pool, the scan and the radix sort come from libcrgpu.so.
//
//   test_tsne_kernels --host-only                    every case without a device: the order model within the bound of the reference
//   test_tsne_kernels --group repulse|attract|affinities
// One line per case, "all tests passed" at the end; the first mismatch or HIP error ends the program with status 1.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "graph_common.h"
#include "kernel_test.h"

namespace tsne_under_test {
#include "tsne.hip"
}
using namespace tsne_under_test;

typedef long double ld_t;
static const uint32_t CH = CRGPU_TSNE_CAND_CHUNK, PR = GRAPH_PART_ROWS;
static double g_worst = 0.0, g_worst_exp = 0.0, g_worst_log = 0.0;
static void within(const char *what, uint64_t at, double got, ld_t ref, double bound) {
    const double dev = (double)fabsl((ld_t)got - ref);
    if (!(dev <= bound)) die("%s[%llu]: %.17g against %.21Lg, off by %.3g, bound %.3g", what, (unsigned long long)at, got, ref, dev, bound);
    if (bound > 0.0) g_worst = std::max(g_worst, dev / bound);
}
enum YKind { Y_NORMAL = 0, Y_DECADES = 1, Y_COINCIDENT = 2 };
static const char *Y_NAMES[3] = {"normal", "twelve decades", "coincident rows"};
static std::vector<double> make_y(uint32_t n, uint32_t D, YKind kind, uint64_t seed) {
    Rng rng(seed);
    std::vector<double> y((size_t)n * D);
    for (uint32_t i = 0; i < n; i++) {
        const double scale = kind == Y_DECADES ? std::pow(10.0, (double)(int)(i % 13u) - 6.0) : 3.0;
        for (uint32_t t = 0; t < D; t++) y[(size_t)i * D + t] = rng.normal() * scale;
    }
    if (kind == Y_COINCIDENT)
        for (uint32_t i = 1; i < n; i += 3)
            for (uint32_t t = 0; t < D; t++) y[(size_t)i * D + t] = y[(size_t)(i - 1) * D + t];  // q = 1 for the pair
    return y;
}

// ---- the order model -----------------------------------------------------------------------------------------------------------------
static double model_colsum(const std::vector<double> &a, uint64_t n, uint32_t ld, uint32_t c) {
    double total = 0.0;
    for (uint64_t r0 = 0; r0 < n; r0 += PR) {
        double s = 0.0;
        for (uint64_t r = r0; r < std::min<uint64_t>(n, r0 + PR); r++) s += a[r * ld + c];
        total += s;
    }
    return total;
}
// rep[i * (D + 1)] = z_i, then neg_i[D]
static std::vector<double> model_repulse(const std::vector<double> &y, uint32_t n, uint32_t D) {
    std::vector<double> rep((size_t)n * (D + 1), 0.0);
    for (uint32_t i = 0; i < n; i++) {
        double z = 0.0, neg[3] = {0.0, 0.0, 0.0};
        for (uint32_t c0 = 0; c0 < n; c0 += CH) {
            double pz = 0.0, pn[3] = {0.0, 0.0, 0.0};
            for (uint32_t j = c0; j < std::min(n, c0 + CH); j++) {
                if (j == i) continue;
                double v[3], d2 = 0.0;
                for (uint32_t t = 0; t < D; t++) v[t] = y[(size_t)i * D + t] - y[(size_t)j * D + t], d2 += v[t] * v[t];
                const double q = 1.0 / (1.0 + d2), qq = q * q;
                pz += q;
                for (uint32_t t = 0; t < D; t++) pn[t] += qq * v[t];
            }
            z += pz;
            for (uint32_t t = 0; t < D; t++) neg[t] += pn[t];
        }
        rep[(size_t)i * (D + 1)] = z;
        for (uint32_t t = 0; t < D; t++) rep[(size_t)i * (D + 1) + 1 + t] = neg[t];
    }
    return rep;
}
// the plain reference of the repulsion and the check of a rep against it; returns the bound of Z
static void check_repulse_ld(const std::vector<double> &y, uint32_t n, uint32_t D, const std::vector<double> &rep, double Z) {
    const double path = (double)std::min(n, CH) + (double)((n + CH - 1) / CH);
    ld_t Zr = 0.0L;
    double Zb = 0.0;
    for (uint32_t i = 0; i < n; i++) {
        ld_t z = 0.0L, neg[3] = {0.0L, 0.0L, 0.0L}, an[3] = {0.0L, 0.0L, 0.0L};
        for (uint32_t j = 0; j < n; j++) {
            if (j == i) continue;
            ld_t v[3], d2 = 0.0L;
            for (uint32_t t = 0; t < D; t++) v[t] = (ld_t)y[(size_t)i * D + t] - (ld_t)y[(size_t)j * D + t], d2 += v[t] * v[t];
            const ld_t q = 1.0L / (1.0L + d2);
            z += q;
            for (uint32_t t = 0; t < D; t++) neg[t] += q * q * v[t], an[t] += fabsl(q * q * v[t]);
        }
        const double own = ((double)n + 4.0 * D + 9.0) * 0x1.0p-64;
        const double zb = (gamma_k(2.0 * D + 2.0 + path) + own) * (double)z;
        within("z", i, rep[(size_t)i * (D + 1)], z, zb);
        for (uint32_t t = 0; t < D; t++) within("neg", (uint64_t)i * D + t, rep[(size_t)i * (D + 1) + 1 + t], neg[t], (gamma_k(4.0 * D + 7.0 + path) + own) * (double)an[t]);
        Zr += z, Zb += zb;
    }
    within("Z", 0, Z, Zr, Zb + (gamma_k((double)PR + (double)((n + PR - 1) / PR)) + ((double)n + 2.0) * 0x1.0p-64) * (double)Zr);
}

struct Csr {
    uint32_t n;
    std::vector<long long> indptr;
    std::vector<int32_t> indices;
    std::vector<double> values;
};
// row 0 is a hub every row names and that names K rows itself (n - 1 entries at the least), the others hold about K; the row `mid`
// gets exactly thr - 1 and mid + 1 exactly thr entries when thr > 0, so that the two straddle a wave threshold of thr
static Csr make_csr(uint32_t n, uint32_t K, uint32_t thr, uint64_t seed) {
    Rng rng(seed);
    std::vector<std::vector<int32_t>> rows(n);
    for (uint32_t i = 1; i < n; i++) rows[i].push_back(0), rows[0].push_back((int32_t)i);
    const uint32_t mid = n / 2;
    for (uint32_t i = 1; i < n; i++) {
        uint32_t want = std::min(K, n - 2u);
        if (thr && i == mid) want = thr - 1u;
        if (thr && i == mid + 1u) want = thr;
        for (uint32_t m = 1; rows[i].size() < want && m < n; m++) {
            const uint32_t j = (i + m * 7u) % n;      // 7 and n need not be coprime: a repeat is skipped
            if (j != i && std::find(rows[i].begin(), rows[i].end(), (int32_t)j) == rows[i].end()) rows[i].push_back((int32_t)j);
        }
    }
    Csr c;
    c.n = n, c.indptr.assign(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) {
        std::sort(rows[i].begin(), rows[i].end());
        for (int32_t j : rows[i]) c.indices.push_back(j), c.values.push_back(rng.unit() / (double)n);
        c.indptr[i + 1] = (long long)c.indices.size();
    }
    return c;
}
static std::vector<double> model_pos(const Csr &c, const std::vector<double> &y, uint32_t D, double e) {
    std::vector<double> pos((size_t)c.n * D, 0.0);
    for (uint32_t i = 0; i < c.n; i++)
        for (long long k = c.indptr[i]; k < c.indptr[i + 1]; k++) {
            const uint32_t j = (uint32_t)c.indices[k];
            double v[3], d2 = 0.0;
            for (uint32_t t = 0; t < D; t++) v[t] = y[(size_t)i * D + t] - y[(size_t)j * D + t], d2 += v[t] * v[t];
            const double w = (e * c.values[k]) * (1.0 / (1.0 + d2));
            for (uint32_t t = 0; t < D; t++) pos[(size_t)i * D + t] += w * v[t];
        }
    return pos;
}
static void check_pos_ld(const Csr &c, const std::vector<double> &y, uint32_t D, double e, const std::vector<double> &pos) {
    for (uint32_t i = 0; i < c.n; i++) {
        ld_t p[3] = {0.0L, 0.0L, 0.0L}, ap[3] = {0.0L, 0.0L, 0.0L};
        for (long long k = c.indptr[i]; k < c.indptr[i + 1]; k++) {
            const uint32_t j = (uint32_t)c.indices[k];
            ld_t v[3], d2 = 0.0L;
            for (uint32_t t = 0; t < D; t++) v[t] = (ld_t)y[(size_t)i * D + t] - (ld_t)y[(size_t)j * D + t], d2 += v[t] * v[t];
            const ld_t w = (ld_t)e * (ld_t)c.values[k] / (1.0L + d2);
            for (uint32_t t = 0; t < D; t++) p[t] += w * v[t], ap[t] += fabsl(w * v[t]);
        }
        const double len = (double)(c.indptr[i + 1] - c.indptr[i]);
        for (uint32_t t = 0; t < D; t++)
            within("pos", (uint64_t)i * D + t, pos[(size_t)i * D + t], p[t], (gamma_k(2.0 * D + 6.0 + len) + (len + 2.0 * D + 8.0) * 0x1.0p-64) * (double)ap[t]);
    }
}
static int sgn(double x) { return x > 0.0 ? 1 : (x < 0.0 ? -1 : 0); }

// ---- group repulse -------------------------------------------------------------------------------------------------------------------
template <uint32_t D>
static void repulse_case(uint32_t n, YKind kind, bool reference) {
    const std::vector<double> y = make_y(n, D, kind, 77u + n + D);
    const std::vector<double> rep = model_repulse(y, n, D);
    const double Z = model_colsum(rep, n, D + 1u, 0u);
    if (reference) check_repulse_ld(y, n, D, rep, Z);
    if (!g_host_only) {
        const uint32_t n_chunks = (n + CH - 1u) / CH;
        const uint32_t seams[4][3] = {{64u, 512u, 0u}, {128u, n > CH ? 3u : 1u, 128u}, {256u, 1024u, 256u}, {64u, 333u, 64u}};  // row tile, cand tile, slab rows
        GBuf<double> d_y(y);
        for (const auto &s : seams) {
            const uint32_t R = s[0], T = s[1], S = s[2] ? s[2] : (n + R - 1u) / R * R;
            GBuf<double> d_slab((uint64_t)S * n_chunks * (D + 1u)), d_rep((uint64_t)n * (D + 1u)), d_parts((uint64_t)(n + PR - 1u) / PR), d_z(1);
            for (uint32_t row0 = 0; row0 < n; row0 += S) {
                const uint32_t rows = std::min(S, n - row0), n_tiles = (rows + R - 1u) / R;
                hipLaunchKernelGGL(k_tsne_repulse<D>, dim3(n_tiles * n_chunks), dim3(R), (size_t)T * D * sizeof(double), g_gpu->ctx->stream, d_y.d, n, row0, rows,
                                   n_tiles, T, d_slab.d);
                hipLaunchKernelGGL(k_tsne_finish, dim3(cr_grid((uint64_t)rows * (D + 1u), TSNE_WG)), dim3(TSNE_WG), 0, g_gpu->ctx->stream, d_slab.d, row0, rows,
                                   n_chunks, D + 1u, d_rep.d);
            }
            cr_colsums(g_gpu->ctx, d_rep.d, n, D + 1u, 1u, d_parts.d, d_z.d);
            g_gpu->launched("k_tsne_repulse");
            (void)d_slab.get("slab");  // only the guard: slots of a last, shorter group keep their fill
            same("rep", d_rep.get("rep"), rep);
            same("Z", d_z.get("Z"), std::vector<double>(1, Z));
            (void)d_parts.get("parts");
        }
    }
    case_done("repulse n = %u, dims %u, %s%s", n, D, Y_NAMES[kind], reference ? "" : " (order model only)");
}
static void group_repulse() {
    const uint32_t sizes[] = {63u, 64u, 65u, 127u, 128u, 129u, 255u, 256u, 257u, CH - 1u, CH, CH + 1u, 2u * CH + 1u};
    for (uint32_t n : sizes) {
        const YKind kind = (YKind)(n % 3u);
        const bool reference = n <= CH + 1u;      // the long double pass over 2 CH + 1 rows would double the group's time
        if (n & 1u) repulse_case<2>(n, kind, reference), repulse_case<3>(n, (YKind)((n + 1u) % 3u), reference && n < CH);
        else repulse_case<3>(n, kind, reference), repulse_case<2>(n, (YKind)((n + 1u) % 3u), reference && n < CH);
    }
}

// ---- group attract -------------------------------------------------------------------------------------------------------------------
template <uint32_t D>
static void attract_case(uint32_t n, uint32_t K, uint32_t thr, YKind kind) {
    const Csr c = make_csr(n, K, thr, 5u + n);
    const std::vector<double> y = make_y(n, D, kind, 99u + n);
    const double e = 12.0, mom = 0.5, eta = 200.0;
    const std::vector<double> rep = model_repulse(y, n, D), pos = model_pos(c, y, D, e);
    const double Z = model_colsum(rep, n, D + 1u, 0u);
    check_pos_ld(c, y, D, e, pos);
    // the update and the centring in the order model
    Rng rng(3u + n);
    std::vector<double> uY((size_t)n * D), gains((size_t)n * D), grad((size_t)n * D), ynew((size_t)n * D), yc((size_t)n * D);
    for (size_t k = 0; k < uY.size(); k++) uY[k] = (k % 5u == 0u) ? 0.0 : rng.normal() * 1e-3, gains[k] = (k % 7u == 0u) ? 0.011 : 0.5 + rng.unit();
    std::vector<double> uY2 = uY, gains2 = gains;
    for (size_t k = 0; k < grad.size(); k++) {
        const size_t i = k / D, t = k % D;
        const double dC = pos[k] - rep[i * (D + 1u) + 1u + t] / Z;
        grad[k] = dC;
        double g = sgn(dC) != sgn(uY[k]) ? gains[k] + 0.2 : gains[k] * 0.8;
        g = g < 0.01 ? 0.01 : g;
        gains2[k] = g, uY2[k] = (mom * uY[k]) - ((eta * g) * dC), ynew[k] = y[k] + uY2[k];
    }
    for (uint32_t t = 0; t < D; t++) {
        const double s = model_colsum(ynew, n, D, t);
        for (uint32_t i = 0; i < n; i++) yc[(size_t)i * D + t] = ynew[(size_t)i * D + t] - s / (double)n;
    }
    if (!g_host_only) {
        GBuf<long long> d_ptr(c.indptr);
        GBuf<int32_t> d_ind(c.indices);
        GBuf<double> d_val(c.values), d_y(y), d_rep(rep), d_z(std::vector<double>(1, Z));
        std::vector<double> first_grad;
        for (uint32_t w : {thr ? thr : 32u, 1u, 0x40000000u, thr ? thr + 1u : 5u}) {
            GBuf<double> d_uY(uY), d_gains(gains), d_ynew((uint64_t)n * D), d_grad((uint64_t)n * D), d_parts((uint64_t)((n + PR - 1u) / PR) * D), d_sums(D), d_yc((uint64_t)n * D);
            for (uint32_t update = 0; update < 2u; update++) {
                TsneStep st = {e, mom, eta, n, w, update};
                hipLaunchKernelGGL((k_tsne_attract<D, false>), dim3(cr_grid(n, TSNE_WG)), dim3(TSNE_WG), 0, g_gpu->ctx->stream, d_ptr.d, d_ind.d, d_val.d, d_y.d, d_rep.d,
                                   d_z.d, st, d_uY.d, d_gains.d, d_ynew.d, d_grad.d);
                hipLaunchKernelGGL((k_tsne_attract<D, true>), dim3(cr_grid((uint64_t)n * 64u, TSNE_WG)), dim3(TSNE_WG), 0, g_gpu->ctx->stream, d_ptr.d, d_ind.d, d_val.d,
                                   d_y.d, d_rep.d, d_z.d, st, d_uY.d, d_gains.d, d_ynew.d, d_grad.d);
            }
            cr_colsums(g_gpu->ctx, d_ynew.d, n, D, D, d_parts.d, d_sums.d);
            hipLaunchKernelGGL(k_tsne_centre, dim3(cr_grid((uint64_t)n * D, TSNE_WG)), dim3(TSNE_WG), 0, g_gpu->ctx->stream, d_ynew.d, (uint64_t)n, D, d_sums.d, d_yc.d);
            g_gpu->launched("k_tsne_attract");
            same("grad", d_grad.get("grad"), grad);
            same("gains", d_gains.get("gains"), gains2);
            same("uY", d_uY.get("uY"), uY2);
            same("Ynew", d_ynew.get("Ynew"), ynew);
            same("Y centred", d_yc.get("Y"), yc);
        }
        // the cost at the device's own P, Y and Z against long double.  r = (p + m) / (q / Z + m) carries 2 D + 6 roundings; log(r) is
        // off by that relative error of r absolutely, plus OCML's 1 ulp = 2^-52 of itself, plus the product's rounding; the row's sum
        // and the 256-row partials add gamma(entries + 256 + partials) of the sum of |terms|
        GBuf<double> d_rowkl(n), d_parts((n + PR - 1u) / PR), d_kl(1);
        hipLaunchKernelGGL(k_tsne_kl<D>, dim3(cr_grid(n, TSNE_WG)), dim3(TSNE_WG), 0, g_gpu->ctx->stream, d_ptr.d, d_ind.d, d_val.d, d_y.d, d_z.d, n, d_rowkl.d);
        cr_colsums(g_gpu->ctx, d_rowkl.d, n, 1u, 1u, d_parts.d, d_kl.d);
        g_gpu->launched("k_tsne_kl");
        const double kl = d_kl.get("kl")[0];
        ld_t ref = 0.0L;
        double bound = 0.0, longest = 0.0;
        for (uint32_t i = 0; i < n; i++) {
            longest = std::max(longest, (double)(c.indptr[i + 1] - c.indptr[i]));
            for (long long k = c.indptr[i]; k < c.indptr[i + 1]; k++) {
                const uint32_t j = (uint32_t)c.indices[k];
                ld_t d2 = 0.0L;
                for (uint32_t t = 0; t < D; t++) {
                    const ld_t v = (ld_t)y[(size_t)i * D + t] - (ld_t)y[(size_t)j * D + t];
                    d2 += v * v;
                }
                const ld_t p = c.values[k], term = p * logl((p + (ld_t)FLT_MIN) / (1.0L / (1.0L + d2) / (ld_t)Z + (ld_t)FLT_MIN));
                ref += term;
                bound += (double)p * (2.0 * D + 7.0) * U + 3.0 * U * (double)fabsl(term);
            }
        }
        ld_t abs_sum = 0.0L;  // the sum of |terms| is at most what the terms' own bound was built from: take it from there
        abs_sum = (ld_t)(bound / (3.0 * U));
        bound += gamma_k(longest + (double)PR + (double)((n + PR - 1u) / PR)) * (double)abs_sum;
        const double dev = (double)fabsl((ld_t)kl - ref);
        if (!(dev <= bound)) die("kl: %.17g against %.21Lg, off by %.3g, bound %.3g", kl, ref, dev, bound);
        g_worst_log = std::max(g_worst_log, dev / bound);
    }
    case_done("attract n = %u, dims %u, K = %u, hub of %lld entries, threshold %u, %s", n, D, K, c.indptr[1], thr, Y_NAMES[kind]);
}
static void group_attract() {
    attract_case<2>(65u, 3u, 0u, Y_NORMAL);
    attract_case<3>(129u, 90u, 64u, Y_DECADES);
    attract_case<2>(257u, 90u, 33u, Y_COINCIDENT);
    attract_case<3>(1200u, 1024u, 100u, Y_NORMAL);
    attract_case<2>(CH + 1u, 90u, 32u, Y_DECADES);
}

// ---- group affinities ----------------------------------------------------------------------------------------------------------------
static void affinities_case(uint32_t n, uint32_t k, double perplexity, uint64_t seed) {
    if (g_host_only) return case_done("affinities n = %u, K = %u: exp and the sort run on the device only", n, k);
    Rng rng(seed);
    std::vector<int32_t> nn((size_t)n * k);
    std::vector<double> dist((size_t)n * k);
    for (uint32_t i = 0; i < n; i++) {
        double d = 0.05 + rng.unit();
        for (uint32_t m = 0; m < k; m++) nn[(size_t)i * k + m] = (int32_t)((i + 1u + m) % n), dist[(size_t)i * k + m] = (d += 0.02 * rng.unit() * (1.0 + 0.01 * m));
    }
    for (uint32_t m = 0; m < k; m++) dist[(size_t)1 * k + m] = 0.0;      // a row of zeros: 200 steps, uniform
    GBuf<int32_t> d_nn(nn);
    GBuf<double> d_dist(dist), d_beta(n), d_cond((uint64_t)n * k);
    GBuf<uint32_t> d_steps(n);
    const double log_perp = std::log(perplexity);
    hipLaunchKernelGGL(k_tsne_search, dim3((n + TSNE_WG - 1u) / TSNE_WG), dim3(TSNE_WG), 0, g_gpu->ctx->stream, d_dist.d, n, k, log_perp, d_beta.d, d_steps.d, d_cond.d);
    g_gpu->launched("k_tsne_search");
    const std::vector<double> beta = d_beta.get("beta"), cond = d_cond.get("cond");
    const std::vector<uint32_t> steps = d_steps.get("steps");
    for (uint32_t i = 0; i < n; i++) {
        // at the device's own beta: bd_m is one product (u relative, which moves exp by bd_m u); OCML's exp 1 ulp = 2 u; s adds k such
        // terms (the largest of those errors) with k roundings; the division u
        std::vector<ld_t> bd(k), p(k);
        ld_t s = (ld_t)DBL_MIN, h = 0.0L, top = 0.0L;
        for (uint32_t m = 0; m < k; m++) {
            const double d2 = dist[(size_t)i * k + m] * dist[(size_t)i * k + m];
            bd[m] = (ld_t)beta[i] * (ld_t)d2, p[m] = expl(-bd[m]), s += p[m], h += bd[m] * p[m], top = std::max(top, bd[m]);
        }
        if (steps[i] < 1u || steps[i] > TSNE_MAX_STEPS) die("row %u took %u steps", i, steps[i]);
        if (steps[i] < TSNE_MAX_STEPS && !(fabsl(h / s + logl(s) - (ld_t)log_perp) < 1e-5L + 1e-9L)) die("row %u: the entropy at its beta is %.3Lg off", i, h / s + logl(s) - (ld_t)log_perp);
        if (i == 1u && (steps[i] != TSNE_MAX_STEPS || cond[(size_t)k] != 1.0 / (DBL_MIN + (double)k))) die("the row of zeros: %u steps, p = %.17g", steps[i], cond[(size_t)k]);
        for (uint32_t m = 0; m < k; m++) {
            const ld_t want = p[m] / s;
            // exp(-bd_m) itself below the normal range (bd_m > 693) is rounded to a denormal, with as few bits as are left: no
            // relative statement there, whatever the size of the quotient; s above 2^-960 is untouched by such terms
            if (p[m] < 0x1.0p-1000L || s < 0x1.0p-960L) continue;
            const double bound = ((double)bd[m] + (double)top + 2.0 + 2.0 + (double)k + 1.0) * U, rel = (double)(fabsl((ld_t)cond[(size_t)i * k + m] - want) / want);
            if (!(rel <= bound)) die("p[%u, %u]: %.17g against %.21Lg, %.3g relative, bound %.3g", i, m, cond[(size_t)i * k + m], want, rel, bound);
            g_worst_exp = std::max(g_worst_exp, rel / bound);
        }
    }
    // the keys, the library's sort, the merge and the row pointers against a host merge of the same conditional rows
    const uint64_t nk = (uint64_t)n * k, n2 = 2u * nk;
    GBuf<uint64_t> d_keys(n2), d_keyt(n2), d_ckeys(n2);
    GBuf<uint32_t> d_perm(n2), d_permt(n2), d_block(4100);
    GBuf<double> d_val(n2);
    GBuf<int32_t> d_ind(n2);
    GBuf<long long> d_ptr(n + 1u);
    hipLaunchKernelGGL(k_pair_keys<uint32_t>, dim3(cr_grid(nk, GRAPH_WG)), dim3(GRAPH_WG), 0, g_gpu->ctx->stream, d_nn.d, n, k, d_keys.d, d_perm.d);
    bool in_tmp = false;
    GOK(cr_radix_sort_u64(g_gpu->ctx, d_keys.d, d_keyt.d, d_perm.d, d_permt.d, n2, 0, std::max(1u, cr_ceil_log2((uint64_t)n * n)), &in_tmp));
    const uint64_t *sk = in_tmp ? d_keyt.d : d_keys.d;
    const uint32_t *sp = in_tmp ? d_permt.d : d_perm.d;
    GOK(compact(g_gpu->ctx, KeyHeadFlag{sk}, TsneEmitMerged{sk, sp, d_cond.d, n2, d_ckeys.d, d_val.d}, n2, d_block.d, d_block.d + 4096));
    uint32_t nnz = 0;
    GOK(read_u32(g_gpu->ctx, d_block.d + 4096, &nnz));
    hipLaunchKernelGGL(k_keys_to_csr<uint32_t>, dim3(cr_grid(std::max<uint64_t>(nnz, n + 1u), GRAPH_WG)), dim3(GRAPH_WG), 0, g_gpu->ctx->stream, d_ckeys.d, (uint64_t)nnz, n, d_ptr.d,
                       d_ind.d, (uint32_t *)nullptr);
    g_gpu->launched("k_keys_to_csr");
    std::vector<std::pair<uint64_t, double>> pairs;
    for (uint64_t e = 0; e < nk; e++) {
        const uint64_t i = e / k, j = (uint64_t)nn[e];
        pairs.push_back({i * n + j, cond[e]}), pairs.push_back({j * n + i, cond[e]});
    }
    std::sort(pairs.begin(), pairs.end());
    std::vector<long long> ptr(n + 1u, 0);
    std::vector<int32_t> ind;
    std::vector<double> val;
    for (size_t a = 0; a < pairs.size();) {
        size_t b = a + 1;
        while (b < pairs.size() && pairs[b].first == pairs[a].first) b++;
        if (b - a > 2) die("a key %zu times", b - a);
        ind.push_back((int32_t)(pairs[a].first % n)), val.push_back((pairs[a].second + (b - a == 2 ? pairs[a + 1].second : 0.0)) / 2.0);
        ptr[pairs[a].first / n + 1]++;
        a = b;
    }
    for (uint32_t i = 0; i < n; i++) ptr[i + 1] += ptr[i];
    if (nnz != ind.size()) die("%u merged entries against %zu", nnz, ind.size());
    std::vector<int32_t> got_ind = d_ind.get("indices");
    std::vector<double> got_val = d_val.get("values");
    got_ind.resize(nnz), got_val.resize(nnz);
    if (got_ind != ind || d_ptr.get("indptr") != ptr) die("the CSR structure differs");
    same("merged values", got_val, val);
    // the normalisation: the total in the stated order, then the division
    GBuf<double> d_parts((nnz + PR - 1u) / PR), d_total(1);
    cr_colsums(g_gpu->ctx, d_val.d, nnz, 1u, 1u, d_parts.d, d_total.d);
    hipLaunchKernelGGL(k_tsne_divide, dim3(cr_grid(nnz, TSNE_WG)), dim3(TSNE_WG), 0, g_gpu->ctx->stream, d_val.d, (uint64_t)nnz, d_total.d);
    g_gpu->launched("k_tsne_divide");
    const double total = model_colsum(val, nnz, 1u, 0u);
    same("total", d_total.get("total"), std::vector<double>(1, total));
    for (double &v : val) v = v / total;
    got_val = d_val.get("values");
    got_val.resize(nnz);
    same("values", got_val, val);
    case_done("affinities n = %u, K = %u, perplexity %g: %u entries, a row of zeros", n, k, perplexity, nnz);
}
static void group_affinities() {
    affinities_case(65u, 3u, 1.0, 11u);
    affinities_case(300u, 90u, 30.0, 12u);
    affinities_case(1100u, 1024u, 341.5, 13u);
}

int main(int argc, char **argv) {
    std::string group;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--host-only")) g_host_only = true;
        else if (!std::strcmp(argv[i], "--group") && i + 1 < argc) group = argv[++i];
        else die("usage: test_tsne_kernels --host-only | --group repulse|attract|affinities");
    }
    if (g_host_only == !group.empty()) die("one of --host-only and --group");
    Gpu *gpu = nullptr;
    if (!g_host_only) g_gpu = gpu = new Gpu();
    if (g_host_only || group == "repulse") group_repulse();
    if (g_host_only || group == "attract") group_attract();
    if (g_host_only || group == "affinities") group_affinities();
    delete gpu;
    if (!g_cases) die("no group %s", group.c_str());
    std::printf("worst deviation to bound: sums %.3f, exp %.3f, log %.3f\n", g_worst, g_worst_exp, g_worst_log);
    std::printf("%d cases, all tests passed\n", g_cases);
    return 0;
}
