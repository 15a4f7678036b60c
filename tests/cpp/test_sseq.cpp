// C++ host-mirror test of the sSeq differential expression (include/crgpu.hpp): Benjamini-Hochberg on the host (ties, n = 1, an
// unclipped p above 1) and the refusals without a device; on the device the two hand-computed 3 x 4 matrices of
// tests/test_sseq_restatement.py: the Poisson case (integers, p = 2 / 16 and 74 / 256, adjusted 1 / 4, both clusters equal, the class
// thresholds change no bit) and the shrinkage case (phi_mm, zeta_hat, delta, phi).
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_sseq.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_sseq_cpp.py)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "crgpu.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                      \
        }                                                                  \
    } while (0)

using U32 = std::vector<uint32_t>;
using U64 = std::vector<uint64_t>;

static void test_host_functions() {
    // ranks 1, 3, 4, 2, 5: n p / rank = 0.05, 0.0667, 0.05, 0.075, 0.5; the running minimum from the top leaves 0.05 four times
    const auto q = crgpu::sseq_adjust_bh({0.01, 0.04, 0.04, 0.03, 0.5});
    CHECK(std::fabs(q[0] - 0.05) < 1e-16 && q[1] == q[2] && std::fabs(q[1] - 0.05) < 1e-16 && std::fabs(q[3] - 0.05) < 1e-16 && q[4] == 0.5);
    CHECK(crgpu::sseq_adjust_bh({0.3}) == std::vector<double>{0.3} && crgpu::sseq_adjust_bh({}).empty());
    CHECK((crgpu::sseq_adjust_bh({1.7, 0.2}) == std::vector<double>{1.0, 0.4}));  // p is not clipped, q is
    double v = 0.0;
    CHECK(crgpu_sseq_adjust_bh(nullptr, 1, &v) == CRGPU_EINVAL && crgpu_sseq_adjust_bh(&v, 1, nullptr) == CRGPU_EINVAL);
    crgpu_matrix_dev m = {4, 6, nullptr, nullptr, nullptr, nullptr};
    crgpu_sseq_args a = {3, 0, 0, 0};
    crgpu_sseq_params *p = nullptr;
    crgpu_sseq_result r = {};
    crgpu_sseq_params_info info = {};
    const int32_t labels[4] = {1, 2, 1, 2};
    CHECK(crgpu_sseq_params_dev(nullptr, &m, &a, &p) == CRGPU_EINVAL && p == nullptr);
    CHECK(crgpu_sseq_params_get(nullptr, nullptr, &info) == CRGPU_EINVAL);
    CHECK(crgpu_sseq_diffexp_dev(nullptr, &m, nullptr, labels, 2, &a, &r) == CRGPU_EINVAL);
    crgpu_sseq_params_free(nullptr, nullptr);
}

static crgpu_matrix_dev *matrix(crgpu::Context &ctx, const std::vector<std::vector<uint32_t>> &x) {
    const uint32_t G = (uint32_t)x.size(), N = (uint32_t)x[0].size(), n_wl = 16;
    U32 wl(n_wl), seen(n_wl, 0), bc, ft, ct;
    for (uint32_t i = 0; i < n_wl; i++) wl[i] = i, seen[i] = i < N ? 1u : 0u;
    ctx.check(crgpu_set_whitelist_packed(ctx.get(), 0, wl.data(), n_wl, 16, wl.data(), n_wl, nullptr));
    ctx.check(crgpu_set_counts(ctx.get(), 0, CRGPU_COUNTS_VALID, seen.data()));
    for (uint32_t c = 0; c < N; c++)
        for (uint32_t g = 0; g < G; g++)
            if (x[g][c]) bc.push_back(c), ft.push_back(g), ct.push_back(x[g][c]);
    void *d[3];
    const U32 *h[3] = {&bc, &ft, &ct};
    for (int i = 0; i < 3; i++) {
        ctx.check(crgpu_malloc(ctx.get(), &d[i], bc.size() * sizeof(uint32_t)));
        ctx.check(crgpu_memcpy_h2d(ctx.get(), d[i], h[i]->data(), bc.size() * sizeof(uint32_t)));
    }
    crgpu_matrix_dev *m = nullptr;
    ctx.check(crgpu_assemble_matrix_dev(ctx.get(), (const uint32_t *)d[0], (const uint32_t *)d[1], (const uint32_t *)d[2], bc.size(), &m));
    for (void *p : d) crgpu_free(ctx.get(), p);
    return m;
}

static int refused(crgpu::Context &ctx, const crgpu_matrix_dev *m, const crgpu::SseqParams &p, const std::vector<int32_t> &labels, uint32_t k) {
    try {
        crgpu::sseq_diffexp(ctx, m, p, labels, k);
    } catch (const crgpu::Error &e) {
        return e.code;
    }
    return CRGPU_OK;
}

static void test_device() {
    crgpu::Context ctx(0);
    {
        // every column sums to 4: size factors 1; var = [0, 1, 1]; every phi_mm is 0: the Poisson limit, binomial terms
        crgpu_matrix_dev *m = matrix(ctx, {{1, 1, 1, 1}, {2, 0, 2, 0}, {1, 3, 1, 3}});
        CHECK(m->n_barcodes == 4);
        crgpu::SseqParams params(ctx, m, 3);
        const auto v = params.download();
        CHECK((v.size_factors == std::vector<double>{1, 1, 1, 1}) && (v.mean == std::vector<double>{1, 1, 2}) && (v.var == std::vector<double>{0, 1, 1}));
        CHECK((v.use == std::vector<uint8_t>{0, 1, 1}) && v.n_used == 2 && v.zeta_hat == 0.0 && std::isnan(v.delta) && std::isnan(v.phi[0]) && v.phi[1] == 0.0);
        const auto o = crgpu::sseq_diffexp(ctx, m, params, {1, 2, 1, 2}, 2);
        CHECK((o.sums_in == U64{2, 4, 2, 2, 0, 6}) && (o.sums_out == U64{2, 0, 6, 2, 4, 2}) && o.s_a[0] == 2.0 && o.s_b[1] == 2.0);
        CHECK((o.n_exact == U64{2, 2}) && (o.n_asymptotic == U64{0, 0}) && o.n_terms == 2 * (5 + 9) && o.n_short == 4);
        for (size_t c = 0; c < 2; c++) {
            CHECK(o.p_values[3 * c] == 1.0 && o.adjusted_p_values[3 * c] == 1.0 && o.below_median[3 * c + 1] == 255);
            CHECK(std::fabs(o.p_values[3 * c + 1] - 2.0 / 16.0) < 1e-15 && std::fabs(o.p_values[3 * c + 2] - 74.0 / 256.0) < 1e-15);
            CHECK(std::fabs(o.adjusted_p_values[3 * c + 1] - 0.25) < 1e-15 && std::fabs(o.adjusted_p_values[3 * c + 2] - 74.0 / 256.0) < 1e-15);
        }
        CHECK(o.p_values[1] == o.p_values[4] && o.p_values[2] == o.p_values[5]);  // the mirrored cluster, bit for bit
        CHECK(o.norm_mean_in[1] == 2.0 && std::fabs(o.log2_fold_change[1] - std::log2(5.0)) < 1e-15);
        const auto w = crgpu::sseq_diffexp(ctx, m, params, {1, 2, 1, 2}, 2, 1, 0xFFFFFFFFu), g = crgpu::sseq_diffexp(ctx, m, params, {1, 2, 1, 2}, 2, 1, 1);
        CHECK(w.n_wave == 4 && g.n_workgroup == 4 && w.p_values == o.p_values && g.p_values == o.p_values && g.adjusted_p_values == o.adjusted_p_values);
        CHECK(refused(ctx, m, params, {1, 1, 1, 1}, 1) == CRGPU_EINVAL && refused(ctx, m, params, {1, 2, 3, 1}, 2) == CRGPU_EINVAL);
        CHECK(refused(ctx, m, params, {1, 1, 1, 1}, 2) == CRGPU_EINVAL && refused(ctx, m, params, {0, 1, 2, 1}, 2) == CRGPU_EINVAL);
        CHECK(crgpu::sseq_diffexp(ctx, m, params, {1, 2, 1, 2}, 2).p_values == o.p_values);  // the context is still good
        crgpu_matrix_dev_free(ctx.get(), m);
    }
    {
        // every column sums to 5; phi_mm = [-, 2, 0]; zeta_hat = 1.99; delta = 1 / 3.9602
        crgpu_matrix_dev *m = matrix(ctx, {{1, 1, 1, 1}, {4, 0, 0, 0}, {0, 4, 4, 4}});
        crgpu::SseqParams params(ctx, m, 3);
        const auto v = params.download();
        const double delta = 1.0 / 3.9602;
        CHECK((v.phi_mm == std::vector<double>{0, 2, 0}) && std::fabs(v.zeta_hat - 1.99) < 1e-15 && std::fabs(v.delta - delta) < 1e-13);
        CHECK(std::isnan(v.phi[0]) && std::fabs(v.phi[1] - (2.0 - 0.01 * delta)) < 1e-13 && std::fabs(v.phi[2] - 1.99 * delta) < 1e-13);
        crgpu_matrix_dev_free(ctx.get(), m);
    }
}

int main(int argc, char **argv) {
    test_host_functions();
    if (argc < 2 || std::strcmp(argv[1], "--host-only") != 0) test_device();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("all tests passed\n");
    return 0;
}
