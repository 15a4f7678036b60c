// C++ host-mirror test of RUN_PCA (include/crgpu.hpp): the host functions without a device (the first three values of
// np.random.RandomState(0).randn, the SVD of a 2 x 2 matrix, the refusals); on the device one fixture of tests/golden/pca_reference.npz
// that tests/test_gpu_pca_cpp.py writes out as raw arrays: the feature order, it and mprod equal, d and the sign-aligned components
// within the bounds of tests/test_gpu_pca.py (16 times the reference's own movement), the same bits from a second call and under a seam.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_pca.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_pca_cpp.py)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
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

static void test_host_functions() {
    const auto r = crgpu::legacy_randn(0, 3);
    CHECK(r[0] == 1.764052345967664 && r[1] == 0.4001572083672233 && r[2] == 0.9787379841057392);
    const double B[4] = {3.0, 1.0, 0.0, 2.0};
    double U[4], s[2], Vt[4];
    CHECK(crgpu_small_svd(B, 2, U, s, Vt) == CRGPU_OK && s[0] >= s[1] && std::fabs(s[0] * s[1] - 6.0) < 1e-14);
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2; j++) CHECK(std::fabs(U[i * 2] * s[0] * Vt[j] + U[i * 2 + 1] * s[1] * Vt[2 + j] - B[i * 2 + j]) < 1e-14);
    CHECK(crgpu_small_svd(nullptr, 2, U, s, Vt) == CRGPU_EINVAL && crgpu_legacy_randn(0, 2, nullptr) == CRGPU_EINVAL);
    double out[2];
    const double mu[2] = {1.0, 2.0}, var[2] = {3.0, 2.0};
    CHECK(crgpu_normalized_dispersion(mu, var, 2, 0, out) == CRGPU_EINVAL && crgpu_normalized_dispersion(mu, var, 2, 20, out) == CRGPU_OK);
    crgpu_matrix_dev m = {4, 6, nullptr, nullptr, nullptr, nullptr};
    crgpu_pca_args a = {};
    crgpu_pca_result res = {};
    a.n_components = 2;
    CHECK(crgpu_pca_dev(nullptr, &m, 5, &a, &res) == CRGPU_EINVAL);
}

template <typename T>
static std::vector<T> slurp(const std::string &path, size_t n) {
    std::vector<T> v(n);
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "cannot read %zu values of %s\n", n, path.c_str());
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

static crgpu_matrix_dev *matrix(crgpu::Context &ctx, const std::vector<int32_t> &dense, uint32_t G, uint32_t N) {
    const uint32_t n_wl = 1024;
    U32 wl(n_wl), seen(n_wl, 0), bc, ft, ct;
    for (uint32_t i = 0; i < n_wl; i++) wl[i] = i, seen[i] = i < N ? 1u : 0u;
    ctx.check(crgpu_set_whitelist_packed(ctx.get(), 0, wl.data(), n_wl, 16, wl.data(), n_wl, nullptr));
    ctx.check(crgpu_set_counts(ctx.get(), 0, CRGPU_COUNTS_VALID, seen.data()));
    for (uint32_t c = 0; c < N; c++)
        for (uint32_t g = 0; g < G; g++)
            if (dense[(size_t)g * N + c]) bc.push_back(c), ft.push_back(g), ct.push_back((uint32_t)dense[(size_t)g * N + c]);
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

static void test_device(const std::string &dir) {
    unsigned G = 0, N = 0, nc = 0, it = 0, mprod = 0, used = 0;
    double bound_d = 0.0, bound_c = 0.0;
    FILE *f = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || std::fscanf(f, "%u %u %u %u %u %u %lf %lf", &G, &N, &nc, &it, &mprod, &used, &bound_d, &bound_c) != 8) {
        std::fprintf(stderr, "cannot read %s/meta.txt\n", dir.c_str());
        std::exit(2);
    }
    std::fclose(f);
    const auto dense = slurp<int32_t>(dir + "/dense.i32", (size_t)G * N);
    const auto features = slurp<int32_t>(dir + "/features.i32", used);
    const auto d_ref = slurp<double>(dir + "/d.f64", nc);
    const auto comp_ref = slurp<double>(dir + "/components.f64", (size_t)nc * G);
    crgpu::Context ctx(0);
    crgpu_matrix_dev *m = matrix(ctx, dense, G, N);
    const auto o = crgpu::pca(ctx, m, G, nc);
    CHECK(o.info.status == CRGPU_PCA_OK && o.info.n_components == nc && o.info.it == it && o.info.mprod == mprod && o.info.n_used_features == used);
    CHECK(o.features_selected == features && o.transformed.size() == (size_t)N * nc);
    double dmax = 0.0, cmax = 0.0, dev_d = 0.0, dev_c = 0.0;
    for (unsigned c = 0; c < nc; c++) {
        dmax = std::fmax(dmax, std::fabs(d_ref[c])), dev_d = std::fmax(dev_d, std::fabs(o.d[c] - d_ref[c]));
        double dot = 0.0, a2 = 0.0, b2 = 0.0;
        for (unsigned g = 0; g < G; g++) {
            const double a = o.components[(size_t)c * G + g], b = comp_ref[(size_t)c * G + g];
            dot += a * b, a2 += a * a, b2 += b * b;
        }
        CHECK(std::fabs(dot) / std::sqrt(a2 * b2) > 0.99);  // first: the alignment must not hide a wrong vector
        const double sign = dot < 0.0 ? -1.0 : 1.0;
        for (unsigned g = 0; g < G; g++) {
            const double b = comp_ref[(size_t)c * G + g];
            cmax = std::fmax(cmax, std::fabs(b)), dev_c = std::fmax(dev_c, std::fabs(sign * o.components[(size_t)c * G + g] - b));
        }
    }
    std::printf("d: deviation %.3g bound %.3g | components: deviation %.3g bound %.3g\n", dev_d / dmax, bound_d, dev_c / cmax, bound_c);
    CHECK(dev_d / dmax <= bound_d && dev_c / cmax <= bound_c);
    const auto again = crgpu::pca(ctx, m, G, nc), seam = crgpu::pca(ctx, m, G, nc, 0, {}, 0, CRGPU_PCA_DEFAULT_THRESHOLD, {}, 64, 5);
    CHECK(std::memcmp(again.transformed.data(), o.transformed.data(), o.transformed.size() * sizeof(double)) == 0);
    CHECK(std::memcmp(seam.transformed.data(), o.transformed.data(), o.transformed.size() * sizeof(double)) == 0 && seam.d == o.d);
    const auto start = crgpu::legacy_randn(0, used);
    const auto given = crgpu::pca(ctx, m, G, nc, 0, {}, 0, CRGPU_PCA_DEFAULT_THRESHOLD, start);
    CHECK(std::memcmp(given.components.data(), o.components.data(), o.components.size() * sizeof(double)) == 0);
    int code = CRGPU_OK;
    try {
        crgpu::pca(ctx, m, G, 0);
    } catch (const crgpu::Error &e) {
        code = e.code;
    }
    CHECK(code == CRGPU_EINVAL);
    CHECK(crgpu::pca(ctx, m, G, nc).d == o.d);  // the context is still good
    crgpu_matrix_dev_free(ctx.get(), m);
}

int main(int argc, char **argv) {
    test_host_functions();
    if (argc >= 2 && std::strcmp(argv[1], "--host-only") != 0) test_device(argv[1]);
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("all tests passed\n");
    return 0;
}
