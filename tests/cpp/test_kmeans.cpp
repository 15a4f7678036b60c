// C++ host-mirror test of the k-means stage (include/crgpu.hpp): the Davies-Bouldin index on the host (a hand-computed case, the
// 1e-3 clamp, a zero count), the refusals, and on the device three planted groups fitted for K = 2, 3, 4 in one call: two runs agree
// bit for bit, K = 3 finds the groups, K = 3 alone equals K = 3 in the list, the first columns of a wider matrix are a view, an
// init array far from the data is relocated.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_kmeans.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_kmeans_cpp.py)
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

static void test_host_functions() {
    // two clusters 5 apart, wss 8 over 2 cells and 18 over 2 cells: scatter 2 and 3, both rows (2 + 3) / 5 = 1
    CHECK(crgpu::kmeans_db_index(2, 2, {0.0, 0.0, 3.0, 4.0}, {8.0, 18.0}, {2, 2}) == 1.0);
    // centres 1e-4 apart are taken as 1e-3 apart; a count of 0 is taken as 1: scatter 1 and 2, (1 + 2) / 1e-3
    CHECK(crgpu::kmeans_db_index(2, 1, {0.0, 1e-4}, {4.0, 4.0}, {4, 0}) == 3.0 / 1e-3);
    CHECK(crgpu::kmeans_db_index(1, 1, {7.0}, {4.0}, {4}) == 0.0);
    double s = 0.0;
    CHECK(crgpu_kmeans_db_index(0, 1, &s, &s, nullptr, &s) == CRGPU_EINVAL && crgpu_kmeans_db_index(65, 1, &s, &s, nullptr, &s) == CRGPU_EINVAL);
    double u[8];
    uint64_t first = 99;
    CHECK(crgpu_kmeans_seed_draws(0, 10, 3, u, &first) == CRGPU_OK && first == 5 && u[0] == 0.5488135039273248 && u[1] == 0.7151893663724195);
    CHECK(crgpu_kmeans_seed_draws(0, 0, 3, u, &first) == CRGPU_EINVAL && crgpu_kmeans_seed_draws(0, 10, 65, u, &first) == CRGPU_EINVAL);
    uint32_t k = 2;
    crgpu_kmeans_args a = {nullptr, 1e-4, 0, 300};
    crgpu_kmeans_result r = {};
    CHECK(crgpu_kmeans_dev(nullptr, &s, 1, 1, 1, &k, 1, &a, &r) == CRGPU_EINVAL);
}

static int refused(crgpu::Context &ctx, const std::vector<double> &x, uint64_t n, uint32_t d, uint64_t ld, const std::vector<uint32_t> &ks) {
    try {
        crgpu::kmeans(ctx, x.data(), n, d, ld, ks);
    } catch (const crgpu::Error &e) {
        return e.code;
    }
    return CRGPU_OK;
}

static void test_fit() {
    crgpu::Context ctx(0);
    // 300 cells x 3 columns: groups of 150, 100 and 50 around (0, 0), (20, 0), (0, 20) with a small seeded jitter; column 2 is noise
    const uint32_t n = 300, ld = 3;
    std::vector<double> x(n * ld);
    uint64_t s = 4242;
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t t = 0; t < ld; t++) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            const double jitter = ((double)(s >> 40) / (double)(1 << 24) - 0.5) * 2.0;
            const uint32_t g = i % 6 < 3 ? 0 : i % 6 < 5 ? 1 : 2;
            x[i * ld + t] = (t == 0 && g == 1 ? 20.0 : t == 1 && g == 2 ? 20.0 : 0.0) + (t == 2 ? 50.0 * jitter : jitter);
        }
    const auto a = crgpu::kmeans(ctx, x.data(), n, 2, ld, {2, 3, 4});
    const auto b = crgpu::kmeans(ctx, x.data(), n, 2, ld, {2, 3, 4});
    CHECK(a.size() == 3 && a[1].n_clusters == 3);
    for (size_t p = 0; p < a.size(); p++) {
        CHECK(a[p].labels == b[p].labels && a[p].clusters == b[p].clusters && a[p].centers == b[p].centers && a[p].wss == b[p].wss);
        CHECK(a[p].inertia == b[p].inertia && a[p].db_score == b[p].db_score && a[p].n_iter == b[p].n_iter && a[p].in_lds);
        uint64_t total = 0;
        for (uint64_t v : a[p].sizes) total += v;
        CHECK(total == n && a[p].n_iter >= 1 && a[p].n_iter <= 300);
    }
    const crgpu::KmeansFit &f = a[1];
    bool planted = true;
    for (uint32_t i = 0; i < n; i++) planted = planted && f.clusters[i] == (i % 6 < 3 ? 1 : i % 6 < 5 ? 2 : 3);  // by size: 150, 100, 50
    CHECK(planted && f.strict && f.relocations == 0 && f.db_score > 0.0 && f.db_score < 0.2);
    CHECK(f.db_score == crgpu::kmeans_db_index(3, 2, f.centers, f.wss, f.sizes));
    // alone or in a list; a view of the first columns or a copy of them
    const auto alone = crgpu::kmeans(ctx, x.data(), n, 2, ld, {3});
    CHECK(alone[0].labels == f.labels && alone[0].centers == f.centers && alone[0].inertia == f.inertia && alone[0].db_score == f.db_score);
    std::vector<double> x2(n * 2);
    for (uint32_t i = 0; i < n; i++) x2[i * 2] = x[i * ld], x2[i * 2 + 1] = x[i * ld + 1];
    const auto copy = crgpu::kmeans(ctx, x2.data(), n, 2, 2, {3});
    CHECK(copy[0].labels == f.labels && copy[0].centers == f.centers && copy[0].inertia == f.inertia && copy[0].wss == f.wss);
    // an init with one centre far from every point: that cluster is empty in round 1 and receives the farthest point
    const auto far = crgpu::kmeans(ctx, x2.data(), n, 2, 2, {3}, 0, {{0.0, 0.0, 20.0, 0.0, 5000.0, 5000.0}});
    CHECK(far[0].relocations == 1 && far[0].clusters == f.clusters);
    // refusals
    CHECK(refused(ctx, x2, n, 2, 2, {0}) == CRGPU_EINVAL && refused(ctx, x2, n, 2, 2, {65}) == CRGPU_EINVAL);
    CHECK(refused(ctx, x2, n, 2, 2, {3, 3}) == CRGPU_EINVAL && refused(ctx, x2, n, 2, 1, {3}) == CRGPU_EINVAL);
    CHECK(refused(ctx, x2, 2, 2, 2, {3}) == CRGPU_EINVAL && refused(ctx, x2, 2, 129, 129, {2}) == CRGPU_EINVAL);
}

int main(int argc, char **argv) {
    test_host_functions();
    if (argc < 2 || std::strcmp(argv[1], "--host-only") != 0) test_fit();
    if (g_fail) {
        std::fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("all tests passed\n");
    return 0;
}
