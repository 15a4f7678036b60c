// C++ host-mirror test of the k-nearest-neighbour stage (include/crgpu.hpp): split()'s rule and the refusals without a device; on the
// device one small fixture (300 rows, 5 of 7 columns, k = 17, two equal rows) against a brute force of its own -- d2 in dimension
// order, the pairs (d2, index) sorted, the first dropped, std::sqrt --, the three seams and a query range, all bit for bit.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_knn.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_knn_cpp.py)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
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
    CHECK(crgpu::graphclust_num_neighbors(2) == 1 && crgpu::graphclust_num_neighbors(100) == 10 && crgpu::graphclust_num_neighbors(2000) == 166);
    CHECK(crgpu::graphclust_num_neighbors(10000) == 250 && crgpu::graphclust_num_neighbors(100000) == 370 && crgpu::graphclust_num_neighbors(1000000) == 490);
    CHECK(crgpu::graphclust_num_neighbors(100, 1, 0.5, 1.0) == 2 && crgpu::graphclust_num_neighbors(100, 1, 1.5, 1.0) == 4);  // half to even
    CHECK(crgpu::graphclust_num_neighbors(10000, 300) == 300 && crgpu::graphclust_num_neighbors(50, 80) == 49);
    uint32_t k = 0;
    CHECK(crgpu_graphclust_num_neighbors(1, 1, -230.0, 120.0, &k) == CRGPU_EINVAL && crgpu_graphclust_num_neighbors(9, 1, -230.0, 120.0, nullptr) == CRGPU_EINVAL);
    const double x[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    crgpu_knn_args a = {0, 0, 0, 0, 0, 0};
    crgpu_knn_result r = {};
    CHECK(crgpu_knn_dev(nullptr, x, 8, 1, 1, 3, &a, &r) == CRGPU_EINVAL);
}

struct Brute {
    std::vector<int32_t> ind, sorted;
    std::vector<double> dist;
};
static Brute brute(const std::vector<double> &x, uint64_t n, uint32_t d, uint64_t ld, uint32_t k) {
    Brute b;
    for (uint64_t i = 0; i < n; i++) {
        std::vector<std::pair<double, int32_t>> p(n);
        for (uint64_t j = 0; j < n; j++) {
            volatile double acc = 0.0;  // a product and a sum, two roundings
            for (uint32_t t = 0; t < d; t++) {
                volatile double v = x[i * ld + t] - x[j * ld + t];
                volatile double sq = v * v;
                acc = acc + sq;
            }
            p[j] = {acc, (int32_t)j};
        }
        std::sort(p.begin(), p.end());
        std::vector<int32_t> row;
        for (uint32_t r = 1; r <= k; r++) b.ind.push_back(p[r].second), b.dist.push_back(std::sqrt(p[r].first)), row.push_back(p[r].second);
        std::sort(row.begin(), row.end());
        b.sorted.insert(b.sorted.end(), row.begin(), row.end());
    }
    return b;
}

static int refused(crgpu::Context &ctx, const std::vector<double> &x, uint64_t n, uint32_t d, uint64_t ld, uint32_t k, uint64_t q0 = 0, uint64_t nq = 0,
                   uint32_t cap = 0) {
    try {
        crgpu::knn(ctx, x.data(), n, d, ld, k, q0, nq, cap);
    } catch (const crgpu::Error &e) {
        return e.code;
    }
    return CRGPU_OK;
}

static void test_device() {
    crgpu::Context ctx(0);
    const uint64_t n = 300, ld = 7;
    const uint32_t d = 5, k = 17;
    std::vector<double> x(n * ld);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (double &v : x) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        v = (double)(s >> 11) / 9007199254740992.0 * 8.0 - 4.0;
    }
    for (uint32_t t = 0; t < d; t++) x[200 * ld + t] = x[31 * ld + t];  // row 200 = row 31 in the columns that count
    const Brute b = brute(x, n, d, ld, k);
    const crgpu::Knn o = crgpu::knn(ctx, x.data(), n, d, ld, k);
    CHECK(o.n_queries == n && o.indices == b.ind && o.sorted_indices == b.sorted);
    CHECK(o.distances.size() == b.dist.size() && std::memcmp(o.distances.data(), b.dist.data(), b.dist.size() * sizeof(double)) == 0);
    CHECK(o.indices[200 * k] == 200 && o.distances[200 * k] == 0.0 && o.indices[31 * k] == 200);  // the duplicate quirk
    CHECK(o.info.in_lds == 1 && o.info.capacity == 64 && o.info.query_tiles == 5 && o.info.pairs_evaluated == n * n && o.info.survivors >= n * (k + 1));
    // the seams move no bit: the smallest buffer, device memory, a tile of 4 candidates
    const crgpu::Knn small = crgpu::knn(ctx, x.data(), n, d, ld, k, 0, 0, k + 5), dev = crgpu::knn(ctx, x.data(), n, d, ld, k, 0, 0, 0, 1),
                     tile = crgpu::knn(ctx, x.data(), n, d, ld, k, 0, 0, 0, 0, 4);
    CHECK(small.indices == o.indices && small.distances == o.distances && small.sorted_indices == o.sorted_indices && small.info.compactions > 5);
    CHECK(dev.indices == o.indices && dev.distances == o.distances && dev.sorted_indices == o.sorted_indices && dev.info.in_lds == 0);
    CHECK(tile.indices == o.indices && tile.distances == o.distances && tile.info.cand_tile == 4);
    // a query range against the same rows of the whole
    const crgpu::Knn part = crgpu::knn(ctx, x.data(), n, d, ld, k, 100, 129);
    CHECK(part.n_queries == 129 && std::equal(part.indices.begin(), part.indices.end(), o.indices.begin() + 100 * k));
    CHECK(std::equal(part.distances.begin(), part.distances.end(), o.distances.begin() + 100 * k));
    CHECK(std::equal(part.sorted_indices.begin(), part.sorted_indices.end(), o.sorted_indices.begin() + 100 * k));
    // refusals with a live context, which stays good
    CHECK(refused(ctx, x, n, d, ld, 0) == CRGPU_EINVAL && refused(ctx, x, n, d, ld, 300) == CRGPU_EINVAL && refused(ctx, x, n, d, 4, k) == CRGPU_EINVAL);
    CHECK(refused(ctx, x, n, d, ld, k, 300, 1) == CRGPU_EINVAL && refused(ctx, x, n, d, ld, k, 0, 0, k + 4) == CRGPU_EINVAL);
    std::vector<double> bad = x;
    bad[17 * ld + 2] = std::nan("");
    CHECK(refused(ctx, bad, n, d, ld, k) == CRGPU_EINVAL);
    bad[17 * ld + 2] = x[17 * ld + 2], bad[17 * ld + 6] = INFINITY;  // beyond the d columns: not looked at
    CHECK(crgpu::knn(ctx, bad.data(), n, d, ld, k).indices == o.indices);
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
