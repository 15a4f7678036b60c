// C++ host-mirror test of CORRECT_CHEMISTRY_BATCH (include/crgpu.hpp): crgpu_mnn_pairs against a brute force over std::set and the
// refusals without a device; on the device two batches (150 + 110 rows, 6 of 8 columns, k = 7): knn_cross against a brute force of its
// own -- d2 in dimension order, the pairs (d2, index) sorted, NOTHING dropped, std::sqrt -- bit for bit, the mutual pairs, and one
// correction step whose corr must lie within 1e-12 of a long double evaluation, bit-identical under the seams and for a sub-list.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_batch_correction.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_batch_correction_cpp.py)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
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

static uint64_t g_s = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
    g_s = g_s * 6364136223846793005ull + 1442695040888963407ull;
    return g_s >> 11;
}

static std::vector<int32_t> brute_mnn(const std::vector<int32_t> &a, uint64_t start_i, const std::vector<int32_t> &b, uint64_t start_j, uint32_t k) {
    std::set<std::pair<int32_t, int32_t>> ij, ji;
    for (size_t e = 0; e < a.size(); e++) ij.insert({(int32_t)(start_i + e / k), a[e]});
    for (size_t e = 0; e < b.size(); e++) ji.insert({b[e], (int32_t)(start_j + e / k)});
    std::vector<int32_t> out;
    for (const auto &p : ij)
        if (ji.count(p)) out.push_back(p.first), out.push_back(p.second);
    return out;
}

static void test_host_functions() {
    const uint32_t k = 4;
    const uint64_t n_i = 50, n_j = 35, start_i = 20, start_j = 70;
    std::vector<int32_t> a(n_i * k), b(n_j * k);
    for (auto &v : a) v = (int32_t)(start_j + next_u64() % n_j);  // with repeats inside a row: the pairs are a set
    for (auto &v : b) v = (int32_t)(start_i + next_u64() % n_i);
    const crgpu::MnnPairs m = crgpu::mnn_pairs(a, start_i, b, start_j, k);
    const std::vector<int32_t> want = brute_mnn(a, start_i, b, start_j, k);
    CHECK(!want.empty() && m.pairs == want);
    std::set<int32_t> first, second;
    for (size_t e = 0; e < want.size(); e += 2) first.insert(want[e]), second.insert(want[e + 1]);
    CHECK(m.n_first == first.size() && m.n_second == second.size());
    uint64_t n = 0, n1 = 0, n2 = 0;
    a[3] = (int32_t)(start_j + n_j);  // outside batch j
    CHECK(crgpu_mnn_pairs(a.data(), n_i, start_i, b.data(), n_j, start_j, k, nullptr, 0, &n, &n1, &n2) == CRGPU_EINVAL);
    CHECK(crgpu_mnn_pairs(nullptr, n_i, start_i, b.data(), n_j, start_j, k, nullptr, 0, &n, &n1, &n2) == CRGPU_EINVAL);
    const double x[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    crgpu_knn_cross_args ca = {0, 4, 4, 4, 0, 0, 0, 0};
    crgpu_knn_result r = {};
    CHECK(crgpu_knn_cross_dev(nullptr, x, 8, 1, 1, 3, &ca, &r) == CRGPU_EINVAL);
    const int32_t cur[2] = {0, 1}, mc[1] = {0}, mr[1] = {5};
    double out[8];
    crgpu_bc_step st = {cur, mc, mr, nullptr, 2, 1};
    crgpu_bc_args ba = {0, 0, 0, 0};
    crgpu_bc_result br = {};
    CHECK(crgpu_batch_correct_dev(nullptr, x, 8, 1, 1, 150.0, &st, 1, out, &ba, &br) == CRGPU_EINVAL);
}

static int refused(crgpu::Context &ctx, const std::vector<double> &x, uint64_t n, uint32_t d, uint64_t ld, double sigma, const std::vector<crgpu::BcStep> &steps,
                   uint32_t pair_tile = 0, uint32_t row_tile = 0) {
    try {
        crgpu::batch_correct(ctx, x.data(), n, d, ld, sigma, steps, false, pair_tile, row_tile);
    } catch (const crgpu::Error &e) {
        return e.code;
    }
    return CRGPU_OK;
}

static void test_device() {
    crgpu::Context ctx(0);
    const uint64_t n_i = 150, n_j = 110, n = n_i + n_j, ld = 8;
    const uint32_t d = 6, k = 7;
    std::vector<double> x(n * ld);
    for (double &v : x) v = (double)next_u64() / 9007199254740992.0 * 0.6 - 0.3;
    // find_knn in both directions against a brute force
    std::vector<int32_t> nn[2];
    for (int dir = 0; dir < 2; dir++) {
        const uint64_t q0 = dir ? n_i : 0, nq = dir ? n_j : n_i, c0 = dir ? 0 : n_i, nc = dir ? n_i : n_j;
        std::vector<int32_t> ind;
        std::vector<double> dist;
        for (uint64_t i = q0; i < q0 + nq; i++) {
            std::vector<std::pair<double, int32_t>> p(nc);
            for (uint64_t j = 0; j < nc; j++) {
                volatile double acc = 0.0;  // a product and a sum, two roundings
                for (uint32_t t = 0; t < d; t++) {
                    volatile double v = x[i * ld + t] - x[(c0 + j) * ld + t];
                    volatile double sq = v * v;
                    acc = acc + sq;
                }
                p[j] = {acc, (int32_t)(c0 + j)};
            }
            std::sort(p.begin(), p.end());
            for (uint32_t r = 0; r < k; r++) ind.push_back(p[r].second), dist.push_back(std::sqrt(p[r].first));
        }
        const crgpu::Knn o = crgpu::knn_cross(ctx, x.data(), n, d, ld, k, q0, nq, c0, nc);
        CHECK(o.indices == ind && o.distances.size() == dist.size() && std::memcmp(o.distances.data(), dist.data(), dist.size() * sizeof(double)) == 0);
        CHECK(o.info.pairs_evaluated == nq * nc);
        const crgpu::Knn small = crgpu::knn_cross(ctx, x.data(), n, d, ld, k, q0, nq, c0, nc, k + 4, 1, 4);
        CHECK(small.indices == o.indices && small.distances == o.distances && small.sorted_indices == o.sorted_indices && small.info.in_lds == 0);
        nn[dir] = o.indices;
    }
    const crgpu::MnnPairs m = crgpu::mnn_pairs(nn[0], 0, nn[1], n_i, k);
    CHECK(m.pairs == brute_mnn(nn[0], 0, nn[1], n_i, k) && m.pairs.size() >= 2);
    // one step: batch j moves towards batch i
    crgpu::BcStep st;
    for (uint64_t c = n_i; c < n; c++) st.cur_rows.push_back((int32_t)c);
    for (size_t e = 0; e < m.pairs.size(); e += 2) st.mnn_cur.push_back(m.pairs[e + 1]), st.mnn_ref.push_back(m.pairs[e]);
    const double sigma = 150.0;
    const crgpu::BatchCorrect o = crgpu::batch_correct(ctx, x.data(), n, d, ld, sigma, {st}, true);
    CHECK(o.corr.size() == 1 && o.corr[0].size() == n_j * d && o.info.pairs_evaluated == n_j * st.mnn_cur.size() && o.info.chunks == 1);
    double worst = 0.0, scale = 0.0;
    for (uint64_t c = 0; c < n_j; c++) {
        long double num[8] = {0}, den = 0;
        for (size_t p = 0; p < st.mnn_cur.size(); p++) {
            long double d2 = 0;
            for (uint32_t t = 0; t < d; t++) {
                const long double v = (long double)x[(n_i + c) * ld + t] - x[(uint64_t)st.mnn_cur[p] * ld + t];
                d2 += v * v;
            }
            const long double w = std::exp(-(long double)(0.5 * sigma) * d2);
            den += w;
            for (uint32_t t = 0; t < d; t++) num[t] += w * ((long double)x[(uint64_t)st.mnn_ref[p] * ld + t] - x[(uint64_t)st.mnn_cur[p] * ld + t]);
        }
        for (uint32_t t = 0; t < d; t++) {
            const long double want = num[t] / den;
            worst = std::max(worst, (double)std::fabs((long double)o.corr[0][c * d + t] - want));
            scale = std::max(scale, (double)std::fabs(want));
            const double moved = x[(n_i + c) * ld + t] + o.corr[0][c * d + t];
            CHECK(o.aligned[(n_i + c) * d + t] == moved);
        }
    }
    CHECK(scale > 0.0 && worst <= 1e-12 * scale);
    for (uint64_t c = 0; c < n_i; c++)
        for (uint32_t t = 0; t < d; t++) CHECK(o.aligned[c * d + t] == x[c * ld + t]);
    // the seams move no bit; a sub-list gives the rows of the whole
    const crgpu::BatchCorrect a = crgpu::batch_correct(ctx, x.data(), n, d, ld, sigma, {st}, true, 8, 16, 16),
                              b = crgpu::batch_correct(ctx, x.data(), n, d, ld, sigma, {st}, true, 64, 64);
    CHECK(a.corr == o.corr && a.aligned == o.aligned && a.info.pair_tile == 8 && a.info.row_tile == 16);
    CHECK(b.corr == o.corr && b.aligned == o.aligned && b.info.pair_tile == 64 && b.info.row_tile == 64);
    crgpu::BcStep part = st;
    part.cur_rows.assign(st.cur_rows.begin() + 40, st.cur_rows.begin() + 77);
    const crgpu::BatchCorrect s = crgpu::batch_correct(ctx, x.data(), n, d, ld, sigma, {part}, true);
    CHECK(std::equal(s.corr[0].begin(), s.corr[0].end(), o.corr[0].begin() + 40 * d));
    // no step: the first d columns as they came
    const crgpu::BatchCorrect none = crgpu::batch_correct(ctx, x.data(), n, d, ld, sigma, {});
    for (uint64_t c = 0; c < n; c++) CHECK(std::memcmp(&none.aligned[c * d], &x[c * ld], d * sizeof(double)) == 0);
    // refusals with a live context, which stays good
    crgpu::BcStep bad = st;
    bad.cur_rows[5] = bad.cur_rows[4];
    CHECK(refused(ctx, x, n, d, ld, sigma, {bad}) == CRGPU_EINVAL && refused(ctx, x, n, d, ld, -1.0, {st}) == CRGPU_EINVAL);
    bad = st, bad.mnn_ref[0] = (int32_t)n;
    CHECK(refused(ctx, x, n, d, ld, sigma, {bad}) == CRGPU_EINVAL && refused(ctx, x, n, d, 5, sigma, {st}) == CRGPU_EINVAL);
    CHECK(refused(ctx, x, n, d, ld, sigma, {st}, 12) == CRGPU_EINVAL && refused(ctx, x, n, d, ld, sigma, {st}, 0, 48) == CRGPU_EINVAL);
    std::vector<double> nanx = x;
    nanx[17 * ld + 2] = std::nan("");
    CHECK(refused(ctx, nanx, n, d, ld, sigma, {st}) == CRGPU_EINVAL);
    CHECK(crgpu::batch_correct(ctx, x.data(), n, d, ld, sigma, {st}, true).corr == o.corr);
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
