// C++ host-mirror test of the aggregate wrappers of include/crgpu.hpp (aggregate_min_antibodies, detect_aggregates, apply_minimum_umis,
// apply_mito_threshold): a 7 x 200 matrix (one other row, five antibody rows, one antigen row) with three planted aggregate columns,
// checked against a brute-force restatement in this file (pairs (value, column) ascending, the K largest), and the hand cases of
// tests/test_aggregates_restatement.py for the two closing filters.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_aggregates.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_aggregates_cpp.py)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
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

using U64 = std::vector<uint64_t>;
using U32 = std::vector<uint32_t>;

// the columns of the k largest pairs (x[c], c)
static std::set<uint32_t> top_k(const U32 &x, uint32_t k) {
    std::vector<std::pair<uint32_t, uint32_t>> p;
    for (uint32_t c = 0; c < x.size(); c++) p.push_back({x[c], c});
    std::sort(p.begin(), p.end());
    std::set<uint32_t> out;
    for (size_t i = p.size() > k ? p.size() - k : 0; i < p.size(); i++) out.insert(p[i].second);
    return out;
}

int main() {
    CHECK(crgpu::aggregate_min_antibodies(5) == 5 && crgpu::aggregate_min_antibodies(12) == 10 && crgpu::aggregate_min_antibodies(27) == 16);
    crgpu::Context ctx(0);
    const uint32_t V = 200, NF = 7, K = 25, n_wl = 256;
    U32 wl(n_wl);
    for (uint32_t i = 0; i < n_wl; i++) wl[i] = i;  // packed 16-mers, ascending: column k is barcode k
    ctx.check(crgpu_set_whitelist_packed(ctx.get(), 0, wl.data(), n_wl, 16, wl.data(), n_wl, nullptr));
    U32 valid(n_wl, 0), corrected(n_wl, 0);
    for (uint32_t c = 0; c < V; c++) valid[c] = 1;
    ctx.check(crgpu_set_counts(ctx.get(), 0, CRGPU_COUNTS_VALID, valid.data()));
    ctx.check(crgpu_set_counts(ctx.get(), 0, CRGPU_COUNTS_CORRECTED, corrected.data()));
    // row 0: other; rows 1 .. 5: antibodies, 5 .. 15 per entry (a zero where the formula says so), 500 in the planted columns; row 6: antigen
    const std::vector<uint8_t> kind = {CRGPU_AGG_KIND_OTHER, CRGPU_AGG_KIND_ANTIBODY, CRGPU_AGG_KIND_ANTIBODY, CRGPU_AGG_KIND_ANTIBODY,
                                       CRGPU_AGG_KIND_ANTIBODY, CRGPU_AGG_KIND_ANTIBODY, CRGPU_AGG_KIND_ANTIGEN};
    std::vector<U32> dense(NF, U32(V, 0));
    for (uint32_t c = 0; c < V; c++) {
        dense[0][c] = 1 + c % 3;
        for (uint32_t r = 1; r <= 5; r++) dense[r][c] = (c * 7 + r * 13) % 17 == 0 ? 0 : 5 + (c * (2 * r + 1) + r * 5) % 11;
        dense[6][c] = 3 + c % 5;
    }
    for (uint32_t c : {4u, 120u, 177u})
        for (uint32_t r = 1; r <= 5; r++) dense[r][c] = 500 + r;
    U32 bc, ft, ct;
    for (uint32_t c = 0; c < V; c++)
        for (uint32_t f = 0; f < NF; f++)
            if (dense[f][c]) bc.push_back(c), ft.push_back(f), ct.push_back(dense[f][c]);
    void *d[3];
    const U32 *h[3] = {&bc, &ft, &ct};
    for (int i = 0; i < 3; i++) {
        ctx.check(crgpu_malloc(ctx.get(), &d[i], bc.size() * sizeof(uint32_t)));
        ctx.check(crgpu_memcpy_h2d(ctx.get(), d[i], h[i]->data(), bc.size() * sizeof(uint32_t)));
    }
    crgpu_matrix_dev *m = nullptr;
    ctx.check(crgpu_assemble_matrix_dev(ctx.get(), (const uint32_t *)d[0], (const uint32_t *)d[1], (const uint32_t *)d[2], bc.size(), &m));
    for (void *p : d) crgpu_free(ctx.get(), p);
    CHECK(m->n_barcodes == V && m->nnz == bc.size());

    // the restatement: every antibody row is a signal row (sum >= 1000), all five are needed
    U32 total(V, 0);
    for (uint32_t r = 1; r <= 5; r++) {
        uint64_t sum = 0;
        for (uint32_t c = 0; c < V; c++) sum += dense[r][c], total[c] += dense[r][c];
        CHECK(sum >= 1000);
    }
    std::vector<uint32_t> votes(V, 0);
    for (uint32_t r = 1; r <= 5; r++)
        for (uint32_t c : top_k(dense[r], K)) votes[c]++;
    U64 expect;
    for (uint32_t c : top_k(total, K))
        if (votes[c] >= 5) expect.push_back(c);
    std::sort(expect.begin(), expect.end());
    CHECK((expect == U64{4, 120, 177}));

    U32 reads(V, 500), corr(V, 10);
    reads[7] = reads[120] = 20000, corr[7] = corr[120] = 15000;
    const auto a = crgpu::detect_aggregates(ctx, m, kind, 0, reads, corr);
    U64 removed = expect;
    removed.push_back(7);
    std::sort(removed.begin(), removed.end());
    CHECK(a.removed == removed && a.reasons.size() == removed.size() && a.kept.size() == V - removed.size());
    for (size_t i = 0; i < a.removed.size() && i < a.reasons.size(); i++) {
        const uint8_t want = a.removed[i] == 7 ? CRGPU_AGG_HIGHLY_CORRECTED : a.removed[i] == 120 ? (CRGPU_AGG_COUNTS | CRGPU_AGG_HIGHLY_CORRECTED) : CRGPU_AGG_COUNTS;
        CHECK(a.reasons[i] == want);
    }
    CHECK(a.info.n_antibodies == 5 && a.info.n_signal == 5 && a.info.top_k == K && a.info.n_candidates == K && a.info.min_antibodies == 5);
    CHECK(a.info.n_aggregates == expect.size() && a.info.in_lds == 1 && a.info.n_slices == 1);
    CHECK(a.antigen_threshold == 7.0 + (7.0 - 6.0) * 3);  // the top 100 antigen sums are 40 x 7, 40 x 6, 20 x 5: q1 = 6, q3 = 7; below 1000
    // without the read tables only the counts decide; K = 50 with two probe barcodes
    const auto b = crgpu::detect_aggregates(ctx, m, kind, 2);
    CHECK(b.info.top_k == 50 && b.info.n_candidates == 50 && b.removed.size() >= expect.size());
    for (uint8_t why : b.reasons) CHECK(why == CRGPU_AGG_COUNTS);
    bool refused = false;
    try {
        crgpu::detect_aggregates(ctx, m, std::vector<uint8_t>(kind.begin(), kind.end() - 1));  // row 6 >= n_features
    } catch (const crgpu::Error &e) {
        refused = true;
    }
    CHECK(refused);
    crgpu_matrix_dev_free(ctx.get(), m);

    // the closing filters: the hand cases of tests/test_aggregates_restatement.py
    const U32 umis = {0, 5, 9, 10, 11, 3, 10};
    CHECK((crgpu::apply_minimum_umis(ctx, umis, {0, 2, 3, 4, 6}, 10) == U64{3, 4, 6}));
    CHECK((crgpu::apply_minimum_umis(ctx, umis, {0, 2, 3, 4, 6}, 0) == U64{0, 2, 3, 4, 6}));
    CHECK(crgpu::apply_minimum_umis(ctx, umis, {0, 2, 3, 4, 6}, 12).empty());
    const U32 tot = {0, 200, 200, 8, 1000, 3}, mito = {0, 20, 21, 1, 100, 3};
    const auto f = crgpu::apply_mito_threshold(ctx, mito, tot, {0, 1, 2, 3, 4, 5}, 10.0);
    CHECK((f.kept == U64{0, 1, 4}) && (f.removed == U64{2, 3, 5}));  // 0 / 0 stays, exactly 10 % stays
    CHECK((crgpu::apply_mito_threshold(ctx, mito, tot, {0, 1, 2, 3, 4, 5}, -1.0).kept == U64{0}));
    refused = false;
    try {
        crgpu::apply_minimum_umis(ctx, umis, {3, 1}, 1);  // not ascending
    } catch (const crgpu::Error &e) {
        refused = true;
    }
    CHECK(refused);
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all tests passed\n");
    return 0;
}
