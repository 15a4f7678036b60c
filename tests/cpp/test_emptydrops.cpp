// C++ host-mirror test of crgpu::sgt_proportions / compute_ambient_pvalues / find_nonambient_barcodes (include/crgpu.hpp): the
// cases of lib/python/cellranger/cell_calling.py:144-263 and stats.py:205-231 that can be worked out by hand.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_emptydrops.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_emptydrops_cpp.py)
#include <cmath>
#include <cstdio>
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

using Cols = std::vector<uint64_t>;

// a device matrix of V columns from (column, feature, count) triplets sorted by (column, feature): column c is the c-th
// barcode of a whitelist of V 16-mers, all marked as seen
static crgpu_matrix_dev *make_matrix(crgpu::Context &ctx, uint32_t V, const std::vector<uint32_t> &bc, const std::vector<uint32_t> &ft,
                                     const std::vector<uint32_t> &ct) {
    std::vector<std::string> seqs;
    for (uint32_t i = 0; i < V; i++) {
        std::string s(16, 'A');
        for (int j = 0; j < 16; j++) s[15 - j] = "ACGT"[(i >> (2 * j)) & 3u];
        seqs.push_back(s);
    }
    crgpu::BarcodeCorrector corr(ctx, 0, crgpu::Whitelist::plain(seqs), {});
    std::vector<uint32_t> seen(V, 1);
    ctx.check(crgpu_set_counts(ctx.get(), 0, CRGPU_COUNTS_VALID, seen.data()));
    void *d[3];
    const std::vector<uint32_t> *h[3] = {&bc, &ft, &ct};
    for (int i = 0; i < 3; i++) {
        ctx.check(crgpu_malloc(ctx.get(), &d[i], bc.size() * sizeof(uint32_t) + 4));
        ctx.check(crgpu_memcpy_h2d(ctx.get(), d[i], h[i]->data(), bc.size() * sizeof(uint32_t)));
    }
    crgpu_matrix_dev *m = nullptr;
    ctx.check(crgpu_assemble_matrix_dev(ctx.get(), (const uint32_t *)d[0], (const uint32_t *)d[1], (const uint32_t *)d[2], bc.size(), &m));
    for (void *p : d) crgpu_free(ctx.get(), p);
    return m;
}

int main() {
    {  // Simple Good-Turing on the host: the two refusals are statuses, a Zipf-like vector sums to one with p0 = n1 / N
        int st = -1;
        CHECK(!crgpu::sgt_proportions({1, 1, 2, 3, 4, 5, 6, 7, 8, 9}, &st) && st == CRGPU_SGT_TOO_FEW);  // 9 distinct frequencies
        std::vector<uint64_t> flat;
        for (uint64_t r = 1; r <= 40; r++) flat.insert(flat.end(), 3, r);
        CHECK(!crgpu::sgt_proportions(flat, &st) && st == CRGPU_SGT_SLOPE);
        std::vector<uint64_t> zipf;
        uint64_t total = 0;
        for (uint64_t r = 1; r <= 12; r++)
            for (uint64_t k = 0; k < (uint64_t)4096 >> r; k++) {  // frequency r occurs 2^(12 - r) times: slope ~ -r log 2 / log r < -1
                zipf.push_back(r);
                total += r;
            }
        const auto g = crgpu::sgt_proportions(zipf, &st);
        CHECK(g && st == CRGPU_OK);
        if (g) {
            double sum = g->second;
            for (double x : g->first) sum += x;
            CHECK(std::fabs(sum - 1.0) < 1e-12 && g->second == 2048.0 / (double)total);
            CHECK(g->first.front() < 1.0 / (double)total && g->first.front() == g->first[1] && g->first.back() > g->first.front());
        }
        bool threw = false;
        try {
            crgpu::sgt_proportions({3, 0, 1});
        } catch (const crgpu::Error &e) {
            threw = e.code == CRGPU_EINVAL;
        }
        CHECK(threw);
    }
    crgpu::Context ctx(0);
    {  // compute_ambient_pvalues + BH by hand: 2 rows x 4 simulations, 4 candidates
        const std::vector<int64_t> sim_n = {5, 9};
        const std::vector<double> tab = {-10.0, -8.0, -6.0, -4.0, /* N = 9 */ -20.0, -19.0, -18.0, -17.0};
        const auto r = crgpu::compute_ambient_pvalues(ctx, {5, 9, 5, 9}, {-11.0, -20.0, -5.0, -1.0}, sim_n, tab);
        // simulated values strictly below: 0, 0 (-20 is not below -20), 3, 4 -> p = 1/5, 1/5, 4/5, 5/5
        CHECK((r.first == std::vector<double>{1.0 / 5, 1.0 / 5, 4.0 / 5, 5.0 / 5}));
        // descending: 1 (k = 4), 4/5 (k = 3), 1/5, 1/5 (k = 2, 1): min(1, min.accumulate(4/4 * 1, 4/3 * 4/5, 4/2 * 1/5, 4/1 * 1/5))
        const double tied = 4.0 / 2.0 * (1.0 / 5);
        CHECK((r.second == std::vector<double>{tied, tied, 1.0, 1.0}));
        bool threw = false;
        try {
            crgpu::compute_ambient_pvalues(ctx, {7}, {-1.0}, sim_n, tab);  // no row for N = 7
        } catch (const crgpu::Error &e) {
            threw = e.code == CRGPU_EINVAL;
        }
        CHECK(threw);
    }
    {  // the ways out without additional cells: 40 columns, column c holds c counts of feature c % 3 (and column 39 a second feature)
        const uint32_t V = 40;
        std::vector<uint32_t> bc, ft, ct, sums(V, 0);
        for (uint32_t c = 1; c < V; c++) {
            bc.push_back(c);
            ft.push_back(c % 3);
            ct.push_back(c);
            sums[c] = c;
        }
        bc.push_back(39);
        ft.push_back(5);
        ct.push_back(2);
        sums[39] += 2;
        crgpu_matrix_dev *m = make_matrix(ctx, V, bc, ft, ct);
        CHECK(m->n_barcodes == V && m->nnz == bc.size());
        void *d_sums = nullptr;
        ctx.check(crgpu_malloc(ctx.get(), &d_sums, V * sizeof(uint32_t)));
        ctx.check(crgpu_matrix_dev_column_sums(ctx.get(), m, nullptr, 0, (uint32_t *)d_sums));
        std::vector<uint32_t> got(V);
        ctx.check(crgpu_memcpy_d2h(ctx.get(), got.data(), d_sums, V * sizeof(uint32_t)));
        CHECK(got == sums);
        const Cols cells = {37, 38, 39};
        // places [10, 30) of the descending order are the columns 29 .. 10: max background 29, 4 features seen, 3 of them in the
        // ambient columns -> fewer than 10 distinct frequencies: the SGT refusal
        auto r = crgpu::find_nonambient_barcodes(ctx, m, (const uint32_t *)d_sums, cells, 10, 30, 5, 100);
        CHECK(r.metrics.status == CRGPU_ED_SGT_NOT_APPLICABLE && r.metrics.n_ambient_used == 20 && r.metrics.max_background_umis == 29);
        CHECK(r.metrics.emptydrops_minimum_umis == 30 && r.metrics.n_eval_features == 4 && r.eval_bcs.empty() && r.called == cells);
        // the range lies behind the last column, or holds the one empty column only
        r = crgpu::find_nonambient_barcodes(ctx, m, (const uint32_t *)d_sums, cells, 50, 60, 5, 100);
        CHECK(r.metrics.status == CRGPU_ED_NO_AMBIENT && r.metrics.max_background_umis == 0 && r.metrics.emptydrops_minimum_umis == 5 && r.called == cells);
        r = crgpu::find_nonambient_barcodes(ctx, m, (const uint32_t *)d_sums, cells, 39, 40, 5, 100);
        CHECK(r.metrics.status == CRGPU_ED_NO_AMBIENT && r.metrics.n_ambient_used == 0 && r.called == cells);
        crgpu_free(ctx.get(), d_sums);
        crgpu_matrix_dev_free(ctx.get(), m);
    }
    {  // a run with candidates.  1023 features in classes r = 1 .. 10 of 2^(10 - r) features; ambient column k - 1 (k = 1 .. 10) holds
       // one count of every feature of a class >= k: the ambient row sum of a class-r feature is r, ten distinct frequencies and no
       // feature without ambient counts.  Column 10 holds 3 r of every feature (the profile's shape, about the likeliest vector of
       // its total: no simulation lies below it), column 11 holds 2000 counts of one class-1 feature (every simulation lies above
       // it), column 12 is the initial cell.  Descending totals: 50000, 6108, 2000, 1023, 511, .., 1.
        crgpu::Context ctx(0);  // its own whitelist of 13 columns
        const uint32_t V = 13, F = 1023, S = 1000;
        std::vector<uint32_t> cls, bc, ft, ct;
        for (uint32_t r = 1; r <= 10; r++) cls.insert(cls.end(), 1u << (10 - r), r);
        CHECK(cls.size() == F);
        for (uint32_t k = 1; k <= 10; k++)
            for (uint32_t f = 1024 - (1u << (11 - k)); f < F; f++) {
                bc.push_back(k - 1);
                ft.push_back(f);
                ct.push_back(1);
            }
        for (uint32_t f = 0; f < F; f++) {
            bc.push_back(10);
            ft.push_back(f);
            ct.push_back(3 * cls[f]);
        }
        bc.insert(bc.end(), {11, 12});
        ft.insert(ft.end(), {0, 1022});
        ct.insert(ct.end(), {2000, 50000});
        crgpu_matrix_dev *m = make_matrix(ctx, V, bc, ft, ct);
        CHECK(m->n_barcodes == V && m->nnz == bc.size());
        void *d_sums = nullptr;
        ctx.check(crgpu_malloc(ctx.get(), &d_sums, V * sizeof(uint32_t)));
        ctx.check(crgpu_matrix_dev_column_sums(ctx.get(), m, nullptr, 0, (uint32_t *)d_sums));
        const auto r = crgpu::find_nonambient_barcodes(ctx, m, (const uint32_t *)d_sums, {12}, 3, 13, 5, S);
        CHECK(r.metrics.status == CRGPU_ED_OK && r.metrics.n_ambient_used == 10 && r.metrics.max_background_umis == 1023);
        CHECK(r.metrics.emptydrops_minimum_umis == 1024 && r.metrics.n_eval_features == F && r.metrics.n_candidates == 2);
        CHECK(r.metrics.n_distinct_n == 2 && r.metrics.n_nonambient == 1 && r.metrics.sgt_slope < -1.0);
        CHECK((r.eval_bcs == Cols{10, 11}) && (r.umis == std::vector<uint32_t>{6108, 2000}));
        CHECK(r.log_likelihood.size() == 2 && r.log_likelihood[1] < r.log_likelihood[0] && r.log_likelihood[0] < 0.0);
        // p = (1 + S) / (1 + S) and 1 / (1 + S); BH over two: min(1, 2/2 * 1) and 2/1 * 1/(1 + S)
        CHECK((r.pvalues == std::vector<double>{1.0, 1.0 / (1 + S)}));
        CHECK((r.pvalues_adj == std::vector<double>{1.0, 2.0 * (1.0 / (1 + S))}));
        CHECK((r.is_nonambient == std::vector<uint8_t>{0, 1}) && (r.called == Cols{11, 12}));
        crgpu_free(ctx.get(), d_sums);
        crgpu_matrix_dev_free(ctx.get(), m);
    }
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all tests passed\n");
    return 0;
}
