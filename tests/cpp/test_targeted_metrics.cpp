// C++ host-mirror test of feature_metrics, targeted_rpu_stats and rpu_gmm (include/crgpu.hpp): collapse_feature_counts
// (lib/python/cellranger/pandas_utils.py:571-661) of a hand-computed molecule table of three barcodes and two libraries, the
// reads-per-UMI statistics of a hand-sized tally, and fit_enrichments' guards and a small fit (targeted/gmm.py).
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_targeted_metrics.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_targeted_metrics_cpp.py)
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

using U = std::vector<uint64_t>;

static void test_stats_on_the_host() {
    // features 0 - 3 targeted, 4 - 7 not; quantifiable (num_umis_cells >= 10): 0, 1, 2, 5, 7
    crgpu::FeatureMetrics t;
    t.num_umis = {20, 30, 12, 0, 50, 11, 9, 40}, t.num_reads = {60, 45, 40, 0, 75, 30, 20, 44};
    t.num_umis_cells = {10, 25, 12, 0, 9, 11, 3, 40}, t.num_reads_cells = {31, 40, 40, 0, 20, 30, 9, 44};
    const auto s = crgpu::targeted_rpu_stats(t, {1, 1, 1, 1, 0, 0, 0, 0});
    CHECK(s.q_feature == std::vector<uint32_t>({0, 1, 2, 5, 7}) && s.q_label == std::vector<uint8_t>({1, 1, 1, 0, 0}));
    CHECK(s.stats.median[0] == 3.1 && s.stats.median[1] == 3.0);                  // 3.1, 1.6, 10 / 3 in cells; 3, 1.5, 10 / 3 over all barcodes
    CHECK(s.stats.mean[2] == (30.0 / 11.0 + 44.0 / 40.0) / 2.0);
    CHECK(s.stats.n_genes[0] == 4 && s.stats.n_genes[1] == 4 && s.stats.n_not_detected[0] == 1 && s.stats.n_detected[1] == 4);
    CHECK(s.stats.n_not_quantifiable[1] == 2 && s.stats.n_quantifiable[0] == 3 && s.stats.n_quantifiable_total == 5);
    CHECK(s.stats.pcr_dupe_reads_frac_on_target == (145.0 - 62.0) / 145.0);
    CHECK(s.q_value.size() == 5 && std::fabs(s.q_value[0] - std::log10(3.1)) < 1e-15);
    // a feature that is not Gene Expression is dropped first; an empty selection gives 0.0
    const auto g = crgpu::targeted_rpu_stats(t, {1, 1, 1, 1, 0, 0, 0, 0}, {1, 1, 1, 1, 1, 0, 1, 0});
    CHECK(g.stats.n_genes[1] == 2 && g.stats.mean[2] == 0.0 && g.stats.cv[3] == 0.0 && g.q_feature == std::vector<uint32_t>({0, 1, 2}));
    bool refused = false;
    try {
        crgpu::targeted_rpu_stats(t, {1, 1});
    } catch (const crgpu::Error &e) {
        refused = e.code == CRGPU_EINVAL;
    }
    CHECK(refused);
}

static void test_hand_computed_table() {
    crgpu::Context ctx(0);
    const std::vector<std::string> wl = {"ACGTACGTACGTACGT", "CCCCACGTACGTACGT", "TTTTACGTACGTACGT"};  // ranks 0, 1, 2
    crgpu::BarcodeCorrector lib0(ctx, 0, crgpu::Whitelist::plain(wl), crgpu::SimpleHistogram{});
    crgpu::BarcodeCorrector lib1(ctx, 1, crgpu::Whitelist::plain(wl), crgpu::SimpleHistogram{});
    lib0.check_and_update({wl[0], wl[1], wl[2]});
    lib1.check_and_update({wl[0], wl[1], wl[2]});
    const std::vector<uint8_t> q(4, 'I');
    // (barcode, library, feature, UMI, reads); every UMI differs from every other in at least two bases.  Cells: barcodes 0 and 2.
    struct Mol {
        uint32_t bc;
        int lib;
        uint32_t feature;
        const char *umi;
        int reads;
    };
    const Mol mols[] = {{0, 0, 0, "AAAC", 2}, {0, 1, 0, "CCAG", 1}, {0, 0, 1, "GGTA", 1}, {0, 0, 2, "TTCG", 3}, {1, 0, 0, "ACCA", 1},
                        {1, 1, 3, "CAGT", 2}, {2, 0, 1, "GTTC", 4}, {2, 0, 2, "TGAA", 5}, {2, 1, 2, "AGGT", 1}};
    crgpu::DupBuilder b(ctx, 4, 4, 2);
    for (const Mol &m : mols)
        for (int r = 0; r < m.reads; r++) b.observe(m.bc, m.lib, m.umi, q, m.feature);
    crgpu_counts *counts = nullptr;
    const crgpu::BarcodeDupMarker marker = b.build(&counts);
    CHECK(marker.umi_counts.size() == 9 && counts != nullptr);
    if (!counts) return;
    try {
        const auto both = crgpu::feature_metrics(ctx, counts, 4, {0, 2}, 3u);
        CHECK(both.num_umis == U({3, 2, 3, 1}) && both.num_reads == U({4, 5, 9, 2}));
        CHECK(both.num_umis_cells == U({2, 2, 3, 0}) && both.num_reads_cells == U({3, 5, 9, 0}));
        const auto l0 = crgpu::feature_metrics(ctx, counts, 4, {0, 2}, 1u);
        CHECK(l0.num_umis == U({2, 2, 2, 0}) && l0.num_reads == U({3, 5, 8, 0}) && l0.num_umis_cells == U({1, 2, 2, 0}) && l0.num_reads_cells == U({2, 5, 8, 0}));
        const auto l1 = crgpu::feature_metrics(ctx, counts, 4, {0, 2}, 2u);
        CHECK(l1.num_umis == U({1, 0, 1, 1}) && l1.num_reads == U({1, 0, 1, 2}) && l1.num_umis_cells == U({1, 0, 1, 0}) && l1.num_reads_cells == U({1, 0, 1, 0}));
        const auto none = crgpu::feature_metrics(ctx, counts, 4, {}, 3u);
        CHECK(none.num_umis == both.num_umis && none.num_umis_cells == U({0, 0, 0, 0}));
        int refused = 0;
        for (int k = 0; k < 4; k++) {
            try {
                if (k == 0) crgpu::feature_metrics(ctx, counts, 4, {0, 2}, 0u);      // an empty mask
                if (k == 1) crgpu::feature_metrics(ctx, counts, 4, {0, 2}, 4u);      // library 2 of two
                if (k == 2) crgpu::feature_metrics(ctx, counts, 5, {0, 2}, 1u);      // not the key layout's n_features
                if (k == 3) crgpu::feature_metrics(ctx, counts, 4, {2, 0}, 1u);      // ranks that do not ascend
            } catch (const crgpu::Error &e) {
                refused += e.code == CRGPU_EINVAL;
            }
        }
        CHECK(refused == 4);
    } catch (...) {
        crgpu_counts_free(ctx.get(), counts);
        throw;
    }
    crgpu_counts_free(ctx.get(), counts);
}

static void test_fit_and_its_guards() {
    crgpu::Context ctx(0);
    // fewer than 30 genes in the larger class: every parameter and count is NaN, nothing runs
    std::vector<double> v;
    std::vector<uint8_t> lab;
    for (int i = 0; i < 22; i++) v.push_back(0.2 + 0.01 * i), lab.push_back(i < 10);
    const auto few = crgpu::rpu_gmm(ctx, v, lab, true);
    CHECK(few.result.fitted == 0 && few.result.n_starts == 0 && std::isnan(few.result.log_rpu_threshold) && std::isnan(few.result.n_offtgt_enriched));
    CHECK(std::isnan(few.start_lk[0]) && few.start_iters[5151] == 0);
    // no off-target gene: threshold 0, the class counts of values >= 0
    const auto on = crgpu::rpu_gmm(ctx, {0.3, -0.1, 0.0}, {1, 1, 1});
    CHECK(on.result.log_rpu_threshold == 0.0 && on.result.n_targeted_enriched == 2.0 && on.result.n_targeted_not_enriched == 1.0);
    CHECK(on.result.n_offtgt_enriched == 0.0 && std::isnan(on.result.mu_high) && on.enriched == std::vector<uint8_t>({1, 0, 1}));
    const auto nothing = crgpu::rpu_gmm(ctx, {}, {});
    CHECK(std::isnan(nothing.result.log_rpu_threshold) && std::isnan(nothing.result.n_targeted_enriched));
    // two well separated groups: 40 targeted genes around 0.6, 60 others around 0.2 (a fixed, spread-out pattern)
    v.clear(), lab.clear();
    for (int i = 0; i < 40; i++) v.push_back(0.6 + 0.004 * ((i * 7) % 40 - 20)), lab.push_back(1);
    for (int i = 0; i < 60; i++) v.push_back(0.2 + 0.003 * ((i * 11) % 60 - 30)), lab.push_back(0);
    const auto fit = crgpu::rpu_gmm(ctx, v, lab, true);
    const crgpu_rpu_gmm_result &r = fit.result;
    CHECK(r.fitted == 1 && r.n_starts == CRGPU_GMM_STARTS && r.winner < CRGPU_GMM_STARTS && r.in_lds == 1);
    CHECK(r.n_targeted_enriched == 40.0 && r.n_targeted_not_enriched == 0.0 && r.n_offtgt_enriched == 0.0 && r.n_offtgt_not_enriched == 60.0);
    CHECK(r.log_rpu_threshold == 0.6 + 0.004 * -20 && std::fabs(r.mu_high - 0.598) < 0.01 && std::fabs(r.mu_low - 0.1985) < 0.01);
    CHECK(r.sd_high == r.sd_low && r.sd_high > 100.0);      // the tied PRECISION, twice
    CHECK(std::fabs(r.alpha_high - 0.4) < 1e-6 && std::fabs(r.alpha_high + r.alpha_low - 1.0) < 1e-12);
    CHECK(fit.start_lk[r.winner] == r.max_lk && fit.start_iters[r.winner] >= 2);
    for (size_t i = 0; i < v.size(); i++) CHECK(fit.enriched[i] == (i < 40 ? 1 : 0));
}

int main() {
    try {
        test_stats_on_the_host();
        test_hand_computed_table();
        test_fit_and_its_guards();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("all tests passed\n");
    return 0;
}
