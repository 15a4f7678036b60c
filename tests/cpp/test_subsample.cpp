// C++ host-mirror test of the read subsampling (include/crgpu.hpp): run_subsampling (lib/python/cellranger/subsample.py:430-654)
// on a hand-computed table of 3 barcodes, 2 genomes and 2 libraries.  Only the rates 1 and 0 are used, whose result does not
// depend on the random stream: rate 1 keeps every read of a molecule, rate 0 none.  make_subsamplings and the summary are host code.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_subsample.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_subsample_cpp.py)
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

using V = std::vector<int64_t>;

static void test_plan_and_summary_on_the_host() {
    // MAPPED: usable reads per cell = [5000.5, 15000]: depths 500, 1000, ..., 4500, trunc(5000.5) = 5000, and the fixed 20000
    const auto plan = crgpu::make_subsamplings(CRGPU_SS_PLAN_MAPPED, {0, 1}, {100, 100}, {1e6, 2e6}, {500050, 1500000}, {3000, 20000});
    CHECK(plan.size() == 11);
    if (plan.size() == 11) {
        CHECK(plan[0].target_read_pairs_per_cell == 500 && plan[9].target_read_pairs_per_cell == 5000 && plan[10].target_read_pairs_per_cell == 20000);
        CHECK(plan[0].library_subsample_rates[0] == 500 * 100.0 / 500050 && plan[0].library_subsample_rates[1] == 500 * 100.0 / 1500000);
        const double r0 = 5000 * 100.0 / 500050, r1 = 5000 * 100.0 / 1500000;  // the largest computed depth: renormalised
        CHECK(plan[9].library_subsample_rates[0] == 1.0 && plan[9].library_subsample_rates[1] == r1 / r0);
        CHECK(plan[10].library_subsample_rates[0] == 0.0 && plan[10].library_subsample_rates[1] == 0.0);  // rates above 1
        CHECK(plan[0].task_type == CRGPU_SS_PER_CELL);
    }
    CHECK(crgpu::make_subsamplings(CRGPU_SS_PLAN_BULK, {0}, {1000}, {700}, {600}, {}).size() == 10);
    CHECK(crgpu::make_subsamplings(CRGPU_SS_PLAN_RAW, {0}, {1000}, {700}, {600}, {}).empty());  // fewer than one read per cell

    crgpu::SubsampleData d;
    d.n_tasks = 1, d.n_genomes = 1, d.n_libs = 1, d.n_features = 2, d.n_cells = 4;
    d.umis_per_bc = {5, 1, 9, 2}, d.read_pairs_per_bc = {16, 4, 28, 7}, d.features_det_per_bc = {3, 1, 4, 2};
    d.read_pairs = {60}, d.umis = {17}, d.total_features_det = {9, 8};
    const std::vector<crgpu::SubsamplingDef> one = {{3000, CRGPU_SS_PER_CELL, {0.5}}};
    auto s = crgpu::subsampling_summary(d, one);
    const double want[7] = {13.75, 11.5, 4.25, 3.5, 2.5, 2.5, 43.0 / 60.0};
    for (int k = 0; k < 7; k++) CHECK(s.first[k] == want[k]);
    CHECK(s.second[0] == 43.0 / 60.0);
    s = crgpu::subsampling_summary(d, one, {1, 1, 0, 1});  // three cells: the middle value
    CHECK(s.first[CRGPU_SS_MEDIAN_UMIS] == 2.0 && s.first[CRGPU_SS_MEDIAN_READ_PAIRS] == 7.0 && s.first[CRGPU_SS_MEAN_FEATURES] == 2.0);
    s = crgpu::subsampling_summary(d, one, {0, 0, 0, 0});
    CHECK(std::isnan(s.first[CRGPU_SS_MEAN_UMIS]) && std::isnan(s.first[CRGPU_SS_MEDIAN_FEATURES]));
}

static void test_hand_computed_tallies() {
    crgpu::Context ctx(0);
    const std::vector<std::string> wl = {"ACGTACGTACGTACGT", "CCCCACGTACGTACGT", "TTTTACGTACGTACGT"};  // ranks 0, 1, 2
    crgpu::BarcodeCorrector lib0(ctx, 0, crgpu::Whitelist::plain(wl), crgpu::SimpleHistogram{});
    crgpu::BarcodeCorrector lib1(ctx, 1, crgpu::Whitelist::plain(wl), crgpu::SimpleHistogram{});
    lib0.check_and_update({wl[0], wl[1], wl[2]});
    lib1.check_and_update({wl[0], wl[1], wl[2]});
    const std::vector<uint8_t> q(4, 'I');
    // features 0, 1: genome 0; 2, 3: genome 1.  Cells: barcode 0 (of both genomes) and barcode 2 (of genome 0 only).
    // (barcode, library, feature, UMI, reads); every UMI differs from every other in at least two bases.
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
    const std::vector<crgpu::SubsamplingDef> tasks = {{1, CRGPU_SS_PER_CELL, {1.0, 1.0}}, {2, CRGPU_SS_PER_CELL, {1.0, 0.0}},
                                                      {3, CRGPU_SS_CELLS_ONLY, {1.0, 0.0}}, {4, CRGPU_SS_BULK, {1.0, 1.0}},
                                                      {5, CRGPU_SS_PER_CELL, {0.0, 0.0}}};
    crgpu::SubsampleData d;
    try {
        d = crgpu::run_subsampling(ctx, counts, tasks, 2, 4, {0, 2}, 2, {0, 0, 1, 1}, {3, 1});
    } catch (...) {
        crgpu_counts_free(ctx.get(), counts);
        throw;
    }
    crgpu_counts_free(ctx.get(), counts);
    auto bc = [&](const V &v, int t) { return V(v.begin() + t * 4, v.begin() + t * 4 + 4); };      // [genome][cell]
    auto tot = [&](const V &v, int t) { return V(v.begin() + t * 2, v.begin() + t * 2 + 2); };     // [genome]
    auto tfd = [&](int t) { return V(d.total_features_det.begin() + t * 8, d.total_features_det.begin() + t * 8 + 8); };
    // task 0, rates (1, 1): feature 0 of barcode 0 sits in both libraries and is ONE feature
    CHECK(bc(d.umis_per_bc, 0) == V({3, 1, 1, 0}) && bc(d.read_pairs_per_bc, 0) == V({4, 4, 3, 0}) && bc(d.features_det_per_bc, 0) == V({2, 1, 1, 0}));
    CHECK(tot(d.read_pairs, 0) == V({9, 11}) && tot(d.umis, 0) == V({5, 4}) && tfd(0) == V({2, 2, 0, 0, 0, 0, 1, 0}));
    // task 1, rates (1, 0): the molecules of library 1 die; barcode 1 is no cell but counts towards the totals
    CHECK(bc(d.umis_per_bc, 1) == V({2, 1, 1, 0}) && bc(d.read_pairs_per_bc, 1) == V({3, 4, 3, 0}) && bc(d.features_det_per_bc, 1) == V({2, 1, 1, 0}));
    CHECK(tot(d.read_pairs, 1) == V({8, 8}) && tot(d.umis, 1) == V({4, 2}) && tfd(1) == V({1, 2, 0, 0, 0, 0, 1, 0}));
    // task 2, cells only: the same cell entries, totals over the cells of each genome
    CHECK(bc(d.umis_per_bc, 2) == bc(d.umis_per_bc, 1) && bc(d.features_det_per_bc, 2) == bc(d.features_det_per_bc, 1));
    CHECK(tot(d.read_pairs, 2) == V({7, 3}) && tot(d.umis, 2) == V({3, 1}) && tfd(2) == tfd(1));
    // task 3, bulk: one group
    CHECK(bc(d.umis_per_bc, 3) == V({5, 5, 4, 4}) && bc(d.read_pairs_per_bc, 3) == V({9, 9, 11, 11}) && bc(d.features_det_per_bc, 3) == V({0, 0, 0, 0}));
    CHECK(tot(d.read_pairs, 3) == V({9, 11}) && tot(d.umis, 3) == V({5, 4}) && tfd(3) == V({3, 2, 0, 0, 0, 0, 3, 1}));
    // task 4, all rates 0: zeros
    CHECK(bc(d.umis_per_bc, 4) == V({0, 0, 0, 0}) && tot(d.read_pairs, 4) == V({0, 0}) && tfd(4) == V(8, 0));
    CHECK(d.any_reads == std::vector<uint8_t>({1, 1, 1, 1}));
    CHECK(d.info.n_molecules == 9 && d.info.n_groups == 3 && d.info.n_active_tasks == 4 && d.info.n_lane == 9);
    const auto s = crgpu::subsampling_summary(d, tasks, {3, 1});
    CHECK(s.first[(0 * 2 + 0) * 7 + CRGPU_SS_MEDIAN_UMIS] == 2.0 && s.first[(0 * 2 + 1) * 7 + CRGPU_SS_MEDIAN_UMIS] == 1.0);
    CHECK(s.first[(3 * 2 + 1) * 7 + CRGPU_SS_MEAN_FEATURES] == 2.0 && s.second[0] == 11.0 / 20.0 && s.second[4] == 0.0);
    bool refused = false;
    try {
        crgpu::run_subsampling(ctx, nullptr, tasks, 2, 4, {0, 2});
    } catch (const crgpu::Error &e) {
        refused = e.code == CRGPU_EINVAL;
    }
    CHECK(refused);
}

int main(int argc, char **argv) {
    try {
        test_plan_and_summary_on_the_host();
        if (argc < 2 || std::string(argv[1]) != "--host-only") test_hand_computed_tallies();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("all tests passed\n");
    return 0;
}
