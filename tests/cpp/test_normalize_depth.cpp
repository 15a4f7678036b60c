// C++ host-mirror test of the depth normalisation (include/crgpu.hpp): normalize_depth (NORMALIZE_DEPTH of aggr,
// mro/rna/stages/aggregator/normalize_depth/__init__.py) on a hand-computed table of 3 barcodes, 4 features, 2 classes and 2
// libraries.  Only the rates 1 and 0 are used, whose result does not depend on the random stream: rate 1 keeps every read of a
// molecule, rate 0 none.  normalize_depth_plan is host code.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_normalize_depth.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_normalize_depth_cpp.py)
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
using D = std::vector<double>;
using I = std::vector<int32_t>;

static void test_plan_on_the_host() {
    // usable reads per cell 100, 300 (type 0) and none (type 1 has no cells)
    CHECK(crgpu::normalize_depth_plan({0, 0, 1}, {1000, 3000, 500}, {10, 10, 0}) == D({1.0, 100.0 / 300.0, 0.0}));
    CHECK(crgpu::normalize_depth_plan({0, 1, 0}, {1000, 3000, 500}, {10, 10, 0}) == D({0.0, 1.0, 0.0}));
    CHECK(crgpu::normalize_depth_plan({0, 0, 1}, {1000, 3000, 500}, {10, 10, 0}, false) == D({1.0, 1.0, 1.0}));
    CHECK(crgpu::normalize_depth_plan({0, 0}, {1000, 4000}, {10, 10}, true, true, {0, 1}, 2.0) == D({1.0, 0.5}));    // applied
    CHECK(crgpu::normalize_depth_plan({0, 0}, {1000, 4000}, {10, 10}, true, true, {0, 1}, 5.0) == D({1.0, 0.25}));   // 1.25 > 1: refused
    bool refused = false;
    try {
        crgpu::normalize_depth_plan({0, 0}, {1000, -1}, {10, 10});
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
    // features 0, 1: class 0; 2, 3: class 1.  Cells: barcode 0 (of both classes) and barcode 2 (of class 0 only).
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
    const std::vector<uint8_t> fclass = {0, 0, 1, 1};
    try {
        // rates (1, 1): feature 0 of barcode 0 sits in both libraries and is ONE entry of two molecules
        {
            const auto r = crgpu::normalize_depth(ctx, counts, {1.0, 1.0}, 4, {0, 2}, fclass, 2, {3, 1}, 0, true);
            const auto h = r.matrix.download();
            CHECK(h.barcode_rank == std::vector<uint32_t>({0, 1, 2}) && h.indptr == V({0, 3, 5, 7}));
            CHECK(h.indices == I({0, 1, 2, 0, 3, 1, 2}) && h.data == I({2, 1, 1, 1, 1, 1, 2}));
            CHECK(r.raw_mapped_reads == V({9, 11}) && r.flt_mapped_reads == V({8, 3}));
            CHECK(r.reads_per_lib == V({16, 4}) && r.kept_reads_per_lib == V({16, 4}) && r.kept_molecules_per_lib == V({6, 3}));
            CHECK(r.kept == std::vector<uint32_t>({2, 1, 3, 1, 1, 2, 4, 5, 1}));   // table order: (barcode, library, feature)
            CHECK(r.info.n_molecules == 9 && r.info.n_lane == 9 && r.info.n_kept_molecules == 9 && r.info.n_triplets == 7);
            // the targeted case of main(): feature 1 leaves, the rows behind it move up
            const auto s = crgpu::select_features(ctx, r.matrix, {1, 0, 1, 1}).download();
            CHECK(s.barcode_rank == h.barcode_rank && s.indptr == V({0, 2, 4, 5}) && s.indices == I({0, 1, 0, 2, 1}) && s.data == I({2, 1, 1, 1, 2}));
        }
        // rates (1, 0): the molecules of library 1 die
        {
            const auto r = crgpu::normalize_depth(ctx, counts, {1.0, 0.0}, 4, {0, 2}, fclass, 2, {3, 1}, 0, true);
            const auto h = r.matrix.download();
            CHECK(h.indptr == V({0, 3, 4, 6}) && h.indices == I({0, 1, 2, 0, 1, 2}) && h.data == I({1, 1, 1, 1, 1, 1}));
            CHECK(r.raw_mapped_reads == V({8, 8}) && r.flt_mapped_reads == V({7, 3}));
            CHECK(r.reads_per_lib == V({16, 4}) && r.kept_reads_per_lib == V({16, 0}) && r.kept_molecules_per_lib == V({6, 0}));
            CHECK(r.kept == std::vector<uint32_t>({2, 1, 3, 0, 1, 0, 4, 5, 0}));
        }
        // rates (0, 0): every column stays, empty
        {
            const auto r = crgpu::normalize_depth(ctx, counts, {0.0, 0.0}, 4, {0, 2}, fclass, 2, {3, 1});
            const auto h = r.matrix.download();
            CHECK(h.barcode_rank == std::vector<uint32_t>({0, 1, 2}) && h.indptr == V({0, 0, 0, 0}) && h.indices.empty());
            CHECK(r.raw_mapped_reads == V({0, 0}) && r.flt_mapped_reads == V({0, 0}) && r.kept_reads_per_lib == V({0, 0}) && r.reads_per_lib == V({16, 4}));
        }
        bool refused = false;
        try {
            crgpu::normalize_depth(ctx, counts, {1.5, 0.0}, 4);
        } catch (const crgpu::Error &e) {
            refused = e.code == CRGPU_EINVAL;
        }
        CHECK(refused);
    } catch (...) {
        crgpu_counts_free(ctx.get(), counts);
        throw;
    }
    crgpu_counts_free(ctx.get(), counts);
}

int main(int argc, char **argv) {
    try {
        test_plan_on_the_host();
        if (argc < 2 || std::string(argv[1]) != "--host-only") test_hand_computed_table();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("all tests passed\n");
    return 0;
}
