// C++ host-mirror test of crgpu::multigenome_analysis (include/crgpu.hpp): two small wells of
// lib/python/cellranger/analysis/multigenome.py:80-335 whose integers were worked out with numpy (np.random.seed(0),
// np.random.choice, np.percentile) and are compiled in.  F1: the branch of classify_gems changes between samples; F2: a pure
// species, where the fold-change test sends the thresholds to the percentile of c0 + c1.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_multigenome.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_multigenome_cpp.py)
#include <cmath>
#include <cstdio>
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

using U8 = std::vector<uint8_t>;

// column sums and the sums weighted by the sample's number: a sample out of place changes the second
static void sums(const std::vector<int64_t> &bc, int64_t plain[3], int64_t weighted[3]) {
    for (int k = 0; k < 3; k++) plain[k] = weighted[k] = 0;
    for (size_t s = 0; s < bc.size() / 3; s++)
        for (int k = 0; k < 3; k++) {
            plain[k] += bc[3 * s + k];
            weighted[k] += (int64_t)s * bc[3 * s + k];
        }
}
static std::vector<int> branches(const std::vector<int32_t> &br) {
    std::vector<int> n(4, 0);
    for (int32_t b : br) n[b]++;
    return n;
}

int main() {
    crgpu::Context ctx(0);
    int64_t plain[3], weighted[3];
    {  // F1
        const auto r = crgpu::multigenome_analysis(ctx, {900, 800, 700, 650, 12, 3, 40, 0, 5}, {10, 7, 0, 30, 600, 500, 40, 0, 450});
        const auto &m = r.result;
        CHECK((r.call == U8{0, 0, 0, 0, 1, 1, 0, 0, 1}));  // the tie (40, 40) and the empty barcode are genome0
        CHECK(m.n == 9 && m.observed_multiplets == 0 && m.observed_genome0 == 6 && m.observed_genome1 == 3);
        CHECK(m.obs_thresh0 == 665.0 && m.obs_thresh1 == 460.0 && m.obs_branch == CRGPU_MG_BRANCH_PERCENTILES);
        CHECK(m.sum_c0_genome0 == 3090 && m.sum_all_genome0 == 3177 && m.sum_c1_genome1 == 1550 && m.sum_all_genome1 == 1570);
        CHECK(m.sum_max_single == 4640 && m.sum_all_single == 4747 && m.purity0 == 3090.0 / 3177.0 && m.purity_overall == 4640.0 / 4747.0);
        sums(r.boot_counts, plain, weighted);
        CHECK(plain[0] == 100 && plain[1] == 5865 && plain[2] == 3035);
        CHECK(weighted[0] == 42123 && weighted[1] == 2924166 && weighted[2] == 1529211);
        CHECK(r.boot_counts[6] == 0 && r.boot_counts[7] == 5 && r.boot_counts[8] == 4 && r.boot_counts[2998] == 8);
        CHECK((branches(r.boot_branch) == std::vector<int>{25, 975, 0, 0}));
        CHECK(r.boot_thresholds[0] == 650.0 && r.boot_thresholds[1] == 500.0);
        CHECK(m.inferred_multiplets == 0 && m.boot_mean == 0.025383333333333334 && m.rate_bounds_set == 1 && m.multiplet_rate_ub == 0.0);
        CHECK(m.multiplet_rate == m.boot_mean / 9.0 && r.boot.size() == 1000);
    }
    {  // F2
        const auto r = crgpu::multigenome_analysis(ctx, {1200, 900, 2000, 1500, 0, 1100, 700, 1, 1300, 800, 950, 0},
                                                   {0, 1, 2, 0, 1, 0, 0, 2, 1, 0, 0, 2});
        const auto &m = r.result;
        CHECK((r.call == U8{0, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 1}));
        CHECK(m.n == 12 && m.observed_multiplets == 0 && m.observed_genome0 == 9 && m.observed_genome1 == 3);
        CHECK(m.obs_thresh0 == 2.1 && m.obs_thresh1 == 2.1 && m.obs_branch == CRGPU_MG_BRANCH_PERCENTILES_SUM);
        CHECK(m.sum_c0_genome0 == 10450 && m.sum_all_genome0 == 10454 && m.sum_c1_genome1 == 5 && m.sum_all_genome1 == 6);
        sums(r.boot_counts, plain, weighted);
        CHECK(plain[0] == 435 && plain[1] == 8668 && plain[2] == 2897);
        CHECK(weighted[0] == 211036 && weighted[1] == 4354627 && weighted[2] == 1428337);
        CHECK((branches(r.boot_branch) == std::vector<int>{29, 0, 0, 971}));
        CHECK(m.inferred_multiplets == 1 && m.boot_mean == 0.943120238095238 && m.multiplet_rate_ub == 0.5625 && m.multiplet_rate_lb == 0.0);
    }
    {  // one sample: no bounds; no barcodes: a zeroed result
        const auto one = crgpu::multigenome_analysis(ctx, {500, 400, 450, 3}, {2, 1, 350, 300}, 1);
        CHECK(one.result.rate_bounds_set == 0 && one.result.observed_multiplets == 1 && one.boot_counts.size() == 3);
        const auto none = crgpu::multigenome_analysis(ctx, {}, {}, 10);
        CHECK(none.result.n == 0 && none.result.inferred_multiplets == 0 && none.call.empty());
    }
    CHECK((crgpu::multigenome_top_two({5, 9, 7}) == std::vector<uint32_t>{1, 2}));
    CHECK((crgpu::multigenome_top_two({7, 7, 7}) == std::vector<uint32_t>{1, 2}));  // equal totals: the larger index first
    CHECK((crgpu::multigenome_top_two({9, 4, 4}) == std::vector<uint32_t>{0, 2}));
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all tests passed\n");
    return 0;
}
