// C++ host-mirror test of crgpu::filter_cellular_barcodes_ordmag / _fixed_cutoff (include/crgpu.hpp): the cases of
// lib/python/cellranger/cell_calling_helpers.py:864-964 that can be worked out by hand (no random draw matters).
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_cell_calling.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_cell_calling_cpp.py)
#include <cmath>
#include <cstdio>
#include <optional>
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

int main() {
    crgpu::Context ctx(0);
    {  // one non-zero barcode: every resample is that barcode, the estimate ends at the floor of 50 recovered cells
        const auto r = crgpu::filter_cellular_barcodes_ordmag(ctx, {0, 5, 0}, std::nullopt);
        CHECK(r.top_bc_idx == Cols{1});
        CHECK(r.metrics.n_nonzero == 1 && r.metrics.recovered_cells == 50 && r.metrics.estimated == 1);
        CHECK(r.metrics.recovered_boot[0] == 2 && r.metrics.loss_boot[99] == 0.5);  // (1 - 2)^2 / 2 is the first minimum
        CHECK(r.metrics.baseline_bc_idx == 0 && r.metrics.top_n_boot[0] == 1 && r.metrics.top_n_boot[99] == 1);
        CHECK(r.metrics.filtered_bcs == 1 && r.metrics.filtered_bcs_cutoff_set == 0);  // the tie loop never runs
        CHECK(r.metrics.filtered_bcs_mean == 1.0 && r.metrics.filtered_bcs_var == 0.0 && std::isnan(r.metrics.filtered_bcs_lb));
    }
    {  // recovered_cells given: the floor still applies, nothing is estimated
        const auto r = crgpu::filter_cellular_barcodes_ordmag(ctx, {0, 5, 0}, 7);
        CHECK(r.top_bc_idx == Cols{1} && r.metrics.recovered_cells == 50 && r.metrics.estimated == 0 && r.metrics.recovered_boot[0] == 0);
    }
    {  // all-zero counts and no counts at all: no cells, zeroed metrics, no error
        const auto r = crgpu::filter_cellular_barcodes_ordmag(ctx, {0, 0, 0, 0}, std::nullopt);
        CHECK(r.top_bc_idx.empty() && r.metrics.n_nonzero == 0 && r.metrics.filtered_bcs == 0);
        CHECK(crgpu::filter_cellular_barcodes_ordmag(ctx, {}, 100).top_bc_idx.empty());
    }
    {  // fixed cutoff: among equal counts the larger column wins; the cutoff is the count at descending place top_n
        const std::vector<uint32_t> counts = {3, 7, 7, 0, 1};
        auto r = crgpu::filter_cellular_barcodes_fixed_cutoff(ctx, counts, 1);
        CHECK(r.top_bc_idx == Cols{2} && r.metrics.filtered_bcs == 1 && r.metrics.filtered_bcs_cutoff_set && r.metrics.filtered_bcs_cutoff == 7);
        r = crgpu::filter_cellular_barcodes_fixed_cutoff(ctx, counts, 3);
        CHECK((r.top_bc_idx == Cols{0, 1, 2}) && r.metrics.filtered_bcs_cutoff == 1);
        r = crgpu::filter_cellular_barcodes_fixed_cutoff(ctx, counts, 100);  // more than the non-zero barcodes
        CHECK((r.top_bc_idx == Cols{0, 1, 2, 4}) && r.metrics.filtered_bcs == 4 && r.metrics.filtered_bcs_cutoff_set && r.metrics.filtered_bcs_cutoff == 0);
        CHECK(r.metrics.filtered_bcs_lb == 4.0 && r.metrics.filtered_bcs_ub == 4.0 && r.metrics.filtered_bcs_var == 0.0);
    }
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all tests passed\n");
    return 0;
}
