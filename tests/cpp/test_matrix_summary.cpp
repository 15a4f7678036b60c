// C++ host-mirror test of the matrix-summary wrappers of include/crgpu.hpp (reads_per_column, matrix_summary, matrix_summary_stats):
// the hand-computed 6 x 8 matrix of tests/matrix_summary_numpy.py::hand_matrix -- features 0 1 2 in class 0, 3 4 in class 1, 5 in
// none; the cells are columns 1 (class 0), 3 (both) and 6 (class 1).
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_matrix_summary.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_matrix_summary_cpp.py)
#include <cmath>
#include <cstdint>
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

using U64 = std::vector<uint64_t>;
using U32 = std::vector<uint32_t>;

template <typename T, size_t N>
static std::vector<T> vec(const T (&a)[N], uint32_t n = N) {
    return std::vector<T>(a, a + n);
}

int main() {
    crgpu::Context ctx(0);
    const uint32_t n_wl = 16;
    U32 wl(n_wl);
    for (uint32_t i = 0; i < n_wl; i++) wl[i] = i;  // packed 16-mers, ascending: column k is barcode k
    ctx.check(crgpu_set_whitelist_packed(ctx.get(), 0, wl.data(), n_wl, 16, wl.data(), n_wl, nullptr));
    const U32 reads = {20, 30, 1, 40, 15, 2, 50, 7};
    U32 valid(n_wl, 0), corrected(n_wl, 0);
    for (size_t c = 0; c < reads.size(); c++) valid[c] = reads[c] - 1, corrected[c] = 1;
    ctx.check(crgpu_set_counts(ctx.get(), 0, CRGPU_COUNTS_VALID, valid.data()));
    ctx.check(crgpu_set_counts(ctx.get(), 0, CRGPU_COUNTS_CORRECTED, corrected.data()));
    // (column, feature, count) in column order, the features ascending; column 2 is empty
    const U32 bc = {0, 0, 1, 1, 1, 3, 3, 3, 3, 3, 4, 4, 5, 6, 6, 6, 7};
    const U32 ft = {0, 5, 0, 1, 3, 0, 2, 3, 4, 5, 1, 4, 2, 0, 3, 4, 5};
    const U32 ct = {3, 9, 5, 1, 7, 2, 4, 1, 6, 2, 8, 1, 1, 11, 2, 2, 4};
    void *d[3];
    const U32 *h[3] = {&bc, &ft, &ct};
    for (int i = 0; i < 3; i++) {
        ctx.check(crgpu_malloc(ctx.get(), &d[i], bc.size() * sizeof(uint32_t)));
        ctx.check(crgpu_memcpy_h2d(ctx.get(), d[i], h[i]->data(), bc.size() * sizeof(uint32_t)));
    }
    crgpu_matrix_dev *m = nullptr;
    ctx.check(crgpu_assemble_matrix_dev(ctx.get(), (const uint32_t *)d[0], (const uint32_t *)d[1], (const uint32_t *)d[2], bc.size(), &m));
    for (void *p : d) crgpu_free(ctx.get(), p);
    CHECK(m->n_barcodes == 8 && m->nnz == 17);

    const U32 r = crgpu::reads_per_column(ctx, m);
    CHECK(r == reads);
    const std::vector<uint8_t> fc = {0, 0, 0, 1, 1, CRGPU_MS_NO_CLASS};
    const auto s = crgpu::matrix_summary(ctx, m, {1, 3, 6}, 6, fc, 2, {1, 3, 2}, r, true);
    CHECK((s.counts_per_feature == U64{7, 1, 4, 3, 8, 0}) && (s.cells_ge2_per_feature == U64{2, 0, 1, 1, 2, 0}));
    CHECK(s.reads_all == 165 && s.reads_union == 120);
    const auto &c0 = s.classes[0], &c1 = s.classes[1];
    CHECK(c0.n_features_class == 3 && c0.n_cells == 2 && c1.n_features_class == 2 && c1.n_cells == 2);
    CHECK(c0.raw_total_counts == 35 && c1.raw_total_counts == 19);
    CHECK(c0.union_total_counts == 23 && c0.union_nnz == 5 && c1.union_total_counts == 18 && c1.union_nnz == 5);
    CHECK(c0.cells_total_counts == 12 && c0.cells_nnz == 4 && c0.genes_detected == 3);
    CHECK(c1.cells_total_counts == 11 && c1.cells_nnz == 4 && c1.genes_detected == 2);
    CHECK(c0.counts_sum == 12 && c0.counts_sumsq_hi == 0 && c0.counts_sumsq_lo == 72 && c0.genes_sum == 4 && c0.genes_sumsq_lo == 8);
    CHECK(c1.counts_sum == 11 && c1.counts_sumsq_lo == 65 && c0.reads_cells == 70 && c1.reads_cells == 90);
    CHECK((vec(c0.counts_q) == U32{6, 6, 6, 6, 6, 6}) && (vec(c1.counts_q) == U32{4, 7, 4, 7, 4, 7}) && (vec(c1.genes_q) == U32{2, 2, 2, 2, 2, 2}));
    CHECK(c0.n_top == 3 && (vec(c0.top_counts_feature, 3) == U32{0, 2, 1}) && (vec(c0.top_counts_value, 3) == U64{7, 4, 1}));
    CHECK((vec(c0.top_cells_feature, 3) == U32{0, 2, 1}) && (vec(c0.top_cells_value, 3) == U64{2, 1, 0}));
    CHECK(c1.n_top == 2 && (vec(c1.top_counts_feature, 2) == U32{4, 3}) && (vec(c1.top_counts_value, 2) == U64{8, 3}));
    CHECK((s.counts_per_cell == U32{6, 6, 0, 0, 7, 4}) && (s.genes_per_cell == U32{2, 2, 0, 0, 2, 2}));
    const auto f = crgpu::matrix_summary_stats(s, 1);
    CHECK(f.counts_mean == 5.5 && f.counts_median == 5.5 && f.counts_iqr == 1.5 && f.counts_std == 1.5 && f.counts_cv == 1.5 / 5.5);
    CHECK(f.genes_mean == 2.0 && f.genes_cv == 0.0 && f.density == 1.0 && f.cum_frac == 11.0 / 19.0);
    CHECK(f.dupe_frac == 1.0 - 11.0 / 90.0 && f.reads_per_cell == 45.0 && f.reads_cum_frac == 90.0 / 165.0);

    // no cells, one class over every feature, no read table
    const auto none = crgpu::matrix_summary(ctx, m, {}, 6);
    CHECK(none.classes.size() == 1 && none.classes[0].n_cells == 0 && none.classes[0].raw_total_counts == 69 && none.reads_all == 0);
    CHECK(std::isnan(crgpu::matrix_summary_stats(none, 0).counts_mean) && std::isnan(crgpu::matrix_summary_stats(none, 0).dupe_frac));
    bool refused = false;
    try {
        crgpu::matrix_summary(ctx, m, {3, 1}, 6);  // not ascending
    } catch (const crgpu::Error &e) {
        refused = true;
    }
    CHECK(refused);
    crgpu_matrix_dev_free(ctx.get(), m);
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all tests passed\n");
    return 0;
}
