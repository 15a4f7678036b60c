// C++ host-mirror test of the multiplexed-Flex wrappers of include/crgpu.hpp (rtl_tags .. remove_high_occupancy_gems): the
// hand-computed well of tests/test_rtl_tags_restatement.py -- five GEMs, three probe barcodes, every column a cell:
//   GEM 0: probes 0 1   GEM 1: 0   GEM 2: 1 2   GEM 3: 0 1 2   GEM 4: 0
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_rtl_tags.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_rtl_tags_cpp.py)
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

int main() {
    crgpu::Context ctx(0);
    const uint32_t n_gel = 8, n_probe = 3;
    std::vector<uint32_t> gel(n_gel), probe(n_probe);
    for (uint32_t i = 0; i < n_gel; i++) gel[i] = i;  // packed 16-mers, ascending
    for (uint32_t i = 0; i < n_probe; i++) probe[i] = i;
    const uint32_t seg_n[2] = {n_gel, n_probe}, seg_len[2] = {16, 8};
    const uint32_t *seqs[2] = {gel.data(), probe.data()};
    ctx.check(crgpu_set_barcode_segments(ctx.get(), 0, 2, seg_n, seg_len, seqs));
    const std::vector<uint32_t> ranks = {0, 1, 3, 7, 8, 9, 10, 11, 12};  // gel * 3 + probe
    std::vector<uint32_t> seen(n_gel * n_probe, 0), ft(ranks.size(), 0), ct;
    for (size_t k = 0; k < ranks.size(); k++) {
        seen[ranks[k]] = 1;
        ct.push_back(10 + (uint32_t)k);
    }
    ctx.check(crgpu_set_counts(ctx.get(), 0, CRGPU_COUNTS_VALID, seen.data()));
    void *d[3];
    const std::vector<uint32_t> *h[3] = {&ranks, &ft, &ct};
    for (int i = 0; i < 3; i++) {
        ctx.check(crgpu_malloc(ctx.get(), &d[i], ranks.size() * sizeof(uint32_t)));
        ctx.check(crgpu_memcpy_h2d(ctx.get(), d[i], h[i]->data(), ranks.size() * sizeof(uint32_t)));
    }
    crgpu_matrix_dev *m = nullptr;
    ctx.check(crgpu_assemble_matrix_dev(ctx.get(), (const uint32_t *)d[0], (const uint32_t *)d[1], (const uint32_t *)d[2], ranks.size(), &m));
    for (void *p : d) crgpu_free(ctx.get(), p);
    CHECK(m->n_barcodes == 9);

    const auto t = crgpu::rtl_tags(ctx, m, {0, 1, 2}, 3, {0}, 1);
    CHECK((t.tags == std::vector<uint8_t>{0, 1, 0, 1, 2, 0, 1, 2, 0}));
    CHECK((t.barcodes_per_tag == U64{4, 3, 2}));
    CHECK((t.umi_per_tag == U64{10 + 12 + 15 + 18, 11 + 13 + 16, 14 + 17}));

    const U64 cells = {0, 1, 2, 3, 4, 5, 6, 7, 8};
    const auto r = crgpu::rtl_gem_runs(ctx, m, t.tags, 3, cells);
    CHECK(r.n_probe == 3 && r.n_tags == 3 && r.n_gems == 5 && r.gems_with_cells == 5 && r.n_cells == 9);
    CHECK(r.gems_per_tag[0] == 4 && r.gems_per_tag[1] == 3 && r.gems_per_tag[2] == 2);
    CHECK(r.common[0 * 64 + 1] == 2 && r.common[0 * 64 + 2] == 1 && r.common[1 * 64 + 2] == 2 && r.common[1 * 64 + 0] == 0);
    CHECK(r.cells_per_gem_hist[1] == 2 && r.cells_per_gem_hist[2] == 2 && r.cells_per_gem_hist[3] == 1);
    CHECK(r.cells_per_probe[0] == 4 && r.cells_per_probe[1] == 3 && r.cells_per_probe[2] == 2);
    CHECK(r.first_cell_col_per_probe[0] == 0 && r.first_cell_col_per_probe[1] == 1 && r.first_cell_col_per_probe[2] == 4);
    const auto rows = crgpu::rtl_overlap_rows(r);
    CHECK(rows.size() == 3);
    if (rows.size() == 3) {
        CHECK(rows[0].tag1 == 0 && rows[0].tag2 == 1 && rows[0].gems1 == 4 && rows[0].gems2 == 3 && rows[0].common_gems == 2);
        CHECK(rows[0].overlap == 2.0 / 3.0 && rows[1].overlap == 0.5 && rows[2].overlap == 1.0);
    }
    const auto occ = crgpu::rtl_occupancy_summary(r);
    CHECK(occ.zero_bin == 69691 && occ.estimated_lambda == 9.0 / 69696.0 && occ.total_probe_barcodes == 3);

    // the columns of two samples: tags 0 and 2 -> sample 0, tag 1 -> none; all columns, three cells, an empty cell call
    const std::vector<uint8_t> sot = {0, 0xFF, 0};
    const auto all_cols = crgpu::rtl_sample_columns(ctx, m, t.tags, sot, 2);
    CHECK(all_cols.size() == 2 && (all_cols[0] == U64{0, 2, 4, 5, 7, 8}) && all_cols[1].empty());
    const U64 some = {1, 2, 7}, nobody;
    CHECK((crgpu::rtl_sample_columns(ctx, m, t.tags, {1, 0, 0}, 2, &some) == std::vector<U64>{{1, 7}, {2}}));
    const auto empty_call = crgpu::rtl_sample_columns(ctx, m, t.tags, sot, 2, &nobody);
    CHECK(empty_call[0].empty() && empty_call[1].empty());
    CHECK(crgpu::rtl_sample_columns(ctx, m, t.tags, {0xFF, 0xFF, 0xFF}, 1)[0].empty());  // no tag with a sample: nothing to free

    // medians per probe rank over all nine cells: probe 0 has 10 12 15 18 (even: (12 + 15) / 2), probe 1 has 11 13 16, probe 2 has 14 17
    const std::vector<uint32_t> sums = {10, 11, 12, 13, 14, 15, 16, 17, 18};
    const auto med = crgpu::rtl_medians(ctx, m, sums, cells, 3);
    CHECK((med.n_nonzero == U64{4, 3, 2}) && (med.median == U64{13, 13, 15}));
    // the antibody part: tags 0 1 2 = AB001 BC001 BC002; every probe rank's counts are reverse-translated to AB001
    const std::vector<uint8_t> kind = {CRGPU_RTL_KIND_ANTIBODY, CRGPU_RTL_KIND_RTL, CRGPU_RTL_KIND_RTL};
    crgpu::RtlMedians m1;
    m1.n_nonzero = {4, 0, 0}, m1.median = {25, 0, 0};
    crgpu::RtlAntibody ab;
    ab.ab_tag_of_probe = {0, 0, 0};
    ab.ab_min_count = crgpu::rtl_ab_thresholds(m1, {0, 1, 2}, kind);
    CHECK((ab.ab_min_count == U64{3, UINT64_MAX, UINT64_MAX}));
    ab.ab_min_count[0] = 30;   // GEM 0: 10 + 11 = 21; GEM 1: 12; GEM 2: 13 + 14 = 27; GEM 3: 15 + 16 + 17 = 48; GEM 4: 18
    ab.ab_sums = sums;
    // probe 0 -> tag 1, probes 1 and 2 -> tag 2; the cells are columns 0 (GEM 0, tag 1) and 7 (GEM 3, tag 2)
    const auto ra = crgpu::rtl_gem_runs(ctx, m, {1, 2, 1, 2, 2, 1, 2, 2, 1}, 3, {0, 7}, &ab);
    CHECK(ra.gems_per_tag[0] == 1 && ra.gems_per_tag[1] == 1 && ra.gems_per_tag[2] == 1 && ra.present[0] && ra.present[1] && ra.present[2]);
    CHECK(ra.common[0 * 64 + 2] == 1 && ra.common[0 * 64 + 1] == 0 && ra.common[1 * 64 + 2] == 0);
    const auto sus = crgpu::rtl_suspicious_pairings(crgpu::rtl_overlap_rows(ra), kind, {-1, 0, -1});   // BC001 is paired with AB001
    CHECK(sus.size() == 1 && sus[0].tag1 == 2 && sus[0].tag2 == 0 && sus[0].gems1 == 1 && sus[0].gems2 == 1 && sus[0].common_gems == 1 &&
          sus[0].overlap == 1.0);

    const auto rem = crgpu::remove_high_occupancy_gems(ctx, m, cells, 1);
    CHECK((rem.kept == U64{2, 8}));
    CHECK(rem.summary.high_occupancy_gems == 3 && rem.summary.cells_in_high_occupancy_gems == 7 && rem.summary.n_kept == 2);
    CHECK(rem.summary.fraction_cell_gems_high_occupancy == 3.0 / 5.0 && rem.summary.fraction_cells_in_high_occupancy_gems == 7.0 / 9.0);
    const auto none = crgpu::remove_high_occupancy_gems(ctx, m, {}, 1);
    CHECK(none.kept.empty() && std::isnan(none.summary.fraction_cell_gems_high_occupancy));

    // a cell subset: only GEM 3 keeps all three tags
    const auto r2 = crgpu::rtl_gem_runs(ctx, m, t.tags, 3, {2, 5, 6, 7});
    CHECK(r2.gems_per_tag[0] == 2 && r2.gems_per_tag[1] == 1 && r2.gems_per_tag[2] == 1 && r2.common[0 * 64 + 1] == 1 && r2.gems_with_cells == 2);
    crgpu_matrix_dev_free(ctx.get(), m);
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all tests passed\n");
    return 0;
}
