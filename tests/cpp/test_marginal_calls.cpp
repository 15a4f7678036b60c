// C++ host-mirror test of the marginal caller (include/crgpu.hpp): the seed hook and the contaminant rule on the host; on the device a
// small well with planted guides among gene rows: the planted cells are called, a row without an entry is skipped, a row of one distinct
// value calls every cell that holds it, two runs agree bit for bit, the refusals.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_marginal_calls.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_marginal_calls_cpp.py)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

typedef std::vector<uint32_t> U32;

static void test_host_functions() {
    double u[30];
    uint64_t first[10];
    CHECK(crgpu_marginal_seed_draws(1000, u, first) == CRGPU_OK);
    CHECK(u[0] == 0.5488135039273248 && u[1] == 0.7151893663724195 && u[2] == 0.6027633760716439);  // RandomState(0)
    CHECK(first[0] == 548 && first[1] == 544);                                                      // u[0], u[3] = 0.5448... of 1000 cells
    for (int j = 0; j < 10; j++) CHECK(first[j] < 1000 && u[3 * j] >= 0.0 && u[3 * j] < 1.0);
    CHECK(crgpu_marginal_seed_draws(0, u, first) == CRGPU_EINVAL);
    // three tags over four cells: tag 1 is constant (every correlation with it is NaN) and 50-fold below; tag 2 follows tag 0
    const uint64_t c[3][4] = {{2700, 0, 2700, 0}, {15, 15, 15, 15}, {1350, 0, 1350, 3}};
    uint64_t sx[3] = {0, 0, 0}, sxx[3] = {0, 0, 0}, sxy[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            sxy[i * 3 + j] = 0;
            for (int v = 0; v < 4; v++) sxy[i * 3 + j] += c[i][v] * c[j][v];
        }
    for (int i = 0; i < 3; i++) {
        for (int v = 0; v < 4; v++) sx[i] += c[i][v];
        sxx[i] = sxy[i * 3 + i];
    }
    const uint32_t order[3] = {0, 1, 2};
    uint8_t flags[3];
    int32_t src[9];
    CHECK(crgpu_tag_contaminants(3, 4, sx, sxx, sxy, order, 10, 50.0, 0.5, flags, src) == CRGPU_OK);
    CHECK(flags[0] == 0 && flags[1] == 1 && flags[2] == 1 && src[0] == -1 && src[3] == -1 && src[6] == 0 && src[7] == -1);
    const uint32_t twice[3] = {0, 0, 2};
    CHECK(crgpu_tag_contaminants(3, 4, sx, sxx, sxy, twice, 10, 50.0, 0.5, flags, src) == CRGPU_EINVAL);
}

static void test_device() {
    crgpu::Context ctx(0);
    const uint32_t V = 200, NF = 9, n_wl = 256;
    U32 wl(n_wl);
    for (uint32_t i = 0; i < n_wl; i++) wl[i] = i;  // packed 16-mers, ascending: column k is barcode k
    ctx.check(crgpu_set_whitelist_packed(ctx.get(), 0, wl.data(), n_wl, 16, wl.data(), n_wl, nullptr));
    U32 valid(n_wl, 0), corrected(n_wl, 0);
    for (uint32_t c = 0; c < V; c++) valid[c] = 1;
    ctx.check(crgpu_set_counts(ctx.get(), 0, CRGPU_COUNTS_VALID, valid.data()));
    ctx.check(crgpu_set_counts(ctx.get(), 0, CRGPU_COUNTS_CORRECTED, corrected.data()));
    // rows 0, 2, 3, 5, 8: genes.  Row 1: a guide in every fourth cell (40 .. 70 UMIs) over a background of 0 / 1.  Row 4: no entry.
    // Row 6: the value 5 in every fifth cell, nothing else.  Row 7: a second guide in cells 10 .. 29.
    std::vector<U32> dense(NF, U32(V, 0));
    for (uint32_t c = 0; c < V; c++) {
        for (uint32_t f : {0u, 2u, 3u, 5u, 8u}) dense[f][c] = (c * 7 + f * 3) % 5;
        dense[1][c] = c % 4 == 0 ? 40 + (c * 13) % 31 : (c % 3 == 0 ? 1 : 0);
        dense[6][c] = c % 5 == 0 ? 5 : 0;
        dense[7][c] = c >= 10 && c < 30 ? 25 + c : (c % 7 == 0 ? 2 : 0);
    }
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
    CHECK(m->n_barcodes == V);

    const U32 rows = {1, 4, 6, 7};
    const auto a = crgpu::marginal_calls(ctx, m, rows, NF, 3);
    const auto b = crgpu::marginal_calls(ctx, m, rows, NF, 3);
    CHECK(a.rows.size() == 4 && a.indptr.size() == 5 && a.features_per_cell.size() == V);
    CHECK(std::memcmp(a.rows.data(), b.rows.data(), 4 * sizeof(crgpu_marginal_row)) == 0 && a.indptr == b.indptr && a.columns == b.columns &&
          a.features_per_cell == b.features_per_cell);
    // row 1: exactly the planted cells; the lowest count among them is the observed threshold
    CHECK(a.rows[0].status == CRGPU_MC_FITTED && a.rows[0].cells_assigned == 50 && a.rows[0].umi_threshold_observed == 40);
    CHECK(a.rows[0].mean_high > 1.6 && a.rows[0].mean_low < 0.2 && std::fabs(a.rows[0].weight_high - 0.25) < 0.01 && a.rows[0].n_distinct > 3);
    for (int64_t e = a.indptr[0]; e < a.indptr[1]; e++) CHECK(a.columns[e] == 4 * (uint32_t)(e - a.indptr[0]));
    // row 4: nothing to fit
    CHECK(a.rows[1].status == CRGPU_MC_SKIPPED && a.rows[1].cells_assigned == 0 && a.rows[1].umi_threshold_observed == -1 && a.rows[1].total_umis == 0);
    // row 6: one distinct non-zero value, 5 >= 3: every cell that holds it
    CHECK(a.rows[2].status == CRGPU_MC_FITTED && a.rows[2].cells_assigned == 40 && a.rows[2].n_distinct == 2 && a.rows[2].umi_threshold_observed == 5);
    CHECK(a.rows[2].total_umis == 200 && std::fabs(a.rows[2].mean_high - std::log10(6.0)) < 1e-12 && a.rows[2].mean_low == 0.0);
    // row 7: cells 10 .. 29
    CHECK(a.rows[3].cells_assigned == 20 && a.rows[3].umi_threshold_observed == 35);
    for (int64_t e = a.indptr[3]; e < a.indptr[4]; e++) CHECK(a.columns[e] == 10 + (uint32_t)(e - a.indptr[3]));
    uint64_t n0 = 0, n1 = 0, nm = 0;
    for (uint32_t c = 0; c < V; c++) {
        const uint32_t want = (c % 4 == 0) + (c % 5 == 0) + (c >= 10 && c < 30);
        CHECK(a.features_per_cell[c] == want);
        (want == 0 ? n0 : want == 1 ? n1 : nm)++;
    }
    CHECK(a.cells_with_0 == n0 && a.cells_with_1 == n1 && a.cells_with_many == nm);
    // with umi_threshold 6 the value 5 is never called
    const auto hi = crgpu::marginal_calls(ctx, m, rows, NF, 6);
    CHECK(hi.rows[2].status == CRGPU_MC_FITTED && hi.rows[2].cells_assigned == 0 && hi.rows[2].umi_threshold_observed == -1 && hi.rows[0].cells_assigned == 50);
    // refusals
    for (const auto &bad : {std::make_pair(U32{1, 4, 6, 7}, 0u), std::make_pair(U32{4, 1}, 1u), std::make_pair(U32{1, NF}, 1u)}) {
        int code = 0;
        try {
            crgpu::marginal_calls(ctx, m, bad.first, NF, bad.second);
        } catch (const crgpu::Error &e) {
            code = e.code;
        }
        CHECK(code == CRGPU_EINVAL);
    }
    // the contaminant rule through the moments of the device: row 1 has 2 750 UMIs or more; row 4 none (dropped); rows 6 and 7 have 200
    // and 942 (< 1000), and no pair is correlated
    const auto tc = crgpu::tag_contaminants(ctx, m, rows, NF, {0, 1, 2, 3});
    CHECK(tc.flags.size() == 4 && tc.flags[0] == 0 && tc.flags[1] == 2 && tc.flags[2] == 1 && tc.flags[3] == 1);
    CHECK(a.rows[3].total_umis == 942 && a.rows[0].total_umis >= 2750);
    for (const auto &s : tc.sources) CHECK(s.empty());
    crgpu_matrix_dev_free(ctx.get(), m);
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
