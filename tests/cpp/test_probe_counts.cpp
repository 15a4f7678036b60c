// C++ host-mirror test of BarcodeDupMarker::probe_counts (include/crgpu.hpp): BcUmiInfo::probe_counts
// (cr_types/src/types.rs:190-204) of a hand-computed batch of two barcodes, as ProbeBarcodeCount entries
// (types.rs:141-146) in (barcode, probe_idx) order.
// Build: g++ -std=c++17 -Iinclude tests/cpp/test_probe_counts.cpp -Lcellranger_amd -lcrgpu   (see tests/test_gpu_probe_counts_cpp.py)
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

using crgpu::BarcodeCorrector;
using crgpu::SimpleHistogram;
using crgpu::Whitelist;
using Qual = std::vector<uint8_t>;

static bool same(const crgpu::ProbeBarcodeCount &c, uint32_t barcode, uint32_t probe, uint32_t count) {
    return c.barcode == barcode && c.probe_idx == probe && c.umi_count == count;
}

static void test_probe_counts_of_two_barcodes() {
    crgpu::Context ctx(0);
    BarcodeCorrector corrector(ctx, 0, Whitelist::plain({"ACGTACGTACGTACGT", "TTTTACGTACGTACGT"}), SimpleHistogram{});
    std::vector<std::string> seen(7, "ACGTACGTACGTACGT");
    seen.insert(seen.end(), 3, "TTTTACGTACGTACGT");
    corrector.check_and_update(seen);
    const Qual q(4, 'I');
    const uint32_t g0 = 0, g1 = 1, g2 = 2;
    // every UMI differs from every other in at least three bases and no UMI occurs with two features: one molecule per
    // (barcode, feature, UMI), no correction, no low support.  The probes are NOT ordered like the features.
    crgpu::DupBuilder b(ctx, 3, 4);
    // barcode 0: six molecules -> probe 2: 2 molecules, probe 5: 3 molecules, one without a probe
    b.observe(0, 0, "ACGT", q, g0, true, 5);
    b.observe(0, 0, "ACGT", q, g0, true, 5);  // a second read of the same molecule
    b.observe(0, 0, "CATG", q, g0, true, 2);
    b.observe(0, 0, "GTAC", q, g1, true, 5);
    b.observe(0, 0, "TGCA", q, g2);           // CRGPU_NO_PROBE
    b.observe(0, 0, "AGAG", q, g2, true, 2);
    b.observe(0, 0, "CTCT", q, g1, true, 5);
    // barcode 1: three molecules -> probe 0: 1, probe 7: 2
    b.observe(1, 0, "ACGT", q, g2, true, 7);
    b.observe(1, 0, "CATG", q, g0, true, 7);
    b.observe(1, 0, "GTAC", q, g1, true, 0);
    const crgpu::BarcodeDupMarker m = b.build();
    CHECK(m.umi_counts.size() == 9);
    CHECK(m.probe_counts.size() == 4);
    if (m.probe_counts.size() == 4) {
        CHECK(same(m.probe_counts[0], 0, 2, 2));
        CHECK(same(m.probe_counts[1], 0, 5, 3));
        CHECK(same(m.probe_counts[2], 1, 0, 1));
        CHECK(same(m.probe_counts[3], 1, 7, 2));
    }
    // without probes the histogram stays empty and nothing else changes
    crgpu::DupBuilder plain(ctx, 3, 4);
    plain.observe(0, 0, "ACGT", q, g0);
    plain.observe(1, 0, "CATG", q, g1);
    const crgpu::BarcodeDupMarker p = plain.build();
    CHECK(p.umi_counts.size() == 2 && p.feature_counts.size() == 2 && p.probe_counts.empty());
}

int main() {
    try {
        test_probe_counts_of_two_barcodes();
    } catch (const std::exception &e) {
        std::fprintf(stderr, "unexpected exception: %s\n", e.what());
        return 2;
    }
    if (g_fail) return 1;
    std::printf("all tests passed\n");
    return 0;
}
