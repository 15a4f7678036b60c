// The sizing arithmetic of the barcode stage (cellranger_amd/csrc/barcode_plan.h: the first section of barcode.hip) at pinned values: the staging batch, the
// sampling batch, the miss-record capacity, the rank bits, the table mode, the plan of the counted table rounds and the rule
// of pass B's barcode-order path.  Equal values mean equal requests to the context's pool, which matches exact sizes.
// Build: g++ -std=c++17 -Icellranger_amd/csrc tests/cpp/test_barcode_plan.cpp   (see tests/test_barcode_plan.py)
#include <cstdio>

#include "barcode_plan.h"

static int g_fail = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); \
            g_fail++;                                                      \
        }                                                                  \
    } while (0)

static const uint64_t G = 1000000000ull;  // the headline's reads

struct List {  // what plan_rank_bits and plan_k2_sorted read of a context
    uint32_t n_canon;
};
static uint32_t rank_bits(uint32_t n_canon) {
    const List l{n_canon};
    return plan_rank_bits(&l);
}
static bool k2_sorted(bool use_rec, bool uniform, bool buffers, uint64_t entries, const char *env, uint32_t n_canon) {
    const List l{n_canon};
    return plan_k2_sorted(use_rec, uniform, buffers, entries, env, &l);
}

static void test_constants() {
    CHECK(BIN_SIZE == 32768u && MB_TILE == 4096 && MB_MAX_BUCKETS == 1024 && SI_MISS_BUCKET == 31u);
    CHECK(MB_STAGE_BUDGET == (8ull << 30) && HC_MAX_RANK_BITS == 24u && LH_REGIONS == 4096u);
    CHECK(LH_FULL == 0 && LH_SPLIT == 1 && LH_HOTCNT == 3);
}

static void test_staging() {
    const struct {
        uint32_t n_buckets;
        uint64_t n, sb;
        uint32_t slices;
    } rows[] = {{23, G, 186736640ull, 22},        {1, 5000, 8192, 512},         {31, 1ull << 20, 1048576, 16},
                {32, 1ull << 20, 1048576, 16}, {208, G, 20647936ull, 2}, {1024, G, 4194304ull, 1}};
    for (const auto &r : rows) {
        const StagePlan s = plan_staging(r.n_buckets, r.n);
        CHECK(s.sb == r.sb && s.slices == r.slices);
        CHECK(s.sb % MB_TILE == 0);
    }
}

static void test_sampling_batch_and_records() {
    CHECK(plan_sampling_batch(G) == 4194304ull);
    CHECK(plan_sampling_batch(1ull << 20) == 262144ull);
    // H = 995805696, 7 launches: 995805696 / 4096 / 3 = 81038, + 2048 + 7 * 512
    CHECK(plan_miss_record_cap(G, 4194304ull, 186736640ull) == 86670u);
}

static void test_rank_bits_and_mode() {
    CHECK(rank_bits(737280u) == 20u);
    CHECK(rank_bits((1u << 24) - 1u) <= HC_MAX_RANK_BITS);  // LH_HOTCNT allowed
    CHECK(rank_bits(1u << 24) > HC_MAX_RANK_BITS);          // ... and refused
    CHECK(rank_bits((1u << 24) - 1u) == 24u && rank_bits(1u << 24) == 25u);
    CHECK(plan_table_mode(nullptr, 20, 23) == LH_HOTCNT);
    CHECK(plan_table_mode(nullptr, 25, 32) == LH_SPLIT);
    CHECK(plan_table_mode(nullptr, 25, 31) == LH_FULL);
    CHECK(plan_table_mode("1", 20, 23) == LH_SPLIT);
    CHECK(plan_table_mode("0", 20, 23) == LH_FULL);
}

static void test_round_plan() {
    const uint64_t sb = 186736640ull, first = 4194304ull;
    const struct {
        double cold_frac;
        uint64_t round, cap;
        bool counted;
    } rows[] = {{0.0, 995807232ull, 12219, true}, {0.05, 995807232ull, 24375, true}, {0.10, 905969664ull, 44300, true},
                {0.30, 0, 0, false},              {0.50, 0, 0, false}};
    for (const auto &r : rows) {
        const RoundPlan p = plan_table_rounds(r.cold_frac, sb, G, first, sb, nullptr);
        CHECK(p.counted == r.counted);
        if (r.counted) CHECK(p.round == r.round && p.cap == r.cap);
    }
    RoundPlan p = plan_table_rounds(0.10, 1048576, 1ull << 20, 262144, 1048576, nullptr);
    CHECK(p.counted && p.round == 786432ull && p.cap == 102ull);
    p = plan_table_rounds(0.10, 20000768ull, 20000000ull, 4194304ull, 20000768ull, nullptr);
    CHECK(p.counted && p.round == 15806464ull && p.cap == 835ull);
    // a forced cap replaces cap: the rounds stay on while all regions fit into one bucket of the staging area
    uint64_t forced = 8;
    p = plan_table_rounds(0.10, sb, G, first, sb, &forced);
    CHECK(p.counted && p.round == 905969664ull && p.cap == 8ull);
    forced = sb / LH_REGIONS;  // 45590: 45590 * 4096 <= 186736640
    CHECK(plan_table_rounds(0.10, sb, G, first, sb, &forced).counted);
    forced = sb / LH_REGIONS + 1;
    p = plan_table_rounds(0.10, sb, G, first, sb, &forced);
    CHECK(!p.counted && p.cap == forced);
    // a staging area of 128 entries per region or fewer: no counted rounds
    CHECK(!plan_table_rounds(0.10, 128ull * LH_REGIONS, 1ull << 20, 262144, 128ull * LH_REGIONS, nullptr).counted);
}

static void test_k2_sorted_rule() {
    const uint64_t entries = 4096ull * 86670ull;
    CHECK(!k2_sorted(true, true, true, entries, nullptr, 1u << 21));
    CHECK(k2_sorted(true, true, true, entries, nullptr, (1u << 21) + 1u));
    CHECK(!k2_sorted(true, true, true, entries, "0", (1u << 21) + 1u));
    CHECK(k2_sorted(true, true, true, entries, "1", 1000u));
    // the switch forces nothing that the call cannot do
    CHECK(!k2_sorted(false, true, true, entries, "1", 1u << 22));
    CHECK(!k2_sorted(true, false, true, entries, "1", 1u << 22));
    CHECK(!k2_sorted(true, true, false, entries, "1", 1u << 22));
    CHECK(!k2_sorted(true, true, true, 0xFFFFFFFFull, "1", 1u << 22));
    CHECK(k2_sorted(true, true, true, 0xFFFFFFFEull, "1", 1u << 22));
}

int main() {
    test_constants();
    test_staging();
    test_sampling_batch_and_records();
    test_rank_bits_and_mode();
    test_round_plan();
    test_k2_sorted_rule();
    if (g_fail) {
        std::fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    std::printf("all tests passed\n");
    return 0;
}
