// test_perturbation_kernels.hip -- the two kernels of the MEASURE_PERTURBATIONS bootstrap by direct launch into guarded buffers, at
// constructed shapes.  The sums are integers: the device must EQUAL the host model, there is no bound.
//
//   k_pb_draws (cellranger_amd/csrc/perturbations.h), through pb_order_tasks / pb_launch_draws, against a host model that walks the
//       positions q = 0 .. n - 1 of every draw in order with a host Philox4x64-10 and a 128-bit multiply-high.  One launch holds columns
//       of n = 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, LDS_CELLS and LDS_CELLS + 1 cells (30 % dense), a column of zeros, a column with a
//       count in every cell, and five cells of 2^31 - 1, whose sum needs more than 32 bits.  Every launch is made with lds_cells =
//       LDS_CELLS (all but the last size staged in LDS) and with lds_cells = 1 (every column of two cells or more read from global
//       memory); B in {1, 2, 9} with draws_per_wg in {1, 4, 8}: a chunk boundary falls on, before and after the last draw.
//   k_pb_gather against the dense columns built on the host: a gene with 0, 1, 64 and 65 entries in the group, the first and the last
//       gene, the first and the last group, a gene present only outside the group, a gene in every cell, the entries of cells in no
//       group behind the last gene.  The pool is filled with 0xFF bytes first, so a word that was not written shows.
//   The host Philox is checked against words recorded from np.random.Philox(counter=[0, s, 0, 0], key=[11, 0]).random_raw().
//
// The production text is compiled here inside a namespace under cellranger_amd.build.FLAGS; the context and the pool come from
// libcrgpu.so.
//   test_perturbation_kernels --host-only              the host model against the recorded words and the built shapes, no device
//   test_perturbation_kernels --group draws|gather     the cases of a group on the device
#include <algorithm>
#include <chrono>
#include <cmath>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "kernel_test.h"

// sseq.h, sseq_pair.h and perturbations.h DEFINE the opaque types of their entry points; inside the namespace those are other types than
// the ones include/crgpu.h declares, so the entry points that take them get names of their own here (the program calls none of them)
#define crgpu_sseq_params_dev under_test_sseq_params_dev
#define crgpu_sseq_params_free under_test_sseq_params_free
#define crgpu_sseq_params_get under_test_sseq_params_get
#define crgpu_sseq_diffexp_dev under_test_sseq_diffexp_dev
#define crgpu_sseq_pairs_create_dev under_test_sseq_pairs_create_dev
#define crgpu_sseq_pairs_free under_test_sseq_pairs_free
#define crgpu_sseq_pair_dev under_test_sseq_pair_dev
#define crgpu_sseq_pair_bootstrap_dev under_test_sseq_pair_bootstrap_dev
namespace pb_under_test {
#include "perturbations.h"
}
using namespace pb_under_test;

// ---- the host model -------------------------------------------------------------------------------------------------------------------
static uint64_t mulhi64(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }
static void philox_host(uint64_t c0, uint64_t c1, uint64_t k0, uint64_t w[4]) {
    uint64_t c2 = 0, c3 = 0, k1 = 0;
    for (int r = 0; r < 10; r++) {
        const uint64_t hi0 = mulhi64(0xD2E7470EE14C6C93ull, c0), lo0 = 0xD2E7470EE14C6C93ull * c0;
        const uint64_t hi1 = mulhi64(0xCA5A826395121157ull, c2), lo1 = 0xCA5A826395121157ull * c2;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += 0x9E3779B97F4A7C15ull, k1 += 0xBB67AE8584CAA73Bull;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}
static uint64_t stream_word(uint64_t seed, uint64_t s, uint32_t q) {
    uint64_t w[4];
    philox_host(1ull + (q >> 2), s, seed, w);
    return w[q & 3u];
}
static uint64_t model_sum(const uint32_t *col, uint32_t n, uint64_t seed, uint64_t s) {
    uint64_t sum = 0;
    for (uint32_t q = 0; q < n; q++) sum += col[mulhi64(stream_word(seed, s, q), n)];
    return sum;
}
static void check_recorded_words() {
    // np.random.Philox(counter=[0, (3 << 33) | (1 << 32) | 7, 0, 0], key=[11, 0]).random_raw(8) and the indices (w * 8) >> 64
    const uint64_t want[8] = {0xf924fa6b47b8dc7bull, 0x469a4719c831bda5ull, 0x6300f5c4dc7e703cull, 0xae02a6f92279dfb9ull,
                              0xbb56cbc36031517full, 0xf06b7f7ea3a43bfeull, 0x663af7675eef5502ull, 0x7ac83acc7f890937ull};
    const uint32_t want_idx[8] = {7, 2, 3, 5, 5, 7, 3, 3};
    const uint64_t s = (3ull << 33) | (1ull << 32) | 7ull;
    for (uint32_t q = 0; q < 8u; q++) {
        if (stream_word(11, s, q) != want[q]) die("host Philox: word %u is %016llx, numpy gives %016llx", q, (unsigned long long)stream_word(11, s, q), (unsigned long long)want[q]);
        if (mulhi64(want[q], 8) != want_idx[q]) die("multiply-high of word %u", q);
    }
    // the sums of draws 0, 1, 2 of side a of stream 3 over the column 1 .. 7 (tests/perturbations_numpy.bootstrap_sums)
    const uint32_t col[7] = {1, 2, 3, 4, 5, 6, 7};
    const uint64_t want_sum[3] = {26, 36, 30};
    for (uint32_t b = 0; b < 3u; b++)
        if (model_sum(col, 7, 11, (3ull << 33) | b) != want_sum[b]) die("model sum of draw %u", b);
    case_done("host Philox4x64-10 and the model sum: the words numpy recorded");
}

// ---- k_pb_draws ----------------------------------------------------------------------------------------------------------------------
static const uint32_t LDS_CELLS = 300;
enum ColKind { C_SPARSE, C_ZEROS, C_FULL, C_BIG };
struct ColSpec {
    uint32_t n;
    ColKind kind;
};
static const ColSpec COLS[] = {{1, C_SPARSE},   {3, C_SPARSE},   {4, C_SPARSE},   {5, C_SPARSE},         {63, C_SPARSE},            {64, C_SPARSE}, {65, C_SPARSE},
                               {255, C_SPARSE}, {256, C_SPARSE}, {257, C_SPARSE}, {LDS_CELLS, C_SPARSE}, {LDS_CELLS + 1u, C_SPARSE}, {65, C_ZEROS},  {257, C_FULL},
                               {5, C_BIG},      {LDS_CELLS + 1u, C_FULL}};
static const uint32_t N_COLS = sizeof(COLS) / sizeof(COLS[0]);

static void group_draws() {
    Rng rng(7);
    const uint64_t seed = 0x1234567887654321ull;
    std::vector<uint32_t> pool;
    std::vector<PbTask> tasks;
    for (uint32_t c = 0; c < N_COLS; c++) {
        // large streams and side 1 as well: the bits 32 and 33 .. 63 of the counter word (bit 31 of a stream is shifted out)
        const uint64_t s = ((uint64_t)(c % 3u == 2u ? 0xFFFFFFF0u + c : c) << 33) | ((uint64_t)(c & 1u) << 32);
        tasks.push_back(PbTask{pool.size(), s, COLS[c].n, c});
        for (uint32_t i = 0; i < COLS[c].n; i++) {
            uint32_t v = 0;
            switch (COLS[c].kind) {
            case C_SPARSE: v = rng.unit() < 0.3 ? 1u + (uint32_t)rng.below(1000) : 0u; break;
            case C_ZEROS: v = 0u; break;
            case C_FULL: v = 1u + (uint32_t)rng.below(50000); break;
            case C_BIG: v = 0x7FFFFFFFu; break;
            }
            pool.push_back(v);
        }
    }
    for (uint32_t B : {1u, 2u, 9u}) {
        std::vector<unsigned long long> model((uint64_t)N_COLS * B);
        for (uint32_t c = 0; c < N_COLS; c++)
            for (uint32_t b = 0; b < B; b++) model[(uint64_t)c * B + b] = model_sum(pool.data() + tasks[c].off, tasks[c].n, seed, tasks[c].s | b);
        if (B == 9u) {
            bool above = false;
            for (uint32_t b = 0; b < B; b++) above |= model[14ull * B + b] > 0xFFFFFFFFull;
            if (!above || model[14ull * B] != 5ull * 0x7FFFFFFFull) die("draws: the column of five 2^31 - 1 does not sum above 32 bits");
            for (uint32_t b = 0; b < B; b++)
                if (model[12ull * B + b] != 0) die("draws: the column of zeros");
        }
        for (uint32_t dpw : {1u, 4u, 8u})
            for (uint32_t lds_cells : {LDS_CELLS, 1u}) {
                std::vector<PbTask> ordered = tasks;
                const uint32_t n_lds = pb_order_tasks(ordered, lds_cells);
                uint32_t expect_lds = 0;
                for (const PbTask &t : tasks) expect_lds += t.n <= lds_cells;
                if (n_lds != expect_lds || n_lds != (lds_cells == 1u ? 1u : N_COLS - 2u)) die("draws: %u tasks take the LDS path at lds_cells = %u", n_lds, lds_cells);
                for (uint32_t i = 0; i < N_COLS; i++)
                    if ((i < n_lds) != (ordered[i].n <= lds_cells)) die("draws: task %u is on the wrong side of the order", i);
                if (!g_host_only) {
                    GBuf<uint32_t> pb(pool);
                    GBuf<PbTask> tb(ordered);
                    GBuf<unsigned long long> ob((uint64_t)N_COLS * B);
                    GOK(pb_launch_draws(g_gpu->ctx, pb.d, tb.d, ordered, n_lds, B, dpw, seed, ob.d));
                    g_gpu->launched("k_pb_draws");
                    GOK(crgpu_synchronize(g_gpu->ctx));
                    same("sums", ob.get("sums"), model);
                    (void)pb.get("pool"), (void)tb.get("tasks");
                }
                case_done("k_pb_draws: B = %u, %u draws per workgroup, lds_cells = %u (%u of %u columns in LDS)", B, dpw, lds_cells, n_lds, N_COLS);
            }
    }
}

// ---- k_pb_gather ---------------------------------------------------------------------------------------------------------------------
static void group_gather() {
    Rng rng(21);
    const uint32_t G = 6, K = 4, CELLS = 130;
    const uint64_t Npos = (uint64_t)K * CELLS;
    // entries of gene g in group k; -1 = a random half
    const int count[G][K] = {{0, 1, 64, 65}, {130, 130, 130, 130}, {0, 0, -1, 0}, {-1, -1, -1, -1}, {0, 0, 0, 0}, {65, -1, 64, 1}};
    std::vector<uint64_t> keys;
    std::vector<uint32_t> vals, dense((uint64_t)G * Npos, 0u);
    for (uint32_t g = 0; g < G; g++)
        for (uint32_t k = 0; k < K; k++) {
            std::vector<uint8_t> has(CELLS, 0);
            if (count[g][k] < 0) {
                for (uint32_t c = 0; c < CELLS; c++) has[c] = rng.unit() < 0.5;
            } else {
                for (int left = count[g][k]; left > 0;) {
                    const uint32_t c = (uint32_t)rng.below(CELLS);
                    if (!has[c]) has[c] = 1, left--;
                }
            }
            if (g == 0u && k == 1u) std::fill(has.begin(), has.end(), 0), has[CELLS - 1u] = 1;  // the single entry in the last cell
            if (g == 5u && k == 3u) std::fill(has.begin(), has.end(), 0), has[0] = 1;           // and in the first
            for (uint32_t c = 0; c < CELLS; c++)
                if (has[c]) {
                    const uint64_t p = (uint64_t)k * CELLS + c;
                    const uint32_t v = 1u + (uint32_t)rng.below(g == 1u ? 4000000000u : 1000u);
                    keys.push_back((uint64_t)g * Npos + p), vals.push_back(v), dense[(uint64_t)g * Npos + p] = v;
                }
        }
    for (uint32_t i = 0; i < 37u; i++) keys.push_back((uint64_t)G * Npos), vals.push_back(0u);  // the entries of cells in no group
    const uint64_t nnz = keys.size();
    if (!std::is_sorted(keys.begin(), keys.end())) die("gather: the keys are not ascending");
    // every (gene, group), in an order that is not the order of the keys
    std::vector<PbCol> cols;
    std::vector<uint32_t> want;
    for (uint32_t j = 0; j < G * K; j++) {
        const uint32_t i = (j * 7u) % (G * K), g = i / K, k = i % K;  // 7 and 24 are coprime
        cols.push_back(PbCol{g, k * CELLS, (k + 1u) * CELLS, 0u, want.size()});
        uint32_t n_in = 0;
        for (uint32_t c = 0; c < CELLS; c++) {
            want.push_back(dense[(uint64_t)g * Npos + (uint64_t)k * CELLS + c]);
            n_in += want.back() != 0u;
        }
        if (count[g][k] >= 0 && n_in != (uint32_t)count[g][k]) die("gather: gene %u has %u entries in group %u, built for %d", g, n_in, k, count[g][k]);
    }
    if (!g_host_only) {
        GBuf<uint64_t> kb(keys);
        GBuf<uint32_t> vb(vals), pool(want.size());
        GBuf<PbCol> cb(cols);
        hipLaunchKernelGGL(k_pb_gather, dim3(((uint32_t)cols.size() + 3u) / 4u), dim3(SQ_WG), 0, (hipStream_t)crgpu_stream(g_gpu->ctx), kb.d, vb.d, nnz, Npos, cb.d,
                           (uint32_t)cols.size(), pool.d);
        g_gpu->launched("k_pb_gather");
        GOK(crgpu_synchronize(g_gpu->ctx));
        same("columns", pool.get("columns"), want);
        (void)kb.get("keys"), (void)vb.get("vals"), (void)cb.get("cols");
    }
    case_done("k_pb_gather: %u columns of %u cells over %llu entries: 0, 1, 64, 65 and 130 entries, first and last gene and group", (uint32_t)cols.size(), CELLS,
              (unsigned long long)nnz);
}

int main(int argc, char **argv) {
    std::string group;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--host-only")) g_host_only = true;
        else if (!std::strcmp(argv[i], "--group") && i + 1 < argc) group = argv[++i];
        else die("usage: test_perturbation_kernels --host-only | --group draws|gather");
    }
    if (!g_host_only && group != "draws" && group != "gather") die("usage: test_perturbation_kernels --host-only | --group draws|gather");
    Gpu *gpu = nullptr;
    if (!g_host_only) g_gpu = gpu = new Gpu();
    if (g_host_only) check_recorded_words();
    if (g_host_only || group == "draws") group_draws();
    if (g_host_only || group == "gather") group_gather();
    delete gpu;
    std::printf("all tests passed (%d cases)\n", g_cases);
    return 0;
}
