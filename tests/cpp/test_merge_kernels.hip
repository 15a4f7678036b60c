// test_merge_kernels.hip -- the two kernels of MERGE_CLUSTERS by direct launch into guarded buffers, at constructed shapes.
//
//   k_sq_pair_row_sums (cellranger_amd/csrc/sseq_pair.h)   against a HOST ORDER MODEL bit for bit (the entry of concatenated index r in lane
//       r % 64, a lane's entries in ascending r, lane 0 of the butterfly 32 .. 1; both sides unfused f64), and against a long double sum in
//       index order within a bound derived here.  The longest path to an output holds: the division val / sf (one rounding; for the sum
//       of squares the product v * v of the ROUNDED v, which the reference squares too: one rounding), ceil(n / 64) additions of the
//       lane's chain of which the first, to 0.0, is exact, and the six additions of the butterfly: 1 + (ceil(n / 64) - 1) + 6 <=
//       n / 64 + 7 roundings, so |dev - ref| <= gamma(n / 64 + 7) * sum |terms| with gamma(k) = k u / (1 - k u), u = 2^-53 (Higham,
//       Accuracy and Stability, 3.1 / 4.2), n the entries of the gene in the pair.  x_a and x_b are integers and must be equal.
//       Shapes: side a of 1, 2 and 3 groups with exactly 0, 1, 63, 64, 65, 127, 128 and 129 entries of a gene, a gene in no cell, a gene
//       only in groups outside the pair, the first and the last gene, the first and the last group, the entries of cells in no group
//       behind the last gene.
//   k_mc_median (cellranger_amd/csrc/merge_clusters.hip)    against std::nth_element at segment sizes 1, 2, 3, 255, 256, 257 and 4097 with
//       all values equal, values that differ in the lowest byte only, in the sign only, negatives, denormals, -0 / +0 and normal values;
//       an exact selection, compared as numbers.
//
// The production text is compiled here inside namespaces under cellranger_amd.build.FLAGS; the context and the pool come from
// libcrgpu.so.
//   test_merge_kernels --host-only              every case without a device: the order model within the bound, the host twin of the radix
//                                               select against std::nth_element
//   test_merge_kernels --group pair|select      the cases of a group on the device
#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "kernel_test.h"

// sseq.h and sseq_pair.h DEFINE the two opaque types of their entry points; inside the namespace those are other types than the ones
// include/crgpu.h declares, so the seven entry points that take them get names of their own here (the program calls none of them)
#define crgpu_sseq_params_dev under_test_sseq_params_dev
#define crgpu_sseq_params_free under_test_sseq_params_free
#define crgpu_sseq_params_get under_test_sseq_params_get
#define crgpu_sseq_diffexp_dev under_test_sseq_diffexp_dev
#define crgpu_sseq_pairs_create_dev under_test_sseq_pairs_create_dev
#define crgpu_sseq_pairs_free under_test_sseq_pairs_free
#define crgpu_sseq_pair_dev under_test_sseq_pair_dev
namespace sseq_under_test {
#include "sseq_pair.h"
}
namespace merge_under_test {
#include "merge_clusters.hip"
}
using namespace sseq_under_test;
using namespace merge_under_test;

static uint64_t bits(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}
static long double gam(uint64_t k) { return (long double)k * 0x1.0p-53L / (1.0L - (long double)k * 0x1.0p-53L); }
// lane 0 of the butterfly 32, 16, 8, 4, 2, 1
static double wave0(const double *in) {
    double x[64], y[64];
    for (int i = 0; i < 64; i++) x[i] = in[i];
    for (int d = 32; d >= 1; d >>= 1) {
        for (int i = 0; i < 64; i++) y[i] = x[i] + x[i ^ d];
        for (int i = 0; i < 64; i++) x[i] = y[i];
    }
    return x[0];
}
static long double g_worst = 0.0L;

// ---- k_sq_pair_row_sums ------------------------------------------------------------------------------------------------------------------
static const uint32_t LENGTHS[8] = {0, 1, 63, 64, 65, 127, 128, 129};
static const uint32_t N_GROUPS = 7, GROUP_CELLS = 140;  // group 6 is never listed

static void pair_case(uint32_t groups_a, uint32_t first_group, uint64_t seed) {
    Rng rng(seed);
    const uint32_t G = 11;  // gene 0 .. 7: LENGTHS entries in side a; 8: in no cell; 9: only outside the pair; 10: everywhere
    const uint64_t Npos = (uint64_t)N_GROUPS * GROUP_CELLS;
    // side a = groups first_group .. + groups_a, side b = the next two groups (cyclic over the groups 0 .. 5)
    std::vector<uint32_t> side;
    for (uint32_t j = 0; j < groups_a + 2u; j++) side.push_back((first_group + j) % 6u);
    std::vector<uint32_t> ga(side.begin(), side.begin() + groups_a), gb(side.begin() + groups_a, side.end());
    std::sort(ga.begin(), ga.end()), std::sort(gb.begin(), gb.end());
    std::vector<SqRun> runs;
    uint32_t base = 0;
    for (uint32_t j = 0; j < ga.size() + gb.size(); j++) {
        const uint32_t k = j < ga.size() ? ga[j] : gb[j - ga.size()];
        runs.push_back(SqRun{k * GROUP_CELLS, (k + 1u) * GROUP_CELLS, base, 0u});
        base += GROUP_CELLS;
    }
    const uint32_t Np = base;
    std::vector<uint8_t> listed(N_GROUPS, 0), in_a(N_GROUPS, 0);
    for (uint32_t k : ga) listed[k] = in_a[k] = 1;
    for (uint32_t k : gb) listed[k] = 1;
    std::vector<double> sf(Np);
    for (double &v : sf) v = 0.25 + 3.0 * rng.unit();
    // the sorted entries
    std::vector<uint64_t> keys;
    std::vector<uint32_t> vals;
    for (uint32_t g = 0; g < G; g++) {
        uint32_t left = g < 8u ? LENGTHS[g] : 0u;  // entries still to place in side a, its first cells in concatenated order
        std::vector<uint8_t> has(Npos, 0);
        for (uint32_t k : ga)
            for (uint32_t c = 0; c < GROUP_CELLS && left; c++, left--) has[(size_t)k * GROUP_CELLS + c] = 1;
        for (uint64_t p = 0; p < Npos; p++) {
            const uint32_t k = (uint32_t)(p / GROUP_CELLS);
            if (g == 8u) continue;
            if (g == 9u) has[p] = !listed[k];
            else if (g == 10u) has[p] = 1;
            else if (!in_a[k]) has[p] = rng.unit() < 0.5;
        }
        for (uint64_t p = 0; p < Npos; p++)
            if (has[p]) keys.push_back((uint64_t)g * Npos + p), vals.push_back(1u + (uint32_t)rng.below(g == 10u ? 4000000u : 1000u));
    }
    for (uint32_t i = 0; i < 37u; i++) keys.push_back((uint64_t)G * Npos), vals.push_back(0u);  // the entries of cells in no group
    const uint64_t nnz = keys.size();

    // the order model and the reference
    std::vector<double> m1(G), m2(G);
    std::vector<unsigned long long> mxa(G, 0), mxb(G, 0);
    std::vector<long double> r1(G, 0.0L), r2(G, 0.0L), a1(G, 0.0L), a2(G, 0.0L);
    std::vector<uint64_t> n_of(G, 0);
    for (uint32_t g = 0; g < G; g++) {
        double l1[64] = {0}, l2[64] = {0};
        uint64_t r = 0;
        for (uint32_t j = 0; j < runs.size(); j++)
            for (uint64_t i = 0; i < nnz; i++) {
                if (keys[i] < (uint64_t)g * Npos + runs[j].lo || keys[i] >= (uint64_t)g * Npos + runs[j].hi) continue;
                const double v = (double)vals[i] / sf[runs[j].base + (uint32_t)(keys[i] - (uint64_t)g * Npos - runs[j].lo)];
                l1[r % 64u] += v, l2[r % 64u] += v * v;
                (j < ga.size() ? mxa[g] : mxb[g]) += vals[i];
                const long double t1 = (long double)vals[i] / (long double)sf[runs[j].base + (uint32_t)(keys[i] - (uint64_t)g * Npos - runs[j].lo)];
                const long double t2 = (long double)v * (long double)v;
                r1[g] += t1, a1[g] += fabsl(t1), r2[g] += t2, a2[g] += fabsl(t2);
                r++;
            }
        m1[g] = wave0(l1), m2[g] = wave0(l2), n_of[g] = r;
    }
    for (uint32_t g = 0; g < 8u; g++) {
        uint64_t in_side_a = 0;
        for (uint64_t i = 0; i < nnz; i++)
            if (keys[i] / Npos == g && in_a[(keys[i] % Npos) / GROUP_CELLS]) in_side_a++;
        if (in_side_a != LENGTHS[g]) die("pair case: gene %u has %llu entries in side a, built for %u", g, (unsigned long long)in_side_a, LENGTHS[g]);
    }
    if (n_of[8] != 0 || n_of[9] != 0 || n_of[10] != Np) die("pair case: the genes 8, 9, 10 are not what they are for");

    std::vector<double> d1 = m1, d2 = m2;
    if (!g_host_only) {
        GBuf<uint64_t> kb(keys);
        GBuf<uint32_t> vb(vals);
        GBuf<SqRun> rb(runs);
        GBuf<double> sb(sf), s1(G), s2(G);
        GBuf<unsigned long long> xa(G), xb(G);
        hipLaunchKernelGGL(k_sq_pair_row_sums, dim3((G + 3u) / 4u), dim3(SQ_WG), 0, (hipStream_t)crgpu_stream(g_gpu->ctx), kb.d, vb.d, nnz, Npos, G, rb.d, (uint32_t)runs.size(),
                           (uint32_t)ga.size(), sb.d, s1.d, s2.d, xa.d, xb.d);
        g_gpu->launched("k_sq_pair_row_sums");
        GOK(crgpu_synchronize(g_gpu->ctx));
        d1 = s1.get("s1"), d2 = s2.get("s2");
        same("s1", d1, m1), same("s2", d2, m2);
        same("x_a", xa.get("x_a"), mxa), same("x_b", xb.get("x_b"), mxb);
        (void)kb.get("keys"), (void)vb.get("vals"), (void)sb.get("sf"), (void)rb.get("runs");
    }
    for (uint32_t g = 0; g < G; g++) {
        const long double b1 = gam(n_of[g] / 64u + 7u) * a1[g], b2 = gam(n_of[g] / 64u + 7u) * a2[g];
        const long double e1 = fabsl((long double)d1[g] - r1[g]), e2 = fabsl((long double)d2[g] - r2[g]);
        if (!(e1 <= b1) || !(e2 <= b2))
            die("pair case: gene %u of %llu entries is %.3Lg / %.3Lg from the reference, the bounds are %.3Lg / %.3Lg", g, (unsigned long long)n_of[g], e1, e2, b1, b2);
        if (b1 > 0.0L) g_worst = std::max(g_worst, std::max(e1 / b1, e2 / b2));
        if (n_of[g] == 0 && (bits(d1[g]) != 0 || bits(d2[g]) != 0)) die("pair case: gene %u has no entry and a sum that is not +0", g);
    }
    case_done("k_sq_pair_row_sums: side a of %u groups from group %u, %llu entries, %u pair cells", groups_a, first_group, (unsigned long long)nnz, Np);
}

static void group_pair() {
    uint64_t seed = 1;
    for (uint32_t groups_a = 1; groups_a <= 3u; groups_a++)
        for (uint32_t first : {0u, 2u, 5u}) pair_case(groups_a, first, seed++);  // 5: side a wraps to the first groups, the last group listed
    std::printf("group pair: the worst deviation is %.3Lg of its bound\n", g_worst);
}

// ---- k_mc_median ---------------------------------------------------------------------------------------------------------------------
enum Kind { K_EQUAL, K_LOW_BYTE, K_SIGN, K_NEGATIVE, K_DENORMAL, K_ZEROS, K_NORMAL, N_KINDS };
static const char *KIND_NAMES[N_KINDS] = {"all equal", "lowest byte", "sign only", "negatives", "denormals", "-0 / +0", "normal"};
static double make_value(Kind kind, Rng &rng) {
    uint64_t b;
    double v;
    switch (kind) {
    case K_EQUAL: return 3.25;
    case K_LOW_BYTE: b = 0x4009000000000000ull | rng.below(256); std::memcpy(&v, &b, 8); return v;
    case K_SIGN: return rng.below(2) ? 1.5 : -1.5;
    case K_NEGATIVE: return -std::fabs(rng.nonzero()) * 1e3;
    case K_DENORMAL: b = (rng.below(2) << 63) | (1ull + rng.below(1ull << 40)); std::memcpy(&v, &b, 8); return v;
    case K_ZEROS: return rng.below(2) ? 0.0 : -0.0;
    default: return rng.normal();
    }
}
static double median_nth(std::vector<double> v) {
    const size_t n = v.size();
    std::nth_element(v.begin(), v.begin() + n / 2, v.end());
    const double hi = v[n / 2];
    if (n % 2) return hi;
    return (*std::max_element(v.begin(), v.begin() + n / 2) + hi) / 2.0;
}
// the host twin of mc_select: eight passes over the bytes of the order-preserving image
static double select_model(const std::vector<double> &x, uint32_t rank) {
    uint64_t prefix = 0;
    for (uint32_t pass = 0; pass < 8u; pass++) {
        const uint32_t shift = 56u - 8u * pass;
        const uint64_t above = pass ? ~0ull << (shift + 8u) : 0ull;
        uint32_t hist[256] = {0};
        for (double v : x)
            if ((mc_key(v) & above) == prefix) hist[(mc_key(v) >> shift) & 255u]++;
        uint32_t run = 0, b = 0;
        for (; b < 255u && rank >= run + hist[b]; b++) run += hist[b];
        prefix |= (uint64_t)b << shift, rank -= run;
    }
    return mc_value(prefix);
}

static void group_select() {
    const uint32_t sizes[7] = {1, 2, 3, 255, 256, 257, 4097};
    for (int kind = 0; kind < N_KINDS; kind++) {
        // one launch per kind: the seven sizes are the clusters, two dimensions
        Rng rng(100 + kind);
        const uint32_t K = 7, d = 2;
        std::vector<uint32_t> start(K + 1, 0);
        for (uint32_t c = 0; c < K; c++) start[c + 1] = start[c] + sizes[c];
        const uint64_t n = start[K];
        std::vector<double> xs(d * n), want(K * d);
        for (double &v : xs) v = make_value((Kind)kind, rng);
        for (uint32_t c = 0; c < K; c++)
            for (uint32_t t = 0; t < d; t++) {
                std::vector<double> seg(xs.begin() + t * n + start[c], xs.begin() + t * n + start[c + 1]);
                want[c * d + t] = median_nth(seg);
                const double hi = select_model(seg, sizes[c] / 2u);
                const double model = sizes[c] % 2u ? hi : (select_model(seg, sizes[c] / 2u - 1u) + hi) / 2.0;
                if (!(model == want[c * d + t])) die("select model, %s, %u values: %.17g, std::nth_element gives %.17g", KIND_NAMES[kind], sizes[c], model, want[c * d + t]);
            }
        if (!g_host_only) {
            GBuf<double> xb(xs), med((uint64_t)K * d);
            GBuf<uint32_t> sb(start);
            hipLaunchKernelGGL(k_mc_median, dim3(K, d), dim3(MC_WG), 0, (hipStream_t)crgpu_stream(g_gpu->ctx), xb.d, n, sb.d, d, med.d);
            g_gpu->launched("k_mc_median");
            GOK(crgpu_synchronize(g_gpu->ctx));
            const std::vector<double> got = med.get("medians");
            (void)xb.get("xs"), (void)sb.get("start");
            for (uint32_t i = 0; i < K * d; i++)
                if (!(got[i] == want[i])) die("k_mc_median, %s, %u values, dimension %u: %.17g (%a), std::nth_element gives %.17g (%a)", KIND_NAMES[kind], sizes[i / d], i % d, got[i], got[i], want[i], want[i]);
        }
        case_done("k_mc_median: %s at 1, 2, 3, 255, 256, 257 and 4097 values", KIND_NAMES[kind]);
    }
    for (double v : {0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 1.7976931348623157e308, -1.7976931348623157e308})
        if (bits(mc_value(mc_key(v))) != bits(v)) die("mc_value(mc_key(%a)) is %a", v, mc_value(mc_key(v)));
    if (!(mc_key(-1.0) < mc_key(-0.0) && mc_key(-0.0) < mc_key(0.0) && mc_key(0.0) < mc_key(5e-324) && mc_key(1.0) < mc_key(2.0) && mc_key(-2.0) < mc_key(-1.0)))
        die("mc_key does not keep the order of the doubles");
    case_done("mc_key / mc_value: the order and the round trip");
}

int main(int argc, char **argv) {
    std::string group;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--host-only")) g_host_only = true;
        else if (!std::strcmp(argv[i], "--group") && i + 1 < argc) group = argv[++i];
        else die("usage: test_merge_kernels --host-only | --group pair|select");
    }
    if (!g_host_only && group != "pair" && group != "select") die("usage: test_merge_kernels --host-only | --group pair|select");
    Gpu *gpu = nullptr;
    if (!g_host_only) g_gpu = gpu = new Gpu();
    if (g_host_only || group == "pair") group_pair();
    if (g_host_only || group == "select") group_select();
    delete gpu;
    std::printf("all tests passed (%d cases)\n", g_cases);
    return 0;
}
