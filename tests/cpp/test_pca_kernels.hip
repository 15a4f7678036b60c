// test_pca_kernels.hip -- the kernels of cellranger_amd/csrc/pca.hip one by one, at constructed shapes, each f64 output against two
// references: an ORDER MODEL (a host loop that takes the steps of the device code in its order: a lane's serial chain, the butterfly
// 32 .. 1, the partials ascending; both sides are unfused f64, so the bits must agree) and a PLAIN REFERENCE of the operation itself
// (long double, index order, written from the definition), from which the device may differ by a bound derived here:
//
//     a sum of products whose longest path to the output holds d additions:   |dev - ref| <= gamma(d + 1) * sum |terms|,
//     gamma(k) = k u / (1 - k u), u = 2^-53   (one rounding for the product, one per addition; Higham, Accuracy and Stability, 3.1 / 4.2)
//     plus the reference's own error (n + 2) * 2^-64 * sum |terms|  (n terms in long double: a product and at most n additions each).
//     d = ceil(n / 64) + 6 for a wave sum (the lane's chain, six butterfly steps), PCA_PART_ROWS / 64 + 6 + n_parts for a dot (a lane
//     of k_pca_dots always makes its four additions, of an exact 0 where the rows have run out).
//
// The kernels, pca_prepare, pca_scale, pca_regather and PcaLanczos are file-local, so this program compiles the production text
// itself, inside a namespace: the same text under the same flags (the wrapper takes them from cellranger_amd.build.FLAGS), not the
// library's object code.  The context, the pool and the radix sort come from libcrgpu.so.  (The namespace keeps the 17 kernels apart
// from the library's; the four extern "C" host functions of pca.hip keep their names, this program calls none of them.)
//
//   test_pca_kernels --host-only                               every case without a device: the order model within the bound of the
//                                                              reference, libm's log2 within LIBM_LOG2_ULPS of the rounded log2l
//   test_pca_kernels --group prepare|operator|dense|project    the cases of a group on the device
//
// One line per case, the worst deviation-to-bound ratio per group, "all tests passed" at the end; the first mismatch or HIP error
// prints the case and ends the program with status 1 (nothing is launched after it).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <memory>
#include <numeric>
#include <vector>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "kernel_test.h"

namespace pca_under_test {
#include "pca.hip"
}
using namespace pca_under_test;

// libm's log2(1.0 + x) against the rounded log2l(1.0L + x) over every logged case of this program, in ulps of the result, measured
// with --host-only (which asserts it).  The argument 1.0 + x is rounded to f64 before the logarithm, as numpy's log2(1 + m) rounds
// it, and for x << 1 that rounding alone moves the result by about 2^-53 / (x ln 2), many ulps of a small logarithm: hence the size
// of the figure.  The device gets 4 times the figure, floored at 1 ulp.  A second, sharper figure leaves that rounding out: libm
// against the rounded log2l of the f64 sum 1.0 + x, the argument the device's log2 is given as well; the device gets 4 times it too.
#ifndef LIBM_LOG2_ULPS
#define LIBM_LOG2_ULPS 86
#endif
#ifndef LIBM_LOG2_ARG_ULPS
#define LIBM_LOG2_ARG_ULPS 1
#endif
#define DEV_LOG2_ULPS (4 * LIBM_LOG2_ULPS > 1 ? 4 * LIBM_LOG2_ULPS : 1)
#define DEV_LOG2_ARG_ULPS (4 * LIBM_LOG2_ARG_ULPS > 1 ? 4 * LIBM_LOG2_ARG_ULPS : 1)

static const uint32_t WV = CR_WAVE;             // lanes of a wave
static const uint32_t WG = PCA_WG;              // threads of the fixed-size launches
static const uint32_t PR = PCA_PART_ROWS;       // rows of a partial of the dots
static const uint32_t PC = PCA_PROJ_CHUNK;      // components a pass of the projection keeps in registers
static const uint32_t WPW = PCA_WG / CR_WAVE;   // waves of a workgroup of the dots

static uint64_t bits(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}
enum VecKind { VEC_NORMAL = 0, VEC_DECADES = 1, VEC_UNIT = 2 };
static const char *VEC_NAMES[3] = {"normal", "decades", "unit"};
// VEC_DECADES: alternating signs over twelve decades, so that the order of a sum shows in its bits
static std::vector<double> make_vec(uint64_t n, VecKind kind, uint64_t unit_at, Rng &rng) {
    std::vector<double> v(n, 0.0);
    for (uint64_t i = 0; i < n; i++) {
        if (kind == VEC_NORMAL) v[i] = rng.normal();
        else if (kind == VEC_DECADES) v[i] = ((i & 1u) ? -1.0 : 1.0) * (1.0 + rng.unit()) * std::pow(10.0, (double)(int)(i % 13u) - 6.0);
    }
    if (kind == VEC_UNIT) v[unit_at] = 1.0;
    return v;
}

template <typename T>
static std::vector<T> download(const void *d, uint64_t n) {
    std::vector<T> h(n);
    if (n) GOK(crgpu_memcpy_d2h(g_gpu->ctx, h.data(), d, n * sizeof(T)));
    return h;
}
#define FILL_F64 0xFF
#define FILL_INT 0xA5
static const double NaN = std::numeric_limits<double>::quiet_NaN();
static double filled_f64() {  // what FILL_F64 leaves in an f64 nobody wrote
    double v;
    std::memset(&v, FILL_F64, sizeof(v));
    return v;
}

// ---- the references -----------------------------------------------------------------------------------------------------------
static const long double U53 = 0x1.0p-53L, U64 = 0x1.0p-64L;
static long double gam(uint64_t k) { return (long double)k * U53 / (1.0L - (long double)k * U53); }
// lane 0 of the butterfly 32, 16, 8, 4, 2, 1 (ref_butterfly of test_block_utils.hip)
static double wave0(const double *in) {
    double x[64], y[64];
    for (int i = 0; i < 64; i++) x[i] = in[i];
    for (int d = 32; d >= 1; d >>= 1) {
        for (int i = 0; i < 64; i++) y[i] = x[i] + x[i ^ d];
        for (int i = 0; i < 64; i++) x[i] = y[i];
    }
    return x[0];
}
static uint64_t dwave(uint64_t cnt) { return (cnt + WV - 1) / WV + 6; }                  // additions on the longest path of a wave sum
static uint64_t ddot(uint64_t n) { return PR / WV + 6 + (n + PR - 1) / PR; }             // ... of a dot over n rows
struct Ref {  // a sum of terms in long double, index order
    long double s = 0.0L, abs = 0.0L;
    uint64_t n = 0;
    void term(long double t) { s += t, abs += fabsl(t), n++; }
    void mul(double a, double b) { term((long double)a * (long double)b); }
    long double bound(uint64_t d) const { return gam(d + 1) * abs + (long double)(n + 2) * U64 * abs; }
};
// a scalar a kernel subtracts: the value it is given, what it stands for, and the additions behind it
struct Scalar {
    double value = 0.0;
    Ref ref;
    uint64_t depth = 0;
    static Scalar exact(double v) {
        Scalar s;
        s.value = v, s.ref.s = v, s.ref.abs = fabsl((long double)v);
        return s;
    }
};

static long double g_worst = 0.0L;
static std::string g_worst_at;
// the order model within the bound of the reference; the device value, when there is one, bit-equal to the model
static void judge(const char *what, uint64_t idx, double model, const double *dev, long double ref, long double bound) {
    const double got = dev ? *dev : model;
    if (dev && bits(*dev) != bits(model))
        die("%s [%llu]: the device has %a (%.17g), the order model %a (%.17g), the reference %.21Lg", what, (unsigned long long)idx, *dev, *dev, model, model, ref);
    const long double dev_err = fabsl((long double)got - ref);
    if (!(dev_err <= bound)) die("%s [%llu]: %.17g is %.3Lg from the reference %.21Lg, the bound is %.3Lg", what, (unsigned long long)idx, got, dev_err, ref, bound);
    if (bound > 0.0L && dev_err / bound > g_worst) g_worst = dev_err / bound, g_worst_at = what;
}
static int64_t ulp_distance(double a, double b) {  // both finite and of one sign
    const int64_t x = (int64_t)bits(a), y = (int64_t)bits(b);
    return x > y ? x - y : y - x;
}

// ---- matrices built by hand -------------------------------------------------------------------------------------------------
struct Case {
    std::string name;
    uint64_t V = 0;  // columns of the matrix
    uint32_t G = 0;  // rows of the matrix
    std::vector<long long> indptr{0};
    std::vector<int32_t> indices, data;
    bool has_bcs = false, has_fmap = false;
    std::vector<uint32_t> bcs;
    std::vector<int32_t> fmap;
    uint32_t F = 0;
    void column(const std::vector<uint32_t> &rows, Rng &rng, int32_t base = 0) {  // rows ascending
        for (uint32_t r : rows) {
            indices.push_back((int32_t)r);
            data.push_back(base ? base + (int32_t)V : (rng.below(16) ? 1 + (int32_t)rng.below(5) : 1 + (int32_t)rng.below(1000)));
        }
        indptr.push_back((long long)indices.size());
        V++;
    }
    void column_with_sum(uint32_t sum, Rng &rng) {  // up to four entries that add up to sum
        const uint32_t k = std::min<uint32_t>(sum, 4);
        std::vector<uint32_t> rows;
        for (uint32_t r = 0; r < G && rows.size() < k; r++)
            if (rng.below(G - r) < k - rows.size()) rows.push_back(r);
        for (uint32_t j = 0; j < k; j++) indices.push_back((int32_t)rows[j]), data.push_back(j + 1 < k ? 1 : (int32_t)(sum - (k - 1)));
        indptr.push_back((long long)indices.size());
        V++;
    }
};
static std::vector<uint32_t> sample(uint32_t G, uint32_t L, Rng &rng) {  // L of the rows 0 .. G - 1, ascending
    std::vector<uint32_t> rows;
    for (uint32_t r = 0; r < G && rows.size() < L; r++)
        if (rng.below(G - r) < L - rows.size()) rows.push_back(r);
    return rows;
}
static std::vector<uint32_t> range(uint32_t lo, uint32_t hi) {
    std::vector<uint32_t> r;
    for (uint32_t i = lo; i < hi; i++) r.push_back(i);
    return r;
}
static Case from_features(const char *name, uint64_t N, const std::vector<std::vector<uint32_t>> &cells_of, Rng &rng) {
    Case c;
    c.name = name, c.G = c.F = (uint32_t)cells_of.size();
    std::vector<std::vector<uint32_t>> rows(N);
    for (uint32_t f = 0; f < c.G; f++)
        for (uint32_t b : cells_of[f]) rows[b].push_back(f);
    for (uint64_t b = 0; b < N; b++) c.column(rows[b], rng);
    return c;
}

static Case case_lengths(Rng &rng) {
    Case c;
    c.name = "lengths", c.G = c.F = WG + 44u;
    const uint32_t lens[16] = {0, 1, 2, WV - 1, WV, WV + 1, 2 * WV - 1, 2 * WV, 2 * WV + 1, 3 * WV - 1, 3 * WV, 3 * WV + 1, WG, c.G, 0, 1};
    for (uint32_t L : lens) c.column(sample(c.G, L, rng), rng);
    return c;
}
static Case case_holes(Rng &rng) {
    Case c;
    const uint32_t L0 = 2 * WV + 2;  // a column of three chunks of the ballot compaction, the last one of two entries
    c.name = "holes", c.G = L0 + 40u;
    std::vector<uint8_t> used(c.G, 0);
    used[0] = used[WV - 1] = used[WV] = used[WV + 1] = used[L0 - 1] = 1;
    for (uint32_t r = L0; r < c.G; r++) used[r] = r % 3u != 0u;
    used[c.G - 1] = 1, used[c.G - 2] = 0;
    c.column(range(0, L0), rng);   // its used entries sit at 0, 63, 64, 65 and 129
    c.column(range(1, 21), rng);   // not empty, nothing used
    std::vector<uint32_t> last = range(1, 5);
    last.push_back(c.G - 1);
    c.column(last, rng);           // the last entry alone is used
    std::vector<uint32_t> alt;
    bool need = true;
    for (uint32_t r = L0; r < c.G; r++)
        if ((used[r] != 0) == need) alt.push_back(r), need = !need;
    c.column(alt, rng);            // every second entry is used
    c.column({}, rng);
    const uint32_t more[6] = {5, 40, WV + 1, c.G, 1, WV};
    for (uint32_t L : more) c.column(sample(c.G, L, rng), rng);
    uint32_t n_used = 0;
    for (uint8_t u : used) n_used += u;
    uint32_t stride = 7;
    while (std::gcd(stride, n_used) != 1u) stride += 2;
    c.has_fmap = true, c.fmap.assign(c.G, -1), c.F = n_used + 2u;  // two features at the end that no row maps to
    for (uint32_t r = 0, k = 0; r < c.G; r++)
        if (used[r]) c.fmap[r] = (int32_t)((k++ * stride + 3u) % n_used);  // a permutation, not monotone
    return c;
}
static Case case_subset(Rng &rng) {
    Case c;
    c.name = "subset", c.G = c.F = 50;
    for (uint32_t b = 0; b < 40; b++) {
        const bool listed = b % 3u == 1u || b == 39u;
        c.column(sample(c.G, listed ? (b * 7u) % 30u : 1u + (b * 5u) % 30u, rng), rng, listed ? 0 : 100000);  // unlisted: values that may appear nowhere
        if (listed) c.bcs.push_back(b);
    }
    c.has_bcs = true;
    return c;
}
static Case case_features_small(uint32_t F, Rng &rng) {
    const uint32_t N = 5;
    std::vector<std::vector<uint32_t>> cells(F);
    for (uint32_t f = 0; f < F; f++) {
        if (f == 0 || f == F - 1 || (f >= F / 2 && f < F / 2 + 10)) continue;  // empty: the first, the last, a run in the middle
        for (uint32_t b = 0; b < N; b++)
            if (f == 1 || (f == 2 && b != 1) || (f > 2 && rng.below(2))) cells[f].push_back(b);  // 1: every cell; 2: all but one
    }
    char name[64];
    std::snprintf(name, sizeof(name), "features F=%u N=%u", F, N);
    return from_features(name, N, cells, rng);
}
static Case case_features_wide(Rng &rng) {
    const uint32_t N = 2 * WV + 2;
    const uint32_t sizes[12] = {WV - 1, WV, WV + 1, 2 * WV, 2 * WV + 1, N, 0, 1, 2, N, 7, 0};
    std::vector<std::vector<uint32_t>> cells;
    for (uint32_t s : sizes) cells.push_back(sample(N, s, rng));
    char name[64];
    std::snprintf(name, sizeof(name), "features F=12 N=%u", N);
    return from_features(name, N, cells, rng);
}
static Case case_key_bits(uint32_t F, uint32_t N, Rng &rng) {
    std::vector<std::vector<uint32_t>> cells(F);
    for (uint32_t f = 0; f < F; f++)
        for (uint32_t b = 0; b < N; b++)
            if (F * N <= 4u || (f == 0 && b == 0) || (f == F - 1 && b == N - 1) || rng.below(8) == 0) cells[f].push_back(b);  // the largest key exists
    char name[64];
    std::snprintf(name, sizeof(name), "key bits F*N=%u", F * N);
    return from_features(name, N, cells, rng);
}
static Case case_median(const char *name, const std::vector<uint32_t> &sums, Rng &rng) {
    Case c;
    c.name = name, c.G = c.F = 20;
    for (uint32_t s : sums) c.column_with_sum(s, rng);
    return c;
}
// more columns than pca_wave_grid has waves at 64 threads, more entries than cr_grid's default cap has threads of PCA_WG
static Case case_tall(Rng &rng) {
    Case c;
    const uint64_t wave_cap = pca_wave_grid(1ull << 40, WV), grid_cap = cr_grid(1ull << 40, 1);
    const uint64_t N = wave_cap + WV + 1;
    const uint32_t per = (uint32_t)(grid_cap * WG / N + 1);
    c.name = "tall", c.G = c.F = WV;
    c.indices.reserve(N * per), c.data.reserve(N * per);
    for (uint64_t b = 0; b < N; b++) c.column(sample(c.G, per, rng), rng);
    if ((uint64_t)c.indices.size() <= grid_cap * WG) die("tall: %zu entries do not exceed %llu", c.indices.size(), (unsigned long long)(grid_cap * WG));
    return c;
}

// ---- the preparation on the host ------------------------------------------------------------------------------------------
struct Prep {
    uint64_t N = 0, nnz = 0;
    uint32_t F = 0;
    std::vector<uint32_t> sums_all, cnt, sums, col, tcell, tpos;
    std::vector<double> factor, x, val, tval;
    std::vector<uint64_t> rowptr, keys, keys_sorted, tptr;
    double median = 0.0;
};
static double log2_of(double x) { return std::log2(1.0 + x); }
static Prep host_prepare(const Case &c, bool logged) {
    Prep p;
    p.N = c.has_bcs ? c.bcs.size() : c.V, p.F = c.F;
    p.sums_all.assign(c.V, 0);
    for (uint64_t b = 0; b < c.V; b++)
        for (long long i = c.indptr[b]; i < c.indptr[b + 1]; i++)
            if (!c.has_fmap || c.fmap[c.indices[i]] >= 0) p.sums_all[b] += (uint32_t)c.data[i];
    p.cnt.assign(p.N, 0), p.sums.resize(p.N), p.factor.resize(p.N), p.rowptr.assign(p.N + 1, 0);
    for (uint64_t b = 0; b < p.N; b++) {
        const uint64_t m = c.has_bcs ? c.bcs[b] : b;
        for (long long i = c.indptr[m]; i < c.indptr[m + 1]; i++)
            if (!c.has_fmap || c.fmap[c.indices[i]] >= 0) p.cnt[b]++;
        p.sums[b] = p.sums_all[m], p.rowptr[b + 1] = p.rowptr[b] + p.cnt[b];
    }
    std::vector<uint32_t> sorted = p.sums;  // np.median of the sums, 0 taken as 1
    std::sort(sorted.begin(), sorted.end());
    p.median = p.N % 2 ? (double)sorted[p.N / 2] : ((double)sorted[p.N / 2 - 1] + (double)sorted[p.N / 2]) / 2.0;
    if (p.median < 1.0) p.median = 1.0;
    p.nnz = p.rowptr[p.N];
    for (uint64_t b = 0; b < p.N; b++) {
        const uint64_t m = c.has_bcs ? c.bcs[b] : b;
        p.factor[b] = p.median / (double)p.sums[b];
        for (long long i = c.indptr[m]; i < c.indptr[m + 1]; i++) {
            const int32_t f = c.has_fmap ? c.fmap[c.indices[i]] : c.indices[i];
            if (f < 0) continue;
            const double x = (double)c.data[i] * p.factor[b];
            p.col.push_back((uint32_t)f), p.x.push_back(x), p.val.push_back(logged ? log2_of(x) : x);
            p.keys.push_back((uint64_t)(uint32_t)f * p.N + b);
        }
    }
    // the transposition: the entries by (feature, cell); a counting sort by feature keeps the cells ascending
    p.tptr.assign((size_t)p.F + 1, 0);
    for (uint32_t f : p.col) p.tptr[f + 1]++;
    for (uint32_t f = 0; f < p.F; f++) p.tptr[f + 1] += p.tptr[f];
    std::vector<uint64_t> at(p.tptr.begin(), p.tptr.end() - 1);
    p.tpos.resize(p.nnz), p.tcell.resize(p.nnz), p.keys_sorted.resize(p.nnz);
    for (uint64_t b = 0; b < p.N; b++)
        for (uint64_t i = p.rowptr[b]; i < p.rowptr[b + 1]; i++) {
            const uint64_t o = at[p.col[i]]++;
            p.tpos[o] = (uint32_t)i, p.tcell[o] = (uint32_t)b, p.keys_sorted[o] = p.keys[i];
        }
    for (uint64_t o = 1; o < p.nnz; o++)
        if (p.keys_sorted[o - 1] >= p.keys_sorted[o]) die("%s: the host's transposition is not strictly ascending at %llu", c.name.c_str(), (unsigned long long)o);
    return p;
}
static void transpose_values(Prep &p) {
    p.tval.resize(p.nnz);
    for (uint64_t o = 0; o < p.nnz; o++) p.tval[o] = p.val[p.tpos[o]];
}

static int64_t g_libm_ulps = 0, g_libm_arg_ulps = 0, g_dev_ulps = 0, g_dev_arg_ulps = 0;
// log2l(1.0L + x) rounded to f64, and log2l of the f64 sum 1.0 + x, against libm (always) and against the device's values (when given)
static void check_logged(const Case &c, const Prep &p, const double *dev) {
    for (uint64_t i = 0; i < p.nnz; i++) {
        const double want = (double)log2l(1.0L + (long double)p.x[i]), want_arg = (double)log2l((long double)(1.0 + p.x[i])), host = log2_of(p.x[i]);
        if (!std::isfinite(want) || want <= 0.0 || !std::isfinite(want_arg) || want_arg <= 0.0) die("%s: log2l(1 + %a) = %a, %a", c.name.c_str(), p.x[i], want, want_arg);
        const int64_t dh = ulp_distance(host, want), da = ulp_distance(host, want_arg);
        if (dh > LIBM_LOG2_ULPS) die("%s: libm's log2(1 + %a) = %a lies %lld ulps from the rounded log2l %a, LIBM_LOG2_ULPS is %d", c.name.c_str(), p.x[i], host, (long long)dh, want, LIBM_LOG2_ULPS);
        if (da > LIBM_LOG2_ARG_ULPS) die("%s: libm's log2(1 + %a) = %a lies %lld ulps from the rounded log2l of the f64 argument %a, LIBM_LOG2_ARG_ULPS is %d", c.name.c_str(), p.x[i], host, (long long)da, want_arg, LIBM_LOG2_ARG_ULPS);
        g_libm_ulps = std::max(g_libm_ulps, dh), g_libm_arg_ulps = std::max(g_libm_arg_ulps, da);
        if (!dev) continue;
        if (!std::isfinite(dev[i]) || dev[i] <= 0.0 || ulp_distance(dev[i], want) > DEV_LOG2_ULPS)
            die("%s: val[%llu] = %a for x = %a, the rounded log2l is %a: more than %d ulps", c.name.c_str(), (unsigned long long)i, dev[i], p.x[i], want, DEV_LOG2_ULPS);
        if (ulp_distance(dev[i], want_arg) > DEV_LOG2_ARG_ULPS)
            die("%s: val[%llu] = %a for x = %a, the rounded log2l of the f64 argument is %a: more than %d ulps", c.name.c_str(), (unsigned long long)i, dev[i], p.x[i], want_arg, DEV_LOG2_ARG_ULPS);
        g_dev_ulps = std::max(g_dev_ulps, ulp_distance(dev[i], want)), g_dev_arg_ulps = std::max(g_dev_arg_ulps, ulp_distance(dev[i], want_arg));
        const long double r = std::max((long double)ulp_distance(dev[i], want) / DEV_LOG2_ULPS, (long double)ulp_distance(dev[i], want_arg) / DEV_LOG2_ARG_ULPS);
        if (r > g_worst) g_worst = r, g_worst_at = "log2(1 + x)";
    }
}

// Mean and variance of every feature over N cells, zeros included, from the transposed values.
// The order model: lane l adds the entries l, l + 64, ...; the butterfly; lane 0 adds the terms of the zeros as k_pca_meanvar has them.
// The reference: mean = sum x / N and var = (sum (x - mean)^2 + n_zero mean^2) / N with the true mean, in long double.
// The bound.  mean: S a wave sum of cnt non-negative entries (no product) and one division: gamma(dwave + 1) * mean.
// var: the device evaluates scikit-learn's  (T - C^2 / N) / N  with  T = sum (x - m)^2 + n_zero m^2,  C = sum (x - m) - n_zero m  for
// ITS rounded mean m.  In exact arithmetic that is the variance for ANY m (C = N (mean - m), T = N var + N (mean - m)^2), so only the
// rounding of the evaluation counts.  T is a sum of non-negative terms: x - m (1 rounding), its square (1), the wave sum (dwave), the
// term of the zeros (its two products are no deeper), their addition (1), then T - ... (1) and / N (1): gamma(dwave + 6) * T.
// C is a sum of terms of both signs, A = sum |x - m| + n_zero |m|: |C' - C| <= e = gamma(dwave + 2) * A  (the difference, the wave sum, one
// product or one subtraction), so C'^2 / N is within (2 |C| e + e^2) / N of C^2 / N, its own two roundings and the two behind it
// within gamma(4) * (|C| + e)^2 / N <= gamma(dwave + 6) * the same.  All of it over N.  The reference's own error is (cnt + 2) 2^-64 T / N.
static void check_meanvar(const std::string &name, const Prep &p, const double *dev_mean, const double *dev_var) {
    const double n = (double)p.N;
    for (uint32_t f = 0; f < p.F; f++) {
        const uint64_t lo = p.tptr[f], hi = p.tptr[f + 1], cnt = hi - lo;
        double lanes[64];
        for (uint32_t l = 0; l < 64; l++) {
            double s = 0.0;
            for (uint64_t i = lo + l; i < hi; i += 64) s += p.tval[i];
            lanes[l] = s;
        }
        const double mean = wave0(lanes) / n;
        double lc[64], lv[64];
        for (uint32_t l = 0; l < 64; l++) {
            double corr = 0.0, var = 0.0;
            for (uint64_t i = lo + l; i < hi; i += 64) {
                const double diff = p.tval[i] - mean;
                corr += diff, var += diff * diff;
            }
            lc[l] = corr, lv[l] = var;
        }
        double corr = wave0(lc), var = wave0(lv);
        const double n_zero = (double)(p.N - cnt);
        if (cnt != p.N) corr -= n_zero * mean;
        corr = corr * corr / n;
        if (cnt != p.N) var += n_zero * (mean * mean);
        const double var_model = (var - corr) / n;

        const long double Nl = (long double)p.N, nz = (long double)(p.N - cnt), m = (long double)mean;
        long double S = 0.0L, T = 0.0L, C = 0.0L, A = 0.0L, D = 0.0L;
        for (uint64_t i = lo; i < hi; i++) S += (long double)p.tval[i];
        const long double mean_ref = S / Nl;
        for (uint64_t i = lo; i < hi; i++) {
            const long double d = (long double)p.tval[i] - mean_ref, dm = (long double)p.tval[i] - m;
            D += d * d, T += dm * dm, C += dm, A += fabsl(dm);
        }
        const long double var_ref = (D + nz * mean_ref * mean_ref) / Nl;
        T += nz * m * m, C -= nz * m, A += nz * fabsl(m);
        const uint64_t dw = dwave(cnt);
        const long double e = gam(dw + 2) * A, c2 = (fabsl(C) + e) * (fabsl(C) + e) / Nl;
        const long double mean_bound = gam(dw + 1) * mean_ref + (long double)(cnt + 2) * U64 * mean_ref;
        const long double var_bound = (gam(dw + 6) * (T + c2) + (2.0L * fabsl(C) * e + e * e) / Nl) / Nl + (long double)(cnt + 2) * U64 * T / Nl;
        judge((name + " mean").c_str(), f, mean, dev_mean ? dev_mean + f : nullptr, mean_ref, mean_bound);
        judge((name + " var").c_str(), f, var_model, dev_var ? dev_var + f : nullptr, var_ref, var_bound);
        if (cnt == 0 && (bits(mean) != 0 || bits(var_model) != 0)) die("%s: feature %u without entries has mean %a, var %a", name.c_str(), f, mean, var_model);
    }
}

// val and tval after pca_scale: one rounded product an entry, in both orders
static std::vector<double> make_inv_scale(uint32_t F, Rng &rng) {
    std::vector<double> inv(F);
    for (double &v : inv) v = 0.25 + 4.0 * rng.unit();
    return inv;
}
static void scale_values(Prep &p, const std::vector<double> &inv) {
    for (uint64_t i = 0; i < p.nnz; i++) p.val[i] = p.val[i] * inv[p.col[i]];
    transpose_values(p);
}

struct DevCase {  // the matrix, the lists and the sums on the device
    GBuf<long long> indptr;
    GBuf<int32_t> indices, data, fmap;
    GBuf<uint32_t> bcs, sums_all;
    crgpu_matrix_dev m;
    DevCase(const Case &c, const Prep &p)
        : indptr(c.indptr, FILL_INT), indices(c.indices, FILL_INT), data(c.data, FILL_INT), fmap(c.fmap, FILL_INT), bcs(c.bcs, FILL_INT), sums_all(p.sums_all, FILL_INT) {
        m.n_barcodes = c.V, m.nnz = c.indices.size(), m.d_barcode_rank = nullptr;
        m.d_indptr = (const int64_t *)indptr.d, m.d_indices = indices.d, m.d_data = data.d;
    }
};

// pca_prepare and pca_scale as the stage calls them, then every kernel of the preparation once more by direct launch of two
// workgroups into buffers of this program (pca_prepare allocates its own, which cannot carry a guard), bit-equal to the first run
static void run_prepare(const Case &c, bool logged, uint32_t wg, Rng &rng) {
    Prep p = host_prepare(c, logged);
    const std::vector<double> inv = make_inv_scale(p.F, rng);
    const std::string name = c.name + (logged ? " logged" : " unlogged") + " wg=" + std::to_string(wg);
    if (g_host_only) {
        if (logged) check_logged(c, p, nullptr);
        transpose_values(p);
        check_meanvar(name, p, nullptr, nullptr);
        for (double v : p.val)
            if (!std::isfinite(v)) die("%s: the host's value %a", name.c_str(), v);
        case_done("%s: N=%llu F=%u nnz=%llu median=%g (host only)", name.c_str(), (unsigned long long)p.N, p.F, (unsigned long long)p.nnz, p.median);
        return;
    }
    crgpu_ctx *ctx = g_gpu->ctx;
    DevCase D(c, p);
    {  // the host's sums against the library's under the same mask
        std::vector<uint8_t> mask(c.G, 1);
        for (uint32_t r = 0; r < c.G && c.has_fmap; r++) mask[r] = c.fmap[r] >= 0;
        GBuf<uint32_t> lib_sums(c.V, FILL_INT);
        GOK(crgpu_matrix_dev_column_sums(ctx, &D.m, c.has_fmap ? mask.data() : nullptr, c.G, lib_sums.d));
        same((name + " sums_all").c_str(), lib_sums.get("sums_all"), p.sums_all);
    }
    const uint32_t *d_bcs = c.has_bcs ? D.bcs.d : nullptr;
    const int32_t *d_fmap = c.has_fmap ? D.fmap.d : nullptr;
    PcaPrep P;
    GOK(pca_prepare(ctx, &D.m, c.G, d_bcs, p.N, d_fmap, p.F, D.sums_all.d, logged, wg, P));
    if (P.N != p.N || P.F != p.F || P.nnz != p.nnz) die("%s: N, F, nnz = %llu, %u, %llu, expected %llu, %u, %llu", name.c_str(), (unsigned long long)P.N, P.F, (unsigned long long)P.nnz, (unsigned long long)p.N, p.F, (unsigned long long)p.nnz);
    same((name + " rowptr").c_str(), download<uint64_t>(P.rowptr.p, p.N + 1), p.rowptr);
    same((name + " col").c_str(), download<uint32_t>(P.col.p, p.nnz), p.col);
    same((name + " sorted keys").c_str(), download<uint64_t>(P.d_keys(), p.nnz), p.keys_sorted);
    same((name + " sorted entry numbers").c_str(), download<uint32_t>(P.d_perm(), p.nnz), p.tpos);
    const std::vector<double> val = download<double>(P.val.p, p.nnz);
    for (uint64_t i = 0; i < p.nnz; i++)
        if (!std::isfinite(val[i])) die("%s: val[%llu] = %a", name.c_str(), (unsigned long long)i, val[i]);
    if (logged) check_logged(c, p, val.data());
    else same((name + " val = count * factor").c_str(), val, p.x);
    p.val = val;  // from here on every check starts from the device's own values
    transpose_values(p);
    same((name + " tptr").c_str(), download<uint64_t>(P.tptr.p, (uint64_t)p.F + 1), p.tptr);
    same((name + " tcell").c_str(), download<uint32_t>(P.tcell.p, p.nnz), p.tcell);
    same((name + " tval").c_str(), download<double>(P.tval.p, p.nnz), p.tval);
    if (P.mean.size() != p.F || P.var.size() != p.F) die("%s: %zu means, %zu variances", name.c_str(), P.mean.size(), P.var.size());
    check_meanvar(name, p, P.mean.data(), P.var.data());

    // the direct launches, before the scaling: k_pca_count, k_pca_fill, k_pca_gather, k_pca_tptr, k_pca_meanvar
    hipStream_t st = ctx->stream;
    const uint64_t nnz = p.nnz;
    GBuf<uint64_t> d_rowptr(p.rowptr, FILL_INT), d_keys_sorted(p.keys_sorted, FILL_INT);
    GBuf<uint32_t> d_tpos(p.tpos, FILL_INT);
    GBuf<double> d_factor(p.factor, FILL_F64), d_inv(inv, FILL_F64);
    {
        GBuf<uint32_t> cnt(p.N, FILL_INT), sums(p.N, FILL_INT), flag(std::vector<uint32_t>(1, 0u), FILL_INT);
        hipLaunchKernelGGL(k_pca_count, dim3(2), dim3(wg), 0, st, D.indptr.d, D.indices.d, d_bcs, p.N, c.G, d_fmap, D.sums_all.d, cnt.d, sums.d, flag.d);
        g_gpu->launched("k_pca_count");
        same((name + " k_pca_count cnt").c_str(), cnt.get("cnt"), p.cnt);
        same((name + " k_pca_count sums").c_str(), sums.get("sums"), p.sums);
        if (flag.get("flag")[0] != 0u) die("%s: k_pca_count raised its flag", name.c_str());
    }
    GBuf<double> r_val(nnz, FILL_F64);
    GBuf<uint32_t> r_col(nnz, FILL_INT);
    if (nnz) {
        GBuf<uint64_t> keys(nnz, FILL_INT);
        GBuf<uint32_t> perm(nnz, FILL_INT);
        hipLaunchKernelGGL(k_pca_fill, dim3(2), dim3(wg), 0, st, D.indptr.d, D.indices.d, D.data.d, d_bcs, p.N, c.G, d_fmap, d_factor.d, logged ? 1 : 0, d_rowptr.d,
                           r_col.d, r_val.d, keys.d, perm.d);
        g_gpu->launched("k_pca_fill");
        same((name + " k_pca_fill col").c_str(), r_col.get("col"), p.col);
        same((name + " k_pca_fill val").c_str(), r_val.get("val"), p.val);
        same((name + " k_pca_fill keys").c_str(), keys.get("keys"), p.keys);
        const std::vector<uint32_t> pm = perm.get("perm");
        for (uint64_t i = 0; i < nnz; i++)
            if (pm[i] != (uint32_t)i) die("%s: k_pca_fill perm[%llu] = %u", name.c_str(), (unsigned long long)i, pm[i]);
    }
    GBuf<double> r_tval(nnz, FILL_F64);
    GBuf<uint32_t> r_tcell(nnz, FILL_INT);
    GBuf<uint64_t> r_tptr((uint64_t)p.F + 1, FILL_INT);
    if (nnz) {
        hipLaunchKernelGGL(k_pca_gather, dim3(2), dim3(WG), 0, st, d_keys_sorted.d, d_tpos.d, r_val.d, p.N, nnz, r_tval.d, r_tcell.d);
        g_gpu->launched("k_pca_gather");
        same((name + " k_pca_gather tval").c_str(), r_tval.get("tval"), p.tval);
        same((name + " k_pca_gather tcell").c_str(), r_tcell.get("tcell"), p.tcell);
    }
    {
        hipLaunchKernelGGL(k_pca_tptr, dim3(p.F / WG + 1u), dim3(WG), 0, st, d_keys_sorted.d, nnz, p.N, p.F, r_tptr.d);
        g_gpu->launched("k_pca_tptr");
        same((name + " k_pca_tptr").c_str(), r_tptr.get("tptr"), p.tptr);
        GBuf<double> mean(p.F, FILL_F64), var(p.F, FILL_F64);
        hipLaunchKernelGGL(k_pca_meanvar, dim3(2), dim3(wg), 0, st, r_tptr.d, r_tval.d, p.N, p.F, mean.d, var.d);
        g_gpu->launched("k_pca_meanvar");
        same((name + " k_pca_meanvar mean").c_str(), mean.get("mean"), P.mean);
        same((name + " k_pca_meanvar var").c_str(), var.get("var"), P.var);
    }
    // pca_scale, and k_pca_scale by direct launch
    GOK(pca_scale(ctx, P, d_inv.d));
    scale_values(p, inv);
    same((name + " scaled val").c_str(), download<double>(P.val.p, nnz), p.val);
    same((name + " scaled tval").c_str(), download<double>(P.tval.p, nnz), p.tval);
    same((name + " tcell after the scaling").c_str(), download<uint32_t>(P.tcell.p, nnz), p.tcell);
    if (nnz) {
        hipLaunchKernelGGL(k_pca_scale, dim3(2), dim3(WG), 0, st, r_val.d, r_col.d, nnz, d_inv.d);
        g_gpu->launched("k_pca_scale");
        same((name + " k_pca_scale").c_str(), r_val.get("val"), p.val);
    }
    case_done("%s: N=%llu F=%u nnz=%llu median=%g", name.c_str(), (unsigned long long)p.N, p.F, (unsigned long long)p.nnz, p.median);
}

// k_pca_feature_counts: counts[row] += count over the listed columns, rows >= G left out.  Integers, exact in any order: the host's
// histogram over the listed columns.  The counts are an accumulator (zeroed, the guard behind them kept); one, two and the stage's
// number of workgroups, so that the loop over the list makes further trips.
static void run_feature_counts(const Case &c, uint32_t G) {
    if (g_host_only) return;
    std::vector<uint32_t> bcs = c.bcs;
    if (!c.has_bcs)
        for (uint64_t b = 0; b < c.V; b++) bcs.push_back((uint32_t)b);
    std::vector<unsigned long long> want(G, 0ull);
    for (uint32_t b : bcs)
        for (long long i = c.indptr[b]; i < c.indptr[b + 1]; i++)
            if ((uint32_t)c.indices[i] < G) want[c.indices[i]] += (unsigned long long)(uint32_t)c.data[i];
    const std::string name = "k_pca_feature_counts " + c.name + " G=" + std::to_string(G);
    GBuf<long long> indptr(c.indptr, FILL_INT);
    GBuf<int32_t> indices(c.indices, FILL_INT), data(c.data, FILL_INT);
    GBuf<uint32_t> d_bcs(bcs, FILL_INT);
    const uint64_t N = bcs.size();
    for (uint32_t wg : {WV, 2 * WV, WG})
        for (uint32_t grid : {1u, 2u, pca_wave_grid(N, wg)}) {
            GBuf<unsigned long long> counts(G, FILL_INT);
            counts.zero();
            hipLaunchKernelGGL(k_pca_feature_counts, dim3(grid), dim3(wg), 0, g_gpu->ctx->stream, indptr.d, indices.d, data.d, d_bcs.d, N, G, counts.d);
            g_gpu->launched("k_pca_feature_counts");
            same((name + " wg=" + std::to_string(wg) + " grid=" + std::to_string(grid)).c_str(), counts.get("counts"), want);
        }
    unsigned long long top = 0;
    for (unsigned long long v : want) top = std::max(top, v);
    case_done("%s: %llu listed columns of %llu, the largest count %llu", name.c_str(), (unsigned long long)N, (unsigned long long)c.V, top);
}
static Case case_big_counts() {  // counts whose sum over the columns passes 2^32
    Case c;
    c.name = "big counts", c.G = c.F = 6;
    for (uint32_t b = 0; b < 5; b++) {
        for (uint32_t r = b % 2u; r < c.G; r += 2) c.indices.push_back((int32_t)r), c.data.push_back(r == 2 ? 1 : r == 4 ? (int32_t)0x80000001u : 0x7FFFFFFF);  // row 4: a count above 2^31, taken as unsigned
        c.indptr.push_back((long long)c.indices.size()), c.V++;
    }
    return c;
}

static void group_prepare() {
    Rng rng(0x5eed9ca1ull);
    std::vector<Case> both, logged_only;
    both.push_back(case_lengths(rng));
    both.push_back(case_holes(rng));
    logged_only.push_back(case_subset(rng));
    for (uint32_t F : {WG - 1u, WG, WG + 1u}) logged_only.push_back(case_features_small(F, rng));
    logged_only.push_back(case_features_wide(rng));
    logged_only.push_back(case_key_bits(2, 2, rng));
    logged_only.push_back(case_key_bits(WG, 4, rng));
    logged_only.push_back(case_key_bits(WG + 1u, 4, rng));
    logged_only.push_back(case_median("median odd, ties", {5, 5, 5, 9, 2, 2, 12}, rng));
    logged_only.push_back(case_median("median even, between two sums", {1, 3, 3, 4, 7, 7, 10, 12}, rng));
    logged_only.push_back(case_median("median 0 of mostly empty columns", {0, 0, 6, 0, 3, 0, 8, 0, 2}, rng));
    logged_only.push_back(case_median("median 0.5 of half empty columns", {0, 0, 0, 0, 1, 5, 2, 9}, rng));
    for (uint32_t wg : {WV, 2 * WV, WG}) {
        for (const Case &c : both) run_prepare(c, false, wg, rng), run_prepare(c, true, wg, rng);
        for (const Case &c : logged_only) run_prepare(c, true, wg, rng);
    }
    const Case tall = case_tall(rng);
    run_prepare(tall, true, WV, rng);
    // the counts per feature of the thresholding: the column subset (the unlisted columns' values appear nowhere), rows at and above
    // G left out, sums above 2^32, more listed columns than the grid has waves
    run_feature_counts(logged_only[0], logged_only[0].G);
    run_feature_counts(both[1], both[1].G), run_feature_counts(both[1], WV + 1);
    run_feature_counts(case_big_counts(), 6), run_feature_counts(case_big_counts(), 5);
    run_feature_counts(tall, tall.G);
}

// ---- the operator ---------------------------------------------------------------------------------------------------------
// the dots: slab[part][c] and out[c] as k_pca_dots and k_pca_dots_finish compute them
static void dots_model(const double *y, const double *X, uint64_t ld, uint32_t ncols, uint64_t n, std::vector<double> &slab, std::vector<double> &out) {
    const uint32_t n_parts = (uint32_t)((n + PR - 1) / PR);
    slab.assign((size_t)n_parts * ncols, 0.0), out.assign(ncols, 0.0);
    for (uint32_t part = 0; part < n_parts; part++)
        for (uint32_t c = 0; c < ncols; c++) {
            double lanes[64];
            for (uint32_t l = 0; l < 64; l++) {
                double a = 0.0;
                for (uint32_t u = 0; u < PR / WV; u++) {
                    const uint64_t r = (uint64_t)part * PR + l + (uint64_t)WV * u;
                    a += r < n ? y[r] * X[(size_t)c * ld + r] : 0.0;
                }
                lanes[l] = a;
            }
            slab[(size_t)part * ncols + c] = wave0(lanes);
        }
    for (uint32_t c = 0; c < ncols; c++) {
        double a = 0.0;
        for (uint32_t part = 0; part < n_parts; part++) a += slab[(size_t)part * ncols + c];
        out[c] = a;
    }
}
static Scalar dot_scalar(const std::vector<double> &y, const std::vector<double> &x) {  // what PcaLanczos::dot leaves in scal
    Scalar s;
    std::vector<double> slab, out;
    dots_model(y.data(), x.data(), y.size(), 1, y.size(), slab, out);
    s.value = out[0], s.depth = ddot(y.size());
    for (size_t i = 0; i < y.size(); i++) s.ref.mul(y[i], x[i]);
    return s;
}

struct View {  // a prepared matrix as the device holds it
    uint64_t N = 0, nnz = 0;
    uint32_t F = 0;
    std::vector<uint64_t> rowptr, tptr;
    std::vector<uint32_t> col, tcell;
    std::vector<double> val, tval;
};
// w = A v - cv
static void check_av(const std::string &name, const View &A, const std::vector<double> &v, const Scalar &cv, int64_t unit_at, const double *dev,
                     std::vector<long double> *bounds) {
    for (uint64_t c = 0; c < A.N; c++) {
        const uint64_t lo = A.rowptr[c], hi = A.rowptr[c + 1];
        double lanes[64];
        for (uint32_t l = 0; l < 64; l++) {
            double a = 0.0;
            for (uint64_t i = lo + l; i < hi; i += 64) a += A.val[i] * v[A.col[i]];
            lanes[l] = a;
        }
        const double model = wave0(lanes) - cv.value;
        Ref r;
        for (uint64_t i = lo; i < hi; i++) r.mul(A.val[i], v[A.col[i]]);
        r.s -= cv.ref.s, r.abs += cv.ref.abs, r.n += cv.ref.n;
        const long double b = r.bound(std::max(dwave(hi - lo), cv.depth) + 1);
        judge(name.c_str(), c, model, dev ? dev + c : nullptr, r.s, b);
        if (bounds) (*bounds)[c] = b;
        if (lo == hi && bits(model) != bits(-cv.value)) die("%s: the row %llu without entries gives %a, not -cv = %a", name.c_str(), (unsigned long long)c, model, -cv.value);
        if (unit_at >= 0) {  // one column of the matrix, exactly
            double entry = 0.0;
            for (uint64_t i = lo; i < hi; i++)
                if (A.col[i] == (uint32_t)unit_at) entry = A.val[i];
            if (bits(model) != bits(entry - cv.value)) die("%s: a unit vector gives %a in row %llu, the entry minus cv is %a", name.c_str(), model, (unsigned long long)c, entry - cv.value);
        }
    }
}
// f = A^T w - sw * center
static void check_atw(const std::string &name, const View &A, const std::vector<double> &w, const Scalar &sw, const std::vector<double> &center, int64_t unit_at,
                      const double *dev, std::vector<long double> *bounds) {
    for (uint32_t f = 0; f < A.F; f++) {
        const uint64_t lo = A.tptr[f], hi = A.tptr[f + 1];
        double lanes[64];
        for (uint32_t l = 0; l < 64; l++) {
            double a = 0.0;
            for (uint64_t i = lo + l; i < hi; i += 64) a += A.tval[i] * w[A.tcell[i]];
            lanes[l] = a;
        }
        const double model = wave0(lanes) - sw.value * center[f];
        Ref r;
        for (uint64_t i = lo; i < hi; i++) r.mul(A.tval[i], w[A.tcell[i]]);
        r.s -= sw.ref.s * (long double)center[f], r.abs += sw.ref.abs * fabsl((long double)center[f]), r.n += sw.ref.n + 1;
        const long double b = r.bound(std::max(dwave(hi - lo), sw.depth + 1) + 1);  // sw * center[f]: one product more on its path
        judge(name.c_str(), f, model, dev ? dev + f : nullptr, r.s, b);
        if (bounds) (*bounds)[f] = b;
        if (lo == hi && bits(model) != bits(-(sw.value * center[f]))) die("%s: the feature %u without entries gives %a, not -sw * center", name.c_str(), f, model);
        if (unit_at >= 0) {
            double entry = 0.0;
            for (uint64_t i = lo; i < hi; i++)
                if (A.tcell[i] == (uint32_t)unit_at) entry = A.tval[i];
            if (bits(model) != bits(entry - sw.value * center[f])) die("%s: a unit vector gives %a for feature %u, the entry minus sw * center is %a", name.c_str(), model, f, entry - sw.value * center[f]);
        }
    }
}
// <A v, w> = <v, A^T w> for the operator A - 1 c^T, within the two bounds added: sum |w_c| bound_av[c] + sum |v_f| bound_atw[f], and
// the error of the two long double sums themselves.  Needs no model.
static void check_adjoint(const std::string &name, const std::vector<double> &v, const std::vector<double> &w, const std::vector<double> &av, const std::vector<double> &atw,
                          const std::vector<long double> &b_av, const std::vector<long double> &b_atw) {
    Ref l, r;
    long double tol = 0.0L;
    for (size_t c = 0; c < w.size(); c++) l.mul(w[c], av[c]), tol += fabsl((long double)w[c]) * b_av[c];
    for (size_t f = 0; f < v.size(); f++) r.mul(v[f], atw[f]), tol += fabsl((long double)v[f]) * b_atw[f];
    tol += (long double)(l.n + r.n + 2) * U64 * (l.abs + r.abs);
    const long double err = fabsl(l.s - r.s);
    if (!(err <= tol)) die("%s: <A v, w> = %.21Lg, <v, A^T w> = %.21Lg, %.3Lg apart, the two bounds add up to %.3Lg", name.c_str(), l.s, r.s, err, tol);
    if (tol > 0.0L && err / tol > g_worst) g_worst = err / tol, g_worst_at = name;
}

static void run_operator(const Case &c, uint32_t wg, Rng &rng) {
    Prep p = host_prepare(c, true);
    const std::vector<double> inv = make_inv_scale(p.F, rng);
    View A;
    A.N = p.N, A.F = p.F, A.nnz = p.nnz;
    PcaPrep P;
    PcaLanczos L;
    std::unique_ptr<DevCase> D;
    if (g_host_only) {
        scale_values(p, inv);
        A.rowptr = p.rowptr, A.tptr = p.tptr, A.col = p.col, A.tcell = p.tcell, A.val = p.val, A.tval = p.tval;
    } else {
        crgpu_ctx *ctx = g_gpu->ctx;
        D.reset(new DevCase(c, p));
        GBuf<double> d_inv(inv, FILL_F64);
        GOK(pca_prepare(ctx, &D->m, c.G, c.has_bcs ? D->bcs.d : nullptr, p.N, c.has_fmap ? D->fmap.d : nullptr, p.F, D->sums_all.d, true, wg, P));
        GOK(pca_scale(ctx, P, d_inv.d));
        if (P.nnz != p.nnz) die("%s: nnz %llu, expected %llu", c.name.c_str(), (unsigned long long)P.nnz, (unsigned long long)p.nnz);
        A.rowptr = download<uint64_t>(P.rowptr.p, p.N + 1), A.tptr = download<uint64_t>(P.tptr.p, (uint64_t)p.F + 1);
        A.col = download<uint32_t>(P.col.p, p.nnz), A.tcell = download<uint32_t>(P.tcell.p, p.nnz);
        A.val = download<double>(P.val.p, p.nnz), A.tval = download<double>(P.tval.p, p.nnz);
        same((c.name + " rowptr").c_str(), A.rowptr, p.rowptr), same((c.name + " tptr").c_str(), A.tptr, p.tptr);
        same((c.name + " col").c_str(), A.col, p.col), same((c.name + " tcell").c_str(), A.tcell, p.tcell);
        L.ctx = ctx, L.A = &P, L.m = p.N, L.n = p.F, L.wg = wg, L.ppb = 1;
        GOK(L.init(2));
    }
    std::vector<double> center(p.F);
    for (double &x : center) x = rng.nonzero();
    const std::vector<double> ones_m(p.N, 1.0);
    if (!g_host_only) GOK(crgpu_memcpy_h2d(g_gpu->ctx, L.center.p, center.data(), p.F * sizeof(double)));
    struct Set {
        VecKind kind;
        uint64_t vf, wc;
    };
    const Set sets[5] = {{VEC_NORMAL, 0, 0}, {VEC_DECADES, 0, 0}, {VEC_UNIT, 0, 0}, {VEC_UNIT, p.F - 1u, p.N - 1u}, {VEC_UNIT, p.F / 2u, p.N / 2u}};
    uint32_t ordinal = 0;
    for (const Set &s : sets) {
        const std::vector<double> v = make_vec(p.F, s.kind, s.vf, rng), w = make_vec(p.N, s.kind, s.wc, rng);
        const int64_t uv = s.kind == VEC_UNIT ? (int64_t)s.vf : -1, uw = s.kind == VEC_UNIT ? (int64_t)s.wc : -1;
        const std::string name = c.name + " " + VEC_NAMES[s.kind] + (s.kind == VEC_UNIT ? " " + std::to_string(s.vf) + "/" + std::to_string(s.wc) : std::string());
        // through PcaLanczos: the scalars come from the dot kernels, so their model is the dot's
        const Scalar cv = dot_scalar(center, v), sw = dot_scalar(w, ones_m);
        std::vector<long double> b_av(p.N), b_atw(p.F);
        const double s0 = rng.nonzero(), s1 = rng.nonzero();  // the scalars of the direct launches
        if (g_host_only) {
            check_av(name + " PcaLanczos::av", A, v, cv, uv, nullptr, &b_av);
            check_atw(name + " PcaLanczos::atw", A, w, sw, center, uw, nullptr, &b_atw);
            check_av(name + " k_pca_av", A, v, Scalar::exact(s0), uv, nullptr, nullptr);
            check_atw(name + " k_pca_atw", A, w, Scalar::exact(s1), center, uw, nullptr, nullptr);
            continue;
        }
        GBuf<double> d_v(v, FILL_F64), d_w(w, FILL_F64);
        L.ppb = 1u + (ordinal++ % 3u);
        {
            GBuf<double> out_w(p.N, FILL_F64), out_f(p.F, FILL_F64);
            GOK(L.av(d_v.d, out_w.d));
            GOK(L.atw(d_w.d, out_f.d));
            const std::vector<double> scal = download<double>(L.scal.p, 2);
            if (bits(scal[0]) != bits(cv.value) || bits(scal[1]) != bits(sw.value)) die("%s: the scalars c . v, sum w are %a, %a on the device, %a, %a in the dot's model", name.c_str(), scal[0], scal[1], cv.value, sw.value);
            const std::vector<double> hw = out_w.get("w"), hf = out_f.get("f");
            check_av(name + " PcaLanczos::av", A, v, cv, uv, hw.data(), &b_av);
            check_atw(name + " PcaLanczos::atw", A, w, sw, center, uw, hf.data(), &b_atw);
            check_adjoint(name + " adjoint", v, w, hw, hf, b_av, b_atw);
        }
        const std::vector<double> scal{s0, s1, NaN, NaN};
        GBuf<double> d_scal(scal, FILL_F64);
        for (uint32_t grid : {1u, 3u}) {  // 4 and 12 waves: every matrix here has more rows and, but for the widest, more features
            GBuf<double> out_w(p.N, FILL_F64), out_f(p.F, FILL_F64);
            hipLaunchKernelGGL(k_pca_av, dim3(grid), dim3(WG), 0, g_gpu->ctx->stream, P.rowptr.as<uint64_t>(), P.col.as<uint32_t>(), P.val.as<double>(), p.N, d_v.d, d_scal.d, out_w.d);
            g_gpu->launched("k_pca_av");
            hipLaunchKernelGGL(k_pca_atw, dim3(grid), dim3(WG), 0, g_gpu->ctx->stream, P.tptr.as<uint64_t>(), P.tcell.as<uint32_t>(), P.tval.as<double>(), p.F, d_w.d, d_scal.d,
                               L.center.as<double>(), out_f.d);
            g_gpu->launched("k_pca_atw");
            const std::vector<double> hw = out_w.get("w"), hf = out_f.get("f");
            check_av(name + " k_pca_av grid " + std::to_string(grid), A, v, Scalar::exact(s0), uv, hw.data(), nullptr);
            check_atw(name + " k_pca_atw grid " + std::to_string(grid), A, w, Scalar::exact(s1), center, uw, hf.data(), nullptr);
        }
    }
    case_done("operator on %s: %llu x %u, nnz %llu", c.name.c_str(), (unsigned long long)p.N, p.F, (unsigned long long)p.nnz);
}
static void group_operator() {
    Rng rng(0x5eed0be7ull);
    run_operator(case_lengths(rng), WG, rng);
    run_operator(case_holes(rng), 2 * WV, rng);
    run_operator(case_features_wide(rng), WG, rng);
    run_operator(case_tall(rng), WV, rng);
}

// ---- the dense steps --------------------------------------------------------------------------------------------------------
// a column-major n x ncols block with the stride ld: NaN in the padding
static std::vector<double> make_block(uint64_t n, uint64_t ld, uint32_t ncols, VecKind kind, Rng &rng) {
    std::vector<double> X((size_t)ld * ncols, NaN);
    for (uint32_t c = 0; c < ncols; c++) {
        const std::vector<double> col = make_vec(n, kind, 0, rng);
        std::copy(col.begin(), col.end(), X.begin() + (size_t)c * ld);
    }
    return X;
}
static void padding_untouched(const std::string &name, const std::vector<double> &got, const std::vector<double> &before, uint64_t n, uint64_t ld, uint32_t ncols) {
    for (uint32_t c = 0; c < ncols; c++)
        for (uint64_t r = n; r < ld; r++)
            if (bits(got[(size_t)c * ld + r]) != bits(before[(size_t)c * ld + r])) die("%s: the padding row %llu of column %u was written", name.c_str(), (unsigned long long)r, c);
}
static void run_dots(uint64_t n, uint32_t ncols, VecKind kind, Rng &rng) {
    const uint64_t ld = n + 7;
    const std::vector<double> y = make_block(n, ld, 1, kind, rng), X = make_block(n, ld, ncols, kind, rng);
    std::vector<double> slab, out;
    dots_model(y.data(), X.data(), ld, ncols, n, slab, out);
    const uint32_t n_parts = (uint32_t)((n + PR - 1) / PR);
    const std::string name = "dots n=" + std::to_string(n) + " ncols=" + std::to_string(ncols) + " " + VEC_NAMES[kind];
    std::vector<Ref> refs(ncols);
    for (uint32_t c = 0; c < ncols; c++)
        for (uint64_t r = 0; r < n; r++) refs[c].mul(y[r], X[(size_t)c * ld + r]);
    if (g_host_only) {
        for (uint32_t c = 0; c < ncols; c++) judge(name.c_str(), c, out[c], nullptr, refs[c].s, refs[c].bound(ddot(n)));
        return;
    }
    GBuf<double> d_y(y, FILL_F64), d_X(X, FILL_F64);
    for (uint32_t ppb : {1u, 2u, 3u, WV}) {  // above n_parts, and (n_parts = 3, ppb = 2) a last workgroup whose partials run out
        GBuf<double> d_slab((uint64_t)n_parts * ncols, FILL_F64), d_out(ncols, FILL_F64);
        hipLaunchKernelGGL(k_pca_dots, dim3((n_parts + ppb - 1) / ppb), dim3(WG), 0, g_gpu->ctx->stream, d_y.d, d_X.d, ld, ncols, n, n_parts, ppb, d_slab.d);
        g_gpu->launched("k_pca_dots");
        hipLaunchKernelGGL(k_pca_dots_finish, dim3((ncols + WG - 1) / WG), dim3(WG), 0, g_gpu->ctx->stream, d_slab.d, n_parts, ncols, d_out.d);
        g_gpu->launched("k_pca_dots_finish");
        same((name + " ppb=" + std::to_string(ppb) + " slab").c_str(), d_slab.get("slab"), slab);
        const std::vector<double> h = d_out.get("dots");
        for (uint32_t c = 0; c < ncols; c++) judge((name + " ppb=" + std::to_string(ppb)).c_str(), c, out[c], &h[c], refs[c].s, refs[c].bound(ddot(n)));
    }
}
static void run_update(uint64_t n, uint32_t ncols, Rng &rng) {
    const uint64_t ld = n + 7;
    const std::vector<double> y = make_block(n, ld, 1, VEC_DECADES, rng), X = make_block(n, ld, ncols, VEC_NORMAL, rng), coef = make_vec(ncols, VEC_DECADES, 0, rng);
    const std::string name = "update n=" + std::to_string(n) + " ncols=" + std::to_string(ncols);
    std::vector<double> want = y;
    std::vector<Ref> refs(n);
    for (uint64_t r = 0; r < n; r++) {
        double a = 0.0;
        for (uint32_t c = 0; c < ncols; c++) a += X[(size_t)c * ld + r] * coef[c];  // the columns ascending, then y - a
        want[r] = y[r] - a;
        refs[r].term((long double)y[r]);
        for (uint32_t c = 0; c < ncols; c++) refs[r].mul(-X[(size_t)c * ld + r], coef[c]);
    }
    for (uint32_t grid : {0u, 1u}) {
        if (g_host_only) {
            for (uint64_t r = 0; r < n; r++) judge(name.c_str(), r, want[r], nullptr, refs[r].s, refs[r].bound(ncols + 1));
            break;
        }
        GBuf<double> d_y(y, FILL_F64), d_X(X, FILL_F64), d_c(coef, FILL_F64);
        hipLaunchKernelGGL(k_pca_update, dim3(grid ? grid : cr_grid(n, WG)), dim3(WG), 0, g_gpu->ctx->stream, d_y.d, d_X.d, ld, ncols, d_c.d, n);
        g_gpu->launched("k_pca_update");
        const std::vector<double> h = d_y.get("y");
        for (uint64_t r = 0; r < n; r++) judge(name.c_str(), r, want[r], &h[r], refs[r].s, refs[r].bound(ncols + 1));
        padding_untouched(name, h, y, n, ld, 1);
    }
}
static void run_vector_steps(uint64_t n, Rng &rng) {  // k_pca_axpy, k_pca_scal, k_pca_fill_ones: one or two roundings an element, the model is the definition
    if (g_host_only) return;
    const uint64_t ld = n + 7;
    const std::vector<double> y = make_block(n, ld, 1, VEC_DECADES, rng), x = make_block(n, ld, 1, VEC_NORMAL, rng);
    const double alpha = rng.nonzero();
    const std::string name = "n=" + std::to_string(n);
    hipStream_t st = g_gpu->ctx->stream;
    for (uint32_t grid : {0u, 1u}) {
        const uint32_t g = grid ? grid : cr_grid(n, WG);
        GBuf<double> a(y, FILL_F64), s(y, FILL_F64), o(y, FILL_F64), d_x(x, FILL_F64);
        hipLaunchKernelGGL(k_pca_axpy, dim3(g), dim3(WG), 0, st, a.d, alpha, d_x.d, n);
        g_gpu->launched("k_pca_axpy");
        hipLaunchKernelGGL(k_pca_scal, dim3(g), dim3(WG), 0, st, s.d, alpha, n);
        g_gpu->launched("k_pca_scal");
        hipLaunchKernelGGL(k_pca_fill_ones, dim3(g), dim3(WG), 0, st, o.d, n);
        g_gpu->launched("k_pca_fill_ones");
        std::vector<double> wa = y, ws = y, wo = y;
        for (uint64_t r = 0; r < n; r++) wa[r] = y[r] - alpha * x[r], ws[r] = alpha * y[r], wo[r] = 1.0;
        same(("axpy " + name).c_str(), a.get("axpy"), wa);  // the padding behind n included: still the NaN it held
        same(("scal " + name).c_str(), s.get("scal"), ws);
        same(("fill_ones " + name).c_str(), o.get("ones"), wo);
    }
}
// out[:, c] = X[:, 0:mb] M[:, c], t ascending: through PcaLanczos::small_product in place (the restart's use) and by a direct launch
// of one workgroup with ld = n + 7
static void run_small_product(uint64_t n, uint32_t mb, uint32_t k, Rng &rng) {
    const std::string name = "small_product n=" + std::to_string(n) + " mb=" + std::to_string(mb) + " k=" + std::to_string(k);
    const std::vector<double> M = make_vec((size_t)mb * k, VEC_NORMAL, 0, rng);
    for (uint32_t direct = 0; direct < 2; direct++) {
        const uint64_t ld = direct ? n + 7 : n;
        const std::vector<double> X = make_block(n, ld, mb, direct ? VEC_DECADES : VEC_NORMAL, rng);
        std::vector<double> want((size_t)ld * k, filled_f64());
        std::vector<Ref> refs((size_t)n * k);
        for (uint32_t c = 0; c < k; c++)
            for (uint64_t r = 0; r < n; r++) {
                double a = 0.0;
                for (uint32_t t = 0; t < mb; t++) a += X[(size_t)t * ld + r] * M[(size_t)t * k + c], refs[(size_t)c * n + r].mul(X[(size_t)t * ld + r], M[(size_t)t * k + c]);
                want[(size_t)c * ld + r] = a;
            }
        std::vector<double> got;
        if (!g_host_only && direct) {
            GBuf<double> d_X(X, FILL_F64), d_M(M, FILL_F64), d_out((uint64_t)ld * k, FILL_F64);
            hipLaunchKernelGGL(k_pca_small_product, dim3(1), dim3(WG), 0, g_gpu->ctx->stream, d_X.d, ld, n, mb, d_M.d, k, d_out.d);
            g_gpu->launched("k_pca_small_product");
            got = d_out.get("out");
            same((name + " direct").c_str(), got, want);  // the padding rows still hold the NaN of the fill
        } else if (!g_host_only) {
            PcaLanczos L;
            L.ctx = g_gpu->ctx, L.A = nullptr, L.m = L.n = n, L.wg = WG, L.ppb = 1;
            GOK(L.init(mb));
            GBuf<double> d_X(X, FILL_F64);
            GOK(L.small_product(d_X.d, n, M, k, d_X.d));
            got = d_X.get("X");
            for (size_t i = (size_t)n * k; i < got.size(); i++)
                if (bits(got[i]) != bits(X[i])) die("%s in place: element %zu behind the k columns was written", name.c_str(), i);
        }
        for (uint32_t c = 0; c < k; c++)
            for (uint64_t r = 0; r < n; r++)
                judge((name + (direct ? " direct" : " in place")).c_str(), (uint64_t)c * n + r, want[(size_t)c * ld + r], g_host_only ? nullptr : &got[(size_t)c * ld + r],
                      refs[(size_t)c * n + r].s, refs[(size_t)c * n + r].bound(mb));
    }
}
static void group_dense() {
    Rng rng(0x5eedde25ull);
    const uint64_t ns[11] = {1, WV - 1, WV, WV + 1, PR - 1, PR, PR + 1, 2 * PR - 1, 2 * PR, 2 * PR + 1, 3 * PR + 1};
    const uint32_t cols[7] = {1, WPW - 1, WPW, WPW + 1, 2 * WPW, 2 * WPW + 1, PCA_MAX_MB};
    for (uint64_t n : ns) {
        for (uint32_t nc : cols) run_dots(n, nc, nc % 2u ? VEC_DECADES : VEC_NORMAL, rng), run_update(n, nc, rng);
        run_vector_steps(n, rng);
        case_done("dense n=%llu: dots and update at %zu column counts, axpy, scal, fill_ones", (unsigned long long)n, sizeof(cols) / sizeof(cols[0]));
    }
    // n * k off and on a multiple of the workgroup, n = 1, more elements than one workgroup has threads
    const uint64_t sp_n[5] = {1, WV + 1, WG / 2, PR + 1, 3 * PR + 1};
    for (uint64_t n : sp_n) {
        run_small_product(n, 5, 2, rng);
        run_small_product(n, 2 * WPW + 1, 2 * WPW - 2, rng);
        case_done("small_product n=%llu", (unsigned long long)n);
    }
    run_small_product(WV + 1, PCA_MAX_MB, PCA_MAX_MB - 3, rng);
    case_done("small_product mb=%u", PCA_MAX_MB);
}

// ---- the projection -------------------------------------------------------------------------------------------------------
static void group_project() {
    Rng rng(0x5eed9903ull);
    // rows of 0, 1, 64, 65 and 200 entries, one of them with nothing mapped; 13 rows: a second trip for 4 and for 12 waves
    const uint32_t G = 3 * WV + 40, lens[13] = {0, 1, WV, WV + 1, 3 * WV + 8, 5, 0, WV + 1, 1, 3 * WV + 8, WV, 2, WV - 1};
    const uint64_t N = 13, nothing_mapped = 5;
    std::vector<int32_t> pmap(G, -1);
    std::vector<uint32_t> unmapped;
    uint32_t n_used = 0;
    for (uint32_t r = 0; r < G; r++) {
        if (r % 4u == 1u || r % 7u == 3u) unmapped.push_back(r);
        else n_used++;
    }
    for (uint32_t r = 0, k = 0; r < G; r++)
        if (!(r % 4u == 1u || r % 7u == 3u)) pmap[r] = (int32_t)((k++ * 5u + 2u) % n_used);  // needs gcd(5, n_used) = 1
    if (std::gcd(5u, n_used) != 1u) die("project: %u used features share a factor with 5", n_used);
    std::vector<uint64_t> rowptr(1, 0);
    std::vector<uint32_t> col;
    std::vector<double> val;
    for (uint64_t b = 0; b < N; b++) {
        std::vector<uint32_t> rows = sample(G, lens[b], rng);
        if (b == nothing_mapped) rows.assign(unmapped.begin(), unmapped.begin() + lens[b]);
        for (uint32_t r : rows) col.push_back(r), val.push_back(b % 2u ? rng.normal() : 4.0 * rng.unit());
        rowptr.push_back(col.size());
    }
    const uint32_t nus[7] = {1, PC - 1, PC, PC + 1, 2 * PC, 2 * PC + 1, CRGPU_PCA_MAX_COMPONENTS};
    for (uint32_t nu : nus) {
        const std::vector<double> v = make_vec((size_t)n_used * nu, nu % 2u ? VEC_DECADES : VEC_NORMAL, 0, rng);
        std::vector<double> cv(nu);
        for (double &x : cv) x = rng.nonzero();
        std::vector<double> want(N * nu);
        std::vector<Ref> refs(N * nu);
        for (uint64_t b = 0; b < N; b++)
            for (uint32_t comp = 0; comp < nu; comp++) {
                double lanes[64];
                for (uint32_t l = 0; l < 64; l++) {  // the lanes take entries by their index, mapped or not
                    double a = 0.0;
                    for (uint64_t i = rowptr[b] + l; i < rowptr[b + 1]; i += 64) {
                        const int32_t g = pmap[col[i]];
                        if (g < 0) continue;
                        a += val[i] * v[(size_t)g * nu + comp];
                    }
                    lanes[l] = a;
                }
                want[b * nu + comp] = wave0(lanes) - cv[comp];
                Ref &r = refs[b * nu + comp];
                for (uint64_t i = rowptr[b]; i < rowptr[b + 1]; i++)
                    if (pmap[col[i]] >= 0) r.mul(val[i], v[(size_t)pmap[col[i]] * nu + comp]);
                r.term(-(long double)cv[comp]);
                if ((b == nothing_mapped || rowptr[b] == rowptr[b + 1]) && bits(want[b * nu + comp]) != bits(-cv[comp])) die("project: row %llu gives %a, not -cv", (unsigned long long)b, want[b * nu + comp]);
            }
        auto all = [&](const std::string &name, const double *dev) {
            for (uint64_t b = 0; b < N; b++)
                for (uint32_t comp = 0; comp < nu; comp++)
                    judge(name.c_str(), b * nu + comp, want[b * nu + comp], dev ? dev + b * nu + comp : nullptr, refs[b * nu + comp].s,
                          refs[b * nu + comp].bound(dwave(rowptr[b + 1] - rowptr[b]) + 1));
        };
        if (g_host_only) all("project nu=" + std::to_string(nu), nullptr);
        else {
            GBuf<uint64_t> d_rowptr(rowptr, FILL_INT);
            GBuf<uint32_t> d_col(col, FILL_INT);
            GBuf<int32_t> d_pmap(pmap, FILL_INT);
            GBuf<double> d_val(val, FILL_F64), d_v(v, FILL_F64), d_cv(cv, FILL_F64);
            for (uint32_t wg : {WV, WG})
                for (uint32_t grid : {pca_wave_grid(N, wg), 1u}) {
                    GBuf<double> out(N * nu, FILL_F64);
                    hipLaunchKernelGGL(k_pca_project, dim3(grid), dim3(wg), 0, g_gpu->ctx->stream, d_rowptr.d, d_col.d, d_val.d, N, d_pmap.d, d_v.d, nu, d_cv.d, out.d);
                    g_gpu->launched("k_pca_project");
                    const std::vector<double> h = out.get("out");
                    all("project nu=" + std::to_string(nu) + " wg=" + std::to_string(wg) + " grid=" + std::to_string(grid), h.data());
                }
        }
        case_done("project nu=%u: %llu rows, %u of %u features mapped", nu, (unsigned long long)N, n_used, G);
    }
}

int main(int argc, char **argv) {
    std::string group;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--host-only")) g_host_only = true;
        else if (!std::strcmp(argv[i], "--group") && i + 1 < argc) group = argv[++i];
        else die("usage: test_pca_kernels --host-only | --group prepare|operator|dense|project");
    }
    struct Group {
        const char *name;
        void (*run)();
    };
    const Group groups[4] = {{"prepare", group_prepare}, {"operator", group_operator}, {"dense", group_dense}, {"project", group_project}};
    Gpu *gpu = nullptr;
    if (!g_host_only) g_gpu = gpu = new Gpu();
    bool any = false;
    for (const Group &g : groups) {
        if (!group.empty() && group != g.name) continue;
        any = true;
        g_worst = 0.0L, g_worst_at = "-";
        const auto t0 = std::chrono::steady_clock::now();
        g.run();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        std::printf("group %s: worst deviation / bound = %.4Lf at %s; %.0f ms\n", g.name, g_worst, g_worst_at.c_str(), ms);
    }
    if (!any) die("no group is called %s", group.c_str());
    if (group.empty() || group == "prepare") std::printf("libm log2(1 + x): at most %lld ulps from the rounded log2l(1.0L + x) (LIBM_LOG2_ULPS %d, the device gets %d), at most %lld from that of the f64 argument (LIBM_LOG2_ARG_ULPS %d, the device gets %d)\n",
                    (long long)g_libm_ulps, LIBM_LOG2_ULPS, DEV_LOG2_ULPS, (long long)g_libm_arg_ulps, LIBM_LOG2_ARG_ULPS, DEV_LOG2_ARG_ULPS);
    if (!g_host_only && (group.empty() || group == "prepare")) std::printf("device log2(1 + x): at most %lld ulps from the rounded log2l(1.0L + x), at most %lld from that of the f64 argument\n", (long long)g_dev_ulps, (long long)g_dev_arg_ulps);
    delete gpu;
    std::printf("%d cases\nall tests passed\n", g_cases);
    return 0;
}
