// test_block_utils.hip -- the wave and workgroup primitives of cellranger_amd/csrc/block_utils.h, one by one, against host loops that
// take the same steps in the same order.  Every comparison is exact; f64 values are compared as bit patterns.  The header needs
// nothing from the library, so this program links nothing but the HIP runtime.
//
//   test_block_utils --host-only     the host models against plain serial loops (no device is touched)
//   test_block_utils                 every case on the device: one launch of at most a few workgroups each
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "block_utils.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(cond, ...)                                 \
    do {                                                 \
        g_checks++;                                      \
        if (!(cond)) {                                   \
            if (g_fail++ < 20) {                         \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                \
                std::printf("\n");                       \
            }                                            \
        }                                                \
    } while (0)
#define HIP_OK(x)                                                                        \
    do {                                                                                 \
        const hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) {                                                          \
            std::printf("%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            std::exit(2);                                                                \
        }                                                                                \
    } while (0)

static uint64_t bits(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return b;
}
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// mixed signs, magnitudes over 32 decades
static double rnd_decades() {
    const double m = 1.0 + (double)(rnd() >> 11) * 0x1.0p-53;
    const double v = m * std::pow(10.0, (double)(int)(rnd() % 33u) - 16.0);
    return (rnd() & 1u) ? -v : v;
}

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n;
    explicit DevBuf(size_t n_, int fill = 0) : n(n_) {
        HIP_OK(hipMalloc(&p, n * sizeof(T)));
        HIP_OK(hipMemset(p, fill, n * sizeof(T)));
    }
    explicit DevBuf(const std::vector<T> &h) : n(h.size()) {
        HIP_OK(hipMalloc(&p, n * sizeof(T)));
        HIP_OK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
    }
    ~DevBuf() { (void)hipFree(p); }
    std::vector<T> get() const {
        std::vector<T> h(n);
        HIP_OK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
        return h;
    }
};

// ---- host models: the steps of the device code, lane by lane -------------------------------------------------------------------
template <typename T>
static void ref_incl_scan(const T *in, T *out, uint32_t W) {  // lanes 0 .. W - 1
    std::vector<T> x(in, in + W), y(W);
    for (uint32_t d = 1; d < W; d <<= 1) {
        for (uint32_t i = 0; i < W; i++) y[i] = i >= d ? (T)(x[i] + x[i - d]) : x[i];  // own + lower
        x = y;
    }
    for (uint32_t i = 0; i < W; i++) out[i] = x[i];
}
template <typename T, typename Op>
static void ref_butterfly(const T *in, T *out, Op op) {  // 64 lanes, distances 32 .. 1, the result of every lane
    T x[64], y[64];
    for (int i = 0; i < 64; i++) x[i] = in[i];
    for (int d = 32; d >= 1; d >>= 1) {
        for (int i = 0; i < 64; i++) y[i] = op(x[i], x[i ^ d]);
        for (int i = 0; i < 64; i++) x[i] = y[i];
    }
    for (int i = 0; i < 64; i++) out[i] = x[i];
}

// ---- wave_incl_scan ---------------------------------------------------------------------------------------------------------------
// 256 threads: waves 0 .. 2 scan their own 64 values inside `if (lane < W)`, their other lanes do something else; wave 3 has left.
template <typename T, uint32_t W>
__global__ __launch_bounds__(256) void k_scan(const T *__restrict__ in, T *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (wave == 3u) return;
    if (lane < W) out[g] = wave_incl_scan<W>(in[g], lane);
    else out[g] = (T)(in[g] + in[g]);
}
#define N_SCAN_PATTERNS 5
template <typename T>
static T scan_input(uint32_t pattern, uint32_t i);
template <>
uint32_t scan_input<uint32_t>(uint32_t pattern, uint32_t i) {
    switch (pattern) {
        case 0: return 1u;
        case 1: return 0u;
        case 2: return (uint32_t)rnd() & 0xFFFFu;
        case 3: return 0xF0000000u + (uint32_t)(rnd() & 0xFFFFFFu);  // the running sum wraps 2^32 many times
        default: return (i & 1u) ? 0xFFFFFFFFu : (uint32_t)rnd();
    }
}
template <>
double scan_input<double>(uint32_t pattern, uint32_t i) {
    switch (pattern) {
        case 0: return 1.0;
        case 1: return 0.0;
        case 2: return (double)(rnd() >> 11) * 0x1.0p-53;
        case 3: return rnd_decades();
        default: return (i & 1u) ? -rnd_decades() : 1e300 * (double)(rnd() & 7u);  // may overflow to +inf; never a NaN (its bits differ by machine)
    }
}
template <typename T>
static bool same(T a, T b);
template <>
bool same<uint32_t>(uint32_t a, uint32_t b) { return a == b; }
template <>
bool same<double>(double a, double b) { return bits(a) == bits(b); }

template <typename T, uint32_t W>
static void test_scan(const char *tname) {
    std::vector<T> in((size_t)N_SCAN_PATTERNS * 256);
    for (uint32_t p = 0; p < N_SCAN_PATTERNS; p++)
        for (uint32_t i = 0; i < 256; i++) in[(size_t)p * 256 + i] = scan_input<T>(p, i);
    DevBuf<T> d_in(in), d_out(in.size(), 0xA5);
    hipLaunchKernelGGL((k_scan<T, W>), dim3(N_SCAN_PATTERNS), dim3(256), 0, 0, d_in.p, d_out.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<T> out = d_out.get();
    T untouched;
    std::memset(&untouched, 0xA5, sizeof(T));
    for (uint32_t p = 0; p < N_SCAN_PATTERNS; p++)
        for (uint32_t w = 0; w < 4; w++) {
            const size_t o = (size_t)p * 256 + w * 64;
            T ref[64];
            ref_incl_scan(&in[o], ref, W);
            for (uint32_t l = 0; l < 64; l++) {
                const T want = w == 3 ? untouched : l < W ? ref[l] : (T)(in[o + l] + in[o + l]);
                CHECK(same(out[o + l], want), "wave_incl_scan<%u> %s pattern %u wave %u lane %u", W, tname, p, w, l);
            }
        }
}
template <typename T>
static void test_scans(const char *tname) {
    test_scan<T, 2>(tname), test_scan<T, 4>(tname), test_scan<T, 8>(tname);
    test_scan<T, 16>(tname), test_scan<T, 32>(tname), test_scan<T, 64>(tname);
}

// ---- the butterfly reductions -----------------------------------------------------------------------------------------------------
struct RedIn {
    uint32_t u32;
    int i32;
    unsigned long long u64;
    long long i64;
    double f64;
};
struct RedOut {
    uint32_t sum_u32, or_u32, min_u32;
    int max_i32;
    unsigned long long sum_u64;
    long long sum_i64;
    double sum_f64, max_f64;
};
__global__ __launch_bounds__(256) void k_reduce(const RedIn *__restrict__ in, RedOut *__restrict__ out) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    const RedIn x = in[g];
    RedOut r;
    r.sum_u32 = wave_sum(x.u32), r.or_u32 = wave_or(x.u32), r.min_u32 = wave_min(x.u32), r.max_i32 = wave_max(x.i32);
    r.sum_u64 = wave_sum(x.u64), r.sum_i64 = wave_sum(x.i64), r.sum_f64 = wave_sum(x.f64), r.max_f64 = wave_max(x.f64);
    out[g] = r;
}
#define N_RED_PATTERNS 8  // one wave each: two workgroups
static RedIn red_input(uint32_t pattern, uint32_t l) {
    RedIn x;
    switch (pattern) {
        case 0:  // ones
            x = RedIn{1u, 1, 1ull, 1ll, 1.0};
            break;
        case 1:  // random
            x = RedIn{(uint32_t)rnd(), (int)(uint32_t)rnd(), rnd(), (long long)rnd(), (double)(rnd() >> 11) * 0x1.0p-53};
            break;
        case 2:  // u32 sums that wrap, u64 sums above 2^32 made of small and of large terms, negative i64
            x = RedIn{0xFFFFFF00u + l, -(int)(l + 1u), 0xFFFFFFFFull - l, -(long long)(rnd() >> 20), rnd_decades()};
            break;
        case 3:  // a single extreme in lane 0
            x = RedIn{l == 0 ? 3u : 1000u + l, l == 0 ? 7 : -5, (1ull << 40) + l, -(1ll << 40) - (long long)l, l == 0 ? 2.5 : -1.0};
            break;
        case 4:  // a single extreme in lane 63
            x = RedIn{l == 63 ? 3u : 1000u + l, l == 63 ? 7 : -5, 1ull << 33, (l & 1u) ? -(1ll << 33) : (1ll << 33), l == 63 ? 2.5 : -1.0};
            break;
        case 5:  // ties: the extreme in several lanes, +0.0 against -0.0 elsewhere
            x = RedIn{(l % 7u) == 3u ? 5u : 9u, (l % 5u) == 1u ? 100 : 99, l & 3u, -(long long)(l & 3u), (l % 9u) == 4u ? 6.0 : (l & 1u) ? -0.0 : 0.0};
            break;
        case 6:  // all equal; or of single bits
            x = RedIn{1u << (l & 31u), -2147483647 - 1, ~0ull, -1ll, -3.0};
            break;
        default:  // f64 over many decades, mixed signs; the other types at their limits
            x = RedIn{l == 17 ? 0u : 0xFFFFFFFFu, l == 40 ? 2147483647 : (int)l, rnd() >> 1, (long long)(rnd() >> 1), rnd_decades()};
    }
    return x;
}
static void test_reductions() {
    std::vector<RedIn> in((size_t)N_RED_PATTERNS * 64);
    for (uint32_t p = 0; p < N_RED_PATTERNS; p++)
        for (uint32_t l = 0; l < 64; l++) in[(size_t)p * 64 + l] = red_input(p, l);
    DevBuf<RedIn> d_in(in);
    DevBuf<RedOut> d_out(in.size(), 0xA5);
    hipLaunchKernelGGL(k_reduce, dim3(N_RED_PATTERNS / 4), dim3(256), 0, 0, d_in.p, d_out.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<RedOut> out = d_out.get();
    for (uint32_t p = 0; p < N_RED_PATTERNS; p++) {
        const RedIn *x = &in[(size_t)p * 64];
        uint32_t su = 0, ou = 0, mu = 0xFFFFFFFFu;
        int mi = -2147483647 - 1;
        unsigned long long s64 = 0, si64 = 0;
        double f[64], fs[64], fm[64];
        for (uint32_t l = 0; l < 64; l++) {
            su += x[l].u32, ou |= x[l].u32, mu = x[l].u32 < mu ? x[l].u32 : mu, mi = x[l].i32 > mi ? x[l].i32 : mi;
            s64 += x[l].u64, si64 += (unsigned long long)x[l].i64, f[l] = x[l].f64;
        }
        ref_butterfly(f, fs, [](double a, double b) { return a + b; });
        ref_butterfly(f, fm, [](double a, double b) { return std::fmax(a, b); });
        for (uint32_t l = 0; l < 64; l++) {  // the result in ALL 64 lanes
            const RedOut &r = out[(size_t)p * 64 + l];
            CHECK(r.sum_u32 == su, "wave_sum(u32) pattern %u lane %u: %u, expected %u", p, l, r.sum_u32, su);
            CHECK(r.or_u32 == ou, "wave_or pattern %u lane %u: %x, expected %x", p, l, r.or_u32, ou);
            CHECK(r.min_u32 == mu, "wave_min(u32) pattern %u lane %u: %u, expected %u", p, l, r.min_u32, mu);
            CHECK(r.max_i32 == mi, "wave_max(int) pattern %u lane %u: %d, expected %d", p, l, r.max_i32, mi);
            CHECK(r.sum_u64 == s64, "wave_sum(u64) pattern %u lane %u: %llu, expected %llu", p, l, r.sum_u64, s64);
            CHECK((unsigned long long)r.sum_i64 == si64, "wave_sum(i64) pattern %u lane %u: %lld, expected %lld", p, l, r.sum_i64, (long long)si64);
            CHECK(bits(r.sum_f64) == bits(fs[l]), "wave_sum(f64) pattern %u lane %u: %a, expected %a", p, l, r.sum_f64, fs[l]);
            CHECK(bits(r.max_f64) == bits(fm[l]) || (r.max_f64 == 0.0 && fm[l] == 0.0),  // fmax may return either zero
                  "wave_max(f64) pattern %u lane %u: %a, expected %a", p, l, r.max_f64, fm[l]);
        }
    }
}

// ---- block_excl_scan ----------------------------------------------------------------------------------------------------------
// twice in a row over the same LDS words on different data; without the trailing barrier the kernel supplies its own.
// (A missing barrier shows only when waves actually race: a failure here would be intermittent, a pass is no proof.)
template <uint32_t THREADS, bool TB>
__global__ __launch_bounds__(THREADS) void k_bscan(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out_a,
                                                   uint32_t *__restrict__ out_b, uint32_t *__restrict__ tot_a) {
    __shared__ uint32_t lds[THREADS / 64];
    const size_t g = (size_t)blockIdx.x * THREADS + threadIdx.x;
    uint32_t t = 0xA5A5A5A5u;
    out_a[g] = block_excl_scan<THREADS, TB>(a[g], lds, &t);
    tot_a[g] = t;
    if (!TB) __syncthreads();
    out_b[g] = block_excl_scan<THREADS, TB>(b[g], lds, nullptr);
}
template <uint32_t THREADS, bool TB>
static void test_bscan() {
    const uint32_t nb = 3;
    std::vector<uint32_t> a((size_t)nb * THREADS), b(a.size());
    for (uint32_t k = 0; k < nb; k++)
        for (uint32_t i = 0; i < THREADS; i++) {
            a[(size_t)k * THREADS + i] = k == 0 ? 1u : k == 1 ? (uint32_t)(rnd() % 1000u) : 0xFF000000u + (uint32_t)(rnd() & 0xFFFFu);
            b[(size_t)k * THREADS + i] = k == 0 ? (uint32_t)(rnd() % 7u) : k == 1 ? 0u : (uint32_t)rnd();
        }
    DevBuf<uint32_t> d_a(a), d_b(b), d_oa(a.size(), 0xA5), d_ob(a.size(), 0xA5), d_ta(a.size(), 0x5A);
    hipLaunchKernelGGL((k_bscan<THREADS, TB>), dim3(nb), dim3(THREADS), 0, 0, d_a.p, d_b.p, d_oa.p, d_ob.p, d_ta.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<uint32_t> oa = d_oa.get(), ob = d_ob.get(), ta = d_ta.get();
    for (uint32_t k = 0; k < nb; k++) {
        uint32_t tot = 0, ra = 0, rb = 0;
        for (uint32_t i = 0; i < THREADS; i++) tot += a[(size_t)k * THREADS + i];
        for (uint32_t i = 0; i < THREADS; i++) {
            const size_t g = (size_t)k * THREADS + i;
            CHECK(oa[g] == ra, "block_excl_scan<%u, %d> first call, workgroup %u thread %u: %u, expected %u", THREADS, (int)TB, k, i, oa[g], ra);
            CHECK(ob[g] == rb, "block_excl_scan<%u, %d> second call, workgroup %u thread %u: %u, expected %u", THREADS, (int)TB, k, i, ob[g], rb);
            CHECK(ta[g] == tot, "block_excl_scan<%u, %d> total, workgroup %u thread %u: %u, expected %u", THREADS, (int)TB, k, i, ta[g], tot);
            ra += a[g], rb += b[g];
        }
    }
}

// ---- block_reserve_256 ----------------------------------------------------------------------------------------------------------
#define RESERVE_START 1000ull  // the counter before the launch: a workgroup that asks for nothing must come back with 0, not with this
__global__ __launch_bounds__(256) void k_reserve(const uint32_t *__restrict__ counts, unsigned long long *__restrict__ counter,
                                                 unsigned long long *__restrict__ slot) {
    __shared__ __attribute__((aligned(8))) uint32_t lds[10];
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    slot[g] = block_reserve_256(counts[g], counter, lds);
}
static void test_reserve() {
    std::vector<uint32_t> counts(3 * 256);
    unsigned long long total = 0;
    for (uint32_t i = 0; i < 256; i++) {
        counts[i] = 0u, counts[256 + i] = 1u, counts[512 + i] = (rnd() % 3u) ? (uint32_t)(rnd() % 6u) : 0u;
        total += counts[256 + i] + counts[512 + i];
    }
    DevBuf<uint32_t> d_counts(counts);
    DevBuf<unsigned long long> d_counter(std::vector<unsigned long long>(1, RESERVE_START)), d_slot(counts.size(), 0xA5);
    hipLaunchKernelGGL(k_reserve, dim3(3), dim3(256), 0, 0, d_counts.p, d_counter.p, d_slot.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<unsigned long long> slot = d_slot.get();
    const unsigned long long end = d_counter.get()[0];
    CHECK(end == RESERVE_START + total, "block_reserve_256: the counter ends at %llu, expected %llu", end, RESERVE_START + total);
    std::vector<uint8_t> taken(total, 0);
    for (uint32_t k = 0; k < 3; k++) {
        unsigned long long next = 0;  // the slot the workgroup's next thread must receive
        for (uint32_t i = 0; i < 256; i++) {
            const size_t g = (size_t)k * 256 + i;
            if (k == 0) {  // nothing asked for: no atomic, so the base is 0 and not the counter's value
                CHECK(slot[g] == 0ull, "block_reserve_256: thread %u of the empty workgroup received %llu", i, slot[g]);
                continue;
            }
            if (i == 0) next = slot[g];
            CHECK(slot[g] == next, "block_reserve_256: workgroup %u thread %u received %llu, expected %llu", k, i, slot[g], next);
            for (uint32_t c = 0; c < counts[g]; c++) {
                const unsigned long long s = slot[g] + c - RESERVE_START;  // (wraps below the start)
                CHECK(s < total && !taken[s < total ? s : 0], "block_reserve_256: slot %llu of workgroup %u thread %u is outside or taken twice", slot[g] + c, k, i);
                if (s < total) taken[s] = 1;
            }
            next = slot[g] + counts[g];
        }
    }
    for (unsigned long long s = 0; s < total; s++) CHECK(taken[s], "block_reserve_256: slot %llu was not handed out", RESERVE_START + s);
}

// ---- the count tail and the write tail of the compactions ---------------------------------------------------------------------
template <uint32_t WAVES>
__global__ __launch_bounds__(WAVES * 64) void k_bsum(const uint32_t *__restrict__ in, uint32_t *__restrict__ out) {
    __shared__ uint32_t lds[WAVES];
    block_sum_to_first<WAVES>(in[(size_t)blockIdx.x * (WAVES * 64) + threadIdx.x], lds, &out[blockIdx.x]);
}
template <uint32_t WAVES>
static void test_bsum() {
    const uint32_t nb = 4, T = WAVES * 64;
    std::vector<uint32_t> in((size_t)nb * T);
    for (uint32_t k = 0; k < nb; k++)
        for (uint32_t i = 0; i < T; i++)
            in[(size_t)k * T + i] = k == 0 ? 1u : k == 1 ? 0u : k == 2 ? (uint32_t)(rnd() % 9u) : 0xFFF00000u + (uint32_t)(rnd() & 0xFFFFu);
    DevBuf<uint32_t> d_in(in), d_out(nb + 1, 0xA5);
    hipLaunchKernelGGL((k_bsum<WAVES>), dim3(nb), dim3(T), 0, 0, d_in.p, d_out.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<uint32_t> out = d_out.get();
    for (uint32_t k = 0; k < nb; k++) {
        uint32_t s = 0;
        for (uint32_t i = 0; i < T; i++) s += in[(size_t)k * T + i];
        CHECK(out[k] == s, "block_sum_to_first<%u> workgroup %u: %u, expected %u", WAVES, k, out[k], s);
    }
    CHECK(out[nb] == 0xA5A5A5A5u, "block_sum_to_first<%u> wrote behind its output", WAVES);
}

template <uint32_t N>
__global__ __launch_bounds__(256) void k_words(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t *__restrict__ total_out) {
    __shared__ uint32_t ws[N + 1];  // one word more: nobody may touch it
    __shared__ uint32_t total;
    if (threadIdx.x < N) ws[threadIdx.x] = in[(size_t)blockIdx.x * N + threadIdx.x];
    if (threadIdx.x == 0) ws[N] = 0x5A5A5A5Au, total = 0xA5A5A5A5u;
    __syncthreads();
    block_scan_words<N>(ws, &total);  // all 256 threads call it
    __syncthreads();
    if (threadIdx.x <= N) out[(size_t)blockIdx.x * (N + 1) + threadIdx.x] = ws[threadIdx.x];
    if (threadIdx.x == 255) total_out[blockIdx.x] = total;
}
template <uint32_t N>
static void test_words() {
    const uint32_t nb = 4;
    std::vector<uint32_t> in((size_t)nb * N);
    for (uint32_t k = 0; k < nb; k++)
        for (uint32_t i = 0; i < N; i++)
            in[(size_t)k * N + i] = k == 0 ? 1u : k == 1 ? 0u : k == 2 ? (uint32_t)(rnd() % 65u) : 0xF8000000u + (uint32_t)(rnd() & 0xFFFFFu);
    DevBuf<uint32_t> d_in(in), d_out((size_t)nb * (N + 1), 0xA5), d_tot(nb, 0x5A);
    hipLaunchKernelGGL((k_words<N>), dim3(nb), dim3(256), 0, 0, d_in.p, d_out.p, d_tot.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    const std::vector<uint32_t> out = d_out.get(), tot = d_tot.get();
    for (uint32_t k = 0; k < nb; k++) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < N; i++) {
            CHECK(out[(size_t)k * (N + 1) + i] == run, "block_scan_words<%u> workgroup %u word %u: %u, expected %u", N, k, i, out[(size_t)k * (N + 1) + i], run);
            run += in[(size_t)k * N + i];
        }
        CHECK(out[(size_t)k * (N + 1) + N] == 0x5A5A5A5Au, "block_scan_words<%u> workgroup %u wrote behind its words", N, k);
        CHECK(tot[k] == run, "block_scan_words<%u> workgroup %u total: %u, expected %u", N, k, tot[k], run);
    }
}

// ---- the host models against plain loops ------------------------------------------------------------------------------------------
static void test_host_models() {
    for (uint32_t W = 2; W <= 64; W <<= 1)
        for (int rep = 0; rep < 8; rep++) {
            uint32_t in[64], out[64], run = 0;
            double fin[64], fout[64], frun = 0.0;
            for (uint32_t i = 0; i < 64; i++) in[i] = (uint32_t)rnd(), fin[i] = (double)(rnd() & 0xFFFFu);  // integers: any order is exact
            ref_incl_scan(in, out, W), ref_incl_scan(fin, fout, W);
            for (uint32_t i = 0; i < W; i++) {
                run += in[i], frun += fin[i];
                CHECK(out[i] == run, "host scan model, u32, W %u lane %u", W, i);
                CHECK(fout[i] == frun, "host scan model, f64, W %u lane %u", W, i);
            }
        }
    for (int rep = 0; rep < 8; rep++) {
        double f[64], fs[64], fm[64], s = 0.0, m = -1.0;
        for (int i = 0; i < 64; i++) f[i] = (double)(rnd() & 0xFFFFFu), s += f[i], m = f[i] > m ? f[i] : m;
        ref_butterfly(f, fs, [](double a, double b) { return a + b; });
        ref_butterfly(f, fm, [](double a, double b) { return std::fmax(a, b); });
        for (int i = 0; i < 64; i++) CHECK(fs[i] == s && fm[i] == m, "host butterfly model, lane %d", i);
        // lane 0 of the butterfly adds the operand pairs of a tree of downward shifts, in its order
        double t[128] = {0};
        for (int i = 0; i < 64; i++) t[i] = f[i] = rnd_decades();
        for (int d = 32; d >= 1; d >>= 1)
            for (int i = 0; i < 64; i++) t[i] = t[i] + t[i + d];  // ascending i: t[i + d] is still the value before the step
        ref_butterfly(f, fs, [](double a, double b) { return a + b; });
        CHECK(bits(t[0]) == bits(fs[0]), "the butterfly's lane 0 against the downward tree: %a, %a", fs[0], t[0]);
    }
}

int main(int argc, char **argv) {
    bool host_only = false;
    for (int i = 1; i < argc; i++) host_only |= std::strcmp(argv[i], "--host-only") == 0;
    test_host_models();
    if (!host_only) {
        test_scans<uint32_t>("u32"), test_scans<double>("f64");
        test_reductions();
        test_bscan<64, true>(), test_bscan<64, false>(), test_bscan<256, true>(), test_bscan<256, false>();
        test_bscan<1024, true>(), test_bscan<1024, false>();
        test_reserve();
        test_bsum<4>(), test_bsum<16>();
        test_words<4>(), test_words<32>(), test_words<64>();
    }
    std::printf("%d checks, %d failed%s\n", g_checks, g_fail, host_only ? " (host only)" : "");
    if (g_fail) return 1;
    std::printf("all tests passed\n");
    return 0;
}
