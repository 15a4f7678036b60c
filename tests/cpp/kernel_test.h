// kernel_test.h -- what the kernel test programs (test_{pca,tsne,umap,louvain}_kernels.hip) share: how a program ends on a mismatch, the
// line of a finished case, the generator of the constructed inputs, the context, guarded device buffers and the bit comparison.
// Included before and outside the namespace that wraps the unit under test.
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "stage_common.h"

static const uint64_t GUARD = 64;
static const double U = 0x1.0p-53;

[[noreturn]] static void die(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::fprintf(stdout, "FAIL ");
    std::vfprintf(stdout, fmt, ap);
    std::fprintf(stdout, "\n");
    va_end(ap);
    std::fflush(stdout);
    std::exit(1);
}
static bool g_host_only = false;
static int g_cases = 0;
static void case_done(const char *fmt, ...) {
    char b[400];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(b, sizeof(b), fmt, ap);
    va_end(ap);
    std::printf("ok   %s%s\n", b, g_host_only ? " (host only)" : "");
    g_cases++;
}
static double gamma_k(double k) { return k * U / (1.0 - k * U); }  // Higham, Accuracy and Stability, 3.1
// the same bytes element by element: for an f64 the same bits, a NaN's and the sign of a zero included
template <typename T>
static void same(const char *what, const std::vector<T> &got, const std::vector<T> &want) {
    if (got.size() != want.size()) die("%s: %zu values against %zu", what, got.size(), want.size());
    for (size_t i = 0; i < got.size(); i++) {
        if (std::memcmp(&got[i], &want[i], sizeof(T)) == 0) continue;
        if constexpr (std::is_floating_point<T>::value)
            die("%s[%zu]: %.17g (%a) on the device, %.17g (%a) in the order model", what, i, (double)got[i], (double)got[i], (double)want[i], (double)want[i]);
        else
            die("%s[%zu]: %lld on the device, %lld in the order model", what, i, (long long)got[i], (long long)want[i]);
    }
}

struct Rng {  // splitmix64
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint64_t below(uint64_t m) { return next() % m; }
    double unit() { return ((double)(next() >> 11) + 0.5) * 0x1.0p-53; }  // (0, 1)
    double normal() { return std::sqrt(-2.0 * std::log(unit())) * std::cos(6.283185307179586 * unit()); }
    double nonzero() {  // a normal value away from 0
        const double x = normal();
        return x < 0.0 ? x - 0.25 : x + 0.25;
    }
};

// ---- the device ----------------------------------------------------------------------------------------------------------------------
struct Gpu {
    crgpu_ctx *ctx = nullptr;
    Gpu() {
        const int rc = crgpu_create(&ctx, 0, 1, 0, nullptr);
        if (rc != CRGPU_OK) die("crgpu_create -> %d: %s", rc, crgpu_last_error(nullptr));
    }
    ~Gpu() { crgpu_destroy(ctx); }
    void ok(int rc, const char *what) const {
        if (rc != CRGPU_OK) die("%s -> %d: %s", what, rc, crgpu_last_error(ctx));
    }
    void launched(const char *what) const {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) die("launch of %s: %s", what, hipGetErrorString(e));
    }
};
static Gpu *g_gpu = nullptr;
#define GOK(call) g_gpu->ok((call), #call)
// n elements and GUARD more behind them, all filled with one byte before anything is launched (0xFF: every f64 a NaN); get() asserts
// that the guard came back untouched
template <typename T>
struct GBuf {
    T *d = nullptr;
    uint64_t n;
    int fill;
    GBuf(uint64_t n_, int fill_ = 0xFF) : n(n_), fill(fill_) {
        void *p = nullptr;
        GOK(crgpu_malloc(g_gpu->ctx, &p, (n + GUARD) * sizeof(T)));
        d = (T *)p;
        GOK(crgpu_memset(g_gpu->ctx, d, fill, (n + GUARD) * sizeof(T)));
    }
    GBuf(const std::vector<T> &h, int fill_ = 0xFF) : GBuf(h.size(), fill_) {
        if (n) GOK(crgpu_memcpy_h2d(g_gpu->ctx, d, h.data(), n * sizeof(T)));
    }
    void zero() { GOK(crgpu_memset(g_gpu->ctx, d, 0, n * sizeof(T))); }  // an accumulator: the elements 0, the guard as it was
    GBuf(const GBuf &) = delete;
    GBuf &operator=(const GBuf &) = delete;
    ~GBuf() { (void)crgpu_free(g_gpu->ctx, d); }
    std::vector<T> get(const char *what) const {
        std::vector<T> h(n + GUARD);
        GOK(crgpu_memcpy_d2h(g_gpu->ctx, h.data(), d, (n + GUARD) * sizeof(T)));
        const unsigned char *g = (const unsigned char *)(h.data() + n);
        for (uint64_t i = 0; i < GUARD * sizeof(T); i++)
            if (g[i] != (unsigned char)fill) die("%s: byte %llu behind the %llu elements of the buffer was written", what, (unsigned long long)i, (unsigned long long)n);
        h.resize(n);
        return h;
    }
};
