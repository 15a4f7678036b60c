// Differential test of the device sort (cellranger_amd/csrc/sort.hip) against std::stable_sort on the host: every entry point
// that the stages stand on -- cr_radix_sort_u32 / _u64 / _u64_full, the finishing step cr_order_runs behind a sort on the top
// bits, cr_partition_by_owner[_kv], cr_scan_small -- plus the host-side digit plans (cr_sweep_plan, cr_sort_low_bits).
// All data are integers: every comparison is exact.  The payload of a sort is the input index, so the expected payload of a
// stable sort is known exactly; key bits outside the sorted range are random and have to arrive unchanged.
//
// The sizes are derived from the tuning constants of sort.hip, which the Python wrapper (tests/test_gpu_sort_cpp.py) reads
// out of the source text and passes as --const NAME=VALUE: a retuned constant moves the cases with it.
//
//   test_sort --host-only                      the digit plans, no device
//   test_sort --group u32|u64|finish|partition|scan|large  --const CHUNK=16384 ...
//
// One line per case, "all tests passed" at the end; the first mismatch prints the case, the index and the two values and
// ends the program with status 1.
// Build: hipcc --offload-arch=gfx950 -std=c++17 -Icellranger_amd/csrc -Iinclude tests/cpp/test_sort.hip -Lcellranger_amd -lcrgpu
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "common.h"

// sort.hip entry points that common.h does not declare (stage_common.h does, with much else)
int cr_scan_small(crgpu_ctx *ctx, uint32_t *d_data, uint64_t n, uint32_t *d_total_out);
int cr_partition_by_owner(crgpu_ctx *ctx, const uint64_t *d_in, uint64_t *d_out, uint64_t n, uint32_t sh_bc, uint32_t n_ranks,
                          const uint32_t *bounds, uint64_t *counts_out);

// fixed seeds, one per group; a case adds its ordinal
static const uint64_t SEED_U32 = 0x5eed0032ull, SEED_U64 = 0x5eed0064ull, SEED_FINISH = 0x5eedf1a1ull, SEED_PART = 0x5eed9a27ull,
                      SEED_SCAN = 0x5eed5ca9ull, SEED_LARGE = 0x5eed1a26ull;

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

static std::map<std::string, uint64_t> g_const;
static uint64_t C(const char *name) {
    auto it = g_const.find(name);
    if (it == g_const.end()) die("constant %s was not given (--const %s=VALUE)", name, name);
    return it->second;
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
};

static uint64_t bitmask(uint32_t bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1ull; }

static void parallel_for(size_t n, const std::function<void(size_t)> &fn) {
    size_t nt = std::thread::hardware_concurrency();
    nt = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(nt, 16), n));
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; t++)
        th.emplace_back([&] {
            for (size_t i = next++; i < n; i = next++) fn(i);
        });
    for (auto &t : th) t.join();
}

// ---- the device ---------------------------------------------------------------------------------------------------------------
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
    template <typename T>
    T *alloc(uint64_t count) {
        void *p = nullptr;
        ok(crgpu_malloc(ctx, &p, std::max<uint64_t>(count, 1) * sizeof(T)), "crgpu_malloc");
        return (T *)p;
    }
    void up(void *d, const void *h, uint64_t bytes) {
        if (bytes) ok(crgpu_memcpy_h2d(ctx, d, h, bytes), "crgpu_memcpy_h2d");
    }
    void down(void *h, const void *d, uint64_t bytes) {
        if (bytes) ok(crgpu_memcpy_d2h(ctx, h, d, bytes), "crgpu_memcpy_d2h");
    }
    void fill(void *d, int v, uint64_t bytes) {
        if (bytes) ok(crgpu_memset(ctx, d, v, bytes), "crgpu_memset");
    }
};
#define GOK(g, call) (g).ok((call), #call)

// elements behind the n a call is given: filled with GUARD_BYTE, they must come back untouched
static const uint64_t GUARD = 64;
static const int GUARD_BYTE = 0xA5;
template <typename T>
static T guard_value() {
    T v;
    std::memset(&v, GUARD_BYTE, sizeof(T));
    return v;
}

// ---- radix sorts: cases, the host reference, the comparison -----------------------------------------------------------------
static const char *PATTERN_NAMES[7] = {"uniform", "all-equal", "ascending", "descending", "two-values", "hot-digit-99", "shuffled-iota"};

template <typename K>
struct SortCase {
    uint64_t n = 0;
    uint32_t lo = 0, hi = 0;
    int pattern = 0;
    bool kv = false;
    uint64_t seed = 0;
    std::vector<K> in;            // the keys as given
    std::vector<uint32_t> order;  // std::stable_sort of 0 .. n-1 by the sorted bits: expected payload, expected key = in[order[i]]
    std::string name(const char *entry) const {
        char b[200];
        std::snprintf(b, sizeof(b), "%s %s n=%llu bits=[%u,%u) %s", entry, kv ? "keys+payload" : "keys", (unsigned long long)n, lo, hi,
                      PATTERN_NAMES[pattern]);
        return b;
    }
    void release() {
        std::vector<K>().swap(in);
        std::vector<uint32_t>().swap(order);
    }
};

// non-decreasing over i = 0 .. n-1, within `t` bits
static uint64_t ascending_field(uint64_t i, uint64_t n, uint32_t t) {
    if (t >= 40 || n <= (1ull << t)) return i;
    return i * (1ull << t) / n;
}

template <typename K>
static void prepare_sort_case(SortCase<K> &c) {
    const uint32_t t = c.hi - c.lo, kbits = 8 * sizeof(K);
    const uint64_t M = bitmask(t), n = c.n;
    Rng rng(c.seed);
    std::vector<uint64_t> field(n);
    switch (c.pattern) {
        case 0:
            for (auto &f : field) f = rng.next() & M;
            break;
        case 1: {
            const uint64_t v = rng.next() & M;
            for (auto &f : field) f = v;
            break;
        }
        case 2:
            for (uint64_t i = 0; i < n; i++) field[i] = ascending_field(i, n, t) & M;
            break;
        case 3:
            for (uint64_t i = 0; i < n; i++) field[i] = ascending_field(n - 1 - i, n, t) & M;
            break;
        case 4: {
            const uint64_t a = rng.next() & M;
            uint64_t b = rng.next() & M;
            if (b == a) b = a ^ 1ull;
            for (uint64_t i = 0; i < n; i++) field[i] = (i & 1) ? a : b;
            break;
        }
        case 5: {  // 99 % of the keys carry one value of the first pass's digit
            const uint64_t hot = rng.next() & 0xFFull;
            for (auto &f : field) {
                f = rng.next() & M;
                if (rng.below(100) != 0) f = ((f & ~0xFFull) | hot) & M;
            }
            break;
        }
        default: {
            std::vector<uint32_t> p(n);
            std::iota(p.begin(), p.end(), 0u);
            for (uint64_t i = n; i > 1; i--) std::swap(p[i - 1], p[rng.below(i)]);
            for (uint64_t i = 0; i < n; i++) field[i] = p[i] & M;
        }
    }
    c.in.resize(n);
    const uint64_t keep = t >= 64 ? ~0ull : (M << c.lo);
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t garbage = rng.next() & ~keep & bitmask(kbits);
        c.in[i] = (K)(((field[i] << c.lo) & keep) | garbage);
    }
    c.order.resize(n);
    std::iota(c.order.begin(), c.order.end(), 0u);
    const uint32_t lo = c.lo;
    const K *in = c.in.data();
    std::stable_sort(c.order.begin(), c.order.end(),
                     [=](uint32_t a, uint32_t b) { return (((uint64_t)in[a] >> lo) & M) < (((uint64_t)in[b] >> lo) & M); });
}

template <typename K>
struct SortBufs {
    Gpu &g;
    uint64_t cap;
    K *d_keys, *d_tmp;
    uint32_t *d_vals, *d_vtmp;
    std::vector<K> hk, gk;
    std::vector<uint32_t> hv, gv;
    SortBufs(Gpu &g_, uint64_t cap_) : g(g_), cap(cap_) {
        d_keys = g.alloc<K>(cap + GUARD);
        d_tmp = g.alloc<K>(cap + GUARD);
        d_vals = g.alloc<uint32_t>(cap + GUARD);
        d_vtmp = g.alloc<uint32_t>(cap + GUARD);
    }
    ~SortBufs() {
        crgpu_free(g.ctx, d_keys);
        crgpu_free(g.ctx, d_tmp);
        crgpu_free(g.ctx, d_vals);
        crgpu_free(g.ctx, d_vtmp);
    }
    // keys (and the payload 0 .. n-1) into the first buffers, guards behind them and behind n in the second buffers
    void load(const std::vector<K> &in, bool kv) {
        const uint64_t n = in.size();
        if (n > cap) die("test bug: %llu keys for buffers of %llu", (unsigned long long)n, (unsigned long long)cap);
        hk.assign(in.begin(), in.end());
        hk.resize(n + GUARD, guard_value<K>());
        g.up(d_keys, hk.data(), hk.size() * sizeof(K));
        g.fill(d_tmp, GUARD_BYTE, (n + GUARD) * sizeof(K));
        if (kv) {
            hv.resize(n);
            std::iota(hv.begin(), hv.end(), 0u);
            hv.resize(n + GUARD, guard_value<uint32_t>());
            g.up(d_vals, hv.data(), hv.size() * sizeof(uint32_t));
            g.fill(d_vtmp, GUARD_BYTE, (n + GUARD) * sizeof(uint32_t));
        }
    }
    // the result (n elements and the guards) from the buffer result_in_tmp names; the guards of the other buffer are checked too
    void fetch(const std::string &name, uint64_t n, bool kv, bool in_tmp) {
        gk.resize(n + GUARD);
        g.down(gk.data(), in_tmp ? d_tmp : d_keys, gk.size() * sizeof(K));
        check_guard(name, "keys", gk.data() + n);
        K other[GUARD];
        g.down(other, (in_tmp ? d_keys : d_tmp) + n, sizeof(other));
        check_guard(name, "the other key buffer", other);
        if (kv) {
            gv.resize(n + GUARD);
            g.down(gv.data(), in_tmp ? d_vtmp : d_vals, gv.size() * sizeof(uint32_t));
            check_guard(name, "payload", gv.data() + n);
            uint32_t vo[GUARD];
            g.down(vo, (in_tmp ? d_vals : d_vtmp) + n, sizeof(vo));
            check_guard(name, "the other payload buffer", vo);
        }
    }
    template <typename T>
    static void check_guard(const std::string &name, const char *what, const T *p) {
        for (uint64_t i = 0; i < GUARD; i++)
            if (p[i] != guard_value<T>())
                die("%s: %s: element n+%llu behind the data was overwritten: got 0x%llx expected 0x%llx", name.c_str(), what,
                    (unsigned long long)i, (unsigned long long)p[i], (unsigned long long)guard_value<T>());
    }
};

template <typename K>
static void compare_sorted(const std::string &name, const SortCase<K> &c, const SortBufs<K> &b) {
    for (uint64_t i = 0; i < c.n; i++) {
        const K want = c.in[c.order[i]];
        if (b.gk[i] != want)
            die("%s: key at index %llu: got 0x%llx expected 0x%llx", name.c_str(), (unsigned long long)i, (unsigned long long)b.gk[i],
                (unsigned long long)want);
    }
    if (c.kv)
        for (uint64_t i = 0; i < c.n; i++)
            if (b.gv[i] != c.order[i])
                die("%s: payload at index %llu: got %u expected %u (stable order)", name.c_str(), (unsigned long long)i, b.gv[i], c.order[i]);
}

// cases are prepared (input + host reference) in parallel, a batch at a time, and run on the device one after the other
template <typename CASE>
static void run_batched(std::vector<CASE> &cases, const std::function<void(CASE &)> &prepare, const std::function<void(CASE &)> &run,
                        size_t batch = 32) {
    for (size_t b0 = 0; b0 < cases.size(); b0 += batch) {
        const size_t b1 = std::min(cases.size(), b0 + batch);
        parallel_for(b1 - b0, [&](size_t i) { prepare(cases[b0 + i]); });
        for (size_t i = b0; i < b1; i++) {
            run(cases[i]);
            cases[i].release();
        }
    }
}

static std::vector<uint64_t> ladder(uint64_t chunk) {
    return {0, 1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, 4 * chunk - 1, 4 * chunk + 1, 9 * chunk + 17};
}

static uint64_t g_cases = 0;
static void passed(const std::string &name) {
    std::printf("ok %s\n", name.c_str());
    g_cases++;
}

static void group_u32(Gpu &g) {
    const uint64_t chunk = C("CHUNK");  // 32-bit keys: the same chunk with and without a payload
    static const uint32_t ranges[][2] = {{0, 32}, {0, 2}, {0, 1}, {3, 11}, {5, 14}, {0, 17}, {0, 18}, {7, 32}};
    std::vector<SortCase<uint32_t>> cases;
    for (int kv = 0; kv < 2; kv++)
        for (uint64_t n : ladder(chunk))
            for (auto &r : ranges)
                for (int p = 0; p < 7; p++) {
                    SortCase<uint32_t> c;
                    c.n = n, c.lo = r[0], c.hi = r[1], c.pattern = p, c.kv = kv != 0, c.seed = SEED_U32 + cases.size();
                    cases.push_back(c);
                }
    SortBufs<uint32_t> b(g, 9 * chunk + 17);
    run_batched<SortCase<uint32_t>>(cases, prepare_sort_case<uint32_t>, [&](SortCase<uint32_t> &c) {
        const std::string name = c.name("cr_radix_sort_u32");
        b.load(c.in, c.kv);
        bool in_tmp = false;
        GOK(g, cr_radix_sort_u32(g.ctx, b.d_keys, b.d_tmp, c.kv ? b.d_vals : nullptr, c.kv ? b.d_vtmp : nullptr, c.n, c.lo, c.hi, &in_tmp));
        b.fetch(name, c.n, c.kv, in_tmp);
        compare_sorted(name, c, b);
        passed(name);
    });
}

static void group_u64(Gpu &g) {
    static const uint32_t ranges[][2] = {{0, 64}, {0, 61}, {12, 57}, {0, 40}, {0, 33}, {0, 9}};
    std::vector<SortCase<uint64_t>> cases;
    uint64_t cap = 0;
    for (int kv = 0; kv < 2; kv++) {
        const uint64_t chunk = kv ? C("CHUNK_KV64") : C("CHUNK");
        std::vector<uint64_t> ns = ladder(chunk);
        // more than OS_GROUP x 8 XCDs chunks: every XCD's ticket counter enters its second group; 9 chunks already need a
        // second round of SORT_LB look-back reads
        const uint64_t many = std::max<uint64_t>(70, C("OS_GROUP") * 8 + 6);
        if (9 <= C("SORT_LB")) ns.push_back((C("SORT_LB") + 1) * chunk + 17);
        ns.push_back(many * chunk + 3);
        for (uint64_t n : ns) {
            cap = std::max(cap, n);
            for (auto &r : ranges)
                for (int p = 0; p < 7; p++) {
                    SortCase<uint64_t> c;
                    c.n = n, c.lo = r[0], c.hi = r[1], c.pattern = p, c.kv = kv != 0, c.seed = SEED_U64 + cases.size();
                    cases.push_back(c);
                }
        }
    }
    SortBufs<uint64_t> b(g, cap);
    run_batched<SortCase<uint64_t>>(cases, prepare_sort_case<uint64_t>, [&](SortCase<uint64_t> &c) {
        uint32_t *v = c.kv ? b.d_vals : nullptr, *vt = c.kv ? b.d_vtmp : nullptr;
        for (int variant = 0; variant < 3; variant++) {
            if (variant == 2 && c.lo != 0) continue;  // _full sorts from bit 0
            const std::string name =
                c.name(variant == 0 ? "cr_radix_sort_u64" : variant == 1 ? "cr_radix_sort_u64 CRGPU_SORT_STATUS64=1" : "cr_radix_sort_u64_full");
            b.load(c.in, c.kv);
            bool in_tmp = false;
            if (variant == 1) setenv("CRGPU_SORT_STATUS64", "1", 1);  // read per call
            const int rc = variant == 2 ? cr_radix_sort_u64_full(g.ctx, b.d_keys, b.d_tmp, v, vt, c.n, c.hi, &in_tmp)
                                        : cr_radix_sort_u64(g.ctx, b.d_keys, b.d_tmp, v, vt, c.n, c.lo, c.hi, &in_tmp);
            if (variant == 1) unsetenv("CRGPU_SORT_STATUS64");
            g.ok(rc, name.c_str());
            b.fetch(name, c.n, c.kv, in_tmp);
            compare_sorted(name, c, b);
            passed(name);
        }
    });
    uint64_t fallbacks = 0;
    GOK(g, crgpu_get_stat(g.ctx, CRGPU_STAT_SORT_FALLBACKS, &fallbacks));
    std::printf("look-back watchdog fallbacks: %llu\n", (unsigned long long)fallbacks);
}

// ---- the finishing step -------------------------------------------------------------------------------------------------------
// A buffer is built as it lies after the passes on the top bits: runs of equal (key >> low), top values ascending.  The input is
// a shuffle of it that keeps the relative order inside every run, so the stable sort on [low, hi) reproduces the layout exactly
// and every run meets the descent / word / span / workgroup borders it was placed on.
struct RunBuilder;
// ONE_DESCENT: ascending but for a single descent at index `split`.  SPARSE_HIGH (more than 9 low bits, where the walk through
// memory buckets twice): nearly all keys in the last bucket of the bits above the low eight, the other buckets hold 2, 2, 1, 0, ...
enum RunKind { RANDOM, ORDERED, COPIES, ONE_DESCENT, SPARSE_HIGH };

struct FinishCase {
    std::string label;
    uint32_t low = 0, hi = 0;
    uint64_t seed = 0;
    bool expect_fell_back = false;
    int heads_rotation = -1;  // >= 0: only this one of the head variants (the long single-lane walks are run once per payload mode)
    std::function<void(RunBuilder &)> build;
    // prepared:
    std::vector<uint64_t> in;            // keys as given to the sort on the top bits
    std::vector<uint64_t> post;          // ... as they lie after it
    std::vector<uint32_t> post_val;      // ... and the payload (input index) that lies there
    std::vector<uint32_t> run_start;     // start of every run in `post`, plus n
    std::vector<uint8_t> run_unordered;  // the run holds a descent
    std::vector<uint32_t> order;         // stable full sort of the input: expected keys in[order[i]]
    void release() {
        std::vector<uint64_t>().swap(in);
        std::vector<uint64_t>().swap(post);
        std::vector<uint32_t>().swap(post_val);
        std::vector<uint32_t>().swap(run_start);
        std::vector<uint8_t>().swap(run_unordered);
        std::vector<uint32_t>().swap(order);
    }
};

struct RunBuilder {
    uint32_t low;
    Rng rng;
    std::vector<uint32_t> lows;       // low bits of every key
    std::vector<uint32_t> run_start;  // start of every run
    RunBuilder(uint32_t low_, uint64_t seed) : low(low_), rng(seed) {}
    uint64_t pos() const { return lows.size(); }
    void run(uint64_t len, RunKind kind, uint64_t split = 0) {
        if (!len) return;
        const uint32_t lm = (uint32_t)bitmask(low);
        run_start.push_back((uint32_t)pos());
        std::vector<uint32_t> v(len);
        for (auto &x : v) x = (uint32_t)rng.next() & lm;
        if (kind == COPIES) std::fill(v.begin(), v.end(), v[0]);
        if (kind == SPARSE_HIGH && low >= 10) {
            const uint32_t nb = 1u << (low - 8);
            uint64_t at = 0;
            for (auto &x : v) x = ((nb - 1) << 8) | (x & 0xFFu);
            for (uint32_t d = 0; d + 1 < nb && at + 2 <= len / 2; d++) {
                if (d % 4 == 3) continue;
                v[at++] = (d << 8) | 200u;
                if (d % 4 != 2) v[at++] = (d << 8) | 100u;
            }
            for (uint64_t i = len; i > 1; i--) std::swap(v[i - 1], v[rng.below(i)]);
        }
        if (kind == ORDERED || kind == ONE_DESCENT) std::sort(v.begin(), v.end());
        if (kind == ONE_DESCENT) {
            if (len < 2 || split < 1 || split >= len) die("test bug: a descent at %llu of %llu keys", (unsigned long long)split, (unsigned long long)len);
            v[0] = 0, v[len - 1] = lm;  // the largest keys first: the only descent is where the smallest follows the largest
            std::rotate(v.begin(), v.begin() + (len - split), v.end());
        }
        lows.insert(lows.end(), v.begin(), v.end());
    }
    // single keys and, one time in eight, a short run in random order, up to position `target`
    void pad_to(uint64_t target) {
        if (target < pos()) die("test bug: cannot pad back from %llu to %llu", (unsigned long long)pos(), (unsigned long long)target);
        while (pos() < target) {
            uint64_t len = 1;
            if (rng.below(8) == 0) len = 2 + rng.below(C("RR_SHORT") - 1);
            run(std::min<uint64_t>(len, target - pos()), RANDOM);
        }
    }
    void pad(uint64_t count) { pad_to(pos() + count); }
    // a run whose index `before` lies on `border`
    void across(uint64_t border, uint64_t len, RunKind kind, uint64_t before) {
        pad_to(border - before);
        run(len, kind, before);
    }
    uint64_t next_multiple(uint64_t m, uint64_t room) const { return (pos() + room + m - 1) / m * m; }
};

static void prepare_finish_case(FinishCase &c) {
    RunBuilder rb(c.low, c.seed);
    c.build(rb);
    const uint64_t n = rb.pos();
    const uint32_t n_runs = (uint32_t)rb.run_start.size(), t = c.hi - c.low;
    c.run_start = rb.run_start;
    c.run_start.push_back((uint32_t)n);
    // top values: ascending, spread over all bits of [low, hi)
    const uint64_t step = (t >= 64 ? ~0ull : (1ull << t)) / std::max<uint32_t>(n_runs, 1u);
    if (step < 1) die("test bug: %u runs do not fit %u top bits", n_runs, t);
    c.post.resize(n);
    c.run_unordered.assign(n_runs, 0);
    for (uint32_t r = 0; r < n_runs; r++) {
        const uint64_t top = (uint64_t)r * step + rb.rng.below(step);
        for (uint32_t i = c.run_start[r]; i < c.run_start[r + 1]; i++) {
            c.post[i] = (top << c.low) | rb.lows[i];
            if (i > c.run_start[r] && rb.lows[i] < rb.lows[i - 1]) c.run_unordered[r] = 1;
        }
    }
    // the input: a random permutation that keeps the order inside every run
    std::vector<uint32_t> slot(n);
    std::iota(slot.begin(), slot.end(), 0u);
    for (uint64_t i = n; i > 1; i--) std::swap(slot[i - 1], slot[rb.rng.below(i)]);
    for (uint32_t r = 0; r < n_runs; r++) std::sort(slot.begin() + c.run_start[r], slot.begin() + c.run_start[r + 1]);
    c.in.resize(n);
    for (uint64_t i = 0; i < n; i++) c.in[slot[i]] = c.post[i];
    c.post_val = slot;
    c.order.resize(n);
    std::iota(c.order.begin(), c.order.end(), 0u);
    const uint64_t *in = c.in.data();
    std::stable_sort(c.order.begin(), c.order.end(), [=](uint32_t a, uint32_t b) { return in[a] < in[b]; });
}

struct HeadVariant {
    uint32_t shift;
    uint64_t tile;
};

static void group_finish(Gpu &g) {
    const uint64_t RR_SHORT = C("RR_SHORT"), OR_CAP = C("OR_CAP"), RL_CAP = C("RL_CAP"), OR_MAX = C("OR_MAX");
    const uint64_t span = 64 * C("FD_ITEMS"), share = 64 * C("RR_WORDS");
    const std::vector<uint64_t> classes = {1, 2, RR_SHORT, RR_SHORT + 1, OR_CAP, OR_CAP + 1, 64, 65, RL_CAP, RL_CAP + 1};
    static const uint32_t lows[] = {1, 5, 7, 8, 10, 11, 16};
    std::vector<FinishCase> cases;
    int rotation = 0;
    for (uint32_t low : lows) {
        const uint32_t hi = low == 16 ? 64 : low == 8 ? 56 : 61;
        auto add = [&](const char *label, bool fell_back, int heads_rotation, std::function<void(RunBuilder &)> build) {
            FinishCase c;
            c.label = label, c.low = low, c.hi = hi, c.seed = SEED_FINISH + cases.size(), c.expect_fell_back = fell_back;
            c.heads_rotation = heads_rotation, c.build = std::move(build);
            cases.push_back(std::move(c));
        };
        // every class of run length, in every kind, at arbitrary places; then on the borders of the kernels' shares
        add("all classes and borders", false, -1, [=](RunBuilder &b) {
            b.run(RR_SHORT + 1, RANDOM);  // the very start of the buffer
            for (uint64_t len : classes) {
                b.pad(1 + b.rng.below(100));
                b.run(len, RANDOM);
                if (len < 2) continue;
                b.pad(1 + b.rng.below(100));
                b.run(len, ORDERED);
                b.pad(1 + b.rng.below(100));
                b.run(len, COPIES);
                b.pad(1 + b.rng.below(100));
                b.run(len, ONE_DESCENT, 1);
                b.pad(1 + b.rng.below(100));
                b.run(len, ONE_DESCENT, len - 1);
            }
            // across a 64-key word of the descent mask that is no span border, the run's only descent exactly on it
            uint32_t k = 0;
            for (uint64_t len : classes) {
                if (len < 2) continue;
                const uint64_t before = len / 2;
                b.across(b.next_multiple(span, before) + 64 * (1 + k++ % (span / 64 - 1)), len, ONE_DESCENT, before);
                b.across(b.next_multiple(span, before) + 64 * (1 + k++ % (span / 64 - 1)), len, RANDOM, before);
            }
            // across a span of k_find_descents (the first left neighbour of a wave comes from memory)
            for (uint64_t len : classes) {
                if (len < 2) continue;
                const uint64_t before = len / 2;
                b.across(b.next_multiple(span, before), len, ONE_DESCENT, before);
                b.across(b.next_multiple(span, before), len, RANDOM, before);
            }
            // across the share of one k_repair_runs workgroup: a short, a medium, a long run and one walked through memory
            uint64_t border = b.next_multiple(share, RL_CAP);
            b.across(border, RR_SHORT, ONE_DESCENT, RR_SHORT / 2);
            border += share;
            b.across(border, OR_CAP + 1, ONE_DESCENT, (OR_CAP + 1) / 2);
            border += share;
            b.across(border, 65, ONE_DESCENT, 32);
            border += share;
            b.across(border, RL_CAP + 1, RANDOM, RL_CAP / 2);
            b.pad(1 + b.rng.below(100));
            b.run(RL_CAP + 1, SPARSE_HIGH);
            b.pad(1 + b.rng.below(100));
            b.run(2 * RL_CAP, SPARSE_HIGH);
            b.pad(1 + b.rng.below(100));
            b.run(64, RANDOM);  // the very end of the buffer
        });
        add("no descent at all", false, -1, [=](RunBuilder &b) {
            for (int rep = 0; rep < 3; rep++)
                for (uint64_t len : classes) {
                    b.run(len, ORDERED);
                    b.run(len, COPIES);
                    for (uint64_t s = b.rng.below(70); s > 0; s--) b.run(1, RANDOM);
                }
        });
        for (uint64_t len : classes)  // the whole buffer one run: its start and its end at once
            add(("one run of " + std::to_string(len)).c_str(), false, -1, [=](RunBuilder &b) { b.run(len, RANDOM); });
        add("short run at the end", false, -1, [=](RunBuilder &b) {
            b.run(RR_SHORT, RANDOM);
            b.pad(700);
            b.run(2, ONE_DESCENT, 1);
        });
        // OR_MAX keys: still ordered by one lane through memory, across a workgroup's share
        add("a run of OR_MAX", false, rotation++, [=](RunBuilder &b) {
            b.pad_to(share > OR_MAX / 2 + 1000 ? share - OR_MAX / 2 : 1000);
            b.run(OR_MAX, RANDOM);
            b.pad(300);
            b.run(RL_CAP, RANDOM);
        });
        add("a run of OR_MAX + 1", true, rotation++, [=](RunBuilder &b) {
            b.pad(500);
            b.run(OR_MAX + 1, RANDOM);
            b.pad(200);
            b.run(65, RANDOM);
        });
    }
    uint64_t cap = 8 * share;
    SortBufs<uint64_t> b(g, cap);
    uint32_t *d_counts = g.alloc<uint32_t>(cap / span + 2);
    std::vector<uint32_t> got_counts;
    run_batched<FinishCase>(cases, prepare_finish_case, [&](FinishCase &c) {
        const uint64_t n = c.in.size();
        // tiles of one span of k_find_descents (512 keys) and of four (2048)
        std::vector<HeadVariant> variants = {{0, 0}, {1, span}, {1, 4 * span}};
        if (c.low != 1) variants.push_back({c.low, span}), variants.push_back({c.low, 4 * span});
        if (c.heads_rotation >= 0) variants = {variants[c.heads_rotation % variants.size()]};
        for (int kv = 0; kv < 2; kv++)
            for (const HeadVariant &hv : variants) {
                char nm[256];
                std::snprintf(nm, sizeof(nm), "finish %s low=%u hi=%u n=%llu %s heads(shift=%u,tile=%llu)", c.label.c_str(), c.low, c.hi,
                              (unsigned long long)n, kv ? "keys+payload" : "keys", hv.shift, (unsigned long long)hv.tile);
                const std::string name = nm;
                b.load(c.in, kv != 0);
                bool in_tmp = false, fell_back = false;
                uint32_t *v = kv ? b.d_vals : nullptr, *vt = kv ? b.d_vtmp : nullptr;
                GOK(g, cr_radix_sort_u64(g.ctx, b.d_keys, b.d_tmp, v, vt, n, c.low, c.hi, &in_tmp));
                uint64_t *keys = in_tmp ? b.d_tmp : b.d_keys;
                uint32_t *vals = kv ? (in_tmp ? b.d_vtmp : b.d_vals) : nullptr;
                CrRunHeads heads{hv.shift, hv.tile, d_counts, false};
                const uint64_t n_tiles = hv.tile ? (n + hv.tile - 1) / hv.tile : 0;
                if (hv.tile) g.fill(d_counts, 0xEE, (n_tiles + 1) * sizeof(uint32_t));
                GOK(g, cr_order_runs(g.ctx, keys, vals, n, c.low, &fell_back, hv.tile ? &heads : nullptr));
                if (fell_back != c.expect_fell_back) die("%s: fell_back is %d, expected %d", nm, (int)fell_back, (int)c.expect_fell_back);
                b.fetch(name, n, kv != 0, in_tmp);
                if (fell_back) {
                    // a run too long for the repair: the buffer still holds every (key, payload) pair, the heads are void, and the
                    // sort on all bits puts it right
                    if (hv.tile && heads.valid) die("%s: the head counts are marked valid although the repair fell back", nm);
                    std::vector<std::pair<uint64_t, uint32_t>> have(n), want(n);
                    for (uint64_t i = 0; i < n; i++) have[i] = {b.gk[i], kv ? b.gv[i] : 0u}, want[i] = {c.in[i], kv ? (uint32_t)i : 0u};
                    std::sort(have.begin(), have.end());
                    std::sort(want.begin(), want.end());
                    for (uint64_t i = 0; i < n; i++)
                        if (have[i] != want[i])
                            die("%s: after the fall-back the buffer is not the input's multiset: sorted pair %llu: got (0x%llx, %u) expected (0x%llx, %u)",
                                nm, (unsigned long long)i, (unsigned long long)have[i].first, have[i].second,
                                (unsigned long long)want[i].first, want[i].second);
                    // (guards: the buffers are used as they are, the result buffer is the first one now)
                    bool flip = false;
                    GOK(g, cr_radix_sort_u64_full(g.ctx, keys, in_tmp ? b.d_keys : b.d_tmp, vals, kv ? (in_tmp ? b.d_vals : b.d_vtmp) : nullptr, n,
                                                  c.hi, &flip));
                    b.fetch(name, n, kv != 0, in_tmp != flip);
                }
                for (uint64_t i = 0; i < n; i++) {
                    const uint64_t want = c.in[c.order[i]];
                    if (b.gk[i] != want)
                        die("%s: key at index %llu: got 0x%llx expected 0x%llx", nm, (unsigned long long)i, (unsigned long long)b.gk[i],
                            (unsigned long long)want);
                }
                if (kv) {
                    // equal whole keys: the same SET of payloads as the stable sort gives (the in-place bucket permutation of
                    // or_flag_permute promises no order among them) ...
                    std::vector<uint32_t> tmp;
                    for (uint64_t a = 0; a < n;) {
                        uint64_t e = a + 1;
                        while (e < n && b.gk[e] == b.gk[a]) e++;
                        tmp.assign(b.gv.begin() + a, b.gv.begin() + e);
                        std::sort(tmp.begin(), tmp.end());
                        for (uint64_t i = a; i < e; i++)
                            if (tmp[i - a] != c.order[i])
                                die("%s: payloads of the equal keys at [%llu, %llu): sorted, number %llu: got %u expected %u", nm,
                                    (unsigned long long)a, (unsigned long long)e, (unsigned long long)(i - a), tmp[i - a], c.order[i]);
                        a = e;
                    }
                    // ... but a run without a descent is not rewritten at all
                    if (!fell_back)
                        for (size_t r = 0; r + 1 < c.run_start.size(); r++) {
                            if (c.run_unordered[r]) continue;
                            for (uint32_t i = c.run_start[r]; i < c.run_start[r + 1]; i++)
                                if (b.gv[i] != c.post_val[i])
                                    die("%s: payload at index %u of a run that was in order: got %u expected %u", nm, i, b.gv[i], c.post_val[i]);
                        }
                }
                if (hv.tile && !fell_back) {
                    // shift <= low and the tile is a multiple of a span: nothing but a failed allocation keeps the counts away
                    // (fewer than two keys: there is nothing to finish and the caller counts the heads itself)
                    if (n < 2 && !heads.valid) {
                        passed(name);
                        continue;
                    }
                    if (!heads.valid) die("%s: the head counts did not come back valid", nm);
                    got_counts.resize(n_tiles + 1);
                    g.down(got_counts.data(), d_counts, (n_tiles + 1) * sizeof(uint32_t));
                    if (got_counts[n_tiles] != 0xEEEEEEEEu) die("%s: the word behind the %llu tile counts was overwritten", nm, (unsigned long long)n_tiles);
                    for (uint64_t tl = 0; tl < n_tiles; tl++) {
                        uint32_t want = 0;
                        for (uint64_t i = tl * hv.tile; i < std::min(n, (tl + 1) * hv.tile); i++)
                            want += i == 0 || (c.in[c.order[i]] >> hv.shift) != (c.in[c.order[i - 1]] >> hv.shift);
                        if (got_counts[tl] != want)
                            die("%s: run heads of tile %llu: got %u expected %u", nm, (unsigned long long)tl, got_counts[tl], want);
                    }
                }
                passed(name);
            }
    }, 16);
    crgpu_free(g.ctx, d_counts);
}

// ---- the partition by owner -----------------------------------------------------------------------------------------------------
static const uint32_t PART_N_CANON = 1000, PART_BC_LEN = 6, PART_SH_BC = 40;

static void set_whitelist(Gpu &g) {
    std::string seqs;
    for (uint32_t i = 0; i < PART_N_CANON; i++)
        for (int j = PART_BC_LEN - 1; j >= 0; j--) seqs.push_back("ACGT"[(i >> (2 * j)) & 3u]);
    GOK(g, crgpu_set_whitelist(g.ctx, 0, seqs.data(), PART_N_CANON, PART_BC_LEN, seqs.data(), PART_N_CANON, nullptr));
}

struct PartCase {
    uint64_t n = 0, seed = 0;
    uint32_t n_ranks = 0;
    bool explicit_bounds = false, kv = false;
    std::vector<uint32_t> bounds;  // n_ranks + 1 (explicit or the equal widths)
    std::vector<uint64_t> in;
    std::vector<uint32_t> order;
    std::vector<uint64_t> counts;
    void release() {
        std::vector<uint64_t>().swap(in);
        std::vector<uint32_t>().swap(order);
    }
};

static uint32_t owner_of(const std::vector<uint32_t> &bounds, uint32_t bc) {  // the first r with bounds[r + 1] > bc
    return (uint32_t)(std::upper_bound(bounds.begin() + 1, bounds.end(), bc) - (bounds.begin() + 1));
}

static void prepare_part_case(PartCase &c) {
    Rng rng(c.seed);
    const uint32_t R = c.n_ranks;
    c.bounds.assign(R + 1, 0);
    if (c.explicit_bounds) {
        // ascending, empty ranges among them, the last bound beyond the list
        for (uint32_t r = 1; r < R; r++) c.bounds[r] = (uint32_t)rng.below(PART_N_CANON + 1);
        std::sort(c.bounds.begin() + 1, c.bounds.begin() + R);
        for (uint32_t r = 2; r < R; r += 5) c.bounds[r] = c.bounds[r - 1];
        c.bounds[R] = PART_N_CANON + 17;
    } else {
        const uint32_t width = (PART_N_CANON + R - 1) / R;
        for (uint32_t r = 0; r <= R; r++) c.bounds[r] = r * width;
    }
    // half of the keys sit exactly on a bound or one below it
    std::vector<uint32_t> edge;
    for (uint32_t r = 0; r <= R; r++)
        for (int d = 0; d < 2; d++)
            if (c.bounds[r] >= (uint32_t)d && c.bounds[r] - d < PART_N_CANON) edge.push_back(c.bounds[r] - d);
    edge.push_back(PART_N_CANON - 1);
    c.in.resize(c.n);
    for (auto &k : c.in) {
        const uint32_t bc = rng.below(2) ? edge[rng.below(edge.size())] : (uint32_t)rng.below(PART_N_CANON);
        k = ((uint64_t)bc << PART_SH_BC) | (rng.next() & bitmask(PART_SH_BC));
    }
    c.order.resize(c.n);
    std::iota(c.order.begin(), c.order.end(), 0u);
    std::vector<uint32_t> own(c.n);
    c.counts.assign(R, 0);
    for (uint64_t i = 0; i < c.n; i++) {
        own[i] = owner_of(c.bounds, (uint32_t)(c.in[i] >> PART_SH_BC));
        if (own[i] >= R) die("test bug: owner %u of %u ranks", own[i], R);
        c.counts[own[i]]++;
    }
    const uint32_t *o = own.data();
    std::stable_sort(c.order.begin(), c.order.end(), [=](uint32_t a, uint32_t b) { return o[a] < o[b]; });
}

static void group_partition(Gpu &g) {
    set_whitelist(g);
    static const uint32_t ranks[] = {1, 2, 3, 255, 256};
    std::vector<PartCase> cases;
    uint64_t cap = 0;
    for (int kv = 0; kv < 2; kv++) {
        std::vector<uint64_t> ns = ladder(kv ? C("CHUNK_KV64") : C("CHUNK"));
        ns.pop_back();  // up to 4 chunks + 1
        for (uint64_t n : ns)
            for (uint32_t R : ranks)
                for (int eb = 0; eb < 2; eb++) {
                    PartCase c;
                    c.n = n, c.n_ranks = R, c.explicit_bounds = eb != 0, c.kv = kv != 0, c.seed = SEED_PART + cases.size();
                    cap = std::max(cap, n);
                    cases.push_back(c);
                }
    }
    uint64_t *d_in = g.alloc<uint64_t>(cap + GUARD), *d_out = g.alloc<uint64_t>(cap + GUARD);
    uint32_t *d_vin = g.alloc<uint32_t>(cap + GUARD), *d_vout = g.alloc<uint32_t>(cap + GUARD);
    std::vector<uint64_t> gk;
    std::vector<uint32_t> hv, gv;
    run_batched<PartCase>(cases, prepare_part_case, [&](PartCase &c) {
        char nm[200];
        std::snprintf(nm, sizeof(nm), "cr_partition_by_owner%s n=%llu n_ranks=%u %s", c.kv ? "_kv" : "", (unsigned long long)c.n, c.n_ranks,
                      c.explicit_bounds ? "explicit bounds" : "equal widths");
        const uint64_t n = c.n;
        g.up(d_in, c.in.data(), n * sizeof(uint64_t));
        g.fill(d_out, GUARD_BYTE, (n + GUARD) * sizeof(uint64_t));
        if (c.kv) {
            hv.resize(n);
            std::iota(hv.begin(), hv.end(), 0u);
            g.up(d_vin, hv.data(), n * sizeof(uint32_t));
            g.fill(d_vout, GUARD_BYTE, (n + GUARD) * sizeof(uint32_t));
        }
        std::vector<uint64_t> counts(c.n_ranks, ~0ull);
        const uint32_t *bounds = c.explicit_bounds ? c.bounds.data() : nullptr;
        if (c.kv)
            GOK(g, cr_partition_by_owner_kv(g.ctx, d_in, d_out, d_vin, d_vout, n, PART_SH_BC, c.n_ranks, bounds, counts.data()));
        else
            GOK(g, cr_partition_by_owner(g.ctx, d_in, d_out, n, PART_SH_BC, c.n_ranks, bounds, counts.data()));
        for (uint32_t r = 0; r < c.n_ranks; r++)
            if (counts[r] != c.counts[r])
                die("%s: counts_out[%u]: got %llu expected %llu", nm, r, (unsigned long long)counts[r], (unsigned long long)c.counts[r]);
        gk.resize(n + GUARD);
        g.down(gk.data(), d_out, gk.size() * sizeof(uint64_t));
        SortBufs<uint64_t>::check_guard(nm, "keys", gk.data() + n);
        for (uint64_t i = 0; i < n; i++)
            if (gk[i] != c.in[c.order[i]])
                die("%s: key at index %llu: got 0x%llx expected 0x%llx", nm, (unsigned long long)i, (unsigned long long)gk[i],
                    (unsigned long long)c.in[c.order[i]]);
        if (c.kv) {
            gv.resize(n + GUARD);
            g.down(gv.data(), d_vout, gv.size() * sizeof(uint32_t));
            SortBufs<uint32_t>::check_guard(nm, "payload", gv.data() + n);
            for (uint64_t i = 0; i < n; i++)
                if (gv[i] != c.order[i]) die("%s: payload at index %llu: got %u expected %u (stable order)", nm, (unsigned long long)i, gv[i], c.order[i]);
        }
        passed(nm);
    });
    // refused inputs: the error code, and nothing written
    {
        const uint64_t n = 1000;
        Rng rng(SEED_PART ^ 0xbadull);
        std::vector<uint64_t> in(n);
        for (auto &k : in) k = (rng.below(PART_N_CANON) << PART_SH_BC) | (rng.next() & bitmask(PART_SH_BC));
        g.up(d_in, in.data(), n * sizeof(uint64_t));
        struct Refusal {
            const char *what;
            uint32_t n_ranks;
            std::vector<uint32_t> bounds;
            bool with_bounds;
        };
        const std::vector<Refusal> refusals = {
            {"n_ranks 0", 0, {}, false},
            {"n_ranks 257", 257, {}, false},
            {"bounds that do not start at 0", 3, {1, 300, 600, PART_N_CANON}, true},
            {"descending bounds", 3, {0, 600, 300, PART_N_CANON}, true},
            {"a last bound inside the list", 3, {0, 300, 600, PART_N_CANON - 1}, true},
        };
        for (const Refusal &r : refusals)
            for (int kv = 0; kv < 2; kv++) {
                g.fill(d_out, GUARD_BYTE, n * sizeof(uint64_t));
                g.fill(d_vout, GUARD_BYTE, n * sizeof(uint32_t));
                std::vector<uint64_t> counts(300, 0);
                const uint32_t *bounds = r.with_bounds ? r.bounds.data() : nullptr;
                const int rc = kv ? cr_partition_by_owner_kv(g.ctx, d_in, d_out, d_vin, d_vout, n, PART_SH_BC, r.n_ranks, bounds, counts.data())
                                  : cr_partition_by_owner(g.ctx, d_in, d_out, n, PART_SH_BC, r.n_ranks, bounds, counts.data());
                if (rc != CRGPU_EINVAL) die("partition with %s: returned %d, expected CRGPU_EINVAL (%d)", r.what, rc, CRGPU_EINVAL);
                gk.resize(n);
                gv.resize(n);
                g.down(gk.data(), d_out, n * sizeof(uint64_t));
                g.down(gv.data(), d_vout, n * sizeof(uint32_t));
                for (uint64_t i = 0; i < n; i++)
                    if (gk[i] != guard_value<uint64_t>() || gv[i] != guard_value<uint32_t>())
                        die("partition with %s: the output was written at index %llu: got 0x%llx expected 0x%llx", r.what, (unsigned long long)i,
                            (unsigned long long)gk[i], (unsigned long long)guard_value<uint64_t>());
                passed(std::string("partition refuses ") + r.what + (kv ? " (kv)" : ""));
            }
    }
    crgpu_free(g.ctx, d_in);
    crgpu_free(g.ctx, d_out);
    crgpu_free(g.ctx, d_vin);
    crgpu_free(g.ctx, d_vout);
}

// ---- the small scan -------------------------------------------------------------------------------------------------------------
static void group_scan(Gpu &g) {
    static const uint64_t ns[] = {0, 1, 1023, 1024, 1025, 4096, 5000};
    uint32_t *d = g.alloc<uint32_t>(5000 + GUARD), *d_total = g.alloc<uint32_t>(2);
    Rng rng(SEED_SCAN);
    for (uint64_t n : ns)
        for (int with_total = 0; with_total < 2; with_total++) {
            char nm[100];
            std::snprintf(nm, sizeof(nm), "cr_scan_small n=%llu %s total_out", (unsigned long long)n, with_total ? "with" : "without");
            std::vector<uint32_t> h(n + GUARD, guard_value<uint32_t>()), got(n + GUARD);
            for (uint64_t i = 0; i < n; i++) h[i] = (uint32_t)rng.below(800000);  // 5000 of them stay below 2^32
            g.up(d, h.data(), h.size() * sizeof(uint32_t));
            g.fill(d_total, GUARD_BYTE, 2 * sizeof(uint32_t));
            GOK(g, cr_scan_small(g.ctx, d, n, with_total ? d_total : nullptr));
            g.down(got.data(), d, got.size() * sizeof(uint32_t));
            uint32_t tot[2];
            g.down(tot, d_total, sizeof(tot));
            uint64_t acc = 0;
            for (uint64_t i = 0; i < n; i++) {
                if (got[i] != (uint32_t)acc) die("%s: prefix at index %llu: got %u expected %llu", nm, (unsigned long long)i, got[i], (unsigned long long)acc);
                acc += h[i];
            }
            SortBufs<uint32_t>::check_guard(nm, "data", got.data() + n);
            const uint32_t want_total = with_total ? (uint32_t)acc : guard_value<uint32_t>();
            if (tot[0] != want_total) die("%s: total: got %u expected %u", nm, tot[0], want_total);
            if (tot[1] != guard_value<uint32_t>()) die("%s: the word behind the total was overwritten: got %u", nm, tot[1]);
            passed(nm);
        }
    crgpu_free(g.ctx, d);
    crgpu_free(g.ctx, d_total);
}

// ---- more keys than SORT_MAX_BLOCKS tiles of four chunks ----------------------------------------------------------------------
static void group_large(Gpu &g) {
    const uint64_t chunk = C("CHUNK");
    // the block count is capped, a tile becomes five chunks, k_scan_digits runs SORT_MAX_BLOCKS / 256 rounds
    const uint64_t n = C("SORT_MAX_BLOCKS") * 4 * chunk + 3 * chunk + 5;
    const uint32_t lo = 4, hi = 12;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> keys(n), vals(n);
    parallel_for(64, [&](size_t part) {
        Rng rng(SEED_LARGE + part);
        for (uint64_t i = n * part / 64; i < n * (part + 1) / 64; i++) keys[i] = (uint32_t)rng.next(), vals[i] = (uint32_t)i;
    });
    uint32_t *d_k = g.alloc<uint32_t>(n), *d_t = g.alloc<uint32_t>(n), *d_v = g.alloc<uint32_t>(n), *d_vt = g.alloc<uint32_t>(n);
    g.up(d_k, keys.data(), n * 4);
    g.up(d_v, vals.data(), n * 4);
    bool in_tmp = false;
    GOK(g, cr_radix_sort_u32(g.ctx, d_k, d_t, d_v, d_vt, n, lo, hi, &in_tmp));
    std::vector<uint32_t> gk(n);
    g.down(gk.data(), in_tmp ? d_t : d_k, n * 4);
    g.down(vals.data(), in_tmp ? d_vt : d_v, n * 4);  // (the payload given was the index)
    // host counting sort, checked in one pass over the input: key i belongs at the next free place of its digit
    std::vector<uint64_t> cursor(257, 0);
    for (uint64_t i = 0; i < n; i++) cursor[((keys[i] >> lo) & 0xFFu) + 1]++;
    for (int d = 0; d < 256; d++) cursor[d + 1] += cursor[d];
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t p = cursor[(keys[i] >> lo) & 0xFFu]++;
        if (gk[p] != keys[i]) die("large n=%llu bits=[%u,%u): key at index %llu: got 0x%x expected 0x%x", (unsigned long long)n, lo, hi, (unsigned long long)p, gk[p], keys[i]);
        if (vals[p] != (uint32_t)i) die("large n=%llu bits=[%u,%u): payload at index %llu: got %u expected %llu", (unsigned long long)n, lo, hi, (unsigned long long)p, vals[p], (unsigned long long)i);
    }
    crgpu_free(g.ctx, d_k);
    crgpu_free(g.ctx, d_t);
    crgpu_free(g.ctx, d_v);
    crgpu_free(g.ctx, d_vt);
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    char nm[160];
    std::snprintf(nm, sizeof(nm), "cr_radix_sort_u32 keys+payload n=%llu bits=[%u,%u) uniform (%.2f s with the host reference)", (unsigned long long)n, lo, hi, s);
    passed(nm);
}

// ---- the digit plans (host only) ------------------------------------------------------------------------------------------------
static uint32_t passes_for(uint32_t t) { return std::min((t + 7) / 8, (t + 8) / 9); }

static void host_plans() {
    uint64_t plans = 0;
    for (uint32_t lo = 0; lo < 64; lo++)
        for (uint32_t hi = lo + 1; hi <= 64; hi++) {
            SweepPlan plan;
            uint32_t widths[OS_MAX_PASSES];
            std::memset(&plan, 0xFF, sizeof(plan));
            if (!cr_sweep_plan(lo, hi, &plan, widths)) die("cr_sweep_plan(%u, %u) found no plan", lo, hi);
            const uint32_t t = hi - lo;
            if (plan.n_passes != passes_for(t)) die("cr_sweep_plan(%u, %u): %u passes, expected %u", lo, hi, plan.n_passes, passes_for(t));
            uint32_t sh = lo, end = lo;
            bool seen9 = false;
            for (uint32_t p = 0; p < plan.n_passes; p++) {
                if (widths[p] != 8 && widths[p] != 9) die("cr_sweep_plan(%u, %u): pass %u is %u bits wide", lo, hi, p, widths[p]);
                if (seen9 && widths[p] == 8) die("cr_sweep_plan(%u, %u): an 8-bit pass (%u) above a 9-bit one", lo, hi, p);
                seen9 = seen9 || widths[p] == 9;
                if (plan.shift[p] != sh) die("cr_sweep_plan(%u, %u): pass %u starts at bit %u, expected %u", lo, hi, p, plan.shift[p], sh);
                uint32_t b = 0;
                while (b < 32 && ((plan.mask[p] >> b) & 1u)) b++;
                if (b == 0 || b > widths[p] || plan.mask[p] != (uint32_t)bitmask(b)) die("cr_sweep_plan(%u, %u): pass %u has the mask 0x%x", lo, hi, p, plan.mask[p]);
                end = plan.shift[p] + b;
                if (p + 1 < plan.n_passes && b != widths[p]) die("cr_sweep_plan(%u, %u): pass %u masks %u of its %u bits", lo, hi, p, b, widths[p]);
                sh += widths[p];
            }
            if (end != hi) die("cr_sweep_plan(%u, %u): the digits end at bit %u", lo, hi, end);
            plans++;
        }
    std::printf("ok cr_sweep_plan: %llu plans\n", (unsigned long long)plans);
    SweepPlan plan;
    uint32_t widths[OS_MAX_PASSES];
    if (cr_sweep_plan(5, 5, &plan, widths) || cr_sweep_plan(9, 3, &plan, widths)) die("cr_sweep_plan accepts an empty bit range");

    const uint32_t max_low = (uint32_t)C("OR_MAX_LOW_BITS");
    uint64_t checked = 0;
    for (uint32_t total = 1; total <= 64; total++)
        for (uint32_t umi = 0; umi <= 40; umi++) {
            const uint32_t low = cr_sort_low_bits(total, umi);
            if (low > max_low) die("cr_sort_low_bits(%u, %u) = %u, more than %u", total, umi, low, max_low);
            if (total <= 27 && low) die("cr_sort_low_bits(%u, %u) = %u, expected 0 up to 27 bits", total, umi, low);
            if (low) {
                if (low >= total) die("cr_sort_low_bits(%u, %u) = %u leaves no bit to the passes", total, umi, low);
                if (umi < 14 + (low - 1)) die("cr_sort_low_bits(%u, %u) = %u leaves fewer than 14 UMI bits above the cut", total, umi, low);
                if (passes_for(total - low) >= passes_for(total)) die("cr_sort_low_bits(%u, %u) = %u saves no pass", total, umi, low);
            }
            checked++;
        }
    static const uint32_t documented[][3] = {{61, 24, 7}, {64, 24, 10}, {50, 24, 5}, {47, 24, 11}};
    for (auto &d : documented)
        if (cr_sort_low_bits(d[0], d[1]) != d[2]) die("cr_sort_low_bits(%u, %u) = %u, documented %u", d[0], d[1], cr_sort_low_bits(d[0], d[1]), d[2]);
    std::printf("ok cr_sort_low_bits: %llu cases\n", (unsigned long long)checked);
}

int main(int argc, char **argv) {
    bool host_only = false;
    std::string group;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "--host-only") {
            host_only = true;
        } else if (a == "--group" && i + 1 < argc) {
            group = argv[++i];
        } else if (a == "--const" && i + 1 < argc) {
            const std::string kv = argv[++i];
            const size_t eq = kv.find('=');
            if (eq == std::string::npos) die("--const %s: expected NAME=VALUE", kv.c_str());
            g_const[kv.substr(0, eq)] = std::strtoull(kv.c_str() + eq + 1, nullptr, 0);
        } else {
            die("usage: test_sort [--host-only | --group u32|u64|finish|partition|scan|large] --const NAME=VALUE ...");
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    if (host_only || group.empty()) host_plans();
    if (!host_only) {
        static const struct {
            const char *name;
            void (*fn)(Gpu &);
        } groups[] = {{"u32", group_u32}, {"u64", group_u64}, {"finish", group_finish}, {"partition", group_partition}, {"scan", group_scan}, {"large", group_large}};
        bool found = false;
        for (auto &gr : groups) {
            if (!group.empty() && group != gr.name) continue;
            found = true;
            Gpu g;  // a context of its own per group: the partition sets a whitelist, the others have none
            gr.fn(g);
        }
        if (!found) die("unknown group %s", group.c_str());
    }
    std::printf("%llu device cases in %.2f s\n", (unsigned long long)g_cases, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    std::printf("all tests passed\n");
    return 0;
}
