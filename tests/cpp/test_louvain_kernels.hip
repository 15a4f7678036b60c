// test_louvain_kernels.hip -- the kernels of cellranger_amd/csrc/louvain.hip by direct launch into guarded buffers, at constructed shapes.
// Everything in louvain.hip is an integer, so everything here is compared bit for bit with a HOST ORDER MODEL written with std::map:
// the round (the gather of w_i(C), the maximum of (G, C == own, -C), the singleton rule, the labels, tot, size and the count of moves
// of the buffer it writes), both sums of S, the decision and the latch, the class lists, the union, the structure check, the degrees,
// the dense renumbering, the composition and the aggregation; and the shared k_keys_to_csr of graph_common.h on hand-made keys.
//
// louvain.hip is compiled here inside a namespace: the same text under the same flags (cellranger_amd.build.FLAGS), not the library's
// object code.  The context, the pool, the scan and the radix sort come from libcrgpu.so.
//
//   test_louvain_kernels --host-only              every case without a device: the order model against hand-computed values and against
//                                                 its own invariants (the tot of a round add up to M, S from a dense matrix)
//   test_louvain_kernels --group round|levels|csr
// One line per case, "all tests passed" at the end; the first mismatch or HIP error ends the program with status 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "graph_common.h"
#include "kernel_test.h"

namespace louvain_under_test {
#include "louvain.hip"
}
using namespace louvain_under_test;

static uint64_t g_tie_own = 0, g_tie_other = 0, g_dropped = 0, g_one_label = 0;  // branches the model took

// ---- the order model -----------------------------------------------------------------------------------------------------------------
struct Graph {  // a symmetric CSR, ascending columns, a self-loop once
    uint32_t n = 0;
    std::vector<long long> indptr;
    std::vector<int32_t> indices;
    std::vector<uint32_t> weights, k;
    uint64_t M = 0;
};
static Graph make_graph(uint32_t n, const std::map<std::pair<uint32_t, uint32_t>, uint32_t> &edges) {
    std::vector<std::map<uint32_t, uint32_t>> rows(n);
    for (const auto &e : edges) rows[e.first.first][e.first.second] = e.second, rows[e.first.second][e.first.first] = e.second;
    Graph g;
    g.n = n, g.indptr.assign(n + 1, 0), g.k.assign(n, 0);
    for (uint32_t i = 0; i < n; i++) {
        for (const auto &c : rows[i]) g.indices.push_back((int32_t)c.first), g.weights.push_back(c.second), g.k[i] += c.second;
        g.indptr[i + 1] = (long long)g.indices.size();
        g.M += g.k[i];
    }
    return g;
}
struct Labelled {  // labels with what a round derives from them
    std::vector<int32_t> lab;
    std::vector<uint32_t> tot, size;
    uint64_t inside = 0, squares = 0;
    uint32_t moved = 0;
    long long S(uint64_t M) const { return (long long)inside * (long long)M - (long long)squares; }
};
static Labelled derive(const Graph &g, const std::vector<int32_t> &lab) {
    Labelled o;
    o.lab = lab, o.tot.assign(g.n, 0), o.size.assign(g.n, 0);
    for (uint32_t i = 0; i < g.n; i++) {
        o.tot[lab[i]] += g.k[i], o.size[lab[i]] += 1;
        for (long long e = g.indptr[i]; e < g.indptr[i + 1]; e++)
            if (lab[g.indices[e]] == lab[i]) o.inside += g.weights[e];
    }
    for (uint32_t c = 0; c < g.n; c++) o.squares += (uint64_t)o.tot[c] * o.tot[c];
    return o;
}
static Labelled model_round(const Graph &g, const Labelled &cur) {
    std::vector<int32_t> next(g.n);
    uint32_t moved = 0;
    for (uint32_t i = 0; i < g.n; i++) {
        const int32_t own = cur.lab[i];
        const long long ki = g.k[i], M = (long long)g.M;
        std::map<int32_t, long long> w;
        w[own] = 0;
        for (long long e = g.indptr[i]; e < g.indptr[i + 1]; e++)
            if ((uint32_t)g.indices[e] != i) w[cur.lab[g.indices[e]]] += g.weights[e];
        if (w.size() == 2 && g.indptr[i + 1] - g.indptr[i] >= 3) g_one_label++;  // every neighbour in one community that is not the own
        bool have = false;
        long long bestG = 0;
        int32_t bestC = 0;
        for (const auto &c : w) {  // ascending C: a later candidate wins with a larger G, or with an equal G when it is the own community
            const long long G = c.second * M - ((long long)cur.tot[c.first] - (c.first == own ? ki : 0)) * ki;
            if (!have || G > bestG) {
                have = true, bestG = G, bestC = c.first;
            } else if (G == bestG) {
                if (c.first == own) g_tie_own++, bestC = own;
                else if (bestC == own) g_tie_own++;
                else g_tie_other++;
            }
        }
        int32_t to = own;
        if (bestC != own) {
            if (cur.size[own] == 1u && cur.size[bestC] == 1u && bestC > own) g_dropped++;
            else to = bestC, moved++;
        }
        next[i] = to;
    }
    Labelled o = derive(g, next);
    o.moved = moved;
    return o;
}
// S of a labelling from the dense matrix: the model's invariant
static long long dense_S(const Graph &g, const std::vector<int32_t> &lab) {
    std::vector<uint64_t> A((size_t)g.n * g.n, 0);
    for (uint32_t i = 0; i < g.n; i++)
        for (long long e = g.indptr[i]; e < g.indptr[i + 1]; e++) A[(size_t)i * g.n + g.indices[e]] = g.weights[e];
    long long S = 0;
    std::set<int32_t> ids(lab.begin(), lab.end());
    for (int32_t C : ids) {
        uint64_t in = 0, tot = 0;
        for (uint32_t i = 0; i < g.n; i++)
            for (uint32_t j = 0; j < g.n; j++) {
                if (lab[i] == C) tot += A[(size_t)i * g.n + j];
                if (lab[i] == C && lab[j] == C) in += A[(size_t)i * g.n + j];
            }
        S += (long long)(in * g.M) - (long long)(tot * tot);
    }
    return S;
}

// ---- a round on the device -----------------------------------------------------------------------------------------------------------
struct DevGraph {
    GBuf<long long> ptr;
    GBuf<int32_t> ind;
    GBuf<uint32_t> w, k;
    uint32_t n;
    explicit DevGraph(const Graph &g) : ptr(g.indptr), ind(g.indices), w(g.weights), k(g.k), n(g.n) {}
    LvGraph view() const { return LvGraph{ptr.d, ind.d, w.d, k.d, n}; }
    void guards() const { (void)ptr.get("indptr"), (void)ind.get("indices"), (void)w.get("weights"), (void)k.get("k"); }
};
// One round from `cur` under the thresholds, then the decision; *next_out = the model's next labelling when the round counted
static bool round_case(const char *name, const Graph &g, const std::vector<int32_t> &lab, uint32_t wave_max, uint32_t lds_max, Labelled *next_out = nullptr) {
    const Labelled cur = derive(g, lab), want = model_round(g, cur);
    uint64_t tot_sum = 0, size_sum = 0;
    for (uint32_t c = 0; c < g.n; c++) tot_sum += want.tot[c], size_sum += want.size[c];
    if (tot_sum != g.M || size_sum != g.n) die("%s: the model's tot add up to %llu of %llu", name, (unsigned long long)tot_sum, (unsigned long long)g.M);
    if (g.n <= 300 && (want.S(g.M) != dense_S(g, want.lab) || cur.S(g.M) != dense_S(g, cur.lab))) die("%s: the model's S is not the dense matrix's", name);
    const bool counts = want.moved != 0 && want.S(g.M) > cur.S(g.M);
    if (next_out) *next_out = want;
    std::vector<uint32_t> list1, list2;
    uint32_t in_wave = 0;
    for (uint32_t i = 0; i < g.n; i++) {
        const uint64_t d = (uint64_t)(g.indptr[i + 1] - g.indptr[i]);
        if (d > wave_max && d <= lds_max) list1.push_back(i);
        else if (d > wave_max) list2.push_back(i);
        else in_wave++;
    }
    if (!g_host_only) {
        crgpu_ctx *ctx = g_gpu->ctx;
        DevGraph dg(g);
        GBuf<int32_t> lab0(cur.lab), lab1(g.n);
        GBuf<uint32_t> tot0(cur.tot), tot1(g.n), size0(cur.size), size1(g.n), d_l1(std::max<size_t>(list1.size(), 1)), d_l2(std::max<size_t>(list2.size(), 1)), d_block(4100);
        LvLevel lv = {{lab0.d, lab1.d}, {tot0.d, tot1.d}, {size0.d, size1.d}};
        // the class lists by the library's compaction
        uint32_t n1 = 0, n2 = 0;
        if (lds_max > wave_max) {
            GOK(compact(ctx, LvClassFlag{dg.ptr.d, wave_max, lds_max}, LvEmitNode{d_l1.d}, g.n, d_block.d, d_block.d + 4096));
            GOK(read_u32(ctx, d_block.d + 4096, &n1));
        }
        GOK(compact(ctx, LvClassFlag{dg.ptr.d, std::max(wave_max, lds_max), ~0ull}, LvEmitNode{d_l2.d}, g.n, d_block.d, d_block.d + 4096));
        GOK(read_u32(ctx, d_block.d + 4096, &n2));
        if (n1 != list1.size() || n2 != list2.size()) die("%s: %u and %u nodes in the class lists against %zu and %zu", name, n1, n2, list1.size(), list2.size());
        std::vector<uint32_t> got1 = d_l1.get("list 1"), got2 = d_l2.get("list 2");
        got1.resize(n1), got2.resize(n2);
        same("the workgroup class", got1, list1), same("the device-table class", got2, list2);
        uint64_t max_deg = 0;
        for (uint32_t i : list2) max_deg = std::max<uint64_t>(max_deg, (uint64_t)(g.indptr[i + 1] - g.indptr[i]));
        const uint32_t dev_slots = lv_slots(max_deg, 64u), groups = std::max<uint32_t>(1u, std::min<uint32_t>(n2, 3u));  // fewer tables than nodes: they are reused
        GBuf<int32_t> tk((uint64_t)groups * dev_slots);
        GBuf<uint32_t> tv((uint64_t)groups * dev_slots);
        for (int latched = 0; latched < 2; latched++) {
            LvState st;
            std::memset(&st, 0, sizeof(st));
            st.S = cur.S(g.M), st.M = g.M, st.max_rounds = 2u, st.stopped = latched ? 1u : 0u, st.rounds = 1u;
            st.inside = 77, st.squares = 88, st.moved = 99u;  // what an earlier round left: k_lv_prep zeroes them
            GBuf<LvState> d_st(std::vector<LvState>(1, st));
            const uint32_t node_grid = cr_grid(g.n, LV_WG), wave_grid = cr_grid((uint64_t)g.n * 64u, LV_WG);
            hipLaunchKernelGGL(k_lv_prep, dim3(node_grid), dim3(LV_WG), 0, ctx->stream, lv, g.n, d_st.d);
            hipLaunchKernelGGL(k_lv_round<0>, dim3(wave_grid), dim3(LV_WG), 0, ctx->stream, dg.view(), lv, d_st.d, wave_max, (const uint32_t *)nullptr, 0u,
                               (int32_t *)nullptr, (uint32_t *)nullptr, 0u);
            if (n1)
                hipLaunchKernelGGL(k_lv_round<1>, dim3(cr_grid((uint64_t)n1 * LV_WG, LV_WG)), dim3(LV_WG), 0, ctx->stream, dg.view(), lv, d_st.d, wave_max,
                                   (const uint32_t *)d_l1.d, n1, (int32_t *)nullptr, (uint32_t *)nullptr, 0u);
            if (n2)
                hipLaunchKernelGGL(k_lv_round<2>, dim3(groups), dim3(LV_WG), 0, ctx->stream, dg.view(), lv, d_st.d, wave_max, (const uint32_t *)d_l2.d, n2, tk.d,
                                   tv.d, dev_slots);
            hipLaunchKernelGGL(k_lv_inside, dim3(wave_grid), dim3(LV_WG), 0, ctx->stream, dg.view(), lv, d_st.d, 2u);
            hipLaunchKernelGGL(k_lv_squares, dim3(node_grid), dim3(LV_WG), 0, ctx->stream, lv, g.n, d_st.d, 2u);
            g_gpu->launched("the round");
            LvState mid = d_st.get("the state")[0];
            if (latched) {  // after the latch a round is a no-op: the other buffer keeps its fill, the state its values
                if (std::memcmp(&mid, &st, sizeof(st)) != 0) die("%s: a latched round wrote the state", name);
                const std::vector<int32_t> l1 = lab1.get("labels 1");
                if (l1 != want.lab) die("%s: a latched round wrote the labels", name);
            } else {
                if (mid.moved != want.moved || mid.inside != want.inside || mid.squares != want.squares)
                    die("%s: moved %u inside %llu squares %llu against %u %llu %llu", name, mid.moved, (unsigned long long)mid.inside, (unsigned long long)mid.squares,
                        want.moved, (unsigned long long)want.inside, (unsigned long long)want.squares);
                same("the labels of the round", lab1.get("labels 1"), want.lab);
                same("tot of the round", tot1.get("tot 1"), want.tot), same("size of the round", size1.get("size 1"), want.size);
            }
            hipLaunchKernelGGL(k_lv_decide, dim3(1), dim3(64), 0, ctx->stream, d_st.d);
            g_gpu->launched("k_lv_decide");
            const LvState end = d_st.get("the state")[0];
            if (latched) {
                if (std::memcmp(&end, &st, sizeof(st)) != 0) die("%s: a latched decision wrote the state", name);
            } else {
                const LvState e = {counts ? want.S(g.M) : cur.S(g.M), want.inside, want.squares, g.M, counts ? 1u : 0u, 1u, counts ? 2u : 1u, want.moved, 2u, 0u};  // max_rounds 2: latched either way
                if (std::memcmp(&end, &e, sizeof(e)) != 0)
                    die("%s: the decision: S %lld cur %u stopped %u rounds %u against S %lld cur %u stopped 1 rounds %u", name, end.S, end.cur, end.stopped, end.rounds, e.S,
                        e.cur, e.rounds);
            }
        }
        same("the labels read", lab0.get("labels 0"), cur.lab), same("tot read", tot0.get("tot 0"), cur.tot), same("size read", size0.get("size 0"), cur.size);
        dg.guards(), (void)tk.get("table keys"), (void)tv.get("table weights"), (void)d_block.get("block");
    }
    case_done("round %-28s n %4u, thresholds %4u / %4u: %u rows on a wave, %zu on a workgroup, %zu on a device table; %u move, the round %s", name, g.n, wave_max,
              lds_max, in_wave, list1.size(), list2.size(), want.moved, counts ? "counts" : "is discarded");
    return counts;
}
static Graph random_graph(uint32_t n, uint32_t extra, uint32_t wmax, bool hub, uint64_t seed) {
    Rng r(seed);
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> e;
    for (uint32_t i = 0; i + 1 < n; i++) e[{i, i + 1}] = 1u + r.below(wmax);
    for (uint32_t t = 0; t < extra; t++) {
        const uint32_t a = r.below(n), b = r.below(n);
        e[{std::min(a, b), std::max(a, b)}] = 1u + r.below(wmax);  // a == b: a self-loop
    }
    if (hub)
        for (uint32_t i = 1; i < n; i++) e[{0u, i}] = 1u + r.below(wmax);
    return make_graph(n, e);
}
static std::vector<int32_t> random_labels(uint32_t n, uint32_t groups, uint64_t seed) {
    Rng r(seed);
    std::vector<int32_t> lab(n);
    for (uint32_t i = 0; i < n; i++) lab[i] = (int32_t)r.below(std::min(groups, n));
    return lab;
}
static std::vector<int32_t> identity(uint32_t n) {
    std::vector<int32_t> lab(n);
    for (uint32_t i = 0; i < n; i++) lab[i] = (int32_t)i;
    return lab;
}
static void group_round() {
    {  // hand-computed: two triangles joined by an edge take two rounds to S = 70
        const Graph g = make_graph(6, {{{0, 1}, 1}, {{0, 2}, 1}, {{1, 2}, 1}, {{3, 4}, 1}, {{3, 5}, 1}, {{4, 5}, 1}, {{2, 3}, 1}});
        Labelled a, b;
        if (!round_case("two triangles, round 1", g, identity(6), 127, 2047, &a) || !round_case("two triangles, round 2", g, a.lab, 127, 2047, &b))
            die("two triangles: both rounds count");
        if (b.S(g.M) != 70 || g.M != 14 || b.lab != std::vector<int32_t>({0, 0, 0, 4, 4, 4})) die("two triangles: S %lld", b.S(g.M));
        if (round_case("two triangles, round 3", g, b.lab, 127, 2047)) die("two triangles: a third round counts");
    }
    {  // ties on G.  The path a - i - b: (0, 0, 2) ties the own community with b's and i stays; (0, 1, 2) ties a's with b's and i takes a's
        const Graph g = make_graph(3, {{{0, 1}, 1}, {{1, 2}, 1}});
        const uint64_t own0 = g_tie_own, other0 = g_tie_other;
        Labelled o;
        round_case("a tie of own and another", g, {0, 0, 2}, 127, 2047, &o);
        if (o.lab[1] != 0 || g_tie_own == own0) die("the tie of own and another: node 1 goes to %d", o.lab[1]);
        round_case("a tie of two others", g, {0, 1, 2}, 127, 2047, &o);
        if (o.lab[1] != 0 || g_tie_other == other0) die("the tie of two others: node 1 goes to %d", o.lab[1]);
        const uint64_t dropped0 = g_dropped;
        const Graph pair = make_graph(2, {{{0, 1}, 1}});
        round_case("the singleton rule on one edge", pair, identity(2), 127, 2047, &o);  // 0 would go to 1 (dropped), 1 goes to 0
        if (o.lab != std::vector<int32_t>({0, 0}) || g_dropped != dropped0 + 1) die("one edge: %d %d", o.lab[0], o.lab[1]);
    }
    {  // rows whose neighbours all share one label: a star whose leaves are one community, on every class
        std::map<std::pair<uint32_t, uint32_t>, uint32_t> e;
        for (uint32_t i = 1; i < 40; i++) e[{0u, i}] = i;
        for (uint32_t i = 1; i + 1 < 40; i++) e[{i, i + 1}] = 1;
        const Graph g = make_graph(40, e);
        std::vector<int32_t> lab(40, 7);
        lab[0] = 0;
        const uint64_t before = g_one_label;
        for (uint32_t wave_max : {127u, 38u, 4u}) round_case("neighbours of one label", g, lab, wave_max, wave_max == 4u ? 16u : 2047u);
        if (g_one_label == before) die("no row had its neighbours in one community");
    }
    // a hub row of n - 1 entries beside short rows, identity labels and grouped labels, every class
    for (uint32_t n : {63u, 65u, 257u})
        for (int grouped = 0; grouped < 2; grouped++) {
            const Graph g = random_graph(n, 2 * n, 9, true, 100 + n);
            const std::vector<int32_t> lab = grouped ? random_labels(n, 7, n) : identity(n);
            round_case(grouped ? "hub, 7 groups" : "hub, identity", g, lab, 127, 2047);
            round_case(grouped ? "hub, 7 groups" : "hub, identity", g, lab, 4, 16);
            round_case(grouped ? "hub, 7 groups" : "hub, identity", g, lab, 4, 2);  // no workgroup class: lds_deg_max below wave_deg_max
        }
    {  // weights near 2^28: M = 2^31 - 2, products beyond 2^60
        const Graph g = make_graph(4, {{{0, 1}, (1u << 28) - 1u}, {{1, 2}, 1u << 28}, {{2, 3}, 1u << 28}, {{0, 3}, 1u << 28}});
        if (g.M != (1ull << 31) - 2) die("M = %llu", (unsigned long long)g.M);
        round_case("weights near 2^28", g, identity(4), 127, 2047);
        round_case("weights near 2^28", g, {0, 0, 2, 2}, 127, 2047);
    }
    {  // a row at exactly each class boundary, at the default thresholds and at small ones
        auto boundary = [](uint32_t t1, uint32_t t2, uint32_t groups, uint64_t seed) {
            const uint32_t first = 4, n = first + t2 + 2;
            std::map<std::pair<uint32_t, uint32_t>, uint32_t> e;
            const uint32_t want[4] = {t2, t2 + 1, t1, t1 + 1};  // entries of the nodes 0 .. 3
            Rng r(seed);
            for (uint32_t v = 0; v < 4; v++)
                for (uint32_t j = 0; j < want[v]; j++) e[{v, first + j}] = 1u + r.below(5);
            const Graph g = make_graph(n, e);
            for (uint32_t v = 0; v < 4; v++)
                if ((uint32_t)(g.indptr[v + 1] - g.indptr[v]) != want[v]) die("the boundary graph: node %u has %lld entries", v, g.indptr[v + 1] - g.indptr[v]);
            round_case("class boundaries, identity", g, identity(n), t1, t2);
            round_case("class boundaries, grouped", g, random_labels(n, groups, seed), t1, t2);
        };
        boundary(LV_WAVE_DEG_CAP, LV_WG_DEG_CAP, 50, 7);
        boundary(5, 9, 4, 8);
        boundary(63, 64, 9, 9);  // a row of exactly a wave's width and one more
    }
}

// ---- the levels ----------------------------------------------------------------------------------------------------------------------
static void levels_case(uint32_t n, uint32_t k, uint32_t groups, uint64_t seed) {
    // a directed neighbour matrix: k distinct columns per row, a row may name itself, every row names node 0
    Rng r(seed);
    std::vector<long long> in_ptr(n + 1);
    std::vector<int32_t> in_ind;
    std::set<uint64_t> ukeys;
    for (uint32_t i = 0; i < n; i++) {
        std::set<uint32_t> row = {0u};
        while (row.size() < std::min(k, n)) row.insert(r.below(n));
        in_ptr[i] = (long long)in_ind.size();
        for (uint32_t j : row) in_ind.push_back((int32_t)j), ukeys.insert((uint64_t)i * n + j), ukeys.insert((uint64_t)j * n + i);
    }
    in_ptr[n] = (long long)in_ind.size();
    const uint64_t nnz_in = in_ind.size(), nnz = ukeys.size();
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> e;
    for (uint64_t key : ukeys)
        if (key / n <= key % n) e[{(uint32_t)(key / n), (uint32_t)(key % n)}] = 1u;
    Graph g = make_graph(n, e);
    if (g.indices.size() != nnz) die("the model's union");
    // the aggregation by random labels with unused ids
    std::vector<int32_t> lab = random_labels(n, groups, seed + 1);
    for (auto &c : lab) c = (int32_t)(((uint32_t)c * 3u + 1u) % n);
    const Labelled cur = derive(g, lab);
    std::vector<int32_t> newid(n, -1), dense(n);
    uint32_t n_c = 0;
    for (uint32_t c = 0; c < n; c++)
        if (cur.size[c]) newid[c] = (int32_t)n_c++;
    for (uint32_t i = 0; i < n; i++) dense[i] = newid[lab[i]];
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> agg;
    for (uint32_t i = 0; i < n; i++)
        for (long long q = g.indptr[i]; q < g.indptr[i + 1]; q++) {
            const uint32_t C = (uint32_t)dense[i], D = (uint32_t)dense[g.indices[q]];
            if (C < D) agg[{C, D}] += g.weights[q];
            else if (C == D) agg[{C, C}] += g.weights[q];  // both directions and the diagonal: in_C
        }
    const Graph ag = make_graph(n_c, agg);
    if (ag.M != g.M) die("the model's aggregation changes M: %llu from %llu", (unsigned long long)ag.M, (unsigned long long)g.M);
    for (uint32_t c = 0; c < n; c++)
        if (cur.size[c] && ag.k[newid[c]] != cur.tot[c]) die("the model's k' is not tot");
    const Labelled top = derive(ag, identity(n_c));
    if (top.S(ag.M) != cur.S(g.M)) die("the model's aggregation changes S");
    if (!g_host_only) {
        crgpu_ctx *ctx = g_gpu->ctx;
        const uint64_t n_keys = 2 * nnz_in;
        GBuf<long long> d_inptr(in_ptr), d_ptr(n + 1), d_ptr2(n_c + 1);
        GBuf<int32_t> d_inind(in_ind), d_ind(nnz), d_ind2(ag.indices.size()), d_lab(lab), d_newid(n), d_dense(n), d_comp(lab);
        GBuf<uint64_t> d_keys(n_keys), d_keyt(n_keys), d_ckeys(n_keys);
        GBuf<uint32_t> d_perm(n_keys), d_permt(n_keys), d_block(4100), d_w(nnz), d_k(n), d_w2(ag.indices.size()), d_size(cur.size), d_flag(1);
        uint32_t *d_count = d_block.d + 4096;
        hipLaunchKernelGGL(k_lv_keys, dim3(cr_grid(nnz_in, LV_WG)), dim3(LV_WG), 0, ctx->stream, (const long long *)d_inptr.d, (const int32_t *)d_inind.d, n, nnz_in,
                           d_keys.d);
        g_gpu->launched("k_lv_keys");
        bool in_tmp = false;
        GOK(cr_radix_sort_u64(ctx, d_keys.d, d_keyt.d, nullptr, nullptr, n_keys, 0, std::max(1u, cr_ceil_log2((uint64_t)n * n)), &in_tmp));
        const uint64_t *sorted = in_tmp ? d_keyt.d : d_keys.d;
        GOK(compact(ctx, KeyHeadFlag{sorted}, LvEmitKey{sorted, d_ckeys.d}, n_keys, d_block.d, d_count));
        uint32_t merged = 0;
        GOK(read_u32(ctx, d_count, &merged));
        if (merged != nnz) die("%u merged entries against %llu", merged, (unsigned long long)nnz);
        hipLaunchKernelGGL(k_keys_to_csr<uint32_t>, dim3(cr_grid(std::max<uint64_t>(nnz, n + 1), GRAPH_WG)), dim3(GRAPH_WG), 0, ctx->stream, (const uint64_t *)d_ckeys.d, nnz, n, d_ptr.d,
                           d_ind.d, d_w.d);
        g_gpu->launched("k_keys_to_csr");
        same("the union's indptr", d_ptr.get("indptr"), g.indptr), same("the union's indices", d_ind.get("indices"), g.indices);
        same("the union's weights", d_w.get("weights"), g.weights);
        // the structure check: the union passes; a swapped pair, a zero weight, an unequal twin and a missing twin are flagged
        auto check = [&](const std::vector<int32_t> &ind, const std::vector<uint32_t> &w) {
            GBuf<int32_t> di(ind);
            GBuf<uint32_t> dw(w);
            GOK(crgpu_memset(ctx, d_flag.d, 0, sizeof(uint32_t)));
            hipLaunchKernelGGL(k_lv_check, dim3(cr_grid(nnz, LV_WG)), dim3(LV_WG), 0, ctx->stream, (const long long *)d_ptr.d, (const int32_t *)di.d,
                               (const uint32_t *)dw.d, n, nnz, d_flag.d);
            g_gpu->launched("k_lv_check");
            (void)di.get("indices"), (void)dw.get("weights");
            return d_flag.get("flag")[0];
        };
        if (check(g.indices, g.weights) != 0u) die("the union is refused");
        {
            uint32_t row = 1;  // a row of two entries or more whose first two columns are off the diagonal
            while (g.indptr[row + 1] - g.indptr[row] < 2) row++;
            std::vector<int32_t> swapped = g.indices;
            std::swap(swapped[g.indptr[row]], swapped[g.indptr[row] + 1]);
            if (!(check(swapped, g.weights) & LV_BAD_ORDER)) die("a swapped pair passes");
            std::vector<uint32_t> zero = g.weights, unequal = g.weights;
            zero[g.indptr[row]] = 0u, unequal[g.indptr[row]] = 2u;
            if (!(check(g.indices, zero) & LV_BAD_WEIGHT)) die("a weight of 0 passes");
            if (check(g.indices, unequal) != LV_BAD_TWIN) die("an unequal twin passes");
        }
        // the degrees
        LvState st;
        std::memset(&st, 0, sizeof(st));
        GBuf<LvState> d_st(std::vector<LvState>(1, st));
        hipLaunchKernelGGL(k_lv_degrees, dim3(cr_grid((uint64_t)n * 64u, LV_WG)), dim3(LV_WG), 0, ctx->stream, (const long long *)d_ptr.d, (const uint32_t *)d_w.d, n,
                           d_k.d, d_st.d);
        g_gpu->launched("k_lv_degrees");
        same("k", d_k.get("k"), g.k);
        st = d_st.get("the state")[0];
        uint32_t longest = 0;
        for (uint32_t i = 0; i < n; i++) longest = std::max(longest, (uint32_t)(g.indptr[i + 1] - g.indptr[i]));
        if (st.M != g.M || st.max_deg != longest) die("M %llu, the longest row %u against %llu, %u", (unsigned long long)st.M, st.max_deg, (unsigned long long)g.M, longest);
        // the identity and its S
        {
            GBuf<int32_t> l0(n), l1(n);
            GBuf<uint32_t> t0(n), t1(n), s0(n), s1(n);
            LvLevel lv = {{l0.d, l1.d}, {t0.d, t1.d}, {s0.d, s1.d}};
            const LvGraph gv = {d_ptr.d, d_ind.d, d_w.d, d_k.d, n};
            hipLaunchKernelGGL(k_lv_identity, dim3(cr_grid(n, LV_WG)), dim3(LV_WG), 0, ctx->stream, lv, (const uint32_t *)d_k.d, n);
            hipLaunchKernelGGL(k_lv_inside, dim3(cr_grid((uint64_t)n * 64u, LV_WG)), dim3(LV_WG), 0, ctx->stream, gv, lv, d_st.d, 0u);
            hipLaunchKernelGGL(k_lv_squares, dim3(cr_grid(n, LV_WG)), dim3(LV_WG), 0, ctx->stream, lv, n, d_st.d, 0u);
            hipLaunchKernelGGL(k_lv_begin, dim3(1), dim3(64), 0, ctx->stream, d_st.d, 5u);
            g_gpu->launched("k_lv_begin");
            const Labelled id = derive(g, identity(n));
            same("the identity", l0.get("labels 0"), id.lab), same("its tot", t0.get("tot 0"), id.tot), same("its size", s0.get("size 0"), id.size);
            st = d_st.get("the state")[0];
            const LvState e = {id.S(g.M), id.inside, id.squares, g.M, 0u, 0u, 0u, 0u, 5u, longest};
            if (std::memcmp(&st, &e, sizeof(e)) != 0) {  // once more with the state read between the sums and k_lv_begin
                LvState z;
                std::memset(&z, 0, sizeof(z));
                z.M = g.M, z.max_deg = longest;
                GBuf<LvState> d_again(std::vector<LvState>(1, z));
                hipLaunchKernelGGL(k_lv_inside, dim3(cr_grid((uint64_t)n * 64u, LV_WG)), dim3(LV_WG), 0, ctx->stream, gv, lv, d_again.d, 0u);
                hipLaunchKernelGGL(k_lv_squares, dim3(cr_grid(n, LV_WG)), dim3(LV_WG), 0, ctx->stream, lv, n, d_again.d, 0u);
                const LvState mid = d_again.get("the state")[0];
                die("the state a level begins with: S %lld against %lld (inside %llu squares %llu); once more, read before k_lv_begin: inside %llu squares %llu "
                    "against %llu %llu", st.S, e.S, (unsigned long long)st.inside, (unsigned long long)st.squares, (unsigned long long)mid.inside,
                    (unsigned long long)mid.squares, (unsigned long long)id.inside, (unsigned long long)id.squares);
            }
        }
        // the dense renumbering, the composition
        GOK(compact(ctx, LvUsedFlag{d_size.d}, LvEmitId{d_newid.d}, n, d_block.d, d_count));
        uint32_t got_nc = 0;
        GOK(read_u32(ctx, d_count, &got_nc));
        if (got_nc != n_c) die("%u communities against %u", got_nc, n_c);
        hipLaunchKernelGGL(k_lv_dense, dim3(cr_grid(n, LV_WG)), dim3(LV_WG), 0, ctx->stream, (const int32_t *)d_lab.d, (const int32_t *)d_newid.d, n, d_dense.d);
        g_gpu->launched("k_lv_dense");
        same("the dense labels", d_dense.get("dense"), dense);
        std::vector<int32_t> got_newid = d_newid.get("newid");
        for (uint32_t c = 0; c < n; c++)
            if (cur.size[c] && got_newid[c] != newid[c]) die("newid[%u] = %d against %d", c, got_newid[c], newid[c]);
        GBuf<int32_t> d_first(n);
        hipLaunchKernelGGL(k_lv_compose, dim3(cr_grid(n, LV_WG)), dim3(LV_WG), 0, ctx->stream, d_first.d, (const int32_t *)d_dense.d, n, 1u);
        hipLaunchKernelGGL(k_lv_compose, dim3(cr_grid(n, LV_WG)), dim3(LV_WG), 0, ctx->stream, d_comp.d, (const int32_t *)d_dense.d, n, 0u);  // comp = lab
        g_gpu->launched("k_lv_compose");
        std::vector<int32_t> composed(n);
        for (uint32_t i = 0; i < n; i++) composed[i] = dense[lab[i]];
        same("the first composition", d_first.get("comp"), dense), same("a later composition", d_comp.get("comp"), composed);
        // the aggregation
        const LvGraph gv = {d_ptr.d, d_ind.d, d_w.d, d_k.d, n};
        hipLaunchKernelGGL(k_lv_agg_keys, dim3(cr_grid(nnz, LV_WG)), dim3(LV_WG), 0, ctx->stream, gv, nnz, (const int32_t *)d_dense.d, n_c, d_keys.d, d_perm.d);
        g_gpu->launched("k_lv_agg_keys");
        GOK(cr_radix_sort_u64(ctx, d_keys.d, d_keyt.d, d_perm.d, d_permt.d, nnz, 0, std::max(1u, cr_ceil_log2((uint64_t)n_c * n_c)), &in_tmp));
        const uint64_t *skeys = in_tmp ? d_keyt.d : d_keys.d;
        const uint32_t *sperm = in_tmp ? d_permt.d : d_perm.d;
        GOK(compact(ctx, KeyHeadFlag{skeys}, LvEmitKey{skeys, d_ckeys.d}, nnz, d_block.d, d_count));
        uint32_t runs = 0;
        GOK(read_u32(ctx, d_count, &runs));
        if (runs != ag.indices.size()) die("%u entries of the aggregated graph against %zu", runs, ag.indices.size());
        GOK(crgpu_memset(ctx, d_w2.d, 0, (uint64_t)runs * sizeof(uint32_t)));
        hipLaunchKernelGGL(k_lv_run_sums, dim3(cr_grid((nnz + LV_RUN_CHUNK - 1u) / LV_RUN_CHUNK, LV_WG)), dim3(LV_WG), 0, ctx->stream, skeys, sperm,
                           (const uint32_t *)d_w.d, nnz, (const uint64_t *)d_ckeys.d, (uint64_t)runs, d_w2.d);
        hipLaunchKernelGGL(k_keys_to_csr<uint32_t>, dim3(cr_grid(std::max<uint64_t>(runs, (uint64_t)n_c + 1u), GRAPH_WG)), dim3(GRAPH_WG), 0, ctx->stream, (const uint64_t *)d_ckeys.d,
                           (uint64_t)runs, n_c, d_ptr2.d, d_ind2.d, (uint32_t *)nullptr);
        g_gpu->launched("the aggregation");
        same("the aggregated indptr", d_ptr2.get("indptr"), ag.indptr), same("the aggregated indices", d_ind2.get("indices"), ag.indices);
        same("the aggregated weights", d_w2.get("weights"), ag.weights);
        (void)d_keys.get("keys"), (void)d_keyt.get("keyt"), (void)d_ckeys.get("ckeys"), (void)d_perm.get("perm"), (void)d_permt.get("permt"), (void)d_block.get("block");
        (void)d_inptr.get("indptr"), (void)d_inind.get("indices"), (void)d_lab.get("labels"), (void)d_size.get("size");
    }
    case_done("levels n %4u k %3u: the union of %llu entries, the check, the degrees, the identity, %u communities, the aggregation to %zu entries", n, k,
              (unsigned long long)nnz, n_c, ag.indices.size());
}
static void group_levels() {
    for (uint32_t n : {63u, 64u, 65u, 255u, 257u}) levels_case(n, 3, 9, 3000 + n);
    levels_case(300, 67, 5, 4001);
    levels_case(300, 20, 300, 4002);  // nearly every community a singleton
    levels_case(1100, 40, 2, 4003);   // two communities: runs of hundreds of thousands of keys
}

// ---- the shared keys-to-CSR kernel ---------------------------------------------------------------------------------------------------
// k_keys_to_csr (graph_common.h) through its launch helper on hand-made sorted distinct keys i * n + j, against a host loop that counts
// the entries of every row; with the weights pointer every weight is 1, without it the weights buffer keeps its fill
static void csr_case(const char *name, uint32_t n, const std::vector<uint64_t> &ckeys, const std::vector<long long> *indptr_by_hand) {
    const uint64_t nnz = ckeys.size();
    for (uint64_t e = 0; e < nnz; e++)
        if (ckeys[e] >= (uint64_t)n * n || (e && ckeys[e - 1] >= ckeys[e])) die("%s: the keys are not sorted distinct keys of %u rows", name, n);
    std::vector<long long> indptr(n + 1, 0);
    std::vector<int32_t> indices(nnz);
    for (uint64_t e = 0; e < nnz; e++) indptr[ckeys[e] / n + 1]++, indices[e] = (int32_t)(ckeys[e] % n);
    for (uint32_t r = 0; r < n; r++) indptr[r + 1] += indptr[r];
    if (indptr_by_hand && indptr != *indptr_by_hand) die("%s: the host loop's indptr is not the one written by hand", name);
    if (!g_host_only)
        for (int weighted = 0; weighted < 2; weighted++) {
            GBuf<uint64_t> d_ckeys(ckeys);
            GBuf<long long> d_ptr(n + 1);
            GBuf<int32_t> d_ind(nnz);
            GBuf<uint32_t> d_w(nnz);
            cr_keys_to_csr(g_gpu->ctx, d_ckeys.d, nnz, n, d_ptr.d, d_ind.d, weighted ? d_w.d : nullptr);
            g_gpu->launched("k_keys_to_csr");
            same("indptr", d_ptr.get("indptr"), indptr), same("indices", d_ind.get("indices"), indices);
            same("weights", d_w.get("weights"), std::vector<uint32_t>(nnz, weighted ? 1u : 0xFFFFFFFFu));
            same("the keys read", d_ckeys.get("ckeys"), ckeys);
        }
    case_done("csr %-36s n %3u, %3llu entries, a grid for %llu threads, with and without weights", name, n, (unsigned long long)nnz,
              (unsigned long long)std::max<uint64_t>(nnz, (uint64_t)n + 1u));
}
static void group_csr() {
    {  // rows 0, 2 and 4 empty: at the start, in the middle and at the end; fewer entries than n + 1
        const std::vector<long long> by_hand = {0, 0, 2, 2, 3, 3};
        csr_case("empty rows at both ends and between", 5, {1 * 5 + 0, 1 * 5 + 4, 3 * 5 + 2}, &by_hand);
    }
    {
        const std::vector<long long> by_hand = {0, 2, 4};
        csr_case("every cell", 2, {0, 1, 2, 3}, &by_hand);
    }
    {  // row 7 holds the columns 0 .. 256, every other row one column: more entries than n + 1 and than a workgroup has threads
        const uint32_t n = 300;
        std::vector<uint64_t> keys;
        for (uint32_t i = 0; i < n; i++) {
            if (i == 7u)
                for (uint32_t j = 0; j < 257u; j++) keys.push_back((uint64_t)i * n + j);
            else keys.push_back((uint64_t)i * n + (i * 7u + 3u) % n);
        }
        if (keys.size() != 257u + 299u) die("the long row: %zu keys", keys.size());
        csr_case("one row of 257 entries", n, keys, nullptr);
    }
}

int main(int argc, char **argv) {
    std::string group;
    for (int i = 1; i < argc; i++) {
        if (!std::strcmp(argv[i], "--host-only")) g_host_only = true;
        else if (!std::strcmp(argv[i], "--group") && i + 1 < argc) group = argv[++i];
        else die("usage: test_louvain_kernels --host-only | --group round|levels|csr");
    }
    if (!g_host_only && group != "round" && group != "levels" && group != "csr") die("usage: test_louvain_kernels --host-only | --group round|levels|csr");
    Gpu *gpu = nullptr;
    if (!g_host_only) g_gpu = gpu = new Gpu();
    if (g_host_only || group == "round") group_round();
    if (g_host_only || group == "levels") group_levels();
    if (g_host_only || group == "csr") group_csr();
    std::printf("branches: %llu ties of own and another, %llu ties of two others, %llu dropped proposals, %llu rows with one label around them\n",
                (unsigned long long)g_tie_own, (unsigned long long)g_tie_other, (unsigned long long)g_dropped, (unsigned long long)g_one_label);
    delete gpu;
    std::printf("all tests passed (%d cases)\n", g_cases);
    return 0;
}
