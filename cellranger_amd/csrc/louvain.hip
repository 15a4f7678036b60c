// louvain.hip -- RUN_GRAPH_CLUSTERING's clustering step on the device: Louvain (Blondel et al. 2008) in synchronous rounds whose every
// quantity is an integer, and on the host the exact modularity of any labelling.
//
// The stage (lib/python/cellranger/analysis/graphclust.py) pipes the neighbour matrix into bin/convert and runs bin/louvain; the
// reference carries the source of neither, so what is here is the published algorithm in the round form include/crgpu.h states and
// tests/louvain_numpy.py restates.  No parity with the binary is claimed.  No floating point below the timings.
//
// Launch structure.
//   k_lv_keys / one radix sort / compaction of the run heads / k_keys_to_csr   the union of both directions (symmetrize = 1): the path
//                                                                          of graph_common.h, as tsne.hip and umap.hip take it
//   k_lv_check                                                             symmetrize = 0: ascending columns, weights >= 1, the twin entry
//   k_lv_degrees                                                           a wave per node: k_i, M, the longest row
//   a round = k_lv_prep, k_lv_round<0 | 1 | 2>, k_lv_inside, k_lv_squares, k_lv_decide
//     k_lv_round   gathers w_i(C) over the labels of the neighbours in an integer hash table (atomicCAS on the key, atomicAdd on the
//                  weight), scans the table for the largest (G, C == own, -C), applies the singleton rule and writes the label into the
//                  other label buffer, adding the node to that buffer's tot and size.  Three degree classes: <0> a wave per node, the
//                  table in the wave's share of LDS; <1> a workgroup per node, the table in LDS; <2> a workgroup per node, the table
//                  in device memory.  The sums are integers and the maximum is over a total order: no insertion order reaches a result.
//     k_lv_decide  one thread: S(c') from the two integer sums; the round counts and the buffers swap when S rises, else the level is
//                  latched as stopped and every later launch of the batch returns at once.  The host reads the latch once per batch.
//   between levels: the dense renumbering by a compaction of the used ids, the keys C * n_C + D, one radix sort, the run heads, the run
//   sums by integer atomicAdd, k_keys_to_csr.
#include <algorithm>
#include <chrono>
#include <climits>
#include <unordered_map>
#include <vector>

#include "graph_common.h"

#define LV_WG 256u
#define LV_WAVES (LV_WG / 64u)
#define LV_WAVE_SLOTS 256u     // table of a wave in LDS: a row of LV_WAVE_DEG_CAP entries and the own community fill half of it
#define LV_WAVE_DEG_CAP 127u
#define LV_WG_SLOTS 4096u      // table of a workgroup in LDS (32 KiB): rows up to LV_WG_DEG_CAP entries
#define LV_WG_DEG_CAP 2047u
#define LV_BATCH 8u
#define LV_MAX_ROUNDS 1000u
#define LV_EMPTY (-1)
#define LV_RUN_CHUNK 16u       // sorted entries a thread adds up before it touches memory
#define LV_DEV_TABLES 64u      // workgroups (and device-memory tables) of the third class at the most
#define LV_DEV_SLOTS_MAX (1ull << 26)
#define LV_BAD_ORDER 1u
#define LV_BAD_WEIGHT 2u
#define LV_BAD_TWIN 4u

struct LvState {
    long long S;                         // of the current labels
    unsigned long long inside, squares;  // of the other buffer: sum of A_ij over c_i = c_j, sum of tot^2
    unsigned long long M;                // k_lv_degrees
    uint32_t cur, stopped, rounds, moved, max_rounds, max_deg;
};
struct LvGraph {
    const long long *indptr;
    const int32_t *indices;
    const uint32_t *weights;
    const uint32_t *k;
    uint32_t n;
};
struct LvLevel {  // both buffers of the labels and of what is derived from them
    int32_t *lab[2];
    uint32_t *tot[2], *size[2];
};

__device__ __forceinline__ uint32_t lv_row_of(const long long *indptr, uint32_t n, uint64_t e) {
    return (uint32_t)(cr_upper_bound(indptr, (uint64_t)n + 1u, (long long)e) - 1u);
}
__device__ __forceinline__ uint32_t lv_hash(int32_t c) { return (uint32_t)c * 0x9E3779B1u; }
// the smallest power of two >= 2 (deg + 1), at least `least`
__host__ __device__ __forceinline__ uint32_t lv_slots(uint64_t deg, uint32_t least) {
    uint64_t s = least;
    while (s < 2u * (deg + 1u)) s <<= 1;
    return (uint32_t)s;
}

// ---- the graph -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LV_WG) void k_lv_keys(const long long *__restrict__ indptr, const int32_t *__restrict__ indices, uint32_t n, uint64_t nnz,
                                                   uint64_t *__restrict__ keys) {
    for (uint64_t e = (uint64_t)blockIdx.x * LV_WG + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * LV_WG) {
        const uint64_t i = lv_row_of(indptr, n, e), j = (uint64_t)(uint32_t)indices[e];
        keys[2 * e] = i * n + j, keys[2 * e + 1] = j * n + i;
    }
}
struct LvEmitKey {
    const uint64_t *keys;
    uint64_t *ckeys;
    struct Pre {};
    __device__ __forceinline__ Pre pre(uint64_t) const { return Pre(); }
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t o, Pre) const { ckeys[o] = keys[i]; }
};
// symmetrize = 0 (indices in range, indptr in order: the host's checks): the columns of a row strictly ascending, weights >= 1, the twin
// entry (j, i) present with the same weight.  A row that is out of order may hide its twin from the search; it is refused for the order.
__global__ __launch_bounds__(LV_WG) void k_lv_check(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    const uint32_t *__restrict__ weights, uint32_t n, uint64_t nnz, uint32_t *__restrict__ flag) {
    for (uint64_t e = (uint64_t)blockIdx.x * LV_WG + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * LV_WG) {
        const uint32_t i = lv_row_of(indptr, n, e);
        const int32_t j = indices[e];
        uint32_t bad = 0;
        if (e > (uint64_t)indptr[i] && indices[e - 1] >= j) bad |= LV_BAD_ORDER;
        if (weights[e] == 0u) bad |= LV_BAD_WEIGHT;
        const uint64_t a = (uint64_t)indptr[j], len = (uint64_t)indptr[j + 1] - a;
        const uint64_t at = cr_lower_bound(indices + a, len, (int32_t)i);
        if (at >= len || indices[a + at] != (int32_t)i || weights[a + at] != weights[e]) bad |= LV_BAD_TWIN;
        if (bad) atomicOr(flag, bad);
    }
}
// a wave per node: k[i] = the row's weights (held at 2^32 - 1: M then fails its limit), st->M += it, st->max_deg = the longest row
__global__ __launch_bounds__(LV_WG) void k_lv_degrees(const long long *__restrict__ indptr, const uint32_t *__restrict__ weights, uint32_t n,
                                                      uint32_t *__restrict__ k, LvState *__restrict__ st) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * LV_WG + threadIdx.x) >> 6, waves = ((uint64_t)gridDim.x * LV_WG) >> 6;
    unsigned long long total = 0;
    uint32_t longest = 0;
    for (uint64_t i = wave0; i < n; i += waves) {
        const uint64_t a = (uint64_t)indptr[i], b = (uint64_t)indptr[i + 1];
        unsigned long long s = 0;
        for (uint64_t e = a + lane; e < b; e += 64u) s += weights[e];
        s = wave_sum(s);
        if (lane == 0u) k[i] = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)s;
        total += s;
        longest = (b - a) > longest ? (uint32_t)(b - a) : longest;  // a graph has fewer than 2^32 entries
    }
    if (lane == 0u) {
        if (total) atomicAdd(&st->M, total);
        atomicMax(&st->max_deg, longest);
    }
}
struct LvClassFlag {  // rows of more than lo and at most hi entries
    const long long *indptr;
    uint64_t lo, hi;
    __device__ __forceinline__ bool operator()(uint64_t i) const {
        const uint64_t d = (uint64_t)(indptr[i + 1] - indptr[i]);
        return d > lo && d <= hi;
    }
};
struct LvEmitNode {
    uint32_t *list;
    struct Pre {};
    __device__ __forceinline__ Pre pre(uint64_t) const { return Pre(); }
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t o, Pre) const { list[o] = (uint32_t)i; }
};

// ---- a level -------------------------------------------------------------------------------------------------------------------------
// c_i = i in buffer 0 with its tot and size; the round state of a level.  The first measurement (k_lv_inside, k_lv_squares on buffer 0,
// then k_lv_begin) gives S of the identity.
// No kernel below stores to a word of the state that it has read unless the stored value or the branch around the store depends on
// what was read: the uniform reads of the state are scalar loads, a store is a vector store, and the two paths do not keep the order
// of a load and a LATER store to the same address (a k_lv_begin that also zeroed both sums read `squares` as 0 on the device).  So
// the sums and the count of moves are zeroed by k_lv_prep, which does not read them, and read by k_lv_begin and k_lv_decide, which do
// not write them.
__global__ __launch_bounds__(LV_WG) void k_lv_identity(LvLevel lv, const uint32_t *__restrict__ k, uint32_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * LV_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LV_WG)
        lv.lab[0][i] = (int32_t)i, lv.tot[0][i] = k[i], lv.size[0][i] = 1u;
}
__global__ __launch_bounds__(64) void k_lv_begin(LvState *__restrict__ st, uint32_t max_rounds) {
    if (threadIdx.x) return;
    st->S = (long long)st->inside * (long long)st->M - (long long)st->squares;
    st->cur = st->stopped = st->rounds = 0u;
    st->max_rounds = max_rounds;
}
// tot and size of the buffer the round writes, both sums of S and the count of moves start at 0
__global__ __launch_bounds__(LV_WG) void k_lv_prep(LvLevel lv, uint32_t n, LvState *__restrict__ st) {
    if (st->stopped) return;
    const uint32_t nx = st->cur ^ 1u;
    if (blockIdx.x == 0u && threadIdx.x == 0u) st->inside = st->squares = 0, st->moved = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * LV_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LV_WG) lv.tot[nx][i] = 0u, lv.size[nx][i] = 0u;
}

struct LvBest {
    long long G;
    int32_t C;
    uint32_t own;
};
// the total order of the candidates: the larger G, then the own community, then the smaller id
__device__ __forceinline__ bool lv_better(const LvBest &a, const LvBest &b) {
    return a.G > b.G || (a.G == b.G && (a.own > b.own || (a.own == b.own && a.C < b.C)));
}
__device__ __forceinline__ LvBest lv_wave_best(LvBest v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        LvBest o;
        o.G = (long long)(((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)((unsigned long long)v.G >> 32), d) << 32) |
                          (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(unsigned long long)v.G, d));
        o.C = __shfl_xor(v.C, d);
        o.own = (uint32_t)__shfl_xor((int)v.own, d);
        if (lv_better(o, v)) v = o;
    }
    return v;
}
// MODE 0: the group is a wave, compiler-level ordering is enough (a wave's LDS accesses complete in program order)
template <int MODE>
__device__ __forceinline__ void lv_group_sync() {
    if (MODE == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}
// MODE 2: the table is in device memory and a workgroup's waves share it within one launch: every access is an agent-scope atomic,
// which is served by the L2 the workgroup's CU sits behind, so no wave reads a stale line of its L1.
template <int MODE>
__device__ __forceinline__ void lv_table_store(int32_t *keys, uint32_t *vals, uint32_t s) {
    if (MODE == 2) {
        __hip_atomic_store(&keys[s], LV_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&vals[s], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        keys[s] = LV_EMPTY, vals[s] = 0u;
    }
}
template <int MODE>
__device__ __forceinline__ void lv_table_load(const int32_t *keys, const uint32_t *vals, uint32_t s, int32_t *c, uint32_t *w) {
    if (MODE == 2) {
        *c = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *w = __hip_atomic_load(&vals[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        *c = keys[s], *w = vals[s];
    }
}
// the table holds at most deg + 1 keys in at least 2 (deg + 1) slots: the probe ends
__device__ __forceinline__ void lv_insert(int32_t *keys, uint32_t *vals, uint32_t mask, int32_t c, uint32_t w) {
    uint32_t s = lv_hash(c) & mask;
    for (;;) {
        const int32_t prev = atomicCAS(&keys[s], LV_EMPTY, c);
        if (prev == LV_EMPTY || prev == c) break;
        s = (s + 1u) & mask;
    }
    if (w) atomicAdd(&vals[s], w);
}
// The node's round.  MODE 0: every node with at most wave_deg_max entries, a wave each.  MODE 1, 2: the nodes of `list`, a workgroup
// each; MODE 2's tables are dev_keys / dev_vals, dev_slots per workgroup.
template <int MODE>
__global__ __launch_bounds__(LV_WG) void k_lv_round(LvGraph g, LvLevel lv, LvState *__restrict__ st, uint32_t wave_deg_max,
                                                    const uint32_t *__restrict__ list, uint32_t n_list, int32_t *__restrict__ dev_keys,
                                                    uint32_t *__restrict__ dev_vals, uint32_t dev_slots) {
    constexpr uint32_t SLOTS = MODE == 0 ? LV_WAVE_SLOTS * LV_WAVES : (MODE == 1 ? LV_WG_SLOTS : 1u);
    __shared__ int32_t lds_keys[SLOTS];
    __shared__ uint32_t lds_vals[SLOTS];
    __shared__ long long red_G[LV_WAVES];
    __shared__ int32_t red_C[LV_WAVES];
    __shared__ uint32_t red_own[LV_WAVES];
    if (st->stopped) return;  // uniform: the level is latched
    const uint32_t cur = st->cur, nx = cur ^ 1u, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const long long M = (long long)st->M;
    const int32_t *__restrict__ lab = lv.lab[cur];
    const uint32_t *__restrict__ tot = lv.tot[cur], *__restrict__ size = lv.size[cur];
    const uint32_t tid = MODE == 0 ? lane : threadIdx.x, width = MODE == 0 ? 64u : LV_WG;
    int32_t *keys = MODE == 0 ? lds_keys + wave * LV_WAVE_SLOTS : (MODE == 1 ? lds_keys : dev_keys + (size_t)blockIdx.x * dev_slots);
    uint32_t *vals = MODE == 0 ? lds_vals + wave * LV_WAVE_SLOTS : (MODE == 1 ? lds_vals : dev_vals + (size_t)blockIdx.x * dev_slots);
    const uint64_t first = MODE == 0 ? ((uint64_t)blockIdx.x * LV_WG + threadIdx.x) >> 6 : blockIdx.x;
    const uint64_t stride = MODE == 0 ? ((uint64_t)gridDim.x * LV_WG) >> 6 : gridDim.x, count = MODE == 0 ? g.n : n_list;
    for (uint64_t it = first; it < count; it += stride) {
        const uint32_t i = MODE == 0 ? (uint32_t)it : list[it];
        const uint64_t a = (uint64_t)g.indptr[i], b = (uint64_t)g.indptr[i + 1], deg = b - a;
        if (MODE == 0 && deg > wave_deg_max) continue;  // uniform in the wave
        const uint32_t slots = lv_slots(deg, 64u), mask = slots - 1u;
        const int32_t own = lab[i];
        const long long ki = (long long)g.k[i];
        for (uint32_t s = tid; s < slots; s += width) lv_table_store<MODE>(keys, vals, s);
        lv_group_sync<MODE>();
        if (tid == 0u) lv_insert(keys, vals, mask, own, 0u);
        for (uint64_t e = a + tid; e < b; e += width) {
            const int32_t j = g.indices[e];
            if ((uint32_t)j != i) lv_insert(keys, vals, mask, lab[j], g.weights[e]);
        }
        lv_group_sync<MODE>();
        LvBest best = {LLONG_MIN, INT_MAX, 0u};
        for (uint32_t s = tid; s < slots; s += width) {
            int32_t c;
            uint32_t w;
            lv_table_load<MODE>(keys, vals, s, &c, &w);
            if (c == LV_EMPTY) continue;
            LvBest cand;
            cand.C = c, cand.own = c == own ? 1u : 0u;
            cand.G = (long long)w * M - ((long long)tot[c] - (cand.own ? ki : 0ll)) * ki;
            if (lv_better(cand, best)) best = cand;
        }
        best = lv_wave_best(best);
        if (MODE != 0) {
            if (lane == 0u) red_G[wave] = best.G, red_C[wave] = best.C, red_own[wave] = best.own;
            __syncthreads();
            if (threadIdx.x == 0u)
                for (uint32_t v = 1; v < LV_WAVES; v++) {
                    const LvBest o = {red_G[v], red_C[v], red_own[v]};
                    if (lv_better(o, best)) best = o;
                }
        }
        if (tid == 0u) {
            int32_t to = own;
            if (best.C != own && !(size[own] == 1u && size[best.C] == 1u && best.C > own)) {
                to = best.C;
                atomicAdd(&st->moved, 1u);
            }
            lv.lab[nx][i] = to;
            atomicAdd(&lv.tot[nx][to], (uint32_t)ki);
            atomicAdd(&lv.size[nx][to], 1u);
        }
        lv_group_sync<MODE>();  // the table and the partials are free again
    }
}
// which: 0 or 1 = that buffer; 2 = the buffer the round wrote.  st->inside += sum of A_ij over the entries with equal labels
__global__ __launch_bounds__(LV_WG) void k_lv_inside(LvGraph g, LvLevel lv, LvState *__restrict__ st, uint32_t which) {
    if (which == 2u && st->stopped) return;
    const int32_t *__restrict__ lab = lv.lab[which == 2u ? st->cur ^ 1u : which];
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * LV_WG + threadIdx.x) >> 6, waves = ((uint64_t)gridDim.x * LV_WG) >> 6;
    unsigned long long s = 0;
    for (uint64_t i = wave0; i < g.n; i += waves) {
        const uint64_t a = (uint64_t)g.indptr[i], b = (uint64_t)g.indptr[i + 1];
        const int32_t own = lab[i];
        for (uint64_t e = a + lane; e < b; e += 64u) s += lab[g.indices[e]] == own ? g.weights[e] : 0u;
    }
    s = wave_sum(s);
    if (lane == 0u && s) atomicAdd(&st->inside, s);
}
__global__ __launch_bounds__(LV_WG) void k_lv_squares(LvLevel lv, uint32_t n, LvState *__restrict__ st, uint32_t which) {
    if (which == 2u && st->stopped) return;
    const uint32_t *__restrict__ tot = lv.tot[which == 2u ? st->cur ^ 1u : which];
    unsigned long long s = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * LV_WG + threadIdx.x; c < n; c += (uint64_t)gridDim.x * LV_WG) s += (unsigned long long)tot[c] * tot[c];
    s = wave_sum(s);
    if ((threadIdx.x & 63u) == 0u && s) atomicAdd(&st->squares, s);
}
// the round counts when a proposal survived and S rose; else the level ends with the labels it had
__global__ __launch_bounds__(64) void k_lv_decide(LvState *__restrict__ st) {
    if (threadIdx.x || st->stopped) return;
    const long long S2 = (long long)st->inside * (long long)st->M - (long long)st->squares;
    if (st->moved == 0u || S2 <= st->S) {
        st->stopped = 1u;
    } else {
        st->cur ^= 1u, st->S = S2, st->rounds += 1u;
        if (st->rounds >= st->max_rounds) st->stopped = 1u;
    }
}

// ---- between levels ------------------------------------------------------------------------------------------------------------------
struct LvUsedFlag {
    const uint32_t *size;
    __device__ __forceinline__ bool operator()(uint64_t c) const { return size[c] != 0u; }
};
struct LvEmitId {  // newid[C] = the rank of C among the used ids
    int32_t *newid;
    struct Pre {};
    __device__ __forceinline__ Pre pre(uint64_t) const { return Pre(); }
    __device__ __forceinline__ void operator()(uint64_t c, uint32_t o, Pre) const { newid[c] = (int32_t)o; }
};
__global__ __launch_bounds__(LV_WG) void k_lv_dense(const int32_t *__restrict__ lab, const int32_t *__restrict__ newid, uint32_t n,
                                                    int32_t *__restrict__ dense) {
    for (uint64_t i = (uint64_t)blockIdx.x * LV_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LV_WG) dense[i] = newid[lab[i]];
}
// comp[i] = dense[comp[i]] (first = 1: comp[i] = dense[i])
__global__ __launch_bounds__(LV_WG) void k_lv_compose(int32_t *__restrict__ comp, const int32_t *__restrict__ dense, uint32_t n, uint32_t first) {
    for (uint64_t i = (uint64_t)blockIdx.x * LV_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * LV_WG) comp[i] = dense[first ? (int32_t)i : comp[i]];
}
__global__ __launch_bounds__(LV_WG) void k_lv_agg_keys(LvGraph g, uint64_t nnz, const int32_t *__restrict__ dense, uint32_t n_c,
                                                       uint64_t *__restrict__ keys, uint32_t *__restrict__ perm) {
    for (uint64_t e = (uint64_t)blockIdx.x * LV_WG + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * LV_WG) {
        const uint32_t i = lv_row_of(g.indptr, g.n, e);
        keys[e] = (uint64_t)(uint32_t)dense[i] * n_c + (uint64_t)(uint32_t)dense[g.indices[e]];
        perm[e] = (uint32_t)e;
    }
}
// sums[o] += the weights of the run of ckeys[o]: a thread adds up LV_RUN_CHUNK consecutive sorted entries and touches memory once per
// run it meets.  Integer adds: no order.
__global__ __launch_bounds__(LV_WG) void k_lv_run_sums(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ perm,
                                                       const uint32_t *__restrict__ weights, uint64_t nnz, const uint64_t *__restrict__ ckeys,
                                                       uint64_t n_runs, uint32_t *__restrict__ sums) {
    const uint64_t chunks = (nnz + LV_RUN_CHUNK - 1u) / LV_RUN_CHUNK;
    for (uint64_t t = (uint64_t)blockIdx.x * LV_WG + threadIdx.x; t < chunks; t += (uint64_t)gridDim.x * LV_WG) {
        const uint64_t q0 = t * LV_RUN_CHUNK, q1 = q0 + LV_RUN_CHUNK < nnz ? q0 + LV_RUN_CHUNK : nnz;
        uint64_t key = keys[q0];
        uint32_t s = 0;
        for (uint64_t q = q0; q < q1; q++) {
            const uint64_t kq = keys[q];
            if (kq != key) {
                atomicAdd(&sums[cr_lower_bound(ckeys, n_runs, key)], s);
                key = kq, s = 0;
            }
            s += weights[perm[q]];
        }
        atomicAdd(&sums[cr_lower_bound(ckeys, n_runs, key)], s);
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
extern "C" int crgpu_modularity(const int64_t *indptr, const int32_t *indices, const uint32_t *weights, uint64_t n, const int32_t *labels, int64_t *S_out,
                                int64_t *M_out) {
    if (!indptr || !labels || !S_out || !M_out || n < 1 || n >= (1ull << 31) || (!indices && indptr[n] != 0)) return CRGPU_EINVAL;
    if (cr_csr_fault(indptr, indices, n, 32u, false).kind != CSR_FINE) return CRGPU_EINVAL;
    for (uint64_t i = 0; i < n; i++)
        if (labels[i] < 0) return CRGPU_EINVAL;
    uint64_t M = 0, inside = 0;
    std::unordered_map<int32_t, uint64_t> tot;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t k = 0;
        for (int64_t e = indptr[i]; e < indptr[i + 1]; e++) {
            const uint64_t w = weights ? weights[e] : 1u;
            if (weights && w == 0) return CRGPU_EINVAL;
            k += w;
            if (labels[indices[e]] == labels[i]) inside += w;
        }
        M += k;
        if (M >= (1ull << 31)) return CRGPU_ERANGE;
        tot[labels[i]] += k;
    }
    if (M < 1) return CRGPU_EINVAL;
    uint64_t squares = 0;
    for (const auto &t : tot) squares += t.second * t.second;
    *S_out = (int64_t)(inside * M) - (int64_t)squares, *M_out = (int64_t)M;
    return CRGPU_OK;
}

struct LvGraphBufs {
    DevBuf ptr, ind, w, k;
    uint64_t nnz = 0;
    uint32_t n = 0;
    LvGraph view() { return LvGraph{ptr.as<long long>(), ind.as<int32_t>(), w.as<uint32_t>(), k.as<uint32_t>(), n}; }
};
static int lv_alloc_graph(crgpu_ctx *ctx, LvGraphBufs &g, uint64_t n, uint64_t nnz) {
    CR_TRY(dmalloc(ctx, g.ptr, (n + 1) * sizeof(int64_t)));
    CR_TRY(dmalloc(ctx, g.ind, nnz * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, g.w, nnz * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, g.k, n * sizeof(uint32_t)));
    return CRGPU_OK;
}
// k, st->M, st->max_deg of the graph; *state = what the device holds afterwards
static int lv_degrees(crgpu_ctx *ctx, LvGraphBufs &g, LvState *d_st, LvState *state) {
    CR_HIP(ctx, hipMemsetAsync(d_st, 0, sizeof(LvState), ctx->stream));
    hipLaunchKernelGGL(k_lv_degrees, dim3(cr_grid((uint64_t)g.n * 64u, LV_WG)), dim3(LV_WG), 0, ctx->stream, g.ptr.as<long long>(), g.w.as<uint32_t>(), g.n,
                       g.k.as<uint32_t>(), d_st);
    CR_HIP(ctx, hipGetLastError());
    return crgpu_memcpy_d2h(ctx, state, d_st, sizeof(LvState));
}
// the nodes with more than lo and at most hi entries -> list, *count
static int lv_class_list(crgpu_ctx *ctx, LvGraphBufs &g, uint64_t lo, uint64_t hi, uint32_t *d_list, uint32_t *d_block, uint32_t *count) {
    CR_TRY(compact(ctx, LvClassFlag{g.ptr.as<long long>(), lo, hi}, LvEmitNode{d_list}, g.n, d_block, d_block + 4096));
    return read_u32(ctx, d_block + 4096, count);
}

extern "C" int crgpu_louvain_dev(crgpu_ctx *ctx, const int64_t *indptr, const int32_t *indices, const uint32_t *weights, uint64_t n,
                                 const crgpu_louvain_args *a, crgpu_louvain_result *res) {
    if (!ctx || !indptr || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const char *who = "crgpu_louvain_dev";
    // every refusal down to the upload comes before the device is touched
    CR_REQUIRE(ctx, n >= 1 && n < (1ull << 31), CRGPU_EINVAL, "%s: %llu nodes, 1 to 2^31 - 1", who, (unsigned long long)n);
    CR_REQUIRE(ctx, a->symmetrize <= 1u && a->reserved0 == 0u, CRGPU_EINVAL, "%s: symmetrize is 0 or 1, reserved is 0", who);
    CR_REQUIRE(ctx, !(a->symmetrize && weights), CRGPU_EINVAL, "%s: symmetrize = 1 takes no weights", who);
    CR_REQUIRE(ctx, a->wave_deg_max <= LV_WAVE_DEG_CAP && a->lds_deg_max <= LV_WG_DEG_CAP, CRGPU_EINVAL, "%s: wave_deg_max at most %u, lds_deg_max at most %u",
               who, LV_WAVE_DEG_CAP, LV_WG_DEG_CAP);
    CR_REQUIRE(ctx, indices || indptr[n] == 0, CRGPU_EINVAL, "%s: indices is NULL", who);
    CR_TRY(cr_check_csr(ctx, who, indptr, indices, n, 32u, false));  // the order of the columns: k_lv_check
    const uint64_t nnz_in = (uint64_t)indptr[n];
    CR_REQUIRE(ctx, nnz_in >= 1, CRGPU_EINVAL, "%s: a graph without an entry has M = 0", who);
    CR_REQUIRE(ctx, nnz_in < (1ull << 31), CRGPU_ERANGE, "%s: %llu entries, fewer than 2^31 (M < 2^31)", who, (unsigned long long)nnz_in);
    const uint32_t wave_max = a->wave_deg_max ? a->wave_deg_max : LV_WAVE_DEG_CAP, lds_max = a->lds_deg_max ? a->lds_deg_max : LV_WG_DEG_CAP;
    const uint32_t batch = a->batch ? a->batch : LV_BATCH, max_rounds = a->max_rounds ? a->max_rounds : LV_MAX_ROUNDS;
    const auto t0 = std::chrono::steady_clock::now();
    res->M = 0, res->levels_needed = res->nnz = 0;
    res->fit_ms = res->union_ms = res->rounds_ms = res->aggregate_ms = 0.0;
    res->n_levels = 0, res->wave_deg_max = wave_max, res->lds_deg_max = lds_max, res->batch = batch;

    const uint64_t n_keys = a->symmetrize ? 2 * nnz_in : nnz_in;
    DevBuf in_ptr, in_ind, keys_b, keyt_b, ckeys_b, perm_b, permt_b, block_b, state_b, flag_b;
    CR_TRY(dmalloc(ctx, keys_b, n_keys * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, keyt_b, n_keys * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, ckeys_b, n_keys * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, perm_b, n_keys * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, permt_b, n_keys * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, block_b, 4100 * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, state_b, sizeof(LvState)));
    uint32_t *d_block = block_b.as<uint32_t>(), *d_count = d_block + 4096;
    LvState *d_st = state_b.as<LvState>(), state;

    // ---- the level-0 graph
    LvGraphBufs ga, gb;
    if (a->symmetrize) {
        CR_TRY(dmalloc(ctx, in_ptr, (n + 1) * sizeof(int64_t)));
        CR_TRY(dmalloc(ctx, in_ind, nnz_in * sizeof(int32_t)));
        CR_TRY(crgpu_memcpy_h2d(ctx, in_ptr.p, indptr, (n + 1) * sizeof(int64_t)));
        CR_TRY(crgpu_memcpy_h2d(ctx, in_ind.p, indices, nnz_in * sizeof(int32_t)));
        hipLaunchKernelGGL(k_lv_keys, dim3(cr_grid(nnz_in, LV_WG)), dim3(LV_WG), 0, ctx->stream, in_ptr.as<long long>(), in_ind.as<int32_t>(), (uint32_t)n, nnz_in,
                           keys_b.as<uint64_t>());
        CR_HIP(ctx, hipGetLastError());
        SortedKeys sk;
        CR_TRY(cr_sort_keys(ctx, keys_b.as<uint64_t>(), keyt_b.as<uint64_t>(), nullptr, nullptr, n_keys, cr_ceil_log2(n * n), &sk));
        uint32_t merged = 0;
        CR_TRY(cr_merge_runs(ctx, sk.keys, LvEmitKey{sk.keys, ckeys_b.as<uint64_t>()}, n_keys, d_block, 1, n_keys, who, "merged entries", &merged));
        ga.n = gb.n = (uint32_t)n, ga.nnz = merged;
        CR_TRY(lv_alloc_graph(ctx, ga, n, merged));
        CR_TRY(lv_alloc_graph(ctx, gb, n, merged));
        cr_keys_to_csr(ctx, ckeys_b.as<uint64_t>(), merged, (uint32_t)n, ga.ptr.as<long long>(), ga.ind.as<int32_t>(), ga.w.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
    } else {
        ga.n = gb.n = (uint32_t)n, ga.nnz = nnz_in;
        CR_TRY(lv_alloc_graph(ctx, ga, n, nnz_in));
        CR_TRY(lv_alloc_graph(ctx, gb, n, nnz_in));
        CR_TRY(crgpu_memcpy_h2d(ctx, ga.ptr.p, indptr, (n + 1) * sizeof(int64_t)));
        CR_TRY(crgpu_memcpy_h2d(ctx, ga.ind.p, indices, nnz_in * sizeof(int32_t)));
        if (weights) {
            CR_TRY(crgpu_memcpy_h2d(ctx, ga.w.p, weights, nnz_in * sizeof(uint32_t)));
        } else {
            CR_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)ga.w.p, 1, nnz_in, ctx->stream));
        }
        CR_TRY(dmalloc(ctx, flag_b, sizeof(uint32_t)));
        CR_HIP(ctx, hipMemsetAsync(flag_b.p, 0, sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(k_lv_check, dim3(cr_grid(nnz_in, LV_WG)), dim3(LV_WG), 0, ctx->stream, ga.ptr.as<long long>(), ga.ind.as<int32_t>(), ga.w.as<uint32_t>(),
                           (uint32_t)n, nnz_in, flag_b.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
        uint32_t flag = 0;
        CR_TRY(read_u32(ctx, flag_b.as<uint32_t>(), &flag));
        CR_REQUIRE(ctx, !(flag & LV_BAD_ORDER), CRGPU_EINVAL, "%s: the columns of a row must be strictly ascending", who);
        CR_REQUIRE(ctx, !(flag & LV_BAD_WEIGHT), CRGPU_EINVAL, "%s: a weight of 0", who);
        CR_REQUIRE(ctx, !(flag & LV_BAD_TWIN), CRGPU_EINVAL, "%s: the graph is not symmetric", who);
    }
    CR_TRY(lv_degrees(ctx, ga, d_st, &state));
    const uint64_t M = state.M;
    CR_REQUIRE(ctx, M >= 1 && M < (1ull << 31), CRGPU_ERANGE, "%s: M = %llu, 1 to 2^31 - 1", who, (unsigned long long)M);
    res->M = (int64_t)M, res->nnz = ga.nnz;
    res->union_ms = cr_ms_since(t0);

    DevBuf lab0, lab1, tot0, tot1, size0, size1, newid_b, dense_b, comp_b, list1_b, list2_b;
    for (DevBuf *b : {&lab0, &lab1, &tot0, &tot1, &size0, &size1, &newid_b, &dense_b, &comp_b, &list1_b, &list2_b}) CR_TRY(dmalloc(ctx, *b, n * sizeof(uint32_t)));
    LvLevel lv = {{lab0.as<int32_t>(), lab1.as<int32_t>()}, {tot0.as<uint32_t>(), tot1.as<uint32_t>()}, {size0.as<uint32_t>(), size1.as<uint32_t>()}};
    LvGraphBufs *g = &ga, *spare = &gb;

    for (uint32_t level = 0; level < CRGPU_LOUVAIN_MAX_LEVELS; level++) {
        const auto t_level = std::chrono::steady_clock::now();
        const uint32_t nl = g->n, max_deg = state.max_deg;
        LvGraph gv = g->view();
        // the nodes of the second and third class, the tables of the third
        uint32_t n1 = 0, n2 = 0, dev_slots = 0, dev_groups = 0;
        DevBuf tk_b, tv_b;
        if (max_deg > wave_max && lds_max > wave_max) CR_TRY(lv_class_list(ctx, *g, wave_max, lds_max, list1_b.as<uint32_t>(), d_block, &n1));
        if (max_deg > std::max(wave_max, lds_max)) {
            CR_TRY(lv_class_list(ctx, *g, std::max(wave_max, lds_max), ~0ull, list2_b.as<uint32_t>(), d_block, &n2));
            CR_REQUIRE(ctx, max_deg < (1u << 30), CRGPU_ERANGE, "%s: a row of %u entries, fewer than 2^30", who, max_deg);
            dev_slots = lv_slots(max_deg, 64u);
            dev_groups = std::min(n2, LV_DEV_TABLES);
            while (dev_groups > 1u && (uint64_t)dev_groups * dev_slots > LV_DEV_SLOTS_MAX) dev_groups >>= 1;
            CR_TRY(dmalloc(ctx, tk_b, (uint64_t)dev_groups * dev_slots * sizeof(int32_t)));
            CR_TRY(dmalloc(ctx, tv_b, (uint64_t)dev_groups * dev_slots * sizeof(uint32_t)));
        }
        const uint32_t node_grid = cr_grid(nl, LV_WG), wave_grid = cr_grid((uint64_t)nl * 64u, LV_WG);
        hipLaunchKernelGGL(k_lv_identity, dim3(node_grid), dim3(LV_WG), 0, ctx->stream, lv, (const uint32_t *)gv.k, nl);
        hipLaunchKernelGGL(k_lv_inside, dim3(wave_grid), dim3(LV_WG), 0, ctx->stream, gv, lv, d_st, 0u);
        hipLaunchKernelGGL(k_lv_squares, dim3(node_grid), dim3(LV_WG), 0, ctx->stream, lv, nl, d_st, 0u);
        hipLaunchKernelGGL(k_lv_begin, dim3(1), dim3(64), 0, ctx->stream, d_st, max_rounds);
        CR_HIP(ctx, hipGetLastError());
        do {
            for (uint32_t r = 0; r < batch; r++) {
                hipLaunchKernelGGL(k_lv_prep, dim3(node_grid), dim3(LV_WG), 0, ctx->stream, lv, nl, d_st);
                hipLaunchKernelGGL(k_lv_round<0>, dim3(wave_grid), dim3(LV_WG), 0, ctx->stream, gv, lv, d_st, wave_max, (const uint32_t *)nullptr, 0u,
                                   (int32_t *)nullptr, (uint32_t *)nullptr, 0u);
                if (n1)
                    hipLaunchKernelGGL(k_lv_round<1>, dim3(cr_grid((uint64_t)n1 * LV_WG, LV_WG)), dim3(LV_WG), 0, ctx->stream, gv, lv, d_st, wave_max,
                                       (const uint32_t *)list1_b.as<uint32_t>(), n1, (int32_t *)nullptr, (uint32_t *)nullptr, 0u);
                if (n2)
                    hipLaunchKernelGGL(k_lv_round<2>, dim3(dev_groups), dim3(LV_WG), 0, ctx->stream, gv, lv, d_st, wave_max,
                                       (const uint32_t *)list2_b.as<uint32_t>(), n2, tk_b.as<int32_t>(), tv_b.as<uint32_t>(), dev_slots);
                hipLaunchKernelGGL(k_lv_inside, dim3(wave_grid), dim3(LV_WG), 0, ctx->stream, gv, lv, d_st, 2u);
                hipLaunchKernelGGL(k_lv_squares, dim3(node_grid), dim3(LV_WG), 0, ctx->stream, lv, nl, d_st, 2u);
                hipLaunchKernelGGL(k_lv_decide, dim3(1), dim3(64), 0, ctx->stream, d_st);
            }
            CR_HIP(ctx, hipGetLastError());
            CR_TRY(crgpu_memcpy_d2h(ctx, &state, d_st, sizeof(LvState)));
        } while (!state.stopped);
        const double level_ms = cr_ms_since(t_level);
        res->rounds_ms += level_ms;
        if (state.rounds == 0u && level) break;  // the first level without a counted round is not reported, unless it is level 0

        const auto t_agg = std::chrono::steady_clock::now();
        uint32_t n_c = 0;
        CR_TRY(compact(ctx, LvUsedFlag{lv.size[state.cur]}, LvEmitId{newid_b.as<int32_t>()}, nl, d_block, d_count));
        CR_TRY(read_u32(ctx, d_count, &n_c));
        CR_REQUIRE(ctx, n_c >= 1 && n_c <= nl, CRGPU_EHIP, "%s: %u communities of %u nodes", who, n_c, nl);
        hipLaunchKernelGGL(k_lv_dense, dim3(node_grid), dim3(LV_WG), 0, ctx->stream, (const int32_t *)lv.lab[state.cur], (const int32_t *)newid_b.as<int32_t>(), nl,
                           dense_b.as<int32_t>());
        hipLaunchKernelGGL(k_lv_compose, dim3(cr_grid(n, LV_WG)), dim3(LV_WG), 0, ctx->stream, comp_b.as<int32_t>(), (const int32_t *)dense_b.as<int32_t>(),
                           (uint32_t)n, level == 0u ? 1u : 0u);
        CR_HIP(ctx, hipGetLastError());
        if (res->level_nodes_out) res->level_nodes_out[level] = nl;
        if (res->level_communities_out) res->level_communities_out[level] = n_c;
        if (res->level_rounds_out) res->level_rounds_out[level] = state.rounds;
        if (res->level_S_out) res->level_S_out[level] = state.S;
        if (res->level_ms_out) res->level_ms_out[level] = level_ms;
        if (res->levels_out && res->levels_needed + nl <= a->levels_capacity)
            CR_TRY(crgpu_memcpy_d2h(ctx, res->levels_out + res->levels_needed, dense_b.p, (uint64_t)nl * sizeof(int32_t)));
        res->levels_needed += nl;
        res->n_levels = level + 1u;
        if (level == 0u && res->level0_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->level0_out, comp_b.p, n * sizeof(int32_t)));
        if (state.rounds == 0u) break;  // level 0 as the identity

        // ---- the next level's graph: A'_CD = the sum of A_ij over c_i = C, c_j = D
        hipLaunchKernelGGL(k_lv_agg_keys, dim3(cr_grid(g->nnz, LV_WG)), dim3(LV_WG), 0, ctx->stream, gv, g->nnz, (const int32_t *)dense_b.as<int32_t>(), n_c,
                           keys_b.as<uint64_t>(), perm_b.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
        SortedKeys sk;
        CR_TRY(cr_sort_keys(ctx, keys_b.as<uint64_t>(), keyt_b.as<uint64_t>(), perm_b.as<uint32_t>(), permt_b.as<uint32_t>(), g->nnz, cr_ceil_log2((uint64_t)n_c * n_c),
                            &sk));
        uint32_t runs = 0;
        CR_TRY(cr_merge_runs(ctx, sk.keys, LvEmitKey{sk.keys, ckeys_b.as<uint64_t>()}, g->nnz, d_block, 1, g->nnz, who, "entries of the aggregated graph", &runs));
        CR_HIP(ctx, hipMemsetAsync(spare->w.p, 0, (uint64_t)runs * sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(k_lv_run_sums, dim3(cr_grid((g->nnz + LV_RUN_CHUNK - 1u) / LV_RUN_CHUNK, LV_WG)), dim3(LV_WG), 0, ctx->stream, sk.keys, sk.perm,
                           (const uint32_t *)gv.weights, g->nnz, (const uint64_t *)ckeys_b.as<uint64_t>(), (uint64_t)runs, spare->w.as<uint32_t>());
        cr_keys_to_csr(ctx, ckeys_b.as<uint64_t>(), runs, n_c, spare->ptr.as<long long>(), spare->ind.as<int32_t>(), nullptr);
        CR_HIP(ctx, hipGetLastError());
        spare->n = n_c, spare->nnz = runs;
        std::swap(g, spare);
        CR_TRY(lv_degrees(ctx, *g, d_st, &state));
        CR_REQUIRE(ctx, state.M == M, CRGPU_EHIP, "%s: the aggregated graph has M = %llu, not %llu", who, (unsigned long long)state.M, (unsigned long long)M);
        res->aggregate_ms += cr_ms_since(t_agg);
    }
    if (res->final_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->final_out, comp_b.p, n * sizeof(int32_t)));
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    res->fit_ms = cr_ms_since(t0);
    return CRGPU_OK;
}
