// knn.hip -- exact k-nearest-neighbour graph of a dense projection: the hot path of RUN_GRAPH_CLUSTERING on the device.
//
// Replaces compute_nearest_neighbors (lib/python/cellranger/analysis/graphclust.py:39-62): scikit-learn 1.7.2's
// BallTree(x, leaf_size).query(rows, k + 1) followed by [:, 1:].  The tree only prunes; what it returns is, for every query row i, the
// k + 1 smallest pairs (d2(i, j), j) over ALL rows j, i included, with
//     d2 = the sum over t = 0 .. d - 1 of (x_t - y_t) * (x_t - y_t), in that order, f64, unfused,
// and the reported distance the correctly rounded root of d2.  (d2, j) is a total order, so the result is a pure function of the
// input: no run, no switch, no query range and no other row can move a bit of it.  d2 >= +0.0 always, so its bit pattern orders as
// the value does and the key of a pair is (bits of d2, j).
// QUIRK kept (it is the reference's): the FIRST pair is dropped, not the pair of the row itself.  A row with an exact duplicate of
// lower index drops the duplicate and keeps itself as a neighbour at distance 0.
//
// crgpu_knn_cross_dev is find_knn of CORRECT_CHEMISTRY_BATCH (lib/python/cellranger/analysis/batch_correction.py:106-115): the same two
// kernels with a candidate range, an index base and a drop count of 0 in KnnShape -- the first k pairs over the candidate rows alone.
//
// Launch structure.  Brute force over tiles, no pruning by any expansion of the norm.
//   k_knn_select   a workgroup owns 64 queries, lane = query, the query's row in registers (d <= 16) or transposed in LDS.  Candidate
//                  tiles stream through LDS; wave w takes candidates w, w + 4, ...: every lane reads the same LDS address.  A query
//                  has a running bound, the (k + 1)-th smallest d2 of its last selection (all ones before the first), and a buffer
//                  of `capacity` pairs: in LDS while 64 buffers fit KNN_LDS_BUF bytes, else in device memory.  A pair with d2 <= bound
//                  is appended (an LDS counter gives the slot: the ORDER in a buffer depends on the run, the SET does not).  Before a
//                  step of at most capacity - (k + 1) candidates the workgroup looks whether a buffer could overflow in it; if one
//                  could, every such buffer and every buffer more than half full is cut to its k + 1 smallest by a bitonic sort in
//                  LDS, which tightens the bound.  A pair of the final answer is never above a bound, ties included.
//   k_knn_final    a workgroup a query: the buffer sorted by (d2, j); ranks 1 .. k are the answer (0 .. k - 1 of a cross query); the
//                  root; the same k indices sorted ascending (the CSR row of merge_nearest_neighbors).
// No floating-point atomic anywhere; the only atomics are the LDS slot counters and three u64 event counters.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "block_utils.h"
#include "common.h"

#define KNN_WG 256u
#define KNN_QT 64u            // queries per workgroup
#define KNN_WAVES (KNN_WG / 64u)
#define KNN_DR 16u            // up to here a query's row is kept in registers
#define KNN_MAX_CAP 4096u     // pairs of a buffer at the most: 48 KiB of LDS for its sort
#define KNN_MAX_TILE 256u     // candidates of an LDS tile at the most
#define KNN_TILE_DOUBLES 2560u  // doubles of a candidate tile: 20 KiB
#define KNN_LDS_BUF 49152u    // bytes of LDS the 64 buffers may take
#define KNN_PAD_KEY 0xFFFFFFFFFFFFFFFFull

// The device matrix holds the rows the call needs; q0, nq: the query rows in it; c0, nc: the candidate rows in it; ibase: what is added
// to a candidate's position among the candidates to give the index reported; drop: pairs left out at the head of the order (1:
// crgpu_knn_dev, 0: crgpu_knn_cross_dev); K = k + drop pairs are kept per query.
struct KnnShape {
    uint32_t d, q0, nq, c0, nc, ibase, drop, K, cap, tile, step, in_lds;
};

// ---- host: the rule of split() ---------------------------------------------------------------------------------------------------
extern "C" int crgpu_graphclust_num_neighbors(uint64_t n, uint32_t num_neighbors, double a, double b, uint32_t *k_out) {
    if (!k_out || n < 2 || !std::isfinite(a) || !std::isfinite(b)) return CRGPU_EINVAL;
    // int(max(num_neighbors, np.round(a + b * np.log10(n)))): round half to even, then the clamp to [1, n - 1]
    const double rule = std::nearbyint(a + b * std::log10((double)n));
    double use = (double)num_neighbors > rule ? (double)num_neighbors : rule;
    const double hi = (double)(n - 1 < 0xFFFFFFFFull ? n - 1 : 0xFFFFFFFFull);
    use = use < 1.0 ? 1.0 : use > hi ? hi : use;
    *k_out = (uint32_t)use;
    return CRGPU_OK;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool knn_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) { return ka < kb || (ka == kb && ia < ib); }

// ascending bitonic sort of p2 (a power of two) pairs in LDS by the whole workgroup; ends with a barrier
__device__ __forceinline__ void knn_bitonic(uint64_t *sk, uint32_t *si, uint32_t p2) {
    for (uint32_t size = 2u; size <= p2; size <<= 1)
        for (uint32_t j = size >> 1; j > 0u; j >>= 1) {
            __syncthreads();
            for (uint32_t e = threadIdx.x; e < (p2 >> 1); e += KNN_WG) {
                const uint32_t lo = ((e & ~(j - 1u)) << 1) | (e & (j - 1u)), hi = lo | j;
                const uint64_t ka = sk[lo], kb = sk[hi];
                const uint32_t ia = si[lo], ib = si[hi];
                const bool up = (lo & size) == 0u;
                if (knn_less(kb, ib, ka, ia) == up) sk[lo] = kb, si[lo] = ib, sk[hi] = ka, si[hi] = ia;
            }
        }
    __syncthreads();
}
__device__ __forceinline__ uint32_t knn_pow2(uint32_t v) {
    uint32_t p = 2u;
    while (p < v) p <<= 1;
    return p;
}
// cnt pairs of one buffer into the sort area, padded to a power of two, sorted
__device__ __forceinline__ uint32_t knn_load_sorted(const uint64_t *bk, const uint32_t *bi, uint32_t cnt, uint64_t *sk, uint32_t *si) {
    const uint32_t p2 = knn_pow2(cnt);
    __syncthreads();  // the sort area is free, the appends are visible
    for (uint32_t e = threadIdx.x; e < p2; e += KNN_WG) {
        const bool have = e < cnt;
        sk[e] = have ? bk[e] : KNN_PAD_KEY;
        si[e] = have ? bi[e] : 0xFFFFFFFFu;
    }
    knn_bitonic(sk, si, p2);
    return p2;
}

// Dynamic LDS, in this order: the candidate tile (tile * d doubles), with !REG the queries transposed (d * 64 doubles), the sort keys
// (pow2(cap) u64), with in_lds the buffer keys (64 * cap u64); then the sort indices (pow2(cap) u32) and the buffer indices.
template <bool REG>
__global__ __launch_bounds__(KNN_WG) void k_knn_select(const double *__restrict__ x, KnnShape s, uint64_t *__restrict__ gkey, uint32_t *__restrict__ gidx,
                                                       uint32_t *__restrict__ gcnt, unsigned long long *__restrict__ counters) {
    extern __shared__ double knn_lds[];
    __shared__ uint32_t s_cnt[KNN_QT];
    __shared__ uint64_t s_bound[KNN_QT];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, d = s.d, K = s.K, cap = s.cap;
    const uint32_t p2cap = knn_pow2(cap);
    double *s_y = knn_lds;
    double *s_q = s_y + (size_t)s.tile * d;
    uint64_t *s_sk = (uint64_t *)(s_q + (REG ? 0u : d * KNN_QT));
    uint64_t *s_bk = s_sk + p2cap;
    uint32_t *s_si = (uint32_t *)(s_bk + (s.in_lds ? KNN_QT * cap : 0u));
    uint32_t *s_bi = s_si + p2cap;
    const uint32_t qt0 = blockIdx.x * KNN_QT, qi = qt0 + lane;
    const bool live = qi < s.nq;
    const uint32_t qrow = s.q0 + (live ? qi : s.nq - 1u);  // a lane without a query computes on the last one and appends nothing
    // the buffer of the tile's query ql
    uint64_t *const tk = s.in_lds ? s_bk : gkey + (size_t)qt0 * cap;
    uint32_t *const ti = s.in_lds ? s_bi : gidx + (size_t)qt0 * cap;

    double xr[REG ? KNN_DR : 1u];
    if (REG) {
#pragma unroll
        for (uint32_t t = 0; t < KNN_DR; t++) xr[t] = t < d ? x[(size_t)qrow * d + t] : 0.0;
    } else {
        for (uint32_t e = tid; e < KNN_QT * d; e += KNN_WG) {
            const uint32_t ql = e / d, t = e % d, q = qt0 + ql;
            s_q[t * KNN_QT + ql] = x[(size_t)(s.q0 + (q < s.nq ? q : s.nq - 1u)) * d + t];
        }
    }
    if (tid < KNN_QT) s_cnt[tid] = 0u, s_bound[tid] = KNN_PAD_KEY;
    uint32_t events = 0, cuts = 0;
    unsigned long long appended = 0;

    for (uint32_t c0 = 0; c0 < s.nc; c0 += s.tile) {
        const uint32_t m = s.nc - c0 < s.tile ? s.nc - c0 : s.tile;
        __syncthreads();  // the previous tile is done with
        for (uint32_t e = tid; e < m * d; e += KNN_WG) s_y[e] = x[(size_t)(s.c0 + c0) * d + e];
        __syncthreads();
        for (uint32_t s0 = 0; s0 < m; s0 += s.step) {
            const uint32_t s1 = s0 + s.step < m ? s0 + s.step : m;
            // could a buffer overflow in this step?  Every wave sees the same counters: the appends ended at a barrier
            if (__syncthreads_or(live && s_cnt[lane] + (s1 - s0) > cap)) {
                events++;
                for (uint32_t ql = 0; ql < KNN_QT; ql++) {
                    const uint32_t cnt = s_cnt[ql] < cap ? s_cnt[ql] : cap;  // uniform
                    // cut what could overflow in this step and, while the workgroup is at it, what is more than half full
                    if (cnt + (s1 - s0) <= cap && 2u * cnt <= K + cap) continue;
                    uint64_t *bk = tk + (size_t)ql * cap;
                    uint32_t *bi = ti + (size_t)ql * cap;
                    knn_load_sorted(bk, bi, cnt, s_sk, s_si);
                    for (uint32_t e = tid; e < K; e += KNN_WG) bk[e] = s_sk[e], bi[e] = s_si[e];
                    if (tid == 0u) s_cnt[ql] = K, s_bound[ql] = s_sk[K - 1u];
                    cuts++;
                }
                __syncthreads();
            }
            const uint64_t bound = s_bound[lane];
            uint64_t *bk = tk + (size_t)lane * cap;
            uint32_t *bi = ti + (size_t)lane * cap;
            for (uint32_t c = s0 + wave; c < s1; c += KNN_WAVES) {
                const double *y = s_y + (size_t)c * d;
                double a = 0.0;
                if (REG) {
#pragma unroll
                    for (uint32_t t = 0; t < KNN_DR; t++)
                        if (t < d) {
                            const double v = xr[t] - y[t];
                            a += v * v;
                        }
                } else {
                    for (uint32_t t = 0; t < d; t++) {
                        const double v = s_q[t * KNN_QT + lane] - y[t];
                        a += v * v;
                    }
                }
                const uint64_t key = (uint64_t)__double_as_longlong(a);
                if (live && key <= bound) {
                    const uint32_t pos = atomicAdd(&s_cnt[lane], 1u);
                    if (pos < cap) bk[pos] = key, bi[pos] = s.ibase + c0 + c;  // pos < cap by the step rule; the test keeps a fault out of memory
                    appended++;
                }
            }
            __syncthreads();
        }
    }
    // the buffers and their counts to device memory
    if (s.in_lds)
        for (uint32_t ql = 0; ql < KNN_QT; ql++) {
            const uint32_t cnt = s_cnt[ql] < cap ? s_cnt[ql] : cap;
            for (uint32_t e = tid; e < cnt; e += KNN_WG) {
                gkey[(size_t)(qt0 + ql) * cap + e] = s_bk[(size_t)ql * cap + e];
                gidx[(size_t)(qt0 + ql) * cap + e] = s_bi[(size_t)ql * cap + e];
            }
        }
    if (tid < KNN_QT) gcnt[qt0 + tid] = s_cnt[tid];
    appended = wave_sum(appended);
    if (lane == 0u) atomicAdd(&counters[2], appended);
    if (tid == 0u) atomicAdd(&counters[0], (unsigned long long)events), atomicAdd(&counters[1], (unsigned long long)cuts);
}

// Dynamic LDS: pow2(cap) u64, then pow2(cap) u32
__global__ __launch_bounds__(KNN_WG) void k_knn_final(KnnShape s, const uint64_t *__restrict__ gkey, const uint32_t *__restrict__ gidx,
                                                      const uint32_t *__restrict__ gcnt, int32_t *__restrict__ ind, double *__restrict__ dist,
                                                      int32_t *__restrict__ sorted, uint32_t *__restrict__ bad) {
    extern __shared__ double knn_lds[];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, K = s.K, drop = s.drop, k = K - drop, cap = s.cap;
    uint64_t *sk = (uint64_t *)knn_lds;
    uint32_t *si = (uint32_t *)(sk + knn_pow2(cap));
    const uint32_t cnt = gcnt[q];
    if (cnt < K || cnt > cap) {  // uniform: never by the rules of k_knn_select; said to the host instead of a wrong row
        if (tid == 0u) atomicOr(bad, 1u);
        return;
    }
    knn_load_sorted(gkey + (size_t)q * cap, gidx + (size_t)q * cap, cnt, sk, si);
    uint32_t mine[(CRGPU_KNN_MAX_K + KNN_WG - 1u) / KNN_WG];
#pragma unroll
    for (uint32_t r = 0; r < (CRGPU_KNN_MAX_K + KNN_WG - 1u) / KNN_WG; r++) {
        const uint32_t e = tid + r * KNN_WG;
        mine[r] = 0xFFFFFFFFu;
        if (e < k) {
            mine[r] = si[e + drop];
            ind[(size_t)q * k + e] = (int32_t)mine[r];
            dist[(size_t)q * k + e] = sqrt(__longlong_as_double((long long)sk[e + drop]));
        }
    }
    // the same k indices ascending
    const uint32_t p2 = knn_pow2(k);
    __syncthreads();
    for (uint32_t e = tid; e < p2; e += KNN_WG) sk[e] = KNN_PAD_KEY, si[e] = 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < (CRGPU_KNN_MAX_K + KNN_WG - 1u) / KNN_WG; r++) {
        const uint32_t e = tid + r * KNN_WG;
        if (e < k) sk[e] = (uint64_t)mine[r];
    }
    knn_bitonic(sk, si, p2);
    for (uint32_t e = tid; e < k; e += KNN_WG) sorted[(size_t)q * k + e] = (int32_t)(uint32_t)sk[e];
}

// ---- the entry point -------------------------------------------------------------------------------------------------------------
static uint32_t knn_host_pow2(uint32_t v) {
    uint32_t p = 2u;
    while (p < v) p <<= 1;
    return p;
}

// What the two entry points share, after each has checked its own arguments: the rows [q0, q0 + nq) query the rows [c0, c0 + nc).
// all_rows: the whole matrix goes to the device (crgpu_knn_dev); else the query rows and behind them the candidate rows
// (crgpu_knn_cross_dev), and a candidate's index is reported as c0 + its position.
struct KnnCall {
    const char *who;
    uint64_t n, ld, q0, nq, c0, nc;
    uint32_t d, k, drop, capacity, force_device, cand_tile, reserved;
    bool all_rows;
};
static int knn_run(crgpu_ctx *ctx, const double *x, const KnnCall &c, crgpu_knn_result *res) {
    const uint32_t d = c.d, k = c.k, K = k + c.drop;
    const uint64_t nq = c.nq;
    // the buffer: by default the power of two from 2 K up, at least 64
    uint32_t cap = c.capacity ? c.capacity : std::min(KNN_MAX_CAP, std::max(64u, knn_host_pow2(2u * K)));
    CR_REQUIRE(ctx, cap >= K + KNN_WAVES && cap <= KNN_MAX_CAP, CRGPU_EINVAL, "%s: a buffer of %u pairs, k + %u = %u to %u", c.who, cap, c.drop + KNN_WAVES,
               K + KNN_WAVES, KNN_MAX_CAP);
    const uint32_t tile_max = std::max(KNN_WAVES, std::min(KNN_MAX_TILE, (KNN_TILE_DOUBLES / d) & ~(KNN_WAVES - 1u)));
    const uint32_t tile = c.cand_tile ? c.cand_tile : tile_max;
    CR_REQUIRE(ctx, tile >= KNN_WAVES && tile <= tile_max && tile % KNN_WAVES == 0u, CRGPU_EINVAL,
               "%s: a candidate tile of %u rows, a multiple of %u up to %u for %u dimensions", c.who, tile, KNN_WAVES, tile_max, d);
    CR_REQUIRE(ctx, c.force_device <= 1u && c.reserved == 0u, CRGPU_EINVAL, "%s: force_device is 0 or 1, reserved 0", c.who);
    const auto t0 = std::chrono::steady_clock::now();
    // the first d columns of the rows that are used, packed; an infinity or a NaN is refused
    const uint64_t seg_lo[2] = {c.all_rows ? 0 : c.q0, c.c0}, seg_n[2] = {c.all_rows ? c.n : c.nq, c.all_rows ? 0 : c.nc};
    std::vector<double> xp((size_t)(seg_n[0] + seg_n[1]) * d);
    size_t at = 0;
    for (int g = 0; g < 2; g++)
        for (uint64_t i = seg_lo[g]; i < seg_lo[g] + seg_n[g]; i++)
            for (uint32_t t = 0; t < d; t++) {
                const double v = x[i * c.ld + t];
                CR_REQUIRE(ctx, std::isfinite(v), CRGPU_EINVAL, "%s: x[%llu, %u] is not finite", c.who, (unsigned long long)i, t);
                xp[at++] = v;
            }

    KnnShape s;
    s.d = d, s.q0 = (uint32_t)(c.all_rows ? c.q0 : 0), s.nq = (uint32_t)nq, s.c0 = (uint32_t)(c.all_rows ? c.c0 : c.nq), s.nc = (uint32_t)c.nc;
    s.ibase = (uint32_t)(c.all_rows ? 0 : c.c0), s.drop = c.drop, s.K = K, s.cap = cap, s.tile = tile;
    s.step = std::min(tile, (cap - K) & ~(KNN_WAVES - 1u));
    s.in_lds = (!c.force_device && (uint64_t)KNN_QT * cap * 12u <= KNN_LDS_BUF) ? 1u : 0u;
    const bool reg = d <= KNN_DR;
    const uint32_t p2cap = knn_host_pow2(cap), n_tiles = (s.nq + KNN_QT - 1u) / KNN_QT;
    const size_t lds_final = (size_t)p2cap * 12u;
    const size_t lds_select = ((size_t)tile * d + (reg ? 0u : (size_t)d * KNN_QT)) * sizeof(double) + lds_final + (s.in_lds ? (size_t)KNN_QT * cap * 12u : 0u);
    CR_REQUIRE(ctx, lds_select <= 160u * 1024u - 1024u, CRGPU_EHIP, "%s: %llu bytes of LDS", c.who, (unsigned long long)lds_select);

    DevBuf x_b, key_b, idx_b, cnt_b, ctr_b, ind_b, dist_b, sorted_b;
    const uint64_t rows = (uint64_t)n_tiles * KNN_QT;
    CR_TRY(dmalloc(ctx, x_b, xp.size() * sizeof(double)));
    CR_TRY(dmalloc(ctx, key_b, rows * cap * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, idx_b, rows * cap * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, cnt_b, rows * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, ctr_b, 4 * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, ind_b, nq * k * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, dist_b, nq * k * sizeof(double)));
    CR_TRY(dmalloc(ctx, sorted_b, nq * k * sizeof(int32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, x_b.p, xp.data(), xp.size() * sizeof(double)));
    CR_HIP(ctx, hipMemsetAsync(ctr_b.p, 0, 4 * sizeof(uint64_t), ctx->stream));
    unsigned long long *d_ctr = ctr_b.as<unsigned long long>();
    uint32_t *d_bad = (uint32_t *)(d_ctr + 3);

    CrEvents<3> events(ctx);
    hipEvent_t *ev = events.e;
    CR_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    if (reg) {
        cr_allow_lds(ctx, (const void *)k_knn_select<true>, lds_select);
        hipLaunchKernelGGL(k_knn_select<true>, dim3(n_tiles), dim3(KNN_WG), lds_select, ctx->stream, x_b.as<double>(), s, key_b.as<uint64_t>(),
                           idx_b.as<uint32_t>(), cnt_b.as<uint32_t>(), d_ctr);
    } else {
        cr_allow_lds(ctx, (const void *)k_knn_select<false>, lds_select);
        hipLaunchKernelGGL(k_knn_select<false>, dim3(n_tiles), dim3(KNN_WG), lds_select, ctx->stream, x_b.as<double>(), s, key_b.as<uint64_t>(),
                           idx_b.as<uint32_t>(), cnt_b.as<uint32_t>(), d_ctr);
    }
    CR_HIP(ctx, hipGetLastError());
    CR_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    cr_allow_lds(ctx, (const void *)k_knn_final, lds_final);
    hipLaunchKernelGGL(k_knn_final, dim3(s.nq), dim3(KNN_WG), lds_final, ctx->stream, s, key_b.as<uint64_t>(), idx_b.as<uint32_t>(), cnt_b.as<uint32_t>(),
                       ind_b.as<int32_t>(), dist_b.as<double>(), sorted_b.as<int32_t>(), d_bad);
    CR_HIP(ctx, hipGetLastError());
    CR_HIP(ctx, hipEventRecord(ev[2], ctx->stream));

    uint64_t ctr[4] = {0, 0, 0, 0};
    CR_TRY(crgpu_memcpy_d2h(ctx, ctr, ctr_b.p, sizeof(ctr)));
    CR_REQUIRE(ctx, (uint32_t)ctr[3] == 0u, CRGPU_EHIP, "%s: a query's buffer lost its count", c.who);
    if (res->indices_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->indices_out, ind_b.p, nq * k * sizeof(int32_t)));
    if (res->distances_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->distances_out, dist_b.p, nq * k * sizeof(double)));
    if (res->sorted_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->sorted_out, sorted_b.p, nq * k * sizeof(int32_t)));
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms_a = 0.0f, ms_b = 0.0f;
    CR_HIP(ctx, hipEventElapsedTime(&ms_a, ev[0], ev[1]));
    CR_HIP(ctx, hipEventElapsedTime(&ms_b, ev[1], ev[2]));
    res->select_ms = ms_a, res->sort_ms = ms_b;
    res->fit_ms = cr_ms_since(t0);
    res->compactions = ctr[0], res->selections = ctr[1], res->survivors = ctr[2], res->pairs_evaluated = nq * c.nc;
    res->in_lds = s.in_lds, res->capacity = cap, res->query_tiles = n_tiles, res->cand_tile = tile;
    return CRGPU_OK;
}

extern "C" int crgpu_knn_dev(crgpu_ctx *ctx, const double *x, uint64_t n, uint32_t d, uint64_t ld, uint32_t k, const crgpu_knn_args *a,
                             crgpu_knn_result *res) {
    if (!ctx || !x || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    // every refusal below and in knn_run comes before the device is touched
    CR_REQUIRE(ctx, n >= 2 && n < (1ull << 31), CRGPU_EINVAL, "crgpu_knn_dev: %llu rows, 2 to 2^31 - 1", (unsigned long long)n);
    CR_REQUIRE(ctx, d >= 1 && d <= CRGPU_KM_MAX_D && ld >= d, CRGPU_EINVAL, "crgpu_knn_dev: %u dimensions (1 to %u) in rows of %llu", d, CRGPU_KM_MAX_D,
               (unsigned long long)ld);
    CR_REQUIRE(ctx, k >= 1 && k <= CRGPU_KNN_MAX_K && k < n, CRGPU_EINVAL, "crgpu_knn_dev: k = %u, 1 to min(%u, the %llu rows - 1)", k, CRGPU_KNN_MAX_K,
               (unsigned long long)n);
    const bool all = a->query_start == 0 && a->n_queries == 0;
    const uint64_t q0 = a->query_start, nq = all ? n : a->n_queries;
    CR_REQUIRE(ctx, nq >= 1 && q0 < n && nq <= n - q0, CRGPU_EINVAL, "crgpu_knn_dev: queries %llu + %llu of %llu rows", (unsigned long long)q0,
               (unsigned long long)a->n_queries, (unsigned long long)n);
    const KnnCall c = {"crgpu_knn_dev", n, ld, q0, nq, 0, n, d, k, 1u, a->capacity, a->force_device, a->cand_tile, a->reserved, true};
    return knn_run(ctx, x, c, res);
}

// find_knn(cur_matrix, ref_matrix, knn) of CORRECT_CHEMISTRY_BATCH: the k first pairs (d2, j) over the candidate rows alone, nothing
// dropped, the indices global row numbers (include/crgpu.h)
extern "C" int crgpu_knn_cross_dev(crgpu_ctx *ctx, const double *x, uint64_t n, uint32_t d, uint64_t ld, uint32_t k, const crgpu_knn_cross_args *a,
                                   crgpu_knn_result *res) {
    if (!ctx || !x || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, n >= 1 && n < (1ull << 31), CRGPU_EINVAL, "crgpu_knn_cross_dev: %llu rows, 1 to 2^31 - 1", (unsigned long long)n);
    CR_REQUIRE(ctx, d >= 1 && d <= CRGPU_KM_MAX_D && ld >= d, CRGPU_EINVAL, "crgpu_knn_cross_dev: %u dimensions (1 to %u) in rows of %llu", d,
               CRGPU_KM_MAX_D, (unsigned long long)ld);
    CR_REQUIRE(ctx, a->n_queries >= 1 && a->query_start < n && a->n_queries <= n - a->query_start, CRGPU_EINVAL,
               "crgpu_knn_cross_dev: queries %llu + %llu of %llu rows", (unsigned long long)a->query_start, (unsigned long long)a->n_queries,
               (unsigned long long)n);
    CR_REQUIRE(ctx, a->n_cands >= 1 && a->cand_start < n && a->n_cands <= n - a->cand_start, CRGPU_EINVAL,
               "crgpu_knn_cross_dev: candidates %llu + %llu of %llu rows", (unsigned long long)a->cand_start, (unsigned long long)a->n_cands,
               (unsigned long long)n);
    CR_REQUIRE(ctx, k >= 1 && k <= CRGPU_KNN_MAX_K && k <= a->n_cands, CRGPU_EINVAL, "crgpu_knn_cross_dev: k = %u, 1 to min(%u, the %llu candidates)", k,
               CRGPU_KNN_MAX_K, (unsigned long long)a->n_cands);
    const KnnCall c = {"crgpu_knn_cross_dev", n, ld, a->query_start, a->n_queries, a->cand_start, a->n_cands, d, k, 0u, a->capacity, a->force_device,
                       a->cand_tile, a->reserved, false};
    return knn_run(ctx, x, c, res);
}

