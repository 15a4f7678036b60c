// kmeans.h -- k-means clustering of a dense projection: RUN_KMEANS on the device (part of matrix_stages.hip).
//
// Replaces run_kmeans (lib/python/cellranger/analysis/kmeans.py:67-95): scikit-learn 1.7.2's KMeans(n_clusters, random_state) --
// k-means++ seeding, Lloyd, inertia -- then compute_db_index and relabel_by_size.  One call fits a LIST of K values on one matrix.
// QUIRKS kept (they are scikit-learn's):
//   * when the seeding potential is 0 every draw lands on cell 0;
//   * a cluster of weight 0 is not left at the origin: _average_centers gives it the row of the FIRST heaviest cluster as that row
//     stands when the loop reaches it -- already averaged when the heaviest cluster has the lower index, the raw sum otherwise;
//   * the centre shift and the inertia add the squared differences four dimensions at a time (_euclidean_dense_dense);
//   * on the strict stop (the labels repeat) the labels are those of the OLD centres, the centres and the inertia the new ones.
//
// Launch structure.  Position p of the K list is the second grid dimension of every kernel but the assign pass, which reads a tile of
// 256 cells ONCE and serves every live position from it.  A position that has stopped (or waits for the host, below) returns at once.
//   seeding, per further centre   k_km_seed_update  closest squared distance per cell, sums of 64 cells taken serially
//                                 k_km_seed_super   sums of 64 such sums, serially
//                                 k_km_seed_locate  the potential (the super sums, serially) and, per trial draw u * potential, the
//                                                   first cell whose cumulative sum reaches it: a walk down the three levels
//                                 k_km_seed_cand    per trial candidate the 256-cell partials of min(closest, distance to it)
//                                 k_km_seed_pick    the partials in ascending order; the smallest potential wins, the first on a tie
//   Lloyd, per round              k_km_assign       label = argmin ||c||^2 - 2 x.c (dimension order, the first centre on a tie);
//                                                   per 256-cell tile the sums and weights per cluster, added in CELL order (the tile's
//                                                   cells are grouped by cluster first, a stable counting sort by ballots)
//                                 k_km_reduce       64 tiles at a time, ascending
//                                 k_km_close_a      the groups ascending; an empty cluster latches "wait for the host"
//                                 k_km_close_b      averages, shifts, the stop rule and its latch, the new centres and norms
//   after the stop                k_km_assign (labels only, where the stop was not strict), k_km_final, k_km_final_close
// Every sum over cells is per-workgroup partials in a slab of plain stores, added by a second kernel in an order that depends on n
// alone: no floating-point atomic; runs, both switches, and a K alone or in a list are bit-identical.  The centres and their norms
// of one position sit in LDS while K * D <= ctx->km_lds_centers (CRGPU_KM_LDS_CENTERS), else they are read from device memory.
// The host reads the latches once per ctx->km_batch rounds (CRGPU_KM_BATCH).  Empty clusters are rare and need a selection over all
// cells: the position parks itself in the round that finds one, the host relocates (_relocate_empty_clusters_dense: the points
// farthest from their own old centre, by distance then index descending, to the empty clusters ascending; nothing when the largest
// distance is 0) and runs that position's k_km_close_b; no other position and no result depends on where in a batch this happens.
// f64 throughout, unfused.
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <vector>

#include "marginal_calls.h"
#include "stage_common.h"

#define KM_WG 256u
#define KM_SEG 64u        // cells per serial sum of the seeding
#define KM_GROUP 64u      // tiles per partial of k_km_reduce
#define KM_MAXK CRGPU_KM_MAX_K
#define KM_MAXD CRGPU_KM_MAX_D
#define KM_MAXT 6u        // 2 + int(log(64)) trial candidates at the most
#define KM_TILE_D 16u     // up to here a tile's rows are kept in LDS and a cell's row in registers

struct KmState {
    double tol, pot;
    uint32_t k, round, stopped, strict, n_iter, paused, relocs, in_lds, changed, seeded, n_trials, reserved;
    uint32_t cand[8];
    uint32_t chosen[KM_MAXK];
};

// ---- host: the draws, the Davies-Bouldin index, the relabelling ----------------------------------------------------------------------
static inline uint32_t km_trials(uint32_t k) {  // 2 + int(np.log(k)); e^1 .. e^4 = 2.7, 7.4, 20.1, 54.6
    return 2u + (k >= 55u ? 4u : k >= 21u ? 3u : k >= 8u ? 2u : k >= 3u ? 1u : 0u);
}
// RandomState(seed).choice(n, p = ones / n): p.cumsum(), cdf /= cdf[-1], searchsorted(side = "right"), without the array
static uint64_t km_first_cell(uint64_t n, double u) {
    const double p = 1.0 / (double)n;
    double last = 0.0;
    for (uint64_t i = 0; i < n; i++) last += p;
    double s = 0.0;
    for (uint64_t i = 0; i < n; i++) {
        s += p;
        if (s / last > u) return i;
    }
    return n - 1;
}
static void km_seed_draws(uint32_t seed, uint64_t n, uint32_t k, double *u_out, uint64_t *first_cell_out) {
    McMt g(seed);
    const uint32_t n_u = 1u + (k - 1u) * km_trials(k);
    for (uint32_t i = 0; i < n_u; i++) u_out[i] = g.random_sample();
    *first_cell_out = km_first_cell(n, u_out[0]);
}
extern "C" int crgpu_kmeans_seed_draws(uint32_t seed, uint64_t n, uint32_t k, double *u_out, uint64_t *first_cell_out) {
    if (!u_out || !first_cell_out || !n || !k || k > KM_MAXK) return CRGPU_EINVAL;
    km_seed_draws(seed, n, k, u_out, first_cell_out);
    return CRGPU_OK;
}

extern "C" int crgpu_kmeans_db_index(uint32_t k, uint32_t d, const double *centers, const double *wss, const uint64_t *counts, double *score) {
    if (!k || k > KM_MAXK || !d || d > KM_MAXD || !centers || !wss || !counts || !score) return CRGPU_EINVAL;
    double scatter[KM_MAXK], worst[KM_MAXK];
    for (uint32_t i = 0; i < k; i++) scatter[i] = std::sqrt(wss[i] / (double)(counts[i] ? counts[i] : 1ull));
    for (uint32_t i = 0; i < k; i++) {
        double mx = 0.0;  // the diagonal is 0 and no entry is negative
        for (uint32_t j = 0; j < k; j++) {
            if (j == i) continue;
            double s = 0.0;
            for (uint32_t t = 0; t < d; t++) {
                const double v = centers[(size_t)i * d + t] - centers[(size_t)j * d + t];
                s += v * v;
            }
            double dist = std::sqrt(s);
            if (std::fabs(dist) < 1e-3) dist = 1e-3;
            const double m = (scatter[j] + scatter[i]) / dist;
            if (m > mx || std::isnan(m)) mx = m;
        }
        worst[i] = mx;
    }
    *score = cr_pairwise_sum(worst, k) / (double)k;
    return CRGPU_OK;
}

// relabel_by_size: argsort(argsort(-bincount(1-based labels))) with a stable order among equal sizes; index 0 has count 0
static void km_relabel(const int32_t *labels, uint64_t n, uint32_t k, const uint64_t *sizes, int32_t *clusters) {
    uint32_t idx[KM_MAXK + 1u], rank[KM_MAXK + 1u];
    for (uint32_t j = 0; j <= k; j++) idx[j] = j;
    std::stable_sort(idx, idx + k + 1u, [&](uint32_t a, uint32_t b) { return (a ? sizes[a - 1u] : 0ull) > (b ? sizes[b - 1u] : 0ull); });
    for (uint32_t r = 0; r <= k; r++) rank[idx[r]] = r;
    for (uint64_t i = 0; i < n; i++) clusters[i] = 1 + (int32_t)rank[labels[i] + 1];
}

// ---- device helpers ------------------------------------------------------------------------------------------------------------------
// _euclidean_dense_dense(squared): four dimensions at a time, then the rest
__device__ __forceinline__ double km_sqdist4(const double *a, const double *b, uint32_t d) {
    double r = 0.0;
    uint32_t t = 0;
    for (; t + 4u <= d; t += 4u) {
        const double d0 = a[t] - b[t], d1 = a[t + 1u] - b[t + 1u], d2 = a[t + 2u] - b[t + 2u], d3 = a[t + 3u] - b[t + 3u];
        r += ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
    }
    for (; t < d; t++) r += (a[t] - b[t]) * (a[t] - b[t]);
    return r;
}
// np.sum of n <= 128 contiguous values
__device__ __forceinline__ double km_np_sum(const double *a, uint32_t n) {
    if (n < 8u) {
        double r = 0.0;
        for (uint32_t i = 0; i < n; i++) r += a[i];
        return r;
    }
    double r[8];
    for (uint32_t j = 0; j < 8u; j++) r[j] = a[j];
    uint32_t i = 8u;
    for (; i < n - (n % 8u); i += 8u)
        for (uint32_t j = 0; j < 8u; j++) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a[i];
    return res;
}
// the squared distance of the seeding (euclidean_distances): ((-2 x.y) + ||y||^2) + ||x||^2, not below 0
__device__ __forceinline__ double km_seed_dist(const double *x, const double *y, uint32_t d, double xx, double yy) {
    double dot = 0.0;
    for (uint32_t t = 0; t < d; t++) dot += x[t] * y[t];
    const double v = (-2.0 * dot + yy) + xx;
    return v > 0.0 ? v : 0.0;
}

// ---- centring ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KM_WG) void k_km_center(const double *__restrict__ x, uint32_t n, uint32_t d, uint64_t ld, const double *__restrict__ mean,
                                                     double *__restrict__ xc, double *__restrict__ xx) {
    const uint32_t i = blockIdx.x * KM_WG + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (uint32_t t = 0; t < d; t++) {
        const double v = x[(size_t)i * ld + t] - mean[t];
        xc[(size_t)i * d + t] = v;
        s += v * v;
    }
    xx[i] = s;
}

// ---- seeding -------------------------------------------------------------------------------------------------------------------------
// round c >= 1: closest = distance to chosen[0] (c == 1) or min(closest, distance to chosen[c - 1]); the sums of 64 cells, serially
__global__ __launch_bounds__(KM_WG) void k_km_seed_update(const double *__restrict__ xc, const double *__restrict__ xx, uint32_t n, uint32_t d,
                                                          const KmState *__restrict__ st, uint32_t c, double *__restrict__ closest,
                                                          double *__restrict__ seg, uint32_t n_seg) {
    __shared__ double s_y[KM_MAXD];
    __shared__ double s_v[KM_WG];
    const uint32_t p = blockIdx.y;
    const KmState *s = st + p;
    if (s->seeded || c >= s->k) return;
    const uint32_t tid = threadIdx.x, ch = s->chosen[c - 1u];
    for (uint32_t t = tid; t < d; t += KM_WG) s_y[t] = xc[(size_t)ch * d + t];
    __syncthreads();
    const uint32_t i = blockIdx.x * KM_WG + tid;
    double v = 0.0;
    if (i < n) {
        v = km_seed_dist(xc + (size_t)i * d, s_y, d, xx[i], xx[ch]);
        double *cl = closest + (size_t)p * n + i;
        if (c > 1u) {
            const double old = *cl;
            v = old < v ? old : v;
        }
        *cl = v;
    }
    s_v[tid] = v;
    __syncthreads();
    if ((tid & 63u) == 0u) {
        const uint32_t sg = blockIdx.x * (KM_WG / KM_SEG) + (tid >> 6);
        if (sg < n_seg) {
            double a = 0.0;
            for (uint32_t j = 0; j < KM_SEG; j++) a += s_v[tid + j];  // a cell beyond n adds +0.0
            seg[(size_t)p * n_seg + sg] = a;
        }
    }
}
__global__ __launch_bounds__(KM_WG) void k_km_seed_super(const KmState *__restrict__ st, uint32_t c, const double *__restrict__ seg, uint32_t n_seg,
                                                         double *__restrict__ sup, uint32_t n_sup) {
    const uint32_t p = blockIdx.y;
    if (st[p].seeded || c >= st[p].k) return;
    const uint32_t u = blockIdx.x * KM_WG + threadIdx.x;
    if (u >= n_sup) return;
    const uint32_t lo = u * KM_SEG, hi = lo + KM_SEG < n_seg ? lo + KM_SEG : n_seg;
    double a = 0.0;
    for (uint32_t j = lo; j < hi; j++) a += seg[(size_t)p * n_seg + j];
    sup[(size_t)p * n_sup + u] = a;
}
// searchsorted(cumulative sum, u * potential), clipped to n - 1.  The cumulative sum is taken down three levels, each serially; a
// level that does not reach the value for rounding ends at its last element.
__global__ __launch_bounds__(64) void k_km_seed_locate(KmState *st, uint32_t c, const double *__restrict__ u_draws, uint32_t u_stride,
                                                       const double *__restrict__ closest, const double *__restrict__ seg, const double *__restrict__ sup,
                                                       uint32_t n, uint32_t n_seg, uint32_t n_sup) {
    __shared__ double s_pot;
    const uint32_t p = blockIdx.x;
    KmState *s = st + p;
    if (s->seeded || c >= s->k) return;
    const double *sp = sup + (size_t)p * n_sup, *sg = seg + (size_t)p * n_seg, *cl = closest + (size_t)p * n;
    if (threadIdx.x == 0u) {
        double a = 0.0;
        for (uint32_t u = 0; u < n_sup; u++) a += sp[u];
        s_pot = a;
        s->pot = a;
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t >= s->n_trials) return;
    const double v = u_draws[(size_t)p * u_stride + 1u + (size_t)(c - 1u) * s->n_trials + t] * s_pot;
    double acc = 0.0;
    uint32_t u = 0;
    for (; u + 1u < n_sup; u++) {
        const double nx = acc + sp[u];
        if (nx >= v) break;
        acc = nx;
    }
    uint32_t g = u * KM_SEG;
    const uint32_t g_hi = g + KM_SEG < n_seg ? g + KM_SEG : n_seg;
    for (; g + 1u < g_hi; g++) {
        const double nx = acc + sg[g];
        if (nx >= v) break;
        acc = nx;
    }
    uint32_t i = g * KM_SEG;
    const uint32_t i_hi = i + KM_SEG < n ? i + KM_SEG : n;
    for (; i + 1u < i_hi; i++) {
        const double nx = acc + cl[i];
        if (nx >= v) break;
        acc = nx;
    }
    s->cand[t] = i;
}
// per trial candidate the tile's sum of min(closest, distance to the candidate): the butterfly, then the four waves ascending
__global__ __launch_bounds__(KM_WG) void k_km_seed_cand(const double *__restrict__ xc, const double *__restrict__ xx, uint32_t n, uint32_t d,
                                                        const KmState *__restrict__ st, uint32_t c, const double *__restrict__ closest,
                                                        double *__restrict__ slab, uint32_t n_tiles) {
    __shared__ double s_y[KM_MAXT * KM_MAXD];
    __shared__ double s_yy[KM_MAXT];
    __shared__ double s_red[KM_WG / 64u][KM_MAXT];
    const uint32_t p = blockIdx.y;
    const KmState *s = st + p;
    if (s->seeded || c >= s->k) return;
    const uint32_t tid = threadIdx.x, T = s->n_trials;
    for (uint32_t e = tid; e < T * d; e += KM_WG) s_y[e] = xc[(size_t)s->cand[e / d] * d + e % d];
    if (tid < T) s_yy[tid] = xx[s->cand[tid]];
    __syncthreads();
    const uint32_t i = blockIdx.x * KM_WG + tid;
    const bool live = i < n;
    const double cl = live ? closest[(size_t)p * n + i] : 0.0, xi = live ? xx[i] : 0.0;
    for (uint32_t t = 0; t < T; t++) {
        double v = 0.0;
        if (live) {
            v = km_seed_dist(xc + (size_t)i * d, s_y + (size_t)t * d, d, xi, s_yy[t]);
            v = cl < v ? cl : v;
        }
        v = wave_sum(v);
        if ((tid & 63u) == 0u) s_red[tid >> 6][t] = v;
    }
    __syncthreads();
    if (tid < T) slab[((size_t)p * n_tiles + blockIdx.x) * KM_MAXT + tid] = ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}
__global__ __launch_bounds__(64) void k_km_seed_pick(KmState *st, uint32_t c, const double *__restrict__ slab, uint32_t n_tiles) {
    __shared__ double s_pot[KM_MAXT];
    const uint32_t p = blockIdx.x;
    KmState *s = st + p;
    if (s->seeded || c >= s->k) return;
    const uint32_t t = threadIdx.x, T = s->n_trials;
    if (t < T) {
        double a = 0.0;
#pragma unroll 8
        for (uint32_t b = 0; b < n_tiles; b++) a += slab[((size_t)p * n_tiles + b) * KM_MAXT + t];
        s_pot[t] = a;
    }
    __syncthreads();
    if (t == 0u) {
        uint32_t best = 0;
        for (uint32_t j = 1; j < T; j++)
            if (s_pot[j] < s_pot[best]) best = j;
        s->chosen[c] = s->cand[best];
    }
}
// the seeded centres and their squared norms
__global__ __launch_bounds__(KM_WG) void k_km_seed_centres(const double *__restrict__ xc, uint32_t d, const KmState *__restrict__ st, double *__restrict__ cen,
                                                           double *__restrict__ cc, uint32_t kd_max) {
    const uint32_t p = blockIdx.y, j = blockIdx.x;
    const KmState *s = st + p;
    if (j >= s->k) return;
    double *row = cen + (size_t)p * kd_max + (size_t)j * d;
    if (!s->seeded)
        for (uint32_t t = threadIdx.x; t < d; t += KM_WG) row[t] = xc[(size_t)s->chosen[j] * d + t];
    __syncthreads();
    if (threadIdx.x == 0u) {
        double a = 0.0;
        for (uint32_t t = 0; t < d; t++) a += row[t] * row[t];
        cc[(size_t)p * KM_MAXK + j] = a;
    }
}

// ---- Lloyd ---------------------------------------------------------------------------------------------------------------------------
// A tile of 256 cells, every live position in turn.  final_labels = 0: a round (labels, the changed latch, the tile's sums and
// weights); 1: the labels under the final centres for the positions whose stop was not strict.
// Dynamic LDS: the centres and norms of one position (lds_centres + KM_MAXK doubles), with TILE the tile's rows (256 d doubles).
template <bool TILE>
__global__ __launch_bounds__(KM_WG) void k_km_assign(const double *__restrict__ xc, uint32_t n, uint32_t d, KmState *st, uint32_t n_ks,
                                                     const double *__restrict__ cen, const double *__restrict__ cc, uint32_t kd_max,
                                                     int32_t *__restrict__ labels, double *__restrict__ slab, uint32_t n_tiles, uint32_t n_stat_max,
                                                     uint32_t lds_centres, uint32_t final_labels) {
    extern __shared__ double km_lds[];
    __shared__ uint32_t s_cnt[KM_WG / 64u][KM_MAXK];  // per wave the cells of each cluster
    __shared__ uint32_t s_off[KM_MAXK + 1u];
    __shared__ uint16_t s_order[KM_WG];
    double *s_c = km_lds, *s_cc = km_lds + lds_centres, *s_x = km_lds + lds_centres + KM_MAXK;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, i0 = blockIdx.x * KM_WG, i = i0 + tid;
    const bool live = i < n;
    double xr[TILE ? KM_TILE_D : 1u];
    if (TILE) {
#pragma unroll
        for (uint32_t t = 0; t < KM_TILE_D; t++) {
            xr[t] = (live && t < d) ? xc[(size_t)i * d + t] : 0.0;
            if (t < d) s_x[(size_t)tid * d + t] = xr[t];
        }
    }
    for (uint32_t p = 0; p < n_ks; p++) {
        const KmState *s = st + p;
        if (final_labels ? (!s->stopped || s->strict) : (s->stopped || s->paused)) continue;  // uniform
        const uint32_t K = s->k, kd = K * d;
        const bool in_lds = s->in_lds != 0u;
        const double *gc = cen + (size_t)p * kd_max, *gcc = cc + (size_t)p * KM_MAXK;
        __syncthreads();  // the previous position's centres and labels are done with
        if (in_lds) {
            for (uint32_t e = tid; e < kd; e += KM_WG) s_c[e] = gc[e];
            if (tid < K) s_cc[tid] = gcc[tid];
        }
        __syncthreads();
        const double *c = in_lds ? s_c : gc, *cn = in_lds ? s_cc : gcc;
        int32_t lab = 0;
        if (live) {
            double best = 0.0;
            const double *xrow = xc + (size_t)i * d;
            for (uint32_t j = 0; j < K; j++) {
                const double *cj = c + (size_t)j * d;
                double dot = 0.0;
                if (TILE) {
#pragma unroll
                    for (uint32_t t = 0; t < KM_TILE_D; t++)
                        if (t < d) dot += xr[t] * cj[t];
                } else {
                    for (uint32_t t = 0; t < d; t++) dot += xrow[t] * cj[t];
                }
                const double v = cn[j] + -2.0 * dot;
                if (j == 0u || v < best) best = v, lab = (int32_t)j;
            }
            int32_t *lp = labels + (size_t)p * n + i;
            const bool changed = *lp != lab;
            *lp = lab;
            if (!final_labels && __any(changed) && (tid & 63u) == 0u) atomicOr(&st[p].changed, 1u);  // lane 0 is live when any lane is
        }
        if (final_labels) continue;
        // The tile's cells grouped by cluster, ascending inside a cluster (a stable counting sort: per wave a ballot per cluster), so
        // that a cluster's sum walks its own cells only -- in cell order, the order of the sum is that of a masked walk of the tile.
        const int32_t mine = live ? lab : -1;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < K; j++) {  // uniform: every lane of every wave votes
            const unsigned long long votes = __ballot(mine == (int32_t)j);
            if (mine == (int32_t)j) rank = (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
            if (lane == 0u) s_cnt[wave][j] = (uint32_t)__popcll(votes);
        }
        __syncthreads();
        if (tid <= K) {  // s_off[j] = the cells of the clusters below j; s_off[K] = the cells of the tile
            uint32_t o = 0;
            for (uint32_t jj = 0; jj < tid; jj++) o += ((s_cnt[0][jj] + s_cnt[1][jj]) + s_cnt[2][jj]) + s_cnt[3][jj];
            s_off[tid] = o;
        }
        __syncthreads();
        if (live) {
            uint32_t pos = s_off[lab] + rank;
            for (uint32_t w = 0; w < wave; w++) pos += s_cnt[w][lab];
            s_order[pos] = (uint16_t)tid;
        }
        __syncthreads();
        // statistic e < K d: the sum of dimension e % d over the tile's cells of cluster e / d; e >= K d: the cluster's weight
        const uint32_t n_stat = kd + K;
        double *out = slab + ((size_t)p * n_tiles + blockIdx.x) * n_stat_max;
        for (uint32_t e = tid; e < n_stat; e += KM_WG) {
            double a = 0.0;
            if (e < kd) {
                const uint32_t j = e / d, t = e % d, hi = s_off[j + 1u];
                if (TILE) {
#pragma unroll 4
                    for (uint32_t o = s_off[j]; o < hi; o++) a += s_x[(size_t)s_order[o] * d + t];
                } else {
#pragma unroll 4
                    for (uint32_t o = s_off[j]; o < hi; o++) a += xc[(size_t)(i0 + s_order[o]) * d + t];
                }
            } else {
                a = (double)(s_off[e - kd + 1u] - s_off[e - kd]);
            }
            out[e] = a;
        }
    }
}
// 64 tiles at a time, ascending
__global__ __launch_bounds__(KM_WG) void k_km_reduce(const KmState *__restrict__ st, uint32_t d, const double *__restrict__ slab, uint32_t n_tiles,
                                                     uint32_t n_stat_max, double *__restrict__ slab2, uint32_t n_groups) {
    const uint32_t p = blockIdx.y, g = blockIdx.x;
    const KmState *s = st + p;
    if (s->stopped || s->paused) return;
    const uint32_t n_stat = s->k * d + s->k, lo = g * KM_GROUP, hi = lo + KM_GROUP < n_tiles ? lo + KM_GROUP : n_tiles;
    for (uint32_t e = threadIdx.x; e < n_stat; e += KM_WG) {
        double a = 0.0;
#pragma unroll 8
        for (uint32_t b = lo; b < hi; b++) a += slab[((size_t)p * n_tiles + b) * n_stat_max + e];
        slab2[((size_t)p * n_groups + g) * n_stat_max + e] = a;
    }
}
// the groups ascending; an empty cluster parks the position for the host
__global__ __launch_bounds__(KM_WG) void k_km_close_a(KmState *st, uint32_t d, const double *__restrict__ slab2, uint32_t n_groups, uint32_t n_stat_max,
                                                      double *__restrict__ sums) {
    __shared__ uint32_t s_empty;
    const uint32_t p = blockIdx.x;
    KmState *s = st + p;
    if (s->stopped || s->paused) return;
    const uint32_t K = s->k, kd = K * d, n_stat = kd + K;
    if (threadIdx.x == 0u) s_empty = 0u;
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < n_stat; e += KM_WG) {
        double a = 0.0;
#pragma unroll 8
        for (uint32_t g = 0; g < n_groups; g++) a += slab2[((size_t)p * n_groups + g) * n_stat_max + e];
        sums[(size_t)p * n_stat_max + e] = a;
        if (e >= kd && a == 0.0) atomicAdd(&s_empty, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0u && s_empty) s->paused = 1u;
}
// _average_centers, _center_shift, the stop rule of _kmeans_single_lloyd; only = one position (after a relocation) or NONE32
__global__ __launch_bounds__(KM_WG) void k_km_close_b(KmState *st, uint32_t d, double *__restrict__ sums, uint32_t n_stat_max, double *__restrict__ cen,
                                                      double *__restrict__ cc, uint32_t kd_max, uint32_t max_iter, uint32_t only) {
    __shared__ double s_shift[KM_MAXK];
    __shared__ uint32_t s_heavy;
    const uint32_t p = blockIdx.x;
    KmState *s = st + p;
    if (s->stopped || s->paused || (only != NONE32 && p != only)) return;
    const uint32_t K = s->k, kd = K * d, tid = threadIdx.x;
    double *sm = sums + (size_t)p * n_stat_max, *c = cen + (size_t)p * kd_max;
    const double *w = sm + kd;
    if (tid == 0u) {
        uint32_t h = 0;
        for (uint32_t j = 1; j < K; j++)
            if (w[j] > w[h]) h = j;
        s_heavy = h;
    }
    __syncthreads();
    const uint32_t heavy = s_heavy;
    const double alpha_h = 1.0 / w[heavy];
    constexpr uint32_t PER = KM_MAXK * KM_MAXD / KM_WG;
    double nv[PER];
#pragma unroll
    for (uint32_t r = 0; r < PER; r++) {
        const uint32_t e = tid + r * KM_WG;
        nv[r] = 0.0;
        if (e >= kd) continue;
        const uint32_t j = e / d, t = e % d;
        if (w[j] > 0.0) {
            const double alpha = 1.0 / w[j];
            nv[r] = sm[e] * alpha;
        } else {
            const double raw = sm[(size_t)heavy * d + t];
            nv[r] = heavy < j ? raw * alpha_h : raw;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < PER; r++) {  // the new centres, in place of the sums
        const uint32_t e = tid + r * KM_WG;
        if (e < kd) sm[e] = nv[r];
    }
    __syncthreads();
    if (tid < K) {  // (center_shift ** 2).sum() squares the root again
        const double shift = sqrt(km_sqdist4(sm + (size_t)tid * d, c + (size_t)tid * d, d));
        s_shift[tid] = shift * shift;
    }
    __syncthreads();
    if (tid == 0u) {
        const uint32_t it = s->round;
        const bool changed = s->changed != 0u;
        s->changed = 0u;
        s->round = it + 1u;
        if (!changed) {
            s->stopped = 1u, s->strict = 1u, s->n_iter = it + 1u;
        } else {
            if (km_np_sum(s_shift, K) <= s->tol || it + 1u >= max_iter) s->stopped = 1u, s->n_iter = it + 1u;
        }
    }
    for (uint32_t e = tid; e < kd; e += KM_WG) c[e] = sm[e];
    __syncthreads();
    if (tid < K) {
        double a = 0.0;
        for (uint32_t t = 0; t < d; t++) a += c[(size_t)tid * d + t] * c[(size_t)tid * d + t];
        cc[(size_t)p * KM_MAXK + tid] = a;
    }
}
// the squared distance of every cell to its own current centre, in dimension order (for the relocation of one position)
__global__ __launch_bounds__(KM_WG) void k_km_own_dist(const double *__restrict__ xc, uint32_t n, uint32_t d, const double *__restrict__ c,
                                                       const int32_t *__restrict__ labels, double *__restrict__ out) {
    const uint32_t i = blockIdx.x * KM_WG + threadIdx.x;
    if (i >= n) return;
    const double *cj = c + (size_t)labels[i] * d;
    double a = 0.0;
    for (uint32_t t = 0; t < d; t++) {
        const double v = xc[(size_t)i * d + t] - cj[t];
        a += v * v;
    }
    out[i] = a;
}
__global__ void k_km_resume(KmState *st, uint32_t p, uint32_t relocs) {
    st[p].paused = 0u;
    st[p].relocs = st[p].relocs + relocs;
}

// per tile and cluster, in cell order: wss on the uncentred data against the centres as returned, the sizes; the tile's inertia
__global__ __launch_bounds__(KM_WG) void k_km_final(const double *__restrict__ x, uint64_t ld, const double *__restrict__ xc, uint32_t n, uint32_t d,
                                                    const double *__restrict__ mean, const KmState *__restrict__ st, const double *__restrict__ cen,
                                                    uint32_t kd_max, const int32_t *__restrict__ labels, double *__restrict__ slab, uint32_t n_tiles) {
    __shared__ double s_in[KM_WG], s_ws[KM_WG];
    __shared__ int32_t s_lab[KM_WG];
    const uint32_t p = blockIdx.y, tid = threadIdx.x, i0 = blockIdx.x * KM_WG, i = i0 + tid;
    const uint32_t K = st[p].k, m = n - i0 < KM_WG ? n - i0 : KM_WG;
    if (i < n) {
        const int32_t lab = labels[(size_t)p * n + i];
        const double *cj = cen + (size_t)p * kd_max + (size_t)lab * d;
        s_lab[tid] = lab;
        s_in[tid] = km_sqdist4(xc + (size_t)i * d, cj, d);
        double a = 0.0;
        for (uint32_t t = 0; t < d; t++) {
            const double v = x[(size_t)i * ld + t] - (cj[t] + mean[t]);
            a += v * v;
        }
        s_ws[tid] = a;
    }
    __syncthreads();
    double *out = slab + ((size_t)p * n_tiles + blockIdx.x) * (2u * KM_MAXK + 1u);
    if (tid < K) {
        double a = 0.0, cnt = 0.0;
#pragma unroll 8
        for (uint32_t q = 0; q < m; q++) {
            const bool mine = s_lab[q] == (int32_t)tid;
            a += mine ? s_ws[q] : 0.0, cnt += mine ? 1.0 : 0.0;
        }
        out[tid] = a, out[KM_MAXK + tid] = cnt;
    } else if (tid == KM_MAXK) {
        double a = 0.0;
#pragma unroll 8
        for (uint32_t q = 0; q < m; q++) a += s_in[q];
        out[2u * KM_MAXK] = a;
    }
}
__global__ __launch_bounds__(KM_WG) void k_km_final_close(const KmState *__restrict__ st, const double *__restrict__ slab, uint32_t n_tiles,
                                                          double *__restrict__ out) {
    const uint32_t p = blockIdx.x, tid = threadIdx.x, K = st[p].k;
    const uint32_t w = 2u * KM_MAXK + 1u;
    if (!(tid < K || (tid >= KM_MAXK && tid < KM_MAXK + K) || tid == 2u * KM_MAXK)) return;
    double a = 0.0;
#pragma unroll 8
    for (uint32_t b = 0; b < n_tiles; b++) a += slab[((size_t)p * n_tiles + b) * w + tid];
    out[(size_t)p * w + tid] = a;
}

// ---- the entry point -----------------------------------------------------------------------------------------------------------------
static void km_launch_assign(crgpu_ctx *ctx, bool tile, uint32_t n_tiles, size_t dyn, const double *xc, uint32_t n, uint32_t d, KmState *st, uint32_t n_ks,
                             const double *cen, const double *cc, uint32_t kd_max, int32_t *labels, double *slab, uint32_t n_stat_max, uint32_t lds_centres,
                             uint32_t final_labels) {
    if (tile)
        hipLaunchKernelGGL(k_km_assign<true>, dim3(n_tiles), dim3(KM_WG), dyn, ctx->stream, xc, n, d, st, n_ks, cen, cc, kd_max, labels, slab, n_tiles,
                           n_stat_max, lds_centres, final_labels);
    else
        hipLaunchKernelGGL(k_km_assign<false>, dim3(n_tiles), dim3(KM_WG), dyn, ctx->stream, xc, n, d, st, n_ks, cen, cc, kd_max, labels, slab, n_tiles,
                           n_stat_max, lds_centres, final_labels);
}

extern "C" int crgpu_kmeans_dev(crgpu_ctx *ctx, const double *x, uint64_t n, uint32_t d, uint64_t ld, const uint32_t *ks, uint32_t n_ks,
                                const crgpu_kmeans_args *a, crgpu_kmeans_result *res) {
    if (!ctx || !x || !ks || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, n_ks >= 1 && n_ks <= CRGPU_KM_MAX_LIST, CRGPU_EINVAL, "crgpu_kmeans_dev: %u values of K, 1 to %u", n_ks, CRGPU_KM_MAX_LIST);
    CR_REQUIRE(ctx, d >= 1 && d <= KM_MAXD && ld >= d, CRGPU_EINVAL, "crgpu_kmeans_dev: %u dimensions (1 to %u) in rows of %llu", d, KM_MAXD,
               (unsigned long long)ld);
    CR_REQUIRE(ctx, n >= 1 && n < (1ull << 31), CRGPU_EINVAL, "crgpu_kmeans_dev: %llu cells, 1 to 2^31 - 1", (unsigned long long)n);
    uint32_t k_max = 0;
    for (uint32_t p = 0; p < n_ks; p++) {
        CR_REQUIRE(ctx, ks[p] >= 1 && ks[p] <= KM_MAXK && ks[p] <= n, CRGPU_EINVAL, "crgpu_kmeans_dev: K = %u, 1 to min(%u, the %llu cells)", ks[p], KM_MAXK,
                   (unsigned long long)n);
        for (uint32_t q = 0; q < p; q++) CR_REQUIRE(ctx, ks[q] != ks[p], CRGPU_EINVAL, "crgpu_kmeans_dev: K = %u is listed twice", ks[p]);
        k_max = std::max(k_max, ks[p]);
    }
    CR_REQUIRE(ctx, a->max_iter >= 1, CRGPU_EINVAL, "crgpu_kmeans_dev: max_iter 0");
    const uint32_t n32 = (uint32_t)n, kd_max = k_max * d, n_stat_max = kd_max + k_max;
    const uint32_t n_tiles = (n32 + KM_WG - 1u) / KM_WG, n_groups = (n_tiles + KM_GROUP - 1u) / KM_GROUP;
    const uint32_t n_seg = (n32 + KM_SEG - 1u) / KM_SEG, n_sup = (n_seg + KM_SEG - 1u) / KM_SEG;
    const uint32_t fw = 2u * KM_MAXK + 1u;
    const auto t0 = std::chrono::steady_clock::now();

    // X.mean(axis = 0) and np.var(X, axis = 0): sums over the rows in row order; the mean of the variances in numpy's pairwise order
    std::vector<double> mean(d, 0.0), var(d, 0.0);
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t t = 0; t < d; t++) mean[t] += x[i * ld + t];
    for (uint32_t t = 0; t < d; t++) {  // an infinity or a NaN anywhere in a column ends in its sum
        CR_REQUIRE(ctx, std::isfinite(mean[t]), CRGPU_EINVAL, "crgpu_kmeans_dev: column %u holds a value that is not finite, or its sum overflows", t);
        mean[t] /= (double)n;
    }
    for (uint64_t i = 0; i < n; i++)
        for (uint32_t t = 0; t < d; t++) {
            const double v = x[i * ld + t] - mean[t];
            var[t] += v * v;
        }
    for (uint32_t t = 0; t < d; t++) {
        CR_REQUIRE(ctx, std::isfinite(var[t]), CRGPU_EINVAL, "crgpu_kmeans_dev: the variance of column %u overflows", t);
        var[t] /= (double)n;
    }
    const double tol = a->tol_factor == 0.0 ? 0.0 : cr_pairwise_sum(var.data(), d) / (double)d * a->tol_factor;

    // the states, the draws, the centres given by the caller (init - X_mean)
    std::vector<KmState> h(n_ks);
    uint32_t u_stride = 1, seed_rounds = 0;
    for (uint32_t p = 0; p < n_ks; p++) u_stride = std::max(u_stride, 1u + (ks[p] - 1u) * km_trials(ks[p]));
    std::vector<double> draws((size_t)n_ks * u_stride, 0.0), cen_h((size_t)n_ks * kd_max, 0.0);
    uint64_t first_cell = 0;
    bool have_first = false;
    for (uint32_t p = 0; p < n_ks; p++) {
        KmState &s = h[p];
        memset(&s, 0, sizeof(s));
        s.tol = tol, s.k = ks[p], s.n_trials = km_trials(ks[p]);
        s.in_lds = ks[p] * d <= ctx->km_lds_centers ? 1u : 0u;
        const double *init = a->init ? a->init[p] : nullptr;
        if (init) {
            s.seeded = 1u;
            for (uint32_t j = 0; j < ks[p]; j++)
                for (uint32_t t = 0; t < d; t++) {
                    CR_REQUIRE(ctx, std::isfinite(init[(size_t)j * d + t]), CRGPU_EINVAL, "crgpu_kmeans_dev: init[%u, %u] of K = %u is not finite", j, t, ks[p]);
                    cen_h[(size_t)p * kd_max + (size_t)j * d + t] = init[(size_t)j * d + t] - mean[t];
                }
            continue;
        }
        McMt g(a->seed);  // the first double, and with it the first cell, is the same for every K
        for (uint32_t i = 0; i < 1u + (ks[p] - 1u) * s.n_trials; i++) draws[(size_t)p * u_stride + i] = g.random_sample();
        if (!have_first) first_cell = km_first_cell(n, draws[(size_t)p * u_stride]), have_first = true;
        s.chosen[0] = (uint32_t)first_cell;
        seed_rounds = std::max(seed_rounds, ks[p]);
    }

    DevBuf x_b, xc_b, xx_b, mean_b, st_b, u_b, cen_b, cc_b, lab_b, close_b, seg_b, sup_b, cslab_b, slab_b, slab2_b, sums_b, fslab_b, fout_b;
    CR_TRY(dmalloc(ctx, x_b, n * ld * sizeof(double)));
    CR_TRY(dmalloc(ctx, xc_b, n * d * sizeof(double)));
    CR_TRY(dmalloc(ctx, xx_b, n * sizeof(double)));
    CR_TRY(dmalloc(ctx, mean_b, d * sizeof(double)));
    CR_TRY(dmalloc(ctx, st_b, n_ks * sizeof(KmState)));
    CR_TRY(dmalloc(ctx, u_b, draws.size() * sizeof(double)));
    CR_TRY(dmalloc(ctx, cen_b, cen_h.size() * sizeof(double)));
    CR_TRY(dmalloc(ctx, cc_b, (uint64_t)n_ks * KM_MAXK * sizeof(double)));
    CR_TRY(dmalloc(ctx, lab_b, (uint64_t)n_ks * n * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, close_b, (uint64_t)n_ks * n * sizeof(double)));
    CR_TRY(dmalloc(ctx, seg_b, (uint64_t)n_ks * n_seg * sizeof(double)));
    CR_TRY(dmalloc(ctx, sup_b, (uint64_t)n_ks * n_sup * sizeof(double)));
    CR_TRY(dmalloc(ctx, cslab_b, (uint64_t)n_ks * n_tiles * KM_MAXT * sizeof(double)));
    CR_TRY(dmalloc(ctx, slab_b, (uint64_t)n_ks * n_tiles * n_stat_max * sizeof(double)));
    CR_TRY(dmalloc(ctx, slab2_b, (uint64_t)n_ks * n_groups * n_stat_max * sizeof(double)));
    CR_TRY(dmalloc(ctx, sums_b, (uint64_t)n_ks * n_stat_max * sizeof(double)));
    CR_TRY(dmalloc(ctx, fslab_b, (uint64_t)n_ks * n_tiles * fw * sizeof(double)));
    CR_TRY(dmalloc(ctx, fout_b, (uint64_t)n_ks * fw * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, x_b.p, x, ((n - 1) * ld + d) * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, mean_b.p, mean.data(), d * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, st_b.p, h.data(), n_ks * sizeof(KmState)));
    CR_TRY(crgpu_memcpy_h2d(ctx, u_b.p, draws.data(), draws.size() * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, cen_b.p, cen_h.data(), cen_h.size() * sizeof(double)));
    CR_HIP(ctx, hipMemsetAsync(lab_b.p, 0xFF, (uint64_t)n_ks * n * sizeof(int32_t), ctx->stream));  // labels_old = -1
    KmState *d_st = st_b.as<KmState>();
    const double *d_xc = xc_b.as<double>(), *d_xx = xx_b.as<double>();
    double *d_cen = cen_b.as<double>(), *d_cc = cc_b.as<double>();

    {
        CrTimer t(ctx, CRGPU_T_MATRIX, n * d);
        hipLaunchKernelGGL(k_km_center, dim3(n_tiles), dim3(KM_WG), 0, ctx->stream, x_b.as<double>(), n32, d, ld, mean_b.as<double>(), xc_b.as<double>(),
                           xx_b.as<double>());
        for (uint32_t c = 1; c < seed_rounds; c++) {
            hipLaunchKernelGGL(k_km_seed_update, dim3(n_tiles, n_ks), dim3(KM_WG), 0, ctx->stream, d_xc, d_xx, n32, d, d_st, c, close_b.as<double>(),
                               seg_b.as<double>(), n_seg);
            hipLaunchKernelGGL(k_km_seed_super, dim3((n_sup + KM_WG - 1u) / KM_WG, n_ks), dim3(KM_WG), 0, ctx->stream, d_st, c, seg_b.as<double>(), n_seg,
                               sup_b.as<double>(), n_sup);
            hipLaunchKernelGGL(k_km_seed_locate, dim3(n_ks), dim3(64), 0, ctx->stream, d_st, c, u_b.as<double>(), u_stride, close_b.as<double>(),
                               seg_b.as<double>(), sup_b.as<double>(), n32, n_seg, n_sup);
            hipLaunchKernelGGL(k_km_seed_cand, dim3(n_tiles, n_ks), dim3(KM_WG), 0, ctx->stream, d_xc, d_xx, n32, d, d_st, c, close_b.as<double>(),
                               cslab_b.as<double>(), n_tiles);
            hipLaunchKernelGGL(k_km_seed_pick, dim3(n_ks), dim3(64), 0, ctx->stream, d_st, c, cslab_b.as<double>(), n_tiles);
        }
        hipLaunchKernelGGL(k_km_seed_centres, dim3(k_max, n_ks), dim3(KM_WG), 0, ctx->stream, d_xc, d, d_st, d_cen, d_cc, kd_max);
        CR_HIP(ctx, hipGetLastError());
    }

    // LDS of the assign pass: the centres and norms of the largest position that keeps them there, the tile's rows up to KM_TILE_D
    const bool tile = d <= KM_TILE_D;
    uint32_t lds_centres = 0;
    for (uint32_t p = 0; p < n_ks; p++)
        if (h[p].in_lds) lds_centres = std::max(lds_centres, ks[p] * d);
    const size_t dyn = ((size_t)lds_centres + KM_MAXK + (tile ? (size_t)KM_WG * d : 0u)) * sizeof(double);
    const uint32_t batch = ctx->km_batch ? ctx->km_batch : 8u;
    std::vector<double> dist, sums(n_stat_max);
    std::vector<int32_t> lab;
    uint64_t rounds = 0;
    while (true) {
        {
            CrTimer t(ctx, CRGPU_T_MATRIX, (uint64_t)batch * n * d);
            for (uint32_t b = 0; b < batch && rounds < a->max_iter; b++, rounds++) {
                km_launch_assign(ctx, tile, n_tiles, dyn, d_xc, n32, d, d_st, n_ks, d_cen, d_cc, kd_max, lab_b.as<int32_t>(), slab_b.as<double>(), n_stat_max,
                                 lds_centres, 0u);
                hipLaunchKernelGGL(k_km_reduce, dim3(n_groups, n_ks), dim3(KM_WG), 0, ctx->stream, d_st, d, slab_b.as<double>(), n_tiles, n_stat_max,
                                   slab2_b.as<double>(), n_groups);
                hipLaunchKernelGGL(k_km_close_a, dim3(n_ks), dim3(KM_WG), 0, ctx->stream, d_st, d, slab2_b.as<double>(), n_groups, n_stat_max,
                                   sums_b.as<double>());
                hipLaunchKernelGGL(k_km_close_b, dim3(n_ks), dim3(KM_WG), 0, ctx->stream, d_st, d, sums_b.as<double>(), n_stat_max, d_cen, d_cc, kd_max,
                                   a->max_iter, NONE32);
            }
            CR_HIP(ctx, hipGetLastError());
        }
        CR_TRY(crgpu_memcpy_d2h(ctx, h.data(), d_st, n_ks * sizeof(KmState)));  // the latches: the one synchronisation of a batch
        bool all = true, parked = false;
        for (uint32_t p = 0; p < n_ks; p++) {
            if (h[p].paused) {  // _relocate_empty_clusters_dense on the host, then this position's k_km_close_b
                parked = true;
                const uint32_t K = ks[p], kd = K * d;
                hipLaunchKernelGGL(k_km_own_dist, dim3(n_tiles), dim3(KM_WG), 0, ctx->stream, d_xc, n32, d, d_cen + (size_t)p * kd_max,
                                   lab_b.as<int32_t>() + (size_t)p * n, close_b.as<double>());
                CR_HIP(ctx, hipGetLastError());
                dist.resize(n), lab.resize(n);
                CR_TRY(crgpu_memcpy_d2h(ctx, dist.data(), close_b.p, n * sizeof(double)));
                CR_TRY(crgpu_memcpy_d2h(ctx, lab.data(), lab_b.as<int32_t>() + (size_t)p * n, n * sizeof(int32_t)));
                CR_TRY(crgpu_memcpy_d2h(ctx, sums.data(), sums_b.as<double>() + (size_t)p * n_stat_max, (size_t)(kd + K) * sizeof(double)));
                std::vector<uint32_t> empty, far(n);
                for (uint32_t j = 0; j < K; j++)
                    if (sums[kd + j] == 0.0) empty.push_back(j);
                for (uint32_t i = 0; i < n32; i++) far[i] = i;
                const size_t ne = std::min<size_t>(empty.size(), n);
                std::partial_sort(far.begin(), far.begin() + ne, far.end(),
                                  [&](uint32_t l, uint32_t r) { return dist[l] > dist[r] || (dist[l] == dist[r] && l > r); });
                uint32_t moved = 0;
                if (ne && dist[far[0]] != 0.0) {
                    for (size_t e = 0; e < ne; e++) {
                        const uint32_t nw = empty[e], fi = far[e], old = (uint32_t)lab[fi];
                        for (uint32_t t = 0; t < d; t++) {
                            const double v = x[(uint64_t)fi * ld + t] - mean[t];
                            sums[(size_t)old * d + t] -= v;
                            sums[(size_t)nw * d + t] = v;
                        }
                        sums[kd + nw] = 1.0, sums[kd + old] -= 1.0;
                        moved++;
                    }
                    CR_TRY(crgpu_memcpy_h2d(ctx, sums_b.as<double>() + (size_t)p * n_stat_max, sums.data(), (size_t)(kd + K) * sizeof(double)));
                }
                hipLaunchKernelGGL(k_km_resume, dim3(1), dim3(1), 0, ctx->stream, d_st, p, moved);
                hipLaunchKernelGGL(k_km_close_b, dim3(n_ks), dim3(KM_WG), 0, ctx->stream, d_st, d, sums_b.as<double>(), n_stat_max, d_cen, d_cc, kd_max,
                                   a->max_iter, p);
                CR_HIP(ctx, hipGetLastError());
            }
            if (!h[p].stopped) all = false;
        }
        if (parked) {
            CR_TRY(crgpu_memcpy_d2h(ctx, h.data(), d_st, n_ks * sizeof(KmState)));
            all = true;
            for (uint32_t p = 0; p < n_ks; p++) all = all && h[p].stopped;
        }
        if (all) break;
        // a parked position loses the rest of its batch, so the rounds enqueued are no count of any position's own
        uint32_t least = a->max_iter;
        for (uint32_t p = 0; p < n_ks; p++)
            if (!h[p].stopped) least = std::min(least, h[p].round);
        rounds = least;
        CR_REQUIRE(ctx, rounds < a->max_iter, CRGPU_EHIP, "crgpu_kmeans_dev: no stop after %u rounds", a->max_iter);
    }

    {
        CrTimer t(ctx, CRGPU_T_MATRIX, n * d);
        km_launch_assign(ctx, tile, n_tiles, dyn, d_xc, n32, d, d_st, n_ks, d_cen, d_cc, kd_max, lab_b.as<int32_t>(), slab_b.as<double>(), n_stat_max, lds_centres,
                         1u);
        hipLaunchKernelGGL(k_km_final, dim3(n_tiles, n_ks), dim3(KM_WG), 0, ctx->stream, x_b.as<double>(), ld, d_xc, n32, d, mean_b.as<double>(), d_st, d_cen,
                           kd_max, lab_b.as<int32_t>(), fslab_b.as<double>(), n_tiles);
        hipLaunchKernelGGL(k_km_final_close, dim3(n_ks), dim3(KM_WG), 0, ctx->stream, d_st, fslab_b.as<double>(), n_tiles, fout_b.as<double>());
        CR_HIP(ctx, hipGetLastError());
    }
    std::vector<double> fout((size_t)n_ks * fw);
    CR_TRY(crgpu_memcpy_d2h(ctx, fout.data(), fout_b.p, fout.size() * sizeof(double)));
    CR_TRY(crgpu_memcpy_d2h(ctx, cen_h.data(), cen_b.p, cen_h.size() * sizeof(double)));
    const double ms = cr_ms_since(t0);
    for (uint32_t p = 0; p < n_ks; p++) {
        crgpu_kmeans_result &r = res[p];
        const uint32_t K = ks[p];
        const double *f = fout.data() + (size_t)p * fw;
        double centers[KM_MAXK * KM_MAXD], wss[KM_MAXK];
        uint64_t sizes[KM_MAXK];
        for (uint32_t j = 0; j < K; j++) {
            wss[j] = f[j], sizes[j] = (uint64_t)f[KM_MAXK + j];
            for (uint32_t t = 0; t < d; t++) centers[(size_t)j * d + t] = cen_h[(size_t)p * kd_max + (size_t)j * d + t] + mean[t];
        }
        r.inertia = f[2u * KM_MAXK], r.fit_ms = ms;
        r.n_iter = h[p].n_iter, r.strict = h[p].strict, r.relocations = h[p].relocs, r.in_lds = h[p].in_lds;
        CR_REQUIRE(ctx, crgpu_kmeans_db_index(K, d, centers, wss, sizes, &r.db_score) == CRGPU_OK, CRGPU_EHIP, "crgpu_kmeans_dev: no score for K = %u", K);
        if (r.centers_out) std::copy(centers, centers + (size_t)K * d, r.centers_out);
        if (r.wss_out) std::copy(wss, wss + K, r.wss_out);
        if (r.sizes_out) std::copy(sizes, sizes + K, r.sizes_out);
        if (r.labels_out || r.clusters_out) {
            lab.resize(n);
            CR_TRY(crgpu_memcpy_d2h(ctx, lab.data(), lab_b.as<int32_t>() + (size_t)p * n, n * sizeof(int32_t)));
            if (r.labels_out) std::copy(lab.begin(), lab.end(), r.labels_out);
            if (r.clusters_out) km_relabel(lab.data(), n, K, sizes, r.clusters_out);
        }
    }
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRGPU_OK;
}
