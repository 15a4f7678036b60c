// merge_clusters.hip -- the medoids and the dendrogram of MERGE_CLUSTERS (mro/rna/stages/analyzer/merge_clusters/__init__.py).
//
// join() of the stage computes, in every round of its loop, the per-cluster median of every principal component
// (pca_df.groupby("cluster").apply(lambda x: x.median(axis=0))) and scipy's linkage(medoids, "complete"), and then tests the sibling
// leaves with a local sSeq comparison (sseq_pair.h).  This unit holds the first two.
//
// crgpu_cluster_medians_dev   the host sorts the rows by label (a counting sort) and uploads them one dimension after the other, so that
//                             the values of (cluster c, dimension t) are one contiguous segment.  k_mc_median: a workgroup per segment
//                             selects the element of a rank by a most-significant-byte-first radix select over the order-preserving u64
//                             image of the doubles: eight passes, each a 256-bin histogram in LDS of the elements that share the prefix
//                             found so far (integer LDS atomics), then the bin that holds the rank.  An odd size takes rank n / 2, an
//                             even size the ranks n / 2 - 1 and n / 2 and (lo + hi) / 2.  An exact selection: no tolerance, no order of
//                             summation, no floating-point atomic.
// crgpu_linkage_complete      host only.  The greedy agglomeration on the full distance matrix; the Lance-Williams update of complete
//                             linkage is max(d(a, j), d(b, j)), so a height is always one of the input distances.  Every cluster keeps
//                             its nearest neighbour by the key (distance, smaller id, larger id); a merge only raises distances, so a
//                             cached neighbour is recomputed only when it was one of the two merged clusters.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"

#define MC_WG 256u

// the u64 whose unsigned order is the order of the doubles (-0 below +0)
__host__ __device__ __forceinline__ uint64_t mc_key(double v) {
    union { double d; uint64_t u; } c;
    c.d = v;
    return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull);
}
__host__ __device__ __forceinline__ double mc_value(uint64_t k) {
    union { double d; uint64_t u; } c;
    c.u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    return c.d;
}

// the key of the element of rank `rank` (0-based, ascending) among x[0 .. n); s_hist: 256 words, s_pick: 2 words of LDS
__device__ uint64_t mc_select(const double *__restrict__ x, uint32_t n, uint32_t rank, uint32_t *s_hist, uint32_t *s_pick) {
    const uint32_t tid = threadIdx.x;
    uint64_t prefix = 0ull;
    for (uint32_t pass = 0; pass < 8u; pass++) {
        const uint32_t shift = 56u - 8u * pass;
        const uint64_t above = pass ? ~0ull << (shift + 8u) : 0ull;  // the bytes fixed so far
        s_hist[tid] = 0u;
        __syncthreads();
        for (uint32_t i = tid; i < n; i += MC_WG) {
            const uint64_t k = mc_key(x[i]);
            if ((k & above) == prefix) atomicAdd(&s_hist[(uint32_t)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0u) {
            uint32_t run = 0u, b = 0u;
            for (; b < 255u && rank >= run + s_hist[b]; b++) run += s_hist[b];
            s_pick[0] = b, s_pick[1] = rank - run;
        }
        __syncthreads();
        prefix |= (uint64_t)s_pick[0] << shift;
        rank = s_pick[1];
        __syncthreads();
    }
    return prefix;
}

// xs: [d][n] the rows sorted by label, start[c] .. start[c + 1] the rows of cluster c; block (c, t)
__global__ __launch_bounds__(MC_WG) void k_mc_median(const double *__restrict__ xs, uint64_t n, const uint32_t *__restrict__ start, uint32_t d,
                                                     double *__restrict__ med) {
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_pick[2];
    const uint32_t c = blockIdx.x, t = blockIdx.y;
    const uint32_t lo = start[c], cnt = start[c + 1u] - lo;
    const double *x = xs + (size_t)t * n + lo;
    const double hi_v = mc_value(mc_select(x, cnt, cnt / 2u, s_hist, s_pick));
    double m = hi_v;
    if (cnt % 2u == 0u) {
        const double lo_v = mc_value(mc_select(x, cnt, cnt / 2u - 1u, s_hist, s_pick));
        m = (lo_v + hi_v) / 2.0;
    }
    if (threadIdx.x == 0u) med[(size_t)c * d + t] = m;
}

extern "C" int crgpu_cluster_medians_dev(crgpu_ctx *ctx, const double *x, uint64_t n, uint32_t d, uint64_t ld, const int32_t *labels, uint32_t K,
                                         double *medians_out, uint64_t *sizes_out) {
    if (!ctx || !x || !labels || !medians_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    // every refusal comes before the device is touched
    CR_REQUIRE(ctx, n >= 1 && n < (1ull << 31), CRGPU_EINVAL, "crgpu_cluster_medians_dev: %llu rows, 1 to 2^31 - 1", (unsigned long long)n);
    CR_REQUIRE(ctx, d >= 1 && d <= CRGPU_KM_MAX_D && ld >= d, CRGPU_EINVAL, "crgpu_cluster_medians_dev: %u dimensions (1 to %u) in rows of %llu", d,
               CRGPU_KM_MAX_D, (unsigned long long)ld);
    CR_REQUIRE(ctx, K >= 1 && K <= CRGPU_SSEQ_MAX_K, CRGPU_EINVAL, "crgpu_cluster_medians_dev: %u clusters, 1 to %u", K, CRGPU_SSEQ_MAX_K);
    std::vector<uint32_t> start(K + 1u, 0);
    for (uint64_t i = 0; i < n; i++) {
        CR_REQUIRE(ctx, labels[i] >= 0 && (uint32_t)labels[i] < K, CRGPU_EINVAL, "crgpu_cluster_medians_dev: label %d of row %llu, 0 to %u", labels[i],
                   (unsigned long long)i, K - 1u);
        start[labels[i] + 1]++;
    }
    for (uint32_t c = 0; c < K; c++) {
        CR_REQUIRE(ctx, start[c + 1u] > 0, CRGPU_EINVAL, "crgpu_cluster_medians_dev: cluster %u is empty", c);
        start[c + 1u] += start[c];
    }
    std::vector<double> xs((size_t)d * n);
    std::vector<uint32_t> next(start.begin(), start.end() - 1);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t p = next[labels[i]]++;
        for (uint32_t t = 0; t < d; t++) {
            const double v = x[i * ld + t];
            CR_REQUIRE(ctx, std::isfinite(v), CRGPU_EINVAL, "crgpu_cluster_medians_dev: row %llu, dimension %u is not finite", (unsigned long long)i, t);
            xs[(size_t)t * n + p] = v;
        }
    }

    DevBuf xs_b, start_b, med_b;
    CR_TRY(dmalloc(ctx, xs_b, xs.size() * sizeof(double)));
    CR_TRY(dmalloc(ctx, start_b, (K + 1ull) * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, med_b, (size_t)K * d * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, xs_b.p, xs.data(), xs.size() * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, start_b.p, start.data(), (K + 1ull) * sizeof(uint32_t)));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, (uint64_t)n * d);
        hipLaunchKernelGGL(k_mc_median, dim3(K, d), dim3(MC_WG), 0, ctx->stream, xs_b.as<double>(), n, start_b.as<uint32_t>(), d, med_b.as<double>());
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(crgpu_memcpy_d2h(ctx, medians_out, med_b.p, (size_t)K * d * sizeof(double)));
    if (sizes_out)
        for (uint32_t c = 0; c < K; c++) sizes_out[c] = start[c + 1u] - start[c];
    return CRGPU_OK;
}

// ---- host: scipy's linkage(points, "complete") -------------------------------------------------------------------------------------------
namespace {
struct McKey {  // the order in which pairs are merged
    double h;
    uint32_t id0, id1;
    bool operator<(const McKey &o) const { return h < o.h || (h == o.h && (id0 < o.id0 || (id0 == o.id0 && id1 < o.id1))); }
};
}  // namespace

extern "C" int crgpu_linkage_complete(const double *pts, uint32_t K, uint32_t d, double *Z) {
    if (!pts || !Z || K < 2 || K > CRGPU_SSEQ_MAX_K || d < 1) return CRGPU_EINVAL;
    for (size_t i = 0; i < (size_t)K * d; i++)
        if (!std::isfinite(pts[i])) return CRGPU_EINVAL;
    std::vector<double> D((size_t)K * K, 0.0);
    for (uint32_t i = 0; i < K; i++)
        for (uint32_t j = i + 1u; j < K; j++) {
            double s = 0.0;
            for (uint32_t t = 0; t < d; t++) {
                const double e = pts[(size_t)i * d + t] - pts[(size_t)j * d + t];
                s += e * e;
            }
            D[(size_t)i * K + j] = D[(size_t)j * K + i] = std::sqrt(s);
        }
    std::vector<uint32_t> id(K), size(K, 1u), nn(K, 0u);
    std::vector<uint8_t> live(K, 1);
    for (uint32_t i = 0; i < K; i++) id[i] = i;
    auto key = [&](uint32_t i, uint32_t j) { return McKey{D[(size_t)i * K + j], std::min(id[i], id[j]), std::max(id[i], id[j])}; };
    auto nearest = [&](uint32_t i) {  // some other live slot exists
        uint32_t best = K;
        for (uint32_t j = 0; j < K; j++)
            if (live[j] && j != i && (best == K || key(i, j) < key(i, best))) best = j;
        nn[i] = best;
    };
    for (uint32_t i = 0; i < K; i++) nearest(i);
    for (uint32_t step = 0; step + 1u < K; step++) {
        uint32_t a = K;
        for (uint32_t i = 0; i < K; i++)
            if (live[i] && (a == K || key(i, nn[i]) < key(a, nn[a]))) a = i;
        uint32_t b = nn[a];
        if (id[b] < id[a]) std::swap(a, b);
        double *z = Z + (size_t)step * 4u;
        z[0] = (double)id[a], z[1] = (double)id[b], z[2] = D[(size_t)a * K + b], z[3] = (double)(size[a] + size[b]);
        // the new cluster takes slot a
        live[b] = 0;
        size[a] += size[b], id[a] = K + step;
        for (uint32_t j = 0; j < K; j++)
            if (live[j] && j != a) {
                const double m = std::max(D[(size_t)a * K + j], D[(size_t)b * K + j]);
                D[(size_t)a * K + j] = D[(size_t)j * K + a] = m;
            }
        if (step + 2u < K) {
            nearest(a);
            for (uint32_t j = 0; j < K; j++)
                if (live[j] && j != a && (nn[j] == a || nn[j] == b)) nearest(j);
        }
    }
    return CRGPU_OK;
}
