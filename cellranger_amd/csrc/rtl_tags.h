// rtl_tags.h -- multiplexed Flex (RTL) wells: the tag of every barcode, the columns of every sample, the gel-bead overlap of the probe
// barcodes and the GEM occupancy on the device (part of matrix_stages.hip).
//
// Replaces CALL_TAGS_RTL (lib/rust/cr_lib/src/stages/call_tags_rtl.rs:143-498 with barcode_overlap.rs and
// read_level_multiplexing.rs:22-68) and remove_bcs_from_high_occupancy_gems (lib/python/cellranger/cell_calling_helpers.py:315-424,
// without its read fractions).  The threshold simulation (:273-312) stays on the host: numpy's legacy poisson is serial.
//
// A column of canonical rank r belongs to GEM g = r / n_probe and carries probe rank p = r % n_probe (n_probe = the size of the
// construct's last segment); columns ascend by rank, so the barcodes of one GEM are adjacent columns: a RUN.  Nothing here sorts
// the matrix.  Everything reported is an integer summed with integer atomics (LDS first, one global atomic per workgroup and
// table cell), or an f64 quotient of two such integers taken on the host: no result depends on the order of arrival.
#pragma once

#include <algorithm>
#include <cmath>

#include "stage_common.h"

#define RT_MAX_TAGS CRGPU_RTL_MAX_TAGS
#define RT_MAX_PROBES CRGPU_RTL_MAX_PROBES
#define RT_MAX_TYPES CRGPU_RTL_MAX_TYPES
#define RT_NONE 0xFFu

// the probe segment of the context's construct
static int rt_n_probe(crgpu_ctx *ctx, const char *who, uint32_t *n_probe) {
    CR_REQUIRE(ctx, ctx->n_segments >= 2, CRGPU_ESTATE, "%s: the barcode construct has no probe segment (crgpu_set_barcode_segments)", who);
    const uint32_t n = ctx->seg_n[ctx->n_segments - 1];
    CR_REQUIRE(ctx, n >= 1 && n <= RT_MAX_PROBES, CRGPU_ERANGE, "%s: %u probe barcodes, at most %d", who, n, RT_MAX_PROBES);
    *n_probe = n;
    return CRGPU_OK;
}
// a host table of n <= cap bytes as cap device bytes, the rest RT_NONE
static int rt_upload_table(crgpu_ctx *ctx, DevBuf &b, const uint8_t *h, uint32_t n, uint32_t cap) {
    uint8_t tab[RT_MAX_PROBES];
    memset(tab, 0xFF, sizeof(tab));
    if (n) memcpy(tab, h, n);
    CR_TRY(dmalloc(ctx, b, cap));
    CR_TRY(crgpu_memcpy_h2d(ctx, b.p, tab, cap));
    return hipStreamSynchronize(ctx->stream) == hipSuccess ? CRGPU_OK : cr_fail(ctx, CRGPU_EHIP, "rtl tags: table upload failed");  // (tab is on the stack)
}

// ---- 1. the tag of every column, barcodes and UMIs per tag ----------------------------------------------------------------------
// flag: a column whose probe rank is not on the map
__global__ __launch_bounds__(256) void k_rt_tags(const uint32_t *__restrict__ rank, uint64_t V, uint32_t n_probe,
                                                 const uint8_t *__restrict__ tag_of_probe, uint32_t n_tags, uint8_t *__restrict__ tags,
                                                 unsigned long long *__restrict__ per_tag, uint32_t *__restrict__ flag) {
    __shared__ uint8_t s_tag[RT_MAX_PROBES];
    __shared__ uint32_t s_cnt[RT_MAX_TAGS];
    s_tag[threadIdx.x] = tag_of_probe[threadIdx.x];
    if (threadIdx.x < RT_MAX_TAGS) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < V; c += stride) {
        const uint32_t t = s_tag[rank[c] % n_probe];
        tags[c] = (uint8_t)t;
        if (t < n_tags) atomicAdd(&s_cnt[t], 1u); else *flag = 1u;
    }
    __syncthreads();
    if (threadIdx.x < n_tags && s_cnt[threadIdx.x]) atomicAdd(&per_tag[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}

// one wave per column: every lane keeps one 64-bit sum per feature type (static indices: no scratch), the wave adds them up, lane 0
// adds the wave's sum to the workgroup's LDS table, the workgroup flushes its non-zero cells.  flag: a row >= n_features
__global__ __launch_bounds__(256) void k_rt_umi(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                const int32_t *__restrict__ data, uint64_t V, const uint8_t *__restrict__ tags,
                                                const uint8_t *__restrict__ ftype, uint32_t n_features, uint32_t n_types, uint32_t n_tags,
                                                unsigned long long *__restrict__ umi, uint32_t *__restrict__ flag) {
    __shared__ unsigned long long s_umi[RT_MAX_TYPES * RT_MAX_TAGS];
    for (uint32_t i = threadIdx.x; i < RT_MAX_TYPES * RT_MAX_TAGS; i += 256) s_umi[i] = 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave0; c < V; c += n_waves) {  // uniform in the wave
        const long long s = indptr[c], e = indptr[c + 1];
        const uint32_t t = tags[c];
        if (s >= e || t >= n_tags) continue;
        unsigned long long acc[RT_MAX_TYPES] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (long long i = s + lane; i < e; i += 64) {
            const uint32_t f = (uint32_t)indices[i];
            if (f >= n_features) {
                *flag = 1u;
                continue;
            }
            const uint32_t ft = ftype[f], d = (uint32_t)data[i];
#pragma unroll
            for (int ty = 0; ty < RT_MAX_TYPES; ty++) acc[ty] += ft == (uint32_t)ty ? d : 0u;
        }
#pragma unroll
        for (int ty = 0; ty < RT_MAX_TYPES; ty++) {
            if ((uint32_t)ty >= n_types || !__ballot(acc[ty] != 0ull)) continue;  // uniform
            const unsigned long long w = wave_sum(acc[ty]);
            if (lane == 0) atomicAdd(&s_umi[ty * RT_MAX_TAGS + t], w);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < RT_MAX_TYPES * RT_MAX_TAGS; i += 256)
        if (s_umi[i]) atomicAdd(&umi[i], s_umi[i]);
}

extern "C" int crgpu_rtl_tags_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint8_t *tag_of_probe, uint32_t n_tags,
                                  const uint8_t *feature_type, uint32_t n_features, uint32_t n_types, uint8_t *d_tags_out,
                                  uint64_t *barcodes_per_tag_out, uint64_t *umi_per_tag_out) {
    if (!ctx || !m) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    uint32_t n_probe = 0;
    CR_TRY(rt_n_probe(ctx, "crgpu_rtl_tags_dev", &n_probe));
    CR_REQUIRE(ctx, n_tags >= 1 && n_tags <= RT_MAX_TAGS, CRGPU_ERANGE, "crgpu_rtl_tags_dev: 1 .. %d tags", RT_MAX_TAGS);
    CR_REQUIRE(ctx, n_types <= RT_MAX_TYPES, CRGPU_ERANGE, "crgpu_rtl_tags_dev: at most %d feature types", RT_MAX_TYPES);
    CR_REQUIRE(ctx, tag_of_probe && barcodes_per_tag_out, CRGPU_EINVAL, "crgpu_rtl_tags_dev: NULL tag_of_probe or barcodes_per_tag_out");
    CR_REQUIRE(ctx, !n_types || (umi_per_tag_out && (feature_type || !n_features)), CRGPU_EINVAL,
               "crgpu_rtl_tags_dev: feature types without feature_type or umi_per_tag_out");
    for (uint32_t p = 0; p < n_probe; p++)
        CR_REQUIRE(ctx, tag_of_probe[p] < n_tags || tag_of_probe[p] == RT_NONE, CRGPU_EINVAL, "crgpu_rtl_tags_dev: tag_of_probe[%u] = %u with %u tags", p,
                   tag_of_probe[p], n_tags);
    for (uint32_t f = 0; n_types && f < n_features; f++)
        CR_REQUIRE(ctx, feature_type[f] < n_types || feature_type[f] == RT_NONE, CRGPU_EINVAL, "crgpu_rtl_tags_dev: feature_type[%u] = %u with %u types",
                   f, feature_type[f], n_types);
    memset(barcodes_per_tag_out, 0, n_tags * sizeof(uint64_t));
    if (n_types) memset(umi_per_tag_out, 0, (size_t)n_types * n_tags * sizeof(uint64_t));
    const uint64_t V = m->n_barcodes;
    if (!V) return CRGPU_OK;
    CR_REQUIRE(ctx, d_tags_out != nullptr, CRGPU_EINVAL, "crgpu_rtl_tags_dev: NULL d_tags_out");
    DevBuf top_b, out_b, ft_b;
    CR_TRY(rt_upload_table(ctx, top_b, tag_of_probe, n_probe, RT_MAX_PROBES));
    const uint32_t n_out = RT_MAX_TAGS + RT_MAX_TYPES * RT_MAX_TAGS;
    CR_TRY(dmalloc(ctx, out_b, n_out * sizeof(unsigned long long)));
    CR_HIP(ctx, hipMemsetAsync(out_b.p, 0, n_out * sizeof(unsigned long long), ctx->stream));
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag[2] = {0, 0};
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, 2 * sizeof(uint32_t), ctx->stream));
    unsigned long long *d_out = out_b.as<unsigned long long>();
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, V);
        hipLaunchKernelGGL(k_rt_tags, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, m->d_barcode_rank, V, n_probe, top_b.as<uint8_t>(), n_tags,
                           d_tags_out, d_out, d_flag);
        CR_HIP(ctx, hipGetLastError());
    }
    if (n_types && m->nnz) {
        CR_TRY(dmalloc(ctx, ft_b, n_features ? n_features : 1));
        if (n_features) CR_TRY(crgpu_memcpy_h2d(ctx, ft_b.p, feature_type, n_features));
        CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
        hipLaunchKernelGGL(k_rt_umi, dim3(cr_grid(V * 64, 256)), dim3(256), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data, V,
                           d_tags_out, ft_b.as<uint8_t>(), n_features, n_types, n_tags, d_out + RT_MAX_TAGS, d_flag + 1);
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(crgpu_memcpy_d2h(ctx, flag, d_flag, sizeof(flag)));
    CR_REQUIRE(ctx, !flag[0], CRGPU_EINVAL, "crgpu_rtl_tags_dev: a column carries a probe barcode that is not on the map");
    CR_REQUIRE(ctx, !flag[1], CRGPU_EINVAL, "crgpu_rtl_tags_dev: the matrix holds a row >= n_features (%u)", n_features);
    std::vector<uint64_t> h(n_out);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
    CR_TRY(crgpu_memcpy_d2h(ctx, h.data(), d_out, n_out * sizeof(uint64_t)));
    std::copy(h.begin(), h.begin() + n_tags, barcodes_per_tag_out);
    for (uint32_t ty = 0; ty < n_types; ty++)
        std::copy(h.begin() + RT_MAX_TAGS + ty * RT_MAX_TAGS, h.begin() + RT_MAX_TAGS + ty * RT_MAX_TAGS + n_tags, umi_per_tag_out + (size_t)ty * n_tags);
    return CRGPU_OK;
}

// ---- 2. the columns of every sample: a stable split by the sample of the tag ---------------------------------------------------
// key[i] = the sample of column cols[i] (cols == NULL: column i), n_samples for a column without one; counts[s] = columns per key
__global__ __launch_bounds__(256) void k_rt_sample_keys(const uint8_t *__restrict__ tags, uint64_t V, const uint64_t *__restrict__ cols, uint64_t n,
                                                        const uint8_t *__restrict__ sample_of_tag, uint32_t n_samples, uint32_t *__restrict__ key,
                                                        uint32_t *__restrict__ val, unsigned long long *__restrict__ counts,
                                                        uint32_t *__restrict__ flag) {
    __shared__ uint8_t s_sot[RT_MAX_TAGS];
    __shared__ uint32_t s_cnt[256];
    if (threadIdx.x < RT_MAX_TAGS) s_sot[threadIdx.x] = sample_of_tag[threadIdx.x];
    s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t c = cols ? cols[i] : i;
        uint32_t s = n_samples;
        if (c < V) {
            const uint32_t t = tags[c];
            if (t < RT_MAX_TAGS && s_sot[t] < n_samples) s = s_sot[t];
        } else {
            *flag = 1u;
        }
        key[i] = s;
        val[i] = (uint32_t)c;
        atomicAdd(&s_cnt[s], 1u);
    }
    __syncthreads();
    if (threadIdx.x <= n_samples && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}
__global__ __launch_bounds__(256) void k_rt_widen(const uint32_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = in[i];
}

extern "C" int crgpu_rtl_sample_columns_dev(crgpu_ctx *ctx, const uint8_t *d_tags, uint64_t V, const uint8_t *sample_of_tag, uint32_t n_tags,
                                            uint32_t n_samples, int restricted, const uint64_t *d_cols, uint64_t n_cols,
                                            uint64_t **d_cols_out, uint64_t *offsets_out) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, d_cols_out && offsets_out && sample_of_tag, CRGPU_EINVAL, "crgpu_rtl_sample_columns_dev: NULL argument");
    *d_cols_out = nullptr;
    CR_REQUIRE(ctx, n_tags >= 1 && n_tags <= RT_MAX_TAGS, CRGPU_ERANGE, "crgpu_rtl_sample_columns_dev: 1 .. %d tags", RT_MAX_TAGS);
    CR_REQUIRE(ctx, n_samples >= 1 && n_samples <= 255, CRGPU_ERANGE, "crgpu_rtl_sample_columns_dev: 1 .. 255 samples");
    CR_REQUIRE(ctx, V < 0xFFFFFFFFull, CRGPU_ERANGE, "crgpu_rtl_sample_columns_dev: fewer than 2^32 - 1 columns");
    for (uint32_t t = 0; t < n_tags; t++)
        CR_REQUIRE(ctx, sample_of_tag[t] < n_samples || sample_of_tag[t] == RT_NONE, CRGPU_EINVAL, "crgpu_rtl_sample_columns_dev: sample_of_tag[%u] = %u with %u samples",
                   t, sample_of_tag[t], n_samples);
    CR_REQUIRE(ctx, !restricted || d_cols || !n_cols, CRGPU_EINVAL, "crgpu_rtl_sample_columns_dev: restricted to a NULL column list");
    const uint64_t n = restricted ? n_cols : V;
    if (!restricted) d_cols = nullptr;
    CR_REQUIRE(ctx, n <= V, CRGPU_EINVAL, "crgpu_rtl_sample_columns_dev: more columns listed than the matrix has");
    memset(offsets_out, 0, (n_samples + 1) * sizeof(uint64_t));
    if (!n) return CRGPU_OK;
    CR_REQUIRE(ctx, d_tags != nullptr, CRGPU_EINVAL, "crgpu_rtl_sample_columns_dev: NULL d_tags");
    DevBuf sot_b, key_b, keyt_b, val_b, valt_b, cnt_b;
    CR_TRY(rt_upload_table(ctx, sot_b, sample_of_tag, n_tags, RT_MAX_TAGS));
    for (DevBuf *b : {&key_b, &keyt_b, &val_b, &valt_b}) CR_TRY(dmalloc(ctx, *b, n * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, cnt_b, 256 * sizeof(unsigned long long)));
    CR_HIP(ctx, hipMemsetAsync(cnt_b.p, 0, 256 * sizeof(unsigned long long), ctx->stream));
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_rt_sample_keys, dim3(cr_grid(n, 256)), dim3(256), 0, ctx->stream, d_tags, V, d_cols, n, sot_b.as<uint8_t>(), n_samples,
                       key_b.as<uint32_t>(), val_b.as<uint32_t>(), cnt_b.as<unsigned long long>(), d_flag);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !flag, CRGPU_EINVAL, "crgpu_rtl_sample_columns_dev: a column is out of range");
    uint64_t cnt[256];
    CR_TRY(crgpu_memcpy_d2h(ctx, cnt, cnt_b.p, sizeof(cnt)));
    for (uint32_t s = 0; s < n_samples; s++) offsets_out[s + 1] = offsets_out[s] + cnt[s];
    const uint64_t kept = offsets_out[n_samples];
    if (!kept) return CRGPU_OK;  // no column has a sample: *d_cols_out stays NULL
    // the library's radix sort is stable: inside a sample the columns keep their order
    bool in_tmp = false;
    CR_TRY(cr_radix_sort_u32(ctx, key_b.as<uint32_t>(), keyt_b.as<uint32_t>(), val_b.as<uint32_t>(), valt_b.as<uint32_t>(), n, 0,
                             std::max<uint32_t>(1u, cr_ceil_log2((uint64_t)n_samples + 1)), &in_tmp));
    uint64_t *d_out = nullptr;
    CR_TRY(cr_pool_alloc(ctx, (void **)&d_out, kept * sizeof(uint64_t)));
    hipLaunchKernelGGL(k_rt_widen, dim3(cr_grid(kept, 256)), dim3(256), 0, ctx->stream, in_tmp ? valt_b.as<uint32_t>() : val_b.as<uint32_t>(), kept, d_out);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        cr_pool_free(ctx, d_out);
        return cr_fail(ctx, CRGPU_EHIP, "crgpu_rtl_sample_columns_dev: the split failed");
    }
    *d_cols_out = d_out;
    return CRGPU_OK;
}

// ---- 3. one pass over the runs: overlaps and GEM occupancy ---------------------------------------------------------------------
// the table of k_rt_gem_runs (u64 words)
#define RT_O_GEMS 0u                                          // [64] runs whose mask has the tag
#define RT_O_COMMON (RT_O_GEMS + RT_MAX_TAGS)                 // [T * T], row-major, i < j
#define RT_O_CTAG (RT_O_COMMON + RT_MAX_TAGS * RT_MAX_TAGS)   // [64] cells per tag
#define RT_O_HIST (RT_O_CTAG + RT_MAX_TAGS)                   // [257] runs holding k cells
#define RT_O_CPP (RT_O_HIST + RT_MAX_PROBES + 1)              // [256] cells per probe rank
#define RT_O_FIRST (RT_O_CPP + RT_MAX_PROBES)                 // [256] smallest cell column per probe rank (all ones: none)
#define RT_O_SCAL (RT_O_FIRST + RT_MAX_PROBES)                // runs with a cell, runs, AB-present mask
#define RT_O_WORDS (RT_O_SCAL + 4u)

// One thread per column.  Every thread adds its own column to the per-probe and per-tag cell tables; the thread of a run's FIRST
// column (its predecessor lies in another GEM) walks the run -- at most n_probe columns, across tile and workgroup boundaries,
// the neighbours' ranks come from L2 -- and builds the run's 64-bit tag mask: a bit per tag with a cell in the run and, with the
// antibody part, per tag whose Antibody sums in the run reach the tag's threshold.  The mask goes into the workgroup's LDS tables
// (gems per tag, the T x T pair table: k (k - 1) / 2 additions for k bits); the tables are flushed with global integer atomics.
template <bool AB>
__global__ __launch_bounds__(256) void k_rt_gem_runs(const uint32_t *__restrict__ rank, uint64_t V, uint32_t n_probe, const uint8_t *__restrict__ tags,
                                                     const uint8_t *__restrict__ cell, uint32_t n_tags, const uint8_t *__restrict__ ab_tag_of_probe,
                                                     const uint32_t *__restrict__ ab_sums, const unsigned long long *__restrict__ ab_min,
                                                     unsigned long long *__restrict__ out) {
    __shared__ uint32_t s_common[RT_MAX_TAGS * RT_MAX_TAGS];
    __shared__ uint32_t s_gems[RT_MAX_TAGS], s_ctag[RT_MAX_TAGS], s_hist[RT_MAX_PROBES + 1], s_cpp[RT_MAX_PROBES], s_first[RT_MAX_PROBES];
    __shared__ uint32_t s_scal[2];
    __shared__ unsigned long long s_pres, s_abmin[RT_MAX_TAGS];
    __shared__ uint8_t s_abtag[RT_MAX_PROBES];
    const uint32_t tid = threadIdx.x, TT = n_tags * n_tags;
    for (uint32_t i = tid; i < TT; i += 256) s_common[i] = 0u;
    s_cpp[tid] = 0u;
    s_first[tid] = 0xFFFFFFFFu;
    s_hist[tid] = 0u;
    if (tid == 0) s_hist[RT_MAX_PROBES] = 0u, s_scal[0] = 0u, s_scal[1] = 0u, s_pres = 0ull;
    if (tid < RT_MAX_TAGS) s_gems[tid] = 0u, s_ctag[tid] = 0u;
    if (AB) {
        s_abtag[tid] = ab_tag_of_probe[tid];
        if (tid < RT_MAX_TAGS) s_abmin[tid] = ab_min[tid];
    }
    __syncthreads();
    uint32_t my_runs = 0, my_cell_runs = 0;
    unsigned long long my_pres = 0ull;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + tid; c < V; c += stride) {
        const uint32_t r = rank[c], g = r / n_probe, p = r - g * n_probe;
        if (cell[c]) {
            const uint32_t t = tags[c];
            atomicAdd(&s_cpp[p], 1u);
            atomicMin(&s_first[p], (uint32_t)c);
            if (t < n_tags) atomicAdd(&s_ctag[t], 1u);
        }
        if (AB && ab_sums[c]) {
            const uint32_t at = s_abtag[p];
            if (at < n_tags && s_abmin[at] != ~0ull) my_pres |= 1ull << at;
        }
        if (c && rank[c - 1] / n_probe == g) continue;  // not the head of its run
        unsigned long long mask = 0ull;
        uint32_t n_cell = 0;
        uint64_t end = c;
        for (; end < V; end++) {
            if (end != c && rank[end] / n_probe != g) break;
            if (cell[end]) {
                const uint32_t t = tags[end];
                n_cell++;
                if (t < n_tags) mask |= 1ull << t;
            }
        }
        if (AB) {
            for (uint64_t j = c; j < end; j++) {
                if (!ab_sums[j]) continue;
                const uint32_t at = s_abtag[rank[j] - g * n_probe];
                if (at >= n_tags || ((mask >> at) & 1ull) || s_abmin[at] == ~0ull) continue;
                unsigned long long sum = 0ull;  // the non-zero Antibody sums of the run's columns of this tag
                for (uint64_t k = c; k < end; k++)
                    if (s_abtag[rank[k] - g * n_probe] == at) sum += ab_sums[k];
                if (sum >= s_abmin[at]) mask |= 1ull << at;
            }
        }
        my_runs++;
        if (n_cell) {
            my_cell_runs++;
            atomicAdd(&s_hist[n_cell < RT_MAX_PROBES ? n_cell : RT_MAX_PROBES], 1u);
        }
        for (unsigned long long mi = mask; mi;) {
            const uint32_t i = (uint32_t)__builtin_ctzll(mi);
            mi &= mi - 1ull;
            atomicAdd(&s_gems[i], 1u);
            for (unsigned long long mj = mi; mj;) {
                const uint32_t j = (uint32_t)__builtin_ctzll(mj);
                mj &= mj - 1ull;
                atomicAdd(&s_common[i * n_tags + j], 1u);
            }
        }
    }
    if (my_cell_runs) atomicAdd(&s_scal[0], my_cell_runs);
    if (my_runs) atomicAdd(&s_scal[1], my_runs);
    if (AB && my_pres) atomicOr(&s_pres, my_pres);
    __syncthreads();
    for (uint32_t i = tid; i < TT; i += 256)
        if (s_common[i]) atomicAdd(&out[RT_O_COMMON + (i / n_tags) * RT_MAX_TAGS + i % n_tags], (unsigned long long)s_common[i]);
    if (tid < RT_MAX_TAGS) {
        if (s_gems[tid]) atomicAdd(&out[RT_O_GEMS + tid], (unsigned long long)s_gems[tid]);
        if (s_ctag[tid]) atomicAdd(&out[RT_O_CTAG + tid], (unsigned long long)s_ctag[tid]);
    }
    if (s_hist[tid]) atomicAdd(&out[RT_O_HIST + tid], (unsigned long long)s_hist[tid]);
    if (s_cpp[tid]) atomicAdd(&out[RT_O_CPP + tid], (unsigned long long)s_cpp[tid]);
    if (s_first[tid] != 0xFFFFFFFFu) atomicMin(&out[RT_O_FIRST + tid], (unsigned long long)s_first[tid]);
    if (tid == 0) {
        if (s_hist[RT_MAX_PROBES]) atomicAdd(&out[RT_O_HIST + RT_MAX_PROBES], (unsigned long long)s_hist[RT_MAX_PROBES]);
        if (s_scal[0]) atomicAdd(&out[RT_O_SCAL], (unsigned long long)s_scal[0]);
        if (s_scal[1]) atomicAdd(&out[RT_O_SCAL + 1], (unsigned long long)s_scal[1]);
        if (s_pres) atomicOr(&out[RT_O_SCAL + 2], s_pres);
    }
}

extern "C" int crgpu_rtl_gem_runs_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint8_t *d_tags, uint32_t n_tags, const uint64_t *d_cell_cols,
                                      uint64_t n_cells, const uint8_t *ab_tag_of_probe, const uint32_t *d_ab_sums, const uint64_t *ab_min_count,
                                      crgpu_rtl_gem_runs *res) {
    if (!ctx || !m || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    memset(res, 0, sizeof(*res));
    for (uint32_t p = 0; p < RT_MAX_PROBES; p++) res->first_cell_col_per_probe[p] = ~0ull;
    uint32_t n_probe = 0;
    CR_TRY(rt_n_probe(ctx, "crgpu_rtl_gem_runs_dev", &n_probe));
    res->n_probe = n_probe;
    res->n_tags = n_tags;
    CR_REQUIRE(ctx, n_tags >= 1 && n_tags <= RT_MAX_TAGS, CRGPU_ERANGE, "crgpu_rtl_gem_runs_dev: 1 .. %d tags", RT_MAX_TAGS);
    const bool ab = ab_tag_of_probe || d_ab_sums || ab_min_count;
    const uint64_t V = m->n_barcodes;
    CR_REQUIRE(ctx, !ab || (ab_tag_of_probe && ab_min_count && (d_ab_sums || !V)), CRGPU_EINVAL,
               "crgpu_rtl_gem_runs_dev: the antibody part needs ab_tag_of_probe, d_ab_sums and ab_min_count");
    CR_REQUIRE(ctx, V < 0xFFFFFFFFull, CRGPU_ERANGE, "crgpu_rtl_gem_runs_dev: fewer than 2^32 - 1 columns");
    CR_REQUIRE(ctx, n_cells <= V && (d_cell_cols || !n_cells), CRGPU_EINVAL, "crgpu_rtl_gem_runs_dev: the cell call does not fit the matrix");
    for (uint32_t p = 0; ab && p < n_probe; p++)
        CR_REQUIRE(ctx, ab_tag_of_probe[p] < n_tags || ab_tag_of_probe[p] == RT_NONE, CRGPU_EINVAL, "crgpu_rtl_gem_runs_dev: ab_tag_of_probe[%u] = %u with %u tags",
                   p, ab_tag_of_probe[p], n_tags);
    if (!V) return CRGPU_OK;
    CR_REQUIRE(ctx, d_tags != nullptr, CRGPU_EINVAL, "crgpu_rtl_gem_runs_dev: NULL d_tags");
    DevBuf cell_b, out_b, abt_b, abm_b;
    CR_TRY(dmalloc(ctx, cell_b, V));
    CR_HIP(ctx, hipMemsetAsync(cell_b.p, 0, V, ctx->stream));
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    cr_check_columns<false>(ctx, d_cell_cols, n_cells, V, MarkByte{cell_b.as<uint8_t>()}, d_flag);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_TRY(cr_list_verdict(ctx, flag, "crgpu_rtl_gem_runs_dev", "cell column"));
    CR_TRY(dmalloc(ctx, out_b, RT_O_WORDS * sizeof(unsigned long long)));
    unsigned long long *d_out = out_b.as<unsigned long long>();
    CR_HIP(ctx, hipMemsetAsync(d_out, 0, RT_O_WORDS * sizeof(unsigned long long), ctx->stream));
    CR_HIP(ctx, hipMemsetAsync(d_out + RT_O_FIRST, 0xFF, RT_MAX_PROBES * sizeof(unsigned long long), ctx->stream));
    if (ab) {
        uint64_t mins[RT_MAX_TAGS];
        for (uint32_t t = 0; t < RT_MAX_TAGS; t++) mins[t] = t < n_tags ? ab_min_count[t] : ~0ull;
        CR_TRY(rt_upload_table(ctx, abt_b, ab_tag_of_probe, n_probe, RT_MAX_PROBES));
        CR_TRY(dmalloc(ctx, abm_b, sizeof(mins)));
        CR_TRY(crgpu_memcpy_h2d(ctx, abm_b.p, mins, sizeof(mins)));
        CR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (mins is on the stack)
    }
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, V);
        if (ab)
            hipLaunchKernelGGL(k_rt_gem_runs<true>, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, m->d_barcode_rank, V, n_probe, d_tags,
                               cell_b.as<uint8_t>(), n_tags, abt_b.as<uint8_t>(), d_ab_sums, abm_b.as<unsigned long long>(), d_out);
        else
            hipLaunchKernelGGL(k_rt_gem_runs<false>, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, m->d_barcode_rank, V, n_probe, d_tags,
                               cell_b.as<uint8_t>(), n_tags, (const uint8_t *)nullptr, (const uint32_t *)nullptr,
                               (const unsigned long long *)nullptr, d_out);
        CR_HIP(ctx, hipGetLastError());
    }
    std::vector<uint64_t> h(RT_O_WORDS);
    CR_TRY(crgpu_memcpy_d2h(ctx, h.data(), d_out, RT_O_WORDS * sizeof(uint64_t)));
    std::copy(h.begin() + RT_O_GEMS, h.begin() + RT_O_GEMS + RT_MAX_TAGS, res->gems_per_tag);
    std::copy(h.begin() + RT_O_COMMON, h.begin() + RT_O_COMMON + RT_MAX_TAGS * RT_MAX_TAGS, res->common);
    std::copy(h.begin() + RT_O_CTAG, h.begin() + RT_O_CTAG + RT_MAX_TAGS, res->cells_per_tag);
    std::copy(h.begin() + RT_O_HIST, h.begin() + RT_O_HIST + RT_MAX_PROBES + 1, res->cells_per_gem_hist);
    std::copy(h.begin() + RT_O_CPP, h.begin() + RT_O_CPP + RT_MAX_PROBES, res->cells_per_probe);
    std::copy(h.begin() + RT_O_FIRST, h.begin() + RT_O_FIRST + RT_MAX_PROBES, res->first_cell_col_per_probe);
    res->gems_with_cells = h[RT_O_SCAL];
    res->n_gems = h[RT_O_SCAL + 1];
    res->n_cells = n_cells;
    for (uint32_t t = 0; t < n_tags; t++) res->present[t] = (res->cells_per_tag[t] != 0) || ((h[RT_O_SCAL + 2] >> t) & 1ull);
    return CRGPU_OK;
}

// ---- 4. the median UMI count per cell of every probe rank ----------------------------------------------------------------------
struct RtNzFlag {
    const uint64_t *cols;
    const uint32_t *sums;
    __device__ __forceinline__ bool operator()(uint64_t k) const { return sums[cols[k]] != 0u; }
};
struct RtNzEmit {
    const uint64_t *cols;
    const uint32_t *sums, *rank;
    uint32_t n_probe;
    uint64_t *key;
    struct Pre {
        uint64_t k;
    };
    __device__ __forceinline__ Pre pre(uint64_t k) const {
        const uint64_t c = cols[k];
        return Pre{((uint64_t)(rank[c] % n_probe) << 32) | sums[c]};
    }
    __device__ __forceinline__ void operator()(uint64_t, uint32_t o, Pre p) const { key[o] = p.k; }
};
__global__ __launch_bounds__(256) void k_rt_probe_hist(const uint64_t *__restrict__ key, uint64_t n, unsigned long long *__restrict__ cnt) {
    __shared__ uint32_t s_cnt[RT_MAX_PROBES];
    s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) atomicAdd(&s_cnt[(uint32_t)(key[i] >> 32) & 0xFFu], 1u);
    __syncthreads();
    if (s_cnt[threadIdx.x]) atomicAdd(&cnt[threadIdx.x], (unsigned long long)s_cnt[threadIdx.x]);
}
// one workgroup: the offsets of the probe ranks in the sorted keys, then calculate_median_of_sorted (cr_types/src/utils.rs:57-70)
__global__ __launch_bounds__(256) void k_rt_medians(const uint64_t *__restrict__ key, const unsigned long long *__restrict__ cnt,
                                                    unsigned long long *__restrict__ median) {
    __shared__ unsigned long long s_off[RT_MAX_PROBES];
    if (threadIdx.x == 0) {
        unsigned long long o = 0;
        for (uint32_t p = 0; p < RT_MAX_PROBES; p++) {
            s_off[p] = o;
            o += cnt[p];
        }
    }
    __syncthreads();
    const unsigned long long n = cnt[threadIdx.x], o = s_off[threadIdx.x];
    unsigned long long med = 0ull;
    if (n) {
        const unsigned long long hi = key[o + n / 2] & 0xFFFFFFFFull;
        med = (n & 1ull) ? hi : ((key[o + n / 2 - 1] & 0xFFFFFFFFull) + hi) / 2ull;
    }
    median[threadIdx.x] = med;
}

extern "C" int crgpu_rtl_medians_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint32_t *d_sums, const uint64_t *d_cell_cols, uint64_t n_cells,
                                     uint64_t *n_nonzero_out, uint64_t *median_out) {
    if (!ctx || !m) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    uint32_t n_probe = 0;
    CR_TRY(rt_n_probe(ctx, "crgpu_rtl_medians_dev", &n_probe));
    CR_REQUIRE(ctx, n_nonzero_out && median_out, CRGPU_EINVAL, "crgpu_rtl_medians_dev: NULL output");
    memset(n_nonzero_out, 0, n_probe * sizeof(uint64_t));
    memset(median_out, 0, n_probe * sizeof(uint64_t));
    const uint64_t V = m->n_barcodes;
    CR_REQUIRE(ctx, V < 0xFFFFFFFFull, CRGPU_ERANGE, "crgpu_rtl_medians_dev: fewer than 2^32 - 1 columns");
    CR_REQUIRE(ctx, n_cells <= V, CRGPU_EINVAL, "crgpu_rtl_medians_dev: more cells than columns");
    if (!n_cells) return CRGPU_OK;
    CR_REQUIRE(ctx, d_sums && d_cell_cols, CRGPU_EINVAL, "crgpu_rtl_medians_dev: NULL d_sums or d_cell_cols");
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0, *d_total = ctx->d_scalars + CR_SCALAR_TOTAL, N = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    cr_check_columns<false>(ctx, d_cell_cols, n_cells, V, MarkNone{}, d_flag);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_TRY(cr_list_verdict(ctx, flag, "crgpu_rtl_medians_dev", "cell column"));
    DevBuf key_b, keyt_b, cnt_b;
    CR_TRY(dmalloc(ctx, key_b, n_cells * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, keyt_b, n_cells * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, cnt_b, 2 * RT_MAX_PROBES * sizeof(unsigned long long)));
    CR_HIP(ctx, hipMemsetAsync(cnt_b.p, 0, 2 * RT_MAX_PROBES * sizeof(unsigned long long), ctx->stream));
    CR_TRY(compact(ctx, RtNzFlag{d_cell_cols, d_sums}, RtNzEmit{d_cell_cols, d_sums, m->d_barcode_rank, n_probe, key_b.as<uint64_t>()}, n_cells,
                   ctx->d_sort_hist, d_total));
    CR_TRY(read_u32(ctx, d_total, &N));
    if (!N) return CRGPU_OK;
    bool in_tmp = false;
    CR_TRY(cr_radix_sort_u64(ctx, key_b.as<uint64_t>(), keyt_b.as<uint64_t>(), nullptr, nullptr, N, 0, 40, &in_tmp));
    const uint64_t *sorted = in_tmp ? keyt_b.as<uint64_t>() : key_b.as<uint64_t>();
    unsigned long long *d_cnt = cnt_b.as<unsigned long long>();
    hipLaunchKernelGGL(k_rt_probe_hist, dim3(cr_grid(N, 256)), dim3(256), 0, ctx->stream, sorted, (uint64_t)N, d_cnt);
    CR_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_rt_medians, dim3(1), dim3(256), 0, ctx->stream, sorted, d_cnt, d_cnt + RT_MAX_PROBES);
    CR_HIP(ctx, hipGetLastError());
    uint64_t h[2 * RT_MAX_PROBES];
    CR_TRY(crgpu_memcpy_d2h(ctx, h, d_cnt, sizeof(h)));
    std::copy(h, h + n_probe, n_nonzero_out);
    std::copy(h + RT_MAX_PROBES, h + RT_MAX_PROBES + n_probe, median_out);
    return CRGPU_OK;
}

// ---- 5. host functions (f64, unfused; no context) ------------------------------------------------------------------------------
extern "C" int crgpu_rtl_overlap_rows(const uint64_t *gems_per_tag, const uint64_t *common, const uint8_t *present, uint32_t n_tags,
                                      crgpu_rtl_overlap_row *rows_out, uint32_t cap, uint32_t *n_rows_out) {
    if (!gems_per_tag || !common || !present || !n_rows_out || n_tags < 1 || n_tags > RT_MAX_TAGS)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_rtl_overlap_rows: the three tables, n_rows_out and 1 .. %d tags", RT_MAX_TAGS);
    uint32_t n = 0;
    for (uint32_t i = 0; i < n_tags; i++)
        for (uint32_t j = i + 1; j < n_tags; j++) {
            if (!present[i] || !present[j]) continue;
            if (rows_out && n < cap) {
                crgpu_rtl_overlap_row &r = rows_out[n];
                r.tag1 = i, r.tag2 = j;
                r.gems1 = (int64_t)gems_per_tag[i], r.gems2 = (int64_t)gems_per_tag[j];
                r.common_gems = (int64_t)common[(size_t)i * RT_MAX_TAGS + j];
                r.overlap = (double)r.common_gems / (double)std::min(r.gems1, r.gems2);  // 0 / 0: NaN, as in Rust
            }
            n++;
        }
    *n_rows_out = n;
    if (rows_out && n > cap) return cr_fail(nullptr, CRGPU_ERANGE, "crgpu_rtl_overlap_rows: %u rows, room for %u", n, cap);
    return CRGPU_OK;
}

extern "C" int crgpu_rtl_ab_thresholds(const uint64_t *median, const uint64_t *n_nonzero, const uint8_t *ab_tag_of_probe, uint32_t n_probe,
                                       const uint8_t *tag_kind, uint32_t n_tags, uint64_t *ab_min_count_out) {
    if (!median || !n_nonzero || !ab_tag_of_probe || !tag_kind || !ab_min_count_out || n_tags < 1 || n_tags > RT_MAX_TAGS || n_probe > RT_MAX_PROBES)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_rtl_ab_thresholds: NULL argument or sizes out of range");
    for (uint32_t t = 0; t < n_tags; t++) ab_min_count_out[t] = ~0ull;  // removed: no cell of the tag holds Antibody counts
    for (uint32_t p = 0; p < n_probe; p++) {
        if (!n_nonzero[p]) continue;
        const uint32_t t = ab_tag_of_probe[p];
        if (t >= n_tags) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_rtl_ab_thresholds: probe rank %u has a median and no tag", p);
        if (tag_kind[t] != CRGPU_RTL_KIND_ANTIBODY)
            return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_rtl_ab_thresholds: tag %u was expected to be an antibody probe barcode", t);
        if (ab_min_count_out[t] != ~0ull) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_rtl_ab_thresholds: two probe ranks with medians map to tag %u", t);
        ab_min_count_out[t] = (uint64_t)std::round(0.1 * (double)median[p]);  // f64::round: half away from zero
    }
    return CRGPU_OK;
}

extern "C" int crgpu_rtl_suspicious_pairings(const crgpu_rtl_overlap_row *rows, uint32_t n_rows, const uint8_t *tag_kind, const int32_t *paired_with,
                                             uint32_t n_tags, crgpu_rtl_overlap_row *rows_out, uint32_t *n_rows_out) {
    if ((!rows && n_rows) || !tag_kind || !paired_with || (!rows_out && n_rows) || !n_rows_out || n_tags < 1 || n_tags > RT_MAX_TAGS)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_rtl_suspicious_pairings: NULL argument or tags out of range");
    uint32_t n = 0;
    for (uint32_t k = 0; k < n_rows; k++) {
        crgpu_rtl_overlap_row r = rows[k];
        if (r.tag1 >= n_tags || r.tag2 >= n_tags) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_rtl_suspicious_pairings: row %u names a tag >= %u", k, n_tags);
        const uint8_t k1 = tag_kind[r.tag1], k2 = tag_kind[r.tag2];
        if (!((k1 == CRGPU_RTL_KIND_RTL && k2 == CRGPU_RTL_KIND_ANTIBODY) || (k1 == CRGPU_RTL_KIND_ANTIBODY && k2 == CRGPU_RTL_KIND_RTL))) continue;
        if (k1 != CRGPU_RTL_KIND_RTL) {
            std::swap(r.tag1, r.tag2);
            std::swap(r.gems1, r.gems2);
        }
        if (paired_with[r.tag1] == (int32_t)r.tag2) continue;  // a configured pairing
        rows_out[n++] = r;
    }
    std::sort(rows_out, rows_out + n, [](const crgpu_rtl_overlap_row &a, const crgpu_rtl_overlap_row &b) {
        return a.tag1 != b.tag1 ? a.tag1 < b.tag1 : a.tag2 < b.tag2;
    });
    *n_rows_out = n;
    return CRGPU_OK;
}

// ---- 6. high-occupancy GEMs ----------------------------------------------------------------------------------------------------
extern "C" int crgpu_rtl_occupancy_summary(const uint64_t *cells_per_gem_hist, uint32_t n_probe, uint64_t gems_with_cells, const uint64_t *cells_per_probe,
                                           int64_t total_instrument_partitions, double recovery_factor, uint64_t *zero_bin_out,
                                           double *estimated_lambda_out, uint32_t *total_probe_barcodes_out) {
    if (!cells_per_gem_hist || !cells_per_probe || !zero_bin_out || !estimated_lambda_out || !total_probe_barcodes_out || n_probe < 1 ||
        n_probe > RT_MAX_PROBES)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_rtl_occupancy_summary: NULL argument or n_probe outside 1 .. %d", RT_MAX_PROBES);
    // max(0, int(partitions * recovery_factor - gems)): Python's float product, float difference, truncation
    const double d = (double)total_instrument_partitions * recovery_factor - (double)gems_with_cells;
    const uint64_t zero = d > 0.0 ? (uint64_t)d : 0ull;
    uint64_t num = 0, den = zero;  // np.average(keys, weights): both sums are exact integers below 2^53
    for (uint32_t k = 1; k <= n_probe; k++) {
        num += (uint64_t)k * cells_per_gem_hist[k];
        den += cells_per_gem_hist[k];
    }
    if (!den) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_rtl_occupancy_summary: the weights sum to zero (numpy raises ZeroDivisionError)");
    uint32_t probes = 0;
    for (uint32_t p = 0; p < n_probe; p++) probes += cells_per_probe[p] != 0;
    *zero_bin_out = zero;
    *estimated_lambda_out = (double)num / (double)den;
    *total_probe_barcodes_out = probes;
    return CRGPU_OK;
}

// The cells of one GEM are adjacent in the ascending cell list.  keep[k] = the GEM of cell k holds at most `threshold` cells;
// counters: GEMs above the threshold, cells in them, GEMs with a cell (counted at each GEM's first cell); flag: a column out of range
__global__ __launch_bounds__(256) void k_rt_occupancy(const uint32_t *__restrict__ rank, uint64_t V, const uint64_t *__restrict__ cols, uint64_t n,
                                                      uint32_t n_probe, uint32_t threshold, uint8_t *__restrict__ keep,
                                                      unsigned long long *__restrict__ counters, uint32_t *__restrict__ flag) {
    unsigned long long hi_gems = 0, hi_cells = 0, gems = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
        const uint64_t c = cols[k];
        if (c >= V) {
            *flag = 1u;
            keep[k] = 0u;
            continue;
        }
        const uint32_t g = rank[c] / n_probe;
        uint32_t cnt = 1;
        bool head = true;
        for (uint64_t b = k; b > 0 && cnt <= n_probe; b--) {  // (a list with repeated columns cannot make the walk longer than n_probe)
            const uint64_t cb = cols[b - 1];
            if (cb >= V || rank[cb] / n_probe != g) break;
            cnt++;
            head = false;
        }
        for (uint64_t f = k + 1; f < n && cnt <= 2 * n_probe; f++) {
            const uint64_t cf = cols[f];
            if (cf >= V || rank[cf] / n_probe != g) break;
            cnt++;
        }
        const bool high = cnt > threshold;
        keep[k] = high ? 0u : 1u;
        hi_cells += high;
        hi_gems += high && head;
        gems += head;
    }
    hi_gems = wave_sum(hi_gems), hi_cells = wave_sum(hi_cells), gems = wave_sum(gems);
    if ((threadIdx.x & 63u) == 0) {
        if (hi_gems) atomicAdd(&counters[0], hi_gems);
        if (hi_cells) atomicAdd(&counters[1], hi_cells);
        if (gems) atomicAdd(&counters[2], gems);
    }
}
struct RtKeepFlag {
    const uint8_t *keep;
    __device__ __forceinline__ bool operator()(uint64_t k) const { return keep[k] != 0u; }
};
struct RtKeepEmit {
    const uint64_t *cols;
    uint64_t *out;
    struct Pre {
        uint64_t c;
    };
    __device__ __forceinline__ Pre pre(uint64_t k) const { return Pre{cols[k]}; }
    __device__ __forceinline__ void operator()(uint64_t, uint32_t o, Pre p) const { out[o] = p.c; }
};

extern "C" int crgpu_rtl_remove_high_occupancy_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint64_t *d_cell_cols, uint64_t n_cells,
                                                   uint32_t threshold, uint64_t **d_kept_cols_out, crgpu_rtl_high_occupancy *res) {
    if (!ctx || !m || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    memset(res, 0, sizeof(*res));
    res->threshold = threshold;
    res->fraction_cell_gems_high_occupancy = res->fraction_cells_in_high_occupancy_gems = std::nan("");
    CR_REQUIRE(ctx, d_kept_cols_out != nullptr, CRGPU_EINVAL, "crgpu_rtl_remove_high_occupancy_dev: NULL d_kept_cols_out");
    *d_kept_cols_out = nullptr;
    uint32_t n_probe = 0;
    CR_TRY(rt_n_probe(ctx, "crgpu_rtl_remove_high_occupancy_dev", &n_probe));
    const uint64_t V = m->n_barcodes;
    CR_REQUIRE(ctx, V < 0xFFFFFFFFull && n_cells <= V, CRGPU_ERANGE, "crgpu_rtl_remove_high_occupancy_dev: at most V < 2^32 - 1 cells");
    CR_REQUIRE(ctx, d_cell_cols || !n_cells, CRGPU_EINVAL, "crgpu_rtl_remove_high_occupancy_dev: NULL d_cell_cols");
    uint64_t *d_out = nullptr;
    if (n_cells) {
        DevBuf keep_b, cnt_b;
        CR_TRY(dmalloc(ctx, keep_b, n_cells));
        CR_TRY(dmalloc(ctx, cnt_b, 4 * sizeof(unsigned long long)));
        CR_HIP(ctx, hipMemsetAsync(cnt_b.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
        uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0, *d_total = ctx->d_scalars + CR_SCALAR_TOTAL, kept = 0;
        CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
        {
            CrTimer t(ctx, CRGPU_T_MATRIX, n_cells);
            hipLaunchKernelGGL(k_rt_occupancy, dim3(cr_grid(n_cells, 256)), dim3(256), 0, ctx->stream, m->d_barcode_rank, V, d_cell_cols, n_cells, n_probe,
                               threshold, keep_b.as<uint8_t>(), cnt_b.as<unsigned long long>(), d_flag);
            CR_HIP(ctx, hipGetLastError());
        }
        CR_TRY(read_u32(ctx, d_flag, &flag));
        CR_REQUIRE(ctx, !flag, CRGPU_EINVAL, "crgpu_rtl_remove_high_occupancy_dev: a cell column is out of range");
        uint64_t cnt[4];
        CR_TRY(crgpu_memcpy_d2h(ctx, cnt, cnt_b.p, sizeof(cnt)));
        res->high_occupancy_gems = cnt[0], res->cells_in_high_occupancy_gems = cnt[1], res->gems_with_cells = cnt[2];
        CR_TRY(cr_pool_alloc(ctx, (void **)&d_out, n_cells * sizeof(uint64_t)));
        int rc = compact(ctx, RtKeepFlag{keep_b.as<uint8_t>()}, RtKeepEmit{d_cell_cols, d_out}, n_cells, ctx->d_sort_hist, d_total);
        if (rc == CRGPU_OK) rc = read_u32(ctx, d_total, &kept);
        if (rc == CRGPU_OK && (uint64_t)kept + cnt[1] != n_cells) rc = cr_fail(ctx, CRGPU_EHIP, "high-occupancy GEMs: %u kept and %llu removed of %llu cells", kept, (unsigned long long)cnt[1], (unsigned long long)n_cells);
        if (rc != CRGPU_OK) {
            cr_pool_free(ctx, d_out);
            return rc;
        }
        res->n_kept = kept;
    } else {
        CR_TRY(cr_pool_alloc(ctx, (void **)&d_out, sizeof(uint64_t)));
    }
    res->n_cells = n_cells;
    res->fraction_cell_gems_high_occupancy = cr_robust_divide((double)res->high_occupancy_gems, (double)res->gems_with_cells);
    res->fraction_cells_in_high_occupancy_gems = cr_robust_divide((double)res->cells_in_high_occupancy_gems, (double)res->n_cells);
    *d_kept_cols_out = d_out;
    return CRGPU_OK;
}
