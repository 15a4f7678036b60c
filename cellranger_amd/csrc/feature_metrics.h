// feature_metrics.h -- the per-feature tallies of the molecule table and the reads-per-UMI statistics of a targeted well (part of
// molecule_stages.hip: the tallies read crgpu_counts::d_mkeys / d_mreads).
//
// Replaces, for CALCULATE_TARGETED_METRICS (mro/rna/stages/targeted/calculate_targeted_metrics/__init__.py):
//   pandas_utils.collapse_feature_counts        lib/python/cellranger/pandas_utils.py:571-661   num_umis, num_reads, num_umis_cells,
//                                               num_reads_cells per feature (crgpu_feature_metrics_dev)
//   get_feature_summary_df's ratio columns, get_mean_per_gene_rpu_metrics, the gene counts of get_enrichment_metrics
//                                               __init__.py:167-301                              (crgpu_targeted_rpu_stats, host)
// The reference ORs the pass-filter barcodes of all selected libraries before it counts the `_cells` sums (pandas_utils.py:609-618),
// so ONE ascending list of cell ranks, the union, is the faithful interface.
//
// The table is ordered by (barcode, feature, library, UMI): the molecules of a barcode are contiguous (a SEGMENT) with ascending
// features, a feature's molecules are spread over every barcode, and a gene of every cell is one hot address.  So
//   1. the segment starts come from one compaction over d_mkeys (cr_barcode_segments);
//   2. the membership of a barcode in the cell list is decided ONCE per segment (k_fm_seg_cells: a thread per segment searches
//      d_cell_ranks); k_fm_pass gives every segment to one wave, which loads the bounds and the membership of its next segment
//      one segment ahead.  Every run of equal (barcode, feature) is added up inside the wave first (a segmented
//      sum over shuffles; the run ends come from one ballot): only the first lane of a run touches a counter;
//   3. the counters live in a SLICE of the workgroup's LDS (four u32 per feature; workgroup (s, w) owns slice s of the features
//      and every G-th group of 16 segments; features ascend inside a segment, so a wave finds its slice by two 64-ary searches,
//      segments of at most 256 molecules are read whole and filtered; a u32 read sum that wraps carries 2^32 into a u64 per feature
//      in device memory).  At the end a workgroup stores its slice to the slab [w][feature] with plain coalesced stores;
//      k_fm_slab_sum adds the slab up in 64 bits: no device-memory atomic on a hot feature.
// With ctx->fm_lds_features == 0 (CRGPU_FM_LDS_FEATURES=0) the run sums go to u64 atomics in device memory: the A/B of the slice form.
// Integer sums: no result depends on the order or on the switch.
// Not covered: collapse_feature_counts(downsample=...) (a binomial draw per molecule: Counts.subsample draws those), the CSV writer.
#pragma once

#include <algorithm>
#include <cmath>

#include "stage_common.h"

#define FM_WG 1024u  // threads of a pass workgroup: 16 waves, one segment each
#define FM_WAVES (FM_WG / 64u)
#define FM_UNROLL 4  // rounds of 64 molecules whose loads a wave issues together
#define FM_LDS_BYTES (160u * 1024u - 64u)
#define FM_SLICE_MAX (FM_LDS_BYTES / 16u)  // four u32 per feature
#define FM_READ_BITS 40u                   // a wave's read sum of one run: < 64 * 2^32

struct FmKeys {
    uint32_t sh_bc, sh_feat, bits_feat, sh_libid, bits_lib, n_features;
};

// the sum of v over the lanes [lane, end) of the wave: end = the lane behind the run of `lane`
__device__ __forceinline__ unsigned long long fm_run_sum(unsigned long long v, uint32_t lane, uint32_t end) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_down(v, d);
        if (lane + d < end) v += o;
    }
    return v;
}
// first molecule of [b, e) whose feature is >= bound (the features of a segment ascend): a 64-ary search, the lanes of the wave probe
// 64 places at a time; uniform arguments, uniform result
__device__ __forceinline__ uint32_t fm_lower_bound(const uint64_t *__restrict__ keys, uint32_t b, uint32_t e, uint32_t bound, uint32_t sh_feat,
                                                   uint64_t fmask, uint32_t lane) {
    while (e - b > 64u) {
        const uint32_t step = (e - b + 63u) / 64u;
        const uint64_t pos = (uint64_t)b + (uint64_t)lane * step;  // pos of lane 0 is b
        const bool below = pos < e && (uint32_t)((keys[pos < e ? pos : e - 1u] >> sh_feat) & fmask) < bound;
        const uint32_t cnt = (uint32_t)__popcll(__ballot(below));  // monotone: the first cnt probes are below the bound
        if (!cnt) return b;
        const uint64_t last = (uint64_t)b + (uint64_t)(cnt - 1u) * step, next = last + step;
        e = next < e ? (uint32_t)next : e;
        b = (uint32_t)last + 1u;
    }
    const uint32_t pos = b + lane;
    const bool below = pos < e && (uint32_t)((keys[pos < e ? pos : (e ? e - 1u : 0u)] >> sh_feat) & fmask) < bound;
    return b + (uint32_t)__popcll(__ballot(b < e && below));
}
// one thread per segment: is its barcode in the ascending cell list?
__global__ __launch_bounds__(256) void k_fm_seg_cells(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ seg_start, uint32_t n_seg, uint32_t sh_bc,
                                                      const uint32_t *__restrict__ cells, uint64_t n_cells, const uint32_t *__restrict__ back,
                                                      uint32_t n_back, uint8_t *__restrict__ seg_cell) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg) return;
    const uint64_t bc = keys[seg_start[s]] >> sh_bc;
    const uint32_t r = back ? (bc < n_back ? back[bc] : NONE32) : (uint32_t)bc;
    const uint64_t x = cr_lower_bound(cells, n_cells, r);
    seg_cell[s] = x < n_cells && cells[x] == r && (back || bc <= 0xFFFFFFFFull);
}

template <bool LDS>
__global__ __launch_bounds__(FM_WG) void k_fm_pass(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ reads, const uint32_t *__restrict__ seg_start,
                                                   uint32_t n_seg, const uint8_t *__restrict__ seg_cell, FmKeys K, uint32_t lib_mask, uint32_t slice, uint32_t G,
                                                   uint4 *__restrict__ slab, unsigned long long *__restrict__ carry,
                                                   unsigned long long *__restrict__ gout) {
    extern __shared__ uint32_t fm_s[];  // LDS: umis[slice], reads[slice], umis_cells[slice], reads_cells[slice]
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, nf = K.n_features;
    const uint32_t w = LDS ? blockIdx.x % G : blockIdx.x, n_wg = LDS ? G : gridDim.x;
    const uint32_t lo = LDS ? (blockIdx.x / G) * slice : 0u;
    const uint32_t hi = LDS ? (nf - lo < slice ? nf : lo + slice) : nf;
    if (LDS) {
        for (uint32_t i = tid; i < 4u * slice; i += FM_WG) fm_s[i] = 0u;
        __syncthreads();
    }
    const uint64_t fmask = lowmask(K.bits_feat), lmask = lowmask(K.bits_lib), rmask = (1ull << FM_READ_BITS) - 1ull;
    const uint64_t c_step = (uint64_t)n_wg * FM_WAVES;
    uint64_t c = (uint64_t)w * FM_WAVES + wave;
    uint32_t nb = 0, ne = 0, ncell = 0;  // the bounds and the membership of the wave's next segment, loaded one segment ahead
    if (c < n_seg) nb = seg_start[c], ne = seg_start[c + 1], ncell = seg_cell[c];
    for (; c < n_seg; c += c_step) {  // uniform in the wave
        uint32_t b = nb, e = ne;
        const bool is_cell = ncell != 0u;  // decided once per barcode run (k_fm_seg_cells)
        if (c + c_step < n_seg) nb = seg_start[c + c_step], ne = seg_start[c + c_step + 1], ncell = seg_cell[c + c_step];
        if (b >= e) continue;
        if (LDS && e - b > 64u * FM_UNROLL) {  // a shorter segment is read whole and filtered
            if (lo > 0u) b = fm_lower_bound(keys, b, e, lo, K.sh_feat, fmask, lane);
            if (hi < nf) e = fm_lower_bound(keys, b, e, hi, K.sh_feat, fmask, lane);
            if (b >= e) continue;
        }
        for (uint32_t i0 = b; i0 < e; i0 += 64u * FM_UNROLL) {  // e < 2^32 - 1 - 256: no wrap (nm is bounded by the caller)
            uint64_t key[FM_UNROLL];
            uint32_t rd[FM_UNROLL];
#pragma unroll
            for (int u = 0; u < FM_UNROLL; u++) {  // the loads of FM_UNROLL rounds are issued together
                const uint32_t i = i0 + 64u * u + lane;
                key[u] = i < e ? keys[i] : 0ull;
                rd[u] = i < e ? reads[i] : 0u;
            }
#pragma unroll
            for (int u = 0; u < FM_UNROLL; u++) {
                const bool live = i0 + 64u * u + lane < e;
                const uint32_t f = live ? (uint32_t)((key[u] >> K.sh_feat) & fmask) : NONE32;
                const uint32_t lib = (uint32_t)((key[u] >> K.sh_libid) & lmask);
                const bool mine = live && f >= lo && f < hi;  // hi <= n_features: a counter of this workgroup
                const bool counted = mine && lib < 32u && ((lib_mask >> (lib & 31u)) & 1u);
                if (!__ballot(counted)) continue;  // uniform in the wave
                const uint32_t prev = __shfl_up(f, 1);
                const bool head = lane == 0u || prev != f;
                const unsigned long long hm = __ballot(head);
                const unsigned long long after = lane == 63u ? 0ull : hm & (~0ull << (lane + 1u));
                const uint32_t end = after ? (uint32_t)__builtin_ctzll(after) : 64u;
                const unsigned long long sum = fm_run_sum(counted ? ((1ull << FM_READ_BITS) | rd[u]) : 0ull, lane, end);
                if (!head || !mine || !sum) continue;
                const uint32_t n_run = (uint32_t)(sum >> FM_READ_BITS);
                const unsigned long long r_run = sum & rmask;
                if (LDS) {
                    const uint32_t j = f - lo;  // < slice
                    atomicAdd(&fm_s[j], n_run);
                    const uint32_t old = atomicAdd(&fm_s[slice + j], (uint32_t)r_run);
                    const unsigned long long cy = (r_run >> 32) + ((uint32_t)(old + (uint32_t)r_run) < old ? 1ull : 0ull);
                    if (cy) atomicAdd(&carry[f], cy << 32);  // the u32 counter wrapped
                    if (is_cell) {
                        atomicAdd(&fm_s[2u * slice + j], n_run);
                        const uint32_t oldc = atomicAdd(&fm_s[3u * slice + j], (uint32_t)r_run);
                        const unsigned long long cc = (r_run >> 32) + ((uint32_t)(oldc + (uint32_t)r_run) < oldc ? 1ull : 0ull);
                        if (cc) atomicAdd(&carry[(size_t)nf + f], cc << 32);
                    }
                } else {
                    atomicAdd(&gout[f], (unsigned long long)n_run);
                    atomicAdd(&gout[(size_t)nf + f], r_run);
                    if (is_cell) {
                        atomicAdd(&gout[2 * (size_t)nf + f], (unsigned long long)n_run);
                        atomicAdd(&gout[3 * (size_t)nf + f], r_run);
                    }
                }
            }
        }
    }
    if (LDS) {
        __syncthreads();
        uint4 *row = slab + (size_t)w * nf + lo;
        for (uint32_t i = tid; i < hi - lo; i += FM_WG) row[i] = make_uint4(fm_s[i], fm_s[slice + i], fm_s[2u * slice + i], fm_s[3u * slice + i]);
    }
}

// out: umis[nf], reads[nf], umis_cells[nf], reads_cells[nf]
__global__ __launch_bounds__(256) void k_fm_slab_sum(const uint4 *__restrict__ slab, uint32_t G, uint32_t nf, const unsigned long long *__restrict__ carry,
                                                     unsigned long long *__restrict__ out) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < nf; f += stride) {
        unsigned long long a = 0, b = carry[f], c = 0, d = carry[(size_t)nf + f];
        for (uint32_t g = 0; g < G; g++) {
            const uint4 v = slab[(size_t)g * nf + f];
            a += v.x, b += v.y, c += v.z, d += v.w;
        }
        out[f] = a, out[(size_t)nf + f] = b, out[2 * (size_t)nf + f] = c, out[3 * (size_t)nf + f] = d;
    }
}

extern "C" int crgpu_feature_metrics_dev(crgpu_ctx *ctx, crgpu_counts *c, uint32_t n_features, uint32_t lib_mask, const uint32_t *d_cell_ranks,
                                         uint64_t n_cells, uint64_t *umis_out, uint64_t *reads_out, uint64_t *umis_cells_out,
                                         uint64_t *reads_cells_out) {
    if (!ctx || !c) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const KeyLayout &L = c->layout;
    CR_REQUIRE(ctx, lib_mask != 0u, CRGPU_EINVAL, "crgpu_feature_metrics_dev: an empty library mask");
    for (uint32_t l = 0; l < 32; l++)
        CR_REQUIRE(ctx, !((lib_mask >> l) & 1u) || l < L.n_libs, CRGPU_EINVAL, "crgpu_feature_metrics_dev: library %u lies outside the key layout (%u libraries)",
                   l, L.n_libs);
    CR_REQUIRE(ctx, n_features == L.n_features, CRGPU_EINVAL, "crgpu_feature_metrics_dev: n_features %u, the key layout has %u", n_features, L.n_features);
    CR_REQUIRE(ctx, d_cell_ranks || n_cells == 0, CRGPU_EINVAL, "crgpu_feature_metrics_dev: NULL cell ranks");
    const uint64_t nm = c->n_molecules, nf = n_features;
    CR_REQUIRE(ctx, nm < 0xFFFFFF00ull, CRGPU_ERANGE, "crgpu_feature_metrics_dev: too many molecules");  // u32 positions, a round of 256 behind the last
    uint64_t *outs[4] = {umis_out, reads_out, umis_cells_out, reads_cells_out};
    for (uint64_t *o : outs)
        if (o && nf) memset(o, 0, nf * sizeof(uint64_t));
    CR_TRY(cr_require_ascending_ranks(ctx, d_cell_ranks, n_cells, "crgpu_feature_metrics_dev", "cell barcode rank"));
    if (!nm || !nf) return CRGPU_OK;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
    // ---- the segments: one per barcode with a molecule ----
    DevBuf seg_b, cell_b, out_b, slab_b, carry_b;
    uint32_t n_seg = 0;
    CR_TRY(cr_barcode_segments(ctx, c, "crgpu_feature_metrics_dev", seg_b, &n_seg));
    const uint32_t *seg_start = seg_b.as<uint32_t>();
    const FmKeys K{L.sh_bc(), L.sh_feat(), L.bits_feat, L.sh_libid(), L.bits_lib, n_features};
    CR_TRY(dmalloc(ctx, out_b, 4 * nf * sizeof(unsigned long long)));
    CR_TRY(dmalloc(ctx, cell_b, n_seg));
    const bool lds = ctx->fm_lds_features != 0u;
    const uint64_t n_groups = ((uint64_t)n_seg + FM_WAVES - 1) / FM_WAVES;
    {
        CrTimer t(ctx, CRGPU_T_DEDUP, nm);
        hipLaunchKernelGGL(k_fm_seg_cells, dim3((n_seg + 255u) / 256u), dim3(256), 0, ctx->stream, c->d_mkeys, seg_start, n_seg, L.sh_bc(), d_cell_ranks, n_cells,
                           c->d_back, c->n_back, cell_b.as<uint8_t>());
        if (lds) {
            const uint32_t slice = std::min(std::min(ctx->fm_lds_features, (uint32_t)FM_SLICE_MAX), n_features);
            const uint32_t n_slices = (n_features + slice - 1) / slice;
            const size_t dyn = (size_t)slice * 16;
            int n_cu = 0;
            if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || n_cu < 1) n_cu = 256;
            // One workgroup of 1024 threads fills a CU (two where two slices fit its LDS).  The slices do not carry equal work (the
            // first 10 000 of 36 601 genes hold most molecules), so up to four rounds of workgroups are launched and every slice
            // gets as many as fill the device: the CUs that finish a light slice take workgroups of a heavy one.
            const uint32_t per_cu = 2u * dyn <= FM_LDS_BYTES ? 2u : 1u, fill = (uint32_t)n_cu * per_cu;
            const uint32_t G = std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>(std::min<uint64_t>(fill, 4ull * fill / n_slices), n_groups));
            CR_TRY(dmalloc(ctx, slab_b, (uint64_t)G * nf * sizeof(uint4)));
            CR_TRY(dmalloc(ctx, carry_b, 2 * nf * sizeof(unsigned long long)));
            CR_HIP(ctx, hipMemsetAsync(carry_b.p, 0, 2 * nf * sizeof(unsigned long long), ctx->stream));
            cr_allow_lds(ctx, (const void *)k_fm_pass<true>, dyn);
            hipLaunchKernelGGL(k_fm_pass<true>, dim3(n_slices * G), dim3(FM_WG), dyn, ctx->stream, c->d_mkeys, c->d_mreads, seg_start, n_seg, cell_b.as<uint8_t>(), K,
                               lib_mask, slice, G, slab_b.as<uint4>(), carry_b.as<unsigned long long>(),
                               out_b.as<unsigned long long>());
            CR_HIP(ctx, hipGetLastError());
            hipLaunchKernelGGL(k_fm_slab_sum, dim3(cr_grid(nf, 256)), dim3(256), 0, ctx->stream, slab_b.as<uint4>(), G, n_features,
                               carry_b.as<unsigned long long>(), out_b.as<unsigned long long>());
        } else {
            CR_HIP(ctx, hipMemsetAsync(out_b.p, 0, 4 * nf * sizeof(unsigned long long), ctx->stream));
            hipLaunchKernelGGL(k_fm_pass<false>, dim3(cr_grid(n_groups * FM_WG, FM_WG, 1024)), dim3(FM_WG), 0, ctx->stream, c->d_mkeys, c->d_mreads, seg_start, n_seg,
                               cell_b.as<uint8_t>(), K, lib_mask, 0u, 0u, (uint4 *)nullptr, (unsigned long long *)nullptr,
                               out_b.as<unsigned long long>());
        }
        CR_HIP(ctx, hipGetLastError());
    }
    for (uint32_t k = 0; k < 4; k++)
        if (outs[k]) CR_TRY(crgpu_memcpy_d2h(ctx, outs[k], out_b.as<unsigned long long>() + k * nf, nf * sizeof(uint64_t)));
    return CRGPU_OK;
}

// ---- reads-per-UMI statistics and gene counts (host, f64, unfused; no context) -----------------------------------------------------
// pandas' mean / std(ddof = 1) / median / quantile of a Series with skipna: NaN entries are left out
static void fm_series_stats(std::vector<double> v, bool selected_any, double *mean, double *cv, double *median, double *iqrnorm, double *perc80) {
    const double nan = std::nan("");
    if (!selected_any) {  // reads_per_umi.shape[0] == 0
        *mean = *cv = *median = *iqrnorm = *perc80 = 0.0;
        return;
    }
    v.erase(std::remove_if(v.begin(), v.end(), [](double x) { return std::isnan(x); }), v.end());
    const size_t n = v.size();
    if (!n) {
        *mean = *cv = *median = *iqrnorm = *perc80 = nan;
        return;
    }
    *mean = cr_pairwise_sum(v.data(), n) / (double)n;  // nanops.nanmean: the sum of the values / their count
    double sd = nan;
    if (n > 1) {  // nanops.nanvar: sum((avg - x)^2) / (count - 1)
        std::vector<double> sq(n);
        for (size_t i = 0; i < n; i++) sq[i] = (*mean - v[i]) * (*mean - v[i]);
        sd = std::sqrt(cr_pairwise_sum(sq.data(), n) / (double)(n - 1));
    }
    *cv = cr_robust_divide(sd, *mean);
    std::sort(v.begin(), v.end());
    *median = cr_median_sorted(v);
    // Series.quantile(q) asks np.percentile for q * 100, which divides by 100 again
    *iqrnorm = cr_robust_divide(cr_quantile_sorted(v, 0.75 * 100.0 / 100.0) - cr_quantile_sorted(v, 0.25 * 100.0 / 100.0), *median);
    *perc80 = cr_quantile_sorted(v, 0.80 * 100.0 / 100.0);
}

extern "C" int crgpu_targeted_rpu_stats(uint32_t n_features, const uint64_t *num_umis, const uint64_t *num_reads, const uint64_t *num_umis_cells,
                                        const uint64_t *num_reads_cells, const uint8_t *is_targeted, const uint8_t *is_gex, crgpu_rpu_stats *out,
                                        uint32_t *q_feature_out, double *q_value_out, uint8_t *q_label_out) {
    if (!out || ((!num_umis || !num_reads || !num_umis_cells || !num_reads_cells || !is_targeted) && n_features))
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_targeted_rpu_stats: NULL argument");
    memset(out, 0, sizeof(*out));
    std::vector<double> sel[4];  // [2 * off_target + all_barcodes]
    bool any[2] = {false, false};
    unsigned __int128 t_reads = 0, t_umis = 0;
    uint64_t nq = 0;
    for (uint32_t f = 0; f < n_features; f++) {
        if (is_gex && !is_gex[f]) continue;  // the reference keeps the Gene Expression rows only
        const uint32_t off = is_targeted[f] ? 0u : 1u;
        out->n_genes[off]++;
        if (num_umis_cells[f] == 0) out->n_not_detected[off]++;
        if (num_umis_cells[f] < CRGPU_TARGETED_MIN_UMIS) {
            out->n_not_quantifiable[off]++;
        } else {
            any[off] = true;
            // uint64 / uint64 of pandas: both sides as f64; 0 / 0 is NaN and skipped
            sel[2 * off].push_back((double)num_reads_cells[f] / (double)num_umis_cells[f]);
            sel[2 * off + 1].push_back((double)num_reads[f] / (double)num_umis[f]);
            if (q_feature_out) q_feature_out[nq] = f;
            if (q_value_out) q_value_out[nq] = std::log10((double)num_reads_cells[f] / (double)num_umis_cells[f]);
            if (q_label_out) q_label_out[nq] = off ? 0 : 1;
            nq++;
        }
        if (!off) t_reads += num_reads[f], t_umis += num_umis[f];
    }
    for (uint32_t off = 0; off < 2; off++) {
        out->n_detected[off] = out->n_genes[off] - out->n_not_detected[off];
        out->n_quantifiable[off] = out->n_genes[off] - out->n_not_quantifiable[off];
    }
    out->n_quantifiable_total = nq;
    for (uint32_t k = 0; k < 4; k++) fm_series_stats(sel[k], any[k / 2], &out->mean[k], &out->cv[k], &out->median[k], &out->iqrnorm[k], &out->perc80[k]);
    // robust_divide(total_targeted_reads - total_targeted_umis, total_targeted_reads): Python integers, rounded once by float()
    out->pcr_dupe_reads_frac_on_target = t_reads == 0 ? std::nan("") : (t_reads >= t_umis ? (double)(t_reads - t_umis) : -(double)(t_umis - t_reads)) / (double)t_reads;
    return CRGPU_OK;
}
