// normalize_depth.h -- aggr's depth normalisation of one GEM well: the downsampled UMI matrix and the read sums (part of
// molecule_stages.hip: works on crgpu_counts; the draw kernels and the position map are those of subsample.h).
//
// Replaces main / _update_metrics / _get_new_read_pairs / _get_matrix / summarize_read_matrix of NORMALIZE_DEPTH
// (mro/rna/stages/aggregator/normalize_depth/__init__.py:229-263,316-368,387-517) for one chunk that holds the whole table of one
// well, the rates of split() (:139-176, crgpu_normalize_depth_plan) and CountMatrix.select_features (lib/python/cellranger/
// matrix.py:886-894, crgpu_select_features_dev).  The reference's np.random.binomial on the serial MT19937 stream is replaced: read
// j of molecule m owns word j of the Philox stream m (philox.h), u = word >> 11, and the read is kept iff u < T[library],
// T = floor(frac_reads_kept * 2^53) -- the stream and the rule of subsample.h with one task.
//
//   1. prep     k_ss_prep: the molecules of many reads on the wave and workgroup lists, a key outside the layout;
//   2. draw     k_ss_draw_lane / _wave / _wg with one task: kept[molecule] (u32, device order);
//   3. sums     k_nd_tally, one pass over the table: kept per feature class (all barcodes, and the cells of the class through a
//               table of class masks per barcode), reads, kept reads and kept molecules per library, kept_out in table order.  A
//               wave reduces per class and per library that occurs in its 64 molecules, adds to the workgroup's LDS sums, and the
//               workgroup adds its non-zero sums with 64-bit integer atomics (exact in any order);
//   4. runs     the key order (feature above library above UMI inside a barcode) makes the molecules of a (barcode, feature)
//               pair contiguous, but a run may be one molecule or a whole barcode and crosses every tile edge, so nothing walks
//               a run: the survivors (kept > 0) are compacted to their (barcode, feature) pairs, the heads of the compacted list
//               (a pair that differs from its predecessor) are compacted to the triplets, and a triplet's count is the distance
//               to the next head.  Both steps are the stable compaction of stage_common.h, whose totals are the survivor and triplet
//               counts; the triplets leave in (barcode, feature) order for crgpu_assemble_matrix_dev.
// Nothing is floating point on the device and nothing depends on timing or on the two thresholds of the draw.
#pragma once

#include "stage_common.h"
#include "subsample.h"

#define ND_THREADS 256u
#define ND_MAX_CLASSES 32u
#define ND_SUM_RAW 0u                                 // [class]
#define ND_SUM_FLT ND_MAX_CLASSES                     // [class]
#define ND_SUM_READS (2u * ND_MAX_CLASSES)            // [library]
#define ND_SUM_KEPT (ND_SUM_READS + CRGPU_MAX_LIB)    // [library]
#define ND_SUM_MOLS (ND_SUM_KEPT + CRGPU_MAX_LIB)     // [library]
#define ND_SUMS (ND_SUM_MOLS + CRGPU_MAX_LIB)

// per value of the barcode field: the classes the barcode is a cell of (the table starts as zeros: not a cell)
__global__ __launch_bounds__(256) void k_nd_cell_table(const uint32_t *__restrict__ cells, uint64_t n_cells, const uint32_t *__restrict__ ccm,
                                                       const uint32_t *__restrict__ back, uint32_t n_bc, uint32_t *__restrict__ bc_mask) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t ci = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; ci < n_cells; ci += stride) {
        const uint32_t r = cells[ci];
        uint32_t b = r;
        if (back) {  // CRGPU_OPT_DENSE_BARCODE_KEYS: the field holds the column, back[column] = rank (ascending)
            const uint32_t lo = cr_lower_bound(back, n_bc, r);
            if (lo >= n_bc || back[lo] != r) continue;
            b = lo;
        }
        if (b < n_bc) bc_mask[b] = ccm ? ccm[ci] : 0xFFFFFFFFu;
    }
}

struct NdTally {
    SsKeys K;
    const uint32_t *kept;      // [molecule], device order
    const uint8_t *fclass;     // per feature, NULL: class 0
    const uint32_t *bc_mask;   // k_nd_cell_table, NULL: no cells
    uint32_t sh_bc, n_bc;
    uint32_t *kept_tab;        // kept in table order (written where K.mpos != NULL), or NULL
    unsigned long long *sums;  // [ND_SUMS], zeroed
};

__global__ __launch_bounds__(ND_THREADS) void k_nd_tally(NdTally a) {
    __shared__ unsigned long long s_sum[ND_SUMS];
    for (uint32_t j = threadIdx.x; j < ND_SUMS; j += ND_THREADS) s_sum[j] = 0ull;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // a wave takes 64 consecutive molecules at a time (base is the same in all its lanes)
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x - lane); base < a.K.nm; base += stride) {
        const uint64_t i = base + lane;
        const bool in = i < a.K.nm;
        const uint64_t key = in ? a.K.mkeys[i] : 0ull;
        const uint32_t k = in ? a.kept[i] : 0u, reads = in ? a.K.mreads[i] : 0u;
        const uint32_t f = ss_feature(a.K, key), lib = ss_library(a.K, key);
        const bool ok = in && f < a.K.n_features && lib < a.K.n_libs;  // (k_ss_prep has refused a table with any other key)
        if (ok && a.kept_tab) a.kept_tab[a.K.mpos ? a.K.mpos[i] : i] = k;
        const uint32_t cls = ((ok && a.fclass) ? a.fclass[f] : 0u) & (ND_MAX_CLASSES - 1u);
        const uint32_t b = (uint32_t)(key >> a.sh_bc);
        const bool cell = ok && a.bc_mask && b < a.n_bc && ((a.bc_mask[b] >> cls) & 1u);
        // the classes, then the libraries, that occur among the 64 molecules: one or two of each as a rule
        unsigned long long todo = __ballot(ok);
        while (todo) {
            const uint32_t c = __shfl(cls, __ffsll((long long)todo) - 1);
            const bool mine = ok && cls == c;
            const unsigned long long raw = wave_sum((unsigned long long)(mine ? k : 0u)), flt = wave_sum((unsigned long long)((mine && cell) ? k : 0u));
            if (lane == 0) {
                if (raw) atomicAdd(&s_sum[ND_SUM_RAW + c], raw);
                if (flt) atomicAdd(&s_sum[ND_SUM_FLT + c], flt);
            }
            todo &= ~__ballot(mine);
        }
        todo = __ballot(ok);
        while (todo) {
            const uint32_t l = __shfl(lib, __ffsll((long long)todo) - 1) & (CRGPU_MAX_LIB - 1u);
            const bool mine = ok && lib == l;
            const unsigned long long r = wave_sum((unsigned long long)(mine ? reads : 0u)), kr = wave_sum((unsigned long long)(mine ? k : 0u));
            const unsigned long long km = (unsigned long long)__popcll(__ballot(mine && k > 0u));
            if (lane == 0) {
                if (r) atomicAdd(&s_sum[ND_SUM_READS + l], r);
                if (kr) atomicAdd(&s_sum[ND_SUM_KEPT + l], kr);
                if (km) atomicAdd(&s_sum[ND_SUM_MOLS + l], km);
            }
            todo &= ~__ballot(mine);
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < ND_SUMS; j += ND_THREADS)
        if (s_sum[j]) atomicAdd(&a.sums[j], s_sum[j]);
}

// ---- the runs ---------------------------------------------------------------------------------------------------------------------
struct NdSurvFlag {  // a molecule that keeps at least one read
    const uint32_t *kept;
    __device__ __forceinline__ bool operator()(uint64_t i) const { return kept[i] != 0u; }
};
struct NdEmitPair {  // its (barcode, feature) pair: the key above the library field
    const uint64_t *keys;
    uint32_t sh_feat;
    uint64_t *pair;
    struct Pre {
        uint64_t key;
    };
    __device__ __forceinline__ Pre pre(uint64_t i) const { return Pre{keys[i]}; }
    __device__ __forceinline__ void operator()(uint64_t, uint32_t o, Pre p) const { pair[o] = p.key >> sh_feat; }
};
struct NdHeadFlag {  // first survivor of its pair
    const uint64_t *pair;
    __device__ __forceinline__ bool operator()(uint64_t o) const { return (o == 0) | (pair[o] != pair[o ? o - 1 : 0]); }
};
struct NdEmitTriplet {
    const uint64_t *pair;
    uint32_t bits_feat;
    const uint32_t *back;  // CRGPU_OPT_DENSE_BARCODE_KEYS: column -> rank, else NULL
    uint32_t n_back;
    uint32_t *t_bc, *t_feat, *t_first;
    struct Pre {
        uint64_t pair;
    };
    __device__ __forceinline__ Pre pre(uint64_t o) const { return Pre{pair[o]}; }
    __device__ __forceinline__ void operator()(uint64_t o, uint32_t t, Pre p) const {
        const uint32_t b = (uint32_t)(p.pair >> bits_feat);
        t_bc[t] = (back && b < n_back) ? back[b] : b;
        t_feat[t] = (uint32_t)(p.pair & lowmask(bits_feat));
        t_first[t] = (uint32_t)o;
    }
};
// survivors of a triplet = the distance to the next head
__global__ __launch_bounds__(256) void k_nd_counts(const uint32_t *__restrict__ t_first, uint64_t nt, uint32_t n_surv, uint32_t *__restrict__ t_cnt) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nt; t += stride)
        t_cnt[t] = (t + 1 < nt ? t_first[t + 1] : n_surv) - t_first[t];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static int nd_run(crgpu_ctx *ctx, crgpu_counts *c, const crgpu_normalize_depth_args *a, crgpu_normalize_depth_result *res) {
    const KeyLayout &L = c->layout;
    const uint32_t NL = a->n_libs, F = a->n_features, NK = a->n_classes;
    const uint64_t nm = c->n_molecules, NC = a->n_cells;
    for (int64_t *p : {a->raw_mapped_reads, a->flt_mapped_reads})
        if (p) memset(p, 0, (size_t)NK * sizeof(int64_t));
    for (int64_t *p : {a->reads_per_lib, a->kept_reads_per_lib, a->kept_molecules_per_lib})
        if (p) memset(p, 0, (size_t)NL * sizeof(int64_t));

    uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL;
    CR_TRY(cr_require_ascending_ranks(ctx, a->d_cell_ranks, NC, "crgpu_normalize_depth_dev", "cell barcode rank"));
    if (!nm) return a->matrix ? crgpu_assemble_matrix_dev(ctx, nullptr, nullptr, nullptr, 0, a->matrix) : CRGPU_OK;

    const uint32_t wave_min = std::min<uint32_t>(std::max<uint32_t>(ctx->ss_wave_min, 1u), SS_WAVE_MIN_MAX);
    const uint32_t wg_min = std::min<uint32_t>(std::max<uint32_t>(ctx->ss_wg_min, wave_min), SS_WG_MIN_MAX);
    const uint32_t *d_pos = nullptr;
    CR_TRY(ss_positions(ctx, c, &d_pos));
    const SsKeys K{c->d_mkeys, c->d_mreads, d_pos, nullptr, nm, L.sh_feat(), L.bits_feat, L.sh_libid(), L.bits_lib, F, NL};

    // 1. prep (one genome: any_reads per library, not reported)
    DevBuf small_b, list_b, ctl_b;
    CR_TRY(dmalloc(ctx, small_b, 2ull * NL));
    CR_TRY(dmalloc(ctx, list_b, nm * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, ctl_b, SS_CTL_WORDS * sizeof(uint32_t)));
    uint32_t *list = list_b.as<uint32_t>(), *ctl = ctl_b.as<uint32_t>();
    {
        CrTimer t(ctx, CRGPU_T_DEDUP, nm);
        CR_HIP(ctx, hipMemsetAsync(small_b.p, 0, 2ull * NL, ctx->stream));
        CR_HIP(ctx, hipMemsetAsync(ctl, 0, SS_CTL_WORDS * sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(k_ss_prep, dim3(cr_grid(nm, 256)), dim3(256), 0, ctx->stream, K, (const uint8_t *)nullptr, 1u, wave_min, wg_min,
                           small_b.as<uint8_t>(), small_b.as<uint8_t>() + NL, list, ctl);
        CR_HIP(ctx, hipGetLastError());
    }
    uint32_t h_ctl[SS_CTL_WORDS];
    CR_TRY(crgpu_memcpy_d2h(ctx, h_ctl, ctl, sizeof(h_ctl)));
    CR_REQUIRE(ctx, !h_ctl[SS_CTL_BAD], CRGPU_ESTATE, "crgpu_normalize_depth_dev: a molecule key holds a feature >= %u or a library >= %u", F, NL);
    const uint32_t n_wave = h_ctl[SS_CTL_N_WAVE], n_wg = h_ctl[SS_CTL_N_WG];
    CR_REQUIRE(ctx, (uint64_t)n_wave + n_wg <= nm, CRGPU_EHIP, "crgpu_normalize_depth_dev: inconsistent molecule classes");
    if (res) {
        res->n_molecules = nm;
        res->n_wave = n_wave;
        res->n_workgroup = n_wg;
        res->n_lane = nm - n_wave - n_wg;
    }

    // the thresholds of the one task, the tables of the sums
    std::vector<unsigned long long> h_thr((size_t)CRGPU_MAX_LIB * SS_MAX_BATCH, 0ull);
    for (uint32_t l = 0; l < NL; l++) h_thr[(size_t)l * SS_MAX_BATCH] = (unsigned long long)std::floor(std::ldexp(a->frac_reads_kept[l], 53));  // exact
    const uint32_t n_bc = c->d_back ? c->n_back : c->n_canon;
    DevBuf thr_b, kept_b, tab_b, fclass_b, ccm_b, mask_b, sums_b;
    CR_TRY(dmalloc(ctx, thr_b, h_thr.size() * sizeof(unsigned long long)));
    CR_TRY(crgpu_memcpy_h2d(ctx, thr_b.p, h_thr.data(), h_thr.size() * sizeof(unsigned long long)));
    CR_TRY(dmalloc(ctx, kept_b, nm * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, sums_b, ND_SUMS * sizeof(unsigned long long)));
    if (a->kept_out && d_pos) CR_TRY(dmalloc(ctx, tab_b, nm * sizeof(uint32_t)));
    if (a->feature_class) {
        CR_TRY(dmalloc(ctx, fclass_b, F));
        CR_TRY(crgpu_memcpy_h2d(ctx, fclass_b.p, a->feature_class, F));
    }
    if (NC && n_bc) {
        if (a->cell_class_mask) {
            CR_TRY(dmalloc(ctx, ccm_b, NC * sizeof(uint32_t)));
            CR_TRY(crgpu_memcpy_h2d(ctx, ccm_b.p, a->cell_class_mask, NC * sizeof(uint32_t)));
        }
        CR_TRY(dmalloc(ctx, mask_b, (uint64_t)n_bc * sizeof(uint32_t)));
    }
    uint32_t *kept = kept_b.as<uint32_t>();
    CrEvents<3> events(ctx);
    hipEvent_t *ev = events.e;
    CR_REQUIRE(ctx, ev[0] && ev[1] && ev[2], CRGPU_EHIP, "crgpu_normalize_depth_dev: no event");

    // 2. draw, 3. sums
    const NdTally ta{K, kept, fclass_b.as<uint8_t>(), mask_b.as<uint32_t>(), L.sh_bc(), n_bc, tab_b.as<uint32_t>(), sums_b.as<unsigned long long>()};
    {
        CrTimer t(ctx, CRGPU_T_DEDUP, nm);
        CR_HIP(ctx, hipMemsetAsync(sums_b.p, 0, ND_SUMS * sizeof(unsigned long long), ctx->stream));
        if (mask_b.p) {
            CR_HIP(ctx, hipMemsetAsync(mask_b.p, 0, (uint64_t)n_bc * sizeof(uint32_t), ctx->stream));
            hipLaunchKernelGGL(k_nd_cell_table, dim3(cr_grid(NC, 256)), dim3(256), 0, ctx->stream, a->d_cell_ranks, NC, ccm_b.as<uint32_t>(), c->d_back,
                               n_bc, mask_b.as<uint32_t>());
        }
        (void)hipEventRecord(ev[0], ctx->stream);
        hipLaunchKernelGGL(k_ss_draw_lane, dim3(cr_grid(nm, SS_THREADS, 256u * 16u)), dim3(SS_THREADS), 0, ctx->stream, K, thr_b.as<unsigned long long>(),
                           1u, wave_min, (unsigned long long)a->seed, kept);
        if (n_wave)
            hipLaunchKernelGGL(k_ss_draw_wave, dim3(cr_grid((uint64_t)n_wave * 64, SS_THREADS, 256u * 16u)), dim3(SS_THREADS), 0, ctx->stream, K, list,
                               n_wave, thr_b.as<unsigned long long>(), 1u, (unsigned long long)a->seed, kept);
        if (n_wg)
            hipLaunchKernelGGL(k_ss_draw_wg, dim3(std::min<uint32_t>(n_wg, 256u * 8u)), dim3(SS_THREADS), 0, ctx->stream, K, list + (nm - 1), n_wg,
                               thr_b.as<unsigned long long>(), 1u, (unsigned long long)a->seed, kept);
        (void)hipEventRecord(ev[1], ctx->stream);
        hipLaunchKernelGGL(k_nd_tally, dim3(cr_grid(nm, ND_THREADS)), dim3(ND_THREADS), 0, ctx->stream, ta);
        CR_HIP(ctx, hipGetLastError());
    }
    unsigned long long h_sums[ND_SUMS];
    CR_TRY(crgpu_memcpy_d2h(ctx, h_sums, sums_b.p, sizeof(h_sums)));
    uint64_t n_surv = 0;
    for (uint32_t l = 0; l < NL; l++) n_surv += h_sums[ND_SUM_MOLS + l];
    CR_REQUIRE(ctx, n_surv <= nm, CRGPU_EHIP, "crgpu_normalize_depth_dev: %llu survivors of %llu molecules", (unsigned long long)n_surv,
               (unsigned long long)nm);
    for (uint32_t k = 0; k < NK; k++) {
        if (a->raw_mapped_reads) a->raw_mapped_reads[k] = (int64_t)h_sums[ND_SUM_RAW + k];
        if (a->flt_mapped_reads) a->flt_mapped_reads[k] = (int64_t)h_sums[ND_SUM_FLT + k];
    }
    for (uint32_t l = 0; l < NL; l++) {
        if (a->reads_per_lib) a->reads_per_lib[l] = (int64_t)h_sums[ND_SUM_READS + l];
        if (a->kept_reads_per_lib) a->kept_reads_per_lib[l] = (int64_t)h_sums[ND_SUM_KEPT + l];
        if (a->kept_molecules_per_lib) a->kept_molecules_per_lib[l] = (int64_t)h_sums[ND_SUM_MOLS + l];
    }
    if (a->kept_out) CR_TRY(crgpu_memcpy_d2h(ctx, a->kept_out, d_pos ? tab_b.p : kept_b.p, nm * sizeof(uint32_t)));
    if (res) res->n_kept_molecules = n_surv;

    // 4. runs -> triplets -> matrix
    uint32_t nt = 0;
    if (a->matrix) {
        DevBuf pair_b, tbc_b, tft_b, tfi_b, tcn_b;
        CR_TRY(dmalloc(ctx, pair_b, n_surv * sizeof(uint64_t)));
        for (DevBuf *b : {&tbc_b, &tft_b, &tfi_b, &tcn_b}) CR_TRY(dmalloc(ctx, *b, n_surv * sizeof(uint32_t)));
        if (n_surv) {
            uint32_t ns = 0;
            {
                CrTimer t(ctx, CRGPU_T_DEDUP, nm);
                CR_TRY(compact(ctx, NdSurvFlag{kept}, NdEmitPair{c->d_mkeys, L.sh_feat(), pair_b.as<uint64_t>()}, nm, ctx->d_sort_hist, d_total));
            }
            CR_TRY(read_u32(ctx, d_total, &ns));
            CR_REQUIRE(ctx, ns == n_surv, CRGPU_EHIP, "crgpu_normalize_depth_dev: %u survivors compacted, %llu tallied", ns, (unsigned long long)n_surv);
            {
                CrTimer t(ctx, CRGPU_T_DEDUP, n_surv);
                CR_TRY(compact(ctx, NdHeadFlag{pair_b.as<uint64_t>()},
                               NdEmitTriplet{pair_b.as<uint64_t>(), L.bits_feat, c->d_back, c->n_back, tbc_b.as<uint32_t>(), tft_b.as<uint32_t>(),
                                             tfi_b.as<uint32_t>()},
                               n_surv, ctx->d_sort_hist, d_total));
            }
            CR_TRY(read_u32(ctx, d_total, &nt));
            CR_REQUIRE(ctx, nt >= 1 && nt <= n_surv, CRGPU_EHIP, "crgpu_normalize_depth_dev: %u triplets of %llu survivors", nt, (unsigned long long)n_surv);
            CrTimer t(ctx, CRGPU_T_DEDUP, nt);
            hipLaunchKernelGGL(k_nd_counts, dim3(cr_grid(nt, 256)), dim3(256), 0, ctx->stream, tfi_b.as<uint32_t>(), (uint64_t)nt, (uint32_t)n_surv,
                               tcn_b.as<uint32_t>());
            CR_HIP(ctx, hipGetLastError());
        }
        (void)hipEventRecord(ev[2], ctx->stream);
        CR_TRY(crgpu_assemble_matrix_dev(ctx, tbc_b.as<uint32_t>(), tft_b.as<uint32_t>(), tcn_b.as<uint32_t>(), nt, a->matrix));
    } else {
        (void)hipEventRecord(ev[2], ctx->stream);
    }
    if (res) {
        res->n_triplets = nt;
        float ms = 0.f;
        if (hipEventSynchronize(ev[2]) == hipSuccess) {
            if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) res->draw_ms = ms;
            if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) res->tally_ms = ms;
        }
    }
    return CRGPU_OK;
}

extern "C" int crgpu_normalize_depth_dev(crgpu_ctx *ctx, crgpu_counts *c, const crgpu_normalize_depth_args *a, crgpu_normalize_depth_result *res) {
    if (!ctx || !c || !a) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    if (res) memset(res, 0, sizeof(*res));
    if (a->matrix) *a->matrix = nullptr;
    const KeyLayout &L = c->layout;
    CR_REQUIRE(ctx, !c->sharded, CRGPU_ESTATE, "crgpu_normalize_depth_dev: the counts hold one rank's share of a sharded well");
    CR_REQUIRE(ctx, a->n_classes >= 1 && a->n_classes <= ND_MAX_CLASSES, CRGPU_EINVAL, "crgpu_normalize_depth_dev: n_classes must be 1..32");
    CR_REQUIRE(ctx, a->n_libs == L.n_libs && a->n_features == L.n_features, CRGPU_EINVAL,
               "crgpu_normalize_depth_dev: n_libs %u / n_features %u, the counts were made with %u / %u", a->n_libs, a->n_features, L.n_libs,
               L.n_features);
    CR_REQUIRE(ctx, a->frac_reads_kept, CRGPU_EINVAL, "crgpu_normalize_depth_dev: NULL frac_reads_kept");
    CR_REQUIRE(ctx, a->n_cells == 0 || a->d_cell_ranks, CRGPU_EINVAL, "crgpu_normalize_depth_dev: NULL cell ranks");
    CR_REQUIRE(ctx, a->n_cells < 0xFFFFFFFFull && c->n_molecules < 0xFFFFFFFFull, CRGPU_ERANGE, "crgpu_normalize_depth_dev: too many cells or molecules");
    CR_REQUIRE(ctx, !a->matrix || ctx->canon_set, CRGPU_ESTATE, "crgpu_normalize_depth_dev: no whitelist set");
    for (uint32_t l = 0; l < a->n_libs; l++) {
        const double r = a->frac_reads_kept[l];
        CR_REQUIRE(ctx, r >= 0.0 && r <= 1.0, CRGPU_EINVAL, "crgpu_normalize_depth_dev: frac_reads_kept[%u] = %g is not in [0, 1]", l, r);  // (a NaN fails both)
    }
    for (uint32_t f = 0; a->feature_class && f < a->n_features; f++)
        CR_REQUIRE(ctx, a->feature_class[f] < a->n_classes, CRGPU_EINVAL, "crgpu_normalize_depth_dev: feature %u belongs to class %u of %u", f,
                   a->feature_class[f], a->n_classes);
    const int rc = nd_run(ctx, c, a, res);
    if (rc != CRGPU_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // the temporaries go back to the pool behind this
        if (a->matrix && *a->matrix) {
            crgpu_matrix_dev_free(ctx, *a->matrix);
            *a->matrix = nullptr;
        }
    }
    return rc;
}

// ---- the rates of split() (normalize_depth/__init__.py:139-176), host --------------------------------------------------------------
extern "C" int crgpu_normalize_depth_plan(uint32_t n_libs, const uint32_t *library_type, const double *usable_reads, const double *num_cells,
                                          int downsample, int targeted_aggr, const uint8_t *is_targeted_lib, double targeted_depth_factor,
                                          double *frac_out) {
    if (!n_libs || !library_type || !usable_reads || !num_cells || !frac_out)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_normalize_depth_plan: NULL or empty argument");
    for (uint32_t i = 0; i < n_libs; i++)
        if (!std::isfinite(usable_reads[i]) || usable_reads[i] < 0.0 || !std::isfinite(num_cells[i]) || num_cells[i] < 0.0)
            return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_normalize_depth_plan: library %u has %g usable reads and %g cells", i, usable_reads[i],
                           num_cells[i]);
    if (targeted_aggr && (!std::isfinite(targeted_depth_factor) || targeted_depth_factor < 0.0))
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_normalize_depth_plan: targeted_depth_factor %g", targeted_depth_factor);
    if (!downsample) {
        std::fill(frac_out, frac_out + n_libs, 1.0);
        return CRGPU_OK;
    }
    std::vector<double> rpc(n_libs), frac(n_libs, 0.0);
    for (uint32_t i = 0; i < n_libs; i++) rpc[i] = num_cells[i] > 0.0 ? usable_reads[i] / num_cells[i] : 0.0;
    for (uint32_t i = 0; i < n_libs; i++) {
        double mn = rpc[i];  // the lowest depth of the library's type
        for (uint32_t j = 0; j < n_libs; j++)
            if (library_type[j] == library_type[i] && rpc[j] < mn) mn = rpc[j];
        if (mn != 0.0) frac[i] = mn / rpc[i];
    }
    if (targeted_aggr) {  // _adjust_frac_kept: all or nothing
        std::vector<double> adj(n_libs);
        bool fits = true;
        for (uint32_t i = 0; i < n_libs; i++) {
            adj[i] = ((is_targeted_lib && is_targeted_lib[i]) ? targeted_depth_factor : 1.0) * frac[i];
            fits = fits && adj[i] <= 1.0;
        }
        if (fits) frac = adj;
    }
    std::copy(frac.begin(), frac.end(), frac_out);
    return CRGPU_OK;
}

// ---- CountMatrix.select_features (matrix.py:886-894) for an ascending index list -----------------------------------------------------
// new_row[f] = position of row f among the kept rows, NONE32: dropped.  One wave per column; flag: a row >= n_features.
__global__ __launch_bounds__(256) void k_sf_count(const long long *__restrict__ indptr, const int32_t *__restrict__ indices, uint64_t V,
                                                  const uint32_t *__restrict__ new_row, uint32_t n_features, uint32_t *__restrict__ cnt,
                                                  uint32_t *__restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave0; c < V; c += n_waves) {
        const long long s = indptr[c], e = indptr[c + 1];
        uint32_t n = 0, bad = 0;
        for (long long i = s + lane; i < e; i += 64) {
            const uint32_t f = (uint32_t)indices[i];
            if (f >= n_features)
                bad = 1u;
            else
                n += new_row[f] != NONE32;
        }
        n = wave_sum(n), bad = wave_or(bad);
        if (lane == 0) {
            cnt[c] = n;
            if (bad) *flag = 1u;
        }
    }
}
// the kept entries of a column in their order (tiles of 64, a ballot per tile), rows renumbered; off = the scanned counts
__global__ __launch_bounds__(256) void k_sf_write(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                  const int32_t *__restrict__ data, uint64_t V, const uint32_t *__restrict__ new_row,
                                                  uint32_t n_features, const uint32_t *__restrict__ off, int32_t *__restrict__ io,
                                                  int32_t *__restrict__ dout) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave0; c < V; c += n_waves) {
        const long long s = indptr[c], e = indptr[c + 1];
        uint32_t o = off[c];
        for (long long base = s; base < e; base += 64) {
            const long long i = base + lane;
            const uint32_t f = i < e ? (uint32_t)indices[i] : NONE32;
            const uint32_t r = f < n_features ? new_row[f] : NONE32;
            const unsigned long long keep = __ballot(r != NONE32);
            if (r != NONE32) {
                const uint32_t at = o + (uint32_t)__popcll(keep & ((1ull << lane) - 1ull));
                io[at] = (int32_t)r;
                dout[at] = data[i];
            }
            o += (uint32_t)__popcll(keep);
        }
    }
}

extern "C" int crgpu_select_features_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint8_t *feature_mask, uint32_t n_features,
                                         crgpu_matrix_dev **out) {
    if (!ctx || !out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *out = nullptr;
    CR_REQUIRE(ctx, m && feature_mask && n_features, CRGPU_EINVAL, "crgpu_select_features_dev: NULL matrix or feature mask");
    const uint64_t V = m->n_barcodes;
    std::vector<uint32_t> new_row(n_features);
    uint32_t n_kept = 0;
    for (uint32_t f = 0; f < n_features; f++) new_row[f] = feature_mask[f] ? n_kept++ : NONE32;
    DevBuf row_b, cnt_b;
    CR_TRY(dmalloc(ctx, row_b, (uint64_t)n_features * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, row_b.p, new_row.data(), (uint64_t)n_features * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, cnt_b, (V + 1) * sizeof(uint32_t)));
    uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL, *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, total = 0, bad = 0;
    const long long *pa = (const long long *)m->d_indptr;
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
        CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
        if (V)
            hipLaunchKernelGGL(k_sf_count, dim3(cr_grid(V * 64, 256)), dim3(256), 0, ctx->stream, pa, m->d_indices, V, row_b.as<uint32_t>(), n_features,
                               cnt_b.as<uint32_t>(), d_flag);
        CR_HIP(ctx, hipGetLastError());
        CR_TRY(cr_scan_small(ctx, cnt_b.as<uint32_t>(), V, d_total));
    }
    CR_TRY(read_u32(ctx, d_flag, &bad));
    CR_REQUIRE(ctx, !bad, CRGPU_EINVAL, "crgpu_select_features_dev: the matrix holds a row >= n_features (%u)", n_features);
    CR_TRY(read_u32(ctx, d_total, &total));
    MatrixDevImpl *o = nullptr;
    CR_TRY(cr_new_matrix_dev(ctx, V, total, &o));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
        if (V) {
            CR_HIP(ctx, hipMemcpyAsync(o->d_rank, m->d_barcode_rank, V * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
            hipLaunchKernelGGL(k_sf_write, dim3(cr_grid(V * 64, 256)), dim3(256), 0, ctx->stream, pa, m->d_indices, m->d_data, V, row_b.as<uint32_t>(),
                               n_features, cnt_b.as<uint32_t>(), o->d_indices, o->d_data);
        }
        cr_offsets_to_indptr(ctx, cnt_b.as<uint32_t>(), V, total, o->d_indptr);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            crgpu_matrix_dev_free(ctx, &o->view);
            return cr_fail(ctx, CRGPU_EHIP, "crgpu_select_features_dev: kernel failed");
        }
    }
    *out = &o->view;
    return CRGPU_OK;
}
