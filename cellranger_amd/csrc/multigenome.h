// multigenome.h -- GEM classes, the multiplet bootstrap and the count purities of a multi-genome well on the device (part of
// matrix_stages.hip: the generator, the draw compaction, the batches and the row scan are those of cell_calling.h).
//
// Replaces MultiGenomeAnalysis.run_all (lib/python/cellranger/analysis/multigenome.py:251-335): classify_gems (:138-177),
// _infer_multiplets (:209-249), infer_multiplets_from_observed (:113-135) and the mean purities of compute_count_purity (:80-98).
// The purity-outlier diagnostics (:46-78, scipy's beta.fit / ppf) are NOT covered: a host computes them from c0, c1 and the call.
//
// The reference resamples the n cells 1000 times with np.random.choice(n, n) and runs classify_gems, two or three np.percentile
// calls and three masked sums, on every sample.  A sample only matters through the multiplicity of every cell, so here
//   1. the cells are put in ONE order: A = {c0 > c1} ascending by c0, then B = {c1 > c0} ascending by c1, then c0 == c1 (two
//      stable radix sorts: by the value, then by the class); place[cell] = its position, pc0 / pc1[p] = the counts at place p.  A
//      second order by c0 + c1 serves the fallback: sumv[q] = the q-th smallest sum, pp2[q] = the place of its cell.  The sums are
//      32-bit keys: a cell whose c0 + c1 does not fit is refused with CRGPU_ERANGE;
//   2. OmBootstrap (cell_calling.h) turns the generator's stream into h[sample][place] and scans every row: C[p] = sampled cells
//      at places <= p.  Batches, rounds and the draws of a round that belong to the next batch are its own;
//   3. k_mg_sample, one workgroup per sample: M_A = C[nA - 1], M_B = C[nA + nB - 1] - M_A; the order statistic k of the sampled A
//      cells is pc0[first p : C[p] >= k + 1] (four binary searches, one lane each); numpy's linear interpolation in f64; the
//      fold-change test; when it fires the multiplicities are gathered through pp2, scanned by the workgroup, and the two places
//      where the running sum crosses the wanted ranks give P10(c0 + c1); the three classes are counted with the multiplicities
//      as weights.  The row lives in LDS up to ctx->mg_lds_cells cells and is read from device memory beyond (the gather through
//      pp2 is the only access that is not sequential);
//   4. the unresampled input is a row of ones through the same kernel, which then also writes the call per barcode and the sums
//      of the purities; the summary of the samples is host f64 (crgpu_multigenome_summary).
// Multiplicities and their running sums are u32: a row sums to n < 2^31.  f64 is unfused (-ffp-contract=off, as everywhere).
#pragma once

#include <algorithm>
#include <cmath>

#include "cell_calling.h"
#include "stage_common.h"

// ---- per-genome totals of a device matrix ----------------------------------------------------------------------------------------
// flag: a row outside feature_genome
__global__ __launch_bounds__(256) void k_mg_genome_totals(const int32_t *__restrict__ indices, const int32_t *__restrict__ data, uint64_t nnz,
                                                          const uint8_t *__restrict__ feature_genome, uint32_t n_features, uint32_t n_genomes,
                                                          unsigned long long *__restrict__ totals, uint32_t *__restrict__ flag) {
    __shared__ unsigned long long s_tot[256];
    s_tot[threadIdx.x] = 0ull;
    __syncthreads();
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += stride) {
        const uint32_t f = (uint32_t)indices[i];
        if (f >= n_features) {
            *flag = 1u;
            continue;
        }
        const uint32_t g = feature_genome[f];
        if (g < n_genomes) atomicAdd(&s_tot[g], (unsigned long long)(uint32_t)data[i]);
    }
    __syncthreads();
    if (threadIdx.x < n_genomes && s_tot[threadIdx.x]) atomicAdd(&totals[threadIdx.x], s_tot[threadIdx.x]);
}

extern "C" int crgpu_matrix_dev_genome_totals(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const uint8_t *feature_genome, uint32_t n_features,
                                              uint32_t n_genomes, uint64_t *totals_out) {
    if (!ctx || !m) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_REQUIRE(ctx, n_genomes >= 1 && n_genomes <= 256 && totals_out, CRGPU_EINVAL, "crgpu_matrix_dev_genome_totals: 1 .. 256 genomes and an output");
    CR_REQUIRE(ctx, feature_genome || !n_features, CRGPU_EINVAL, "crgpu_matrix_dev_genome_totals: NULL feature_genome");
    memset(totals_out, 0, n_genomes * sizeof(uint64_t));
    if (!m->nnz) return CRGPU_OK;
    DevBuf fg_b, tot_b;
    CR_TRY(dmalloc(ctx, fg_b, n_features ? n_features : 1));
    if (n_features) CR_TRY(crgpu_memcpy_h2d(ctx, fg_b.p, feature_genome, n_features));
    CR_TRY(dmalloc(ctx, tot_b, 256 * sizeof(unsigned long long)));
    CR_HIP(ctx, hipMemsetAsync(tot_b.p, 0, 256 * sizeof(unsigned long long), ctx->stream));
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, m->nnz);
        hipLaunchKernelGGL(k_mg_genome_totals, dim3(cr_grid(m->nnz, 256)), dim3(256), 0, ctx->stream, m->d_indices, m->d_data, m->nnz,
                           fg_b.as<uint8_t>(), n_features, n_genomes, tot_b.as<unsigned long long>(), d_flag);
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !flag, CRGPU_EINVAL, "crgpu_matrix_dev_genome_totals: the matrix holds a row >= n_features (%u)", n_features);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "");
    return crgpu_memcpy_d2h(ctx, totals_out, tot_b.p, n_genomes * sizeof(uint64_t));
}

// ---- the two orders ------------------------------------------------------------------------------------------------------------
#define MG_SEG_A 0u  // c0 > c1
#define MG_SEG_B 1u  // c1 > c0
#define MG_SEG_E 2u  // c0 == c1: in neither percentile
__device__ __forceinline__ uint32_t mg_seg(uint32_t a, uint32_t b) { return a > b ? MG_SEG_A : b > a ? MG_SEG_B : MG_SEG_E; }

// key[i] = the value a cell is ordered by inside its class, sum[i] = c0 + c1; info[0] = nA, [1] = nB, [2] = a sum beyond 32 bits
__global__ __launch_bounds__(256) void k_mg_keys(const uint32_t *__restrict__ c0, const uint32_t *__restrict__ c1, uint32_t n,
                                                 uint32_t *__restrict__ key, uint32_t *__restrict__ sum, uint32_t *__restrict__ val,
                                                 uint32_t *__restrict__ val2, uint32_t *__restrict__ info) {
    const uint32_t stride = gridDim.x * blockDim.x;
    uint32_t nA = 0, nB = 0, over = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t a = c0[i], b = c1[i], s = mg_seg(a, b);
        key[i] = s == MG_SEG_A ? a : s == MG_SEG_B ? b : 0u;
        sum[i] = a + b;
        over |= (a + b < a) ? 1u : 0u;
        val[i] = i;
        val2[i] = i;
        nA += s == MG_SEG_A;
        nB += s == MG_SEG_B;
    }
    nA = wave_sum(nA), nB = wave_sum(nB), over = wave_or(over);
    if ((threadIdx.x & 63u) == 0) {
        if (nA) atomicAdd(&info[0], nA);
        if (nB) atomicAdd(&info[1], nB);
        if (over) atomicOr(&info[2], 1u);
    }
}
// the class of the cell at every place of the order by value: the key of the second, stable sort
__global__ __launch_bounds__(256) void k_mg_seg_keys(const uint32_t *__restrict__ val, const uint32_t *__restrict__ c0,
                                                     const uint32_t *__restrict__ c1, uint32_t n, uint32_t *__restrict__ key) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride) {
        const uint32_t i = val[j];
        key[j] = mg_seg(c0[i], c1[i]);
    }
}
__global__ __launch_bounds__(256) void k_mg_places(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ c0,
                                                   const uint32_t *__restrict__ c1, uint32_t n, uint32_t *__restrict__ place,
                                                   uint32_t *__restrict__ pc0, uint32_t *__restrict__ pc1) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
        const uint32_t i = perm[p];  // a permutation of 0 .. n-1
        place[i] = p;
        pc0[p] = c0[i];
        pc1[p] = c1[i];
    }
}
__global__ __launch_bounds__(256) void k_mg_sum_places(const uint32_t *__restrict__ perm2, const uint32_t *__restrict__ place, uint32_t n,
                                                       uint32_t *__restrict__ pp2) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < n; q += stride) pp2[q] = place[perm2[q]];
}

// ---- one sample per workgroup --------------------------------------------------------------------------------------------------
// np.percentile(x, 10.0) of M sorted values from its two order statistics (numpy's _lerp): v = (M - 1) * 0.1
__host__ __device__ __forceinline__ void mg_p10_ranks(uint32_t M, uint32_t *k_lo, uint32_t *k_hi, double *g) {
    const double v = (double)(M - 1u) * 0.1, fl = floor(v);
    *k_lo = (uint32_t)fl;
    *k_hi = *k_lo + 1u < M ? *k_lo + 1u : M - 1u;
    *g = v - fl;
}

#define MG_ITEMS 8
// C_all[rows][n]: the scanned multiplicities of the samples of one batch, in place order.  Outputs per sample (row index + the
// pointers' offsets): counts[3] = Multiplets, genome0, genome1; thr[2]; branch.  OBS (one row of ones): also call_out[cell]
// and sums[4] = sum of c0 / c1 over genome0, of c0 / c1 over genome1.
template <bool LDS, bool OBS>
__global__ __launch_bounds__(256) void k_mg_sample(const uint32_t *__restrict__ C_all, uint32_t n, uint32_t nA, uint32_t nB,
                                                   const uint32_t *__restrict__ pc0, const uint32_t *__restrict__ pc1,
                                                   const uint32_t *__restrict__ sumv, const uint32_t *__restrict__ pp2,
                                                   const uint32_t *__restrict__ perm, long long *__restrict__ counts_out,
                                                   double *__restrict__ thr_out, int32_t *__restrict__ branch_out,
                                                   unsigned long long *__restrict__ sums_out, uint8_t *__restrict__ call_out) {
    extern __shared__ uint32_t mg_row[];  // LDS: n words
    __shared__ uint32_t s_stat[4];        // the four order statistics: A lo, A hi, B lo, B hi
    __shared__ double s_thr[2];
    __shared__ int32_t s_branch;
    __shared__ uint32_t s_ws[4], s_carry, s_sumstat[2];
    __shared__ unsigned long long s_red[4][7];
    const uint32_t *row = C_all + (uint64_t)blockIdx.x * n;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (LDS) {
        for (uint32_t i = tid; i < n; i += 256) mg_row[i] = row[i];
        __syncthreads();
    }
    auto C = [&](uint32_t p) -> uint32_t { return LDS ? mg_row[p] : row[p]; };
    auto mult = [&](uint32_t p) -> uint32_t { return C(p) - (p ? C(p - 1u) : 0u); };

    const uint32_t MA = nA ? C(nA - 1u) : 0u, MB = (nA + nB) ? C(nA + nB - 1u) - MA : 0u;
    const bool both = MA && MB;  // uniform
    double gA = 0.0, gB = 0.0;
    if (both) {
        uint32_t kA[2], kB[2];
        mg_p10_ranks(MA, &kA[0], &kA[1], &gA);
        mg_p10_ranks(MB, &kB[0], &kB[1], &gB);
        if (tid < 4) {  // the first place of the segment with C >= target: it exists, C at the segment's end is target's bound
            const bool inB = tid >= 2;
            const uint32_t target = (inB ? MA + kB[tid & 1u] : kA[tid & 1u]) + 1u;
            uint32_t lo = inB ? nA : 0u, hi = (inB ? nA + nB : nA) - 1u;
            while (lo < hi) {
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (C(mid) >= target) hi = mid; else lo = mid + 1u;
            }
            s_stat[tid] = inB ? pc1[lo] : pc0[lo];
        }
    }
    __syncthreads();
    if (tid == 0) {
        double t0 = 10.0, t1 = 10.0;  // DEFAULT_MULTIPLET_THRESHOLD
        int32_t br = CRGPU_MG_BRANCH_DEFAULT;
        if (both) {
            t0 = cr_lerp((double)s_stat[0], (double)s_stat[1], gA);
            t1 = cr_lerp((double)s_stat[2], (double)s_stat[3], gB);
            br = CRGPU_MG_BRANCH_PERCENTILES;
        }
        const double lo = t0 < t1 ? t0 : t1, hi = t0 < t1 ? t1 : t0;
        if (lo < 50.0 && hi / lo > 25.0) br |= 2;  // (lo >= 1: a percentile of A or B is at least 1, the default is 10)
        s_thr[0] = t0;
        s_thr[1] = t1;
        s_branch = br;
        s_carry = 0u;
        s_sumstat[0] = s_sumstat[1] = 0u;
    }
    __syncthreads();
    if (s_branch & 2) {  // uniform: P10 of c0 + c1 over the whole sample, in the order by the sum
        const uint32_t M = C(n - 1u);  // == n
        uint32_t k[2];
        double g;
        mg_p10_ranks(M, &k[0], &k[1], &g);
        for (uint32_t base = 0; base < n; base += 256 * MG_ITEMS) {
            const uint32_t q0 = base + tid * MG_ITEMS;
            uint32_t v[MG_ITEMS], sum = 0;
#pragma unroll
            for (int j = 0; j < MG_ITEMS; j++) {
                sum += q0 + j < n ? mult(pp2[q0 + j]) : 0u;
                v[j] = sum;
            }
            const uint32_t x = wave_incl_scan(sum, lane);
            if (lane == 63) s_ws[wave] = x;
            __syncthreads();
            uint32_t pre = s_carry + x - sum, tot = 0;
            for (uint32_t w = 0; w < 4; w++) {
                if (w < wave) pre += s_ws[w];
                tot += s_ws[w];
            }
            uint32_t before = pre;  // sampled cells ahead of item j
#pragma unroll
            for (int j = 0; j < MG_ITEMS; j++) {
                const uint32_t upto = pre + v[j];
                if (q0 + j < n) {
#pragma unroll
                    for (int r = 0; r < 2; r++)
                        if (before <= k[r] && k[r] < upto) s_sumstat[r] = sumv[q0 + j];  // one item holds rank k[r]
                }
                before = upto;
            }
            __syncthreads();
            if (tid == 0) s_carry += tot;
            __syncthreads();
            if (s_carry > k[1]) break;  // uniform: both ranks are behind
        }
        if (tid == 0) s_thr[0] = s_thr[1] = cr_lerp((double)s_sumstat[0], (double)s_sumstat[1], g);
        __syncthreads();
    }
    const double t0 = s_thr[0], t1 = s_thr[1];
    unsigned long long acc[7] = {0, 0, 0, 0, 0, 0, 0};  // the three classes, then the four purity sums
    for (uint32_t p = tid; p < n; p += 256) {
        const uint32_t w = mult(p);
        if (!OBS && !w) continue;
        const uint32_t a = pc0[p], b = pc1[p];
        const uint32_t cls = ((double)a >= t0 && (double)b >= t1) ? 2u : b > a ? 1u : 0u;
        acc[cls == 2u ? 0 : cls == 0u ? 1 : 2] += w;
        if (OBS) {
            if (call_out) call_out[perm[p]] = (uint8_t)cls;
            if (cls == 0u) {
                acc[3] += a;
                acc[4] += b;
            } else if (cls == 1u) {
                acc[5] += a;
                acc[6] += b;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < (OBS ? 7 : 3); r++) {
        acc[r] = wave_sum(acc[r]);
        if (lane == 0) s_red[wave][r] = acc[r];
    }
    __syncthreads();
    if (tid == 0) {
        for (int r = 0; r < 3; r++) counts_out[(uint64_t)blockIdx.x * 3 + r] = (long long)(s_red[0][r] + s_red[1][r] + s_red[2][r] + s_red[3][r]);
        thr_out[(uint64_t)blockIdx.x * 2] = t0;
        thr_out[(uint64_t)blockIdx.x * 2 + 1] = t1;
        branch_out[blockIdx.x] = s_branch;
        if (OBS)
            for (int r = 0; r < 4; r++) sums_out[r] = s_red[0][3 + r] + s_red[1][3 + r] + s_red[2][3 + r] + s_red[3][3 + r];
    }
}

// ---- the summary of the samples (host, f64) ------------------------------------------------------------------------------------
// infer_multiplets_from_observed (:113-135)
static double mg_infer(int64_t m, int64_t g0, int64_t g1) {
    if (g0 == 0 || g1 == 0) return 0.0;
    const double tot = (double)(g0 + g1);
    const double p = 2.0 * ((double)g0 / tot) * ((double)g1 / tot);
    const double mle = (double)m / p, cap = (double)(m + g0 + g1);
    return cap < mle ? cap : mle;
}

extern "C" int crgpu_multigenome_summary(const int64_t *boot_counts, uint32_t bootstraps, uint64_t n, double *boot_out,
                                         crgpu_multigenome_result *res) {
    if (!boot_counts || !res || bootstraps < 1 || bootstraps > CRGPU_MULTIGENOME_MAX_BOOTSTRAPS)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_multigenome_summary: boot_counts, res and 1 .. %d bootstraps", CRGPU_MULTIGENOME_MAX_BOOTSTRAPS);
    std::vector<double> boot(bootstraps);
    for (uint32_t s = 0; s < bootstraps; s++) boot[s] = mg_infer(boot_counts[3 * s], boot_counts[3 * s + 1], boot_counts[3 * s + 2]);
    if (boot_out) std::copy(boot.begin(), boot.end(), boot_out);
    const double mean = cr_pairwise_sum(boot.data(), bootstraps) / (double)bootstraps, dn = (double)n;
    res->n = n;
    res->boot_mean = mean;
    res->inferred_multiplets = (int64_t)std::nearbyint(mean);  // round(): half to even
    res->multiplet_rate = cr_robust_divide(mean, dn);
    res->normalized_multiplet_rate = 1000.0 * cr_robust_divide(res->multiplet_rate, dn);
    res->multiplet_rate_lb = res->multiplet_rate_ub = 0.0;
    res->rate_bounds_set = bootstraps > 1;
    if (bootstraps > 1) {
        std::sort(boot.begin(), boot.end());
        res->multiplet_rate_lb = cr_robust_divide(cr_quantile_sorted(boot, 2.5 / 100.0), dn);
        res->multiplet_rate_ub = cr_robust_divide(cr_quantile_sorted(boot, 97.5 / 100.0), dn);
    }
    return CRGPU_OK;
}

// ---- the entry point -----------------------------------------------------------------------------------------------------------
struct MgOrder {
    uint32_t n, nA, nB;
    const uint32_t *pc0, *pc1, *sumv, *pp2, *perm;
};
template <bool OBS>
static int mg_launch(crgpu_ctx *ctx, const MgOrder &o, const uint32_t *d_C, uint32_t rows, long long *d_counts, double *d_thr, int32_t *d_branch,
                     unsigned long long *d_sums, uint8_t *d_call) {
    CrTimer t(ctx, CRGPU_T_MATRIX, (uint64_t)rows * o.n);  // (the ledger's slots are fixed: the 32-bit sorts above report under DEDUP)
    if (o.n <= ctx->mg_lds_cells) {
        const size_t lds = (size_t)o.n * sizeof(uint32_t);
        cr_allow_lds(ctx, (const void *)k_mg_sample<true, OBS>, lds);
        hipLaunchKernelGGL((k_mg_sample<true, OBS>), dim3(rows), dim3(256), lds, ctx->stream, d_C, o.n, o.nA, o.nB, o.pc0, o.pc1, o.sumv, o.pp2,
                           o.perm, d_counts, d_thr, d_branch, d_sums, d_call);
    } else {
        hipLaunchKernelGGL((k_mg_sample<false, OBS>), dim3(rows), dim3(256), 0, ctx->stream, d_C, o.n, o.nA, o.nB, o.pc0, o.pc1, o.sumv, o.pp2,
                           o.perm, d_counts, d_thr, d_branch, d_sums, d_call);
    }
    CR_HIP(ctx, hipGetLastError());
    return CRGPU_OK;
}

extern "C" int crgpu_multigenome_dev(crgpu_ctx *ctx, const uint32_t *d_counts0, const uint32_t *d_counts1, uint64_t n64, uint32_t bootstraps,
                                     uint8_t *d_call_out, int64_t *boot_counts_out, double *boot_thresholds_out, int32_t *boot_branch_out,
                                     crgpu_multigenome_result *res) {
    if (!ctx || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    memset(res, 0, sizeof(*res));
    CR_REQUIRE(ctx, bootstraps >= 1 && bootstraps <= CRGPU_MULTIGENOME_MAX_BOOTSTRAPS, CRGPU_EINVAL,
               "crgpu_multigenome_dev: bootstraps must be 1 .. %d", CRGPU_MULTIGENOME_MAX_BOOTSTRAPS);
    CR_REQUIRE(ctx, boot_counts_out != nullptr, CRGPU_EINVAL, "crgpu_multigenome_dev: NULL boot_counts_out");
    CR_REQUIRE(ctx, n64 < 0x80000000ull, CRGPU_ERANGE, "crgpu_multigenome_dev: at most 2^31 - 1 barcodes");
    if (!n64) return CRGPU_OK;  // "Don't compute multiplet / purity metrics if no cells detected"
    CR_REQUIRE(ctx, d_counts0 && d_counts1, CRGPU_EINVAL, "crgpu_multigenome_dev: NULL counts");
    const uint32_t n = (uint32_t)n64, B = bootstraps;

    // 1. the order by class and value, the order by the sum
    DevBuf key_b, keyt_b, val_b, valt_b, sum_b, sumt_b, val2_b, val2t_b, place_b, pc0_b, pc1_b, pp2_b, info_b;
    for (DevBuf *b : {&key_b, &keyt_b, &val_b, &valt_b, &sum_b, &sumt_b, &val2_b, &val2t_b, &place_b, &pc0_b, &pc1_b, &pp2_b})
        CR_TRY(dmalloc(ctx, *b, (uint64_t)n * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, info_b, 4 * sizeof(uint32_t)));
    CR_HIP(ctx, hipMemsetAsync(info_b.p, 0, 4 * sizeof(uint32_t), ctx->stream));
    const dim3 grid(cr_grid(n, 256)), block(256);
    hipLaunchKernelGGL(k_mg_keys, grid, block, 0, ctx->stream, d_counts0, d_counts1, n, key_b.as<uint32_t>(), sum_b.as<uint32_t>(),
                       val_b.as<uint32_t>(), val2_b.as<uint32_t>(), info_b.as<uint32_t>());
    CR_HIP(ctx, hipGetLastError());
    uint32_t info[4] = {0, 0, 0, 0};
    CR_TRY(crgpu_memcpy_d2h(ctx, info, info_b.p, sizeof(info)));
    CR_REQUIRE(ctx, !info[2], CRGPU_ERANGE, "crgpu_multigenome_dev: c0 + c1 of a barcode does not fit 32 bits");
    MgOrder o{};
    o.n = n, o.nA = info[0], o.nB = info[1];
    {
        bool in_tmp = false;
        CR_TRY(cr_radix_sort_u32(ctx, key_b.as<uint32_t>(), keyt_b.as<uint32_t>(), val_b.as<uint32_t>(), valt_b.as<uint32_t>(), n, 0, 32, &in_tmp));
        uint32_t *v = in_tmp ? valt_b.as<uint32_t>() : val_b.as<uint32_t>(), *vt = in_tmp ? val_b.as<uint32_t>() : valt_b.as<uint32_t>();
        uint32_t *k = in_tmp ? keyt_b.as<uint32_t>() : key_b.as<uint32_t>(), *kt = in_tmp ? key_b.as<uint32_t>() : keyt_b.as<uint32_t>();
        hipLaunchKernelGGL(k_mg_seg_keys, grid, block, 0, ctx->stream, v, d_counts0, d_counts1, n, k);
        CR_HIP(ctx, hipGetLastError());
        CR_TRY(cr_radix_sort_u32(ctx, k, kt, v, vt, n, 0, 2, &in_tmp));
        o.perm = in_tmp ? vt : v;
        hipLaunchKernelGGL(k_mg_places, grid, block, 0, ctx->stream, o.perm, d_counts0, d_counts1, n, place_b.as<uint32_t>(),
                           pc0_b.as<uint32_t>(), pc1_b.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
        o.pc0 = pc0_b.as<uint32_t>(), o.pc1 = pc1_b.as<uint32_t>();
        CR_TRY(cr_radix_sort_u32(ctx, sum_b.as<uint32_t>(), sumt_b.as<uint32_t>(), val2_b.as<uint32_t>(), val2t_b.as<uint32_t>(), n, 0, 32, &in_tmp));
        o.sumv = in_tmp ? sumt_b.as<uint32_t>() : sum_b.as<uint32_t>();
        hipLaunchKernelGGL(k_mg_sum_places, grid, block, 0, ctx->stream, in_tmp ? val2t_b.as<uint32_t>() : val2_b.as<uint32_t>(),
                           place_b.as<uint32_t>(), n, pp2_b.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
        o.pp2 = pp2_b.as<uint32_t>();
    }

    // outputs of the per-sample kernel: row B is the unresampled input
    DevBuf cnt_b, thr_b, br_b, sums_b;
    CR_TRY(dmalloc(ctx, cnt_b, (uint64_t)(B + 1) * 3 * sizeof(long long)));
    CR_TRY(dmalloc(ctx, thr_b, (uint64_t)(B + 1) * 2 * sizeof(double)));
    CR_TRY(dmalloc(ctx, br_b, (uint64_t)(B + 1) * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, sums_b, 4 * sizeof(unsigned long long)));
    long long *d_cnt = cnt_b.as<long long>();
    double *d_thr = thr_b.as<double>();
    int32_t *d_br = br_b.as<int32_t>();

    // 2. the samples, batch by batch
    OmBootstrap boot{ctx};
    boot.batch_cap = CRGPU_MULTIGENOME_MAX_BOOTSTRAPS;
    boot.batch_forced = ctx->mg_batch;
    boot.timed = true;
    boot.who = "multigenome";
    CR_TRY(boot.init(n, B, place_b.as<uint32_t>(), nullptr));
    for (uint32_t s0 = 0; s0 < B; s0 += boot.B) {
        const uint32_t s1 = std::min<uint32_t>(B, s0 + boot.B);
        CR_TRY(boot.fill(s0, s1));
        CR_TRY(mg_launch<false>(ctx, o, boot.hist.as<uint32_t>(), s1 - s0, d_cnt + (uint64_t)s0 * 3, d_thr + (uint64_t)s0 * 2, d_br + s0, nullptr,
                                nullptr));
    }
    // 3. the unresampled input: every multiplicity is 1 (the first row of the batch buffer is free again: one in-order stream)
    hipLaunchKernelGGL(k_om_fill, dim3(cr_grid(n, 256)), dim3(256), 0, ctx->stream, boot.hist.as<uint32_t>(), (uint64_t)n, 1u);
    CR_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_om_row_scan, dim3(1), dim3(256), 0, ctx->stream, boot.hist.as<uint32_t>(), n);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(mg_launch<true>(ctx, o, boot.hist.as<uint32_t>(), 1, d_cnt + (uint64_t)B * 3, d_thr + (uint64_t)B * 2, d_br + B,
                           sums_b.as<unsigned long long>(), d_call_out));

    std::vector<int64_t> h_cnt((size_t)(B + 1) * 3);
    std::vector<double> h_thr((size_t)(B + 1) * 2);
    std::vector<int32_t> h_br(B + 1);
    unsigned long long h_sums[4];
    static_assert(sizeof(long long) == sizeof(int64_t), "");
    CR_TRY(crgpu_memcpy_d2h(ctx, h_cnt.data(), d_cnt, h_cnt.size() * sizeof(int64_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, h_thr.data(), d_thr, h_thr.size() * sizeof(double)));
    CR_TRY(crgpu_memcpy_d2h(ctx, h_br.data(), d_br, h_br.size() * sizeof(int32_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, h_sums, sums_b.p, sizeof(h_sums)));
    std::copy(h_cnt.begin(), h_cnt.begin() + (size_t)B * 3, boot_counts_out);
    if (boot_thresholds_out) std::copy(h_thr.begin(), h_thr.begin() + (size_t)B * 2, boot_thresholds_out);
    if (boot_branch_out) std::copy(h_br.begin(), h_br.begin() + B, boot_branch_out);
    for (uint32_t s = 0; s <= B; s++)
        CR_REQUIRE(ctx, h_cnt[3 * s] + h_cnt[3 * s + 1] + h_cnt[3 * s + 2] == (int64_t)n, CRGPU_EHIP,
                   "multigenome: sample %u holds %lld of %u barcodes", s, (long long)(h_cnt[3 * s] + h_cnt[3 * s + 1] + h_cnt[3 * s + 2]), n);

    res->obs_thresh0 = h_thr[(size_t)B * 2];
    res->obs_thresh1 = h_thr[(size_t)B * 2 + 1];
    res->obs_branch = h_br[B];
    res->observed_multiplets = h_cnt[(size_t)B * 3];
    res->observed_genome0 = h_cnt[(size_t)B * 3 + 1];
    res->observed_genome1 = h_cnt[(size_t)B * 3 + 2];
    res->sum_c0_genome0 = h_sums[0];
    res->sum_all_genome0 = h_sums[0] + h_sums[1];
    res->sum_c1_genome1 = h_sums[3];
    res->sum_all_genome1 = h_sums[2] + h_sums[3];
    res->sum_max_single = h_sums[0] + h_sums[3];  // genome0: c0 >= c1, genome1: c1 > c0
    res->sum_all_single = res->sum_all_genome0 + res->sum_all_genome1;
    res->purity0 = cr_robust_divide((double)res->sum_c0_genome0, (double)res->sum_all_genome0);
    res->purity1 = cr_robust_divide((double)res->sum_c1_genome1, (double)res->sum_all_genome1);
    res->purity_overall = cr_robust_divide((double)res->sum_max_single, (double)res->sum_all_single);
    res->generator_words = boot.words_made;
    return crgpu_multigenome_summary(boot_counts_out, B, n, nullptr, res);
}
