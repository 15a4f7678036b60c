// perturbations.h -- the bootstrap of MEASURE_PERTURBATIONS on a plan of sseq_pair.h (part of matrix_stages.hip).
//
// lib/python/cellranger/feature/crispr/measure_perturbations.py tests every perturbation against the Non-Targeting cells with local sSeq
// parameters (crgpu_sseq_pair_dev) and then, for every (perturbation, target gene), draws 500 bootstrap samples in _get_fold_change_cis
// (:504-540): both sides' cells are resampled with replacement, the target gene's counts are summed over each resample, and the 5th and
// 95th percentile of the log2 fold changes are the confidence interval.  Here the sums of all draws of all (perturbation, target) items
// come from two kernels over the plan's transposed entries:
//
// k_pb_gather   a wave per distinct (gene, group): the gene's run inside the group is found with the two searches of k_sq_pair_row_sums
//               and written out as a dense u32[n] column, n = the cells of the group.  A lane that holds entry i writes the zeros
//               between entry i - 1 and entry i and then the value, one more lane writes the zeros behind the last entry: every word
//               of the column is written exactly once, nothing is filled beforehand.  The host lists each (gene, group) once, so the
//               control column of a target gene is gathered once however many perturbations share the target.
// k_pb_draws    a 256-thread workgroup per (item, side, chunk of draws_per_wg draws).  The dense column is staged into dynamic LDS when
//               n <= lds_cells, otherwise it is read from global memory (a few hundred KiB: it stays in L2).  A wave takes whole draws;
//               a lane takes the Philox blocks lane, lane + 64, ... of the draw, four positions per block, and of the last block only
//               the n & 3 words that are positions.  u64 accumulation, wave_sum, lane 0 stores the sum.  No atomics.
// THE STREAM (the reference draws from the unseeded global np.random: there is no stream to reproduce): position q of draw b of side z
// (0 = a, 1 = b) of an item takes the cell at index __umul64hi(w, n) of the side's cells in the plan's (group, cell) order, w = word
// q & 3 of Philox4x64-10(counter = (1 + (q >> 2), s, 0, 0), key = (seed, 0)), s = (stream << 33) | (z << 32) | b: element q of
// np.random.Philox(counter=[0, s, 0, 0], key=[seed, 0]).random_raw().  The multiply-high is biased by less than n / 2^64.  Integer sums
// do not depend on the order of addition, so a sum is a pure function of (plan, item, seed, n_bootstraps) and equal means equal.
#pragma once

#include <algorithm>
#include <map>

#include "philox.h"
#include "sseq_pair.h"

#define PB_DEFAULT_BOOTSTRAPS 500u
#define PB_MAX_BOOTSTRAPS 65536u
#define PB_LDS_BYTES (160u * 1024u)
#define PB_MAX_LDS_CELLS (PB_LDS_BYTES / 4u)  // 40960
#define PB_DEFAULT_LDS_CELLS 16384u           // 64 KiB: two workgroups per CU
#define PB_DEFAULT_DRAWS_PER_WG 8u

struct PbCol {       // a distinct (gene, group)
    uint32_t gene;
    uint32_t lo, hi;  // the group's cells in pos
    uint32_t reserved;
    uint64_t off;     // the column's first word in the pool buffer
};
struct PbTask {      // one side of one item
    uint64_t off;     // its dense column
    uint64_t s;       // (stream << 33) | (z << 32)
    uint32_t n;       // the cells of the side
    uint32_t out_row; // the sums go to out[out_row * B + b]
};

// A wave per column: the gene's entries inside the group as a dense column, every word written once.
__global__ __launch_bounds__(SQ_WG) void k_pb_gather(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t nnz, uint64_t Npos,
                                                     const PbCol *__restrict__ cols, uint32_t n_cols, uint32_t *__restrict__ pool) {
    const uint32_t c = (blockIdx.x * SQ_WG + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (c >= n_cols) return;  // uniform over the wave
    const PbCol col = cols[c];
    const uint32_t n = col.hi - col.lo;
    const uint64_t k0 = (uint64_t)col.gene * Npos;
    const uint64_t glo = cr_lower_bound(keys, nnz, k0), ghi = glo + cr_lower_bound(keys + glo, nnz - glo, k0 + Npos);
    const uint64_t lo = glo + cr_lower_bound(keys + glo, ghi - glo, k0 + col.lo), hi = lo + cr_lower_bound(keys + lo, ghi - lo, k0 + col.hi);
    uint32_t *__restrict__ out = pool + col.off;
    for (uint64_t i = lo + lane; i <= hi; i += 64u) {  // i == hi: the zeros behind the last entry
        const uint32_t from = i > lo ? (uint32_t)(keys[i - 1] - k0 - col.lo) + 1u : 0u;
        const uint32_t to = i < hi ? (uint32_t)(keys[i] - k0 - col.lo) : n;
        for (uint32_t p = from; p < to; p++) out[p] = 0u;
        if (i < hi) out[to] = vals[i];
    }
}

// A workgroup per (task, chunk of draws): the sum of the column over every draw's resample.
template <bool LDS>
__global__ __launch_bounds__(256) void k_pb_draws(const uint32_t *__restrict__ pool, const PbTask *__restrict__ tasks, uint32_t B, uint32_t draws_per_wg,
                                                  uint32_t chunks, uint64_t seed, unsigned long long *__restrict__ out) {
    extern __shared__ uint32_t pb_col[];  // LDS: n words
    const PbTask t = tasks[blockIdx.x / chunks];
    const uint32_t chunk = blockIdx.x % chunks, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n = t.n;
    const uint32_t *__restrict__ col = pool + t.off;
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < n; i += 256u) pb_col[i] = col[i];
        __syncthreads();
    }
    const uint32_t b_end = min(B, (chunk + 1u) * draws_per_wg), n_blocks = (n + 3u) >> 2;
    for (uint32_t b = chunk * draws_per_wg + wave; b < b_end; b += 4u) {  // uniform over the wave
        unsigned long long acc = 0ull;
        for (uint32_t j = lane; j < n_blocks; j += 64u) {
            unsigned long long w[4];
            cr_philox4x64_10(1ull + j, t.s | b, seed, w);
            const uint32_t words = min(4u, n - 4u * j);
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++)
                if (k < words) {
                    const uint32_t idx = (uint32_t)__umul64hi(w[k], (unsigned long long)n);
                    acc += LDS ? pb_col[idx] : col[idx];
                }
        }
        acc = wave_sum(acc);
        if (lane == 0u) out[(uint64_t)t.out_row * B + b] = acc;
    }
}

// the tasks whose column fits lds_cells first (a task's place decides nothing: its output row does) -> their number
static uint32_t pb_order_tasks(std::vector<PbTask> &tasks, uint32_t lds_cells) {
    return (uint32_t)(std::stable_partition(tasks.begin(), tasks.end(), [&](const PbTask &t) { return t.n <= lds_cells; }) - tasks.begin());
}
// launch only: the first n_lds tasks through the LDS kernel, the others through the global one; d_tasks holds `tasks` as ordered by
// pb_order_tasks, each launch gets its part of the array
static int pb_launch_draws(crgpu_ctx *ctx, const uint32_t *d_pool, const PbTask *d_tasks, const std::vector<PbTask> &tasks, uint32_t n_lds, uint32_t B,
                           uint32_t draws_per_wg, uint64_t seed, unsigned long long *d_out) {
    const uint32_t chunks = (B + draws_per_wg - 1u) / draws_per_wg, n_tasks = (uint32_t)tasks.size();
    CR_REQUIRE(ctx, (uint64_t)n_tasks * chunks < (1ull << 31), CRGPU_ERANGE, "crgpu_sseq_pair_bootstrap_dev: %u sides x %u chunks of draws, below 2^31 workgroups",
               n_tasks, chunks);
    uint64_t draws = 0;
    for (const PbTask &t : tasks) draws += (uint64_t)t.n * B;
    CrTimer timer(ctx, CRGPU_T_MATRIX, draws);
    if (n_lds) {
        uint32_t n_max = 0;
        for (uint32_t i = 0; i < n_lds; i++) n_max = std::max(n_max, tasks[i].n);
        const size_t lds = (size_t)n_max * sizeof(uint32_t);
        cr_allow_lds(ctx, (const void *)k_pb_draws<true>, lds);
        hipLaunchKernelGGL(k_pb_draws<true>, dim3(n_lds * chunks), dim3(256), lds, ctx->stream, d_pool, d_tasks, B, draws_per_wg, chunks, seed, d_out);
        CR_HIP(ctx, hipGetLastError());
    }
    if (n_tasks > n_lds) {
        hipLaunchKernelGGL(k_pb_draws<false>, dim3((n_tasks - n_lds) * chunks), dim3(256), 0, ctx->stream, d_pool, d_tasks + n_lds, B, draws_per_wg, chunks, seed,
                           d_out);
        CR_HIP(ctx, hipGetLastError());
    }
    return CRGPU_OK;
}

extern "C" int crgpu_sseq_pair_bootstrap_dev(crgpu_ctx *ctx, const crgpu_sseq_pairs *pl, const crgpu_pb_item *items, uint32_t n_items, const crgpu_pb_args *a,
                                             uint64_t *sums_a_out, uint64_t *sums_b_out) {
    if (!ctx || !pl || !items || !a || !sums_a_out || !sums_b_out || n_items == 0) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const uint32_t G = pl->n_features;
    CR_REQUIRE(ctx, a->n_bootstraps <= PB_MAX_BOOTSTRAPS, CRGPU_EINVAL, "crgpu_sseq_pair_bootstrap_dev: %u bootstraps, at most %u", a->n_bootstraps, PB_MAX_BOOTSTRAPS);
    CR_REQUIRE(ctx, a->lds_cells <= PB_MAX_LDS_CELLS, CRGPU_EINVAL, "crgpu_sseq_pair_bootstrap_dev: lds_cells %u, 160 KiB hold %u", a->lds_cells, PB_MAX_LDS_CELLS);
    CR_REQUIRE(ctx, n_items < (1u << 30), CRGPU_EINVAL, "crgpu_sseq_pair_bootstrap_dev: %u items, below 2^30", n_items);
    for (uint32_t i = 0; i < n_items; i++) {
        const crgpu_pb_item &it = items[i];
        CR_REQUIRE(ctx, it.gene < G, CRGPU_EINVAL, "crgpu_sseq_pair_bootstrap_dev: gene %u of item %u, the plan has %u features", it.gene, i, G);
        CR_REQUIRE(ctx, it.group_a < pl->n_groups && it.group_b < pl->n_groups, CRGPU_EINVAL, "crgpu_sseq_pair_bootstrap_dev: groups %u and %u of item %u, the plan has %u groups",
                   it.group_a, it.group_b, i, pl->n_groups);
        CR_REQUIRE(ctx, it.group_a != it.group_b, CRGPU_EINVAL, "crgpu_sseq_pair_bootstrap_dev: group %u is on both sides of item %u", it.group_a, i);
    }
    const uint32_t B = a->n_bootstraps ? a->n_bootstraps : PB_DEFAULT_BOOTSTRAPS;
    const uint32_t lds_cells = a->lds_cells ? a->lds_cells : PB_DEFAULT_LDS_CELLS;
    const uint32_t draws_per_wg = a->draws_per_wg ? a->draws_per_wg : PB_DEFAULT_DRAWS_PER_WG;

    // every (gene, group) once
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> col_of;
    std::vector<PbCol> cols;
    uint64_t pool_words = 0;
    std::vector<PbTask> tasks;
    for (uint32_t i = 0; i < n_items; i++)
        for (uint32_t z = 0; z < 2u; z++) {
            const uint32_t k = z ? items[i].group_b : items[i].group_a;
            auto ins = col_of.emplace(std::make_pair(items[i].gene, k), (uint32_t)cols.size());
            if (ins.second) {
                cols.push_back(PbCol{items[i].gene, pl->gstart[k], pl->gstart[k + 1u], 0u, pool_words});
                pool_words += pl->gstart[k + 1u] - pl->gstart[k];
            }
            const PbCol &c = cols[ins.first->second];
            tasks.push_back(PbTask{c.off, ((uint64_t)items[i].stream << 33) | ((uint64_t)z << 32), c.hi - c.lo, z * n_items + i});
        }
    const uint32_t n_lds = pb_order_tasks(tasks, lds_cells), n_cols = (uint32_t)cols.size();

    DevBuf col_b, task_b, pool_b, out_b;
    const uint64_t out_words = 2ull * n_items * B;
    CR_TRY(dmalloc(ctx, col_b, cols.size() * sizeof(PbCol)));
    CR_TRY(dmalloc(ctx, task_b, tasks.size() * sizeof(PbTask)));
    CR_TRY(dmalloc(ctx, pool_b, pool_words * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, out_b, out_words * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, col_b.p, cols.data(), cols.size() * sizeof(PbCol)));
    CR_TRY(crgpu_memcpy_h2d(ctx, task_b.p, tasks.data(), tasks.size() * sizeof(PbTask)));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, pool_words);
        hipLaunchKernelGGL(k_pb_gather, dim3((n_cols + 3u) / 4u), dim3(SQ_WG), 0, ctx->stream, pl->d_keys, pl->d_vals, pl->nnz, pl->n_pos, col_b.as<PbCol>(), n_cols,
                           pool_b.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(pb_launch_draws(ctx, pool_b.as<uint32_t>(), task_b.as<PbTask>(), tasks, n_lds, B, draws_per_wg, a->seed, out_b.as<unsigned long long>()));
    CR_TRY(crgpu_memcpy_d2h(ctx, sums_a_out, out_b.p, (uint64_t)n_items * B * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, sums_b_out, out_b.as<uint64_t>() + (uint64_t)n_items * B, (uint64_t)n_items * B * sizeof(uint64_t)));
    return CRGPU_OK;
}

// host only.  QUIRK kept (measure_perturbations.py:527-528): s_a and s_b are the sums of the size factors of the ORIGINAL cells of each
// side (s_a and s_b of crgpu_sseq_pair_result), not of the resampled cells.
extern "C" int crgpu_perturbation_ci(const uint64_t *sums_a, const uint64_t *sums_b, uint32_t n_bootstraps, double s_a, double s_b, double ci_lower, double ci_upper,
                                     double *log2fc_out, double *lower_out, double *upper_out) {
    if (!sums_a || !sums_b || !lower_out || !upper_out || n_bootstraps < 1 || n_bootstraps > PB_MAX_BOOTSTRAPS)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_perturbation_ci: sums_a, sums_b, lower_out, upper_out and 1 .. %u bootstraps", PB_MAX_BOOTSTRAPS);
    if (!(s_a >= 0.0) || !(s_b >= 0.0) || std::isinf(s_a) || std::isinf(s_b))
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_perturbation_ci: size factor sums %g and %g, finite and not negative", s_a, s_b);
    if (!(ci_lower >= 0.0 && ci_lower <= 100.0 && ci_upper >= 0.0 && ci_upper <= 100.0))
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_perturbation_ci: percentiles %g and %g, 0 to 100", ci_lower, ci_upper);
    std::vector<double> fc(n_bootstraps);
    for (uint32_t b = 0; b < n_bootstraps; b++)
        fc[b] = std::log2((1.0 + (double)sums_a[b]) / (1.0 + s_a)) - std::log2((1.0 + (double)sums_b[b]) / (1.0 + s_b));
    if (log2fc_out) std::copy(fc.begin(), fc.end(), log2fc_out);
    std::sort(fc.begin(), fc.end());
    *lower_out = cr_quantile_sorted(fc, ci_lower / 100.0);
    *upper_out = cr_quantile_sorted(fc, ci_upper / 100.0);
    return CRGPU_OK;
}
