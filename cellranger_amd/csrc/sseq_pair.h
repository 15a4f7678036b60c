// sseq_pair.h -- the local sSeq comparison of two groups of cells: the test of MERGE_CLUSTERS (part of matrix_stages.hip).
//
// mro/rna/stages/analyzer/merge_clusters/__init__.py tests every pair of sibling leaves of the medoid dendrogram with sSeq parameters
// computed on the cells of the two leaves alone (get_local_sseq_params of MEASURE_PERTURBATIONS does the same).  With the entry points
// of sseq.h that is crgpu_select_barcodes_dev + crgpu_sseq_params_dev + crgpu_sseq_diffexp_dev with two labels, and the parameters
// re-sort the pair's entries into gene order for every pair.  Here the transpose is made ONCE for a grouping of the cells:
//
// plan (crgpu_sseq_pairs_create_dev)   pos = the grouped cells ordered by (group, cell); every entry of a grouped cell keyed
//                                      row * Npos + pos(cell) and radix-sorted (an entry of a cell in no group gets the key G * Npos
//                                      and sorts behind every gene); the counts per cell in pos order on both sides.
// pair (crgpu_sseq_pair_dev)           a gene's entries of a listed group are one contiguous run of its keys, found with two searches.
//                                      k_sq_pair_row_sums walks the runs of groups_a, then those of groups_b: the entry of concatenated
//                                      index r belongs to lane r % 64, a lane adds its entries in ascending r, the lanes are joined by
//                                      wave_sum -- the order k_sq_row_sums has on the sub-matrix of the pair's cells.  The same walk
//                                      gives x_a and x_b as u64 sums, so a pair needs no atomics.  The median of the pair's counts goes
//                                      through the u32 radix sort; size factors, S and the G-vectors are sq_size_factors and
//                                      sq_gene_params of sseq.h, the tests and Benjamini-Hochberg are sq_run_tests with one cluster.
// So every output equals bit for bit what cluster 1 of the composed path gives on crgpu_select_barcodes_dev(m, the cells of groups_a in
// pos order, then those of groups_b) with labels 1 .. 1, 2 .. 2: a pure function of the plan and the two sets.
#pragma once

#include "sseq.h"

struct SqRun {
    uint32_t lo, hi;    // the group's cells in pos
    uint32_t base;      // the place of its first cell among the pair's cells
    uint32_t reserved;
};

struct crgpu_sseq_pairs {
    uint64_t n_cells = 0, n_pos = 0, nnz = 0;
    uint32_t n_features = 0, n_groups = 0;
    std::vector<uint32_t> gstart;   // [n_groups + 1] in pos; a pair call sends the runs it lists to the device
    std::vector<uint32_t> cnt;      // counts per cell in pos order
    uint64_t *d_keys = nullptr;     // [nnz] ascending: row * n_pos + pos, then G * n_pos for the entries of a cell in no group
    uint32_t *d_vals = nullptr;     // [nnz]
    uint32_t *d_cnt = nullptr;      // [n_pos]
};

// key = row * Npos + pos(cell), G * Npos for a cell in no group; flag: a row >= G
__global__ __launch_bounds__(SQ_WG) void k_sq_pair_keys(const long long *__restrict__ indptr, const int32_t *__restrict__ indices, const int32_t *__restrict__ data,
                                                        uint64_t N, uint64_t Npos, uint32_t G, const uint32_t *__restrict__ pos_of_cell,
                                                        uint64_t *__restrict__ keys, uint32_t *__restrict__ vals, uint32_t *__restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave0; c < N; c += n_waves) {
        const long long s = indptr[c], e = indptr[c + 1];
        const uint32_t p = pos_of_cell[c];
        for (long long i = s + lane; i < e; i += 64) {
            const uint32_t r = (uint32_t)indices[i];
            if (r >= G) atomicOr(flag, 1u);
            if (r >= G || p == NONE32) {
                keys[i] = (uint64_t)G * Npos, vals[i] = 0u;
            } else {
                keys[i] = (uint64_t)r * Npos + p, vals[i] = (uint32_t)data[i];
            }
        }
    }
}

// A wave per gene over the gene's entries in the listed groups, runs[0 .. n_runs_a) = side a, the rest side b: sum x / sf and
// sum (x / sf)^2 in the order of k_sq_row_sums on the sub-matrix (lane = concatenated index % 64), x_a and x_b as integers.
__global__ __launch_bounds__(SQ_WG) void k_sq_pair_row_sums(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, uint64_t nnz, uint64_t Npos,
                                                            uint32_t G, const SqRun *__restrict__ runs, uint32_t n_runs, uint32_t n_runs_a,
                                                            const double *__restrict__ sf, double *__restrict__ s1_out, double *__restrict__ s2_out,
                                                            unsigned long long *__restrict__ xa_out, unsigned long long *__restrict__ xb_out) {
    const uint32_t g = (blockIdx.x * SQ_WG + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (g >= G) return;  // uniform over the wave
    const uint64_t k0 = (uint64_t)g * Npos;
    const uint64_t glo = cr_lower_bound(keys, nnz, k0), ghi = glo + cr_lower_bound(keys + glo, nnz - glo, k0 + Npos);
    double s1 = 0.0, s2 = 0.0;
    unsigned long long xa = 0ull, xb = 0ull;
    uint64_t off = 0;  // entries of the runs before this one
    for (uint32_t j = 0; j < n_runs; j++) {
        const SqRun run = runs[j];
        const uint64_t lo = glo + cr_lower_bound(keys + glo, ghi - glo, k0 + run.lo), hi = lo + cr_lower_bound(keys + lo, ghi - lo, k0 + run.hi);
        unsigned long long x = 0ull;
        for (uint64_t i = lo + ((lane + 64u - (uint32_t)(off & 63u)) & 63u); i < hi; i += 64u) {
            const uint32_t val = vals[i];
            const double v = (double)val / sf[run.base + (uint32_t)(keys[i] - k0 - run.lo)];
            s1 += v, s2 += v * v;
            x += val;
        }
        if (j < n_runs_a) xa += x; else xb += x;
        off += hi - lo;
    }
    s1 = wave_sum(s1), s2 = wave_sum(s2);
    xa = wave_sum(xa), xb = wave_sum(xb);
    if (lane == 0u) s1_out[g] = s1, s2_out[g] = s2, xa_out[g] = xa, xb_out[g] = xb;
}

extern "C" void crgpu_sseq_pairs_free(crgpu_ctx *ctx, crgpu_sseq_pairs *p) {
    if (!p) return;
    if (ctx) {
        CR_ENTER(ctx);
        cr_pool_free(ctx, p->d_keys), cr_pool_free(ctx, p->d_vals), cr_pool_free(ctx, p->d_cnt);
    }
    delete p;
}

static int sq_pairs_build(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const std::vector<uint32_t> &pos_of_cell, const std::vector<uint32_t> &cell_of_pos,
                          crgpu_sseq_pairs *P) {
    const uint64_t N = P->n_cells, Npos = P->n_pos, nnz = P->nnz;
    const uint32_t G = P->n_features;
    // counts per cell, brought into pos order
    DevBuf cnt_b, pos_b, kt_b, vt_b;
    CR_TRY(dmalloc(ctx, cnt_b, N * sizeof(uint32_t)));
    CR_TRY(crgpu_matrix_dev_column_sums(ctx, m, nullptr, 0, cnt_b.as<uint32_t>()));
    std::vector<uint32_t> cnt(N);
    CR_TRY(crgpu_memcpy_d2h(ctx, cnt.data(), cnt_b.p, N * sizeof(uint32_t)));
    P->cnt.resize(Npos);
    for (uint64_t p = 0; p < Npos; p++) P->cnt[p] = cnt[cell_of_pos[p]];
    CR_TRY(cr_pool_alloc(ctx, (void **)&P->d_cnt, Npos * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, P->d_cnt, P->cnt.data(), Npos * sizeof(uint32_t)));

    // the transpose in pos order by one sort
    CR_TRY(dmalloc(ctx, pos_b, N * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, pos_b.p, pos_of_cell.data(), N * sizeof(uint32_t)));
    CR_TRY(cr_pool_alloc(ctx, (void **)&P->d_keys, nnz * sizeof(uint64_t)));
    CR_TRY(cr_pool_alloc(ctx, (void **)&P->d_vals, nnz * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, kt_b, nnz * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, vt_b, nnz * sizeof(uint32_t)));
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, nnz);
        hipLaunchKernelGGL(k_sq_pair_keys, dim3(cr_grid(N * 64, SQ_WG)), dim3(SQ_WG), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data, N, Npos,
                           G, pos_b.as<uint32_t>(), P->d_keys, P->d_vals, d_flag);
        CR_HIP(ctx, hipGetLastError());
    }
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !flag, CRGPU_EINVAL, "crgpu_sseq_pairs_create_dev: the matrix holds a row >= n_features (%u)", G);
    bool in_tmp = false;
    const uint32_t key_bits = std::max(1u, cr_ceil_log2((uint64_t)G * Npos + 1ull));
    CR_TRY(cr_radix_sort_u64(ctx, P->d_keys, kt_b.as<uint64_t>(), P->d_vals, vt_b.as<uint32_t>(), nnz, 0, key_bits, &in_tmp));
    if (in_tmp) {  // the plan keeps the buffers that hold the result
        void *k = kt_b.p, *v = vt_b.p;
        kt_b.p = P->d_keys, vt_b.p = P->d_vals;
        P->d_keys = (uint64_t *)k, P->d_vals = (uint32_t *)v;
    }
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRGPU_OK;
}

extern "C" int crgpu_sseq_pairs_create_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, const int32_t *group_of_cell, uint32_t n_groups,
                                           const crgpu_sseq_pair_args *a, crgpu_sseq_pairs **out) {
    if (!ctx || !m || !group_of_cell || !a || !out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *out = nullptr;
    const uint64_t N = m->n_barcodes, nnz = m->nnz;
    const uint32_t G = a->n_features;
    CR_REQUIRE(ctx, G >= 3, CRGPU_EINVAL, "crgpu_sseq_pairs_create_dev: %u features, at least 3", G);
    CR_REQUIRE(ctx, N >= 2 && N < (1ull << 31), CRGPU_EINVAL, "crgpu_sseq_pairs_create_dev: %llu cells, 2 to 2^31 - 1", (unsigned long long)N);
    CR_REQUIRE(ctx, nnz >= 1, CRGPU_EINVAL, "crgpu_sseq_pairs_create_dev: the matrix is empty, every size factor would be 0 / 0");
    CR_REQUIRE(ctx, n_groups >= 2 && n_groups <= CRGPU_SSEQ_MAX_K, CRGPU_EINVAL, "crgpu_sseq_pairs_create_dev: %u groups, 2 to %u", n_groups, CRGPU_SSEQ_MAX_K);
    std::unique_ptr<crgpu_sseq_pairs> P(new crgpu_sseq_pairs);
    P->n_cells = N, P->nnz = nnz, P->n_features = G, P->n_groups = n_groups;
    P->gstart.assign(n_groups + 1u, 0);
    for (uint64_t c = 0; c < N; c++) {
        CR_REQUIRE(ctx, group_of_cell[c] >= -1 && group_of_cell[c] < (int32_t)n_groups, CRGPU_EINVAL,
                   "crgpu_sseq_pairs_create_dev: group %d of cell %llu, -1 to %u", group_of_cell[c], (unsigned long long)c, n_groups - 1u);
        if (group_of_cell[c] >= 0) P->gstart[group_of_cell[c] + 1]++;
    }
    for (uint32_t k = 0; k < n_groups; k++) {
        CR_REQUIRE(ctx, P->gstart[k + 1u] > 0, CRGPU_EINVAL, "crgpu_sseq_pairs_create_dev: group %u is empty", k);
        P->gstart[k + 1u] += P->gstart[k];
    }
    P->n_pos = P->gstart[n_groups];
    std::vector<uint32_t> pos_of_cell(N, NONE32), cell_of_pos(P->n_pos), next(P->gstart.begin(), P->gstart.end() - 1);
    for (uint64_t c = 0; c < N; c++)
        if (group_of_cell[c] >= 0) {
            const uint32_t p = next[group_of_cell[c]]++;
            pos_of_cell[c] = p, cell_of_pos[p] = (uint32_t)c;
        }
    crgpu_sseq_pairs *raw = P.release();
    const int rc = sq_pairs_build(ctx, m, pos_of_cell, cell_of_pos, raw);
    if (rc != CRGPU_OK) {
        crgpu_sseq_pairs_free(ctx, raw);
        return rc;
    }
    *out = raw;
    return CRGPU_OK;
}

// an ascending list of distinct group ids below n_groups
static int sq_check_group_list(crgpu_ctx *ctx, const uint32_t *g, uint32_t n, uint32_t n_groups, const char *name) {
    CR_REQUIRE(ctx, n >= 1, CRGPU_EINVAL, "crgpu_sseq_pair_dev: %s is empty", name);
    for (uint32_t i = 0; i < n; i++) {
        CR_REQUIRE(ctx, g[i] < n_groups, CRGPU_EINVAL, "crgpu_sseq_pair_dev: group %u of %s, the plan has %u groups", g[i], name, n_groups);
        CR_REQUIRE(ctx, i == 0 || g[i - 1] < g[i], CRGPU_EINVAL, "crgpu_sseq_pair_dev: %s must be strictly ascending (group %u after %u)", name, g[i],
                   i ? g[i - 1] : 0u);
    }
    return CRGPU_OK;
}

extern "C" int crgpu_sseq_pair_dev(crgpu_ctx *ctx, const crgpu_sseq_pairs *pl, const uint32_t *groups_a, uint32_t n_a, const uint32_t *groups_b, uint32_t n_b,
                                   const crgpu_sseq_pair_args *a, crgpu_sseq_pair_result *res) {
    if (!ctx || !pl || !groups_a || !groups_b || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const uint32_t G = pl->n_features;
    CR_REQUIRE(ctx, a->n_features == 0 || a->n_features == G, CRGPU_EINVAL, "crgpu_sseq_pair_dev: the plan has %u features, the arguments say %u", G, a->n_features);
    CR_REQUIRE(ctx, a->de_threshold >= 0.0, CRGPU_EINVAL, "crgpu_sseq_pair_dev: de_threshold %g, 0 (= 0.05) or above", a->de_threshold);
    CR_TRY(sq_check_group_list(ctx, groups_a, n_a, pl->n_groups, "groups_a"));
    CR_TRY(sq_check_group_list(ctx, groups_b, n_b, pl->n_groups, "groups_b"));
    for (uint32_t i = 0, j = 0; i < n_a && j < n_b;) {  // both ascend
        CR_REQUIRE(ctx, groups_a[i] != groups_b[j], CRGPU_EINVAL, "crgpu_sseq_pair_dev: group %u is on both sides", groups_a[i]);
        if (groups_a[i] < groups_b[j]) i++; else j++;
    }
    const double thr = a->de_threshold == 0.0 ? 0.05 : a->de_threshold;

    // the pair's cells: the runs of side a, then those of side b
    const uint32_t n_runs = n_a + n_b;
    std::vector<SqRun> runs(n_runs);
    std::vector<uint32_t> cnt;
    uint64_t Na = 0;
    for (uint32_t j = 0; j < n_runs; j++) {
        const uint32_t k = j < n_a ? groups_a[j] : groups_b[j - n_a];
        runs[j] = SqRun{pl->gstart[k], pl->gstart[k + 1u], (uint32_t)cnt.size(), 0u};
        cnt.insert(cnt.end(), pl->cnt.begin() + pl->gstart[k], pl->cnt.begin() + pl->gstart[k + 1u]);
        if (j + 1u == n_a) Na = cnt.size();
    }
    const uint64_t Np = cnt.size();
    for (uint64_t c = 0; c < Np; c++)
        CR_REQUIRE(ctx, cnt[c] > 0, CRGPU_EINVAL, "crgpu_sseq_pair_dev: a cell without counts (its size factor would be 0)");

    // the median of the pair's counts through the sort
    auto t0 = std::chrono::steady_clock::now();
    DevBuf key_b, keyt_b;
    CR_TRY(dmalloc(ctx, key_b, Np * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, keyt_b, Np * sizeof(uint32_t)));
    for (const SqRun &r : runs)
        CR_HIP(ctx, hipMemcpyAsync(key_b.as<uint32_t>() + r.base, pl->d_cnt + r.lo, (size_t)(r.hi - r.lo) * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    bool in_tmp = false;
    CR_TRY(cr_radix_sort_u32(ctx, key_b.as<uint32_t>(), keyt_b.as<uint32_t>(), nullptr, nullptr, Np, 0, 32, &in_tmp));
    std::vector<uint32_t> sorted(Np);
    CR_TRY(crgpu_memcpy_d2h(ctx, sorted.data(), in_tmp ? keyt_b.p : key_b.p, Np * sizeof(uint32_t)));
    const double median = cr_median_sorted(sorted);
    crgpu_sseq_params P;
    P.n_cells = Np, P.n_features = G;
    const double S = sq_size_factors(cnt.data(), Np, median, P.sf);
    res->ms_median = cr_ms_since(t0);

    // the per-gene sums over the pair's runs
    t0 = std::chrono::steady_clock::now();
    DevBuf sf_b, run_b, s1_b, s2_b, xa_b, xb_b;
    CR_TRY(dmalloc(ctx, sf_b, Np * sizeof(double)));
    CR_TRY(dmalloc(ctx, run_b, n_runs * sizeof(SqRun)));
    CR_TRY(dmalloc(ctx, s1_b, G * sizeof(double)));
    CR_TRY(dmalloc(ctx, s2_b, G * sizeof(double)));
    CR_TRY(dmalloc(ctx, xa_b, G * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, xb_b, G * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, sf_b.p, P.sf.data(), Np * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, run_b.p, runs.data(), n_runs * sizeof(SqRun)));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, pl->nnz);
        hipLaunchKernelGGL(k_sq_pair_row_sums, dim3((G + 3u) / 4u), dim3(SQ_WG), 0, ctx->stream, pl->d_keys, pl->d_vals, pl->nnz, pl->n_pos, G, run_b.as<SqRun>(), n_runs,
                           n_a, sf_b.as<double>(), s1_b.as<double>(), s2_b.as<double>(), xa_b.as<unsigned long long>(), xb_b.as<unsigned long long>());
        CR_HIP(ctx, hipGetLastError());
    }
    std::vector<double> s1(G), s2(G);
    std::vector<uint64_t> xin(G), total(G);
    CR_TRY(crgpu_memcpy_d2h(ctx, s1.data(), s1_b.p, G * sizeof(double)));
    CR_TRY(crgpu_memcpy_d2h(ctx, s2.data(), s2_b.p, G * sizeof(double)));
    CR_TRY(crgpu_memcpy_d2h(ctx, xin.data(), xa_b.p, G * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, total.data(), xb_b.p, G * sizeof(uint64_t)));
    for (uint32_t g = 0; g < G; g++) total[g] += xin[g];
    res->ms_sums = cr_ms_since(t0);

    CR_TRY(sq_gene_params(ctx, "crgpu_sseq_pair_dev", P, s1, s2, S));
    std::vector<double> s_a(1, 0.0), s_b(1, 0.0);  // in the order of the pair's cells
    for (uint64_t c = 0; c < Na; c++) s_a[0] += P.sf[c];
    for (uint64_t c = Na; c < Np; c++) s_b[0] += P.sf[c];

    // the tests of side a against side b: one cluster of sq_run_tests
    std::vector<double> adj;
    if (!res->adjusted_p_values_out) adj.resize(G);
    double *adj_out = res->adjusted_p_values_out ? res->adjusted_p_values_out : adj.data();
    uint64_t n_exact = 0, n_big = 0;
    crgpu_sseq_result r = {};
    r.sums_in_out = res->sums_a_out, r.sums_out_out = res->sums_b_out;
    r.norm_mean_in_out = res->norm_mean_a_out, r.norm_mean_out_out = res->norm_mean_b_out;
    r.log2_fold_change_out = res->log2_fold_change_out, r.p_values_out = res->p_values_out, r.adjusted_p_values_out = adj_out;
    r.below_median_out = res->below_median_out, r.n_exact_out = &n_exact, r.n_asymptotic_out = &n_big;
    const crgpu_sseq_args sa = {G, a->wave_min, a->wg_min, 0u};
    SqTested T;
    CR_TRY(sq_run_tests(ctx, "crgpu_sseq_pair_dev", P, 1u, xin, total, s_a, s_b, &sa, &r, T));
    CR_TRY(sq_write_results(ctx, G, 1u, xin, total, s_a, s_b, T, &r));

    uint64_t n_de = 0;
    for (uint32_t g = 0; g < G; g++) n_de += adj_out[g] < thr ? 1u : 0u;
    if (res->use_out) std::copy(P.use.begin(), P.use.end(), res->use_out);
    if (res->mean_out) std::copy(P.mean.begin(), P.mean.end(), res->mean_out);
    if (res->phi_mm_out) std::copy(P.phi_mm.begin(), P.phi_mm.end(), res->phi_mm_out);
    if (res->phi_out) std::copy(P.phi.begin(), P.phi.end(), res->phi_out);
    res->zeta_hat = P.zeta_hat, res->delta = P.delta, res->s_a = s_a[0], res->s_b = s_b[0];
    res->n_cells_a = Na, res->n_cells_b = Np - Na;
    res->n_exact = n_exact, res->n_asymptotic = n_big, res->n_terms = r.n_terms, res->n_de = n_de;
    res->n_used = P.n_used, res->n_runs = n_runs;
    res->ms_exact = r.ms_exact, res->ms_asymptotic = r.ms_asymptotic, res->ms_bh = r.ms_bh;
    return CRGPU_OK;
}
