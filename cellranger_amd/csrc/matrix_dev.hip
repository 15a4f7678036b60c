// matrix_dev.hip -- the device matrix (crgpu_matrix_dev): the dense barcode index, CSC assembly from the count stage's triplets,
// the sum of two matrices, column selection, free and download.  matrix.hip is the host side of the same boundary; the analysis
// stages on a device matrix are matrix_stages.hip.
#include "stage_common.h"
// ------------------------------------------------------------------------------------------------
// K6 on the device: barcode index + CSC (barcode_index.rs:20-53, count_matrix.rs:382-448)
// ------------------------------------------------------------------------------------------------

// ---- CRGPU_OPT_DENSE_BARCODE_KEYS: the BarcodeIndex of the tables as they stand (cr_types/src/barcode_index.rs:20-53) ------
int cr_dense_ensure(crgpu_ctx *ctx) {
    DenseIndex &D = ctx->dense;
    if (!D.on || D.valid) return CRGPU_OK;
    CR_REQUIRE(ctx, ctx->canon_set && ctx->layout.set, CRGPU_ESTATE, "dense barcode keys: whitelist and key layout first");
    const uint32_t W = ctx->n_canon;
    SeenFlag seen;
    seen.ct.n = 0;
    for (int l = 0; l < CRGPU_MAX_LIB; l++)
        if (ctx->wl[l].set) {
            seen.ct.t[seen.ct.n++] = ctx->wl[l].d_valid;
            seen.ct.t[seen.ct.n++] = ctx->wl[l].d_corrected;
        }
    if (!D.d_fwd) CR_HIP(ctx, hipMalloc((void **)&D.d_fwd, (((size_t)W + 63) / 64) * sizeof(uint4)));
    if (!D.d_back) CR_HIP(ctx, hipMalloc((void **)&D.d_back, (size_t)W * sizeof(uint32_t)));
    uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL;
    uint32_t V = 0;
    {
        CrTimer t(ctx, CRGPU_T_KEYS);
        CR_TRY(compact(ctx, seen, EmitCol{D.d_back}, W, ctx->d_sort_hist, d_total));
    }
    CR_TRY(read_u32(ctx, d_total, &V));
    KeyLayout L = ctx->layout;
    L.bits_bc = V > 1 ? cr_ceil_log2(V) : 1u;
    CR_REQUIRE(ctx, L.total_bits() <= 64, CRGPU_ERANGE,
               "molecule key needs %u bits even with %u barcodes in the index (barcode %u + feature %u + library %u + umi %u + 1) > 64",
               L.total_bits(), V, L.bits_bc, L.bits_feat, L.bits_lib, L.bits_umi + L.bits_ulen);
    D.h_back.resize(V);
    if (V) CR_TRY(crgpu_memcpy_d2h(ctx, D.h_back.data(), D.d_back, (uint64_t)V * sizeof(uint32_t)));
    {   // rank/select table on the host (V set bits, W / 64 words): 16 bytes per 64 ranks
        const size_t n_words = ((size_t)W + 63) / 64;
        std::vector<uint4> t(n_words, make_uint4(0u, 0u, 0u, 0u));
        for (uint32_t c = 0; c < V; c++) {
            const uint32_t r = D.h_back[c];
            if (r & 32u) t[r >> 6].y |= 1u << (r & 31u); else t[r >> 6].x |= 1u << (r & 31u);
        }
        uint32_t run = 0;
        for (size_t w = 0; w < n_words; w++) {
            t[w].z = run;
            run += (uint32_t)__builtin_popcount(t[w].x) + (uint32_t)__builtin_popcount(t[w].y);
        }
        CR_TRY(crgpu_memcpy_h2d(ctx, D.d_fwd, t.data(), n_words * sizeof(uint4)));
    }
    D.V = V;
    D.valid = true;
    ctx->layout = L;
    ctx->ghist.valid = false;
    return CRGPU_OK;
}

__global__ __launch_bounds__(256) void k_csc(const uint32_t *__restrict__ col_rank, uint64_t n_cols,
                                             const uint32_t *__restrict__ t_bc, const uint32_t *__restrict__ t_feat,
                                             const uint32_t *__restrict__ t_cnt, uint64_t nt,
                                             long long *__restrict__ indptr, int32_t *__restrict__ indices,
                                             int32_t *__restrict__ data) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // indptr[c] = first triplet whose barcode rank >= col_rank[c]; columns without counts get empty ranges
    for (uint64_t c = tid; c <= n_cols; c += stride) {
        if (c == n_cols) {
            indptr[c] = (long long)nt;
            continue;
        }
        const uint32_t r = col_rank[c];
        uint64_t lo = 0, hi = nt;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (t_bc[mid] < r) lo = mid + 1; else hi = mid;
        }
        indptr[c] = (long long)lo;
    }
    for (uint64_t i = tid; i < nt; i += stride) {
        indices[i] = (int32_t)t_feat[i];
        data[i] = (int32_t)t_cnt[i];
    }
}

extern "C" int crgpu_assemble_matrix_dev(crgpu_ctx *ctx, const uint32_t *d_bc, const uint32_t *d_feature,
                                         const uint32_t *d_count, uint64_t n_triplets, crgpu_matrix_dev **out) {
    if (!ctx || !out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *out = nullptr;
    CR_REQUIRE(ctx, ctx->canon_set, CRGPU_ESTATE, "crgpu_assemble_matrix_dev: no whitelist set");
    CR_REQUIRE(ctx, n_triplets == 0 || (d_bc && d_feature && d_count), CRGPU_EINVAL, "NULL triplets");
    CR_REQUIRE(ctx, n_triplets < 0xFFFFFFFFull, CRGPU_ERANGE, "too many triplets");
    SeenFlag seen;
    seen.ct.n = 0;
    for (int l = 0; l < CRGPU_MAX_LIB; l++)
        if (ctx->wl[l].set) {
            seen.ct.t[seen.ct.n++] = ctx->wl[l].d_valid;
            seen.ct.t[seen.ct.n++] = ctx->wl[l].d_corrected;
        }
    MatrixDevImpl *m = new (std::nothrow) MatrixDevImpl();
    if (!m) return cr_fail(ctx, CRGPU_ENOMEM, "out of host memory");
    struct Guard {
        crgpu_ctx *c;
        MatrixDevImpl *m;
        bool armed = true;
        ~Guard() {
            if (armed) crgpu_matrix_dev_free(c, &m->view);
        }
    } guard{ctx, m};
    const uint32_t W = ctx->n_canon;
    CR_TRY(cr_pool_alloc(ctx, (void **)&m->d_rank, (size_t)W * sizeof(uint32_t)));
    uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL;
    uint32_t V = 0;
    {
        CrTimer t(ctx, CRGPU_T_MATRIX);
        CR_TRY(compact(ctx, seen, EmitCol{m->d_rank}, W, ctx->d_sort_hist, d_total));
    }
    CR_TRY(read_u32(ctx, d_total, &V));
    CR_TRY(cr_pool_alloc(ctx, (void **)&m->d_indptr, ((size_t)V + 1) * sizeof(long long)));
    CR_TRY(cr_pool_alloc(ctx, (void **)&m->d_indices, n_triplets * sizeof(int32_t)));
    CR_TRY(cr_pool_alloc(ctx, (void **)&m->d_data, n_triplets * sizeof(int32_t)));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX);
        const uint64_t work = n_triplets > V ? n_triplets : (uint64_t)V + 1;
        hipLaunchKernelGGL(k_csc, dim3(cr_grid(work, 256)), dim3(256), 0, ctx->stream, m->d_rank, (uint64_t)V, d_bc, d_feature,
                           d_count, n_triplets, m->d_indptr, m->d_indices, m->d_data);
        CR_HIP(ctx, hipGetLastError());
    }
    m->view.n_barcodes = V;
    m->view.nnz = n_triplets;
    m->view.d_barcode_rank = m->d_rank;
    m->view.d_indptr = (const int64_t *)m->d_indptr;
    m->view.d_indices = m->d_indices;
    m->view.d_data = m->d_data;
    guard.armed = false;
    *out = &m->view;
    return CRGPU_OK;
}

// ------------------------------------------------------------------------------------------------
// aggr-style post-processing on the device
// ------------------------------------------------------------------------------------------------
// merge of two index-sorted columns; WRITE = false counts the merged entries
template <bool WRITE>
__global__ __launch_bounds__(256) void k_sum_columns(uint64_t n_cols, const long long *__restrict__ pa, const int32_t *__restrict__ ia,
                                                     const int32_t *__restrict__ da, const long long *__restrict__ pb,
                                                     const int32_t *__restrict__ ib, const int32_t *__restrict__ db,
                                                     uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off,
                                                     int32_t *__restrict__ io, int32_t *__restrict__ dout) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_cols; c += stride) {
        long long i = pa[c], j = pb[c];
        const long long ie = pa[c + 1], je = pb[c + 1];
        uint32_t o = WRITE ? off[c] : 0u;
        while (i < ie || j < je) {
            const int32_t ra = i < ie ? ia[i] : 0x7FFFFFFF, rb = j < je ? ib[j] : 0x7FFFFFFF;
            if (WRITE) {
                io[o] = ra < rb ? ra : rb;
                dout[o] = (ra <= rb ? da[i] : 0) + (rb <= ra ? db[j] : 0);
            }
            o++;
            i += ra <= rb;
            j += rb <= ra;
        }
        if (!WRITE) cnt[c] = o;
    }
}
__global__ __launch_bounds__(256) void k_ranks_differ(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint64_t n,
                                                      uint32_t *__restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (a[i] != b[i]) *flag = 1u;
}
__global__ __launch_bounds__(256) void k_offsets_to_indptr(const uint32_t *__restrict__ off, uint64_t n, uint32_t total,
                                                           long long *__restrict__ indptr) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride)
        indptr[i] = i < n ? (long long)off[i] : (long long)total;
}
void cr_offsets_to_indptr(crgpu_ctx *ctx, const uint32_t *d_off, uint64_t n, uint32_t total, long long *d_indptr) {
    hipLaunchKernelGGL(k_offsets_to_indptr, dim3(cr_grid(n + 1, 256)), dim3(256), 0, ctx->stream, d_off, n, total, d_indptr);
}
// a column position outside [0, V) (a device list is not checked on the host) is reported through *bad and reads nothing
__global__ __launch_bounds__(256) void k_selected_lengths(const long long *__restrict__ indptr, const uint64_t *__restrict__ cols,
                                                          uint64_t n_sel, uint64_t V, const uint32_t *__restrict__ rank_in,
                                                          uint32_t *__restrict__ len, uint32_t *__restrict__ rank_out,
                                                          uint32_t *__restrict__ bad) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_sel; k += stride) {
        const uint64_t c = cols[k];
        if (c >= V) {
            *bad = 1u;
            len[k] = 0u;
            rank_out[k] = 0u;
            continue;
        }
        len[k] = (uint32_t)(indptr[c + 1] - indptr[c]);
        rank_out[k] = rank_in[c];
    }
}
// one wave per selected column: a contiguous copy of its entries
__global__ __launch_bounds__(256) void k_copy_columns(const long long *__restrict__ indptr, const uint64_t *__restrict__ cols,
                                                      uint64_t n_sel, const uint32_t *__restrict__ off,
                                                      const int32_t *__restrict__ ia, const int32_t *__restrict__ da,
                                                      int32_t *__restrict__ io, int32_t *__restrict__ dout) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t k = wave0; k < n_sel; k += n_waves) {
        const uint64_t c = cols[k];
        const long long s = indptr[c], e = indptr[c + 1];
        const uint32_t o = off[k];
        for (long long i = s + lane; i < e; i += 64) {
            io[o + (i - s)] = ia[i];
            dout[o + (i - s)] = da[i];
        }
    }
}

int cr_new_matrix_dev(crgpu_ctx *ctx, uint64_t V, uint64_t nnz, MatrixDevImpl **out) {
    MatrixDevImpl *m = new (std::nothrow) MatrixDevImpl();
    if (!m) return cr_fail(ctx, CRGPU_ENOMEM, "out of host memory");
    int rc = cr_pool_alloc(ctx, (void **)&m->d_rank, (V ? V : 1) * sizeof(uint32_t));
    if (rc == CRGPU_OK) rc = cr_pool_alloc(ctx, (void **)&m->d_indptr, (V + 1) * sizeof(long long));
    if (rc == CRGPU_OK) rc = cr_pool_alloc(ctx, (void **)&m->d_indices, (nnz ? nnz : 1) * sizeof(int32_t));
    if (rc == CRGPU_OK) rc = cr_pool_alloc(ctx, (void **)&m->d_data, (nnz ? nnz : 1) * sizeof(int32_t));
    if (rc != CRGPU_OK) {
        crgpu_matrix_dev_free(ctx, &m->view);
        return rc;
    }
    m->view.n_barcodes = V;
    m->view.nnz = nnz;
    m->view.d_barcode_rank = m->d_rank;
    m->view.d_indptr = (const int64_t *)m->d_indptr;
    m->view.d_indices = m->d_indices;
    m->view.d_data = m->d_data;
    *out = m;
    return CRGPU_OK;
}

// CountMatrix.merge / merge_matrices (lib/python/cellranger/matrix.py:479-482,1319-1329): element-wise sum of two matrices
// of the same shape -- here two device CSCs over the same columns (same barcode ranks in the same order).
extern "C" int crgpu_sum_matrices_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *a, const crgpu_matrix_dev *b, crgpu_matrix_dev **out) {
    if (!ctx || !out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *out = nullptr;
    CR_REQUIRE(ctx, a && b, CRGPU_EINVAL, "crgpu_sum_matrices_dev: NULL matrix");
    CR_REQUIRE(ctx, a->n_barcodes == b->n_barcodes, CRGPU_EINVAL, "crgpu_sum_matrices_dev: %llu vs %llu columns",
               (unsigned long long)a->n_barcodes, (unsigned long long)b->n_barcodes);
    CR_REQUIRE(ctx, a->nnz + b->nnz < 0xFFFFFFFFull, CRGPU_ERANGE, "crgpu_sum_matrices_dev: too many entries");
    const uint64_t V = a->n_barcodes;
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, *d_total = ctx->d_scalars + CR_SCALAR_TOTAL;
    DevBuf cnt_b;
    CR_TRY(dmalloc(ctx, cnt_b, (V + 1) * sizeof(uint32_t)));
    uint32_t *cnt = cnt_b.as<uint32_t>();
    const long long *pa = (const long long *)a->d_indptr, *pb = (const long long *)b->d_indptr;
    uint32_t differ = 0, total = 0;
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, a->nnz + b->nnz);
        CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
        if (V) {
            hipLaunchKernelGGL(k_ranks_differ, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, a->d_barcode_rank, b->d_barcode_rank, V, d_flag);
            hipLaunchKernelGGL(k_sum_columns<false>, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, V, pa, a->d_indices, a->d_data, pb,
                               b->d_indices, b->d_data, cnt, (const uint32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr);
        }
        CR_HIP(ctx, hipGetLastError());
        CR_TRY(cr_scan_small(ctx, cnt, V, d_total));
    }
    CR_TRY(read_u32(ctx, d_flag, &differ));
    CR_REQUIRE(ctx, !differ, CRGPU_EINVAL, "crgpu_sum_matrices_dev: the matrices hold different barcodes");
    CR_TRY(read_u32(ctx, d_total, &total));
    MatrixDevImpl *m = nullptr;
    CR_TRY(cr_new_matrix_dev(ctx, V, total, &m));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX);
        if (V) {
            CR_HIP(ctx, hipMemcpyAsync(m->d_rank, a->d_barcode_rank, V * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
            hipLaunchKernelGGL(k_sum_columns<true>, dim3(cr_grid(V, 256)), dim3(256), 0, ctx->stream, V, pa, a->d_indices, a->d_data, pb,
                               b->d_indices, b->d_data, (uint32_t *)nullptr, cnt, m->d_indices, m->d_data);
        }
        cr_offsets_to_indptr(ctx, cnt, V, total, m->d_indptr);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            crgpu_matrix_dev_free(ctx, &m->view);
            return cr_fail(ctx, CRGPU_EHIP, "crgpu_sum_matrices_dev: kernel failed");
        }
    }
    *out = &m->view;
    return CRGPU_OK;
}

// CountMatrix.select_barcodes (matrix.py:860-875): the columns at the positions d_cols (device) in the given order.
static int select_columns_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *a, const uint64_t *d_cols, uint64_t n_cols, const char *who,
                              crgpu_matrix_dev **out) {
    DevBuf len_b, rank_b;
    CR_TRY(dmalloc(ctx, len_b, (n_cols + 1) * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, rank_b, (n_cols ? n_cols : 1) * sizeof(uint32_t)));
    uint32_t *d_total = ctx->d_scalars + CR_SCALAR_TOTAL, *d_bad = ctx->d_scalars + CR_SCALAR_FLAG, total = 0, bad = 0;
    const long long *pa = (const long long *)a->d_indptr;
    {
        CrTimer t(ctx, CRGPU_T_MATRIX, n_cols);
        CR_HIP(ctx, hipMemsetAsync(d_bad, 0, sizeof(uint32_t), ctx->stream));
        if (n_cols)
            hipLaunchKernelGGL(k_selected_lengths, dim3(cr_grid(n_cols, 256)), dim3(256), 0, ctx->stream, pa, d_cols, n_cols, a->n_barcodes,
                               a->d_barcode_rank, len_b.as<uint32_t>(), rank_b.as<uint32_t>(), d_bad);
        CR_HIP(ctx, hipGetLastError());
        CR_TRY(cr_scan_small(ctx, len_b.as<uint32_t>(), n_cols, d_total));
    }
    CR_TRY(read_u32(ctx, d_bad, &bad));
    CR_REQUIRE(ctx, !bad, CRGPU_EINVAL, "%s: a column is out of range", who);
    CR_TRY(read_u32(ctx, d_total, &total));
    MatrixDevImpl *m = nullptr;
    CR_TRY(cr_new_matrix_dev(ctx, n_cols, total, &m));
    {
        CrTimer t(ctx, CRGPU_T_MATRIX);
        if (n_cols) {
            CR_HIP(ctx, hipMemcpyAsync(m->d_rank, rank_b.p, n_cols * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
            hipLaunchKernelGGL(k_copy_columns, dim3(cr_grid(n_cols * 64, 256)), dim3(256), 0, ctx->stream, pa, d_cols, n_cols,
                               len_b.as<uint32_t>(), a->d_indices, a->d_data, m->d_indices, m->d_data);
        }
        cr_offsets_to_indptr(ctx, len_b.as<uint32_t>(), n_cols, total, m->d_indptr);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            crgpu_matrix_dev_free(ctx, &m->view);
            return cr_fail(ctx, CRGPU_EHIP, "%s: kernel failed", who);
        }
    }
    *out = &m->view;
    return CRGPU_OK;
}

// ... with `cols` a host array of column positions
extern "C" int crgpu_select_barcodes_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *a, const uint64_t *cols, uint64_t n_cols,
                                         crgpu_matrix_dev **out) {
    if (!ctx || !out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *out = nullptr;
    CR_REQUIRE(ctx, a && (cols || n_cols == 0), CRGPU_EINVAL, "crgpu_select_barcodes_dev: NULL argument");
    for (uint64_t k = 0; k < n_cols; k++)
        CR_REQUIRE(ctx, cols[k] < a->n_barcodes, CRGPU_EINVAL, "crgpu_select_barcodes_dev: column %llu out of range",
                   (unsigned long long)cols[k]);
    DevBuf cols_b;
    CR_TRY(dmalloc(ctx, cols_b, (n_cols ? n_cols : 1) * sizeof(uint64_t)));
    if (n_cols) CR_HIP(ctx, hipMemcpyAsync(cols_b.p, cols, n_cols * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    return select_columns_dev(ctx, a, cols_b.as<uint64_t>(), n_cols, "crgpu_select_barcodes_dev", out);
}

// ... with a device list (the called cells of crgpu_call_cells_ordmag_dev: the filtered matrix)
extern "C" int crgpu_select_barcodes_cols_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *a, const uint64_t *d_cols, uint64_t n_cols,
                                              crgpu_matrix_dev **out) {
    if (!ctx || !out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    *out = nullptr;
    CR_REQUIRE(ctx, a && (d_cols || n_cols == 0), CRGPU_EINVAL, "crgpu_select_barcodes_cols_dev: NULL argument");
    return select_columns_dev(ctx, a, d_cols, n_cols, "crgpu_select_barcodes_cols_dev", out);
}

extern "C" void crgpu_matrix_dev_free(crgpu_ctx *ctx, crgpu_matrix_dev *mv) {
    if (!mv || !ctx) return;
    CR_ENTER(ctx);
    MatrixDevImpl *m = reinterpret_cast<MatrixDevImpl *>(mv);  // view is the first member
    cr_pool_free(ctx, m->d_rank);
    cr_pool_free(ctx, m->d_indptr);
    cr_pool_free(ctx, m->d_indices);
    cr_pool_free(ctx, m->d_data);
    delete m;
}

extern "C" int crgpu_matrix_dev_download(crgpu_ctx *ctx, const crgpu_matrix_dev *mv, uint32_t *rank_out, int64_t *indptr_out,
                                         int32_t *indices_out, int32_t *data_out) {
    if (!ctx || !mv) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    if (rank_out) CR_TRY(crgpu_memcpy_d2h(ctx, rank_out, mv->d_barcode_rank, mv->n_barcodes * sizeof(uint32_t)));
    if (indptr_out) CR_TRY(crgpu_memcpy_d2h(ctx, indptr_out, mv->d_indptr, (mv->n_barcodes + 1) * sizeof(int64_t)));
    if (indices_out) CR_TRY(crgpu_memcpy_d2h(ctx, indices_out, mv->d_indices, mv->nnz * sizeof(int32_t)));
    if (data_out) CR_TRY(crgpu_memcpy_d2h(ctx, data_out, mv->d_data, mv->nnz * sizeof(int32_t)));
    return CRGPU_OK;
}
