// tsne.hip -- RUN_TSNE on the device: the perplexity search, the symmetrised sparse P, the exact gradient and the descent loop.
//
// The stage (mro/rna/stages/analyzer/run_tsne/__init__.py, lib/python/cellranger/analysis/bhtsne.py, lib/rust/cr_ana/src/stages/tsne.rs)
// calls a port of van der Maaten's bh_tsne whose source the reference does not carry; what is here is the published algorithm in the
// theta = 0 limit (no tree), restated in include/crgpu.h and in tests/tsne_numpy.py.  All of it f64, unfused.
//
// Launch structure.
//   k_tsne_search      a lane per row: the bisection on beta over the row's k squared distances, sums left to right over the ranks
//   k_pair_keys        (graph_common.h) two keys per neighbour pair, i * n + j and j * n + i, the pair's number as payload; one radix sort
//   compaction         the first of a run of equal keys is emitted: (value + the other direction's or 0) / 2; k_keys_to_csr
//                      (graph_common.h) by search
//   k_colparts / k_colfinal   (graph_common.h) column sums over partials of 256 rows, left to right, then the partials ascending (one
//                      sum order for the total of P, Z, the column means of Y and the cost)
//   k_tsne_repulse     one workgroup per (row tile, candidate chunk of CRGPU_TSNE_CAND_CHUNK rows), a lane a row with its coordinates in
//                      registers; candidate tiles stream through LDS, every lane reads the same address; no norm expansion; the chunk's
//                      partial (z, neg[dims]) goes to a slab with plain stores
//   k_tsne_finish      adds a row's chunk partials left to right
//   k_tsne_attract     walks a row's CSR entries left to right and applies the update into a second Y; a lane per row below
//                      wave_row_len entries, a wave per row from it on (the lanes compute 64 terms, which are then added in entry order)
//   k_tsne_centre      Y = the second Y minus its column means
// An iteration is these launches and nothing else: no floating-point atomic, no graph capture, no cooperative launch, and the host
// reads nothing inside the loop.  The loop holds + - * / only; exp is in k_tsne_search, log in k_tsne_kl.
// QUIRK kept: a row that is its own neighbour (Context.knn keeps a row whose exact duplicate of lower index took the first place) gives
// the entry (i, i), which takes part in the total of P and in the cost and pulls nothing.
#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <vector>

#include "graph_common.h"

#define TSNE_WG 256u
#define TSNE_MAX_STEPS 200u        // steps of the search at the most
#define TSNE_TOL 1e-5
#define TSNE_MAX_CAND_TILE 1024u   // candidates of an LDS tile at the most: 24 KiB at 3 dimensions
#define TSNE_SLAB_BYTES (256ull << 20)
#define TSNE_EXAGGERATION 12.0

// ---- the perplexity search -----------------------------------------------------------------------------------------------------------
// beta_out[i] = the beta the row was made with, steps_out[i] = evaluations of H, cond[i * k + m] = p_m / s
__global__ __launch_bounds__(TSNE_WG) void k_tsne_search(const double *__restrict__ dist, uint32_t n, uint32_t k, double log_perp,
                                                         double *__restrict__ beta_out, uint32_t *__restrict__ steps_out, double *__restrict__ cond) {
    const uint32_t i = blockIdx.x * TSNE_WG + threadIdx.x;
    if (i >= n) return;
    const double *d = dist + (size_t)i * k;
    double beta = 1.0, lo = -DBL_MAX, hi = DBL_MAX, used = 1.0, s = DBL_MIN;
    uint32_t steps = 0;
    while (steps < TSNE_MAX_STEPS) {
        double sum = 0.0, h = 0.0;
        for (uint32_t m = 0; m < k; m++) {
            const double d2 = d[m] * d[m], bd = beta * d2, p = exp(-bd);
            sum += p;
            h += bd * p;
        }
        s = DBL_MIN + sum;
        const double H = h / s + log(s), diff = H - log_perp;
        used = beta;
        steps++;
        if (fabs(diff) < TSNE_TOL) break;
        if (diff > 0.0) {
            lo = beta;
            beta = (hi == DBL_MAX || hi == -DBL_MAX) ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = (lo == -DBL_MAX || lo == DBL_MAX) ? beta / 2.0 : (beta + lo) / 2.0;
        }
    }
    beta_out[i] = used;
    steps_out[i] = steps;
    for (uint32_t m = 0; m < k; m++) cond[(size_t)i * k + m] = exp(-(used * (d[m] * d[m]))) / s;
}

// ---- the symmetrised P ---------------------------------------------------------------------------------------------------------------
// A key occurs once per direction at the most (a row's neighbours are distinct), so a run has one or two members and the order of the
// two does not reach the sum.
struct TsneEmitMerged {
    const uint64_t *keys;
    const uint32_t *perm;
    const double *cond;
    uint64_t n2;
    uint64_t *ckeys;
    double *values;
    struct Pre {};
    __device__ __forceinline__ Pre pre(uint64_t) const { return Pre(); }
    __device__ __forceinline__ void operator()(uint64_t i, uint32_t o, Pre) const {
        const uint64_t key = keys[i];
        const double a = cond[perm[i] >> 1];
        const double b = (i + 1 < n2 && keys[i + 1] == key) ? cond[perm[i + 1] >> 1] : 0.0;
        ckeys[o] = key;
        values[o] = (a + b) / 2.0;
    }
};
__global__ __launch_bounds__(TSNE_WG) void k_tsne_divide(double *__restrict__ v, uint64_t nnz, const double *__restrict__ total) {
    const double t = total[0];
    for (uint64_t e = (uint64_t)blockIdx.x * TSNE_WG + threadIdx.x; e < nnz; e += (uint64_t)gridDim.x * TSNE_WG) v[e] = v[e] / t;
}

// ---- the gradient --------------------------------------------------------------------------------------------------------------------
// The rows row0 .. row0 + rows of Y against the candidate chunk blockIdx.x / n_tiles; dynamic LDS: cand_tile * DIMS doubles.
// slab[(chunk * rows + r) * (DIMS + 1)] = z, then neg[DIMS]
template <uint32_t DIMS>
__global__ __launch_bounds__(TSNE_WG) void k_tsne_repulse(const double *__restrict__ Y, uint32_t n, uint32_t row0, uint32_t rows, uint32_t n_tiles,
                                                          uint32_t cand_tile, double *__restrict__ slab) {
    extern __shared__ double tsne_lds[];
    const uint32_t R = blockDim.x, tid = threadIdx.x, tile = blockIdx.x % n_tiles, chunk = blockIdx.x / n_tiles;
    const uint32_t r = tile * R + tid;
    const bool live = r < rows;
    const uint32_t i = row0 + (live ? r : rows - 1u);  // a lane without a row computes on the last one and stores nothing
    double yi[DIMS], neg[DIMS], z = 0.0;
#pragma unroll
    for (uint32_t t = 0; t < DIMS; t++) yi[t] = Y[(size_t)i * DIMS + t], neg[t] = 0.0;
    const uint32_t c_lo = chunk * CRGPU_TSNE_CAND_CHUNK, c_hi = n - c_lo < CRGPU_TSNE_CAND_CHUNK ? n : c_lo + CRGPU_TSNE_CAND_CHUNK;
    for (uint32_t c0 = c_lo; c0 < c_hi; c0 += cand_tile) {
        const uint32_t m = c_hi - c0 < cand_tile ? c_hi - c0 : cand_tile;
        __syncthreads();  // the previous tile is done with
        for (uint32_t e = tid; e < m * DIMS; e += R) tsne_lds[e] = Y[(size_t)c0 * DIMS + e];
        __syncthreads();
#pragma unroll 4
        for (uint32_t c = 0; c < m; c++) {
            double v[DIMS], d2 = 0.0;
#pragma unroll
            for (uint32_t t = 0; t < DIMS; t++) {
                v[t] = yi[t] - tsne_lds[c * DIMS + t];
                d2 += v[t] * v[t];
            }
            double q = 1.0 / (1.0 + d2);
            q = (c0 + c == i) ? 0.0 : q;  // the pair (i, i) is no pair: it adds +0.0, which moves no bit
            z += q;
            const double qq = q * q;
#pragma unroll
            for (uint32_t t = 0; t < DIMS; t++) neg[t] += qq * v[t];
        }
    }
    if (live) {
        const size_t at = ((size_t)chunk * rows + r) * (DIMS + 1u);
        slab[at] = z;
#pragma unroll
        for (uint32_t t = 0; t < DIMS; t++) slab[at + 1u + t] = neg[t];
    }
}
// rep[(row0 + r) * W + c] = the chunk partials of row r, column c, left to right; W = dims + 1
__global__ __launch_bounds__(TSNE_WG) void k_tsne_finish(const double *__restrict__ slab, uint32_t row0, uint32_t rows, uint32_t n_chunks, uint32_t W,
                                                         double *__restrict__ rep) {
    const uint64_t total = (uint64_t)rows * W;
    for (uint64_t e = (uint64_t)blockIdx.x * TSNE_WG + threadIdx.x; e < total; e += (uint64_t)gridDim.x * TSNE_WG) {
        double s = 0.0;
        for (uint32_t ch = 0; ch < n_chunks; ch++) s += slab[(size_t)ch * rows * W + e];
        rep[(size_t)row0 * W + e] = s;
    }
}

__device__ __forceinline__ int tsne_sign(double x) { return x > 0.0 ? 1 : (x < 0.0 ? -1 : 0); }

struct TsneStep {
    double e, momentum, eta;
    uint32_t n, thr, update;
};
// zq[0] = Z.  update = 1: gains, uY and Ynew = Y + uY are written; 0: grad = dC.  A row belongs to the launch with WAVE = (its
// entries >= thr).
template <uint32_t DIMS, bool WAVE>
__global__ __launch_bounds__(TSNE_WG) void k_tsne_attract(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                          const double *__restrict__ values, const double *__restrict__ Y, const double *__restrict__ rep,
                                                          const double *__restrict__ zq, TsneStep s, double *__restrict__ uY, double *__restrict__ gains,
                                                          double *__restrict__ Ynew, double *__restrict__ grad) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t gtid = (uint64_t)blockIdx.x * TSNE_WG + threadIdx.x, gsize = (uint64_t)gridDim.x * TSNE_WG;
    const uint64_t first = WAVE ? gtid >> 6 : gtid, stride = WAVE ? gsize >> 6 : gsize;
    const double Z = zq[0];
    for (uint64_t i = first; i < s.n; i += stride) {
        const uint64_t a = (uint64_t)indptr[i], b = (uint64_t)indptr[i + 1];
        if (((b - a) >= s.thr) != WAVE) continue;  // uniform in a wave when WAVE
        double yi[DIMS], pos[DIMS];
#pragma unroll
        for (uint32_t t = 0; t < DIMS; t++) yi[t] = Y[i * DIMS + t], pos[t] = 0.0;
        if (WAVE) {
            for (uint64_t e0 = a; e0 < b; e0 += 64u) {
                const uint64_t e = e0 + lane;
                double term[DIMS];
#pragma unroll
                for (uint32_t t = 0; t < DIMS; t++) term[t] = 0.0;  // a lane past the end adds +0.0, which moves no bit
                if (e < b) {
                    const uint32_t j = (uint32_t)indices[e];
                    double v[DIMS], d2 = 0.0;
#pragma unroll
                    for (uint32_t t = 0; t < DIMS; t++) {
                        v[t] = yi[t] - Y[(size_t)j * DIMS + t];
                        d2 += v[t] * v[t];
                    }
                    const double w = (s.e * values[e]) * (1.0 / (1.0 + d2));
#pragma unroll
                    for (uint32_t t = 0; t < DIMS; t++) term[t] = w * v[t];
                }
                for (int l = 0; l < 64; l++) {
#pragma unroll
                    for (uint32_t t = 0; t < DIMS; t++) pos[t] += __shfl(term[t], l);
                }
            }
            if (lane != 0u) continue;
        } else {
            for (uint64_t e = a; e < b; e++) {
                const uint32_t j = (uint32_t)indices[e];
                double v[DIMS], d2 = 0.0;
#pragma unroll
                for (uint32_t t = 0; t < DIMS; t++) {
                    v[t] = yi[t] - Y[(size_t)j * DIMS + t];
                    d2 += v[t] * v[t];
                }
                const double w = (s.e * values[e]) * (1.0 / (1.0 + d2));
#pragma unroll
                for (uint32_t t = 0; t < DIMS; t++) pos[t] += w * v[t];
            }
        }
#pragma unroll
        for (uint32_t t = 0; t < DIMS; t++) {
            const double dC = pos[t] - rep[i * (DIMS + 1u) + 1u + t] / Z;
            if (s.update) {
                double g = gains[i * DIMS + t], u = uY[i * DIMS + t];
                g = tsne_sign(dC) != tsne_sign(u) ? g + 0.2 : g * 0.8;
                g = g < 0.01 ? 0.01 : g;
                u = (s.momentum * u) - ((s.eta * g) * dC);
                gains[i * DIMS + t] = g, uY[i * DIMS + t] = u;
                Ynew[i * DIMS + t] = yi[t] + u;
            } else {
                grad[i * DIMS + t] = dC;
            }
        }
    }
}
// Y = Ynew - sums / n
__global__ __launch_bounds__(TSNE_WG) void k_tsne_centre(const double *__restrict__ Ynew, uint64_t n, uint32_t dims, const double *__restrict__ sums,
                                                         double *__restrict__ Y) {
    const uint64_t total = n * dims;
    for (uint64_t e = (uint64_t)blockIdx.x * TSNE_WG + threadIdx.x; e < total; e += (uint64_t)gridDim.x * TSNE_WG)
        Y[e] = Ynew[e] - sums[e % dims] / (double)n;
}
// rowkl[i] = the row's entries left to right: p * log((p + FLT_MIN) / (q / Z + FLT_MIN))
template <uint32_t DIMS>
__global__ __launch_bounds__(TSNE_WG) void k_tsne_kl(const long long *__restrict__ indptr, const int32_t *__restrict__ indices, const double *__restrict__ values,
                                                     const double *__restrict__ Y, const double *__restrict__ zq, uint32_t n, double *__restrict__ rowkl) {
    const double Z = zq[0];
    for (uint64_t i = (uint64_t)blockIdx.x * TSNE_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TSNE_WG) {
        double s = 0.0;
        for (uint64_t e = (uint64_t)indptr[i]; e < (uint64_t)indptr[i + 1]; e++) {
            const uint32_t j = (uint32_t)indices[e];
            double d2 = 0.0;
#pragma unroll
            for (uint32_t t = 0; t < DIMS; t++) {
                const double v = Y[i * DIMS + t] - Y[(size_t)j * DIMS + t];
                d2 += v * v;
            }
            const double q = 1.0 / (1.0 + d2), p = values[e];
            s += p * log((p + (double)FLT_MIN) / (q / Z + (double)FLT_MIN));
        }
        rowkl[i] = s;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
// the seams of a call, checked
struct TsneSeams {
    uint32_t row_tile, cand_tile, slab_rows, wave_row_len;
};
static int tsne_seams(crgpu_ctx *ctx, const char *who, const crgpu_tsne_args *a, uint64_t n, uint32_t dims, TsneSeams *out) {
    const uint32_t R = a->row_tile ? a->row_tile : 64u, T = a->cand_tile ? a->cand_tile : 512u, W = a->wave_row_len ? a->wave_row_len : 32u;
    CR_REQUIRE(ctx, R == 64u || R == 128u || R == 256u, CRGPU_EINVAL, "%s: a row tile of %u rows, 64, 128 or 256", who, R);
    CR_REQUIRE(ctx, T >= 1u && T <= TSNE_MAX_CAND_TILE, CRGPU_EINVAL, "%s: a candidate tile of %u rows, 1 to %u", who, T, TSNE_MAX_CAND_TILE);
    CR_REQUIRE(ctx, a->slab_rows % R == 0u && a->reserved == 0u, CRGPU_EINVAL, "%s: slab_rows is a multiple of the row tile, reserved 0", who);
    const uint64_t n_chunks = (n + CRGPU_TSNE_CAND_CHUNK - 1u) / CRGPU_TSNE_CAND_CHUNK, padded = (n + R - 1u) / R * R;
    uint64_t S = a->slab_rows ? a->slab_rows : std::max<uint64_t>(R, TSNE_SLAB_BYTES / (n_chunks * (dims + 1u) * sizeof(double)) / R * R);
    S = std::min<uint64_t>(S, padded);
    out->row_tile = R, out->cand_tile = T, out->slab_rows = (uint32_t)S, out->wave_row_len = W;
    return CRGPU_OK;
}

static int tsne_check_finite(crgpu_ctx *ctx, const char *who, const char *what, const double *v, uint64_t count) {
    for (uint64_t e = 0; e < count; e++) CR_REQUIRE(ctx, std::isfinite(v[e]), CRGPU_EINVAL, "%s: %s[%llu] is not finite", who, what, (unsigned long long)e);
    return CRGPU_OK;
}
// indptr, indices, values of a caller: the structure (fewer than 2^32 entries, indices strictly ascending within a row), finite values
static int tsne_check_csr(crgpu_ctx *ctx, const char *who, const int64_t *indptr, const int32_t *indices, const double *values, uint64_t n, uint64_t *nnz_out) {
    CR_TRY(cr_check_csr(ctx, who, indptr, indices, n, 32u, true));
    *nnz_out = (uint64_t)indptr[n];
    return tsne_check_finite(ctx, who, "values", values, *nnz_out);
}

// What the gradient and the loop share: P and Y on the device and the buffers of an iteration
struct TsneState {
    uint32_t n = 0, dims = 0, n_chunks = 0;
    uint64_t nnz = 0;
    TsneSeams seams;
    DevBuf indptr, indices, values, Y, Ynew, uY, gains, grad, rep, slab, parts, scal, rowkl;
    double *zq() { return scal.as<double>(); }            // Z
    double *sums() { return scal.as<double>() + 4; }      // the column sums of Ynew
    double *klq() { return scal.as<double>() + 8; }       // the cost
};
static int tsne_state(crgpu_ctx *ctx, TsneState &S, const int64_t *indptr, const int32_t *indices, const double *values, const double *y, uint64_t n,
                      uint32_t dims, uint64_t nnz, const TsneSeams &seams) {
    S.n = (uint32_t)n, S.dims = dims, S.nnz = nnz, S.seams = seams, S.n_chunks = (uint32_t)((n + CRGPU_TSNE_CAND_CHUNK - 1u) / CRGPU_TSNE_CAND_CHUNK);
    const uint64_t yb = n * dims * sizeof(double), n_parts = (n + GRAPH_PART_ROWS - 1u) / GRAPH_PART_ROWS;
    CR_TRY(dmalloc(ctx, S.indptr, (n + 1) * sizeof(int64_t)));
    CR_TRY(dmalloc(ctx, S.indices, std::max<uint64_t>(1, nnz) * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, S.values, std::max<uint64_t>(1, nnz) * sizeof(double)));
    CR_TRY(dmalloc(ctx, S.Y, yb));
    CR_TRY(dmalloc(ctx, S.Ynew, yb));
    CR_TRY(dmalloc(ctx, S.uY, yb));
    CR_TRY(dmalloc(ctx, S.gains, yb));
    CR_TRY(dmalloc(ctx, S.grad, yb));
    CR_TRY(dmalloc(ctx, S.rep, n * (dims + 1u) * sizeof(double)));
    CR_TRY(dmalloc(ctx, S.slab, (uint64_t)seams.slab_rows * S.n_chunks * (dims + 1u) * sizeof(double)));
    CR_TRY(dmalloc(ctx, S.parts, n_parts * (dims + 1u) * sizeof(double)));
    CR_TRY(dmalloc(ctx, S.scal, 16 * sizeof(double)));
    CR_TRY(dmalloc(ctx, S.rowkl, n * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, S.indptr.p, indptr, (n + 1) * sizeof(int64_t)));
    if (nnz) {
        CR_TRY(crgpu_memcpy_h2d(ctx, S.indices.p, indices, nnz * sizeof(int32_t)));
        CR_TRY(crgpu_memcpy_h2d(ctx, S.values.p, values, nnz * sizeof(double)));
    }
    CR_TRY(crgpu_memcpy_h2d(ctx, S.Y.p, y, yb));
    return CRGPU_OK;
}
// rep and Z at the Y of the state; ev: an event pair around the launches, or NULL
template <uint32_t DIMS>
static int tsne_repulsion(crgpu_ctx *ctx, TsneState &S, hipEvent_t *ev) {
    const uint32_t R = S.seams.row_tile;
    const size_t lds = (size_t)S.seams.cand_tile * DIMS * sizeof(double);
    if (ev) CR_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    for (uint32_t row0 = 0; row0 < S.n; row0 += S.seams.slab_rows) {
        const uint32_t rows = std::min(S.seams.slab_rows, S.n - row0), n_tiles = (rows + R - 1u) / R;
        hipLaunchKernelGGL(k_tsne_repulse<DIMS>, dim3(n_tiles * S.n_chunks), dim3(R), lds, ctx->stream, S.Y.as<double>(), S.n, row0, rows, n_tiles,
                           S.seams.cand_tile, S.slab.as<double>());
        hipLaunchKernelGGL(k_tsne_finish, dim3(cr_grid((uint64_t)rows * (DIMS + 1u), TSNE_WG)), dim3(TSNE_WG), 0, ctx->stream, S.slab.as<double>(), row0, rows,
                           S.n_chunks, DIMS + 1u, S.rep.as<double>());
    }
    if (ev) CR_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    cr_colsums(ctx, S.rep.as<double>(), S.n, DIMS + 1u, 1u, S.parts.as<double>(), S.zq());
    CR_HIP(ctx, hipGetLastError());
    return CRGPU_OK;
}
template <uint32_t DIMS>
static int tsne_attraction(crgpu_ctx *ctx, TsneState &S, const TsneStep &st) {
    const uint32_t g_lane = cr_grid(S.n, TSNE_WG), g_wave = cr_grid((uint64_t)S.n * 64u, TSNE_WG);
    hipLaunchKernelGGL((k_tsne_attract<DIMS, false>), dim3(g_lane), dim3(TSNE_WG), 0, ctx->stream, S.indptr.as<long long>(), S.indices.as<int32_t>(),
                       S.values.as<double>(), S.Y.as<double>(), S.rep.as<double>(), S.zq(), st, S.uY.as<double>(), S.gains.as<double>(), S.Ynew.as<double>(),
                       S.grad.as<double>());
    hipLaunchKernelGGL((k_tsne_attract<DIMS, true>), dim3(g_wave), dim3(TSNE_WG), 0, ctx->stream, S.indptr.as<long long>(), S.indices.as<int32_t>(),
                       S.values.as<double>(), S.Y.as<double>(), S.rep.as<double>(), S.zq(), st, S.uY.as<double>(), S.gains.as<double>(), S.Ynew.as<double>(),
                       S.grad.as<double>());
    CR_HIP(ctx, hipGetLastError());
    return CRGPU_OK;
}
// the cost at the Y of the state with the Z in zq
template <uint32_t DIMS>
static int tsne_cost(crgpu_ctx *ctx, TsneState &S) {
    hipLaunchKernelGGL(k_tsne_kl<DIMS>, dim3(cr_grid(S.n, TSNE_WG)), dim3(TSNE_WG), 0, ctx->stream, S.indptr.as<long long>(), S.indices.as<int32_t>(),
                       S.values.as<double>(), S.Y.as<double>(), S.zq(), S.n, S.rowkl.as<double>());
    cr_colsums(ctx, S.rowkl.as<double>(), S.n, 1u, 1u, S.parts.as<double>(), S.klq());
    CR_HIP(ctx, hipGetLastError());
    return CRGPU_OK;
}
template <uint32_t DIMS>
static int tsne_gradient(crgpu_ctx *ctx, TsneState &S, double exaggeration) {
    CR_TRY(tsne_repulsion<DIMS>(ctx, S, nullptr));
    TsneStep st = {exaggeration, 0.0, 0.0, S.n, S.seams.wave_row_len, 0u};
    CR_TRY(tsne_attraction<DIMS>(ctx, S, st));
    return tsne_cost<DIMS>(ctx, S);
}
template <uint32_t DIMS>
static int tsne_loop(crgpu_ctx *ctx, TsneState &S, const crgpu_tsne_args *a, double eta, hipEvent_t *ev) {
    CR_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    for (uint32_t it = 0; it < a->n_iters; it++) {
        const uint64_t iter = (uint64_t)a->first_iter + it;
        CR_TRY(tsne_repulsion<DIMS>(ctx, S, it + 1u == a->n_iters ? ev + 2 : nullptr));
        TsneStep st = {iter < a->stop_lying_iter ? TSNE_EXAGGERATION : 1.0, iter < a->mom_switch_iter ? 0.5 : 0.8, eta, S.n, S.seams.wave_row_len, 1u};
        CR_TRY(tsne_attraction<DIMS>(ctx, S, st));
        cr_colsums(ctx, S.Ynew.as<double>(), S.n, DIMS, DIMS, S.parts.as<double>(), S.sums());
        hipLaunchKernelGGL(k_tsne_centre, dim3(cr_grid((uint64_t)S.n * DIMS, TSNE_WG)), dim3(TSNE_WG), 0, ctx->stream, S.Ynew.as<double>(), (uint64_t)S.n, DIMS,
                           S.sums(), S.Y.as<double>());
    }
    CR_HIP(ctx, hipGetLastError());
    CR_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    // the cost at the Y the loop ends on, with its own exact Z
    CR_TRY(tsne_repulsion<DIMS>(ctx, S, nullptr));
    return tsne_cost<DIMS>(ctx, S);
}

static void tsne_clear(crgpu_tsne_result *r) {
    r->sum_q = r->kl = r->p_total = 0.0;
    r->fit_ms = r->search_ms = r->csr_ms = r->loop_ms = r->repulse_ms = 0.0;
    r->nnz = r->pairs_evaluated = 0;
    r->row_tile = r->cand_tile = r->slab_rows = r->wave_row_len = r->n_chunks = r->n_groups = r->max_steps = r->reserved = 0;
}
static void tsne_report(crgpu_tsne_result *r, const TsneState &S) {
    r->nnz = S.nnz, r->row_tile = S.seams.row_tile, r->cand_tile = S.seams.cand_tile, r->slab_rows = S.seams.slab_rows;
    r->wave_row_len = S.seams.wave_row_len, r->n_chunks = S.n_chunks, r->n_groups = (S.n + S.seams.slab_rows - 1u) / S.seams.slab_rows;
}

// ---- the entry points ----------------------------------------------------------------------------------------------------------------
extern "C" int crgpu_tsne_affinities_dev(crgpu_ctx *ctx, const int32_t *nn_indices, const double *nn_distances, uint64_t n, uint32_t k, double perplexity,
                                         const crgpu_tsne_args *a, crgpu_tsne_result *res) {
    if (!ctx || !nn_indices || !nn_distances || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const char *who = "crgpu_tsne_affinities_dev";
    // every refusal below comes before the device is touched
    CR_REQUIRE(ctx, n >= 2 && n < (1ull << 31), CRGPU_EINVAL, "%s: %llu rows, 2 to 2^31 - 1", who, (unsigned long long)n);
    CR_REQUIRE(ctx, k >= 1 && k <= CRGPU_KNN_MAX_K && k < n, CRGPU_EINVAL, "%s: k = %u, 1 to min(%u, the %llu rows - 1)", who, k, CRGPU_KNN_MAX_K,
               (unsigned long long)n);
    CR_REQUIRE(ctx, std::isfinite(perplexity) && perplexity >= 1.0, CRGPU_EINVAL, "%s: a perplexity of %g, finite and at least 1", who, perplexity);
    CR_REQUIRE(ctx, a->reserved == 0u, CRGPU_EINVAL, "%s: reserved is 0", who);
    CR_REQUIRE(ctx, 2 * n * k < (1ull << 32), CRGPU_ERANGE, "%s: %llu neighbour pairs, fewer than 2^31", who, (unsigned long long)(n * k));
    CR_TRY(cr_check_knn_lists(ctx, who, nn_indices, nn_distances, n, k));
    const auto t0 = std::chrono::steady_clock::now();
    tsne_clear(res);
    const uint64_t nk = n * k, n2 = 2 * nk;
    DevBuf nn_b, dist_b, beta_b, steps_b, cond_b, keys_b, keyt_b, perm_b, permt_b, ckeys_b, val_b, ind_b, ptr_b, block_b, parts_b, scal_b;
    CR_TRY(dmalloc(ctx, nn_b, nk * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, dist_b, nk * sizeof(double)));
    CR_TRY(dmalloc(ctx, beta_b, n * sizeof(double)));
    CR_TRY(dmalloc(ctx, steps_b, n * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, cond_b, nk * sizeof(double)));
    CR_TRY(dmalloc(ctx, keys_b, n2 * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, keyt_b, n2 * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, perm_b, n2 * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, permt_b, n2 * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, ckeys_b, n2 * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, val_b, n2 * sizeof(double)));
    CR_TRY(dmalloc(ctx, ind_b, n2 * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, ptr_b, (n + 1) * sizeof(int64_t)));
    CR_TRY(dmalloc(ctx, block_b, 4100 * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, parts_b, ((n2 + GRAPH_PART_ROWS - 1u) / GRAPH_PART_ROWS) * sizeof(double)));
    CR_TRY(dmalloc(ctx, scal_b, 2 * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, nn_b.p, nn_indices, nk * sizeof(int32_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, dist_b.p, nn_distances, nk * sizeof(double)));

    CrEvents<4> events(ctx);
    hipEvent_t *ev = events.e;
    CR_HIP(ctx, hipEventRecord(ev[0], ctx->stream));
    hipLaunchKernelGGL(k_tsne_search, dim3((uint32_t)((n + TSNE_WG - 1u) / TSNE_WG)), dim3(TSNE_WG), 0, ctx->stream, dist_b.as<double>(), (uint32_t)n, k,
                       std::log(perplexity), beta_b.as<double>(), steps_b.as<uint32_t>(), cond_b.as<double>());
    CR_HIP(ctx, hipGetLastError());
    CR_HIP(ctx, hipEventRecord(ev[1], ctx->stream));
    cr_pair_keys(ctx, nn_b.as<int32_t>(), (uint32_t)n, k, keys_b.as<uint64_t>(), perm_b.as<uint32_t>());
    CR_HIP(ctx, hipGetLastError());
    SortedKeys sk;
    CR_TRY(cr_sort_keys(ctx, keys_b.as<uint64_t>(), keyt_b.as<uint64_t>(), perm_b.as<uint32_t>(), permt_b.as<uint32_t>(), n2, cr_ceil_log2(n * n), &sk));
    uint32_t nnz32 = 0;
    CR_TRY(cr_merge_runs(ctx, sk.keys, TsneEmitMerged{sk.keys, sk.perm, cond_b.as<double>(), n2, ckeys_b.as<uint64_t>(), val_b.as<double>()}, n2,
                         block_b.as<uint32_t>(), nk, n2, who, "merged entries", &nnz32));
    const uint64_t nnz = nnz32;
    cr_keys_to_csr(ctx, ckeys_b.as<uint64_t>(), nnz, (uint32_t)n, ptr_b.as<long long>(), ind_b.as<int32_t>(), nullptr);
    cr_colsums(ctx, val_b.as<double>(), nnz, 1u, 1u, parts_b.as<double>(), scal_b.as<double>());
    hipLaunchKernelGGL(k_tsne_divide, dim3(cr_grid(nnz, TSNE_WG)), dim3(TSNE_WG), 0, ctx->stream, val_b.as<double>(), nnz, scal_b.as<double>());
    CR_HIP(ctx, hipGetLastError());
    CR_HIP(ctx, hipEventRecord(ev[2], ctx->stream));

    std::vector<uint32_t> steps(n);
    CR_TRY(crgpu_memcpy_d2h(ctx, steps.data(), steps_b.p, n * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, &res->p_total, scal_b.p, sizeof(double)));
    if (res->beta_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->beta_out, beta_b.p, n * sizeof(double)));
    if (res->steps_out) std::copy(steps.begin(), steps.end(), res->steps_out);
    if (res->cond_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->cond_out, cond_b.p, nk * sizeof(double)));
    if (res->indptr_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->indptr_out, ptr_b.p, (n + 1) * sizeof(int64_t)));
    if (res->indices_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->indices_out, ind_b.p, nnz * sizeof(int32_t)));
    if (res->values_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->values_out, val_b.p, nnz * sizeof(double)));
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms_a = 0.0f, ms_b = 0.0f;
    CR_HIP(ctx, hipEventElapsedTime(&ms_a, ev[0], ev[1]));
    CR_HIP(ctx, hipEventElapsedTime(&ms_b, ev[1], ev[2]));
    res->search_ms = ms_a, res->csr_ms = ms_b, res->nnz = nnz;
    res->max_steps = *std::max_element(steps.begin(), steps.end());
    res->fit_ms = cr_ms_since(t0);
    return CRGPU_OK;
}

extern "C" int crgpu_tsne_gradient_dev(crgpu_ctx *ctx, const int64_t *indptr, const int32_t *indices, const double *values, const double *y, uint64_t n,
                                       uint32_t dims, double exaggeration, const crgpu_tsne_args *a, crgpu_tsne_result *res) {
    if (!ctx || !indptr || !indices || !values || !y || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const char *who = "crgpu_tsne_gradient_dev";
    CR_REQUIRE(ctx, n >= 2 && n < (1ull << 31), CRGPU_EINVAL, "%s: %llu rows, 2 to 2^31 - 1", who, (unsigned long long)n);
    CR_REQUIRE(ctx, dims == 2u || dims == 3u, CRGPU_EINVAL, "%s: %u dimensions, 2 or 3", who, dims);
    CR_REQUIRE(ctx, std::isfinite(exaggeration), CRGPU_EINVAL, "%s: an exaggeration of %g", who, exaggeration);
    TsneSeams seams;
    CR_TRY(tsne_seams(ctx, who, a, n, dims, &seams));
    uint64_t nnz = 0;
    CR_TRY(tsne_check_csr(ctx, who, indptr, indices, values, n, &nnz));
    CR_TRY(tsne_check_finite(ctx, who, "y", y, n * dims));
    const auto t0 = std::chrono::steady_clock::now();
    tsne_clear(res);
    TsneState S;
    CR_TRY(tsne_state(ctx, S, indptr, indices, values, y, n, dims, nnz, seams));
    CR_TRY(dims == 2u ? tsne_gradient<2>(ctx, S, exaggeration) : tsne_gradient<3>(ctx, S, exaggeration));
    if (res->grad_out) CR_TRY(crgpu_memcpy_d2h(ctx, res->grad_out, S.grad.p, n * dims * sizeof(double)));
    CR_TRY(crgpu_memcpy_d2h(ctx, &res->sum_q, S.zq(), sizeof(double)));
    CR_TRY(crgpu_memcpy_d2h(ctx, &res->kl, S.klq(), sizeof(double)));
    tsne_report(res, S);
    res->pairs_evaluated = n * (n - 1);
    res->fit_ms = cr_ms_since(t0);
    return CRGPU_OK;
}

extern "C" int crgpu_tsne_dev(crgpu_ctx *ctx, const int64_t *indptr, const int32_t *indices, const double *values, uint64_t n, uint32_t dims, double *y,
                              double *uY, double *gains, const crgpu_tsne_args *a, crgpu_tsne_result *res) {
    if (!ctx || !indptr || !indices || !values || !y || !uY || !gains || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    const char *who = "crgpu_tsne_dev";
    CR_REQUIRE(ctx, n >= 2 && n < (1ull << 31), CRGPU_EINVAL, "%s: %llu rows, 2 to 2^31 - 1", who, (unsigned long long)n);
    CR_REQUIRE(ctx, dims == 2u || dims == 3u, CRGPU_EINVAL, "%s: %u dimensions, 2 or 3", who, dims);
    const double eta = a->eta == 0.0 ? 200.0 : a->eta;
    CR_REQUIRE(ctx, std::isfinite(eta) && eta > 0.0, CRGPU_EINVAL, "%s: eta = %g, finite and positive (0 = 200)", who, a->eta);
    CR_REQUIRE(ctx, (uint64_t)a->first_iter + a->n_iters <= a->max_iter, CRGPU_EINVAL, "%s: iterations %u + %u of %u", who, a->first_iter, a->n_iters,
               a->max_iter);
    TsneSeams seams;
    CR_TRY(tsne_seams(ctx, who, a, n, dims, &seams));
    uint64_t nnz = 0;
    CR_TRY(tsne_check_csr(ctx, who, indptr, indices, values, n, &nnz));
    CR_TRY(tsne_check_finite(ctx, who, "y", y, n * dims));
    CR_TRY(tsne_check_finite(ctx, who, "uY", uY, n * dims));
    CR_TRY(tsne_check_finite(ctx, who, "gains", gains, n * dims));
    const auto t0 = std::chrono::steady_clock::now();
    tsne_clear(res);
    TsneState S;
    CR_TRY(tsne_state(ctx, S, indptr, indices, values, y, n, dims, nnz, seams));
    const uint64_t yb = n * dims * sizeof(double);
    CR_TRY(crgpu_memcpy_h2d(ctx, S.uY.p, uY, yb));
    CR_TRY(crgpu_memcpy_h2d(ctx, S.gains.p, gains, yb));
    CrEvents<4> events(ctx);
    CR_TRY(dims == 2u ? tsne_loop<2>(ctx, S, a, eta, events.e) : tsne_loop<3>(ctx, S, a, eta, events.e));
    CR_TRY(crgpu_memcpy_d2h(ctx, y, S.Y.p, yb));
    CR_TRY(crgpu_memcpy_d2h(ctx, uY, S.uY.p, yb));
    CR_TRY(crgpu_memcpy_d2h(ctx, gains, S.gains.p, yb));
    CR_TRY(crgpu_memcpy_d2h(ctx, &res->sum_q, S.zq(), sizeof(double)));
    CR_TRY(crgpu_memcpy_d2h(ctx, &res->kl, S.klq(), sizeof(double)));
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    CR_HIP(ctx, hipEventElapsedTime(&ms, events.e[0], events.e[1]));
    res->loop_ms = ms;
    if (a->n_iters) {
        CR_HIP(ctx, hipEventElapsedTime(&ms, events.e[2], events.e[3]));
        res->repulse_ms = ms;
    }
    tsne_report(res, S);
    res->pairs_evaluated = n * (n - 1) * ((uint64_t)a->n_iters + 1u);
    res->fit_ms = cr_ms_since(t0);
    return CRGPU_OK;
}
