// pca.hip -- RUN_PCA on the device: the dispersion order of the features, the IRLBA operator and the projection of every barcode.
//
// Replaces run_pca with normalize_and_transpose (lib/python/cellranger/analysis/pca.py:49-209, 212-229), normalize_by_umi,
// summarize_columns and get_normalized_dispersion (analysis/stats.py), irlb (analysis/irlb.py:61-231) and select_axes_above_threshold
// (matrix.py:788-810).  The retry of the stage (threshold 2, then 0) is the caller's: crgpu_pca_result.status says why a call gave
// nothing.  All of it f64, unfused (-ffp-contract=off), no floating-point atomic, no graph, no cooperative launch; every kernel loop
// is bounded by its arguments.
//
// Host arithmetic (exported, no device): crgpu_legacy_randn (MT19937 + the legacy polar method), crgpu_normalized_dispersion
// (np.percentile, np.unique, binned_statistic's medians), crgpu_small_svd (one-sided Jacobi), and the stable NaN-last order of the
// dispersions.
//
// A preparation (pca_prepare), run for the thresholded matrix (unlogged: the dispersion), the PCA matrix and the full matrix:
//   k_pca_count       a wave per barcode: the entries that map to a used feature; the sums are crgpu_matrix_dev_column_sums' under the
//                     mask of the used features, their median comes through the radix sort, the factors median / sum are host f64
//   k_pca_fill        a wave per barcode compacts its entries in order (ballot + popcount): the feature, the value count * factor or
//                     log2(1 + count * factor), the key feature * N + barcode
//   the radix sort    of the keys with the entry number as payload: the transpose
//   k_pca_gather      the transposed values and barcodes;  k_pca_tptr  the first entry of every feature (a search per feature)
//   k_pca_meanvar     a wave per feature over its transposed entries, scikit-learn 1.7.2's mean_variance_axis: lane l takes the entries
//                     l, l + 64, ..., the lanes are joined by the tree 32, 16, 8, 4, 2, 1; the terms of the implicit zeros are added
//                     by lane 0 as the formula has them
//   k_pca_scale       value *= (1 / scale)[feature], once, then the gather again
// The operator A - 1 c^T:  k_pca_av  w = A v - (c . v), a wave per cell;  k_pca_atw  f = A^T w - (sum w) c, a wave per feature.  The
// sum order of an output element depends on the number of its entries alone (lane l: l, l + 64, ...; the same tree).
// The dense steps:  k_pca_dots  the dots of a vector with the first j columns of V or W over partials of 256 rows (a wave takes a
// column, a lane four rows, the tree), plain stores to a slab;  k_pca_dots_finish  adds the partials in order;  k_pca_update  y -= X c;
// k_pca_axpy, k_pca_scal;  k_pca_small_product  the restart products, tall-skinny times small.
// The projection:  k_pca_project  a wave per barcode of the full matrix, eight components at a time in registers.
// The loop is the host's, statement by statement as irlb has it; it reads s and fn (two scalars a step).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <numeric>
#include <vector>

#include "stage_common.h"

#define PCA_WG 256u
#define PCA_PART_ROWS 256u     // rows of a partial of the dots: fixed, no seam moves it
#define PCA_MAX_MB 148u        // min(nu + 20, 3 nu) at nu = 128
#define PCA_TOL 1e-4
#define PCA_MAXIT 50u
#define PCA_NBINS 20u
#define PCA_PROJ_CHUNK 8u

// ---- host: np.random.RandomState(seed).randn(n) ------------------------------------------------------------------------------------
struct PcaMt {
    uint32_t mt[624];
    int pos;
    explicit PcaMt(uint32_t seed) {
        for (int i = 0; i < 624; i++) {  // init_genrand
            mt[i] = seed;
            seed = 1812433253u * (seed ^ (seed >> 30)) + (uint32_t)i + 1u;
        }
        pos = 624;
    }
    uint32_t next() {
        if (pos == 624) {
            for (int i = 0; i < 624; i++) {
                const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            pos = 0;
        }
        uint32_t y = mt[pos++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return y;
    }
    double next_double() {  // 53 bits from two words
        const uint32_t a = next() >> 5, b = next() >> 6;
        return ((double)a * 67108864.0 + (double)b) / 9007199254740992.0;
    }
};

extern "C" int crgpu_legacy_randn(uint32_t seed, uint64_t n, double *out) {
    if (!out && n) return CRGPU_EINVAL;
    PcaMt rng(seed);
    bool has = false;
    double cached = 0.0;
    for (uint64_t i = 0; i < n; i++) {
        if (has) {
            out[i] = cached, has = false;
            continue;
        }
        double x1, x2, r2;
        do {
            x1 = 2.0 * rng.next_double() - 1.0;
            x2 = 2.0 * rng.next_double() - 1.0;
            r2 = x1 * x1 + x2 * x2;
        } while (r2 >= 1.0 || r2 == 0.0);
        const double f = std::sqrt(-2.0 * std::log(r2) / r2);
        cached = f * x1, has = true;  // the second value of the pair waits for the next call
        out[i] = f * x2;
    }
    return CRGPU_OK;
}

// ---- host: get_normalized_dispersion -----------------------------------------------------------------------------------------------
// np.sort's order of doubles: NaN after every number
static inline bool pca_less(double a, double b) { return a < b || (std::isnan(b) && !std::isnan(a)); }
// np.median: NaN when a value is NaN; the middle value, or (a + b) / 2 of the two middle ones
static double pca_median(std::vector<double> &v) {
    std::sort(v.begin(), v.end(), pca_less);
    if (std::isnan(v.back())) return std::nan("");
    const size_t n = v.size();
    return n % 2 ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0;
}
// scipy.stats.binned_statistic(x, values, "median", bins = edges): bin[i] from 1 (np.digitize: the edges <= x; x == the last edge goes
// to the last bin), med[b - 1] the median of bin b, NaN when it is empty
static void pca_binned_median(const double *x, const double *values, uint64_t n, const std::vector<double> &edges, std::vector<uint32_t> &bin,
                              std::vector<double> &med) {
    const size_t nb = edges.size() - 1;
    std::vector<std::vector<double>> per(nb);
    bin.resize(n);
    for (uint64_t i = 0; i < n; i++) {
        size_t b = (size_t)(std::upper_bound(edges.begin(), edges.end(), x[i]) - edges.begin());
        if (x[i] == edges.back()) b = nb;
        b = std::min(std::max<size_t>(b, 1), nb);  // every x lies inside the edges: they start at its minimum and end at its maximum
        bin[i] = (uint32_t)b;
        per[b - 1].push_back(values[i]);
    }
    med.assign(nb, std::nan(""));
    for (size_t b = 0; b < nb; b++)
        if (!per[b].empty()) med[b] = pca_median(per[b]);
}

extern "C" int crgpu_normalized_dispersion(const double *mu, const double *var, uint64_t n, uint32_t nbins, double *out) {
    if (!mu || !var || !out || n == 0 || nbins == 0 || nbins > 100) return CRGPU_EINVAL;
    std::vector<double> disp(n);
    for (uint64_t i = 0; i < n; i++) disp[i] = (var[i] - mu[i]) / (mu[i] * mu[i]);
    std::vector<double> sorted(mu, mu + n);
    for (double v : sorted)
        if (std::isnan(v)) return CRGPU_EINVAL;
    std::sort(sorted.begin(), sorted.end());
    std::vector<double> q;
    for (uint32_t p = 0; p < 100; p += 100 / nbins) q.push_back(cr_quantile_sorted(sorted, (double)p / 100.0));  // np.arange(0, 100, 100 // nbins)
    q.push_back(sorted.back());
    std::sort(q.begin(), q.end());
    q.erase(std::unique(q.begin(), q.end()), q.end());
    if (q.size() <= 1) {  // every mean the same: the raw dispersion
        std::copy(disp.begin(), disp.end(), out);
        return CRGPU_OK;
    }
    std::vector<uint32_t> bin;
    std::vector<double> meds, mads, dev(n);
    pca_binned_median(mu, disp.data(), n, q, bin, meds);
    for (uint64_t i = 0; i < n; i++) dev[i] = std::fabs(disp[i] - meds[bin[i] - 1]);
    pca_binned_median(mu, dev.data(), n, q, bin, mads);
    for (uint64_t i = 0; i < n; i++) out[i] = (disp[i] - meds[bin[i] - 1]) / mads[bin[i] - 1];  // x / 0 and 0 / 0 as IEEE has them
    return CRGPU_OK;
}

// np.argsort(dispersion, kind = "stable")[-count:]
static std::vector<uint32_t> pca_feature_order(const std::vector<double> &disp, uint32_t count) {
    std::vector<uint32_t> order(disp.size());
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return pca_less(disp[a], disp[b]); });
    return std::vector<uint32_t>(order.end() - count, order.end());
}

// ---- host: the SVD of B ------------------------------------------------------------------------------------------------------------
// One-sided Jacobi (Hestenes) in f64 on the columns of A = B V (row-major n x n): B V = U S.  The pairs (p, q), p < q, are taken in
// row-cyclic order until a sweep rotates nothing.  A first run starts from V = I.  Its rounding errors grow with the number of rotations a
// column has seen, so V is then made orthonormal again (Gram-Schmidt, twice), A = B V is taken afresh (B is bidiagonal with one full
// column: two or three products an entry) and the sweeps run once more, from nearly orthogonal columns: a sweep or two of tiny angles.
// That is done twice.  The singular values are the column norms, descending (equal ones by column).
// SIGN RULE: no sign is normalised -- a singular pair carries the sign these rotations leave it, a function of B alone.
static void pca_jacobi_sweeps(std::vector<double> &A, std::vector<double> &V, uint32_t n) {
    const double eps = std::numeric_limits<double>::epsilon();
    for (uint32_t sweep = 0; sweep < 60u; sweep++) {
        bool rotated = false;
        for (uint32_t p = 0; p + 1 < n; p++)
            for (uint32_t q = p + 1; q < n; q++) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (uint32_t i = 0; i < n; i++) {
                    const double ap = A[(size_t)i * n + p], aq = A[(size_t)i * n + q];
                    alpha += ap * ap, beta += aq * aq, gamma += ap * aq;
                }
                if (gamma == 0.0 || std::fabs(gamma) <= eps * std::sqrt(alpha * beta)) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), sn = c * t;
                for (uint32_t i = 0; i < n; i++) {
                    double &ap = A[(size_t)i * n + p], &aq = A[(size_t)i * n + q];
                    const double x = ap, y = aq;
                    ap = c * x - sn * y, aq = sn * x + c * y;
                    double &vp = V[(size_t)i * n + p], &vq = V[(size_t)i * n + q];
                    const double vx = vp, vy = vq;
                    vp = c * vx - sn * vy, vq = sn * vx + c * vy;
                }
            }
        if (!rotated) break;
    }
}
extern "C" int crgpu_small_svd(const double *B, uint32_t n, double *U, double *s, double *Vt) {
    if (!B || !U || !s || !Vt || n == 0 || n > PCA_MAX_MB) return CRGPU_EINVAL;
    for (uint32_t i = 0; i < n * n; i++)
        if (!std::isfinite(B[i])) return CRGPU_EINVAL;
    std::vector<double> A(B, B + (size_t)n * n), V((size_t)n * n, 0.0);
    for (uint32_t i = 0; i < n; i++) V[(size_t)i * n + i] = 1.0;
    pca_jacobi_sweeps(A, V, n);
    for (uint32_t refine = 0; refine < 2u; refine++) {
        for (uint32_t j = 0; j < n; j++) {  // the columns of V orthonormal again
            for (uint32_t pass = 0; pass < 2u; pass++)
                for (uint32_t c = 0; c < j; c++) {
                    double d = 0.0;
                    for (uint32_t i = 0; i < n; i++) d += V[(size_t)i * n + j] * V[(size_t)i * n + c];
                    for (uint32_t i = 0; i < n; i++) V[(size_t)i * n + j] -= d * V[(size_t)i * n + c];
                }
            double a = 0.0;
            for (uint32_t i = 0; i < n; i++) a += V[(size_t)i * n + j] * V[(size_t)i * n + j];
            a = std::sqrt(a);
            for (uint32_t i = 0; i < n; i++) V[(size_t)i * n + j] /= a;
        }
        for (uint32_t i = 0; i < n; i++)
            for (uint32_t j = 0; j < n; j++) {
                double acc = 0.0;
                for (uint32_t k = 0; k < n; k++)
                    if (B[(size_t)i * n + k] != 0.0) acc += B[(size_t)i * n + k] * V[(size_t)k * n + j];
                A[(size_t)i * n + j] = acc;
            }
        pca_jacobi_sweeps(A, V, n);
    }
    std::vector<double> norm(n);
    std::vector<uint32_t> order(n);
    for (uint32_t j = 0; j < n; j++) {
        double a = 0.0;
        for (uint32_t i = 0; i < n; i++) a += A[(size_t)i * n + j] * A[(size_t)i * n + j];
        norm[j] = std::sqrt(a), order[j] = j;
    }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return norm[a] > norm[b]; });
    for (uint32_t r = 0; r < n; r++) {
        const uint32_t j = order[r];
        s[r] = norm[j];
        for (uint32_t i = 0; i < n; i++) Vt[(size_t)r * n + i] = V[(size_t)i * n + j];
        if (norm[j] > 0.0)
            for (uint32_t i = 0; i < n; i++) U[(size_t)i * n + r] = A[(size_t)i * n + j] / norm[j];
        else
            for (uint32_t i = 0; i < n; i++) U[(size_t)i * n + r] = 0.0;
    }
    // a singular value of exactly 0 leaves its left vector open: the first unit vectors, orthogonalised against the columns before
    for (uint32_t r = 0; r < n; r++) {
        if (s[r] > 0.0) continue;
        for (uint32_t e = 0; e < n; e++) {
            std::vector<double> u(n, 0.0);
            u[e] = 1.0;
            for (uint32_t pass = 0; pass < 2u; pass++)
                for (uint32_t c = 0; c < n; c++) {
                    if (c == r || (s[c] == 0.0 && c > r)) continue;
                    double d = 0.0;
                    for (uint32_t i = 0; i < n; i++) d += u[i] * U[(size_t)i * n + c];
                    for (uint32_t i = 0; i < n; i++) u[i] -= d * U[(size_t)i * n + c];
                }
            double a = 0.0;
            for (uint32_t i = 0; i < n; i++) a += u[i] * u[i];
            if (a < 0.25) continue;
            a = std::sqrt(a);
            for (uint32_t i = 0; i < n; i++) U[(size_t)i * n + r] = u[i] / a;
            break;
        }
    }
    return CRGPU_OK;
}

// ---- device: the preparation --------------------------------------------------------------------------------------------------------
// cnt[b] = the entries of barcode b (column bcs[b], or b) whose row maps to a used feature (fmap NULL: every row); sums[b] = sums_all[column]
__global__ __launch_bounds__(PCA_WG) void k_pca_count(const long long *__restrict__ indptr, const int32_t *__restrict__ indices, const uint32_t *__restrict__ bcs,
                                                      uint64_t N, uint32_t G, const int32_t *__restrict__ fmap, const uint32_t *__restrict__ sums_all,
                                                      uint32_t *__restrict__ cnt, uint32_t *__restrict__ sums, uint32_t *__restrict__ flag) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t b = wave0; b < N; b += n_waves) {
        const uint64_t c = bcs ? bcs[b] : b;
        const long long s = indptr[c], e = indptr[c + 1];
        uint32_t n = 0;
        for (long long i = s + lane; i < e; i += 64) {
            const uint32_t r = (uint32_t)indices[i];
            if (r >= G) atomicOr(flag, 1u);
            else if (!fmap || fmap[r] >= 0) n++;
        }
        n = wave_sum(n);
        if (lane == 0u) cnt[b] = n, sums[b] = sums_all[c];
    }
}
// counts[row] += count over the listed barcodes: integers, exact in any order
__global__ __launch_bounds__(PCA_WG) void k_pca_feature_counts(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                               const int32_t *__restrict__ data, const uint32_t *__restrict__ bcs, uint64_t N, uint32_t G,
                                                               unsigned long long *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t b = wave0; b < N; b += n_waves) {
        const uint64_t c = bcs[b];
        const long long s = indptr[c], e = indptr[c + 1];
        for (long long i = s + lane; i < e; i += 64) {
            const uint32_t r = (uint32_t)indices[i];
            if (r < G) atomicAdd(counts + r, (unsigned long long)(uint32_t)data[i]);
        }
    }
}
// the used entries of a barcode in their order, from rowptr[b]: feature, value, key, entry number
__global__ __launch_bounds__(PCA_WG) void k_pca_fill(const long long *__restrict__ indptr, const int32_t *__restrict__ indices, const int32_t *__restrict__ data,
                                                     const uint32_t *__restrict__ bcs, uint64_t N, uint32_t G, const int32_t *__restrict__ fmap,
                                                     const double *__restrict__ factor, int logged, const uint64_t *__restrict__ rowptr,
                                                     uint32_t *__restrict__ col, double *__restrict__ val, uint64_t *__restrict__ keys, uint32_t *__restrict__ perm) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t b = wave0; b < N; b += n_waves) {
        const uint64_t c = bcs ? bcs[b] : b;
        const long long s = indptr[c], e = indptr[c + 1];
        const uint64_t end = rowptr[b + 1];
        const double fac = factor[b];
        uint64_t at = rowptr[b];
        for (long long base = s; base < e; base += 64) {  // uniform over the wave
            const long long i = base + lane;
            int32_t f = -1;
            if (i < e) {
                const uint32_t r = (uint32_t)indices[i];
                if (r < G) f = fmap ? fmap[r] : (int32_t)r;
            }
            const unsigned long long m = __ballot(f >= 0);
            const uint64_t pos = at + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
            if (f >= 0 && pos < end) {  // pos < end: the counts came from the same entries
                const double x = (double)data[i] * fac;
                col[pos] = (uint32_t)f;
                val[pos] = logged ? log2(1.0 + x) : x;
                keys[pos] = (uint64_t)(uint32_t)f * N + b;
                perm[pos] = (uint32_t)pos;
            }
            at += (uint64_t)__popcll(m);
        }
    }
}
__global__ __launch_bounds__(PCA_WG) void k_pca_gather(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ perm, const double *__restrict__ val,
                                                       uint64_t N, uint64_t nnz, double *__restrict__ tval, uint32_t *__restrict__ tcell) {
    for (uint64_t i = (uint64_t)blockIdx.x * PCA_WG + threadIdx.x; i < nnz; i += (uint64_t)gridDim.x * PCA_WG) {
        const uint32_t p = perm[i];
        tval[i] = p < nnz ? val[p] : 0.0;
        tcell[i] = (uint32_t)(keys[i] % N);
    }
}
__global__ __launch_bounds__(PCA_WG) void k_pca_tptr(const uint64_t *__restrict__ keys, uint64_t nnz, uint64_t N, uint32_t F, uint64_t *__restrict__ tptr) {
    const uint32_t f = blockIdx.x * PCA_WG + threadIdx.x;
    if (f > F) return;
    tptr[f] = f == F ? nnz : cr_lower_bound(keys, nnz, (uint64_t)f * N);
}
// mean_variance_axis of scikit-learn 1.7.2 (sparsefuncs_fast.pyx, _csr_mean_variance_axis0, unit weights) per feature
__global__ __launch_bounds__(PCA_WG) void k_pca_meanvar(const uint64_t *__restrict__ tptr, const double *__restrict__ tval, uint64_t N, uint32_t F,
                                                        double *__restrict__ mean_out, double *__restrict__ var_out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const double n = (double)N;
    for (uint64_t f = wave0; f < F; f += n_waves) {
        const uint64_t lo = tptr[f], hi = tptr[f + 1];
        double sum = 0.0;
        for (uint64_t i = lo + lane; i < hi; i += 64u) sum += tval[i];
        sum = wave_sum(sum);
        const double mean = __shfl(sum, 0) / n;
        double corr = 0.0, var = 0.0;
        for (uint64_t i = lo + lane; i < hi; i += 64u) {
            const double diff = tval[i] - mean;
            corr += diff, var += diff * diff;
        }
        corr = wave_sum(corr), var = wave_sum(var);
        if (lane == 0u) {
            const double n_zero = (double)(N - (hi - lo));
            if (hi - lo != N) corr -= n_zero * mean;
            corr = corr * corr / n;
            if (hi - lo != N) var += n_zero * (mean * mean);
            mean_out[f] = mean, var_out[f] = (var - corr) / n;
        }
    }
}
__global__ __launch_bounds__(PCA_WG) void k_pca_scale(double *__restrict__ val, const uint32_t *__restrict__ col, uint64_t nnz, const double *__restrict__ inv_scale) {
    for (uint64_t i = (uint64_t)blockIdx.x * PCA_WG + threadIdx.x; i < nnz; i += (uint64_t)gridDim.x * PCA_WG) val[i] *= inv_scale[col[i]];
}

// ---- device: the operator -----------------------------------------------------------------------------------------------------------
// w[cell] = sum over the cell's entries of value * v[feature], minus scal[0] = c . v
__global__ __launch_bounds__(PCA_WG) void k_pca_av(const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ col, const double *__restrict__ val, uint64_t N,
                                                   const double *__restrict__ v, const double *__restrict__ scal, double *__restrict__ w) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const double cv = scal[0];
    for (uint64_t c = wave0; c < N; c += n_waves) {
        const uint64_t lo = rowptr[c], hi = rowptr[c + 1];
        double a = 0.0;
        for (uint64_t i = lo + lane; i < hi; i += 64u) a += val[i] * v[col[i]];
        a = wave_sum(a);
        if (lane == 0u) w[c] = a - cv;
    }
}
// f[feature] = sum over the feature's transposed entries of value * w[cell], minus scal[1] * c[feature]  (scal[1] = sum w)
__global__ __launch_bounds__(PCA_WG) void k_pca_atw(const uint64_t *__restrict__ tptr, const uint32_t *__restrict__ tcell, const double *__restrict__ tval, uint32_t F,
                                                    const double *__restrict__ w, const double *__restrict__ scal, const double *__restrict__ center,
                                                    double *__restrict__ f_out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const double sw = scal[1];
    for (uint64_t f = wave0; f < F; f += n_waves) {
        const uint64_t lo = tptr[f], hi = tptr[f + 1];
        double a = 0.0;
        for (uint64_t i = lo + lane; i < hi; i += 64u) a += tval[i] * w[tcell[i]];
        a = wave_sum(a);
        if (lane == 0u) f_out[f] = a - sw * center[f];
    }
}

// ---- device: the dense steps ----------------------------------------------------------------------------------------------------------
// slab[part][c] = the dot of y with column c of X (column-major, stride ld) over the rows part * 256 .. + 255: a workgroup takes
// parts_per_block partials, a wave the columns wave, wave + 4, ...; a lane the rows lane, lane + 64, lane + 128, lane + 192 of the partial
__global__ __launch_bounds__(PCA_WG) void k_pca_dots(const double *__restrict__ y, const double *__restrict__ X, uint64_t ld, uint32_t ncols, uint64_t n,
                                                     uint32_t n_parts, uint32_t parts_per_block, double *__restrict__ slab) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t q = 0; q < parts_per_block; q++) {
        const uint32_t part = blockIdx.x * parts_per_block + q;
        if (part >= n_parts) return;  // uniform over the workgroup
        const uint64_t r0 = (uint64_t)part * PCA_PART_ROWS + lane;
        double yv[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; u++) yv[u] = r0 + 64u * u < n ? y[r0 + 64u * u] : 0.0;
        for (uint32_t c = wave; c < ncols; c += PCA_WG / 64u) {
            const double *x = X + (size_t)c * ld;
            double a = 0.0;
#pragma unroll
            for (uint32_t u = 0; u < 4u; u++) a += r0 + 64u * u < n ? yv[u] * x[r0 + 64u * u] : 0.0;
            a = wave_sum(a);
            if (lane == 0u) slab[(size_t)part * ncols + c] = a;
        }
    }
}
__global__ __launch_bounds__(PCA_WG) void k_pca_dots_finish(const double *__restrict__ slab, uint32_t n_parts, uint32_t ncols, double *__restrict__ out) {
    const uint32_t c = blockIdx.x * PCA_WG + threadIdx.x;
    if (c >= ncols) return;
    double a = 0.0;
    for (uint32_t p = 0; p < n_parts; p++) a += slab[(size_t)p * ncols + c];
    out[c] = a;
}
// y -= X c over the first ncols columns, in column order
__global__ __launch_bounds__(PCA_WG) void k_pca_update(double *__restrict__ y, const double *__restrict__ X, uint64_t ld, uint32_t ncols,
                                                       const double *__restrict__ coef, uint64_t n) {
    for (uint64_t r = (uint64_t)blockIdx.x * PCA_WG + threadIdx.x; r < n; r += (uint64_t)gridDim.x * PCA_WG) {
        double a = 0.0;
        for (uint32_t c = 0; c < ncols; c++) a += X[(size_t)c * ld + r] * coef[c];
        y[r] = y[r] - a;
    }
}
__global__ __launch_bounds__(PCA_WG) void k_pca_axpy(double *__restrict__ y, double alpha, const double *__restrict__ x, uint64_t n) {
    for (uint64_t r = (uint64_t)blockIdx.x * PCA_WG + threadIdx.x; r < n; r += (uint64_t)gridDim.x * PCA_WG) y[r] = y[r] - alpha * x[r];
}
__global__ __launch_bounds__(PCA_WG) void k_pca_scal(double *__restrict__ y, double alpha, uint64_t n) {
    for (uint64_t r = (uint64_t)blockIdx.x * PCA_WG + threadIdx.x; r < n; r += (uint64_t)gridDim.x * PCA_WG) y[r] = alpha * y[r];
}
__global__ __launch_bounds__(PCA_WG) void k_pca_fill_ones(double *__restrict__ y, uint64_t n) {
    for (uint64_t r = (uint64_t)blockIdx.x * PCA_WG + threadIdx.x; r < n; r += (uint64_t)gridDim.x * PCA_WG) y[r] = 1.0;
}
// out[:, c] = X[:, 0:mb] M[:, c] for c < k, M row-major mb x k, t ascending
__global__ __launch_bounds__(PCA_WG) void k_pca_small_product(const double *__restrict__ X, uint64_t ld, uint64_t n, uint32_t mb, const double *__restrict__ M,
                                                              uint32_t k, double *__restrict__ out) {
    const uint64_t total = n * k;
    for (uint64_t e = (uint64_t)blockIdx.x * PCA_WG + threadIdx.x; e < total; e += (uint64_t)gridDim.x * PCA_WG) {
        const uint64_t r = e % n;
        const uint32_t c = (uint32_t)(e / n);
        double a = 0.0;
        for (uint32_t t = 0; t < mb; t++) a += X[(size_t)t * ld + r] * M[(size_t)t * k + c];
        out[(size_t)c * ld + r] = a;
    }
}

// ---- device: the projection ---------------------------------------------------------------------------------------------------------
// out[b][comp] = sum over the entries of barcode b with pmap[feature] >= 0 of value * v[pmap[feature]][comp], minus cv[comp]; v row-major
// used features x nu.  A barcode without entries gets -cv.
__global__ __launch_bounds__(PCA_WG) void k_pca_project(const uint64_t *__restrict__ rowptr, const uint32_t *__restrict__ col, const double *__restrict__ val,
                                                        uint64_t N, const int32_t *__restrict__ pmap, const double *__restrict__ v, uint32_t nu,
                                                        const double *__restrict__ cv, double *__restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t b = wave0; b < N; b += n_waves) {
        const uint64_t lo = rowptr[b], hi = rowptr[b + 1];
        for (uint32_t c0 = 0; c0 < nu; c0 += PCA_PROJ_CHUNK) {
            double a[PCA_PROJ_CHUNK];
#pragma unroll
            for (uint32_t u = 0; u < PCA_PROJ_CHUNK; u++) a[u] = 0.0;
            for (uint64_t i = lo + lane; i < hi; i += 64u) {
                const int32_t g = pmap[col[i]];
                if (g < 0) continue;
                const double x = val[i];
                const double *vr = v + (size_t)g * nu;
#pragma unroll
                for (uint32_t u = 0; u < PCA_PROJ_CHUNK; u++)
                    if (c0 + u < nu) a[u] += x * vr[c0 + u];
            }
#pragma unroll
            for (uint32_t u = 0; u < PCA_PROJ_CHUNK; u++) {
                const double t = wave_sum(a[u]);
                if (lane == 0u && c0 + u < nu) out[b * nu + c0 + u] = t - cv[c0 + u];
            }
        }
    }
}

// ---- host: the preparation --------------------------------------------------------------------------------------------------------------
struct PcaPrep {  // a normalised sub-matrix, cells x features, in both orders
    uint64_t N = 0, nnz = 0;
    uint32_t F = 0;
    DevBuf rowptr, col, val, keys, keys_tmp, perm, perm_tmp, tval, tcell, tptr;
    bool in_tmp = false;
    std::vector<double> mean, var;
    const uint64_t *d_keys() { return in_tmp ? keys_tmp.as<uint64_t>() : keys.as<uint64_t>(); }
    const uint32_t *d_perm() { return in_tmp ? perm_tmp.as<uint32_t>() : perm.as<uint32_t>(); }
};

static inline uint32_t pca_wave_grid(uint64_t rows, uint32_t wg) { return cr_grid(rows * 64u, wg, 1u << 16); }

static int pca_regather(crgpu_ctx *ctx, PcaPrep &P) {
    if (P.nnz == 0) return CRGPU_OK;
    hipLaunchKernelGGL(k_pca_gather, dim3(cr_grid(P.nnz, PCA_WG)), dim3(PCA_WG), 0, ctx->stream, P.d_keys(), P.d_perm(), P.val.as<double>(), P.N, P.nnz,
                       P.tval.as<double>(), P.tcell.as<uint32_t>());
    CR_HIP(ctx, hipGetLastError());
    return CRGPU_OK;
}

// d_bcs: the columns of m taken as cells (NULL: all N = m->n_barcodes); d_fmap: row of m -> feature 0 .. F - 1 or -1 (NULL: the identity,
// F = G); d_sums_all: per column of m the sum over the used features
static int pca_prepare(crgpu_ctx *ctx, const crgpu_matrix_dev *m, uint32_t G, const uint32_t *d_bcs, uint64_t N, const int32_t *d_fmap, uint32_t F,
                       const uint32_t *d_sums_all, bool logged, uint32_t wg, PcaPrep &P) {
    P.N = N, P.F = F;
    DevBuf cnt_b, sum_b, key_b, keyt_b, fac_b;
    CR_TRY(dmalloc(ctx, cnt_b, N * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, sum_b, N * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, key_b, N * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, keyt_b, N * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, fac_b, N * sizeof(double)));
    uint32_t *d_flag = ctx->d_scalars + CR_SCALAR_FLAG, flag = 0;
    CR_HIP(ctx, hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_pca_count, dim3(pca_wave_grid(N, wg)), dim3(wg), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, d_bcs, N, G, d_fmap,
                       d_sums_all, cnt_b.as<uint32_t>(), sum_b.as<uint32_t>(), d_flag);
    CR_HIP(ctx, hipGetLastError());
    CR_TRY(read_u32(ctx, d_flag, &flag));
    CR_REQUIRE(ctx, !flag, CRGPU_EINVAL, "crgpu_pca_dev: the matrix holds a row >= n_features (%u)", G);
    // the median of the sums through the sort, the factors, the row pointers
    CR_HIP(ctx, hipMemcpyAsync(key_b.p, sum_b.p, N * sizeof(uint32_t), hipMemcpyDeviceToDevice, ctx->stream));
    bool in_tmp = false;
    CR_TRY(cr_radix_sort_u32(ctx, key_b.as<uint32_t>(), keyt_b.as<uint32_t>(), nullptr, nullptr, N, 0, 32, &in_tmp));
    std::vector<uint32_t> cnt(N), sums(N), sorted(N);
    CR_TRY(crgpu_memcpy_d2h(ctx, cnt.data(), cnt_b.p, N * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, sums.data(), sum_b.p, N * sizeof(uint32_t)));
    CR_TRY(crgpu_memcpy_d2h(ctx, sorted.data(), in_tmp ? keyt_b.p : key_b.p, N * sizeof(uint32_t)));
    const double median = std::max(1.0, cr_median_sorted(sorted));
    std::vector<double> factor(N);
    std::vector<uint64_t> rowptr(N + 1, 0);
    for (uint64_t b = 0; b < N; b++) {
        factor[b] = median / (double)sums[b];  // a barcode without counts: x / 0, never used, it has no entries
        rowptr[b + 1] = rowptr[b] + cnt[b];
    }
    const uint64_t nnz = rowptr[N];
    P.nnz = nnz;
    CR_REQUIRE(ctx, nnz < (1ull << 32), CRGPU_ERANGE, "crgpu_pca_dev: %llu entries, fewer than 2^32", (unsigned long long)nnz);
    const uint64_t room = std::max<uint64_t>(nnz, 1);
    CR_TRY(dmalloc(ctx, P.rowptr, (N + 1) * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, P.col, room * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, P.val, room * sizeof(double)));
    CR_TRY(dmalloc(ctx, P.keys, room * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, P.keys_tmp, room * sizeof(uint64_t)));
    CR_TRY(dmalloc(ctx, P.perm, room * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, P.perm_tmp, room * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, P.tval, room * sizeof(double)));
    CR_TRY(dmalloc(ctx, P.tcell, room * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, P.tptr, ((uint64_t)F + 1) * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, P.rowptr.p, rowptr.data(), (N + 1) * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, fac_b.p, factor.data(), N * sizeof(double)));
    DevBuf mean_b, var_b;
    CR_TRY(dmalloc(ctx, mean_b, (uint64_t)F * sizeof(double)));
    CR_TRY(dmalloc(ctx, var_b, (uint64_t)F * sizeof(double)));
    if (nnz) {
        hipLaunchKernelGGL(k_pca_fill, dim3(pca_wave_grid(N, wg)), dim3(wg), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data, d_bcs, N, G,
                           d_fmap, fac_b.as<double>(), logged ? 1 : 0, P.rowptr.as<uint64_t>(), P.col.as<uint32_t>(), P.val.as<double>(), P.keys.as<uint64_t>(),
                           P.perm.as<uint32_t>());
        CR_HIP(ctx, hipGetLastError());
        const uint32_t key_bits = std::max(1u, cr_ceil_log2((uint64_t)F * N));
        CR_TRY(cr_radix_sort_u64(ctx, P.keys.as<uint64_t>(), P.keys_tmp.as<uint64_t>(), P.perm.as<uint32_t>(), P.perm_tmp.as<uint32_t>(), nnz, 0, key_bits,
                                 &P.in_tmp));
    }
    CR_TRY(pca_regather(ctx, P));
    hipLaunchKernelGGL(k_pca_tptr, dim3(F / PCA_WG + 1u), dim3(PCA_WG), 0, ctx->stream, P.d_keys(), nnz, N, F, P.tptr.as<uint64_t>());
    hipLaunchKernelGGL(k_pca_meanvar, dim3(pca_wave_grid(F, wg)), dim3(wg), 0, ctx->stream, P.tptr.as<uint64_t>(), P.tval.as<double>(), N, F, mean_b.as<double>(),
                       var_b.as<double>());
    CR_HIP(ctx, hipGetLastError());
    P.mean.resize(F), P.var.resize(F);
    CR_TRY(crgpu_memcpy_d2h(ctx, P.mean.data(), mean_b.p, (uint64_t)F * sizeof(double)));
    CR_TRY(crgpu_memcpy_d2h(ctx, P.var.data(), var_b.p, (uint64_t)F * sizeof(double)));
    return CRGPU_OK;
}

// value *= (1 / scale)[feature] in both orders; d_inv: device, F doubles
static int pca_scale(crgpu_ctx *ctx, PcaPrep &P, const double *d_inv) {
    if (P.nnz == 0) return CRGPU_OK;
    hipLaunchKernelGGL(k_pca_scale, dim3(cr_grid(P.nnz, PCA_WG)), dim3(PCA_WG), 0, ctx->stream, P.val.as<double>(), P.col.as<uint32_t>(), P.nnz, d_inv);
    CR_HIP(ctx, hipGetLastError());
    return pca_regather(ctx, P);
}

// ---- host: Lanczos ----------------------------------------------------------------------------------------------------------------------
struct PcaLanczos {
    crgpu_ctx *ctx;
    PcaPrep *A;
    uint64_t m, n;  // cells, features
    uint32_t mb, wg, ppb;
    DevBuf V, W, F, tmp, slab, dots, scal, ones, center, small;

    int init(uint32_t mb_) {
        mb = mb_;
        const uint64_t big = std::max(m, n);
        CR_TRY(dmalloc(ctx, V, n * mb * sizeof(double)));
        CR_TRY(dmalloc(ctx, W, m * mb * sizeof(double)));
        CR_TRY(dmalloc(ctx, F, n * sizeof(double)));
        CR_TRY(dmalloc(ctx, tmp, big * mb * sizeof(double)));
        CR_TRY(dmalloc(ctx, slab, ((big + PCA_PART_ROWS - 1) / PCA_PART_ROWS) * mb * sizeof(double)));
        CR_TRY(dmalloc(ctx, dots, mb * sizeof(double)));
        CR_TRY(dmalloc(ctx, scal, 4 * sizeof(double)));
        CR_TRY(dmalloc(ctx, ones, big * sizeof(double)));
        CR_TRY(dmalloc(ctx, center, n * sizeof(double)));
        CR_TRY(dmalloc(ctx, small, (uint64_t)mb * mb * sizeof(double)));
        CR_HIP(ctx, hipMemsetAsync(V.p, 0, n * mb * sizeof(double), ctx->stream));
        CR_HIP(ctx, hipMemsetAsync(W.p, 0, m * mb * sizeof(double), ctx->stream));
        hipLaunchKernelGGL(k_pca_fill_ones, dim3(cr_grid(big, PCA_WG)), dim3(PCA_WG), 0, ctx->stream, ones.as<double>(), big);
        CR_HIP(ctx, hipGetLastError());
        return CRGPU_OK;
    }
    double *Vc(uint32_t j) { return V.as<double>() + (size_t)j * n; }
    double *Wc(uint32_t j) { return W.as<double>() + (size_t)j * m; }
    // out[c] = y . X[:, c], c < ncols (device)
    int dot(const double *y, const double *X, uint64_t ld, uint32_t ncols, uint64_t len, double *out) {
        const uint32_t n_parts = (uint32_t)((len + PCA_PART_ROWS - 1) / PCA_PART_ROWS);
        hipLaunchKernelGGL(k_pca_dots, dim3((n_parts + ppb - 1) / ppb), dim3(PCA_WG), 0, ctx->stream, y, X, ld, ncols, len, n_parts, ppb, slab.as<double>());
        hipLaunchKernelGGL(k_pca_dots_finish, dim3((ncols + PCA_WG - 1) / PCA_WG), dim3(PCA_WG), 0, ctx->stream, slab.as<double>(), n_parts, ncols, out);
        CR_HIP(ctx, hipGetLastError());
        return CRGPU_OK;
    }
    int norm(const double *y, uint64_t len, double *out) {  // np.linalg.norm: the root of y . y
        CR_TRY(dot(y, y, len, 1, len, scal.as<double>() + 2));
        double sq = 0.0;
        CR_TRY(crgpu_memcpy_d2h(ctx, &sq, scal.as<double>() + 2, sizeof(double)));
        *out = std::sqrt(sq);
        return CRGPU_OK;
    }
    int scale(double *y, double alpha, uint64_t len) {
        hipLaunchKernelGGL(k_pca_scal, dim3(cr_grid(len, PCA_WG)), dim3(PCA_WG), 0, ctx->stream, y, alpha, len);
        CR_HIP(ctx, hipGetLastError());
        return CRGPU_OK;
    }
    int axpy(double *y, double alpha, const double *x, uint64_t len) {
        hipLaunchKernelGGL(k_pca_axpy, dim3(cr_grid(len, PCA_WG)), dim3(PCA_WG), 0, ctx->stream, y, alpha, x, len);
        CR_HIP(ctx, hipGetLastError());
        return CRGPU_OK;
    }
    int orthog(double *y, const double *X, uint64_t len, uint32_t ncols) {  // y - X (y . X)
        if (ncols == 0) return CRGPU_OK;
        CR_TRY(dot(y, X, len, ncols, len, dots.as<double>()));
        hipLaunchKernelGGL(k_pca_update, dim3(cr_grid(len, PCA_WG)), dim3(PCA_WG), 0, ctx->stream, y, X, len, ncols, dots.as<double>(), len);
        CR_HIP(ctx, hipGetLastError());
        return CRGPU_OK;
    }
    int av(const double *v, double *w) {  // w = A v - (c . v)
        CR_TRY(dot(center.as<double>(), v, n, 1, n, scal.as<double>()));
        hipLaunchKernelGGL(k_pca_av, dim3(pca_wave_grid(m, wg)), dim3(wg), 0, ctx->stream, A->rowptr.as<uint64_t>(), A->col.as<uint32_t>(), A->val.as<double>(), m, v,
                           scal.as<double>(), w);
        CR_HIP(ctx, hipGetLastError());
        return CRGPU_OK;
    }
    int atw(const double *w, double *f) {  // f = A^T w - (sum w) c
        CR_TRY(dot(w, ones.as<double>(), m, 1, m, scal.as<double>() + 1));
        hipLaunchKernelGGL(k_pca_atw, dim3(pca_wave_grid(n, wg)), dim3(wg), 0, ctx->stream, A->tptr.as<uint64_t>(), A->tcell.as<uint32_t>(), A->tval.as<double>(),
                           (uint32_t)n, w, scal.as<double>(), center.as<double>(), f);
        CR_HIP(ctx, hipGetLastError());
        return CRGPU_OK;
    }
    // X[:, 0:k] = X[:, 0:mb] M, M row-major mb x k on the host
    int small_product(double *X, uint64_t len, const std::vector<double> &M, uint32_t k, double *out) {
        if (k == 0) return CRGPU_OK;
        CR_TRY(crgpu_memcpy_h2d(ctx, small.p, M.data(), (uint64_t)mb * k * sizeof(double)));
        hipLaunchKernelGGL(k_pca_small_product, dim3(cr_grid(len * k, PCA_WG)), dim3(PCA_WG), 0, ctx->stream, X, len, len, mb, small.as<double>(), k,
                           tmp.as<double>());
        CR_HIP(ctx, hipGetLastError());
        CR_HIP(ctx, hipMemcpyAsync(out, tmp.p, len * k * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        return CRGPU_OK;
    }
};

static inline double pca_invcheck(double x) { return x > 2.0 * std::numeric_limits<double>::epsilon() ? 1.0 / x : 0.0; }

// irlb(A, nu, center = c) on the prepared matrix; start: n values, not yet normalised.  d[nu], v[n x nu] row-major
static int pca_irlb(crgpu_ctx *ctx, PcaPrep &A, const std::vector<double> &center, const std::vector<double> &start, uint32_t nu, uint32_t wg, uint32_t ppb,
                    std::vector<double> &d, std::vector<double> &v, uint32_t *it_out, uint32_t *mprod_out, uint32_t *mb_out) {
    PcaLanczos L;
    L.ctx = ctx, L.A = &A, L.m = A.N, L.n = A.F, L.wg = wg, L.ppb = ppb;
    const uint64_t m = L.m, n = L.n;
    const uint32_t mb = (uint32_t)std::min<uint64_t>(std::min<uint64_t>(nu + 20u, 3u * nu), std::min(m, n));
    *mb_out = mb;
    CR_TRY(L.init(mb));
    CR_TRY(crgpu_memcpy_h2d(ctx, L.center.p, center.data(), n * sizeof(double)));
    CR_TRY(crgpu_memcpy_h2d(ctx, L.Vc(0), start.data(), n * sizeof(double)));
    double s = 0.0, fn = 0.0, smax = 1.0;
    CR_TRY(L.norm(L.Vc(0), n, &s));  // the Frobenius norm of the whole V, whose other columns are 0
    CR_REQUIRE(ctx, s > 0.0 && std::isfinite(s), CRGPU_EINVAL, "crgpu_pca_dev: the start vector has the norm %g", s);
    CR_TRY(L.scale(L.Vc(0), 1.0 / s, n));  // V[:, 0] / norm: a division by the norm
    uint32_t it = 0, mprod = 0, j = 0, k = nu;
    std::vector<double> B((size_t)mb * mb, 0.0), U((size_t)mb * mb), S(mb), Vt((size_t)mb * mb), R(mb), M;
    while (it < PCA_MAXIT) {
        if (it > 0) j = k;
        CR_TRY(L.av(L.Vc(j), L.Wc(j)));
        mprod++;
        if (it > 0) CR_TRY(L.orthog(L.Wc(j), L.W.as<double>(), m, j));
        CR_TRY(L.norm(L.Wc(j), m, &s));
        CR_TRY(L.scale(L.Wc(j), pca_invcheck(s), m));
        while (j < mb) {
            double *F = L.F.as<double>();
            CR_TRY(L.atw(L.Wc(j), F));
            mprod++;
            CR_TRY(L.axpy(F, s, L.Vc(j), n));
            CR_TRY(L.orthog(F, L.V.as<double>(), n, j + 1u));
            CR_TRY(L.norm(F, n, &fn));
            CR_TRY(L.scale(F, pca_invcheck(fn), n));
            if (j < mb - 1u) {
                CR_HIP(ctx, hipMemcpyAsync(L.Vc(j + 1u), F, n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
                B[(size_t)j * mb + j] = s, B[(size_t)j * mb + j + 1u] = fn;
                CR_TRY(L.av(L.Vc(j + 1u), L.Wc(j + 1u)));
                mprod++;
                CR_TRY(L.axpy(L.Wc(j + 1u), fn, L.Wc(j), m));
                CR_TRY(L.orthog(L.Wc(j + 1u), L.W.as<double>(), m, j + 1u));
                CR_TRY(L.norm(L.Wc(j + 1u), m, &s));
                CR_TRY(L.scale(L.Wc(j + 1u), pca_invcheck(s), m));
            } else {
                B[(size_t)j * mb + j] = s;
            }
            j++;
        }
        CR_REQUIRE(ctx, crgpu_small_svd(B.data(), mb, U.data(), S.data(), Vt.data()) == CRGPU_OK, CRGPU_ESTATE,
                   "crgpu_pca_dev: B holds a value that is not finite at restart %u", it);
        for (uint32_t i = 0; i < mb; i++) R[i] = fn * U[(size_t)(mb - 1u) * mb + i];
        smax = it < 1u ? S[0] : std::max(S[0], smax);
        uint32_t conv = 0;
        for (uint32_t i = 0; i < nu; i++) conv += std::fabs(R[i]) < PCA_TOL * smax ? 1u : 0u;
        if (conv >= nu) break;
        CR_REQUIRE(ctx, mb >= 3u, CRGPU_ESTATE, "crgpu_pca_dev: a restart with a working dimension of %u (the reference indexes from the end there)", mb);
        k = std::min(std::max(conv + nu, k), mb - 3u);
        M.assign((size_t)mb * k, 0.0);
        for (uint32_t t = 0; t < mb; t++)
            for (uint32_t c = 0; c < k; c++) M[(size_t)t * k + c] = Vt[(size_t)c * mb + t];  // S[2].transpose()[:, 0:k]
        CR_TRY(L.small_product(L.V.as<double>(), n, M, k, L.V.as<double>()));
        CR_HIP(ctx, hipMemcpyAsync(L.Vc(k), L.F.p, n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        std::fill(B.begin(), B.end(), 0.0);
        for (uint32_t l = 0; l < k; l++) B[(size_t)l * mb + l] = S[l], B[(size_t)l * mb + k] = R[l];
        for (uint32_t t = 0; t < mb; t++)
            for (uint32_t c = 0; c < k; c++) M[(size_t)t * k + c] = U[(size_t)t * mb + c];
        CR_TRY(L.small_product(L.W.as<double>(), m, M, k, L.W.as<double>()));
        it++;
    }
    M.assign((size_t)mb * nu, 0.0);
    for (uint32_t t = 0; t < mb; t++)
        for (uint32_t c = 0; c < nu; c++) M[(size_t)t * nu + c] = Vt[(size_t)c * mb + t];
    CR_TRY(crgpu_memcpy_h2d(ctx, L.small.p, M.data(), (uint64_t)mb * nu * sizeof(double)));
    hipLaunchKernelGGL(k_pca_small_product, dim3(cr_grid(n * nu, PCA_WG)), dim3(PCA_WG), 0, ctx->stream, L.V.as<double>(), n, n, mb, L.small.as<double>(), nu,
                       L.tmp.as<double>());
    CR_HIP(ctx, hipGetLastError());
    std::vector<double> vcm(n * nu);
    CR_TRY(crgpu_memcpy_d2h(ctx, vcm.data(), L.tmp.p, n * nu * sizeof(double)));
    v.resize(n * nu), d.assign(S.begin(), S.begin() + nu);
    for (uint64_t g = 0; g < n; g++)
        for (uint32_t c = 0; c < nu; c++) v[g * nu + c] = vcm[(size_t)c * n + g];
    *it_out = it, *mprod_out = mprod;
    return CRGPU_OK;
}

// ---- the entry point ------------------------------------------------------------------------------------------------------------------------
extern "C" int crgpu_pca_dev(crgpu_ctx *ctx, const crgpu_matrix_dev *m, uint32_t n_features, const crgpu_pca_args *a, crgpu_pca_result *res) {
    if (!ctx || !m || !a || !res) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    // every refusal below comes before the device is touched
    const uint64_t V = m->n_barcodes;
    const uint32_t G = n_features;
    CR_REQUIRE(ctx, a->n_components >= 1 && a->n_components <= CRGPU_PCA_MAX_COMPONENTS, CRGPU_EINVAL, "crgpu_pca_dev: %u components, 1 to %u", a->n_components,
               CRGPU_PCA_MAX_COMPONENTS);
    CR_REQUIRE(ctx, G >= 2 && G < (1u << 31), CRGPU_EINVAL, "crgpu_pca_dev: %u features, 2 to 2^31 - 1", G);
    CR_REQUIRE(ctx, V >= 2 && V < (1ull << 31), CRGPU_EINVAL, "crgpu_pca_dev: %llu barcodes, 2 to 2^31 - 1", (unsigned long long)V);
    CR_REQUIRE(ctx, (a->pca_bc_indices != nullptr) == (a->n_pca_bcs != 0), CRGPU_EINVAL, "crgpu_pca_dev: pca_bc_indices and n_pca_bcs go together");
    CR_REQUIRE(ctx, (a->start != nullptr) == (a->n_start != 0), CRGPU_EINVAL, "crgpu_pca_dev: start and n_start go together");
    const uint32_t wg = a->wave_block ? a->wave_block : PCA_WG;
    CR_REQUIRE(ctx, wg == 64u || wg == 128u || wg == 256u, CRGPU_EINVAL, "crgpu_pca_dev: wave_block %u, 64, 128 or 256", wg);
    const uint32_t ppb = a->dot_parts_per_block ? a->dot_parts_per_block : 1u;
    CR_REQUIRE(ctx, ppb <= 64u && a->reserved0 == 0u && a->reserved1 == 0u, CRGPU_EINVAL, "crgpu_pca_dev: dot_parts_per_block %u (up to 64), reserved 0", ppb);
    for (uint64_t i = 0; i < a->n_start; i++)
        CR_REQUIRE(ctx, std::isfinite(a->start[i]), CRGPU_EINVAL, "crgpu_pca_dev: start[%llu] is not finite", (unsigned long long)i);
    for (uint64_t i = 1; i < a->n_pca_bcs; i++)
        CR_REQUIRE(ctx, a->pca_bc_indices[i - 1] < a->pca_bc_indices[i], CRGPU_EINVAL, "crgpu_pca_dev: pca_bc_indices must be strictly ascending");

    const auto t0 = std::chrono::steady_clock::now();
    res->status = CRGPU_PCA_OK, res->n_components = 0, res->n_used_features = 0, res->n_thresholded_features = 0, res->it = 0, res->mprod = 0, res->m_b = 0;
    res->reserved = 0, res->n_thresholded_barcodes = 0, res->n_pca_barcodes = 0;
    res->fit_ms = res->prepare_ms = res->lanczos_ms = res->project_ms = 0.0;
    const uint32_t thr = a->min_count_threshold;

    // thresholding: the barcodes first, then the features of what is left (select_axes_above_threshold)
    DevBuf sums_b, tb_b, fc_b;
    CR_TRY(dmalloc(ctx, sums_b, V * sizeof(uint32_t)));
    CR_TRY(crgpu_matrix_dev_column_sums(ctx, m, nullptr, 0, sums_b.as<uint32_t>()));
    std::vector<uint32_t> sums(V), T_b;
    CR_TRY(crgpu_memcpy_d2h(ctx, sums.data(), sums_b.p, V * sizeof(uint32_t)));
    for (uint64_t c = 0; c < V; c++)
        if (sums[c] > thr) T_b.push_back((uint32_t)c);
    res->n_thresholded_barcodes = T_b.size();
    if (T_b.empty()) {
        res->status = CRGPU_PCA_NULL_AXIS;
        return CRGPU_OK;
    }
    CR_TRY(dmalloc(ctx, tb_b, T_b.size() * sizeof(uint32_t)));
    CR_TRY(dmalloc(ctx, fc_b, (uint64_t)G * sizeof(uint64_t)));
    CR_TRY(crgpu_memcpy_h2d(ctx, tb_b.p, T_b.data(), T_b.size() * sizeof(uint32_t)));
    CR_HIP(ctx, hipMemsetAsync(fc_b.p, 0, (uint64_t)G * sizeof(uint64_t), ctx->stream));
    hipLaunchKernelGGL(k_pca_feature_counts, dim3(pca_wave_grid(T_b.size(), wg)), dim3(wg), 0, ctx->stream, (const long long *)m->d_indptr, m->d_indices, m->d_data,
                       tb_b.as<uint32_t>(), (uint64_t)T_b.size(), G, fc_b.as<unsigned long long>());
    CR_HIP(ctx, hipGetLastError());
    std::vector<uint64_t> fcount(G);
    CR_TRY(crgpu_memcpy_d2h(ctx, fcount.data(), fc_b.p, (uint64_t)G * sizeof(uint64_t)));
    std::vector<uint32_t> T_f;
    std::vector<int32_t> fmap(G, -1);
    std::vector<uint8_t> mask(G, 0);
    for (uint32_t f = 0; f < G; f++)
        if (fcount[f] > thr) fmap[f] = (int32_t)T_f.size(), mask[f] = 1, T_f.push_back(f);
    res->n_thresholded_features = (uint32_t)T_f.size();
    if (T_f.empty()) {
        res->status = CRGPU_PCA_NULL_AXIS;
        return CRGPU_OK;
    }
    const uint64_t n_tb = T_b.size();
    const uint32_t n_tf = (uint32_t)T_f.size();
    for (uint64_t i = 0; i < a->n_pca_bcs; i++)
        CR_REQUIRE(ctx, a->pca_bc_indices[i] < n_tb, CRGPU_EINVAL, "crgpu_pca_dev: pca_bc_indices[%llu] = %llu of %llu thresholded barcodes", (unsigned long long)i,
                   (unsigned long long)a->pca_bc_indices[i], (unsigned long long)n_tb);
    const uint64_t n_pb = a->n_pca_bcs ? a->n_pca_bcs : n_tb;
    const uint32_t n_pf = a->pca_features == 0u || a->pca_features > n_tf ? n_tf : a->pca_features;
    res->n_pca_barcodes = n_pb;
    uint32_t nu = a->n_components;
    const uint64_t rank = std::min<uint64_t>(n_pf, n_pb);
    if (rank < nu) {
        if (thr == CRGPU_PCA_DEFAULT_THRESHOLD) {  // the stage retries without a threshold
            res->status = CRGPU_PCA_RANK_TOO_SMALL;
            return CRGPU_OK;
        }
        nu = (uint32_t)rank;
    }
    CR_REQUIRE(ctx, n_pf >= 2 && n_pb >= 2, CRGPU_EINVAL, "crgpu_pca_dev: the PCA matrix is %llu x %u, at least 2 x 2", (unsigned long long)n_pb, n_pf);
    CR_REQUIRE(ctx, !a->start || a->n_start == n_pf, CRGPU_EINVAL, "crgpu_pca_dev: %llu start values for %u used features", (unsigned long long)a->n_start, n_pf);

    // the dispersion of the thresholded matrix (unlogged) and the order of the features
    DevBuf fmap_b, msum_b;
    CR_TRY(dmalloc(ctx, fmap_b, (uint64_t)G * sizeof(int32_t)));
    CR_TRY(dmalloc(ctx, msum_b, V * sizeof(uint32_t)));
    std::vector<double> dispersion(n_tf);
    {
        PcaPrep T;
        CR_TRY(crgpu_memcpy_h2d(ctx, fmap_b.p, fmap.data(), (uint64_t)G * sizeof(int32_t)));
        CR_TRY(crgpu_matrix_dev_column_sums(ctx, m, mask.data(), G, msum_b.as<uint32_t>()));
        CR_TRY(pca_prepare(ctx, m, G, tb_b.as<uint32_t>(), n_tb, fmap_b.as<int32_t>(), n_tf, msum_b.as<uint32_t>(), false, wg, T));
        CR_TRY(crgpu_normalized_dispersion(T.mean.data(), T.var.data(), n_tf, PCA_NBINS, dispersion.data()));
    }
    const std::vector<uint32_t> order = pca_feature_order(dispersion, n_pf);  // positions among the thresholded features
    std::vector<uint32_t> cols(n_pf);                                         // org_cols_used
    std::fill(fmap.begin(), fmap.end(), -1);
    std::fill(mask.begin(), mask.end(), 0);
    for (uint32_t g = 0; g < n_pf; g++) cols[g] = T_f[order[g]], fmap[cols[g]] = (int32_t)g, mask[cols[g]] = 1;
    if (res->dispersion_out) {
        for (uint32_t f = 0; f < G; f++) res->dispersion_out[f] = std::nan("");
        for (uint32_t t = 0; t < n_tf; t++) res->dispersion_out[T_f[t]] = dispersion[t];
    }
    if (res->features_selected_out) std::copy(cols.begin(), cols.end(), res->features_selected_out);
    res->n_used_features = n_pf, res->n_components = nu;

    // the PCA matrix: logged, centred and scaled
    std::vector<double> d, v;
    {
        PcaPrep P;
        std::vector<uint32_t> P_b(n_pb);
        for (uint64_t i = 0; i < n_pb; i++) P_b[i] = T_b[a->n_pca_bcs ? a->pca_bc_indices[i] : i];
        DevBuf pb_b, inv_b;
        CR_TRY(dmalloc(ctx, pb_b, n_pb * sizeof(uint32_t)));
        CR_TRY(dmalloc(ctx, inv_b, (uint64_t)n_pf * sizeof(double)));
        CR_TRY(crgpu_memcpy_h2d(ctx, pb_b.p, P_b.data(), n_pb * sizeof(uint32_t)));
        CR_TRY(crgpu_memcpy_h2d(ctx, fmap_b.p, fmap.data(), (uint64_t)G * sizeof(int32_t)));
        CR_TRY(crgpu_matrix_dev_column_sums(ctx, m, mask.data(), G, msum_b.as<uint32_t>()));
        CR_TRY(pca_prepare(ctx, m, G, pb_b.as<uint32_t>(), n_pb, fmap_b.as<int32_t>(), n_pf, msum_b.as<uint32_t>(), true, wg, P));
        std::vector<double> inv(n_pf), center(n_pf), start(n_pf);
        for (uint32_t g = 0; g < n_pf; g++) {
            const double sc = std::sqrt(P.var[g] == 0.0 ? 1.0 : P.var[g]);
            inv[g] = 1.0 / sc, center[g] = P.mean[g] / sc;
        }
        CR_TRY(crgpu_memcpy_h2d(ctx, inv_b.p, inv.data(), (uint64_t)n_pf * sizeof(double)));
        CR_TRY(pca_scale(ctx, P, inv_b.as<double>()));
        if (a->start) std::copy(a->start, a->start + n_pf, start.begin());
        else CR_TRY(crgpu_legacy_randn(a->seed, n_pf, start.data()));
        CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        res->prepare_ms = cr_ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        CR_TRY(pca_irlb(ctx, P, center, start, nu, wg, ppb, d, v, &res->it, &res->mprod, &res->m_b));
        res->lanczos_ms = cr_ms_since(t1);
    }
    if (res->d_out) std::copy(d.begin(), d.end(), res->d_out);
    if (res->variance_explained_out)
        for (uint32_t c = 0; c < nu; c++) res->variance_explained_out[c] = d[c] * d[c] / ((double)(n_pb - 1u) * (double)n_pf);
    if (res->components_out) {
        std::fill(res->components_out, res->components_out + (size_t)nu * G, 0.0);
        for (uint32_t g = 0; g < n_pf; g++)
            for (uint32_t c = 0; c < nu; c++) res->components_out[(size_t)c * G + cols[g]] = v[(size_t)g * nu + c];
    }

    // the projection of every barcode of the full matrix, with the full matrix's own median, centre and scale
    if (res->transformed_out) {
        const auto t2 = std::chrono::steady_clock::now();
        PcaPrep Fm;
        CR_TRY(pca_prepare(ctx, m, G, nullptr, V, nullptr, G, sums_b.as<uint32_t>(), true, wg, Fm));
        std::vector<double> inv(G), cv(nu, 0.0);
        for (uint32_t f = 0; f < G; f++) inv[f] = 1.0 / std::sqrt(Fm.var[f] == 0.0 ? 1.0 : Fm.var[f]);
        for (uint32_t g = 0; g < n_pf; g++) {
            const uint32_t f = cols[g];
            const double cs = Fm.mean[f] / std::sqrt(Fm.var[f] == 0.0 ? 1.0 : Fm.var[f]);  // (full_center / full_scale)[cols]
            for (uint32_t c = 0; c < nu; c++) cv[c] += cs * v[(size_t)g * nu + c];
        }
        DevBuf inv_b, v_b, cv_b, out_b;
        CR_TRY(dmalloc(ctx, inv_b, (uint64_t)G * sizeof(double)));
        CR_TRY(dmalloc(ctx, v_b, (uint64_t)n_pf * nu * sizeof(double)));
        CR_TRY(dmalloc(ctx, cv_b, nu * sizeof(double)));
        CR_TRY(dmalloc(ctx, out_b, V * nu * sizeof(double)));
        CR_TRY(crgpu_memcpy_h2d(ctx, inv_b.p, inv.data(), (uint64_t)G * sizeof(double)));
        CR_TRY(crgpu_memcpy_h2d(ctx, v_b.p, v.data(), (uint64_t)n_pf * nu * sizeof(double)));
        CR_TRY(crgpu_memcpy_h2d(ctx, cv_b.p, cv.data(), nu * sizeof(double)));
        CR_TRY(crgpu_memcpy_h2d(ctx, fmap_b.p, fmap.data(), (uint64_t)G * sizeof(int32_t)));
        if (Fm.nnz) {
            hipLaunchKernelGGL(k_pca_scale, dim3(cr_grid(Fm.nnz, PCA_WG)), dim3(PCA_WG), 0, ctx->stream, Fm.val.as<double>(), Fm.col.as<uint32_t>(), Fm.nnz,
                               inv_b.as<double>());
            CR_HIP(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(k_pca_project, dim3(pca_wave_grid(V, wg)), dim3(wg), 0, ctx->stream, Fm.rowptr.as<uint64_t>(), Fm.col.as<uint32_t>(), Fm.val.as<double>(), V,
                           fmap_b.as<int32_t>(), v_b.as<double>(), nu, cv_b.as<double>(), out_b.as<double>());
        CR_HIP(ctx, hipGetLastError());
        CR_TRY(crgpu_memcpy_d2h(ctx, res->transformed_out, out_b.p, V * nu * sizeof(double)));
        res->project_ms = cr_ms_since(t2);
    }
    res->fit_ms = cr_ms_since(t0);
    return CRGPU_OK;
}
