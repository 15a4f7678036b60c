"""Thin Python host over the C ABI (include/crgpu.h): device buffers + one method per entry point.

The product path: every method ends in a libcrgpu call; there is no CPU implementation behind
any of them (a missing library / GPU raises CrgpuError).
"""
import collections
import csv
import ctypes as C
import io
import math
import os
import time

import numpy as np

from . import _lib
from ._lib import (COUNTS_CORRECTED, COUNTS_PRIOR, COUNTS_VALID, MISS, NO_FEATURE, CrgpuError, MatrixView,
                   Records, SynthOut, SynthParams, ptr)

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def pack_seqs(seqs, length=None):
    """list of str/bytes or (n, len) uint8 ASCII array -> (packed uint32[n], len).  ACGT only."""
    a = ascii_matrix(seqs, length)
    n, L = a.shape
    if L > 16:
        raise ValueError("sequences longer than 16 bases do not fit 32 bits")
    code = np.full(256, 255, dtype=np.uint8)
    code[_ACGT] = np.arange(4, dtype=np.uint8)
    c = code[a]
    if (c == 255).any():
        raise ValueError("non-ACGT base")
    out = np.zeros(n, dtype=np.uint32)
    for j in range(L):
        out = (out << np.uint32(2)) | c[:, j].astype(np.uint32)
    return out, L


def unpack_seqs(packed, length):
    packed = np.asarray(packed, dtype=np.uint32)
    out = np.zeros((len(packed), length), dtype=np.uint8)
    for j in range(length):
        out[:, j] = _ACGT[(packed >> np.uint32(2 * (length - 1 - j))) & np.uint32(3)]
    return out


def compute_feature_dist(counts, feature_types=None):
    """compute_feature_dist (feature_checker.rs:8-50) through the C ABI (host code)"""
    c = np.ascontiguousarray(counts, dtype=np.int64)
    t = None if feature_types is None else np.ascontiguousarray(feature_types, dtype=np.uint32)
    out = np.zeros(len(c), np.float64)
    rc = _lib.load().crgpu_compute_feature_dist(ptr(c), ptr(t), len(c), ptr(out))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_compute_feature_dist")
    return out


def synth_rows_host(seed, first, n, feature, feat_seq, L, offset, row_stride, err=0.005, n_rate=0.0005):
    """host twin of Context.synth_rows: (seq rows, qual rows) uint8 (n, row_stride)"""
    fs = np.ascontiguousarray(feat_seq, dtype=np.uint64)
    ft = None if feature is None else np.ascontiguousarray(feature, dtype=np.uint32)
    s, q = np.zeros((n, row_stride), np.uint8), np.zeros((n, row_stride), np.uint8)
    rc = _lib.load().crgpu_synth_rows_host(seed, first, n, ptr(ft), ptr(fs), len(fs), L, offset, row_stride,
                                           int(round(err * 65536)), int(round(n_rate * (1 << 20))), ptr(s), ptr(q))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_synth_rows_host")
    return s, q


def compile_feature_pattern(pattern, length):
    """compile_pattern (feature_extraction.rs:307-343): the regular expression as text, None for a rejected pattern"""
    buf = C.create_string_buffer(4096)
    rc = _lib.load().crgpu_compile_feature_pattern(pattern.encode(), length, buf, 4096)
    return buf.value.decode() if rc == 0 else None


def ascii_matrix(seqs, length=None):
    if isinstance(seqs, np.ndarray) and seqs.dtype == np.uint8 and seqs.ndim == 2:
        return np.ascontiguousarray(seqs)
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    if length is None:
        length = len(bs[0]) if bs else 0
    if any(len(b) != length for b in bs):
        raise ValueError("sequences must all have length %d" % length)
    return np.frombuffer(b"".join(bs), dtype=np.uint8).reshape(len(bs), length).copy()


class DeviceArray:
    """A device allocation owned through crgpu_malloc/crgpu_free (or adopted from a library call that returns a
    library-owned buffer to be released with crgpu_free: `adopt`)."""

    def __init__(self, ctx, shape, dtype, adopt=None):
        self.ctx = ctx
        self.shape = (shape,) if np.isscalar(shape) else tuple(shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        if adopt is not None:
            self.ptr = int(adopt)
            return
        p = C.c_void_p()
        ctx._check(ctx.L.crgpu_malloc(ctx.h, C.byref(p), max(self.nbytes, 1)))
        self.ptr = p.value

    @property
    def size(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def to_host(self, count=None):
        n = self.size if count is None else int(count)
        out = np.empty(n, dtype=self.dtype)
        if n:
            self.ctx._check(self.ctx.L.crgpu_memcpy_d2h(self.ctx.h, ptr(out), self.ptr, n * self.dtype.itemsize))
        if count is None:
            out = out.reshape(self.shape)
        return out

    def upload(self, arr):
        a = np.ascontiguousarray(arr, dtype=self.dtype)
        assert a.nbytes <= self.nbytes
        if a.nbytes:
            self.ctx._check(self.ctx.L.crgpu_memcpy_h2d(self.ctx.h, self.ptr, ptr(a), a.nbytes))
        return self

    def zero(self):
        self.ctx._check(self.ctx.L.crgpu_memset(self.ctx.h, self.ptr, 0, self.nbytes))
        return self

    def free(self):
        if self.ptr is not None and self.ctx.h:
            self.ctx.L.crgpu_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    @property
    def __cuda_array_interface__(self):
        # lets torch.as_tensor(..., device="cuda") alias the buffer for collectives
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (self.ptr, False), "version": 2}


def _p(x):
    if x is None:
        return None
    if isinstance(x, DeviceArray):
        return C.c_void_p(x.ptr)
    if hasattr(x, "data_ptr"):  # torch tensor
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


class Matrix:
    """Host view of crgpu_matrix (the arrays write_matrix_h5 stores; count_matrix.rs:382-448)."""

    def __init__(self, ctx, mv_ptr):
        self.ctx, self._mv = ctx, mv_ptr
        m = mv_ptr.contents
        self.n_barcodes, self.nnz = int(m.n_barcodes), int(m.nnz)
        self.n_features, self.cb_len = int(m.n_features), int(m.cb_len)

        def arr(p, dtype, n):
            if n == 0:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(p), dtype=dtype).copy()

        self.barcode_rank = arr(m.barcode_rank, np.uint32, self.n_barcodes)
        self.barcode_seq = arr(m.barcode_seq, np.uint32, self.n_barcodes)
        self.indptr = arr(m.indptr, np.int64, self.n_barcodes + 1)
        self.indices = arr(m.indices, np.int32, self.nnz)
        self.data = arr(m.data, np.int32, self.nnz)
        self.gem_group = arr(m.gem_group, np.uint16, self.n_barcodes) if m.gem_group else None
        # barcodes longer than 16 bases (segmented constructs): barcode_seq = the first 16 bases, barcode_seq_hi = the rest
        self.barcode_seq_hi = arr(m.barcode_seq_hi, np.uint32, self.n_barcodes) if m.barcode_seq_hi else None

    def barcodes_ascii(self):
        if self.barcode_seq_hi is None:
            return unpack_seqs(self.barcode_seq, self.cb_len)
        return np.concatenate([unpack_seqs(self.barcode_seq, 16), unpack_seqs(self.barcode_seq_hi, self.cb_len - 16)], axis=1)

    def write_mtx(self, mtx_path, barcodes_path=None, metadata_line='%metadata_json: {"format_version": 2}',
                  gem_group=1):
        self.ctx._check(self.ctx.L.crgpu_write_mtx(self.ctx.h, self._mv, metadata_line.encode(),
                                                   None if mtx_path is None else str(mtx_path).encode(),
                                                   None if barcodes_path is None else str(barcodes_path).encode(),
                                                   gem_group))

    def free(self):
        if self._mv is not None and self.ctx.h:
            self.ctx.L.crgpu_matrix_free(self.ctx.h, self._mv)
        self._mv = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class MatrixDev:
    """crgpu_matrix_dev: device-resident CSC (barcode_rank, indptr, indices, data)."""

    def __init__(self, ctx, mv_ptr):
        self.ctx, self._mv = ctx, mv_ptr
        self.n_barcodes, self.nnz = int(mv_ptr.contents.n_barcodes), int(mv_ptr.contents.nnz)

    def download(self):
        V, nnz = self.n_barcodes, self.nnz
        rank, indptr = np.zeros(V, np.uint32), np.zeros(V + 1, np.int64)
        indices, data = np.zeros(nnz, np.int32), np.zeros(nnz, np.int32)
        self.ctx._check(self.ctx.L.crgpu_matrix_dev_download(self.ctx.h, self._mv, ptr(rank), ptr(indptr), ptr(indices), ptr(data)))
        return rank, indptr, indices, data

    def free(self):
        if self._mv is not None and self.ctx.h:
            self.ctx.L.crgpu_matrix_dev_free(self.ctx.h, self._mv)
        self._mv = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SseqParams:
    """crgpu_sseq_params: the sSeq parameters of one matrix, resident on the device (Context.sseq_params)"""

    def __init__(self, ctx, h, n_cells, n_features):
        self.ctx, self._h, self.n_cells, self.n_features = ctx, h, n_cells, n_features

    def download(self):
        """-> dict(size_factors f64[N], mean_g, var_g, phi_mm_g, phi_g f64[G], use_g bool[G], zeta_hat, delta, n_used)"""
        N, G = self.n_cells, self.n_features
        o = dict(size_factors=np.zeros(N), mean_g=np.zeros(G), var_g=np.zeros(G), phi_mm_g=np.zeros(G), phi_g=np.zeros(G))
        use = np.zeros(G, np.uint8)
        info = _lib.SseqParamsInfo(size_factors_out=ptr(o["size_factors"]), mean_out=ptr(o["mean_g"]), var_out=ptr(o["var_g"]),
                                   phi_mm_out=ptr(o["phi_mm_g"]), phi_out=ptr(o["phi_g"]), use_out=ptr(use))
        self.ctx._check(self.ctx.L.crgpu_sseq_params_get(self.ctx.h, self._h, C.byref(info)))
        o.update(use_g=use != 0, zeta_hat=info.zeta_hat, delta=info.delta, n_used=int(info.n_used))
        return o

    def free(self):
        if self._h is not None and self.ctx.h:
            self.ctx.L.crgpu_sseq_params_free(self.ctx.h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SseqPairs:
    """crgpu_sseq_pairs: one matrix and one grouping of its cells, transposed once for every local sSeq test of two sets of groups
    (Context.sseq_pairs; csrc/sseq_pair.h)"""

    VECTORS = (("use", np.uint8), ("mean", np.float64), ("phi_mm", np.float64), ("phi", np.float64), ("sums_a", np.uint64), ("sums_b", np.uint64),
               ("norm_mean_a", np.float64), ("norm_mean_b", np.float64), ("log2_fold_change", np.float64), ("p_values", np.float64),
               ("adjusted_p_values", np.float64), ("below_median", np.uint8))

    def __init__(self, ctx, h, n_groups, n_features):
        self.ctx, self._h, self.n_groups, self.n_features = ctx, h, n_groups, n_features

    def compare(self, groups_a, groups_b, de_threshold=0.0, wave_min=0, wg_min=0, vectors=True):
        """crgpu_sseq_pair_dev: the cells of groups_a against those of groups_b (ascending, distinct, disjoint lists of group ids), the
        sSeq parameters computed on these cells alone -> dict(zeta_hat, delta, n_used, s_a, s_b, n_cells_a, n_cells_b, n_exact,
        n_asymptotic, n_terms, n_de = genes with adjusted p < de_threshold (0 = 0.05), ms_*) and, with vectors, per gene use, mean, phi_mm,
        phi, sums_a, sums_b, norm_mean_a, norm_mean_b, log2_fold_change, p_values, adjusted_p_values, below_median.  Every value equals
        bit for bit cluster 1 of Context.sseq_params + Context.sseq_diffexp on the sub-matrix of the pair's cells in (group, cell) order"""
        ga, gb = np.ascontiguousarray(groups_a, dtype=np.uint32).reshape(-1), np.ascontiguousarray(groups_b, dtype=np.uint32).reshape(-1)
        G = self.n_features
        o = {k: np.zeros(G, t) for k, t in self.VECTORS} if vectors else {}
        r = _lib.SseqPairResult(**{k + "_out": ptr(v) for k, v in o.items()})
        a = _lib.SseqPairArgs(n_features=G, wave_min=int(wave_min), wg_min=int(wg_min), de_threshold=float(de_threshold))
        self.ctx._check(self.ctx.L.crgpu_sseq_pair_dev(self.ctx.h, self._h, ptr(ga), len(ga), ptr(gb), len(gb), C.byref(a), C.byref(r)))
        o.update(zeta_hat=r.zeta_hat, delta=r.delta, s_a=r.s_a, s_b=r.s_b, n_cells_a=int(r.n_cells_a), n_cells_b=int(r.n_cells_b), n_exact=int(r.n_exact),
                 n_asymptotic=int(r.n_asymptotic), n_terms=int(r.n_terms), n_de=int(r.n_de), n_used=int(r.n_used), n_runs=int(r.n_runs),
                 ms_median=r.ms_median, ms_sums=r.ms_sums, ms_exact=r.ms_exact, ms_asymptotic=r.ms_asymptotic, ms_bh=r.ms_bh)
        return o

    def bootstrap(self, items, n_bootstraps=500, seed=0, lds_cells=0, draws_per_wg=0):
        """crgpu_sseq_pair_bootstrap_dev: items = rows of (gene, group_a, group_b, stream) -> (sums_a, sums_b) u64[n_items, B]: the sum of the
        gene over draw b's resample (with replacement) of the cells of group_a / of group_b, each side one group of the plan.  The
        stream is Philox keyed (seed, 0), numbered by the item's `stream`, the side and the draw (include/crgpu.h); the reference's
        unseeded np.random stream is not reproduced.  lds_cells and draws_per_wg change no value"""
        it = np.ascontiguousarray(items, dtype=np.uint32).reshape(-1, 4)
        B = int(n_bootstraps) if n_bootstraps else 500
        sa, sb = np.zeros((len(it), B), np.uint64), np.zeros((len(it), B), np.uint64)
        a = _lib.PbArgs(n_bootstraps=int(n_bootstraps), lds_cells=int(lds_cells), draws_per_wg=int(draws_per_wg), seed=int(seed))
        self.ctx._check(self.ctx.L.crgpu_sseq_pair_bootstrap_dev(self.ctx.h, self._h, ptr(it), len(it), C.byref(a), ptr(sa), ptr(sb)))
        return sa, sb

    def free(self):
        if self._h is not None and self.ctx.h:
            self.ctx.L.crgpu_sseq_pairs_free(self.ctx.h, self._h)
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class CellCall:
    """Result of Context.call_cells_ordmag: `cols` = the called columns (DeviceArray of u64, ascending positions in the count
    vector / the matrix the counts came from), `n_cells`, `metrics` = crgpu_ordmag_result as a dict (BarcodeFilterResults of
    cell_calling_helpers.py:832-955 plus the bootstrap's per-sample values)."""

    def __init__(self, ctx, cols, n_cells, res, matrix=None):
        self.ctx, self.cols, self.n_cells, self._matrix = ctx, cols, n_cells, matrix
        if isinstance(res, dict):  # a merged call (Context.call_additional_cells) keeps the metrics of the initial one
            self.metrics = dict(res)
            return
        m = {}
        for name, _ in _lib.OrdmagResult._fields_:
            v = getattr(res, name)
            m[name] = np.array(v[:]) if hasattr(v, "__len__") else v
        m["filtered_bcs_cutoff"] = m["filtered_bcs_cutoff"] if m.pop("filtered_bcs_cutoff_set") else None
        m["estimated"] = bool(m["estimated"])
        self.metrics = m

    def cols_host(self):
        return self.cols.to_host(self.n_cells)

    def ranks_dev(self, m=None):
        """canonical ranks of the called cells (DeviceArray of u32, strictly ascending): what Counts.probe_metrics and
        Counts.probe_matrix take; `m` = the MatrixDev whose columns were counted (default: the one the call was made on)"""
        m = m or self._matrix
        if m is None:
            raise ValueError("the call was made on a bare count vector: pass the MatrixDev its columns belong to")
        out = self.ctx.empty(self.n_cells, np.uint32)
        self.ctx._check(self.ctx.L.crgpu_cell_ranks_dev(self.ctx.h, m._mv, _p(self.cols), self.n_cells, _p(out)))
        return out

    @property
    def ranks(self):
        return self.ranks_dev().to_host(self.n_cells)

    def filtered_matrix(self, m=None):
        """the filtered feature-barcode matrix: the called columns of `m` (MatrixDev), selected on the device"""
        m = m or self._matrix
        if m is None:
            raise ValueError("the call was made on a bare count vector: pass the MatrixDev to filter")
        mv = C.POINTER(_lib.MatrixDevView)()
        self.ctx._check(self.ctx.L.crgpu_select_barcodes_cols_dev(self.ctx.h, m._mv, _p(self.cols), self.n_cells, C.byref(mv)))
        return MatrixDev(self.ctx, mv)


class AdditionalCells:
    """Result of Context.call_additional_cells (find_nonambient_barcodes, cell_calling.py:144-263).  Per candidate, in
    ascending column order (the rows of nonambient_summary): eval_cols, umis, obs_loglk, n_lower, pvalues, pvalues_adj,
    is_nonambient (numpy).  `status` = 0 or which `return None` of the reference was taken (status_text), `metrics` =
    crgpu_emptydrops_result as a dict, `call` = the merged CellCall (initial cells + non-ambient candidates), whose
    .filtered_matrix() and .ranks work as after the initial call.  profile_p / eval_features and sim_n / sim_loglk are set
    when they were asked for."""

    def __init__(self, ctx, res, arr, initial, matrix):
        self.metrics = {name: getattr(res, name) for name, _ in _lib.EmptydropsResult._fields_}
        self.status = int(res.status)
        self.status_text = _lib.ED_STATUS[self.status]
        n = int(arr.n_candidates)

        def take(name, dtype, count):
            p = getattr(arr, name)
            if not (p and count):
                return np.zeros(0, dtype)  # (an unused allocation goes with crgpu_emptydrops_arrays_free below)
            setattr(arr, name, None)  # adopted: released with the DeviceArray
            return DeviceArray(ctx, count, dtype, adopt=p).to_host(count)

        self.eval_cols = take("d_eval_cols", np.uint64, n)
        self.umis = take("d_umis", np.uint32, n)
        self.obs_loglk = take("d_obs_loglk", np.float64, n)
        self.n_lower = take("d_n_lower", np.uint32, n)
        self.pvalues = take("d_pvalues", np.float64, n)
        self.pvalues_adj = take("d_pvalues_adj", np.float64, n)
        self.is_nonambient = take("d_is_nonambient", np.uint8, n).astype(bool)
        nf, nd, ns = int(arr.n_eval_features), int(arr.n_distinct_n), int(arr.num_sims)
        self.eval_features = take("d_eval_features", np.uint32, nf) if arr.d_eval_features else None
        self.profile_p = take("d_profile_p", np.float64, nf) if arr.d_profile_p else None
        self.sim_n = take("d_sim_n", np.int64, nd) if arr.d_sim_n else None
        self.sim_loglk = take("d_sim_loglk", np.float64, nd * ns).reshape(nd, ns) if arr.d_sim_loglk else None
        cols, n_called = arr.d_called_cols, int(arr.n_called)
        arr.d_called_cols = None
        d_cols = DeviceArray(ctx, n_called, np.uint64, adopt=cols) if cols else ctx.empty(0, np.uint64)
        self.call = CellCall(ctx, d_cols, n_called, initial.metrics, matrix)
        ctx.L.crgpu_emptydrops_arrays_free(ctx.h, C.byref(arr))  # whatever was not taken


def sgt_proportions(freq):
    """sgt_proportions (sgt.py:97-132) on the host through the C ABI: non-zero item frequencies -> (pstar, p0, slope, status);
    status 0, or _lib.SGT_TOO_FEW / _lib.SGT_SLOPE for the reference's two SimpleGoodTuringError cases (pstar is then None)"""
    f = np.ascontiguousarray(freq, dtype=np.uint64)
    pstar, p0, slope = np.zeros(len(f), np.float64), C.c_double(np.nan), C.c_double(np.nan)
    rc = _lib.load().crgpu_sgt_proportions(ptr(f), len(f), ptr(pstar), C.byref(p0), C.byref(slope))
    if rc < 0:
        raise _lib.CrgpuError(rc, "crgpu_sgt_proportions")
    return (pstar if rc == 0 else None), p0.value, slope.value, rc


class Multigenome:
    """Result of Context.multigenome (MultiGenomeAnalysis.run_all, analysis/multigenome.py:251-335).  `call_dev` = DeviceArray of
    u8 per barcode (_lib.MG_GENOME0 / MG_GENOME1 / MG_MULTIPLET), `call` = its host copy; `boot_counts` int64[B, 3] =
    (Multiplets, genome0, genome1) per bootstrap sample, `boot_thresholds` float64[B, 2], `boot_branch` int32[B]
    (_lib.MG_BRANCH_*), `boot` float64[B] = the inferred multiplets per sample; `obs_thresholds`, `obs_branch`, `observed` =
    (Multiplets, genome0, genome1) of the unresampled input; `purity_sums` (six integers) and `purity` = (genome0, genome1,
    overall); `summary` = the numbers of :287-301 (rate_lb / rate_ub None with one sample); `res` = crgpu_multigenome_result
    as a dict.  From Context.multigenome_from_matrix also `totals`, `top_two`, `count0` / `count1` (DeviceArrays)."""

    def __init__(self, ctx, res, call_dev, boot_counts, boot_thresholds, boot_branch, boot):
        self.ctx, self.call_dev = ctx, call_dev
        self.boot_counts, self.boot_thresholds, self.boot_branch, self.boot = boot_counts, boot_thresholds, boot_branch, boot
        r = self.res = {name: getattr(res, name) for name, _ in _lib.MultigenomeResult._fields_}
        self.n = int(r["n"])
        self.call = call_dev.to_host(self.n) if self.n else np.zeros(0, np.uint8)
        self.obs_thresholds, self.obs_branch = (r["obs_thresh0"], r["obs_thresh1"]), int(r["obs_branch"])
        self.observed = (int(r["observed_multiplets"]), int(r["observed_genome0"]), int(r["observed_genome1"]))
        self.purity_sums = tuple(int(r[k]) for k in ("sum_c0_genome0", "sum_all_genome0", "sum_c1_genome1", "sum_all_genome1",
                                                      "sum_max_single", "sum_all_single"))
        self.purity = (r["purity0"], r["purity1"], r["purity_overall"])
        bounds = bool(r["rate_bounds_set"])
        self.summary = dict(observed_all=self.n, observed_multiplets=self.observed[0], mean=r["boot_mean"],
                            inferred_multiplets=int(r["inferred_multiplets"]), rate=r["multiplet_rate"],
                            normalized_rate=r["normalized_multiplet_rate"], rate_lb=r["multiplet_rate_lb"] if bounds else None,
                            rate_ub=r["multiplet_rate_ub"] if bounds else None)
        self.totals = self.top_two = self.count0 = self.count1 = None


def multigenome_summary(boot_counts, n):
    """the host summary of the multiplet bootstrap through the C ABI (crgpu_multigenome_summary, no context): boot_counts
    int64[B, 3] = (Multiplets, genome0, genome1) per sample -> (boot float64[B], dict as Multigenome.summary without the
    observed entries)"""
    bc = np.ascontiguousarray(boot_counts, dtype=np.int64).reshape(-1, 3)
    boot, res = np.zeros(len(bc), np.float64), _lib.MultigenomeResult()
    rc = _lib.load().crgpu_multigenome_summary(ptr(bc), len(bc), int(n), ptr(boot), C.byref(res))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_multigenome_summary")
    bounds = bool(res.rate_bounds_set)
    return boot, dict(mean=res.boot_mean, inferred_multiplets=int(res.inferred_multiplets), rate=res.multiplet_rate,
                      normalized_rate=res.normalized_multiplet_rate, rate_lb=res.multiplet_rate_lb if bounds else None,
                      rate_ub=res.multiplet_rate_ub if bounds else None)


def multigenome_top_two(totals):
    """the two genomes of the analysis (multigenome.py:256-262): sorted(argsort(totals)[::-1][:2]); among equal totals the
    larger index comes first (a stable ascending argsort, reversed)"""
    return sorted(int(i) for i in np.argsort(np.asarray(totals), kind="stable")[::-1][:2])


def write_gem_classification_csv(path, barcodes, count0, count1, call, genome0, genome1):
    """gem_classification.csv of save_gem_class_csv (multigenome.py:356-384): header barcode,<genome0>,<genome1>,call; the call
    written as the genome's name or Multiplet; line terminator os.linesep"""
    names = {_lib.MG_GENOME0: genome0, _lib.MG_GENOME1: genome1, _lib.MG_MULTIPLET: "Multiplet"}
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator=os.linesep)
        w.writerow(["barcode", genome0, genome1, "call"])
        for bc, a, b, c in zip(barcodes, np.asarray(count0).tolist(), np.asarray(count1).tolist(), np.asarray(call).tolist()):
            w.writerow([bc.decode() if isinstance(bc, bytes) else bc, a, b, names[c]])


def multigenome_metrics(result, genome0, genome1):
    """the summary dictionary of run_all (multigenome.py:287-325) from a Multigenome, without the purity-outlier entries"""
    s, d = result.summary, {}
    if result.n == 0:
        return d  # "Don't compute multiplet / purity metrics if no cells detected"
    d["filtered_bcs_observed_all"] = s["observed_all"]
    d["filtered_bcs_observed_multiplets"] = s["observed_multiplets"]
    d["filtered_bcs_inferred_multiplets"] = s["inferred_multiplets"]
    d["filtered_bcs_inferred_multiplet_rate"] = s["rate"]
    d["filtered_bcs_inferred_normalized_multiplet_rate"] = s["normalized_rate"]
    if s["rate_lb"] is not None:
        d["filtered_bcs_inferred_multiplet_rate_lb"] = s["rate_lb"]
        d["filtered_bcs_inferred_multiplet_rate_ub"] = s["rate_ub"]
    d["%s_filtered_bcs_mean_count_purity" % genome0] = result.purity[0]
    d["%s_filtered_bcs_mean_count_purity" % genome1] = result.purity[1]
    d["multi_filtered_bcs_mean_count_purity"] = result.purity[2]
    return d


class RtlTags:
    """Result of Context.rtl_tags: `tags_dev` = DeviceArray of u8, the tag of every column of `matrix` (kept for the later calls),
    `barcodes_per_tag` u64[n_tags] (all columns, empty ones included), `umi_per_tag` u64[n_types, n_tags] or None."""

    def __init__(self, ctx, matrix, tags_dev, n_tags, barcodes_per_tag, umi_per_tag):
        self.ctx, self.matrix, self.tags_dev, self.n_tags = ctx, matrix, tags_dev, n_tags
        self.barcodes_per_tag, self.umi_per_tag = barcodes_per_tag, umi_per_tag

    @property
    def tags(self):
        return self.tags_dev.to_host(self.matrix.n_barcodes)

    def sample_columns(self, sample_of_tag, n_samples, cols=None):
        """the columns of every sample (sample_barcodes; with a cell call: sample_cell_barcodes): sample_of_tag u8[n_tags], 0xFF =
        no sample; cols = None (all columns), a CellCall, or ascending columns (DeviceArray of u64 / numpy) ->
        (DeviceArray of u64: sample 0's columns, then sample 1's, ..., ascending inside each; offsets u64[n_samples + 1])"""
        ctx = self.ctx
        sot = np.ascontiguousarray(sample_of_tag, dtype=np.uint8)
        if len(sot) != self.n_tags:
            raise ValueError("sample_columns: sample_of_tag must have one entry per tag")
        d_cols, n = None, 0
        if cols is not None:
            if isinstance(cols, CellCall):
                d_cols, n = cols.cols, cols.n_cells
            elif isinstance(cols, DeviceArray):
                d_cols, n = cols, cols.size
            else:
                h = np.ascontiguousarray(cols, dtype=np.uint64)
                d_cols, n = ctx.upload(h) if len(h) else ctx.empty(0, np.uint64), len(h)
        out, off = C.c_void_p(), np.zeros(n_samples + 1, np.uint64)
        ctx._check(ctx.L.crgpu_rtl_sample_columns_dev(ctx.h, _p(self.tags_dev), self.matrix.n_barcodes, ptr(sot), self.n_tags, n_samples,
                                                      int(cols is not None), _p(d_cols) if d_cols is not None else None, n, C.byref(out),
                                                      ptr(off)))
        kept = int(off[-1])
        d_out = DeviceArray(ctx, kept, np.uint64, adopt=out.value) if out.value else ctx.empty(0, np.uint64)
        return d_out, off


class RtlGemRuns:
    """Result of Context.rtl_gem_runs (crgpu_rtl_gem_runs): gems_per_tag, cells_per_tag u64[T]; common u64[T, T] (i < j); present
    bool[T]; cells_per_gem_hist u64[n_probe + 1] ([k] = GEMs holding k cells, [0] unused); cells_per_probe and
    first_cell_col_per_probe u64[n_probe] (all ones: the probe rank has no cell); gems_with_cells, n_gems, n_cells."""

    def __init__(self, res):
        T, P = int(res.n_tags), int(res.n_probe)
        self.n_tags, self.n_probe = T, P
        self.gems_per_tag = np.array(res.gems_per_tag[:T], np.uint64)
        self.common = np.array(res.common[:], np.uint64).reshape(64, 64)[:T, :T].copy()
        self.cells_per_tag = np.array(res.cells_per_tag[:T], np.uint64)
        self.present = np.array(res.present[:T], np.uint8) != 0
        self.cells_per_gem_hist = np.array(res.cells_per_gem_hist[:P + 1], np.uint64)
        self.cells_per_probe = np.array(res.cells_per_probe[:P], np.uint64)
        self.first_cell_col_per_probe = np.array(res.first_cell_col_per_probe[:P], np.uint64)
        self.gems_with_cells, self.n_gems, self.n_cells = int(res.gems_with_cells), int(res.n_gems), int(res.n_cells)


def rtl_tag_kind(identifier):
    """categorize_multiplexing_barcode_id (barcode/src/whitelist.rs:181-192) reduced to what CALL_TAGS_RTL asks: RTL_KIND_RTL for
    BC001 .. BC024 and BC...A-D, RTL_KIND_ANTIBODY for BC025 and above and ABnnn, RTL_KIND_OTHER otherwise"""
    head, tail = identifier[:2], identifier[2:]
    num = int(tail) if tail.isdigit() else None
    if head == "BC" and ((num is not None and num <= 24) or (num is None and identifier[-1:] in "ABCD" and identifier[-1:] != "")):
        return _lib.RTL_KIND_RTL
    if (head == "BC" and num is not None) or (head == "AB" and num is not None):
        return _lib.RTL_KIND_ANTIBODY
    return _lib.RTL_KIND_OTHER


def _rtl_rows(arr, n):
    return [dict(tag1=int(r.tag1), tag2=int(r.tag2), gems1=int(r.gems1), gems2=int(r.gems2), common_gems=int(r.common_gems),
                 overlap=float(r.overlap)) for r in arr[:n]]


def rtl_overlap_rows(gems_per_tag, common, present):
    """calculate_frp_gem_barcode_overlap through the C ABI (crgpu_rtl_overlap_rows, no context): one dict per pair i < j of present
    tags in (i, j) order: tag1, tag2, gems1, gems2, common_gems, overlap (NaN for 0 / 0)"""
    g = np.ascontiguousarray(gems_per_tag, dtype=np.uint64)
    T = len(g)
    full = np.zeros((64, 64), np.uint64)
    full[:T, :T] = np.asarray(common, np.uint64).reshape(T, T)
    pr = np.ascontiguousarray(np.asarray(present) != 0, dtype=np.uint8)
    rows, n = (_lib.RtlOverlapRow * max(1, T * (T - 1) // 2))(), C.c_uint32()
    rc = _lib.load().crgpu_rtl_overlap_rows(ptr(g), ptr(full), ptr(pr), T, rows, len(rows), C.byref(n))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_rtl_overlap_rows")
    return _rtl_rows(rows, n.value)


def rtl_ab_thresholds(median, n_nonzero, ab_tag_of_probe, tag_kind):
    """the Antibody thresholds of detect_suspicious_rtl_ab_pairings (crgpu_rtl_ab_thresholds, no context): u64[n_tags],
    round(0.1 * median) half away from zero, UINT64_MAX = the tag is removed"""
    med, nz = np.ascontiguousarray(median, dtype=np.uint64), np.ascontiguousarray(n_nonzero, dtype=np.uint64)
    abt, kind = np.ascontiguousarray(ab_tag_of_probe, dtype=np.uint8), np.ascontiguousarray(tag_kind, dtype=np.uint8)
    out = np.zeros(len(kind), np.uint64)
    rc = _lib.load().crgpu_rtl_ab_thresholds(ptr(med), ptr(nz), ptr(abt), len(abt), ptr(kind), len(kind), ptr(out))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_rtl_ab_thresholds")
    return out


def rtl_suspicious_pairings(rows, tag_kind, paired_with):
    """the filter at the end of detect_suspicious_rtl_ab_pairings (crgpu_rtl_suspicious_pairings, no context): the RTL + Antibody
    rows that are no configured pairing (paired_with[rtl tag] = antibody tag or -1), RTL first, sorted by (tag1, tag2)"""
    kind, pw = np.ascontiguousarray(tag_kind, dtype=np.uint8), np.ascontiguousarray(paired_with, dtype=np.int32)
    arr, out, n = (_lib.RtlOverlapRow * max(1, len(rows)))(), (_lib.RtlOverlapRow * max(1, len(rows)))(), C.c_uint32()
    for k, r in enumerate(rows):
        arr[k] = _lib.RtlOverlapRow(r["tag1"], r["tag2"], r["gems1"], r["gems2"], r["common_gems"], r["overlap"])
    rc = _lib.load().crgpu_rtl_suspicious_pairings(arr, len(rows), ptr(kind), ptr(pw), len(kind), out, C.byref(n))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_rtl_suspicious_pairings")
    return _rtl_rows(out, n.value)


def rtl_occupancy_summary(cells_per_gem_hist, gems_with_cells, cells_per_probe, total_instrument_partitions=115000,
                          recovery_factor=1 / 1.65):
    """the head of remove_bcs_from_high_occupancy_gems (crgpu_rtl_occupancy_summary, no context) from RtlGemRuns' occupancy
    outputs -> dict(histogram={cells: GEMs} with the zero bin, estimated_lambda, total_probe_barcodes)"""
    hist = np.ascontiguousarray(cells_per_gem_hist, dtype=np.uint64)
    cpp = np.ascontiguousarray(cells_per_probe, dtype=np.uint64)
    zero, lam, probes = C.c_uint64(), C.c_double(), C.c_uint32()
    rc = _lib.load().crgpu_rtl_occupancy_summary(ptr(hist), len(cpp), int(gems_with_cells), ptr(cpp), int(total_instrument_partitions),
                                                 float(recovery_factor), C.byref(zero), C.byref(lam), C.byref(probes))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_rtl_occupancy_summary")
    histogram = {k: int(hist[k]) for k in range(1, len(hist)) if hist[k]}
    histogram[0] = int(zero.value)
    return dict(histogram=histogram, estimated_lambda=lam.value, total_probe_barcodes=int(probes.value))


def high_occupancy_gem_threshold(estimated_lambda, cells_per_probe, first_cell_col_per_probe, total_simulated_gems=1000000):
    """_get_high_occupancy_gem_threshold (cell_calling_helpers.py:273-312) with real numpy: the one number of the stage that comes
    from the host, because np.random.poisson consumes a data-dependent number of uniforms per draw and is serial.  The probe
    barcodes' probabilities are ordered by first appearance among the cells (Counter(probe_bcs)): that order decides which
    simulated barcode a uniform selects, so RtlGemRuns reports it."""
    if estimated_lambda == 0:
        return 0
    cpp = np.asarray(cells_per_probe, np.uint64)
    seen = np.flatnonzero(cpp)
    order = seen[np.argsort(np.asarray(first_cell_col_per_probe, np.uint64)[seen], kind="stable")]
    prob = cpp[order].astype(np.int64) / int(cpp.sum())
    np.random.seed(0)
    gems = np.random.poisson(estimated_lambda, total_simulated_gems)
    gems = gems[gems > 0]
    width = int(gems.max())
    sim = np.random.choice(np.arange(len(prob)), size=(len(gems), width), p=prob)
    # distinct barcodes among the first gems[i] of row i: mask the tail, sort the row, count the steps
    sim = np.where(np.arange(width)[None, :] < gems[:, None], sim, -1)
    sim.sort(axis=1)
    distinct = (np.diff(sim, axis=1) != 0).sum(axis=1) + 1 - (sim[:, 0] == -1)
    return int(np.ceil(np.quantile(distinct, 0.999)))


def call_tags_rtl(ctx, m, call, probe_ids, feature_types=None, type_prefixes=None, pairings=None, antibody_type="Antibody Capture"):
    """CALL_TAGS_RTL (call_tags_rtl.rs:143-301) for the raw MatrixDev `m` and the cell call `call` (CellCall).  probe_ids: the
    (translated) identifier of every probe rank, None = not on the whitelist; feature_types: the type name of every feature;
    type_prefixes: {type name: metric prefix or None}; pairings: {RTL identifier: its antibody identifier} of the multi graph.
    -> dict(tag_ids, tags=RtlTags, runs=RtlGemRuns, barcodes_per_tag={id: count}, rows=[dict with barcode1_id ...], metrics)"""
    ids = sorted(set(i for i in probe_ids if i is not None) | set((pairings or {}).values()))
    tag = {i: t for t, i in enumerate(ids)}
    top = np.array([tag[i] if i is not None else _lib.RTL_NONE for i in probe_ids], np.uint8)
    types, ft = [], None
    if feature_types is not None:
        for ty in feature_types:
            if ty not in types:
                types.append(ty)
        ft = np.array([types.index(ty) for ty in feature_types], np.uint8)
    tags = ctx.rtl_tags(m, top, len(ids), ft, len(types))
    runs = ctx.rtl_gem_runs(m, tags, call)
    rows = rtl_overlap_rows(runs.gems_per_tag, runs.common, runs.present)
    if pairings:
        if feature_types is None:
            raise ValueError("call_tags_rtl: pairings need feature_types")
        kind = np.array([rtl_tag_kind(i) for i in ids], np.uint8)
        abt = np.array([tag[pairings.get(i, i)] if i is not None else _lib.RTL_NONE for i in probe_ids], np.uint8)
        sums = ctx.column_sums(m, np.array([ty == antibody_type for ty in feature_types]))
        nz, med = ctx.rtl_medians(sums, call, m)
        low = rtl_ab_thresholds(med, nz, abt, kind)
        both = ctx.rtl_gem_runs(m, tags, call, ab=(abt, sums, low))
        pw = np.full(len(ids), -1, np.int32)
        for a, b in pairings.items():
            if a in tag:
                pw[tag[a]] = tag[b]
        rows = rows + rtl_suspicious_pairings(rtl_overlap_rows(both.gems_per_tag, both.common, both.present), kind, pw)
    out_rows = [dict(barcode1_id=ids[r["tag1"]], barcode2_id=ids[r["tag2"]], barcode1_gems=r["gems1"], barcode2_gems=r["gems2"],
                     common_gems=r["common_gems"], overlap=r["overlap"]) for r in rows]
    metrics = dict(filtered_gel_bead_barcodes_count=runs.gems_with_cells,
                   filtered_barcodes_per_probe_barcode={ids[t]: int(runs.gems_per_tag[t]) for t in range(len(ids)) if runs.present[t]},
                   probe_barcode_overlap_coefficients={"%s_%s" % (r["barcode1_id"], r["barcode2_id"]): r["overlap"] for r in out_rows})
    for k, ty in enumerate(types):
        prefix = (type_prefixes or {}).get(ty)
        name = "%s_umi_per_probe_barcode" % prefix if prefix else "umi_per_probe_barcode"
        metrics[name] = {ids[t]: int(tags.umi_per_tag[k, t]) for t in range(len(ids)) if tags.umi_per_tag[k, t]}
    return dict(tag_ids=ids, tags=tags, runs=runs, rows=out_rows, metrics=metrics,
                barcodes_per_tag={ids[t]: int(n) for t, n in enumerate(tags.barcodes_per_tag) if n})


class MatrixSummary:
    """Result of Context.matrix_summary (crgpu_matrix_summary_dev): counts_per_feature / cells_ge2_per_feature (numpy u64 per feature,
    over the cells of the feature's own class), classes = one dict per class with the fields of crgpu_matrix_summary_class (arrays as
    lists), reads_all / reads_union (None without a read table), counts_per_cell / genes_per_cell (DeviceArrays of u32
    [n_classes, n_cells], when asked for).  floats(k) = the floats of _report for class k (crgpu_matrix_summary_stats)."""

    def __init__(self, ctx, structs, counts_per_feature, cells_ge2_per_feature, reads_all, reads_union, n_listed, counts_per_cell, genes_per_cell):
        self.ctx, self._structs, self.n_classes, self.n_listed = ctx, structs, len(structs), n_listed
        self.counts_per_feature, self.cells_ge2_per_feature = counts_per_feature, cells_ge2_per_feature
        self.reads_all, self.reads_union = reads_all, reads_union
        self.counts_per_cell, self.genes_per_cell = counts_per_cell, genes_per_cell
        self.classes = []
        for c in structs:
            d = {}
            for name, _ in _lib.MatrixSummaryClass._fields_:
                v = getattr(c, name)
                d[name] = [int(x) for x in v] if hasattr(v, "__len__") else int(v)
            for name in ("top_counts_feature", "top_counts_value", "top_cells_feature", "top_cells_value"):
                d[name] = d[name][:d["n_top"]]
            del d["reserved"]
            self.classes.append(d)

    def floats(self, k, reads_cells=None, reads_all=None):
        """mean / median / cv / iqr / std of the counts and the genes per cell, density, cum_frac, dupe_frac, reads_per_cell and
        reads_cum_frac of class k; reads_cells / reads_all default to the class's own reads and the well's (0 without a read table)"""
        return matrix_summary_stats(self._structs[k], self.classes[k]["reads_cells"] if reads_cells is None else reads_cells,
                                    (self.reads_all or 0) if reads_all is None else reads_all)


def matrix_summary_stats(cls, reads_cells=0, reads_all=0):
    """crgpu_matrix_summary_stats: cls = a _lib.MatrixSummaryClass or a dict of its integer fields -> dict of f64"""
    if isinstance(cls, dict):
        c = _lib.MatrixSummaryClass()
        for name, ctype in _lib.MatrixSummaryClass._fields_:
            if name not in cls:
                continue
            if hasattr(ctype, "_length_"):
                for i, v in enumerate(cls[name]):
                    getattr(c, name)[i] = int(v)
            else:
                setattr(c, name, int(cls[name]))
        cls = c
    out = _lib.MatrixSummaryFloats()
    rc = _lib.load().crgpu_matrix_summary_stats(C.byref(cls), int(reads_cells), int(reads_all), C.byref(out))
    if rc != 0:
        raise CrgpuError(rc, (_lib.load().crgpu_last_error(None) or b"").decode())
    return {name: getattr(out, name) for name, _ in _lib.MatrixSummaryFloats._fields_}


def _robust_divide(a, b):
    a, b = float(a), float(b)
    return float("nan") if b == 0 else a / b


def matrix_summary_metrics(summary, k, genome, feature_ids, total_reads=None, conf_mapped_reads=None, recovered_cells=None, classes=None):
    """the dict of _report (report_matrix.py:269-387) for class k of a MatrixSummary, keys prefixed with `genome` as report_genomes does
    (:479-499; "multi" for a feature type without genomes).  feature_ids[f] = the id of row f.  With total_reads (the library type's
    sequenced reads) also the keys of _report_genome_agnostic_metrics (:76-266) that need no per-genome split of barcode_summary.h5:
    the union of the cells, reads per cell, the difference from recovered_cells, the density over every class, feature_reads_in_cells
    and the usable reads, with the summary's read table standing for the conf-mapped barcoded reads of the library type.  The reference
    computes that block on the sub-matrix of ONE feature type: `classes` lists the classes of the summary that are the genomes of that
    feature type (default: every class, which is right only when the summary holds one feature type); the density and the total UMI
    counts behind `<genome>_total_conf_mapped_deduped_barcoded_reads_per_filtered_bc` are taken over them."""
    c, d = summary.classes[k], {}
    if c["n_cells"]:
        f = summary.floats(k)
        have = summary.reads_all is not None
        d["filtered_gene_bc_matrix_density"] = f["density"]
        d["filtered_bcs_top_genes_with_reads"] = {feature_ids[i]: v for i, v in zip(c["top_counts_feature"], c["top_counts_value"])}
        d["filtered_bcs_top_genes_with_unique_bcs"] = {feature_ids[i]: v for i, v in zip(c["top_cells_feature"], c["top_cells_value"])}
        d["filtered_bcs_total_unique_genes_detected"] = c["genes_detected"]
        d["filtered_bcs_total_counts"] = c["cells_total_counts"]
        for name, pre in (("unique_genes_detected", "genes"), ("counts", "counts")):
            for stat in ("mean", "median", "cv", "iqr"):
                d["filtered_bcs_%s_%s" % (stat, name)] = f["%s_%s" % (pre, stat)]
        d["filtered_bcs_cum_frac"] = f["cum_frac"]
        d["filtered_bcs_cdna_pcr_dupe_reads_frac"] = f["dupe_frac"] if have else 1 - _robust_divide(0, 0)
        d["filtered_bcs_conf_mapped_barcoded_reads_per_filtered_bc"] = f["reads_per_cell"]
        d["filtered_bcs_conf_mapped_barcoded_reads_cum_frac"] = f["reads_cum_frac"]
        d["filtered_bcs_conf_mapped_deduped_barcoded_reads_per_filtered_bc"] = _robust_divide(c["cells_total_counts"], c["n_cells"])
        d["filtered_bcs_conf_mapped_deduped_barcoded_reads_cum_frac"] = f["cum_frac"]
    out = {"%s_%s" % (genome, key): v for key, v in d.items()}
    if total_reads is not None:
        n_union = summary.n_listed
        usable, reads_all = summary.reads_union or 0, summary.reads_all or 0
        out["filtered_bcs_transcriptome_union"] = out["multi_filtered_bcs"] = n_union
        out["reads_per_cell"] = out["multi_transcriptome_total_raw_reads_per_filtered_bc"] = _robust_divide(total_reads, n_union)
        if conf_mapped_reads is not None:
            out["multi_transcriptome_total_conf_mapped_reads_per_filtered_bc"] = _robust_divide(conf_mapped_reads, n_union)
        if recovered_cells is None:
            out["multi_filtered_bcs_difference_from_recovered_cells"] = out["multi_filtered_bcs_relative_difference_from_recovered_cells"] = 0
        else:
            out["multi_filtered_bcs_difference_from_recovered_cells"] = int(n_union) - int(recovered_cells)
            out["multi_filtered_bcs_relative_difference_from_recovered_cells"] = _robust_divide(n_union - recovered_cells, recovered_cells)
        of_type = [summary.classes[i] for i in (range(summary.n_classes) if classes is None else classes)]
        out["multi_filtered_gene_bc_matrix_density"] = _robust_divide(sum(x["union_nnz"] for x in of_type),
                                                                      sum(x["n_features_class"] for x in of_type) * n_union)
        # duplicated per genome for backwards compatibility (:165-194); the deduped read type is the matrix's own total over the union
        out["%s_total_raw_reads_per_filtered_bc" % genome] = _robust_divide(total_reads, n_union)
        if conf_mapped_reads is not None:
            out["%s_total_conf_mapped_reads_per_filtered_bc" % genome] = _robust_divide(conf_mapped_reads, n_union)
        out["%s_total_conf_mapped_deduped_barcoded_reads_per_filtered_bc" % genome] = _robust_divide(
            sum(x["union_total_counts"] for x in of_type), n_union)
        out["multi_filtered_bcs_conf_mapped_barcoded_reads_cum_frac"] = out["feature_reads_in_cells"] = _robust_divide(usable, reads_all)
        out["multi_transcriptome_usable_reads_frac"] = out["frac_feature_reads_usable"] = _robust_divide(usable, total_reads)
        out["multi_usable_reads"] = usable
        out["multi_usable_reads_per_filtered_bc"] = out["feature_reads_usable_per_cell"] = _robust_divide(usable, n_union)
    return out


class Aggregates:
    """Result of Context.remove_aggregates: removed_cols (numpy u64, ascending) with reasons (numpy u8 of _lib.AGG_COUNTS |
    AGG_HIGHLY_CORRECTED | AGG_ANTIGEN per removed column), kept = the other columns (DeviceArray of u64, n_kept of them: what
    crgpu_select_barcodes_cols_dev takes), info = crgpu_aggregates_info as a dict, antigen_threshold (f64, None when no antigen
    feature), libraries = {library type: dict(number_aggregate_GEMs, reads_removed, reads_total: Python ints, the reads None
    when no read table was passed; cols, reads, umis, corrected_reads, frac_corrected_reads, frac_total_reads: numpy arrays over the
    columns removed for that library type)}."""

    def __init__(self, removed_cols, reasons, kept, n_kept, info, antigen_threshold, libraries, disabled):
        self.removed_cols, self.reasons, self.kept, self.n_kept = removed_cols, reasons, kept, n_kept
        self.info, self.antigen_threshold, self.libraries, self.disabled = info, antigen_threshold, libraries, disabled

    def cols_with(self, bits):
        return self.removed_cols[(self.reasons & bits) != 0]


AGG_LIBRARY_PREFIX = {"Antibody Capture": "ANTIBODY_", "Antigen Capture": "ANTIGEN_"}  # get_library_type_metric_prefix


def aggregate_min_antibodies(n_signal):
    """crgpu_aggregate_min_antibodies: int(np.round(n_signal * _calculate_fraction_to_use(n_signal)))"""
    out = C.c_uint32()
    rc = _lib.load().crgpu_aggregate_min_antibodies(int(n_signal), C.byref(out))
    if rc != 0:
        raise CrgpuError(rc, _lib.load().crgpu_last_error(None).decode())
    return out.value


def antigen_outlier_threshold(top_counts):
    """crgpu_antigen_outlier_threshold: (q1, q3, q3 + (q3 - q1) * 3) of the u32 counts, np.quantile's linear rule"""
    x = np.ascontiguousarray(top_counts, dtype=np.uint32)
    q1, q3, t = C.c_double(), C.c_double(), C.c_double()
    rc = _lib.load().crgpu_antigen_outlier_threshold(ptr(x), len(x), C.byref(q1), C.byref(q3), C.byref(t))
    if rc != 0:
        raise CrgpuError(rc, _lib.load().crgpu_last_error(None).decode())
    return q1.value, q3.value, t.value


def aggregate_metrics(agg):
    """the metrics of remove_antibody_antigen_aggregates (cell_calling_helpers.py:206-210) under the reference's names.
    <prefix>reads_lost_to_aggregate_GEMs is reads_removed / reads_total as ONE division (the reference sums per-barcode quotients
    in set order); None without a read table, NaN for a library type without reads"""
    out = {}
    for lib, d in agg.libraries.items():
        prefix = AGG_LIBRARY_PREFIX[lib]
        out[prefix + "number_aggregate_GEMs"] = d["number_aggregate_GEMs"]
        out[prefix + "reads_lost_to_aggregate_GEMs"] = None if d["reads_total"] is None else _robust_divide(d["reads_removed"], d["reads_total"])
    return out


RPU_STAT_NAMES = ("mean", "cv", "median", "iqrnorm", "perc80")
RPU_STAT_SUFFIXES = ("_cells_on_target", "_on_target", "_cells_off_target", "_off_target")      # the index of crgpu_rpu_stats' arrays
MIN_RPU_THRESHOLD = 2.5      # calculate_targeted_metrics/__init__.py:48


def targeted_rpu_stats(num_umis, num_reads, num_umis_cells, num_reads_cells, is_targeted, is_gex=None):
    """crgpu_targeted_rpu_stats (host, no context): the reads-per-UMI statistics of get_mean_per_gene_rpu_metrics under the
    reference's metric names, multi_cdna_pcr_dupe_reads_frac_on_target, the gene counts of get_enrichment_metrics (:167-215), and
    the quantifiable features: q_feature (u32), q_value = log10(num_reads_cells / num_umis_cells), q_label (1 = targeted)"""
    a = [np.ascontiguousarray(x, dtype=np.uint64) for x in (num_umis, num_reads, num_umis_cells, num_reads_cells)]
    F = len(a[0])
    tg = np.ascontiguousarray(is_targeted, dtype=np.uint8)
    gx = None if is_gex is None else np.ascontiguousarray(is_gex, dtype=np.uint8)
    if any(len(x) != F for x in a) or len(tg) != F or (gx is not None and len(gx) != F):
        raise ValueError("targeted_rpu_stats: one entry per feature")
    st = _lib.RpuStats()
    qf, qv, ql = np.zeros(F, np.uint32), np.zeros(F, np.float64), np.zeros(F, np.uint8)
    rc = _lib.load().crgpu_targeted_rpu_stats(F, ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(tg), ptr(gx), C.byref(st), ptr(qf), ptr(qv), ptr(ql))
    if rc != 0:
        raise CrgpuError(rc, (_lib.load().crgpu_last_error(None) or b"").decode())
    out = {}
    for k, suffix in enumerate(RPU_STAT_SUFFIXES):
        for name in RPU_STAT_NAMES:
            out["%s_reads_per_umi_per_gene%s" % (name, suffix)] = getattr(st, name)[k]
    out["multi_cdna_pcr_dupe_reads_frac_on_target"] = st.pcr_dupe_reads_frac_on_target
    for k, suffix in enumerate(("_on_target", "_off_target")):
        out["num_genes_not_detected" + suffix] = int(st.n_not_detected[k])
        out["num_genes_detected" + suffix] = int(st.n_detected[k])
        out["num_genes_not_quantifiable" + suffix] = int(st.n_not_quantifiable[k])
        out["num_genes" + suffix] = int(st.n_genes[k])
        out["num_genes_quantifiable" + suffix] = int(st.n_quantifiable[k])
    nq = int(st.n_quantifiable_total)
    out["q_feature"], out["q_value"], out["q_label"] = qf[:nq].copy(), qv[:nq].copy(), ql[:nq].copy()
    # The reference takes this column with numpy's log10, which is not the C library's to the last bit (about one value in six
    # differs by an ulp).  The Python layer hands the fit numpy's values, so that the threshold is the reference's bit for bit.
    out["q_value"] = np.log10(a[3][qf[:nq]].astype(np.float64) / a[2][qf[:nq]].astype(np.float64))
    return out


def targeted_metrics(ctx, tallies, is_targeted, summary, num_cells, total_reads, targeted_conf_mapped_reads_frac,
                     untargeted_conf_mapped_reads_frac, is_gex=None, target_class=0):
    """The `summary` dict of CALCULATE_TARGETED_METRICS' join (calculate_targeted_metrics/__init__.py:305-385, is_spatial False)
    under the reference's metric names, and the per-feature enriched_rpu column (f64 per Gene Expression feature in feature order:
    1 / 0, NaN where the reference writes NaN).  tallies: Counts.feature_metrics (summed over the ranks of a sharded well);
    summary: a Context.matrix_summary of the FILTERED cells whose class `target_class` holds the target features (its per-cell
    medians are median_umis_per_cell_on_target / median_genes_per_cell_on_target), or the two medians as a pair; num_cells,
    total_reads and the two basic_counter_summary fractions come from the caller.  The enrichment call runs on the device
    (Context.rpu_gmm); the disable_rpu_enrichments rule (:123-155, MIN_RPU_THRESHOLD 2.5) is applied."""
    nan = float("nan")
    st = targeted_rpu_stats(tallies["num_umis"], tallies["num_reads"], tallies["num_umis_cells"], tallies["num_reads_cells"], is_targeted, is_gex)
    if isinstance(summary, MatrixSummary):
        fl = summary.floats(target_class)
        med_umis, med_genes = fl["counts_median"], fl["genes_median"]
    else:
        med_umis, med_genes = (float(x) for x in summary)
    frac = float(targeted_conf_mapped_reads_frac)      # (may be NaN)
    s = {"median_umis_per_cell_on_target": med_umis, "median_genes_per_cell_on_target": med_genes,
         "total_targeted_reads_per_filtered_bc": _robust_divide(frac * total_reads, num_cells),
         "multi_frac_conf_transcriptomic_reads_on_target": targeted_conf_mapped_reads_frac,
         "multi_frac_conf_transcriptomic_reads_off_target": untargeted_conf_mapped_reads_frac}
    s.update({k: v for k, v in st.items() if not k.startswith("q_") and not k.startswith("num_genes")})
    key = s["mean_reads_per_umi_per_gene_cells_on_target"]
    disable = math.isnan(key) or key < MIN_RPU_THRESHOLD
    fit = ctx.rpu_gmm(st["q_value"], st["q_label"])
    te, tn, oe, on = (fit[k] for k in ("n_targeted_enriched", "n_targeted_not_enriched", "n_offtgt_enriched", "n_offtgt_not_enriched"))
    fracs = [f for f in (_robust_divide(oe, oe + te), _robust_divide(oe, oe + on)) if not math.isnan(f)]
    m = {"log_rpu_threshold": fit["log_rpu_threshold"], "lrpu_fitted_mean_1": fit["mu_high"], "lrpu_fitted_mean_2": fit["mu_low"],
         "lrpu_fitted_sd_1": fit["sd_high"], "lrpu_fitted_sd_2": fit["sd_low"], "lrpu_fitted_weight_1": fit["alpha_high"],
         "lrpu_fitted_weight_2": fit["alpha_low"], "frac_on_target_genes_enriched": _robust_divide(te, te + tn),
         "frac_off_target_genes_enriched": min(fracs) if fracs else nan,      # np.nanmin
         "num_rpu_enriched_genes_on_target": te, "num_rpu_non_enriched_genes_on_target": tn,
         "num_rpu_enriched_genes_off_target": oe, "num_rpu_non_enriched_genes_off_target": on}
    thr = fit["log_rpu_threshold"]
    if not math.isnan(thr) and disable:      # the enrichments look bad because the depth is too low: do not report them
        f_on, f_off = m["frac_on_target_genes_enriched"], m["frac_off_target_genes_enriched"]
        if math.isnan(f_on) or f_on < 0.5 or (not math.isnan(f_off) and f_off > 0.5):
            m = {k: nan for k in m}
            thr = nan
    s.update(m)
    s.update({k: v for k, v in st.items() if k.startswith("num_genes")})
    gex = np.ones(len(np.asarray(is_targeted)), bool) if is_gex is None else np.asarray(is_gex).astype(bool)
    uc, rc_ = np.asarray(tallies["num_umis_cells"], np.float64)[gex], np.asarray(tallies["num_reads_cells"], np.float64)[gex]
    col = np.full(int(gex.sum()), nan)
    if not math.isnan(thr):
        with np.errstate(divide="ignore", invalid="ignore"):
            col = (np.log10(rc_ / uc) > thr).astype(np.float64)      # NaN > thr is False, as in pandas
    return s, col


# ---- cell-multiplexed (CMO) wells: the JIBES tag caller ---------------------------------------------------------------------------
N_G = 95000      # feature/throughputs.py
G19_N_GEMS = {"MT": N_G, "LT": 9500, "HT": 190000}
JIBES_MIN_CONFIDENCE = 0.9
JIBES_MULTIPLET, JIBES_BLANK, JIBES_UNASSIGNED = "Multiplet", "Blank", "Unassigned"


class CellEstimateCantConverge(RuntimeError):
    """the reference's CellEstimateCantConvergeException"""


def jibes_expected_cells(n, n_gems=N_G):
    """feature_assigner.calculate_expected_total_cells as a bracketed root (crgpu_jibes_expected_cells, host only)"""
    out = C.c_double()
    rc = _lib.load().crgpu_jibes_expected_cells(int(n), int(n_gems), C.byref(out))
    if rc == _lib.JIBES_CANT_CONVERGE:
        raise CellEstimateCantConverge("Could not converge on an accurate cell estimate.")
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_jibes_expected_cells")
    return out.value


def jibes_latent_states(n, k, n_gems=N_G, max_k_lets=3, estimated_cells=None, blank_prob=0.04, freqs=None):
    """JibesEMO3::new and calculate_latent_state_weights (host only) -> dict(states u8[z, k], prior f64[z], k_let_limited,
    max_multiplets, max_modeled_k_let, estimated_cells).  estimated_cells None: jibes_expected_cells(n, n_gems)."""
    L = _lib.load()
    est = jibes_expected_cells(n, n_gems) if estimated_cells is None else float(estimated_cells)
    su = _lib.JibesSetup()
    states = np.zeros((_lib.JIBES_MAX_STATES, max(int(k), 1)), np.uint8)
    rc = L.crgpu_jibes_latent_states(int(n), int(k), int(n_gems), int(max_k_lets), est, ptr(states), C.byref(su))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_jibes_latent_states: k = %d, max_k_lets = %d" % (k, max_k_lets))
    states = np.ascontiguousarray(states.reshape(-1)[:su.n_states * k].reshape(su.n_states, k))
    fr = None if freqs is None else np.ascontiguousarray(freqs, dtype=np.float64)
    prior = np.zeros(su.n_states, np.float64)
    rc = L.crgpu_jibes_log_prior(ptr(states), su.n_states, int(k), est, int(n_gems), int(max_k_lets), su.k_let_limited, su.max_modeled_k_let,
                                 float(blank_prob), ptr(fr), ptr(prior))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_jibes_log_prior")
    return dict(states=states, prior=prior, k_let_limited=bool(su.k_let_limited), max_multiplets=int(su.max_multiplets),
                max_modeled_k_let=int(su.max_modeled_k_let), estimated_cells=est)


def jibes_initial_parameters(y, calls):
    """jibes.create_initial_parameters (host only): y f64[n, k], calls per barcode a tag index or -1 -> (bg, fg, sd)"""
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 2:
        raise ValueError("jibes_initial_parameters: y is n x k")
    calls = np.ascontiguousarray(calls, dtype=np.int32)
    if len(calls) != len(y):
        raise ValueError("jibes_initial_parameters: one call per barcode")
    k = y.shape[1]
    bg, fg, sd = np.zeros(k), np.zeros(k), np.zeros(k)
    rc = _lib.load().crgpu_jibes_initial_parameters(ptr(y) if len(y) else None, len(y), k, ptr(calls) if len(y) else None, ptr(bg), ptr(fg), ptr(sd))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_jibes_initial_parameters")
    return bg, fg, sd


def call_tags_jibes(ctx, filtered, tag_rows, valid_tags, prelim_calls, throughput="MT", confidence=None, exclude_blanks_from_posterior=False,
                    tag_names=None, n_gems=None, n_features=None, estimated_cells=None, abs_tol=0.1, rel_tol=1e-7, max_reps=50000):
    """run_assignment_stage + JibesTagAssigner.get_tag_assignments on the filtered MatrixDev: tag_rows = the feature rows of the
    Multiplexing Capture library (ascending), valid_tags = a mask over them (the tags the marginal caller saw), prelim_calls = per
    barcode of the matrix an index into the VALID tags or -1 (the marginal caller's call when it is one tag).  Near-zero barcodes
    (<= 12 counts over ALL tag rows) are Blank with probability 1 and never enter the fit.
    -> dict(table = the per-barcode columns of the fit (see Context.jibes_fit) for the kept barcodes, kept, near_zero,
    barcodes_per_tag (per valid tag the matrix columns assigned to it; a Multiplet goes to every tag of its most likely multiplet
    state), non_singlets {Blank, Unassigned, Multiplet} with the near-zero barcodes appended to Blank, snr {snr_<tag>: fg / sd},
    fit)."""
    confidence = JIBES_MIN_CONFIDENCE if confidence is None else confidence
    n_gems = G19_N_GEMS.get(throughput, N_G) if n_gems is None else n_gems
    valid = np.asarray(valid_tags, bool)
    if len(valid) != len(tag_rows) or not valid.any():
        raise ValueError("call_tags_jibes: valid_tags is a mask over tag_rows with at least one tag set")
    names = ["tag%d" % i for i in range(len(valid))] if tag_names is None else [n.decode() if isinstance(n, bytes) else n for n in tag_names]
    names = [n for n, v in zip(names, valid) if v]
    tab = ctx.jibes_tag_counts(filtered, tag_rows, n_features)
    kept, near_zero = tab["kept"], tab["near_zero"]
    y = np.ascontiguousarray(tab["log_counts"][kept][:, valid])
    calls = np.asarray(prelim_calls, np.int32)[kept]
    bg, fg, sd = jibes_initial_parameters(y, calls)
    fit = ctx.jibes_fit(y, bg, fg, sd, n_gems=n_gems, estimated_cells=estimated_cells, abs_tol=abs_tol, rel_tol=rel_tol, max_reps=max_reps,
                        confidence=confidence, exclude_blanks_from_posterior=exclude_blanks_from_posterior)
    k = y.shape[1]
    states = fit["states"]
    per_tag = [[] for _ in range(k)]
    non = {JIBES_BLANK: [], JIBES_UNASSIGNED: [], JIBES_MULTIPLET: []}
    for i, a in enumerate(fit["assignment"].tolist()):
        bc = int(kept[i])
        if a < k:
            per_tag[a].append(bc)
        elif a == k:
            non[JIBES_MULTIPLET].append(bc)
            for t in np.nonzero(states[fit["ml_state"][i]])[0]:
                per_tag[int(t)].append(bc)
        else:
            non[JIBES_BLANK if a == k + 1 else JIBES_UNASSIGNED].append(bc)
    non[JIBES_BLANK] += [int(b) for b in near_zero]
    snr = {"snr_" + n: float(fit["fg"][t] / fit["sd"][t]) for t, n in enumerate(names)}
    return dict(table={q: fit[q] for q in ("probs", "assignment", "assignment_prob", "ml_state")}, kept=kept, near_zero=near_zero,
                barcodes_per_tag=dict(zip(names, per_tag)), non_singlets=non, snr=snr, fit=fit, tag_names=names)


# ---- marginal calls of guides, antibodies and tags ----------------------------------------------------------------------------------
GUIDE_UMI_THRESHOLD = 3
MIN_COUNTS_PER_ANTIBODY = 1000
ANTIBODY_ASSIGNMENT_LIST = (b"CD3", b"CD19", b"CD14")
MIN_COUNTS_PER_TAG, COUNTS_DYNAMIC_RANGE, MAX_ALLOWED_PEARSON_CORRELATION = 1000, 50.0, 0.5
NUM_TOTAL_TAGS = 14


def _robust_divide(a, b):
    return float("nan") if b == 0 else float(a) / float(b)


def assignment_metadata(num_cells, n_single, n_multiple, n_without_umis):
    """AssignmentMetadata of compute_generic_assignment_metadata (feature_assigner.py:234-269, 397-412) from the four integers"""
    with_features = n_single + n_multiple
    return dict(num_cells=int(num_cells), num_cells_without_features=int(num_cells - with_features),
                frac_cells_without_features=_robust_divide(num_cells - with_features, num_cells),
                num_cells_without_feature_umis=int(n_without_umis), frac_cells_without_feature_umis=_robust_divide(n_without_umis, num_cells),
                num_singlets=int(n_single), frac_singlets=_robust_divide(n_single, num_cells), num_multiplets=int(n_multiple),
                frac_multiplets=_robust_divide(n_multiple, num_cells))


class MarginalCalls:
    """crgpu_marginal_calls: the fit and the calls of every listed feature row (Context.marginal_calls).  per_feature: a dict of
    numpy arrays, one value per row (status, in_lds, total_umis, cells_assigned, umi_threshold_observed, mean_low, mean_high,
    weight_low, weight_high, covariance, lower_bound, winner, n_iter, n_distinct); the device arrays are downloaded on request."""

    def __init__(self, ctx, view_ptr, feature_rows, umi_threshold):
        self.ctx, self._v = ctx, view_ptr
        v = view_ptr.contents
        self.feature_rows, self.umi_threshold = np.array(feature_rows, np.uint32), int(umi_threshold)
        self.n_rows, self.n_barcodes, self.n_assigned = int(v.n_rows), int(v.n_barcodes), int(v.n_assigned)
        rows = np.ctypeslib.as_array(C.cast(v.rows, C.POINTER(C.c_uint8)), (self.n_rows * C.sizeof(_lib.MarginalRow),)).copy()
        rec = rows.view(np.dtype([(n, {C.c_uint32: "<u4", C.c_uint64: "<u8", C.c_int64: "<i8", C.c_double: "<f8"}[t]) for n, t in _lib.MarginalRow._fields_]))
        self.per_feature = {n: rec[n].copy() for n, _ in _lib.MarginalRow._fields_ if n != "reserved"}
        self.cells_with_0, self.cells_with_1, self.cells_with_many = int(v.cells_with_0), int(v.cells_with_1), int(v.cells_with_many)
        self.cells_without_umis = int(v.cells_without_umis)
        self.phase_ms = dict(extract=v.ms_extract, histogram=v.ms_histogram, fit=v.ms_fit, assign=v.ms_assign)
        self.has_histograms = bool(v.d_hist_offsets)

    def _down(self, p, n, dtype):
        out = np.zeros(n, dtype)
        if n:
            self.ctx._check(self.ctx.L.crgpu_memcpy_d2h(self.ctx.h, ptr(out), p, out.nbytes))
        return out

    def assignments(self):
        """the assignment matrix as CSR over the listed rows -> (indptr i64[n_rows + 1], columns u32[n_assigned], ascending in a row)"""
        v = self._v.contents
        return self._down(v.d_indptr, self.n_rows + 1, np.int64), self._down(v.d_columns, self.n_assigned, np.uint32)

    def cells_per_feature(self):
        indptr, cols = self.assignments()
        return [cols[indptr[p]:indptr[p + 1]] for p in range(self.n_rows)]

    @property
    def features_per_cell(self):
        return self._down(self._v.contents.d_features_per_cell, self.n_barcodes, np.uint32)

    def umi_thresholds(self):
        """_compute_umi_thresholds: {place in the list: the lowest count among the cells assigned the feature}; rows without a call are left out"""
        t = self.per_feature["umi_threshold_observed"]
        return {p: int(t[p]) for p in range(self.n_rows) if self.per_feature["cells_assigned"][p] > 0}

    def histogram(self, p):
        """(values i32, multiplicities u32) of listed row p, values ascending, the zeros one bin (want_histograms)"""
        if not self.has_histograms:
            raise ValueError("MarginalCalls.histogram: the call was made without want_histograms")
        v = self._v.contents
        off = self._down(v.d_hist_offsets, self.n_rows + 1, np.int64)
        nd = int(self.per_feature["n_distinct"][p])
        isz = 4
        return (self._down(v.d_hist_values + int(off[p]) * isz, nd, np.int32), self._down(v.d_hist_counts + int(off[p]) * isz, nd, np.uint32))

    def metadata(self):
        return assignment_metadata(self.n_barcodes, self.cells_with_1, self.cells_with_many, self.cells_without_umis)

    def free(self):
        if self._v is not None and self.ctx.h:
            self.ctx.L.crgpu_marginal_calls_free(self.ctx.h, self._v)
        self._v = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def tag_contaminants(sum_x, sum_xx, sum_xy, n_cells, order, min_counts=MIN_COUNTS_PER_TAG, dynamic_range=COUNTS_DYNAMIC_RANGE,
                     max_cor=MAX_ALLOWED_PEARSON_CORRELATION):
    """identify_contaminant_tags on the integer moments (crgpu_tag_contaminants, host only): order = the tags sorted by id as a
    permutation -> (flags u8[n]: 0 kept, 1 contaminant, 2 dropped for zero UMIs; sources: per tag the list of its source tags)"""
    sx, sxx = np.ascontiguousarray(sum_x, dtype=np.uint64), np.ascontiguousarray(sum_xx, dtype=np.uint64)
    sxy, order = np.ascontiguousarray(sum_xy, dtype=np.uint64), np.ascontiguousarray(order, dtype=np.uint32)
    n = len(sx)
    flags, src = np.zeros(n, np.uint8), np.full((n, n), -1, np.int32)
    rc = _lib.load().crgpu_tag_contaminants(n, int(n_cells), ptr(sx), ptr(sxx), ptr(sxy), ptr(order), int(min_counts), float(dynamic_range),
                                            float(max_cor), ptr(flags), ptr(src))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_tag_contaminants")
    return flags, [[int(x) for x in row if x >= 0] for row in src]


def marginal_seed_draws(V):
    """test hook: (u f64[10, 3], first_cell u64[10]) of a fit over V cells"""
    u, first = np.zeros((_lib.MC_INITS, 3)), np.zeros(_lib.MC_INITS, np.uint64)
    rc = _lib.load().crgpu_marginal_seed_draws(int(V), ptr(u), ptr(first))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_marginal_seed_draws")
    return u, first


def kmeans_trials(k):
    """2 + int(np.log(k)): the trial candidates scikit-learn draws for each centre after the first"""
    return 2 + int(math.log(k))


def kmeans_seed_draws(seed, n, k):
    """test hook: (u f64[1 + (k - 1) kmeans_trials(k)], first_cell) of a k-means fit over n cells under RandomState(seed)"""
    u, first = np.zeros(1 + (k - 1) * kmeans_trials(k)), C.c_uint64(0)
    rc = _lib.load().crgpu_kmeans_seed_draws(int(seed), int(n), int(k), ptr(u), C.byref(first))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_kmeans_seed_draws")
    return u, int(first.value)


def kmeans_db_index(centers, wss, counts):
    """compute_db_index from its per-cluster sums (crgpu_kmeans_db_index, host only) -> the Davies-Bouldin score"""
    c = np.ascontiguousarray(centers, dtype=np.float64)
    w, cnt = np.ascontiguousarray(wss, dtype=np.float64), np.ascontiguousarray(counts, dtype=np.uint64)
    if c.ndim != 2 or len(w) != len(c) or len(cnt) != len(c):
        raise ValueError("kmeans_db_index: centers is k x d, wss and counts have k values")
    score = C.c_double(0.0)
    rc = _lib.load().crgpu_kmeans_db_index(c.shape[0], c.shape[1], ptr(c), ptr(w), ptr(cnt), C.byref(score))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_kmeans_db_index")
    return score.value


def kmeans_clustering_key(n_clusters, library_prefix=None):
    """format_clustering_key for a k-means clustering; library_prefix "gene_expression" / "antibody_capture" goes in front"""
    key = "kmeans_%d_clusters" % n_clusters
    return "%s_%s" % (library_prefix, key) if library_prefix else key


def run_kmeans(ctx, projection, max_clusters=10, min_clusters=2, seed=0, num_pcs=None, library_prefix=None):
    """RUN_KMEANS for one library type: the cells x PCs projection clustered for K = min_clusters .. min(max_clusters, cells) in one
    device call -> {clustering key: dict(clusters i32[n] 1-based by size, cluster_score, centers, num_clusters, global_sort_key)}"""
    n = np.shape(projection)[0]
    ks = list(range(min_clusters, min(max_clusters, n) + 1))      # split(): max_clusters = min(max_clusters, the number of barcodes)
    if not ks:
        return {}
    out = {}
    for r in ctx.kmeans(projection, ks, seed=seed, num_pcs=num_pcs):
        out[kmeans_clustering_key(r["n_clusters"], library_prefix)] = dict(
            clusters=r["clusters"], cluster_score=r["db_score"], centers=r["centers"], num_clusters=r["n_clusters"], global_sort_key=r["n_clusters"])
    return out


class MatrixRankTooSmall(Exception):
    """run_pca's MatrixRankTooSmallException: min(features, barcodes) after thresholding < n_components at the threshold 2"""


class NullAxisMatrix(Exception):
    """NullAxisMatrixError of select_axes_above_threshold: no barcode, or no feature, with a sum above the threshold"""


def run_pca(ctx, m, n_components=10, pca_features=None, pca_bc_indices=None, seed=0, n_features=None, **seams):
    """RUN_PCA for one library type (mro/rna/stages/analyzer/run_pca/__init__.py:57-80): Context.pca of the filtered MatrixDev `m` (one
    feature type: select_features_dev) at the threshold 2 and, after MatrixRankTooSmall or NullAxisMatrix, at the threshold 0, where
    n_components is reduced to min(features, barcodes) -> the dict of Context.pca with retried = the second call was needed.  Its
    `projection` goes into run_kmeans, run_graph_clustering and correct_chemistry_batch unchanged.  A NullAxisMatrix of the second call
    is raised.  pca_bc_indices are positions among the barcodes THE CALL's threshold leaves"""
    try:
        r = ctx.pca(m, n_components, pca_features, pca_bc_indices, seed, _lib.PCA_DEFAULT_THRESHOLD, n_features=n_features, **seams)
        r["retried"] = False
    except (MatrixRankTooSmall, NullAxisMatrix):
        r = ctx.pca(m, n_components, pca_features, pca_bc_indices, seed, 0, n_features=n_features, **seams)
        r["retried"] = True
    return r


def legacy_randn(seed, n):
    """np.random.RandomState(seed).randn(n) by the library (crgpu_legacy_randn, host only)"""
    out = np.zeros(int(n))
    rc = _lib.load().crgpu_legacy_randn(int(seed), int(n), ptr(out))
    if rc != 0:
        raise ValueError("legacy_randn: refused (%d)" % rc)
    return out


def normalized_dispersion(mu, var, nbins=20):
    """get_normalized_dispersion by the library (crgpu_normalized_dispersion, host only)"""
    mu, var = np.ascontiguousarray(mu, dtype=np.float64), np.ascontiguousarray(var, dtype=np.float64)
    out = np.zeros(len(mu))
    rc = _lib.load().crgpu_normalized_dispersion(ptr(mu), ptr(var), len(mu), int(nbins), ptr(out))
    if rc != 0:
        raise ValueError("normalized_dispersion: refused (%d)" % rc)
    return out


def small_svd(b):
    """B = U diag(s) Vt by the library's one-sided Jacobi (crgpu_small_svd, host only) -> (U, s, Vt)"""
    b = np.ascontiguousarray(b, dtype=np.float64)
    n = len(b)
    u, s, vt = np.zeros((n, n)), np.zeros(n), np.zeros((n, n))
    rc = _lib.load().crgpu_small_svd(ptr(b), n, ptr(u), ptr(s), ptr(vt))
    if rc != 0:
        raise ValueError("small_svd: refused (%d)" % rc)
    return u, s, vt


def graphclust_num_neighbors(n, num_neighbors=None, neighbor_a=None, neighbor_b=None):
    """split() of RUN_GRAPH_CLUSTERING (crgpu_graphclust_num_neighbors, host only): int(max(num_neighbors, np.round(a + b * log10(n))))
    clamped to [1, n - 1]; None = the reference's defaults 1, -230.0, 120.0"""
    k = C.c_uint32(0)
    rc = _lib.load().crgpu_graphclust_num_neighbors(
        int(n), int(_lib.GRAPHCLUST_NEIGHBORS_DEFAULT if num_neighbors is None else num_neighbors),
        float(_lib.GRAPHCLUST_NEIGHBOR_A_DEFAULT if neighbor_a is None else neighbor_a),
        float(_lib.GRAPHCLUST_NEIGHBOR_B_DEFAULT if neighbor_b is None else neighbor_b), C.byref(k))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_graphclust_num_neighbors")
    return int(k.value)


def louvain_labels(num_barcodes, use_bcs, pairs):
    """load_louvain_results: pairs = the (node, community) lines of the louvain binary's output, every level of the hierarchy in turn.
    The first occurrence of a node wins; ids are 1-based; a barcode that was not used gets 0 -> i64[num_barcodes]"""
    labels = np.zeros(int(num_barcodes), dtype=np.int64)
    use_bcs = np.asarray(use_bcs)
    seen = set()
    for node, community in pairs:
        node = int(node)
        if node in seen:
            continue
        seen.add(node)
        labels[use_bcs[node]] = 1 + int(community)
    return labels


def relabel_by_size(labels):
    """relabel_by_size (clustering.py): label l becomes 1 + the rank of l among all labels 0 .. max by descending size; equal sizes
    keep their ascending order.  Label 0 (a barcode that was not used) takes part in the ranking as it does in the reference, so with
    unused barcodes around no cluster is called by their rank"""
    labels = np.asarray(labels)
    by_size = np.argsort(-np.bincount(labels), kind="stable")
    rank = np.empty(len(by_size), dtype=np.int64)
    rank[by_size] = np.arange(len(by_size))
    return 1 + rank[labels]


def write_louvain_edges(file, nn_indptr, nn_indices):
    """pipe_unweighted_edgelist_to_convert's lines: "%d\\t%d\\n" per entry of the neighbour matrix in CSR order (row, then column
    ascending), which is the order nn.tocoo() gives `convert`; file: anything with write(), text or bytes -> the number of lines"""
    indptr, indices = np.asarray(nn_indptr, dtype=np.int64), np.asarray(nn_indices, dtype=np.int64)
    binary = "b" in getattr(file, "mode", "") or isinstance(file, (io.BytesIO, io.BufferedIOBase, io.RawIOBase))
    rows = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
    step = 1 << 16
    for lo in range(0, len(indices), step):
        text = "".join("%d\t%d\n" % ij for ij in zip(rows[lo:lo + step].tolist(), indices[lo:lo + step].tolist()))
        file.write(text.encode("ascii") if binary else text)
    return len(indices)


def louvain_pairs(result):
    """The (node, community) lines `louvain -l -1` would print for Context.louvain's result: every level in turn, a level's nodes
    ascending -> a list of (int, int); louvain_labels keeps the first occurrence of a node, which is its level-0 line"""
    return [(i, int(c)) for level in result["levels"] for i, c in enumerate(np.asarray(level).tolist())]


def modularity(indptr, indices, labels, weights=None):
    """The exact modularity of a labelling (labels >= 0) of a symmetric CSR graph, a self-loop once, weights None = 1
    (crgpu_modularity, host only): S = sum_C (in_C * M - tot_C^2) and M = the sum of all entries as integers -> (S, M, Q = S / M^2)"""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices, labels = np.ascontiguousarray(indices, dtype=np.int32), np.ascontiguousarray(labels, dtype=np.int32)
    n = len(indptr) - 1
    if n < 1 or len(labels) != n or len(indices) < indptr[-1] or (weights is not None and len(weights) != len(indices)):
        raise ValueError("modularity: indptr of n + 1, n labels, indices and weights of indptr[n] elements")
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint32)
    S, M = C.c_int64(0), C.c_int64(0)
    rc = _lib.load().crgpu_modularity(ptr(indptr), ptr(indices), None if w is None else ptr(w), n, ptr(labels), C.byref(S), C.byref(M))
    if rc != 0:
        raise ValueError("modularity: refused (%d)" % rc)
    return int(S.value), int(M.value), S.value / float(M.value) ** 2


def linkage_complete(points):
    """scipy.cluster.hierarchy.linkage(points, "complete") (crgpu_linkage_complete, host only): points f64[K, d], K >= 2 -> Z f64[K - 1, 4],
    rows ascending by height, the smaller id first, the cluster of row s numbered K + s, column 3 its size.  Equal distances merge by the
    smallest (height, id0, id1); scipy's order among ties is not reproduced"""
    pts = np.ascontiguousarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[0] < 2 or pts.shape[1] < 1:
        raise ValueError("linkage_complete: points is K x d with K >= 2")
    z = np.zeros((pts.shape[0] - 1, 4))
    rc = _lib.load().crgpu_linkage_complete(ptr(pts), pts.shape[0], pts.shape[1], ptr(z))
    if rc != 0:
        raise ValueError("linkage_complete: refused (%d)" % rc)
    return z


def merge_clusters(ctx, m, projection, labels, n_features=None, num_pcs=None, de_threshold=0.05):
    """MERGE_CLUSTERS (stages/analyzer/merge_clusters join(), what graph_clustering.rs:156 calls after Louvain), statement by statement:
    m = the filtered MatrixDev with all of its features, projection f64[barcodes x PCs], labels 1-based with 0 for a barcode that was
    not used (run_graph_clustering's labels).  Loop: the per-cluster medians of the PCs (Context.cluster_medians), linkage_complete,
    for every row whose two ids are leaves a local sSeq test (SseqPairs.compare on ONE plan made from the initial labels; a pair
    already tested is skipped), a merge into the smaller label when no gene has adjusted p < de_threshold, then from the top; it ends
    with one cluster or a walk without a merge.  -> dict(labels = the stage's final_labels (relabel_by_size, 0 = not used), steps = per
    iteration and pair dict(iteration, leaf0, leaf1, groups0, groups1 (the initial 0-based groups), skipped, n_de, merged), n_tests,
    n_skipped, n_merges, n_iterations, n_clusters_in, n_clusters_out, plan_ms, medians_ms, linkage_ms, pairs_ms, total_ms)"""
    t_all = time.perf_counter()
    labels = np.asarray(labels)
    x = np.ascontiguousarray(projection, dtype=np.float64)
    if labels.ndim != 1 or len(labels) != m.n_barcodes or x.ndim != 2 or x.shape[0] != len(labels):
        raise ValueError("merge_clusters: one label and one projection row per barcode of the matrix")
    d = x.shape[1] if num_pcs is None else min(x.shape[1], int(num_pcs))
    total_bcs = len(labels)
    use_bcs = np.flatnonzero(labels > 0)
    if len(use_bcs) == 0:
        raise ValueError("merge_clusters: no barcode has a cluster")
    lab = labels[use_bcs].astype(np.int64) - 1
    n_in = int(lab.max()) + 1
    pca = np.ascontiguousarray(x[use_bcs, :d])
    groups = np.full(total_bcs, -1, np.int32)
    groups[use_bcs] = lab
    members = [[g] for g in range(n_in)]      # the initial groups of every current cluster, ascending
    times = dict(plan_ms=0.0, medians_ms=0.0, linkage_ms=0.0, pairs_ms=0.0)
    steps, checked = [], set()
    n_tests = n_skipped = n_merges = n_iterations = 0
    pairs = None
    try:
        while len(members) > 1:
            n_iterations += 1
            if pairs is None:
                t0 = time.perf_counter()
                pairs = ctx.sseq_pairs(m, groups, n_features=n_features)
                times["plan_ms"] += (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            medoids = ctx.cluster_medians(pca, lab, len(members))["medians"]
            t1 = time.perf_counter()
            hc = linkage_complete(medoids)
            times["medians_ms"] += (t1 - t0) * 1e3
            times["linkage_ms"] += (time.perf_counter() - t1) * 1e3
            max_label = len(members) - 1
            any_merged = False
            for step in range(hc.shape[0]):
                if not (hc[step, 0] <= max_label and hc[step, 1] <= max_label):
                    continue
                leaf0, leaf1 = int(hc[step, 0]), int(hc[step, 1])
                rec = dict(iteration=n_iterations, leaf0=leaf0, leaf1=leaf1, groups0=list(members[leaf0]), groups1=list(members[leaf1]), skipped=False,
                           n_de=None, merged=False)
                steps.append(rec)
                key = frozenset((frozenset(members[leaf0]), frozenset(members[leaf1])))
                if key in checked:
                    rec["skipped"] = True
                    n_skipped += 1
                    continue
                checked.add(key)
                t0 = time.perf_counter()
                r = pairs.compare(members[leaf0], members[leaf1], de_threshold=de_threshold, vectors=False)
                times["pairs_ms"] += (time.perf_counter() - t0) * 1e3
                n_tests += 1
                rec["n_de"] = r["n_de"]
                if r["n_de"] == 0:
                    lab[lab == leaf1] = leaf0
                    lab[lab > leaf1] -= 1
                    members[leaf0] = sorted(members[leaf0] + members[leaf1])
                    del members[leaf1]
                    rec["merged"] = any_merged = True
                    n_merges += 1
                    break
            if not any_merged:
                break
    finally:
        if pairs is not None:
            pairs.free()
    final = np.zeros(total_bcs, dtype=np.int64)
    final[use_bcs] = relabel_by_size(lab + 1)
    out = dict(labels=final, steps=steps, n_tests=n_tests, n_skipped=n_skipped, n_merges=n_merges, n_iterations=n_iterations, n_clusters_in=n_in,
               n_clusters_out=len(members))
    out.update(times, total_ms=(time.perf_counter() - t_all) * 1e3)
    return out


def run_graph_clustering(ctx, projection, num_neighbors=None, neighbor_a=None, neighbor_b=None, input_pcs=None, louvain=None,
                         num_barcodes=None, use_bcs=None, queries_per_call=_lib.NN_QUERIES_PER_CHUNK, merge_matrix=None):
    """RUN_GRAPH_CLUSTERING up to the Louvain binary: k by split()'s rule, the exact k nearest neighbours of every row of the cells x PCs
    projection (Context.knn, in calls of queries_per_call rows as the reference's chunks), the neighbour matrix of join()
    -> dict(num_neighbors, indices i32[n, k] by rank, distances f64[n, k], nn_indptr i64[n + 1], nn_indices i32[n k] (row-wise
    ascending: the CSR matrix of merge_nearest_neighbors, every value 1), nn_nodes, nn_links, nn_density, pairs_evaluated, fit_ms).
    louvain: None, or a callable (row, col) -> the (node, community) pairs of the binary's output for that edge list; then also labels
    (louvain_labels(num_barcodes, use_bcs, pairs); default every row in order) and clusters (relabel_by_size(labels)).
    louvain="device": Context.louvain on the neighbour matrix (the published algorithm in synchronous integer rounds, no parity with
    bin/louvain); labels = level 0 plus 1 (0 for a barcode that was not used) = louvain_labels(.., louvain_pairs(result)), clusters =
    relabel_by_size(labels), final_clusters = the same of the last level, levels = the partition of every level, modularity = Q per
    level, louvain = Context.louvain's dict.
    merge_matrix: with a louvain, the filtered MatrixDev (all features, one column per barcode of labels, the projection one row per
    barcode): adds merge = merge_clusters(ctx, merge_matrix, projection, labels, num_pcs=input_pcs), merged_labels = its labels and
    merged_clusters = relabel_by_size(merged_labels), what RUN_GRAPH_CLUSTERING_NG reports; None (the default) changes nothing"""
    if isinstance(louvain, str) and louvain != "device":
        raise ValueError("run_graph_clustering: louvain is None, a callable or \"device\"")
    x = np.asarray(projection)
    if x.ndim != 2:
        raise ValueError("run_graph_clustering: the projection is cells x PCs")
    n = x.shape[0]
    d = x.shape[1] if input_pcs is None else min(x.shape[1], int(input_pcs))
    k = graphclust_num_neighbors(n, num_neighbors, neighbor_a, neighbor_b)
    x = np.ascontiguousarray(x, dtype=np.float64)
    ind, dist, srt = np.zeros((n, k), np.int32), np.zeros((n, k)), np.zeros((n, k), np.int32)
    pairs_evaluated, fit_ms = 0, 0.0
    for q0 in range(0, n, int(queries_per_call)):
        r = ctx.knn(x, k, num_pcs=d, query_start=q0, n_queries=min(int(queries_per_call), n - q0))
        q1 = q0 + len(r["indices"])
        ind[q0:q1], dist[q0:q1], srt[q0:q1] = r["indices"], r["distances"], r["sorted_indices"]
        pairs_evaluated += r["pairs_evaluated"]
        fit_ms += r["fit_ms"]
    out = dict(num_neighbors=k, indices=ind, distances=dist, nn_indptr=np.arange(n + 1, dtype=np.int64) * k, nn_indices=srt.reshape(-1),
               nn_nodes=n, nn_links=n * k, nn_density=(n * k) / float(n * n), pairs_evaluated=pairs_evaluated, fit_ms=fit_ms)
    if isinstance(louvain, str):
        r = ctx.louvain(out["nn_indptr"], out["nn_indices"], symmetrize=True)
        use = np.arange(n) if use_bcs is None else np.asarray(use_bcs)
        out["labels"] = np.zeros(n if num_barcodes is None else int(num_barcodes), dtype=np.int64)
        out["labels"][use] = 1 + r["level0"].astype(np.int64)      # load_louvain_results: the first occurrence of a node is its level-0 line
        final = np.zeros(len(out["labels"]), dtype=np.int64)
        final[use] = 1 + r["final"].astype(np.int64)
        out.update(clusters=relabel_by_size(out["labels"]), final_clusters=relabel_by_size(final), levels=r["levels"],
                   modularity=[S / float(r["M"]) ** 2 for S in r["S"]], louvain=r)
    elif louvain is not None:
        row = np.repeat(np.arange(n, dtype=np.int64), k)
        pairs = louvain(row, out["nn_indices"].astype(np.int64))
        out["labels"] = louvain_labels(n if num_barcodes is None else num_barcodes, np.arange(n) if use_bcs is None else use_bcs, pairs)
        out["clusters"] = relabel_by_size(out["labels"])
    if merge_matrix is not None and louvain is not None:
        out["merge"] = merge_clusters(ctx, merge_matrix, projection, out["labels"], num_pcs=input_pcs)
        out["merged_labels"] = out["merge"]["labels"]
        out["merged_clusters"] = relabel_by_size(out["merged_labels"])
    return out


def get_tsne_name(feature_type, n_components):
    """get_tsne_name of stages/analyzer/run_tsne: "gene_expression_2-d\""""
    return "%s_%d-d" % (feature_type.replace(" ", "_").lower(), n_components)


def get_tsne_key(feature_type, n_components):
    """get_tsne_key of stages/analyzer/run_tsne: the bare number for Gene Expression (pre-3.0 HDF5 files), else "antibody_capture_2\""""
    if feature_type == "Gene Expression":
        return str(n_components)
    return "%s_%d" % (feature_type.replace(" ", "_").lower(), n_components)


def tsne_feature_input(m, n_features=None):
    """The t-SNE input of the feature types without a PCA (antibody-only and the other non-gene-expression types of
    stages/analyzer/run_tsne): the dense cells x features matrix log2(1 + count) of a filtered MatrixDev, made on the host from
    MatrixDev.download().  More than 128 features: ValueError (the neighbour search takes at most 128 columns)"""
    _, indptr, indices, data = m.download()
    n_cells = len(indptr) - 1
    F = int(n_features) if n_features is not None else (int(indices.max()) + 1 if len(indices) else 1)
    if F > _lib.TSNE_MAX_FEATURES:
        raise ValueError("tsne_feature_input: %d features, at most %d" % (F, _lib.TSNE_MAX_FEATURES))
    if len(indices) and int(indices.max()) >= F:
        raise ValueError("tsne_feature_input: feature %d of %d" % (int(indices.max()), F))
    x = np.zeros((n_cells, F))
    cols = np.repeat(np.arange(n_cells, dtype=np.int64), np.diff(indptr))
    x[cols, indices] = np.log2(1 + data)
    return x


def tsne_normalize(x):
    """bh_tsne's input normalisation: every column minus its mean (the left-to-right sum over the rows, divided by their number), then
    everything divided by the largest |x| (an all-zero matrix stays as it is)"""
    x = np.array(x, dtype=np.float64)
    x -= np.cumsum(x, axis=0)[-1] / x.shape[0]
    top = np.abs(x).max()
    return x / top if top > 0 else x


def run_tsne(ctx, matrix, tsne_dims=2, input_pcs=None, perplexity=_lib.TSNE_PERPLEXITY, theta=_lib.TSNE_THETA, max_iter=_lib.TSNE_MAX_ITER,
             stop_lying_iter=_lib.TSNE_STOP_LYING_ITER, mom_switch_iter=_lib.TSNE_MOM_SWITCH_ITER, seed=0, init=None,
             feature_type="Gene Expression", queries_per_call=_lib.NN_QUERIES_PER_CHUNK):
    """RUN_TSNE (stages/analyzer/run_tsne, analysis/bhtsne.py) of a cells x columns f64 matrix, at most 128 columns after input_pcs: the
    stage's rules (perplexity = min(perplexity, max(1, -1 + (N - 1) / 3)); all zeros when N - 1 < 3 * perplexity, without a launch),
    tsne_normalize, Context.knn at K = floor(3 * perplexity) in calls of queries_per_call rows, Context.tsne_affinities, Context.tsne.
    The repulsion is exact: theta is taken for signature parity and IGNORED (0 and the default give the same bits).  The start is
    legacy_randn(seed, N * dims) * 1e-4, row-major, or init [N x dims]; the packages' own generators are not reproduced
    -> dict(embedding f64[N, dims], kl, perplexity_used, name, key, num_neighbors, nnz, max_steps, knn_ms, affinities_ms, loop_ms,
    repulse_ms, pairs_evaluated)"""
    x = np.asarray(matrix, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("run_tsne: the matrix is cells x columns")
    if input_pcs is not None:
        x = x[:, :int(input_pcs)]
    dims = int(tsne_dims)
    if dims not in (2, 3):
        raise ValueError("run_tsne: %d dimensions, 2 or 3" % dims)
    N = x.shape[0]
    perplexity = min(perplexity, max(1, -1 + float(N - 1) / 3))
    out = dict(embedding=np.zeros((N, dims)), kl=0.0, perplexity_used=perplexity, name=get_tsne_name(feature_type, dims),
               key=get_tsne_key(feature_type, dims), num_neighbors=0, nnz=0, max_steps=0, knn_ms=0.0, affinities_ms=0.0, loop_ms=0.0, repulse_ms=0.0,
               pairs_evaluated=0)
    if N - 1 < 3 * perplexity:
        return out
    if x.shape[1] > _lib.TSNE_MAX_FEATURES:
        raise ValueError("run_tsne: %d columns, at most %d" % (x.shape[1], _lib.TSNE_MAX_FEATURES))
    x = np.ascontiguousarray(tsne_normalize(x))
    K = int(3 * perplexity)
    ind, dist = np.zeros((N, K), np.int32), np.zeros((N, K))
    for q0 in range(0, N, int(queries_per_call)):
        r = ctx.knn(x, K, query_start=q0, n_queries=min(int(queries_per_call), N - q0))
        ind[q0:q0 + len(r["indices"])], dist[q0:q0 + len(r["indices"])] = r["indices"], r["distances"]
        out["knn_ms"] += r["fit_ms"]
    P = ctx.tsne_affinities(ind, dist, perplexity)
    if init is None:
        y = (legacy_randn(seed, N * dims) * 1e-4).reshape(N, dims)
    else:
        y = np.array(init, dtype=np.float64)
        if y.shape != (N, dims):
            raise ValueError("run_tsne: init is %d x %d" % (N, dims))
    r = ctx.tsne(P["indptr"], P["indices"], P["values"], y, first_iter=0, n_iters=int(max_iter), max_iter=int(max_iter),
                 stop_lying_iter=int(stop_lying_iter), mom_switch_iter=int(mom_switch_iter))
    out.update(embedding=r["y"], kl=r["kl"], num_neighbors=K, nnz=P["nnz"], max_steps=P["max_steps"], affinities_ms=P["fit_ms"], loop_ms=r["loop_ms"],
               repulse_ms=r["repulse_ms"], pairs_evaluated=r["pairs_evaluated"])
    return out


def get_umap_name(feature_type, n_components):
    """get_tsne_name with EmbeddingType::Umap (cr_ana/src/types.rs): "gene_expression_2-d\""""
    return get_tsne_name(feature_type, n_components)


def get_umap_key(feature_type, n_components):
    """get_tsne_key with EmbeddingType::Umap: the bare number for Gene Expression, else "antibody_capture_2\""""
    return get_tsne_key(feature_type, n_components)


def umap_ab(min_dist=_lib.UMAP_MIN_DIST, spread=_lib.UMAP_SPREAD):
    """umap-learn's find_ab_params (crgpu_umap_ab, host only): the least-squares fit of 1 / (1 + a x^(2b)) to x < min_dist ? 1 :
    exp(-(x - min_dist) / spread) at linspace(0, 3 spread, 300) -> (a, b)"""
    a, b = C.c_double(), C.c_double()
    rc = _lib.load().crgpu_umap_ab(float(min_dist), float(spread), C.byref(a), C.byref(b))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_umap_ab")
    return a.value, b.value


def umap_metric_input(x, metric="correlation"):
    """The rows the neighbour search of RUN_UMAP runs on -> (rows f64[n, d], angular).  correlation / pearson: every row minus its own
    mean (the left-to-right sum over the columns, divided by their number), then divided by its Euclidean norm (the square root of the
    left-to-right sum of squares); cosine: the division alone; a row of norm 0 stays the zero vector; between unit rows ||u - v||^2 =
    2 (1 - corr), so the dissimilarity of a pair is 0.5 * (dist * dist) (angular True).  euclidean: the rows as they are.  Any other
    name: ValueError"""
    if metric not in _lib.UMAP_METRICS:
        raise ValueError("umap_metric_input: the metric %r, one of %s" % (metric, ", ".join(_lib.UMAP_METRICS)))
    x = np.array(x, dtype=np.float64)
    if metric == "euclidean":
        return x, False
    if metric != "cosine":
        x -= (np.cumsum(x, axis=1)[:, -1] / x.shape[1])[:, None]
    norm = np.sqrt(np.cumsum(x * x, axis=1)[:, -1])
    return x / np.where(norm > 0, norm, 1.0)[:, None], True


def umap_rescale(y):
    """umap-learn's rescale of the start: every column to [0, 10] as 10 * (y - min) / (max - min); a constant column becomes 0"""
    y = np.array(y, dtype=np.float64)
    lo, hi = y.min(axis=0), y.max(axis=0)
    span = hi - lo
    return np.where(span > 0, 10.0 * (y - lo) / np.where(span > 0, span, 1.0), 0.0)


def run_umap(ctx, matrix, umap_dims=2, input_pcs=None, n_neighbors=_lib.UMAP_N_NEIGHBORS, min_dist=_lib.UMAP_MIN_DIST, metric="correlation", seed=0,
             n_epochs=None, init=None, feature_type="Gene Expression", queries_per_call=_lib.NN_QUERIES_PER_CHUNK):
    """RUN_UMAP (cr_ana/src/stages/umap.rs) of a cells x columns f64 matrix, at most 128 columns after input_pcs: n_neighbors =
    min(n_neighbors, N - 1), spread 1, umap_metric_input, Context.knn at k = n_neighbors - 1 in calls of queries_per_call rows (the
    point itself is the first of n_neighbors), Context.umap_graph, umap_ab, Context.umap_epochs over all n_epochs (default 500 up to
    10 000 cells, else 200).  The start is init [N x dims] or the first dims columns of the matrix, every column rescaled to [0, 10]
    (umap_rescale); spectral initialisation is not covered.  N < 3: all zeros without a launch
    -> dict(embedding f64[N, dims], a, b, n_epochs, num_neighbors, nnz, max_steps, name, key, knn_ms, graph_ms, loop_ms, n_active,
    n_negative)"""
    x = np.asarray(matrix, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("run_umap: the matrix is cells x columns")
    if input_pcs is not None:
        x = x[:, :int(input_pcs)]
    dims = int(umap_dims)
    if dims not in (2, 3):
        raise ValueError("run_umap: %d dimensions, 2 or 3" % dims)
    if metric not in _lib.UMAP_METRICS:
        raise ValueError("run_umap: the metric %r, one of %s" % (metric, ", ".join(_lib.UMAP_METRICS)))
    N = x.shape[0]
    n_neighbors = min(int(n_neighbors), N - 1)
    n_epochs = (500 if N <= 10000 else 200) if n_epochs is None else int(n_epochs)
    a, b = umap_ab(min_dist, _lib.UMAP_SPREAD)
    out = dict(embedding=np.zeros((N, dims)), a=a, b=b, n_epochs=n_epochs, num_neighbors=max(n_neighbors, 0), nnz=0, max_steps=0,
               name=get_umap_name(feature_type, dims), key=get_umap_key(feature_type, dims), knn_ms=0.0, graph_ms=0.0, loop_ms=0.0, n_active=0,
               n_negative=0)
    if N < 3:
        return out
    if n_neighbors < 2:
        raise ValueError("run_umap: %d neighbours, at least 2 (the point itself is the first)" % n_neighbors)
    if x.shape[1] > _lib.UMAP_MAX_FEATURES:
        raise ValueError("run_umap: %d columns, at most %d" % (x.shape[1], _lib.UMAP_MAX_FEATURES))
    if init is None:
        if x.shape[1] < dims:
            raise ValueError("run_umap: %d columns give no start of %d dimensions" % (x.shape[1], dims))
        y = x[:, :dims]
    else:
        y = np.asarray(init, dtype=np.float64)
        if y.shape != (N, dims):
            raise ValueError("run_umap: init is %d x %d" % (N, dims))
    y = umap_rescale(y)
    rows, angular = umap_metric_input(x, metric)
    rows = np.ascontiguousarray(rows)
    k = n_neighbors - 1
    ind, dist = np.zeros((N, k), np.int32), np.zeros((N, k))
    for q0 in range(0, N, int(queries_per_call)):
        r = ctx.knn(rows, k, query_start=q0, n_queries=min(int(queries_per_call), N - q0))
        ind[q0:q0 + len(r["indices"])], dist[q0:q0 + len(r["indices"])] = r["indices"], r["distances"]
        out["knn_ms"] += r["fit_ms"]
    g = ctx.umap_graph(ind, 0.5 * (dist * dist) if angular else dist, n_epochs)
    r = ctx.umap_epochs(g["indptr"], g["indices"], g["values"], y, a, b, seed=seed, n_epochs=n_epochs)
    out.update(embedding=r["y"], nnz=g["nnz"], max_steps=g["max_steps"], graph_ms=g["fit_ms"], loop_ms=r["loop_ms"], n_active=r["n_active"],
               n_negative=r["n_negative"])
    return out


def mnn_pairs(a, start_i, b, start_j):
    """mutual_nn[(i, j)] of CORRECT_CHEMISTRY_BATCH's join() (crgpu_mnn_pairs, host only): a i32[n_i, k] = the neighbours in batch j (global
    rows, batch j = the rows from start_j) of the rows start_i .. of batch i, b i32[n_j, k] the other direction
    -> (pairs i32[m, 2] in ascending (row of i, row of j) order, distinct rows of i, distinct rows of j)"""
    a, b = np.ascontiguousarray(a, dtype=np.int32), np.ascontiguousarray(b, dtype=np.int32)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("mnn_pairs: two lists of k neighbours per row")
    pairs = np.zeros((a.size, 2), np.int32)
    m, n_first, n_second = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = _lib.load().crgpu_mnn_pairs(ptr(a), a.shape[0], int(start_i), ptr(b), b.shape[0], int(start_j), a.shape[1], ptr(pairs), len(pairs),
                                     C.byref(m), C.byref(n_first), C.byref(n_second))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_mnn_pairs")
    return pairs[:m.value].copy(), int(n_first.value), int(n_second.value)


def batch_effect_score(ctx, projection, batch_ids, knn_neighbors=None, knn_frac=0.01, max_num_bcs=10000):
    """batch_effect_score (analysis/batch_correction.py:20-103): per row the share of its k nearest rows with its own batch id, rescaled so
    that 1 = the batches mix and the number of batches = they are apart; the mean over the rows.  More than max_num_bcs rows are
    subsampled WITH replacement as the reference does (RandomState(0).choice, sorted); NaN when that loses a batch or leaves one with
    fewer than two rows.  k = knn_neighbors or ceil(knn_frac * rows).  The neighbours are Context.knn's (its first-pair drop is the
    reference's knn_idx[:, 1:]); the fractions and the mean are numpy on the host.  k > 1024 or k >= rows: ValueError"""
    if knn_neighbors is None and knn_frac is None:
        raise ValueError("batch_effect_score: one of knn_neighbors or knn_frac")
    x, ids = np.asarray(projection, dtype=np.float64), np.asarray(batch_ids)
    num_bcs = x.shape[0]
    if x.ndim != 2 or ids.shape != (num_bcs,):
        raise ValueError("batch_effect_score: one batch id per row of the cells x PCs projection")
    n_orig = len(np.unique(ids))
    if max_num_bcs is not None and num_bcs > max_num_bcs:
        select = np.random.RandomState(0).choice(num_bcs, max_num_bcs)
        select.sort()
        x, ids, num_bcs = x[select], ids[select], len(select)
    names, inverse, counts = np.unique(ids, return_inverse=True, return_counts=True)
    if len(names) != n_orig or counts.min() < 2:
        return float("nan")
    k = int(knn_neighbors) if knn_neighbors is not None else int(np.ceil(knn_frac * num_bcs))
    if not 1 <= k <= _lib.KNN_MAX_K or k >= num_bcs:
        raise ValueError("batch_effect_score: k = %d, 1 to min(%d, the %d rows - 1)" % (k, _lib.KNN_MAX_K, num_bcs))
    null_frac = np.array([(c - 1) / (num_bcs - 1) for c in counts.tolist()])[inverse]
    max_frac = np.array([min(c - 1, k) / k for c in counts.tolist()])[inverse]
    knn_idx = ctx.knn(np.ascontiguousarray(x), k)["indices"]
    same_frac = np.mean(ids[:, None] == ids[knn_idx], axis=1)
    local = 1 + (len(names) - 1) * (same_frac - null_frac) / (max_frac - null_frac)
    return float(np.mean(local))


def cbc_schedule(ranges, mutual_nn, overlap, alpha=_lib.CBC_ALPHA, realign_panorama=_lib.CBC_REALIGN_PANORAMA):
    """the panorama loop of CORRECT_CHEMISTRY_BATCH's join() as host code that only produces the merge schedule (it depends on the
    overlaps alone, so it is known before any correction).  ranges: per batch its (first row, end row); mutual_nn: {(i, j): i32[m, 2]},
    overlap: {(i, j): float}, both in (i, j) order -> (align_orders, steps); a step = dict(ref_batches, cur_batches, cur_rows i32,
    mnn_cur i32, mnn_ref i32): the pairs in ascending (cur, ref) order"""
    align_orders = [key for key, v in sorted(overlap.items(), key=lambda kv: kv[1], reverse=True) if v > alpha]
    size = lambda pano: sum(ranges[b][1] - ranges[b][0] for b in pano)  # noqa: E731
    panoramas, count, steps = [], collections.defaultdict(int), []
    for i, j in align_orders:
        at = {}
        for idx, pano in enumerate(panoramas):
            for b in (i, j):
                if b in pano:
                    assert b not in at, "batch is found in multiple panorama"
                    at[b] = idx
        for b in (i, j):
            if b not in at:
                panoramas.append({b})
                at[b] = len(panoramas) - 1
        pi, pj = at[i], at[j]
        if realign_panorama:
            count[i] += 1
            count[j] += 1
            if count[i] > 3 and count[j] > 3:
                continue
        elif pi == pj:
            continue
        if size(panoramas[pi]) < size(panoramas[pj]):       # the larger panorama is the reference
            pi, pj = pj, pi
        cur_batches, ref_batches = sorted(panoramas[pj]), sorted(panoramas[pi])
        cur_rows = np.concatenate([np.arange(ranges[b][0], ranges[b][1], dtype=np.int32) for b in cur_batches])
        matches = [np.zeros((0, 2), np.int32)]
        for ref in ref_batches:
            for cur in cur_batches:
                if ref < cur and (ref, cur) in mutual_nn:
                    matches.append(np.asarray(mutual_nn[(ref, cur)], np.int32).reshape(-1, 2)[:, ::-1])
                if ref > cur and (cur, ref) in mutual_nn:
                    matches.append(np.asarray(mutual_nn[(cur, ref)], np.int32).reshape(-1, 2))
        matches = np.concatenate(matches)
        matches = matches[np.lexsort((matches[:, 1], matches[:, 0]))]
        steps.append(dict(ref_batches=ref_batches, cur_batches=cur_batches, cur_rows=cur_rows, mnn_cur=np.ascontiguousarray(matches[:, 0]),
                          mnn_ref=np.ascontiguousarray(matches[:, 1])))
        if pi != pj:
            panoramas[pi].update(panoramas[pj])
            panoramas.pop(pj)
    return align_orders, steps


def correct_chemistry_batch(ctx, projection, batch_ids, knn=_lib.CBC_KNN, alpha=_lib.CBC_ALPHA, sigma=_lib.CBC_SIGMA,
                            realign_panorama=_lib.CBC_REALIGN_PANORAMA, n_batch_ids=None):
    """CORRECT_CHEMISTRY_BATCH (stages/analyzer/correct_chemistry_batch): split()'s reorder (the batches in id order 0 .. n_batch_ids - 1,
    empty ids skipped), one Context.knn_cross per ordered pair of batches, mnn_pairs and the overlap per unordered pair, align_orders,
    the merge schedule (cbc_schedule), ONE Context.batch_correct with that schedule, both scores, the order put back
    -> dict(aligned f64 in the input's row order, batch_score_before, batch_score_after, mutual_nn {(i, j): i32[m, 2]}, overlap,
    align_orders, steps [dict(ref_batches, cur_batches, n_cur, n_mnn)], need_reorder, ranges, knn_ms, mnn_ms, score_ms, correct =
    Context.batch_correct's counters and times).  A batch smaller than knn: ValueError (the reference pairs the wrong rows there)"""
    x, ids = np.ascontiguousarray(projection, dtype=np.float64), np.asarray(batch_ids)
    if x.ndim != 2 or ids.shape != (x.shape[0],) or not np.issubdtype(ids.dtype, np.integer):
        raise ValueError("correct_chemistry_batch: one integer batch id per row of the cells x PCs projection")
    nb = int(ids.max()) + 1 if n_batch_ids is None else int(n_batch_ids)
    if ids.min() < 0 or ids.max() >= nb:
        raise ValueError("correct_chemistry_batch: batch ids 0 .. %d" % (nb - 1))
    order, ranges, reordered_ids, base = [], [], [], 0
    for b_id in range(nb):
        rows = np.where(ids == b_id)[0]
        if len(rows) == 0:
            continue
        if len(rows) < knn:
            raise ValueError("correct_chemistry_batch: batch %d has %d rows, fewer than knn = %d" % (b_id, len(rows), knn))
        order.append(rows)
        ranges.append((base, base + len(rows)))
        reordered_ids.append(np.full(len(rows), b_id, ids.dtype))
        base += len(rows)
    order, idx_to_batch_id = np.concatenate(order), np.concatenate(reordered_ids)
    need_reorder = not bool(np.all(np.diff(order) >= 0))
    if need_reorder:
        x = np.ascontiguousarray(x[order])
    t0 = time.perf_counter()
    score_before = batch_effect_score(ctx, x, idx_to_batch_id)
    score_ms = (time.perf_counter() - t0) * 1e3
    nn, knn_ms = {}, 0.0
    for i, (lo_i, hi_i) in enumerate(ranges):
        for j, (lo_j, hi_j) in enumerate(ranges):
            if i != j:
                r = ctx.knn_cross(x, knn, lo_i, hi_i - lo_i, lo_j, hi_j - lo_j)
                nn[(i, j)] = r["indices"]
                knn_ms += r["fit_ms"]
    t0 = time.perf_counter()
    mutual_nn, overlap = collections.OrderedDict(), collections.OrderedDict()
    for i in range(len(ranges)):
        for j in range(i + 1, len(ranges)):
            pairs, n_first, n_second = mnn_pairs(nn[(i, j)], ranges[i][0], nn[(j, i)], ranges[j][0])
            mutual_nn[(i, j)] = pairs
            overlap[(i, j)] = max(float(n_first) / (ranges[i][1] - ranges[i][0]), float(n_second) / (ranges[j][1] - ranges[j][0]))
    align_orders, steps = cbc_schedule(ranges, mutual_nn, overlap, alpha, realign_panorama)
    mnn_ms = (time.perf_counter() - t0) * 1e3
    res = ctx.batch_correct(x, steps, sigma)
    aligned = res.pop("aligned")
    t0 = time.perf_counter()
    score_after = batch_effect_score(ctx, aligned, idx_to_batch_id)
    score_ms += (time.perf_counter() - t0) * 1e3
    if need_reorder:
        aligned = aligned[np.argsort(order)]
    return dict(aligned=aligned, batch_score_before=score_before, batch_score_after=score_after, mutual_nn=mutual_nn, overlap=overlap,
                align_orders=align_orders, steps=[dict(ref_batches=s["ref_batches"], cur_batches=s["cur_batches"], n_cur=len(s["cur_rows"]),
                                                       n_mnn=len(s["mnn_cur"])) for s in steps],
                need_reorder=need_reorder, ranges=ranges, knn_ms=knn_ms, mnn_ms=mnn_ms, score_ms=score_ms, correct=res)


def sseq_adjust_bh(p):
    """adjust_pvalue_bh (crgpu_sseq_adjust_bh, host only): Benjamini-Hochberg adjusted p-values in the order of p"""
    p = np.ascontiguousarray(p, dtype=np.float64)
    q = np.zeros(len(p))
    rc = _lib.load().crgpu_sseq_adjust_bh(ptr(p), len(p), ptr(q))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_sseq_adjust_bh")
    return q


def differential_expression_header(n_clusters, cluster_names=None):
    """the header of differential_expression.csv as save_differential_expression_csv writes it: two feature columns, then three per
    cluster (cluster_names: the perturbation names of MEASURE_PERTURBATIONS' tables)"""
    header = ["Feature ID", "Feature Name"]
    for i in range(n_clusters):
        if cluster_names is None:
            header += ["Cluster %d Mean Counts" % (i + 1), "Cluster %d Log2 fold change" % (i + 1), "Cluster %d Adjusted p value" % (i + 1)]
        else:
            header += ["Perturbation %s, Mean Counts" % cluster_names[i], "Perturbation %s, Log2 fold change" % cluster_names[i],
                       "Perturbation %s, Adjusted p value" % cluster_names[i]]
    return header


def run_differential_expression(ctx, m, clusterings, params=None, n_features=None):
    """RUN_DIFFERENTIAL_EXPRESSION for one library type: m = the filtered MatrixDev restricted to that type's rows
    (Context.select_features_dev); clusterings = {key: clusters i32[cells], 1-based} or engine.run_kmeans's dict.  The sSeq parameters
    are computed once (or taken from params) -> {key: f64[G, 3 K]}, per cluster norm_mean_a, log2_fold_change, adjusted_p_value"""
    own = params is None
    if own:
        params = ctx.sseq_params(m, n_features=n_features)
    try:
        out = {}
        for key, clusters in clusterings.items():
            if isinstance(clusters, dict):
                clusters = clusters["clusters"]
            out[key] = ctx.sseq_diffexp(m, params, clusters)["data"]
        return out
    finally:
        if own:
            params.free()


def call_protospacers(ctx, filtered, guide_rows, n_features=None, report_prefix="CRISPR_"):
    """GuideAssigner on the filtered MatrixDev: guide_rows = the feature rows of the CRISPR Guide Capture library (ascending); a cell
    needs at least 3 UMIs of a guide.  -> dict(calls = MarginalCalls, metadata, metrics = the three frac_cells_with_*protospacer
    values, summary = the integers and percentages of the four fixed rows of protospacer_calls_summary, umi_thresholds)"""
    mc = ctx.marginal_calls(filtered, guide_rows, umi_threshold=GUIDE_UMI_THRESHOLD, n_features=n_features)
    md = mc.metadata()
    metrics = {report_prefix + "frac_cells_with_protospacer": md["frac_singlets"] + md["frac_multiplets"],
               report_prefix + "frac_cells_with_single_protospacer": md["frac_singlets"],
               report_prefix + "frac_cells_with_multiple_protospacer": md["frac_multiplets"]}
    summary = {"No guide molecules": (md["num_cells_without_feature_umis"], 100 * md["frac_cells_without_feature_umis"]),
               "No confident call": (md["num_cells_without_features"], 100 * md["frac_cells_without_features"]),
               "1 protospacer assigned": (md["num_singlets"], 100 * md["frac_singlets"]),
               "More than 1 protospacer assigned": (md["num_multiplets"], 100 * md["frac_multiplets"])}
    return dict(calls=mc, metadata=md, metrics=metrics, summary=summary, umi_thresholds=mc.umi_thresholds())


# ---- MEASURE_PERTURBATIONS (stages/feature/measure_perturbations, cellranger/feature/crispr/measure_perturbations.py) ----------------
PERTURBATION_FILTER_LIST = ("None", "Non-Targeting", "Ignore")      # cellranger.constants.FILTER_LIST
PERTURBATION_CONTROL_LIST = ("Non-Targeting",)
MIN_NUMBER_CELLS_PER_PERTURBATION = 10
MIN_COUNTS_PERTURBATION = MIN_COUNTS_CONTROL = 5
NUM_TOP_GENES = 10
PERTURBATION_EFFICIENCY_SUMMARY_COLUMNS = ("Perturbation", "target_string", "Log2 Fold Change", "p Value", "Log2 Fold Change Lower Bound",
                                           "Log2 Fold Change Upper Bound", "Cells with Perturbation", "Mean UMI Count Among Cells with Perturbation",
                                           "Cells with Non-Targeting Guides", "Mean UMI Count Among Cells with Non-Targeting Guides")
TOP_GENES_SUMMARY_COLUMNS = ("Gene Name", "Gene ID", "Log2 Fold Change", "Adjusted p-value")


def _str(x):
    return x.decode() if isinstance(x, bytes) else str(x)


def perturbation_target_info(feature_ref):
    """_get_target_info: feature_ref = the rows of the feature reference as dicts (id, target_gene_id, optional target_gene_name)
    -> {feature id: dict(target_id, target_name)}; a row without a name takes its target id"""
    info = {}
    for row in feature_ref:
        tid = row["target_gene_id"]
        info[row["id"]] = dict(target_id=tid, target_name=row.get("target_gene_name", tid))
    return info


def protospacer_calls(marginal_calls, guide_ids, barcodes):
    """The `calls` of perturbation_clusters from a MarginalCalls (call_protospacers' `calls`): {barcode: (the ids of the guides assigned
    to the cell joined by "|" in row order, their number)} for the cells with a guide, as protospacer_calls_per_cell.csv lists them"""
    indptr, cols = marginal_calls.assignments()
    per_cell = collections.defaultdict(list)
    for p in range(marginal_calls.n_rows):
        for c in cols[indptr[p]:indptr[p + 1]]:
            per_cell[int(c)].append(_str(guide_ids[p]))
    return {_str(barcodes[c]): ("|".join(f), len(f)) for c, f in sorted(per_cell.items())}


def perturbation_clusters(feature_ref, calls, barcodes, by_feature=False, ignore_multiples=False):
    """_get_ps_clusters, statement by statement (_get_bc_targets_dict, _add_bcs_without_ps_calls, _get_ps_clusters_by_target /
    _by_feature, _get_feature_from_bc): calls = {barcode: (feature_call "A|B", num_features)} for the cells with a call
    -> (cluster_per_bc i64[barcodes], 1-based; {cluster: perturbation name}).  The names are sorted to number the clusters; a
    multi-guide cell whose targets are all Non-Targeting is a control cell; "None", "Non-Targeting" and "Ignore" are taken out of a
    multi-guide cell's targets; "Ignore" holds the ignored multiples and, by feature, the cells without a call as well.
    DEVIATION: the reference joins list(set(targets)), whose order depends on the process's hash seed; here the targets are joined
    in sorted order"""
    info = perturbation_target_info(feature_ref)
    bc_targets = {}
    for bc, (feature_call, num_features) in calls.items():
        if feature_call in info:
            tid, tname = info[feature_call]["target_id"], info[feature_call]["target_name"]
        else:
            tid = tname = feature_call
        if num_features > 1:
            if ignore_multiples:
                tid = tname = "Ignore"
            else:
                feats = feature_call.split("|")
                tids, tnames = [info[x]["target_id"] for x in feats], [info[x]["target_name"] for x in feats]
                if set(tids) == set(PERTURBATION_CONTROL_LIST):
                    tid = tname = "Non-Targeting"
                else:
                    tids = sorted(set(tids).difference(PERTURBATION_FILTER_LIST))
                    tnames = sorted(set(tnames).difference(PERTURBATION_FILTER_LIST))
                    if tids:
                        tid, tname = "|".join(tids), "|".join(tnames)
                    else:
                        tid = tname = "Ignore"
        bc_targets[_str(bc)] = dict(num_features=num_features, feature_call=feature_call, target_id=tid, target_name=tname)
    bcs = [_str(bc) for bc in barcodes]
    for bc in bcs:
        if bc not in bc_targets:
            bc_targets[bc] = dict(target_name="None", num_features=-1, target_id="None", feature_call="None")
    if not by_feature:
        id_name = {v["target_id"]: v["target_name"] for v in info.values()}
        per_bc = [bc_targets[bc]["target_id"] for bc in bcs]
        number = {el: i + 1 for i, el in enumerate(sorted(set(per_bc)))}
        names = {b: "|".join(id_name.get(x, x) for x in a.split("|")) for a, b in number.items()}
    else:
        def feature_of(t):
            if t["target_id"] not in PERTURBATION_FILTER_LIST:
                return t["feature_call"]
            return "Ignore" if t["target_id"] == "None" else t["target_id"]

        per_bc = [feature_of(bc_targets[bc]) for bc in bcs]
        number = {el: i + 1 for i, el in enumerate(sorted(set(per_bc)))}
        names = {b: a for a, b in number.items()}
    return np.asarray([number[x] for x in per_bc], dtype=np.int64), names


def perturbation_ci(sums_a, sums_b, s_a, s_b, ci_lower=5.0, ci_upper=95.0):
    """crgpu_perturbation_ci (host only): per draw log2((1 + A) / (1 + s_a)) - log2((1 + B) / (1 + s_b)), then np.percentile at the two
    bounds -> (lower, upper, log2fc f64[B]).  s_a, s_b: the sums of the size factors of the ORIGINAL cells (SseqPairs.compare's), as
    _get_fold_change_cis takes them, not of the resampled cells"""
    A, B = np.ascontiguousarray(sums_a, dtype=np.uint64).reshape(-1), np.ascontiguousarray(sums_b, dtype=np.uint64).reshape(-1)
    if len(A) != len(B):
        raise ValueError("perturbation_ci: one sum per draw and side")
    fc = np.zeros(len(A))
    lo, hi = C.c_double(0.0), C.c_double(0.0)
    rc = _lib.load().crgpu_perturbation_ci(ptr(A), ptr(B), len(A), float(s_a), float(s_b), float(ci_lower), float(ci_upper), ptr(fc), C.byref(lo), C.byref(hi))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_perturbation_ci")
    return lo.value, hi.value, fc


def top_perturbed_genes(result, gene_ids, gene_names, num_genes=NUM_TOP_GENES):
    """sanitize_perturbation_results on one pair's vectors: keep sum_b > 0, keep sum_a >= 5 or sum_b >= 5, order by (|log2 fold change|
    descending, adjusted p, gene name) -> the first num_genes rows as (gene name, gene id, log2 fold change, adjusted p).  (The
    reference's save_top_perturbed_genes slices the COLUMN list with its num_genes_to_keep, so its CSV keeps every row.)"""
    sa, sb = np.asarray(result["sums_a"]), np.asarray(result["sums_b"])
    keep = np.flatnonzero((sb > 0) & ((sa >= MIN_COUNTS_PERTURBATION) | (sb >= MIN_COUNTS_CONTROL)))
    names = np.array([_str(gene_names[g]) for g in keep], dtype=object)
    name_rank = np.unique(names, return_inverse=True)[1] if len(keep) else np.zeros(0, np.int64)
    fc, adj = result["log2_fold_change"][keep], result["adjusted_p_values"][keep]
    order = np.lexsort((name_rank, adj, -np.abs(fc)))[:num_genes]
    return [(_str(gene_names[keep[i]]), _str(gene_ids[keep[i]]), float(fc[i]), float(adj[i])) for i in order]


def measure_perturbations(ctx, m, gene_ids, gene_names, feature_ref, calls, barcodes, by_feature=False, ignore_multiples=False, num_bootstraps=500,
                          seed=0, ci=(5.0, 95.0)):
    """MEASURE_PERTURBATIONS (join() of the stage, get_perturbation_efficiency, _analyze_transcriptome, _get_log2_fold_change): m = the
    filtered MatrixDev restricted to the Gene Expression rows (Context.select_features_dev), gene_ids / gene_names = its rows,
    feature_ref / calls / barcodes as perturbation_clusters.  None where the reference writes nothing: a feature reference without
    target_gene_id or without a Non-Targeting target, no Non-Targeting cell.  A perturbation is tested when its name is not in the
    filter list, not all of its targets are, and it has at least 10 cells.  ONE plan (Context.sseq_pairs): the tested perturbations
    and the control are its groups, every other cell is in none; SseqPairs.compare([p], [control]) per perturbation; ONE
    SseqPairs.bootstrap for all (perturbation, target) items, stream = the item's ordinal; perturbation_ci per item.
    -> dict(log2_fold_change {name: {target: (log2 fc, p, sum_a, sum_b)}}, log2_fold_change_ci {name: {target: (lower, upper)}},
    num_cells_per_perturbation, results_per_perturbation {name: the pair's dict}, results_all_perturbations f64[G, 3 k] (sum_a /
    cells -- raw, not normalised, as the reference --, log2 fold change, adjusted p), cluster_names, summary (the rows of
    construct_perturbation_efficiency_summary, ascending by log2 fold change, the UNADJUSTED p), summary_columns,
    top_perturbed_genes {name: rows}, items, cluster_per_bc, perturbation_keys, plan_ms, pairs_ms, bootstrap_ms, ci_ms, total_ms)"""
    t_all = time.perf_counter()
    feature_ref = list(feature_ref)
    if any("target_gene_id" not in row for row in feature_ref) or "Non-Targeting" not in [row["target_gene_id"] for row in feature_ref]:
        return None
    gene_ids, gene_names = [_str(g) for g in gene_ids], [_str(g) for g in gene_names]
    G = len(gene_ids)
    info = perturbation_target_info(feature_ref)
    if by_feature:
        id_of_name = {x: info[x]["target_id"] for x in info}
    else:
        id_of_name = {info[x]["target_name"]: info[x]["target_id"] for x in info}
    cluster_per_bc, keys = perturbation_clusters(feature_ref, calls, barcodes, by_feature, ignore_multiples)
    if len(cluster_per_bc) != m.n_barcodes:
        raise ValueError("measure_perturbations: one barcode per column of the matrix")
    num_cells = {name: int(np.sum(cluster_per_bc == cluster)) for cluster, name in keys.items()}
    nt = [c for c in keys if keys[c] == "Non-Targeting"]
    if not nt:
        return None
    tested = []     # (cluster, name, target names, target ids)
    for cluster, name in keys.items():
        if name in PERTURBATION_FILTER_LIST:
            continue
        t_names = name.split("|")
        t_ids = [id_of_name[p] for p in t_names]
        if all(x in PERTURBATION_FILTER_LIST for x in t_ids) or int(np.sum(cluster_per_bc == cluster)) < MIN_NUMBER_CELLS_PER_PERTURBATION:
            continue
        tested.append((cluster, name, t_names, t_ids))
    T = len(tested)
    if T > _lib.SSEQ_MAX_K - 1:
        raise ValueError("measure_perturbations: %d tested perturbations, one plan holds at most %d and the control" % (T, _lib.SSEQ_MAX_K - 1))
    times = dict(plan_ms=0.0, pairs_ms=0.0, bootstrap_ms=0.0, ci_ms=0.0)
    fold_change, fold_change_ci, per_perturbation = {}, {}, collections.OrderedDict()
    all_de = np.zeros((G, 3 * T))
    items, item_keys = [], []
    if T:
        groups = np.full(len(cluster_per_bc), -1, np.int32)
        for j, (cluster, _, _, _) in enumerate(tested):
            groups[cluster_per_bc == cluster] = j
        groups[cluster_per_bc == nt[0]] = T
        t0 = time.perf_counter()
        pairs = ctx.sseq_pairs(m, groups, n_groups=T + 1, n_features=G)
        times["plan_ms"] = (time.perf_counter() - t0) * 1e3
        try:
            t0 = time.perf_counter()
            for j, (cluster, name, t_names, t_ids) in enumerate(tested):
                r = pairs.compare([j], [T])
                per_perturbation[name] = r
                all_de[:, 3 * j] = r["sums_a"] / float(r["n_cells_a"])
                all_de[:, 3 * j + 1], all_de[:, 3 * j + 2] = r["log2_fold_change"], r["adjusted_p_values"]
                fold_change[name], fold_change_ci[name] = {}, {}
                for t_name, target in zip(t_names, t_ids):
                    if target in PERTURBATION_FILTER_LIST or target not in gene_ids:      # _get_ko_per_target: no such gene
                        continue
                    g = gene_ids.index(target)
                    fold_change[name][t_name] = (float(r["log2_fold_change"][g]), float(r["p_values"][g]), int(r["sums_a"][g]), int(r["sums_b"][g]))
                    items.append((g, j, T, len(items)))
                    item_keys.append((name, t_name))
            times["pairs_ms"] = (time.perf_counter() - t0) * 1e3
            if items:
                t0 = time.perf_counter()
                sums_a, sums_b = pairs.bootstrap(items, n_bootstraps=num_bootstraps, seed=seed)
                times["bootstrap_ms"] = (time.perf_counter() - t0) * 1e3
                t0 = time.perf_counter()
                for i, (name, t_name) in enumerate(item_keys):
                    r = per_perturbation[name]
                    lo, hi, _ = perturbation_ci(sums_a[i], sums_b[i], r["s_a"], r["s_b"], ci[0], ci[1])
                    fold_change_ci[name][t_name] = (lo, hi)
                times["ci_ms"] = (time.perf_counter() - t0) * 1e3
        finally:
            pairs.free()
    columns = list(PERTURBATION_EFFICIENCY_SUMMARY_COLUMNS)
    columns[1] = "Target Guide" if by_feature else "Target Gene"
    control_cells = num_cells["Non-Targeting"]
    rows = []
    for key in sorted(fold_change):
        n = num_cells[key]
        for ps, res in fold_change[key].items():
            lo, hi = fold_change_ci[key][ps]
            rows.append((key, ps, res[0], res[1], lo, hi, n, _robust_divide(res[2], n), control_cells, _robust_divide(res[3], control_cells)))
    rows.sort(key=lambda row: row[2])      # a stable sort; pandas' default breaks ties in no stated order
    top = {name: top_perturbed_genes(r, gene_ids, gene_names) for name, r in per_perturbation.items()}
    out = dict(log2_fold_change=fold_change, log2_fold_change_ci=fold_change_ci, num_cells_per_perturbation=num_cells,
               results_per_perturbation=per_perturbation, results_all_perturbations=all_de, cluster_names=[t[1] for t in tested], summary=rows,
               summary_columns=columns, top_perturbed_genes=top, items=items, cluster_per_bc=cluster_per_bc, perturbation_keys=keys)
    out.update(times, total_ms=(time.perf_counter() - t_all) * 1e3)
    return out


def write_perturbation_efficiencies_csv(path, result):
    """perturbation_efficiencies.csv as the stage's join() writes it: the summary rows under their columns"""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(result["summary_columns"])
        for row in result["summary"]:
            w.writerow(list(row))


def write_transcriptome_analysis_csv(path, result, gene_ids, gene_names):
    """transcriptome_analysis.csv (save_differential_expression_csv with cluster_names): per gene its id, its name and per tested
    perturbation the mean counts, the log2 fold change and the adjusted p value"""
    header = differential_expression_header(len(result["cluster_names"]), result["cluster_names"])
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(header)
        for g, row in enumerate(result["results_all_perturbations"].tolist()):
            w.writerow([_str(gene_ids[g]), _str(gene_names[g])] + row)


def write_top_perturbed_genes_csv(path, result):
    """top_perturbed_genes.csv: per tested perturbation four columns "Perturbation: <name>, <column>", the rows of top_perturbed_genes"""
    names = [n for n, rows in result["top_perturbed_genes"].items() if rows]
    header = ["Perturbation: %s, %s" % (n, c) for n in names for c in TOP_GENES_SUMMARY_COLUMNS]
    depth = max([len(result["top_perturbed_genes"][n]) for n in names] or [0])
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(header)
        for i in range(depth):
            row = []
            for n in names:
                rows = result["top_perturbed_genes"][n]
                row += list(rows[i]) if i < len(rows) else [""] * 4
            w.writerow(row)


def call_antibodies(ctx, filtered, rows, ids, n_features=None, feature_bc_name="antibody", report_prefix="ANTIBODY_"):
    """AntibodyOrAntigenAssigner on the filtered MatrixDev: rows / ids = the feature rows of the library (ascending) and their ids.
    The reference calls only CD3, CD19 and CD14, and of those only a feature with at least 1000 UMIs: the host picks the rows (a
    first call gives the totals, a second one the fits of the rows that remain).  -> dict(calls = MarginalCalls over `called_rows`
    or None, called_rows, called_ids, metadata, metrics, umi_thresholds)"""
    ids = [i if isinstance(i, bytes) else str(i).encode() for i in ids]
    rows = np.asarray(rows, np.uint32)
    pick = [k for k, i in enumerate(ids) if i in ANTIBODY_ASSIGNMENT_LIST]
    mc = None
    if pick:
        first = ctx.marginal_calls(filtered, rows[pick], n_features=n_features)
        keep = [k for j, k in enumerate(pick) if first.per_feature["total_umis"][j] >= MIN_COUNTS_PER_ANTIBODY]
        if len(keep) == len(pick):
            mc = first
        else:
            first.free()
            pick = keep
            mc = ctx.marginal_calls(filtered, rows[pick], n_features=n_features) if pick else None
    all_rows = ctx.marginal_calls(filtered, rows, n_features=n_features) if mc is None or len(pick) != len(rows) else mc
    without = all_rows.cells_without_umis      # get_num_cells_without_molecules: over the whole library
    if all_rows is not mc:
        all_rows.free()
    md = assignment_metadata(filtered.n_barcodes, mc.cells_with_1 if mc else 0, mc.cells_with_many if mc else 0, without)
    metrics = {report_prefix + "frac_cells_with_" + feature_bc_name: md["frac_singlets"] + md["frac_multiplets"],
               report_prefix + "frac_cells_with_single_" + feature_bc_name: md["frac_singlets"],
               report_prefix + "frac_cells_with_multiple_" + feature_bc_name: md["frac_multiplets"]}
    return dict(calls=mc, called_rows=rows[pick], called_ids=[ids[k] for k in pick], metadata=md, metrics=metrics,
                umi_thresholds=mc.umi_thresholds() if mc else {})


def umi_interval_snr(values, counts, threshold):
    """_get_umi_interval + the log10_snr column (feature_assigner.py:470-474, 492-505) on a histogram: np.percentile over the counts
    the histogram stands for, rounded to 3 places"""
    dense = np.repeat(np.asarray(values, np.int64), np.asarray(counts, np.int64))
    noise, signal = dense[dense < threshold], dense[dense >= threshold]
    q3 = np.percentile(noise, 75) if len(noise) else 0
    q1 = np.percentile(signal, 25) if len(signal) else 0
    return float(np.round(np.log10(q1 + 1) - np.log10(q3 + 1), 3))


def call_tags_marginal(ctx, filtered, tag_rows, tag_ids, n_features=None):
    """TagAssigner (CALL_TAGS_MARGINAL) on the filtered MatrixDev: tag_rows = the feature rows of the Multiplexing Capture library
    (ascending), tag_ids their ids.  -> dict(calls = MarginalCalls over all tag rows, flags u8 per tag (0 kept, 1 contaminant, 2
    dropped for zero UMIs), source_tags (per tag the ids it correlates with), log10_snr per tag (NaN without a call), umi_thresholds,
    features_per_cell u32[V] over the tags that are not contaminants, metadata, nlet_observed i64[15] (cells with 0 .. 14 tags),
    valid_tags bool per tag and prelim_calls i32[V]: what engine.call_tags_jibes takes)."""
    ids = [i if isinstance(i, bytes) else str(i).encode() for i in tag_ids]
    k = len(ids)
    mc = ctx.marginal_calls(filtered, tag_rows, n_features=n_features, want_histograms=True)
    sx, sxx, sxy = ctx.tag_moments(filtered, tag_rows, n_features=n_features)
    order = np.array(sorted(range(k), key=lambda t: ids[t]), np.uint32)
    flags, src = tag_contaminants(sx, sxx, sxy, filtered.n_barcodes, order)
    indptr, cols = mc.assignments()
    V = filtered.n_barcodes
    thr = mc.per_feature["umi_threshold_observed"]
    snr = np.full(k, np.nan)
    for t in range(k):
        if flags[t] != 2 and indptr[t + 1] > indptr[t]:
            snr[t] = umi_interval_snr(*mc.histogram(t), int(thr[t]))
    good = [t for t in range(k) if flags[t] == 0]
    fpc = np.zeros(V, np.uint32)
    for t in good:
        np.add.at(fpc, cols[indptr[t]:indptr[t + 1]], 1)
    md = assignment_metadata(V, int((fpc == 1).sum()), int((fpc > 1).sum()), mc.cells_without_umis)
    nlet = np.bincount(np.minimum(fpc, NUM_TOTAL_TAGS + 1), minlength=NUM_TOTAL_TAGS + 2)[:NUM_TOTAL_TAGS + 1].astype(np.int64)
    valid = np.array([flags[t] == 0 and indptr[t + 1] > indptr[t] for t in range(k)], bool)
    place = np.cumsum(valid) - 1
    prelim = np.full(V, -1, np.int32)
    for t in np.flatnonzero(valid):
        c = cols[indptr[t]:indptr[t + 1]]
        c = c[fpc[c] == 1]
        prelim[c] = place[t]
    return dict(calls=mc, flags=flags, source_tags=[[ids[j] for j in s] for s in src], log10_snr=snr,
                umi_thresholds={t: int(thr[t]) for t in range(k) if flags[t] != 2 and indptr[t + 1] > indptr[t]}, features_per_cell=fpc,
                metadata=md, nlet_observed=nlet, valid_tags=valid, prelim_calls=prelim)


def ordmag_candidates(max_expected_cells=1 << 18):
    """the recovered-cells grid of estimate_recovered_cells_ordmag (cell_calling_helpers.py:879-880); host only"""
    out, n = np.zeros(2000, np.int64), C.c_uint32()
    rc = _lib.load().crgpu_ordmag_candidates(max_expected_cells, ptr(out), len(out), C.byref(n))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_ordmag_candidates")
    return out[: n.value].copy()


def subsample_plan(subsample_type, lib_indices, num_cells_per_lib, raw_reads_per_lib, usable_reads_per_lib, fixed_depths=None,
                   num_additional_depths=_lib.SS_NUM_ADDITIONAL_DEPTHS):
    """make_subsamplings (subsample.py:140-309) through the C ABI, host only: (depths int64[n], rates float64[n][n_libs]) for
    the libraries `lib_indices` of one library type.  subsample_type: _lib.SS_PLAN_*; for SS_PLAN_BULK usable_reads_per_lib are
    the transcriptomic reads.  fixed_depths None: the reference's list for the type (bulk / all others)."""
    if fixed_depths is None:
        fixed_depths = _lib.SS_BULK_FIXED_DEPTHS if subsample_type == _lib.SS_PLAN_BULK else _lib.SS_FIXED_DEPTHS
    idx = np.ascontiguousarray(lib_indices, dtype=np.uint32)
    cells, raw, usable = (np.ascontiguousarray(x, dtype=np.float64) for x in (num_cells_per_lib, raw_reads_per_lib, usable_reads_per_lib))
    assert len(cells) == len(raw) == len(usable)
    fixed = np.ascontiguousarray(fixed_depths, dtype=np.int64)
    cap = len(fixed) + int(num_additional_depths) + 1
    depths, rates, n = np.zeros(cap, np.int64), np.zeros((cap, len(cells)), np.float64), C.c_uint32()
    rc = _lib.load().crgpu_subsample_plan(int(subsample_type), ptr(idx), len(idx), len(cells), ptr(cells), ptr(raw), ptr(usable), ptr(fixed),
                                          len(fixed), int(num_additional_depths), ptr(depths), ptr(rates), cap, C.byref(n))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_subsample_plan")
    return depths[: n.value].copy(), rates[: n.value].copy()


def subsample_summary(data, task_types, cell_genome_mask=None):
    """the per-task, per-genome numbers of calculate_subsampling_metrics (subsample.py:719-845) from the dict Counts.subsample
    returns: (table float64[task][genome][len(_lib.SS_SUMMARY_COLS)], whole-dataset duplication fraction float64[task])"""
    upb, rpb, fpb = (np.ascontiguousarray(data[k], dtype=np.int64) for k in ("umis_per_bc", "read_pairs_per_bc", "features_det_per_bc"))
    rp, um, tfd = (np.ascontiguousarray(data[k], dtype=np.int64) for k in ("read_pairs", "umis", "total_features_det"))
    T, G, NC = upb.shape
    types = np.ascontiguousarray(task_types, dtype=np.uint8)
    assert len(types) == T
    cgm = None if cell_genome_mask is None else np.ascontiguousarray(cell_genome_mask, dtype=np.uint32)
    out, allf = np.zeros((T, G, len(_lib.SS_SUMMARY_COLS)), np.float64), np.zeros(T, np.float64)
    rc = _lib.load().crgpu_subsample_summary(T, G, NC, tfd.shape[2], ptr(types), ptr(cgm), ptr(upb), ptr(rpb), ptr(fpb), ptr(rp), ptr(um),
                                             ptr(tfd), ptr(out), ptr(allf))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_subsample_summary")
    return out, allf


def normalize_depth_plan(library_type, usable_reads, num_cells, downsample=True, targeted_aggr=False, is_targeted_lib=None,
                         targeted_depth_factor=1.0):
    """frac_reads_kept float64[n_libs] of NORMALIZE_DEPTH's split() (normalize_depth/__init__.py:139-176) through the C ABI, host
    only.  library_type: a small integer id per library; usable_reads, num_cells: per library; downsample False: all ones;
    targeted_aggr: _adjust_frac_kept with the libraries marked in is_targeted_lib and targeted_depth_factor."""
    types = np.ascontiguousarray(library_type, dtype=np.uint32)
    usable, cells = (np.ascontiguousarray(x, dtype=np.float64) for x in (usable_reads, num_cells))
    tg = None if is_targeted_lib is None else np.ascontiguousarray(np.asarray(is_targeted_lib) != 0, dtype=np.uint8)
    assert len(types) == len(usable) == len(cells) and (tg is None or len(tg) == len(types))
    frac = np.zeros(len(types), np.float64)
    rc = _lib.load().crgpu_normalize_depth_plan(len(types), ptr(types), ptr(usable), ptr(cells), int(bool(downsample)), int(bool(targeted_aggr)),
                                                ptr(tg), float(targeted_depth_factor), ptr(frac))
    if rc != 0:
        raise _lib.CrgpuError(rc, "crgpu_normalize_depth_plan")
    return frac


class NormalizedDepth:
    """Result of Counts.normalize_depth: `matrix` (MatrixDev: the raw UMI matrix after the draw, over the context's BarcodeIndex),
    `raw_mapped_reads` / `flt_mapped_reads` int64[n_classes], `reads_per_lib` / `kept_reads_per_lib` / `kept_molecules_per_lib`
    int64[n_libs], `kept` (uint32 per molecule in table order, or None) and `result` (crgpu_normalize_depth_result as a dict)."""

    def __init__(self, matrix, sums, kept, result):
        self.matrix, self.kept, self.result = matrix, kept, result
        for k, v in sums.items():
            setattr(self, k, v)


class Counts:
    """crgpu_counts: sorted (barcode, feature, count) triplets + the molecule table."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle
        nt, nm = C.c_uint64(), C.c_uint64()
        ctx._check(ctx.L.crgpu_counts_info(ctx.h, handle, C.byref(nt), C.byref(nm)))
        self.n_triplets, self.n_molecules = nt.value, nm.value

    def triplets(self):
        n = self.n_triplets
        bc, ft, ct = (np.zeros(n, np.uint32) for _ in range(3))
        if n:
            self.ctx._check(self.ctx.L.crgpu_counts_triplets(self.ctx.h, self.h, ptr(bc), ptr(ft), ptr(ct)))
        return bc, ft, ct

    def triplets_dev(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self.ctx._check(self.ctx.L.crgpu_counts_triplets_dev(self.ctx.h, self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def molecules(self):
        n = self.n_molecules
        out = dict(bc=np.zeros(n, np.uint32), lib=np.zeros(n, np.uint8), feature=np.zeros(n, np.uint32),
                   umi=np.zeros(n, np.uint32), read_count=np.zeros(n, np.uint32), utype=np.zeros(n, np.uint8))
        if n:
            self.ctx._check(self.ctx.L.crgpu_counts_molecules(self.ctx.h, self.h, ptr(out["bc"]), ptr(out["lib"]),
                                                              ptr(out["feature"]), ptr(out["umi"]),
                                                              ptr(out["read_count"]), ptr(out["utype"])))
        return out

    def molecule_info(self, gem_group=1):
        """the datasets MoleculeInfoWriter::fill appends (cr_h5/src/molecule_info.rs:972-998)"""
        n = self.n_molecules
        out = dict(gem_group=np.zeros(n, np.uint16), barcode_idx=np.zeros(n, np.uint64), feature_idx=np.zeros(n, np.uint32),
                   library_idx=np.zeros(n, np.uint16), umi=np.zeros(n, np.uint32), count=np.zeros(n, np.uint32),
                   umi_type=np.zeros(n, np.uint32))
        if n:
            self.ctx._check(self.ctx.L.crgpu_counts_molecule_info(
                self.ctx.h, self.h, gem_group, ptr(out["gem_group"]), ptr(out["barcode_idx"]), ptr(out["feature_idx"]),
                ptr(out["library_idx"]), ptr(out["umi"]), ptr(out["count"]), ptr(out["umi_type"])))
        return out

    def probe_idx(self):
        """UmiCount::probe_idx per molecule, in the order of molecules() / molecule_info() (records with d_probe_idx)"""
        out = np.full(self.n_molecules, _lib.NO_PROBE, np.int32)
        if self.n_molecules:
            self.ctx._check(self.ctx.L.crgpu_counts_probe_idx(self.ctx.h, self.h, ptr(out)))
        return out

    def probe_triplets_dev(self, n_probes):
        """BcUmiInfo::probe_counts of every barcode (types.rs:190-204) as device views: (d_bc, d_probe, d_count, n), ordered by
        (barcode rank, probe_idx); valid until free().  Computed on the first request."""
        a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        self.ctx._check(self.ctx.L.crgpu_counts_probe_triplets_dev(self.ctx.h, self.h, n_probes, C.byref(a), C.byref(b), C.byref(c),
                                                                   C.byref(n)))
        return a.value, b.value, c.value, n.value

    def probe_triplets(self, n_probes):
        """the ProbeBarcodeCount stream (types.rs:141-146) on the host: (barcode rank, probe_idx, umi_count) arrays"""
        L, h, n = self.ctx.L, self.ctx.h, C.c_uint64()
        self.ctx._check(L.crgpu_counts_probe_triplets(h, self.h, n_probes, None, None, None, C.byref(n)))
        bc, pr, ct = (np.zeros(n.value, np.uint32) for _ in range(3))
        if n.value:
            self.ctx._check(L.crgpu_counts_probe_triplets(h, self.h, n_probes, ptr(bc), ptr(pr), ptr(ct), C.byref(n)))
        return bc, pr, ct

    def probe_matrix(self, n_probes, sample_ranks=None):
        """raw probe x barcode matrix (probe_barcode_matrix.rs:176-262) as a MatrixDev: columns = sample_ranks (strictly
        ascending canonical ranks; a numpy array is uploaded, a DeviceArray is used as it is) or, when None, the context's
        BarcodeIndex"""
        d_ranks, n = None, 0
        if sample_ranks is not None:
            d_ranks = sample_ranks if isinstance(sample_ranks, DeviceArray) else self.ctx.upload(
                np.ascontiguousarray(sample_ranks, dtype=np.uint32))
            n = d_ranks.size
        out = C.POINTER(_lib.MatrixDevView)()
        self.ctx._check(self.ctx.L.crgpu_assemble_probe_matrix_dev(self.ctx.h, self.h, n_probes, _p(d_ranks), n, C.byref(out)))
        return MatrixDev(self.ctx, out)

    def probe_metrics(self, n_probes, cell_ranks):
        """collate_probe_metrics' sums per probe (gdna_utils.rs:217-237): (umis_in_all_barcodes, umis_in_filtered_barcodes),
        the second over the barcodes of cell_ranks (strictly ascending canonical ranks, numpy or DeviceArray)"""
        d_cells = cell_ranks if isinstance(cell_ranks, DeviceArray) else self.ctx.upload(
            np.ascontiguousarray(cell_ranks, dtype=np.uint32))
        all_, filt = np.zeros(n_probes, np.uint64), np.zeros(n_probes, np.uint64)
        self.ctx._check(self.ctx.L.crgpu_probe_metrics_dev(self.ctx.h, self.h, n_probes, _p(d_cells), d_cells.size, ptr(all_),
                                                           ptr(filt)))
        return all_, filt

    def feature_metrics(self, n_features, cell_ranks, libs=0):
        """collapse_feature_counts (pandas_utils.py:571-661) over the molecule table: dict of num_umis, num_reads, num_umis_cells,
        num_reads_cells (numpy u64 per feature) over the molecules of the libraries `libs` (an index or several:
        filter_library_idx); the `_cells` sums over the barcodes of cell_ranks (strictly ascending canonical ranks, the union of
        the pass-filter barcodes of those libraries; numpy, DeviceArray or None).  Sharded counts give this rank's share: add the
        shares with Context.allreduce_sum."""
        if cell_ranks is None:
            cell_ranks = np.zeros(0, np.uint32)
        d_cells = cell_ranks if isinstance(cell_ranks, DeviceArray) else self.ctx.upload(np.ascontiguousarray(cell_ranks, dtype=np.uint32))
        out = {k: np.zeros(int(n_features), np.uint64) for k in ("num_umis", "num_reads", "num_umis_cells", "num_reads_cells")}
        self.ctx._check(self.ctx.L.crgpu_feature_metrics_dev(self.ctx.h, self.h, int(n_features), _lib_mask("feature_metrics", libs),
                                                             _p(d_cells) if d_cells.size else None, d_cells.size, *(ptr(v) for v in out.values())))
        return out

    def subsample(self, rates, task_types, cell_ranks, n_genomes=1, feature_genome=None, cell_genome_mask=None, feature_mask=None,
                  seed=1, n_features=None):
        """run_subsampling (subsample.py:430-654) on the molecule table, the binomial replaced by a Philox stream (crgpu.h).
        rates: [n_tasks][n_libs]; task_types: _lib.SS_PER_CELL / SS_CELLS_ONLY / SS_BULK per task; cell_ranks: strictly ascending
        canonical ranks, a numpy array or a DeviceArray (CellCall.ranks_dev()); n_features: of the key layout (default: the
        length of feature_genome / feature_mask).  Returns the SubsampleDataDict arrays plus `any_reads` [library][genome] and
        `info` (crgpu_subsample_result as a dict)."""
        rates = np.ascontiguousarray(rates, dtype=np.float64)
        rates = rates.reshape(len(rates), -1) if rates.ndim != 2 else rates
        T, NL = rates.shape
        types = np.ascontiguousarray(task_types, dtype=np.uint8)
        assert len(types) == T
        d_cells = cell_ranks if isinstance(cell_ranks, DeviceArray) else self.ctx.upload(np.ascontiguousarray(cell_ranks, dtype=np.uint32))
        NC, G = d_cells.size, int(n_genomes)
        fg = None if feature_genome is None else np.ascontiguousarray(feature_genome, dtype=np.uint8)
        fm = None if feature_mask is None else np.ascontiguousarray(feature_mask, dtype=np.uint8)
        cgm = None if cell_genome_mask is None else np.ascontiguousarray(cell_genome_mask, dtype=np.uint32)
        if n_features is None:
            if fg is None and fm is None:
                raise ValueError("n_features (of the key layout) is needed without feature_genome / feature_mask")
            n_features = len(fg) if fg is not None else len(fm)
        F = int(n_features)
        assert (fg is None or len(fg) == F) and (fm is None or len(fm) == F) and (cgm is None or len(cgm) == NC)
        out = dict(umis_per_bc=np.zeros((T, G, NC), np.int64), features_det_per_bc=np.zeros((T, G, NC), np.int64),
                   read_pairs_per_bc=np.zeros((T, G, NC), np.int64), read_pairs=np.zeros((T, G), np.int64), umis=np.zeros((T, G), np.int64),
                   total_features_det=np.zeros((T, G, F), np.int64), any_reads=np.zeros((NL, G), np.uint8))
        a = _lib.SubsampleArgs(n_tasks=T, n_genomes=G, n_libs=NL, n_features=F, n_cells=NC, seed=int(seed), rates=ptr(rates), task_type=ptr(types),
                               d_cell_ranks=_p(d_cells), cell_genome_mask=ptr(cgm), feature_genome=ptr(fg), feature_mask=ptr(fm),
                               **{k: ptr(v) for k, v in out.items()})
        res = _lib.SubsampleResult()
        self.ctx._check(self.ctx.L.crgpu_subsample_dev(self.ctx.h, self.h, C.byref(a), C.byref(res)))
        out["any_reads"] = out["any_reads"].astype(bool)
        out["info"] = {name: getattr(res, name) for name, _ in _lib.SubsampleResult._fields_}
        return out

    def normalize_depth(self, frac_reads_kept, cell_ranks=None, feature_class=None, n_classes=1, cell_class_mask=None, seed=0,
                        want_kept=False, n_features=None):
        """NORMALIZE_DEPTH's main (normalize_depth/__init__.py:387-517) for the whole table of one GEM well, the binomial replaced
        by the Philox stream of Counts.subsample (crgpu.h).  frac_reads_kept: per library (normalize_depth_plan); cell_ranks:
        strictly ascending canonical ranks, a numpy array or a DeviceArray, None: no cells; feature_class: per feature the
        (feature type, genome) pair of summarize_read_matrix, None: one class; cell_class_mask: per cell, bit k = a cell of class
        k, None: of every class; n_features: of the key layout (default: the length of feature_class).  -> NormalizedDepth"""
        frac = np.ascontiguousarray(frac_reads_kept, dtype=np.float64).reshape(-1)
        if cell_ranks is None:
            cell_ranks = np.zeros(0, np.uint32)
        d_cells = cell_ranks if isinstance(cell_ranks, DeviceArray) else self.ctx.upload(np.ascontiguousarray(cell_ranks, dtype=np.uint32))
        NC, NK, NL = d_cells.size, int(n_classes), len(frac)
        fc = None if feature_class is None else np.ascontiguousarray(feature_class, dtype=np.uint8)
        ccm = None if cell_class_mask is None else np.ascontiguousarray(cell_class_mask, dtype=np.uint32)
        if n_features is None:
            if fc is None:
                raise ValueError("n_features (of the key layout) is needed without feature_class")
            n_features = len(fc)
        assert (fc is None or len(fc) == int(n_features)) and (ccm is None or len(ccm) == NC)
        sums = dict(raw_mapped_reads=np.zeros(max(NK, 0), np.int64), flt_mapped_reads=np.zeros(max(NK, 0), np.int64),
                    reads_per_lib=np.zeros(NL, np.int64), kept_reads_per_lib=np.zeros(NL, np.int64), kept_molecules_per_lib=np.zeros(NL, np.int64))
        kept = np.zeros(self.n_molecules, np.uint32) if want_kept else None
        mv = C.POINTER(_lib.MatrixDevView)()
        a = _lib.NormalizeDepthArgs(n_libs=NL, n_features=int(n_features), n_classes=NK, n_cells=NC, seed=int(seed), frac_reads_kept=ptr(frac),
                                    feature_class=ptr(fc), d_cell_ranks=_p(d_cells) if NC else None, cell_class_mask=ptr(ccm),
                                    matrix=C.cast(C.pointer(mv), C.c_void_p), kept_out=ptr(kept), **{k: ptr(v) for k, v in sums.items()})
        res = _lib.NormalizeDepthResult()
        self.ctx._check(self.ctx.L.crgpu_normalize_depth_dev(self.ctx.h, self.h, C.byref(a), C.byref(res)))
        return NormalizedDepth(MatrixDev(self.ctx, mv), sums, kept, {name: getattr(res, name) for name, _ in _lib.NormalizeDepthResult._fields_})

    def barcode_summary(self, rank_lo=0, rank_hi=0xFFFFFFFF):
        """BarcodeSummary rows (cr_lib/src/aligner.rs:33-68) of the barcode ranks in [rank_lo, rank_hi), ordered by
        (library, rank): a numpy record array of _lib.BARCODE_SUMMARY_DTYPE"""
        n = C.c_uint64()
        L, h = self.ctx.L, self.ctx.h
        self.ctx._check(L.crgpu_counts_barcode_summary(h, self.h, rank_lo, rank_hi, None, 0, C.byref(n)))
        rows = np.zeros(n.value, _lib.BARCODE_SUMMARY_DTYPE)
        if n.value:
            self.ctx._check(L.crgpu_counts_barcode_summary(h, self.h, rank_lo, rank_hi, ptr(rows), n.value, C.byref(n)))
        return rows

    def corrected_reads_per_column(self, m, libs=0):
        """the umi_corrected_reads (barcode_summary) of every column of the MatrixDev `m`, the libraries `libs` (an index or several:
        the libraries of one library type) added up -> DeviceArray of u32; the counterpart of Context.reads_per_column"""
        out = self.ctx.empty(m.n_barcodes, np.uint32)
        self.ctx._check(self.ctx.L.crgpu_counts_corrected_reads_per_column(self.ctx.h, self.h, m._mv, _lib_mask("corrected_reads_per_column", libs), _p(out)))
        return out

    def free(self):
        if self.h is not None and self.ctx.h:
            self.ctx.L.crgpu_counts_free(self.ctx.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _lib_mask(who, libs):
    mask = 0
    for l in ([libs] if np.isscalar(libs) else libs):
        if not 0 <= int(l) < 32:
            raise ValueError("%s: library %r" % (who, l))
        mask |= 1 << int(l)
    return mask


def get_unique_id():
    """rendezvous token of an RCCL communicator (rank 0 makes it and ships the bytes to the other processes)"""
    L = _lib.load()
    buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
    rc = L.crgpu_get_unique_id(buf)
    if rc != 0:
        raise CrgpuError(rc, (L.crgpu_last_error(None) or b"").decode())
    return buf.raw


def local_group_id(n_ranks):
    """rendezvous token for n_ranks contexts inside THIS process (one host thread each)"""
    L = _lib.load()
    buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
    rc = L.crgpu_local_group_id(n_ranks, buf)
    if rc != 0:
        raise CrgpuError(rc, (L.crgpu_last_error(None) or b"").decode())
    return buf.raw


class Context:
    """crgpu_ctx: one per (process, device, rank).  n_ranks / rank / unique_id: see crgpu_create in crgpu.h."""

    def __init__(self, device=0, n_ranks=1, rank=0, unique_id=None):
        self.L = _lib.load()
        h = C.c_void_p()
        uid = None
        if unique_id is not None:
            assert len(unique_id) == _lib.UNIQUE_ID_BYTES
            uid = C.create_string_buffer(bytes(unique_id), _lib.UNIQUE_ID_BYTES)
        rc = self.L.crgpu_create(C.byref(h), device, n_ranks, rank, uid)
        if rc != 0:
            raise CrgpuError(rc, (self.L.crgpu_last_error(None) or b"").decode())
        self.h = h
        self.device = device
        self.n_ranks, self.rank = n_ranks, rank
        self.cb_len = None
        self.n_canon = None

    # ---- options / collectives (crgpu.h "collectives") ---------------------------------------------
    def set_option(self, option, value):
        self._check(self.L.crgpu_set_option(self.h, option, int(value)))

    def trust_unchanged_buffers(self, on=True):
        """promise that buffers handed from one call to the next are only written through this context"""
        self.set_option(_lib.OPT_BUFFERS_UNCHANGED_BETWEEN_CALLS, 1 if on else 0)

    def invalidate(self):
        self._check(self.L.crgpu_invalidate(self.h))

    def stat(self, which=0):
        v = C.c_uint64()
        self._check(self.L.crgpu_get_stat(self.h, which, C.byref(v)))
        return v.value

    def barrier(self):
        self._check(self.L.crgpu_barrier(self.h))

    def allreduce_counts(self, lib=-1, which=COUNTS_VALID):
        self._check(self.L.crgpu_allreduce_counts(self.h, lib, which))

    def allreduce_max(self, value):
        v = C.c_double(float(value))
        self._check(self.L.crgpu_allreduce_max_f64(self.h, C.byref(v)))
        return v.value

    def allreduce_sum(self, values):
        """element-wise sum over the ranks of a small int64 host array, in place"""
        assert values.dtype == np.int64 and values.flags["C_CONTIGUOUS"]
        self._check(self.L.crgpu_allreduce_sum_i64(self.h, ptr(values), len(values)))
        return values

    def exchange_keys(self, d_keys, n_keys):
        """C2: (DeviceArray of this rank's keys, n, bounds)"""
        p, n = C.c_void_p(), C.c_uint64()
        bounds = np.zeros(self.n_ranks + 1, np.uint32)
        self._check(self.L.crgpu_exchange_keys_dev(self.h, _p(d_keys), n_keys, C.byref(p), C.byref(n), ptr(bounds)))
        return DeviceArray(self, max(n.value, 1), np.uint64, adopt=p.value), n.value, bounds

    def gatherv(self, d_src, nbytes, dtype, root=0):
        """C3 for one array: (DeviceArray on root / None elsewhere, per-rank element counts on root)"""
        p = C.c_void_p()
        per = np.zeros(self.n_ranks, np.uint64)
        self._check(self.L.crgpu_gatherv_dev(self.h, _p(d_src), nbytes, root, C.byref(p), ptr(per)))
        if self.rank != root:
            return None, None
        item = np.dtype(dtype).itemsize
        counts = [int(x) // item for x in per]
        return DeviceArray(self, max(sum(counts), 1), dtype, adopt=p.value), counts

    def gather_triplets(self, counts, root=0):
        """C3: on root ((bc, feature, count) DeviceArrays, n_total), elsewhere (None, 0)"""
        a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._check(self.L.crgpu_gather_triplets_dev(self.h, counts.h, root, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        if self.rank != root:
            return None, 0
        return tuple(DeviceArray(self, max(n.value, 1), np.uint32, adopt=x.value) for x in (a, b, c)), n.value

    def close(self):
        if getattr(self, "h", None):
            self.L.crgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise CrgpuError(rc, (self.L.crgpu_last_error(self.h) or b"").decode())

    # ---- memory -------------------------------------------------------------------------------
    def empty(self, shape, dtype):
        return DeviceArray(self, shape, dtype)

    def zeros(self, shape, dtype):
        return DeviceArray(self, shape, dtype).zero()

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        return DeviceArray(self, a.shape, a.dtype).upload(a)

    def stream_handle(self):
        """the hipStream_t of the context as an integer (torch.cuda.ExternalStream)"""
        return int(self.L.crgpu_stream(self.h) or 0)

    def synchronize(self):
        self._check(self.L.crgpu_synchronize(self.h))

    def trim(self):
        self._check(self.L.crgpu_trim(self.h))

    # ---- timing -------------------------------------------------------------------------------
    def timing(self, on=True):
        self._check(self.L.crgpu_timing_enable(self.h, int(on)))

    def timing_reset(self):
        self._check(self.L.crgpu_timing_reset(self.h))

    def timing_get(self):
        ms = np.zeros(len(_lib.T_NAMES), np.float64)
        ln = np.zeros(len(_lib.T_NAMES), np.uint64)
        un = np.zeros(len(_lib.T_NAMES), np.uint64)
        self._check(self.L.crgpu_timing_get(self.h, ptr(ms), ptr(ln), ptr(un)))
        return {k: (float(ms[i]), int(ln[i]), int(un[i])) for i, k in enumerate(_lib.T_NAMES)}

    # ---- whitelist ------------------------------------------------------------------------------
    def set_whitelist(self, lib, keys, canon=None, translate_to=None, length=None):
        """keys/canon: list of str, ASCII matrix, or packed uint32 (then `length` is required)."""
        def packed(x):
            if isinstance(x, np.ndarray) and x.dtype == np.uint32:
                return np.ascontiguousarray(x), length
            return pack_seqs(x)
        pk, L1 = packed(keys)
        if canon is None:
            pc, L2 = pk, L1
        else:
            pc, L2 = packed(canon)
        assert L1 == L2 and L1 is not None
        tt = None if translate_to is None else np.ascontiguousarray(translate_to, dtype=np.uint32)
        self._check(self.L.crgpu_set_whitelist_packed(self.h, lib, ptr(pk), len(pk), L1, ptr(pc), len(pc), ptr(tt)))
        self.cb_len, self.n_canon = L1, len(pc)

    def set_whitelist_ascii(self, lib, keys, canon=None, translate_to=None):
        k = ascii_matrix(keys)
        c = k if canon is None else ascii_matrix(canon)
        tt = None if translate_to is None else np.ascontiguousarray(translate_to, dtype=np.uint32)
        self._check(self.L.crgpu_set_whitelist(self.h, lib, k.tobytes(), k.shape[0], k.shape[1], c.tobytes(),
                                               c.shape[0], ptr(tt)))
        self.cb_len, self.n_canon = k.shape[1], c.shape[0]

    def canon_order(self):
        order = np.zeros(self.n_canon, np.uint32)
        seqs = np.zeros(self.n_canon, np.uint32)
        self._check(self.L.crgpu_get_canon_order(self.h, ptr(order), ptr(seqs)))
        return order, seqs

    # ---- barcode stage ---------------------------------------------------------------------------
    def pack(self, d_seq, d_qual, n, length, d_packed, d_qualn, d_flags=None):
        self._check(self.L.crgpu_pack_dev(self.h, _p(d_seq), _p(d_qual), n, length, _p(d_packed), _p(d_qualn), _p(d_flags)))

    def pack_rows(self, d_seq_rows, d_qual_rows, n, row_stride, offset, length, d_packed, d_qualn, d_flags=None):
        """pack bases [offset, offset + length) of every row_stride-byte read row (barcode / UMI ranges of R1)"""
        self._check(self.L.crgpu_pack_rows_dev(self.h, _p(d_seq_rows), _p(d_qual_rows), n, row_stride, offset, length,
                                               _p(d_packed), _p(d_qualn), _p(d_flags)))

    def match_and_count(self, d_cb, d_flags, n, d_idx_out):
        self._check(self.L.crgpu_match_and_count_dev(self.h, _p(d_cb), _p(d_flags), n, _p(d_idx_out)))

    def set_posterior(self, max_expected_barcode_errors, bc_confidence_threshold):
        self._check(self.L.crgpu_set_posterior(self.h, float(max_expected_barcode_errors), float(bc_confidence_threshold)))

    def correct(self, d_cb, d_qualn, d_flags, n, d_idx_inout, d_corrected_out=None):
        self._check(self.L.crgpu_correct_dev(self.h, _p(d_cb), _p(d_qualn), _p(d_flags), n, _p(d_idx_inout), _p(d_corrected_out)))

    def get_counts(self, lib, which=COUNTS_VALID):
        out = np.zeros(self.n_canon, np.uint32)
        self._check(self.L.crgpu_get_counts(self.h, lib, which, ptr(out)))
        return out

    def set_counts(self, lib, which, counts):
        c = np.ascontiguousarray(counts, dtype=np.uint32)
        assert len(c) == self.n_canon
        self._check(self.L.crgpu_set_counts(self.h, lib, which, ptr(c)))

    def reset_counts(self):
        self._check(self.L.crgpu_reset_counts(self.h))

    def counts_dev(self, lib, which):
        p = C.c_void_p()
        self._check(self.L.crgpu_counts_dev(self.h, lib, which, C.byref(p)))
        return p.value

    def barcode_correction_metrics(self, lib=0):
        """BARCODE_CORRECTION summary pieces of one library (barcode_correction.rs:409-448) as a dict"""
        m = _lib.BcCorrectionMetrics()
        self._check(self.L.crgpu_barcode_correction_metrics(self.h, lib, C.byref(m)))
        return {f: getattr(m, f) for f, _ in _lib.BcCorrectionMetrics._fields_}

    def total_barcode_counts(self, min_reads_to_report_bc=1000):
        """(ranks, counts) of total_barcode_counts restricted to whitelist barcodes (barcode_correction.rs:360,380-390)"""
        n = C.c_uint64()
        self._check(self.L.crgpu_total_barcode_counts(self.h, min_reads_to_report_bc, None, None, 0, C.byref(n)))
        ranks, counts = np.zeros(n.value, np.uint32), np.zeros(n.value, np.uint64)
        if n.value:
            self._check(self.L.crgpu_total_barcode_counts(self.h, min_reads_to_report_bc, ptr(ranks), ptr(counts), n.value, C.byref(n)))
        return ranks, counts

    def match_and_count_host(self, lib, seq_ascii, qual):
        s = ascii_matrix(seq_ascii)
        q = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8)
        idx = np.zeros(s.shape[0], np.uint32)
        self._check(self.L.crgpu_match_and_count(self.h, lib, ptr(s), ptr(q), s.shape[0], ptr(idx)))
        return idx

    def correct_host(self, lib, seq_ascii, qual, idx):
        s = ascii_matrix(seq_ascii)
        q = None if qual is None else np.ascontiguousarray(qual, dtype=np.uint8)
        idx = np.ascontiguousarray(idx, dtype=np.uint32).copy()
        flag = np.zeros(s.shape[0], np.uint8)
        self._check(self.L.crgpu_correct(self.h, lib, ptr(s), ptr(q), s.shape[0], ptr(idx), ptr(flag)))
        return idx, flag

    # ---- count stage -------------------------------------------------------------------------------
    def set_key_layout(self, n_features, umi_len, n_libs=1, multiplexing_lib_mask=0):
        self._check(self.L.crgpu_set_key_layout(self.h, n_features, umi_len, n_libs, multiplexing_lib_mask))
        self.n_features, self.umi_len = n_features, umi_len

    def set_target_filter(self, on_target=None, min_read_count=0):
        """targeted-panel UMI filter (mark_dups.rs:311-320); None switches it off"""
        a = None if on_target is None else np.ascontiguousarray(on_target, dtype=np.uint8)
        self._check(self.L.crgpu_set_target_filter(self.h, ptr(a), 0 if a is None else len(a), int(min_read_count)))

    def records(self, n, umi_len, d_bc_idx, d_umi, d_umi_qualn, d_feature, d_flags=None, d_umi_len=None, d_probe_idx=None):
        r = Records()
        r.n, r.umi_len = n, umi_len
        r.d_bc_idx, r.d_umi, r.d_umi_qualn = _p(d_bc_idx), _p(d_umi), _p(d_umi_qualn)
        r.d_feature, r.d_flags, r.d_umi_len = _p(d_feature), _p(d_flags), _p(d_umi_len)
        r.d_probe_idx = _p(d_probe_idx)
        return r

    def count_host(self, n_features, bc_idx, umi, umi_qualn, feature, flags=None, umi_len_per_read=None, probe_idx=None,
                   want_dupinfo=True, want_counts=False):
        """crgpu_count_host: records in HOST arrays -> (Matrix, per-read crgpu_dupinfo records or None[, Counts])"""
        def h(a, dt):
            return None if a is None else np.ascontiguousarray(a, dtype=dt)
        bc_idx, umi, feature = h(bc_idx, np.uint32), h(umi, np.uint32), h(feature, np.uint32)
        umi_qualn, flags, ulen, probe = h(umi_qualn, np.uint8), h(flags, np.uint8), h(umi_len_per_read, np.uint8), h(probe_idx, np.int32)
        n = len(bc_idx)
        r = Records()
        r.n, r.umi_len = n, (umi_qualn.shape[1] if umi_qualn.ndim == 2 else self.umi_len)
        r.d_bc_idx, r.d_umi, r.d_umi_qualn, r.d_feature = ptr(bc_idx), ptr(umi), ptr(umi_qualn), ptr(feature)
        r.d_flags, r.d_umi_len, r.d_probe_idx = ptr(flags), ptr(ulen), ptr(probe)
        dup = np.zeros(n, _lib.DUPINFO_DTYPE) if want_dupinfo else None
        mv = C.POINTER(MatrixView)()
        ch = C.c_void_p()
        self._check(self.L.crgpu_count_host(self.h, C.byref(r), n_features, C.byref(mv), ptr(dup) if n else None,
                                            C.byref(ch) if want_counts else None))
        m = Matrix(self, mv)
        return (m, dup, Counts(self, ch)) if want_counts else (m, dup)

    def set_umi_min_len(self, umi_min_len):
        """per-read UMI lengths umi_min_len .. umi_len (after set_key_layout)"""
        self._check(self.L.crgpu_set_umi_min_len(self.h, umi_min_len))

    def pack_rows_var(self, d_seq_rows, d_qual_rows, d_read_len, n, row_stride, offset, length, min_length, d_packed, d_qualn, d_len):
        """UmiExtractor::extract_umi on read rows: per-read length max(min(read_len - offset, length), min_length)"""
        self._check(self.L.crgpu_pack_rows_var_dev(self.h, _p(d_seq_rows), _p(d_qual_rows), _p(d_read_len), n, row_stride, offset,
                                                   length, min_length, _p(d_packed), _p(d_qualn), _p(d_len)))

    def build_keys(self, recs, d_keys_out):
        n = C.c_uint64()
        self._check(self.L.crgpu_build_keys_dev(self.h, C.byref(recs), _p(d_keys_out), C.byref(n)))
        return n.value

    def partition_keys(self, d_keys, n, n_ranks, d_keys_out, bounds=None):
        counts = np.zeros(n_ranks, np.uint64)
        b = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.uint32)
        assert b is None or len(b) == n_ranks + 1
        self._check(self.L.crgpu_partition_keys_dev(self.h, _p(d_keys), n, n_ranks, ptr(b), _p(d_keys_out), ptr(counts)))
        return counts

    def balanced_bounds(self, n_ranks):
        b = np.zeros(n_ranks + 1, np.uint32)
        self._check(self.L.crgpu_balanced_bounds(self.h, n_ranks, ptr(b)))
        return b

    def count_keys(self, d_keys, n_keys):
        h = C.c_void_p()
        self._check(self.L.crgpu_count_keys_dev(self.h, _p(d_keys), n_keys, C.byref(h)))
        return Counts(self, h)

    def count_records(self, recs, d_processed_umi=None, d_read_count=None, d_dupflags=None):
        """dedup from the records + per-read DupInfo (device output arrays, any may be None)"""
        h = C.c_void_p()
        self._check(self.L.crgpu_count_records_dev(self.h, C.byref(recs), C.byref(h), _p(d_processed_umi), _p(d_read_count),
                                                   _p(d_dupflags)))
        return Counts(self, h)

    def count_records_sharded(self, recs, d_processed_umi=None, d_read_count=None, d_dupflags=None):
        """collective: dedup of one well sharded over the ranks, DupInfo of this rank's own reads (crgpu.h)"""
        h = C.c_void_p()
        self._check(self.L.crgpu_count_records_sharded_dev(self.h, C.byref(recs), C.byref(h), _p(d_processed_umi), _p(d_read_count),
                                                           _p(d_dupflags)))
        return Counts(self, h)

    def enable_barcode_summary(self, on=True):
        """count_keys keeps what Counts.barcode_summary needs (count_records always does)"""
        self._check(self.L.crgpu_enable_barcode_summary(self.h, int(bool(on))))

    def write_barcode_summary_csv(self, rows, path, gem_group=1, library_types=(("Gene Expression", 0),)):
        """barcode_summary.csv of ALIGN_AND_COUNT (align_and_count.rs:806-817).  library_types[lib] = (display
        string of the LibraryType, its rank in the enum's order); libraries of equal rank are one type."""
        rows = np.ascontiguousarray(rows, dtype=_lib.BARCODE_SUMMARY_DTYPE)
        n = len(library_types)
        order = np.array([t[1] for t in library_types], np.uint32)
        names = (C.c_char_p * n)(*[t[0].encode() for t in library_types])
        self._check(self.L.crgpu_write_barcode_summary_csv(self.h, ptr(rows), len(rows), gem_group, ptr(order), names, n,
                                                           path.encode()))

    def shard_metrics(self, d_cb, d_cb_qualn, cb_len, d_umi, d_umi_qualn, umi_len, d_idx, n):
        """MAKE_SHARD's barcode / UMI read metrics as a dict of counts (make_shard_metrics.rs:263-332)"""
        m = _lib.ShardMetrics()
        self._check(self.L.crgpu_shard_metrics_dev(self.h, _p(d_cb), _p(d_cb_qualn), cb_len, _p(d_umi), _p(d_umi_qualn), umi_len,
                                                   _p(d_idx), n, C.byref(m)))
        return {f: int(getattr(m, f)) for f in _lib.SHARD_METRIC_FIELDS}

    def rows_metrics(self, d_seq_rows, d_qual_rows, n, row_stride, d_len=None):
        """frac_n_bases / frac_q30_bases of one read of the pair over FASTQ rows, as a dict of counts"""
        m = _lib.RowsMetrics()
        self._check(self.L.crgpu_rows_metrics_dev(self.h, _p(d_seq_rows), _p(d_qual_rows), _p(d_len), n, row_stride, C.byref(m)))
        return {f: int(getattr(m, f)) for f, _ in _lib.RowsMetrics._fields_}

    def homopolymer_metrics(self, d_r1_rows, r1_stride, n, d_r2_rows=None, r2_stride=0, d_r1_len=None, d_r2_len=None, run_len=15):
        """{A,C,G,T}_perfect_homopolymer: reads whose R1 or R2 holds run_len equal bases in a row"""
        out = np.zeros(4, np.uint64)
        self._check(self.L.crgpu_homopolymer_metrics_dev(self.h, _p(d_r1_rows), r1_stride, _p(d_r1_len), _p(d_r2_rows), r2_stride,
                                                         _p(d_r2_len), n, run_len, ptr(out)))
        return dict(zip("ACGT", (int(x) for x in out)))

    def fastq_to_rows(self, d_text, n_bytes, row_stride, max_records, d_seq_rows, d_qual_rows, d_len=None):
        """FASTQ text (device) -> rows; returns the number of records"""
        n = C.c_uint64()
        self._check(self.L.crgpu_fastq_to_rows_dev(self.h, _p(d_text), n_bytes, row_stride, max_records, _p(d_seq_rows), _p(d_qual_rows),
                                                   _p(d_len), C.byref(n)))
        return n.value

    def sum_matrices(self, a, b):
        """CountMatrix.merge: element-wise sum of two matrices of the same shape"""
        mv = C.POINTER(MatrixView)()
        self._check(self.L.crgpu_sum_matrices(self.h, a._mv, b._mv, C.byref(mv)))
        return Matrix(self, mv)

    def select_barcodes(self, m, cols):
        """CountMatrix.select_barcodes: the given columns in the given order"""
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        mv = C.POINTER(MatrixView)()
        self._check(self.L.crgpu_select_barcodes(self.h, m._mv, ptr(cols), len(cols), C.byref(mv)))
        return Matrix(self, mv)

    def sum_matrices_dev(self, a, b):
        """element-wise sum of two device CSCs over the same columns"""
        mv = C.POINTER(_lib.MatrixDevView)()
        self._check(self.L.crgpu_sum_matrices_dev(self.h, a._mv, b._mv, C.byref(mv)))
        return MatrixDev(self, mv)

    def select_barcodes_dev(self, m, cols):
        """the given columns of a device CSC in the given order"""
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        mv = C.POINTER(_lib.MatrixDevView)()
        self._check(self.L.crgpu_select_barcodes_dev(self.h, m._mv, ptr(cols), len(cols), C.byref(mv)))
        return MatrixDev(self, mv)

    def select_features_dev(self, m, feature_mask):
        """CountMatrix.select_features for an ascending index list: the rows of the MatrixDev `m` whose feature_mask entry is
        non-zero, renumbered to their position among the kept rows; every column stays"""
        mask = np.ascontiguousarray(np.asarray(feature_mask) != 0, dtype=np.uint8)
        mv = C.POINTER(_lib.MatrixDevView)()
        self._check(self.L.crgpu_select_features_dev(self.h, m._mv, ptr(mask), len(mask), C.byref(mv)))
        out = MatrixDev(self, mv)
        out.n_features = int(mask.sum())      # the rows that are left (Context.sseq_params reads it)
        return out

    # ---- cell calling ----------------------------------------------------------------------------------
    def column_sums(self, m, feature_mask=None):
        """get_counts_per_bc of a feature sub-matrix: per column of the MatrixDev `m` the sum over the features whose
        feature_mask entry is non-zero (None: all) -> DeviceArray of u32"""
        out = self.empty(m.n_barcodes, np.uint32)
        mask = None if feature_mask is None else np.ascontiguousarray(np.asarray(feature_mask) != 0, dtype=np.uint8)
        self._check(self.L.crgpu_matrix_dev_column_sums(self.h, m._mv, ptr(mask), 0 if mask is None else len(mask), _p(out)))
        return out

    def call_cells_ordmag(self, counts, recovered_cells=None, max_expected_cells=1 << 18, force_cells=None):
        """filter_cellular_barcodes_ordmag (force_cells: filter_cellular_barcodes_fixed_cutoff) of one GEM group on the device.
        counts: a MatrixDev (its column sums over all features are taken), a DeviceArray of u32 or a numpy array of UMI totals
        per column -> CellCall"""
        matrix = counts if isinstance(counts, MatrixDev) else None
        if matrix is not None:
            d = self.column_sums(matrix)
        elif isinstance(counts, DeviceArray):
            d = counts
        else:
            d = self.upload(np.ascontiguousarray(counts, dtype=np.uint32))
        res, cols, n = _lib.OrdmagResult(), C.c_void_p(), C.c_uint64()
        self._check(self.L.crgpu_call_cells_ordmag_dev(self.h, _p(d), d.size, recovered_cells or 0, max_expected_cells,
                                                       force_cells or 0, C.byref(res), C.byref(cols), C.byref(n)))
        # no barcode called: an empty list of our own, so that .ranks / .filtered_matrix work on an all-zero well, too
        d_cols = DeviceArray(self, n.value, np.uint64, adopt=cols.value) if cols.value else self.empty(0, np.uint64)
        return CellCall(self, d_cols, n.value, res, matrix)

    # ---- multi-genome wells ---------------------------------------------------------------------------
    def genome_totals(self, m, feature_genome, n_genomes):
        """per-genome sums of the MatrixDev `m` (txome_counts of multigenome.py:259): feature_genome[f] = the genome of row f,
        a value >= n_genomes = not counted -> numpy u64[n_genomes]"""
        fg = np.ascontiguousarray(feature_genome, dtype=np.uint8)
        out = np.zeros(n_genomes, np.uint64)
        self._check(self.L.crgpu_matrix_dev_genome_totals(self.h, m._mv, ptr(fg), len(fg), n_genomes, ptr(out)))
        return out

    def multigenome(self, counts0, counts1, bootstraps=1000):
        """classify_gems, the multiplet bootstrap and the mean purities (multigenome.py:80-301) of the filtered barcodes whose
        UMI totals over the two genomes are counts0 / counts1 (DeviceArrays of u32 or numpy arrays) -> Multigenome"""
        d0, d1 = (x if isinstance(x, DeviceArray) else self.upload(np.ascontiguousarray(x, dtype=np.uint32)) for x in (counts0, counts1))
        n = d0.size
        if d1.size != n:
            raise ValueError("multigenome: counts0 and counts1 differ in length")
        if d0.dtype != np.uint32 or d1.dtype != np.uint32:
            raise TypeError("multigenome: device counts must be u32 (as Context.column_sums gives them)")
        call = self.empty(n, np.uint8)
        bc, thr, br = np.zeros((bootstraps, 3), np.int64), np.zeros((bootstraps, 2), np.float64), np.zeros(bootstraps, np.int32)
        res = _lib.MultigenomeResult()
        self._check(self.L.crgpu_multigenome_dev(self.h, _p(d0), _p(d1), n, bootstraps, _p(call), ptr(bc), ptr(thr), ptr(br), C.byref(res)))
        boot = multigenome_summary(bc, n)[0] if n else np.zeros(bootstraps, np.float64)
        out = Multigenome(self, res, call, bc, thr, br, boot)
        out.count0, out.count1 = d0, d1
        return out

    def multigenome_from_matrix(self, filtered_matrix, feature_genome, n_genomes, bootstraps=1000):
        """run_all (multigenome.py:251-335) on the filtered MatrixDev: per-genome totals, the top two genomes, their column sums,
        then Context.multigenome; the result also carries totals, top_two (ascending genome indices) and count0 / count1"""
        fg = np.ascontiguousarray(feature_genome, dtype=np.uint8)
        totals = self.genome_totals(filtered_matrix, fg, n_genomes)
        top = multigenome_top_two(totals)
        if len(top) != 2:
            raise ValueError("multigenome_from_matrix: the analysis needs at least two genomes")
        d0, d1 = (self.column_sums(filtered_matrix, fg == g) for g in top)
        out = self.multigenome(d0, d1, bootstraps)
        out.totals, out.top_two = totals, top
        return out

    # ---- multiplexed Flex (RTL) wells ------------------------------------------------------------------
    def _rtl_probes(self, who):
        """the size of the construct's probe segment as Context.set_barcode_segments recorded it; the host tables per probe rank
        are sized by it, so a construct this object does not know is refused instead of guessed"""
        n = getattr(self, "rtl_n_probe", 0)
        if not n:
            raise ValueError("%s: no GelBeadAndProbe construct was set through Context.set_barcode_segments" % who)
        return n

    def rtl_tags(self, m, tag_of_probe, n_tags, feature_type=None, n_types=0):
        """the tag of every column of the raw MatrixDev `m`, the barcodes per tag and (with feature_type u8[n_features], values
        < n_types or 0xFF) the UMIs per feature type and tag (read_level_multiplexing.rs:22-68) -> RtlTags"""
        if not isinstance(m, MatrixDev):
            raise TypeError("rtl_tags: a MatrixDev (a sharded well gathers its matrix first)")
        top = np.ascontiguousarray(tag_of_probe, dtype=np.uint8)
        if len(top) != self._rtl_probes("rtl_tags"):
            raise ValueError("rtl_tags: tag_of_probe must have one entry per probe barcode (%d)" % self.rtl_n_probe)
        ft = None if feature_type is None else np.ascontiguousarray(feature_type, dtype=np.uint8)
        d_tags = self.empty(m.n_barcodes, np.uint8)
        per_tag = np.zeros(n_tags, np.uint64)
        umi = np.zeros((n_types, n_tags), np.uint64) if n_types else None
        self._check(self.L.crgpu_rtl_tags_dev(self.h, m._mv, ptr(top), n_tags, ptr(ft), 0 if ft is None else len(ft), n_types, _p(d_tags),
                                              ptr(per_tag), ptr(umi)))
        return RtlTags(self, m, d_tags, n_tags, per_tag, umi)

    def rtl_gem_runs(self, m, tags, call, ab=None):
        """one pass over the GEMs of the raw MatrixDev `m`: gel-bead overlaps of the tags and the GEM occupancy of the cell call
        `call` (CellCall).  ab = (ab_tag_of_probe u8[n_probe], Antibody column sums as DeviceArray of u32, ab_min_count u64[n_tags])
        turns the antibody part on (detect_suspicious_rtl_ab_pairings) -> RtlGemRuns"""
        res = _lib.RtlGemRuns()
        abt = d_sums = low = None
        if ab is not None:
            abt, d_sums, low = np.ascontiguousarray(ab[0], dtype=np.uint8), ab[1], np.ascontiguousarray(ab[2], dtype=np.uint64)
            if not isinstance(d_sums, DeviceArray):
                d_sums = self.upload(np.ascontiguousarray(d_sums, dtype=np.uint32))
            if d_sums.dtype != np.uint32 or d_sums.size != m.n_barcodes or len(low) != tags.n_tags:
                raise ValueError("rtl_gem_runs: the Antibody sums are u32 per column, ab_min_count has one entry per tag")
            if len(abt) != self._rtl_probes("rtl_gem_runs"):
                raise ValueError("rtl_gem_runs: ab_tag_of_probe must have one entry per probe barcode (%d)" % self.rtl_n_probe)
        self._check(self.L.crgpu_rtl_gem_runs_dev(self.h, m._mv, _p(tags.tags_dev), tags.n_tags, _p(call.cols), call.n_cells, ptr(abt),
                                                  _p(d_sums), ptr(low), C.byref(res)))
        return RtlGemRuns(res)

    def rtl_medians(self, counts, call, m=None):
        """get_median_umi_per_cell for one feature type: counts = the column sums of the raw matrix under that type's mask
        (DeviceArray of u32) -> (n_nonzero u64[n_probe], median u64[n_probe]) per probe rank"""
        m = m or call._matrix
        if m is None:
            raise ValueError("rtl_medians: pass the MatrixDev the counts belong to")
        P = self._rtl_probes("rtl_medians")
        nz, med = np.zeros(256, np.uint64), np.zeros(256, np.uint64)
        self._check(self.L.crgpu_rtl_medians_dev(self.h, m._mv, _p(counts), _p(call.cols), call.n_cells, ptr(nz), ptr(med)))
        return nz[:P], med[:P]

    def remove_high_occupancy_gems(self, m, call, threshold):
        """remove_bcs_from_high_occupancy_gems (cell_calling_helpers.py:315-424) behind its threshold: the cells of GEMs with more
        than `threshold` cells are dropped -> (CellCall of the kept columns, dict of crgpu_rtl_high_occupancy)"""
        res, out = _lib.RtlHighOccupancy(), C.c_void_p()
        self._check(self.L.crgpu_rtl_remove_high_occupancy_dev(self.h, m._mv, _p(call.cols), call.n_cells, int(threshold), C.byref(out),
                                                               C.byref(res)))
        kept = DeviceArray(self, int(res.n_kept), np.uint64, adopt=out.value)
        d = {name: getattr(res, name) for name, _ in _lib.RtlHighOccupancy._fields_ if name != "reserved"}
        return CellCall(self, kept, int(res.n_kept), dict(call.metrics), m), d

    # ---- protein aggregates, the closing filters of a cell call ------------------------------------------
    def _per_column(self, who, x, V):
        """a u32 value per column as a DeviceArray (a numpy array is uploaded)"""
        d = x if isinstance(x, DeviceArray) else self.upload(np.ascontiguousarray(x, dtype=np.uint32))
        if d.dtype != np.uint32 or d.size != V:
            raise ValueError("%s: a u32 value per column of the matrix (%d)" % (who, V))
        return d

    def take_columns(self, src, cols, n=None):
        """src[cols] on the device: src a DeviceArray of u8 or u32 per column, cols a DeviceArray / numpy array of u64 -> numpy"""
        d_cols = cols if isinstance(cols, DeviceArray) else self.upload(np.ascontiguousarray(cols, dtype=np.uint64))
        n = d_cols.size if n is None else int(n)
        out = self.empty(n, src.dtype)
        self._check(self.L.crgpu_take_columns_dev(self.h, _p(src), src.dtype.itemsize, src.size, _p(d_cols), n, _p(out)))
        return out.to_host(n)

    def sum_u32(self, d):
        out = C.c_uint64()
        self._check(self.L.crgpu_sum_u32_dev(self.h, _p(d), d.size, C.byref(out)))
        return out.value

    def aggregates_by_counts(self, m, feature_kind, num_probe_barcodes=None, reasons=None):
        """detect_aggregate_barcodes (analysis.py:133-185) on the raw MatrixDev `m`: feature_kind u8[n_features] of _lib.AGG_KIND_*,
        reasons: a DeviceArray of u8 per column that gets _lib.AGG_COUNTS -> (numpy u64 of the columns, ascending; info dict)"""
        kind = np.ascontiguousarray(feature_kind, dtype=np.uint8)
        K = 25 * max(int(num_probe_barcodes or 0), 1)
        cols, n, info = np.zeros(K, np.uint64), C.c_uint32(), _lib.AggregatesInfo()
        self._check(self.L.crgpu_aggregates_by_counts_dev(self.h, m._mv, ptr(kind), len(kind), int(num_probe_barcodes or 0), _p(reasons), ptr(cols), K,
                                                          C.byref(n), C.byref(info)))
        return cols[:n.value], {name: getattr(info, name) for name, _ in _lib.AggregatesInfo._fields_ if name != "reserved"}

    def highly_corrected(self, reads, corrected_reads, reasons):
        """detect_highly_corrected_bcs (analysis.py:91-99) over two DeviceArrays of u32 per column (Context.reads_per_column,
        Counts.corrected_reads_per_column): marks _lib.AGG_HIGHLY_CORRECTED in `reasons` -> the number of columns marked"""
        n = C.c_uint64()
        if reads.size != corrected_reads.size or reads.size != reasons.size:
            raise ValueError("highly_corrected: one entry per column in every array")
        self._check(self.L.crgpu_aggregates_highly_corrected_dev(self.h, _p(reads), _p(corrected_reads), reads.size, _p(reasons), C.byref(n)))
        return n.value

    def antigen_outliers(self, m, feature_kind, reasons=None):
        """detect_outlier_umis_bcs (analysis.py:77-88) -> (numpy u64 of the columns, ascending; the threshold)"""
        kind = np.ascontiguousarray(feature_kind, dtype=np.uint8)
        cols, n, thr = np.zeros(100, np.uint64), C.c_uint32(), C.c_double()
        self._check(self.L.crgpu_aggregates_antigen_outliers_dev(self.h, m._mv, ptr(kind), len(kind), _p(reasons), ptr(cols), 100, C.byref(n),
                                                                 C.byref(thr)))
        return cols[:n.value], thr.value

    def remove_aggregates(self, m, feature_kind, num_probe_barcodes=None, reads=None, corrected_reads=None, disable=False):
        """remove_antibody_antigen_aggregates (cell_calling_helpers.py:214-270) on the raw MatrixDev `m`.  feature_kind u8[n_features]
        of _lib.AGG_KIND_*; a library type takes part when it has a feature.  reads / corrected_reads: {library type: u32 per column}
        (DeviceArrays of Context.reads_per_column / Counts.corrected_reads_per_column, or numpy arrays); the highly corrected
        barcodes need both for "Antibody Capture".  disable: detect and report, return `m` itself (disable_ab_aggregate_detection)
        -> (MatrixDev, Aggregates)"""
        kind = np.ascontiguousarray(feature_kind, dtype=np.uint8)
        V = m.n_barcodes
        reads = {k: self._per_column("remove_aggregates", v, V) for k, v in (reads or {}).items()}
        corrected = {k: self._per_column("remove_aggregates", v, V) for k, v in (corrected_reads or {}).items()}
        reasons = self.zeros(V, np.uint8)
        info, thr, bits = None, None, {}
        AB, AG = "Antibody Capture", "Antigen Capture"
        if (kind == _lib.AGG_KIND_ANTIBODY).any():
            bits[AB] = (_lib.AGG_COUNTS | _lib.AGG_HIGHLY_CORRECTED, _lib.AGG_KIND_ANTIBODY)
            if AB in reads and AB in corrected:
                self.highly_corrected(reads[AB], corrected[AB], reasons)
            _, info = self.aggregates_by_counts(m, kind, num_probe_barcodes, reasons)
        if (kind == _lib.AGG_KIND_ANTIGEN).any():
            bits[AG] = (_lib.AGG_ANTIGEN, _lib.AGG_KIND_ANTIGEN)
            _, thr = self.antigen_outliers(m, kind, reasons)
        kept, n_kept, rem, n_rem = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        self._check(self.L.crgpu_aggregates_partition_dev(self.h, _p(reasons), V, C.byref(kept), C.byref(n_kept), C.byref(rem), C.byref(n_rem)))
        d_kept = DeviceArray(self, n_kept.value, np.uint64, adopt=kept.value)
        d_rem = DeviceArray(self, n_rem.value, np.uint64, adopt=rem.value)
        removed = d_rem.to_host(n_rem.value)
        why = self.take_columns(reasons, d_rem, n_rem.value)
        libraries = {}
        for lib, (mask, k) in bits.items():
            cols = removed[(why & mask) != 0]
            d = {"number_aggregate_GEMs": int(len(cols)), "cols": cols, "reads_removed": None, "reads_total": None}
            d["umis"] = self.take_columns(self.column_sums(m, kind == k), cols)
            if lib in reads:
                d["reads"] = self.take_columns(reads[lib], cols)
                d["reads_removed"], d["reads_total"] = int(d["reads"].sum(dtype=np.uint64)), self.sum_u32(reads[lib])
                with np.errstate(divide="ignore", invalid="ignore"):
                    d["frac_total_reads"] = d["reads"].astype(np.float64) / np.float64(d["reads_total"])
                    if lib in corrected:
                        d["corrected_reads"] = self.take_columns(corrected[lib], cols)
                        d["frac_corrected_reads"] = d["corrected_reads"].astype(np.float64) / d["reads"].astype(np.float64)
            libraries[lib] = d
        agg = Aggregates(removed, why, d_kept, n_kept.value, info, thr, libraries, bool(disable))
        if disable:
            return m, agg
        mv = C.POINTER(_lib.MatrixDevView)()
        self._check(self.L.crgpu_select_barcodes_cols_dev(self.h, m._mv, _p(d_kept), n_kept.value, C.byref(mv)))
        return MatrixDev(self, mv), agg

    def apply_minimum_umis(self, call, umis, minimum_umis):
        """apply_global_minimum_umis_threshold (cell_calling_helpers.py:749-785) of one GEM group and genome: the cells of the
        CellCall whose entry of `umis` (u32 per column of the matrix: Context.column_sums with the feature types' mask) is >=
        minimum_umis, in their order -> CellCall"""
        V = umis.size if isinstance(umis, DeviceArray) else len(umis)
        d = self._per_column("apply_minimum_umis", umis, V)
        out, n = C.c_void_p(), C.c_uint64()
        self._check(self.L.crgpu_filter_cells_min_umis_dev(self.h, _p(d), V, _p(call.cols), call.n_cells, int(minimum_umis), C.byref(out), C.byref(n)))
        return CellCall(self, DeviceArray(self, n.value, np.uint64, adopt=out.value), n.value, dict(call.metrics), call._matrix)

    def apply_mito_threshold(self, call, mito_umis, total_umis, max_mito_percent):
        """apply_mitochondrial_threshold (cell_calling_helpers.py:671-746) of one GEM group and genome: mito_umis / total_umis = u32
        per column of the matrix (Context.column_sums over the mitochondrial genes / over all Gene Expression rows of the genome).
        Cells with 100.0 * mito / total > max_mito_percent leave (0 / 0 is NaN and stays)
        -> (CellCall, dict(cols, total_umis, mt_pct: numpy arrays over the removed cells, threshold))"""
        V = total_umis.size if isinstance(total_umis, DeviceArray) else len(total_umis)
        d_t, d_m = self._per_column("apply_mito_threshold", total_umis, V), self._per_column("apply_mito_threshold", mito_umis, V)
        kept, n_kept, rem, n_rem = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
        self._check(self.L.crgpu_filter_cells_mito_dev(self.h, _p(d_m), _p(d_t), V, _p(call.cols), call.n_cells, float(max_mito_percent), C.byref(kept),
                                                       C.byref(n_kept), C.byref(rem), C.byref(n_rem)))
        d_rem = DeviceArray(self, n_rem.value, np.uint64, adopt=rem.value)
        tot, mt = self.take_columns(d_t, d_rem, n_rem.value), self.take_columns(d_m, d_rem, n_rem.value)
        with np.errstate(divide="ignore", invalid="ignore"):      # (a removed cell has a percentage: total 0 only with mito > 0, inf)
            pct = 100.0 * mt.astype(np.float64) / tot.astype(np.float64)      # the device's own expression, f64 and unfused on both sides
        summary = {"cols": d_rem.to_host(n_rem.value), "total_umis": tot, "mt_pct": pct, "threshold": float(max_mito_percent)}
        return CellCall(self, DeviceArray(self, n_kept.value, np.uint64, adopt=kept.value), n_kept.value, dict(call.metrics), call._matrix), summary

    # ---- the summary metrics of the filtered matrix ---------------------------------------------------
    def reads_per_column(self, m, libs=0):
        """the counted reads (VALID + CORRECTED) of every column of the MatrixDev `m`, the libraries `libs` (an index or several: the
        libraries of one library type) added up -> DeviceArray of u32"""
        mask = 0
        for l in ([libs] if np.isscalar(libs) else libs):
            if not 0 <= int(l) < 32:
                raise ValueError("reads_per_column: library %r" % (l,))
            mask |= 1 << int(l)
        out = self.empty(m.n_barcodes, np.uint32)
        self._check(self.L.crgpu_matrix_dev_reads_per_column(self.h, m._mv, mask, _p(out)))
        return out

    def matrix_summary(self, m, cells, feature_class=None, n_classes=1, cell_class_mask=None, reads=None, per_cell=False, n_features=None):
        """the integers behind report_matrix's _report / _report_genome_agnostic_metrics on the RAW MatrixDev `m`.  cells: a CellCall,
        the AdditionalCells of an EmptyDrops merge, or a device / numpy array of ascending columns.  feature_class u8[n_features]
        (0xFF: in no class; None: every feature in class 0, n_features then comes from the argument or the key layout),
        cell_class_mask u32 per listed cell (bit k: a cell of class k; None: of every class), reads = Context.reads_per_column (or a
        numpy array per column), per_cell: keep counts_per_cell / genes_per_cell on the device -> MatrixSummary"""
        if isinstance(cells, AdditionalCells):
            cells = cells.call
        if isinstance(cells, CellCall):
            d_cols, n_cells = cells.cols, cells.n_cells
        elif isinstance(cells, DeviceArray):
            d_cols, n_cells = cells, cells.size
        else:
            h = np.ascontiguousarray(cells, dtype=np.uint64)
            d_cols, n_cells = (self.upload(h) if len(h) else None), len(h)
        if d_cols is not None and n_cells and d_cols.dtype != np.uint64:
            raise TypeError("matrix_summary: the cell columns are u64 (as the cell call returns them)")
        fc = None if feature_class is None else np.ascontiguousarray(feature_class, dtype=np.uint8)
        if fc is not None:
            n_features = len(fc)
        elif n_features is None:
            n_features = getattr(self, "n_features", None)
            if n_features is None:
                raise ValueError("matrix_summary: pass feature_class or n_features")
        cm = None if cell_class_mask is None else np.ascontiguousarray(cell_class_mask, dtype=np.uint32)
        if cm is not None and len(cm) != n_cells:
            raise ValueError("matrix_summary: cell_class_mask has one entry per listed cell (%d)" % n_cells)
        if reads is not None and not isinstance(reads, DeviceArray):
            reads = self.upload(np.ascontiguousarray(reads, dtype=np.uint32))
        if reads is not None and (reads.dtype != np.uint32 or reads.size != m.n_barcodes):
            raise ValueError("matrix_summary: reads are u32 per column of the matrix")
        per_f, ge2 = np.zeros(n_features, np.uint64), np.zeros(n_features, np.uint64)
        structs = (_lib.MatrixSummaryClass * n_classes)()
        r_all, r_union = C.c_uint64(), C.c_uint64()
        cpc = gpc = None
        if per_cell:
            cpc, gpc = self.zeros((n_classes, n_cells), np.uint32), self.zeros((n_classes, n_cells), np.uint32)
        self._check(self.L.crgpu_matrix_summary_dev(self.h, m._mv, n_features, n_classes, ptr(fc), _p(d_cols) if n_cells else None, n_cells, ptr(cm),
                                                    _p(reads), ptr(per_f), ptr(ge2), structs, C.byref(r_all), C.byref(r_union), _p(cpc), _p(gpc)))
        have = reads is not None
        return MatrixSummary(self, list(structs), per_f, ge2, r_all.value if have else None, r_union.value if have else None, n_cells, cpc, gpc)

    def rpu_gmm(self, values, labels, want_starts=False):
        """fit_enrichments(tgt_label, values, method=BOTH_TIED) (targeted/gmm.py:116-183) on the device: values = log10 reads per
        UMI of the quantifiable genes (f64), labels = 1 for a targeted gene.  -> dict of the seven RpuFitParams (sd_high / sd_low
        are the tied PRECISION, as the reference reports them), the four ClassStats (f64, NaN where the reference has NaN),
        `enriched` (u8 per gene: value >= threshold), winner, n_starts, max_lk, fitted, in_lds, fit_ms; want_starts adds start_lk
        (f64[5152]) and start_iters (u32[5152])."""
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        lab = np.ascontiguousarray(labels).astype(np.uint8).reshape(-1)
        if len(v) != len(lab):
            raise ValueError("rpu_gmm: one label per value")
        enriched = np.zeros(len(v), np.uint8)
        lk = np.zeros(_lib.GMM_STARTS, np.float64) if want_starts else None
        it = np.zeros(_lib.GMM_STARTS, np.uint32) if want_starts else None
        a = _lib.RpuGmmArgs(start_lk_out=ptr(lk), start_iters_out=ptr(it), enriched_out=ptr(enriched) if len(v) else None, reserved=0)
        res = _lib.RpuGmmResult()
        self._check(self.L.crgpu_rpu_gmm_dev(self.h, ptr(v) if len(v) else None, ptr(lab) if len(v) else None, len(v), C.byref(a), C.byref(res)))
        out = {name: getattr(res, name) for name, _ in _lib.RpuGmmResult._fields_}
        out["enriched"] = enriched
        if want_starts:
            out["start_lk"], out["start_iters"] = lk, it
        return out

    # ---- cell-multiplexed (CMO) wells ------------------------------------------------------------------
    def jibes_tag_counts(self, m, tag_rows, n_features=None):
        """the tag table of the filtered MatrixDev `m` (JibesTagAssigner.__init__): tag_rows = the feature rows of the Multiplexing
        Capture library, ascending -> dict(counts i32[V, n_rows], row_sums u64[V], near_zero / kept = the columns whose sum over ALL
        tag rows is <= 12 / above, log_counts f64[V, n_rows] = np.log10(counts + 1.0), taken by numpy as the reference takes it)"""
        rows = np.ascontiguousarray(tag_rows, dtype=np.uint32)
        if n_features is None:
            n_features = getattr(self, "n_features", None)
            if n_features is None:
                raise ValueError("jibes_tag_counts: pass n_features")
        V = m.n_barcodes
        counts, sums = np.zeros((V, len(rows)), np.int32), np.zeros(V, np.uint64)
        nz, kept, n_nz = np.zeros(V, np.uint64), np.zeros(V, np.uint64), C.c_uint64()
        self._check(self.L.crgpu_jibes_tag_counts_dev(self.h, m._mv, ptr(rows), len(rows), int(n_features), ptr(counts), ptr(sums), ptr(nz), C.byref(n_nz),
                                                      ptr(kept)))
        return dict(counts=counts, row_sums=sums, near_zero=nz[:n_nz.value].copy(), kept=kept[:V - n_nz.value].copy(),
                    log_counts=np.log10(counts + 1.0))

    def marginal_calls(self, m, feature_rows, umi_threshold=1, n_features=None, want_histograms=False):
        """call_presence_with_gmm_ab for every listed feature row of the filtered MatrixDev `m` (csrc/marginal_calls.h): feature_rows
        ascending; a cell is assigned a feature when its count >= umi_threshold and falls to the mixture's upper component
        -> MarginalCalls"""
        rows = np.ascontiguousarray(feature_rows, dtype=np.uint32)
        if n_features is None:
            n_features = getattr(self, "n_features", None)
            if n_features is None:
                raise ValueError("marginal_calls: pass n_features")
        out = C.POINTER(_lib.MarginalCalls)()
        self._check(self.L.crgpu_marginal_calls_dev(self.h, m._mv, ptr(rows), len(rows), int(n_features), int(umi_threshold), 1 if want_histograms else 0,
                                                    C.byref(out)))
        return MarginalCalls(self, out, rows, umi_threshold)

    def kmeans(self, projection, n_clusters, seed=0, num_pcs=None, init=None, max_iter=300, tol=1e-4):
        """scikit-learn 1.7.2's KMeans(n_clusters = K, random_state = seed) with the reference's Davies-Bouldin score and relabel_by_size
        (csrc/kmeans.h) for one K or a list of distinct K on the f64 projection [cells x PCs]; num_pcs takes the first columns as a view;
        init: None, or one k x d array (n_clusters an int), or a list with None or an array per K (scikit-learn's init = array)
        -> one dict per K: n_clusters, labels i32[n], clusters i32[n] (1-based, the largest first), centers f64[K, d], inertia, n_iter,
        strict, relocations, sizes u64[K], wss f64[K], db_score, in_lds, fit_ms"""
        x = np.ascontiguousarray(projection, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("kmeans: the projection is cells x PCs")
        n, ld = x.shape
        d = ld if num_pcs is None else int(num_pcs)
        single = np.ndim(n_clusters) == 0
        ks = np.ascontiguousarray([n_clusters] if single else n_clusters, dtype=np.uint32)
        inits = [init] if single else (list(init) if init is not None else None)
        a = _lib.KmeansArgs(init=None, tol_factor=float(tol), seed=int(seed), max_iter=int(max_iter))
        keep = []
        if inits is not None and any(i is not None for i in inits):
            if len(inits) != len(ks):
                raise ValueError("kmeans: one init (or None) per K")
            arr = (C.c_void_p * len(ks))()
            for p, i in enumerate(inits):
                if i is None:
                    continue
                i = np.ascontiguousarray(i, dtype=np.float64)
                if i.shape != (int(ks[p]), d):
                    raise ValueError("kmeans: init of K = %d is %d x %d" % (ks[p], ks[p], d))
                keep.append(i)
                arr[p] = i.ctypes.data
            a.init = C.cast(arr, C.POINTER(C.c_void_p))
        res = (_lib.KmeansResult * len(ks))()
        outs = []
        for p, k in enumerate(ks):
            k = int(k)
            o = dict(n_clusters=k, labels=np.zeros(n, np.int32), clusters=np.zeros(n, np.int32), centers=np.zeros((k, d)),
                     sizes=np.zeros(k, np.uint64), wss=np.zeros(k))
            res[p].labels_out, res[p].clusters_out, res[p].centers_out = ptr(o["labels"]), ptr(o["clusters"]), ptr(o["centers"])
            res[p].sizes_out, res[p].wss_out = ptr(o["sizes"]), ptr(o["wss"])
            outs.append(o)
        self._check(self.L.crgpu_kmeans_dev(self.h, ptr(x), n, d, ld, ptr(ks), len(ks), C.byref(a), res))
        for p, o in enumerate(outs):
            r = res[p]
            o.update(inertia=r.inertia, db_score=r.db_score, fit_ms=r.fit_ms, n_iter=int(r.n_iter), strict=bool(r.strict),
                     relocations=int(r.relocations), in_lds=bool(r.in_lds))
        return outs

    def knn(self, projection, k, num_pcs=None, query_start=0, n_queries=None, capacity=0, force_device=False, cand_tile=0):
        """BallTree(x).query(rows, k + 1) then [:, 1:] of scikit-learn 1.7.2, exactly and by brute force on the device (csrc/knn.hip): for
        the rows query_start .. query_start + n_queries (default: to the end) of the f64 projection [cells x PCs] the k entries after
        the first in the order of the pairs (d2, index) over all rows; num_pcs takes the first columns as a view.  A row with an exact
        duplicate of lower index keeps itself as a neighbour.  capacity / force_device / cand_tile: test seams, no result depends on them
        -> dict(indices i32[q, k] by rank, distances f64[q, k], sorted_indices i32[q, k] ascending per row, compactions, selections,
        survivors, pairs_evaluated, in_lds, capacity, query_tiles, cand_tile, fit_ms, select_ms, sort_ms)"""
        x = np.ascontiguousarray(projection, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("knn: the projection is cells x PCs")
        n, ld = x.shape
        d = ld if num_pcs is None else int(num_pcs)
        q0 = int(query_start)
        nq = n - q0 if n_queries is None else int(n_queries)
        if q0 < 0 or nq < 1 or q0 + nq > n:
            raise ValueError("knn: queries %d + %d of %d rows" % (q0, nq, n))
        k = int(k)
        if not 1 <= k <= _lib.KNN_MAX_K:      # the output arrays need a shape; the library refuses the rest
            raise ValueError("knn: k = %d, 1 to %d" % (k, _lib.KNN_MAX_K))
        o = dict(indices=np.zeros((nq, k), np.int32), distances=np.zeros((nq, k)), sorted_indices=np.zeros((nq, k), np.int32))
        a = _lib.KnnArgs(query_start=q0, n_queries=nq, capacity=int(capacity), force_device=1 if force_device else 0, cand_tile=int(cand_tile))
        r = _lib.KnnResult(indices_out=ptr(o["indices"]), distances_out=ptr(o["distances"]), sorted_out=ptr(o["sorted_indices"]))
        self._check(self.L.crgpu_knn_dev(self.h, ptr(x), n, d, ld, k, C.byref(a), C.byref(r)))
        o.update(compactions=int(r.compactions), selections=int(r.selections), survivors=int(r.survivors), pairs_evaluated=int(r.pairs_evaluated),
                 in_lds=bool(r.in_lds), capacity=int(r.capacity), query_tiles=int(r.query_tiles), cand_tile=int(r.cand_tile), fit_ms=r.fit_ms,
                 select_ms=r.select_ms, sort_ms=r.sort_ms)
        return o

    def knn_cross(self, projection, k, query_start, n_queries, cand_start, n_cands, num_pcs=None, capacity=0, force_device=False, cand_tile=0):
        """find_knn(cur_matrix, ref_matrix, knn) of CORRECT_CHEMISTRY_BATCH = BallTree(ref).query(cur, k), exactly and by brute force on
        the device (crgpu_knn_cross_dev, csrc/knn.hip): for the rows query_start .. + n_queries of the f64 projection [cells x PCs] the
        first k entries in the order of the pairs (d2, index) over the rows cand_start .. + n_cands ALONE; nothing is dropped; the
        indices are global row numbers.  k > n_cands is refused.  capacity / force_device / cand_tile: test seams, no result depends on
        them -> the dict of Context.knn (pairs_evaluated = n_queries * n_cands)"""
        x = np.ascontiguousarray(projection, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("knn_cross: the projection is cells x PCs")
        n, ld = x.shape
        d = ld if num_pcs is None else int(num_pcs)
        q0, nq, c0, nc, k = int(query_start), int(n_queries), int(cand_start), int(n_cands), int(k)
        if q0 < 0 or nq < 1 or q0 + nq > n or c0 < 0 or nc < 1 or c0 + nc > n:
            raise ValueError("knn_cross: queries %d + %d, candidates %d + %d of %d rows" % (q0, nq, c0, nc, n))
        if not 1 <= k <= _lib.KNN_MAX_K:      # the output arrays need a shape; the library refuses the rest
            raise ValueError("knn_cross: k = %d, 1 to %d" % (k, _lib.KNN_MAX_K))
        o = dict(indices=np.zeros((nq, k), np.int32), distances=np.zeros((nq, k)), sorted_indices=np.zeros((nq, k), np.int32))
        a = _lib.KnnCrossArgs(query_start=q0, n_queries=nq, cand_start=c0, n_cands=nc, capacity=int(capacity), force_device=1 if force_device else 0,
                              cand_tile=int(cand_tile))
        r = _lib.KnnResult(indices_out=ptr(o["indices"]), distances_out=ptr(o["distances"]), sorted_out=ptr(o["sorted_indices"]))
        self._check(self.L.crgpu_knn_cross_dev(self.h, ptr(x), n, d, ld, k, C.byref(a), C.byref(r)))
        o.update(compactions=int(r.compactions), selections=int(r.selections), survivors=int(r.survivors), pairs_evaluated=int(r.pairs_evaluated),
                 in_lds=bool(r.in_lds), capacity=int(r.capacity), query_tiles=int(r.query_tiles), cand_tile=int(r.cand_tile), fit_ms=r.fit_ms,
                 select_ms=r.select_ms, sort_ms=r.sort_ms)
        return o

    @staticmethod
    def _tsne_report(r):
        return dict(sum_q=r.sum_q, kl=r.kl, p_total=r.p_total, fit_ms=r.fit_ms, search_ms=r.search_ms, csr_ms=r.csr_ms, loop_ms=r.loop_ms,
                    repulse_ms=r.repulse_ms, nnz=int(r.nnz), pairs_evaluated=int(r.pairs_evaluated), row_tile=int(r.row_tile), cand_tile=int(r.cand_tile),
                    slab_rows=int(r.slab_rows), wave_row_len=int(r.wave_row_len), n_chunks=int(r.n_chunks), n_groups=int(r.n_groups),
                    max_steps=int(r.max_steps))

    @staticmethod
    def _tsne_csr(who, indptr, indices, values):
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        indices, values = np.ascontiguousarray(indices, dtype=np.int32), np.ascontiguousarray(values, dtype=np.float64)
        if indptr.ndim != 1 or len(indptr) < 2 or indices.ndim != 1 or indices.shape != values.shape or int(indptr[-1]) != len(indices):
            raise ValueError("%s: indptr i64[n + 1], indices and values of indptr[n] entries each" % who)
        return indptr, indices, values

    def tsne_affinities(self, nn_indices, nn_distances, perplexity):
        """The perplexity search and the symmetrised sparse P of Barnes-Hut t-SNE on the device (crgpu_tsne_affinities_dev,
        csrc/tsne.hip) from Context.knn's indices and distances [n, k] at k = floor(3 * perplexity): per row the bisection on beta
        (start 1, at most 200 steps, |H - log(perplexity)| < 1e-5), the union of both directions with the value (p_ij + p_ji) / 2, CSR
        with ascending indices, the values divided by their total (256-entry partials, then the partials ascending)
        -> dict(beta f64[n], steps u32[n], cond f64[n, k] by rank, indptr i64[n + 1], indices i32[nnz], values f64[nnz], p_total,
        max_steps, nnz, fit_ms, search_ms, csr_ms, ...)"""
        ind, dist = np.ascontiguousarray(nn_indices, dtype=np.int32), np.ascontiguousarray(nn_distances, dtype=np.float64)
        if ind.ndim != 2 or ind.shape != dist.shape:
            raise ValueError("tsne_affinities: indices and distances of one shape [n, k]")
        n, k = ind.shape
        if not 1 <= k <= _lib.KNN_MAX_K or 2 * n * k >= 1 << 32:      # the output arrays need a shape; the library refuses the rest
            raise ValueError("tsne_affinities: k = %d, 1 to %d, and fewer than 2^31 pairs" % (k, _lib.KNN_MAX_K))
        o = dict(beta=np.zeros(n), steps=np.zeros(n, np.uint32), cond=np.zeros((n, k)), indptr=np.zeros(n + 1, np.int64))
        indices, values = np.zeros(2 * n * k, np.int32), np.zeros(2 * n * k)
        a = _lib.TsneArgs()
        r = _lib.TsneResult(beta_out=ptr(o["beta"]), steps_out=ptr(o["steps"]), cond_out=ptr(o["cond"]), indptr_out=ptr(o["indptr"]),
                            indices_out=ptr(indices), values_out=ptr(values))
        self._check(self.L.crgpu_tsne_affinities_dev(self.h, ptr(ind), ptr(dist), n, k, float(perplexity), C.byref(a), C.byref(r)))
        o.update(self._tsne_report(r))
        o.update(indices=indices[:o["nnz"]].copy(), values=values[:o["nnz"]].copy())
        return o

    def tsne_gradient(self, indptr, indices, values, y, exaggeration=1.0, row_tile=0, cand_tile=0, slab_rows=0, wave_row_len=0):
        """bh_tsne's gradient (a quarter of the analytic one), Z and the cost at y [n, 2 or 3] for a CSR P, with exact repulsion over all
        n (n - 1) ordered pairs (crgpu_tsne_gradient_dev): dC = pos - neg / Z in the one sum order of include/crgpu.h.  row_tile /
        cand_tile / slab_rows / wave_row_len: test seams, no result depends on them
        -> dict(grad f64[n, dims], sum_q, kl, pairs_evaluated, the seams used, n_chunks, n_groups, fit_ms)"""
        indptr, indices, values = self._tsne_csr("tsne_gradient", indptr, indices, values)
        y = np.ascontiguousarray(y, dtype=np.float64)
        n = len(indptr) - 1
        if y.ndim != 2 or y.shape[0] != n:
            raise ValueError("tsne_gradient: y is %d x dims" % n)
        grad = np.zeros_like(y)
        a = _lib.TsneArgs(row_tile=int(row_tile), cand_tile=int(cand_tile), slab_rows=int(slab_rows), wave_row_len=int(wave_row_len))
        r = _lib.TsneResult(grad_out=ptr(grad))
        self._check(self.L.crgpu_tsne_gradient_dev(self.h, ptr(indptr), ptr(indices), ptr(values), ptr(y), n, y.shape[1], float(exaggeration),
                                                   C.byref(a), C.byref(r)))
        o = self._tsne_report(r)
        o["grad"] = grad
        return o

    def tsne(self, indptr, indices, values, y, uY=None, gains=None, first_iter=0, n_iters=None, max_iter=_lib.TSNE_MAX_ITER,
             stop_lying_iter=_lib.TSNE_STOP_LYING_ITER, mom_switch_iter=_lib.TSNE_MOM_SWITCH_ITER, eta=_lib.TSNE_ETA, row_tile=0, cand_tile=0,
             slab_rows=0, wave_row_len=0):
        """The descent of bh_tsne on a CSR P on the device (crgpu_tsne_dev): the iterations first_iter .. first_iter + n_iters (default:
        to max_iter) from y [n, 2 or 3], uY (default 0) and gains (default 1); exaggeration 12 before stop_lying_iter, momentum 0.5
        before mom_switch_iter and 0.8 from it on, eta 200.  The inputs are not written.  A run cut into two calls (pass y, uY, gains of
        the first on) equals one call bit for bit.  The seams as Context.tsne_gradient
        -> dict(y, uY, gains f64[n, dims], kl and sum_q at y, loop_ms, repulse_ms, pairs_evaluated, ...)"""
        indptr, indices, values = self._tsne_csr("tsne", indptr, indices, values)
        n = len(indptr) - 1
        y = np.array(y, dtype=np.float64, order="C")
        if y.ndim != 2 or y.shape[0] != n:
            raise ValueError("tsne: y is %d x dims" % n)
        uY = np.zeros_like(y) if uY is None else np.array(uY, dtype=np.float64, order="C")
        gains = np.ones_like(y) if gains is None else np.array(gains, dtype=np.float64, order="C")
        if uY.shape != y.shape or gains.shape != y.shape:
            raise ValueError("tsne: uY and gains have the shape of y")
        n_iters = int(max_iter) - int(first_iter) if n_iters is None else int(n_iters)
        if first_iter < 0 or n_iters < 0:
            raise ValueError("tsne: iterations %d + %d" % (first_iter, n_iters))
        a = _lib.TsneArgs(eta=float(eta), first_iter=int(first_iter), n_iters=n_iters, max_iter=int(max_iter), stop_lying_iter=int(stop_lying_iter),
                          mom_switch_iter=int(mom_switch_iter), row_tile=int(row_tile), cand_tile=int(cand_tile), slab_rows=int(slab_rows),
                          wave_row_len=int(wave_row_len))
        r = _lib.TsneResult()
        self._check(self.L.crgpu_tsne_dev(self.h, ptr(indptr), ptr(indices), ptr(values), n, y.shape[1], ptr(y), ptr(uY), ptr(gains), C.byref(a),
                                          C.byref(r)))
        o = self._tsne_report(r)
        o.update(y=y, uY=uY, gains=gains)
        return o

    @staticmethod
    def _umap_report(r):
        return dict(wmax=r.wmax, fit_ms=r.fit_ms, search_ms=r.search_ms, csr_ms=r.csr_ms, loop_ms=r.loop_ms, nnz=int(r.nnz), n_active=int(r.n_active),
                    n_negative=int(r.n_negative), wave_row_len=int(r.wave_row_len), rows_per_wg=int(r.rows_per_wg), max_steps=int(r.max_steps))

    def umap_graph(self, nn_indices, nn_distances, n_epochs):
        """The fuzzy kNN graph of UMAP on the device (crgpu_umap_graph_dev, csrc/umap.hip) from neighbour indices and dissimilarities
        [n, k] by rank: per row rho (the first distance > 0) and the search for sigma (at most 64 steps, |psum - log2(k + 1)| < 1e-5,
        floored at 1e-3 of the mean distance), the memberships, the union of both directions with the value (a + b) - a * b (twin
        entries carry equal bits), pruned below wmax / n_epochs, CSR with ascending indices
        -> dict(rho f64[n], sigma f64[n], steps u32[n], indptr i64[n + 1], indices i32[nnz], values f64[nnz], wmax, max_steps, nnz,
        fit_ms, search_ms, csr_ms, ...)"""
        ind, dist = np.ascontiguousarray(nn_indices, dtype=np.int32), np.ascontiguousarray(nn_distances, dtype=np.float64)
        if ind.ndim != 2 or ind.shape != dist.shape:
            raise ValueError("umap_graph: indices and distances of one shape [n, k]")
        n, k = ind.shape
        if not 1 <= k <= _lib.KNN_MAX_K or 2 * n * k >= 1 << 32:      # the output arrays need a shape; the library refuses the rest
            raise ValueError("umap_graph: k = %d, 1 to %d, and fewer than 2^31 pairs" % (k, _lib.KNN_MAX_K))
        if not 0 <= int(n_epochs) < 1 << 32:
            raise ValueError("umap_graph: %d epochs" % n_epochs)
        o = dict(rho=np.zeros(n), sigma=np.zeros(n), steps=np.zeros(n, np.uint32), indptr=np.zeros(n + 1, np.int64))
        indices, values = np.zeros(2 * n * k, np.int32), np.zeros(2 * n * k)
        r = _lib.UmapResult(rho_out=ptr(o["rho"]), sigma_out=ptr(o["sigma"]), steps_out=ptr(o["steps"]), indptr_out=ptr(o["indptr"]),
                            indices_out=ptr(indices), values_out=ptr(values))
        self._check(self.L.crgpu_umap_graph_dev(self.h, ptr(ind), ptr(dist), n, k, int(n_epochs), C.byref(r)))
        o.update(self._umap_report(r))
        o.update(indices=indices[:o["nnz"]].copy(), values=values[:o["nnz"]].copy())
        return o

    def umap_epochs(self, indptr, indices, values, y, a, b, seed=0, first_epoch=0, n_run=None, n_epochs=500, epoch_of_next_sample=None,
                    epoch_of_next_negative_sample=None, gamma=1.0, initial_alpha=1.0, negative_sample_rate=_lib.UMAP_NEGATIVE_SAMPLE_RATE,
                    want_delta=False, wave_row_len=0, rows_per_wg=0):
        """The epochs first_epoch .. first_epoch + n_run (default: to n_epochs) of UMAP's layout on a CSR graph on the device
        (crgpu_umap_epochs_dev) in the per-epoch batch form of include/crgpu.h: every term from y [n, 2 or 3] as it stood at the
        epoch's start, negative samples from Philox stream `epoch` with key seed.  At first_epoch 0 the library sets the two schedule
        states; a later call takes those of the call before it.  The inputs are not written.  A run cut into two calls equals one
        call bit for bit.  wave_row_len / rows_per_wg: test seams, no result depends on them
        -> dict(y f64[n, dims], epoch_of_next_sample, epoch_of_next_negative_sample f64[nnz], delta (want_delta: of the last epoch),
        n_active, n_negative, wmax, loop_ms, fit_ms, ...)"""
        indptr, indices, values = self._tsne_csr("umap_epochs", indptr, indices, values)
        n = len(indptr) - 1
        y = np.array(y, dtype=np.float64, order="C")
        if y.ndim != 2 or y.shape[0] != n:
            raise ValueError("umap_epochs: y is %d x dims" % n)
        n_run = int(n_epochs) - int(first_epoch) if n_run is None else int(n_run)
        if first_epoch < 0 or n_run < 0 or n_epochs < 0:
            raise ValueError("umap_epochs: epochs %d + %d of %d" % (first_epoch, n_run, n_epochs))
        if first_epoch and (epoch_of_next_sample is None or epoch_of_next_negative_sample is None):
            raise ValueError("umap_epochs: a call that does not start at epoch 0 takes the two schedule states")
        state = [np.zeros(len(values)) if s is None or not first_epoch else np.array(s, dtype=np.float64, order="C")
                 for s in (epoch_of_next_sample, epoch_of_next_negative_sample)]
        if state[0].shape != values.shape or state[1].shape != values.shape:
            raise ValueError("umap_epochs: the schedule states have one value per entry")
        delta = np.zeros_like(y) if want_delta else None
        args = _lib.UmapArgs(a=float(a), b=float(b), gamma=float(gamma), initial_alpha=float(initial_alpha), seed=int(seed), first_epoch=int(first_epoch),
                             n_run=n_run, n_epochs=int(n_epochs), negative_sample_rate=int(negative_sample_rate), wave_row_len=int(wave_row_len),
                             rows_per_wg=int(rows_per_wg))
        r = _lib.UmapResult(delta_out=ptr(delta) if want_delta else None)
        self._check(self.L.crgpu_umap_epochs_dev(self.h, ptr(indptr), ptr(indices), ptr(values), n, y.shape[1], ptr(y), ptr(state[0]), ptr(state[1]),
                                                 C.byref(args), C.byref(r)))
        o = self._umap_report(r)
        o.update(y=y, epoch_of_next_sample=state[0], epoch_of_next_negative_sample=state[1], delta=delta)
        return o

    def louvain(self, indptr, indices, weights=None, symmetrize=True, max_rounds=None, wave_deg_max=0, lds_deg_max=0, batch=0):
        """Louvain on the device (crgpu_louvain_dev, csrc/louvain.hip): the published algorithm in the synchronous integer rounds of
        include/crgpu.h on a CSR graph.  symmetrize=True (the stage): the union of both directions of an unweighted neighbour matrix,
        weights None; False: a symmetric CSR with ascending columns and weights >= 1 (None = 1).  Two runs and tests/louvain_numpy.py
        agree bit for bit; no parity with bin/louvain.  wave_deg_max / lds_deg_max / batch: test seams, no result depends on them
        -> dict(levels: a list of i32[nodes of the level], nodes, communities, rounds, S: lists per level, M, level0 i32[n], final
        i32[n], nnz, fit_ms, union_ms, rounds_ms, aggregate_ms, level_ms: per level the host time of its rounds, wave_deg_max, lds_deg_max,
        batch)"""
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        if indptr.ndim != 1 or len(indptr) < 2:
            raise ValueError("louvain: indptr of n + 1 elements, n >= 1")
        n = len(indptr) - 1
        raw = np.asarray(indices)
        if raw.size and (raw.min() < -(1 << 31) or raw.max() >= 1 << 31):
            raise ValueError("louvain: an index outside the nodes")
        indices = np.ascontiguousarray(raw, dtype=np.int32)
        if indices.ndim != 1 or len(indices) < indptr[-1]:
            raise ValueError("louvain: indices of indptr[n] elements")
        w = None
        if weights is not None:
            w = np.asarray(weights)
            if w.shape != indices.shape or (w.size and (w.min() < 0 or w.max() >= 1 << 32)):
                raise ValueError("louvain: one u32 weight per entry")
            w = np.ascontiguousarray(w, dtype=np.uint32)
        capacity = 4 * n + 64
        while True:
            flat, level0, final = np.zeros(capacity, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
            per = [np.zeros(_lib.LOUVAIN_MAX_LEVELS, np.uint32) for _ in range(3)] + [np.zeros(_lib.LOUVAIN_MAX_LEVELS, np.int64),
                                                                                          np.zeros(_lib.LOUVAIN_MAX_LEVELS)]
            args = _lib.LouvainArgs(symmetrize=1 if symmetrize else 0, max_rounds=0 if max_rounds is None else int(max_rounds),
                                    wave_deg_max=int(wave_deg_max), lds_deg_max=int(lds_deg_max), batch=int(batch), levels_capacity=capacity)
            r = _lib.LouvainResult(levels_out=ptr(flat), level0_out=ptr(level0), final_out=ptr(final), level_nodes_out=ptr(per[0]),
                                   level_communities_out=ptr(per[1]), level_rounds_out=ptr(per[2]), level_S_out=ptr(per[3]), level_ms_out=ptr(per[4]))
            self._check(self.L.crgpu_louvain_dev(self.h, ptr(indptr), ptr(indices), None if w is None else ptr(w), n, C.byref(args), C.byref(r)))
            if r.levels_needed <= capacity:
                break
            capacity = int(r.levels_needed)      # a pure function of its input: the second call gives the same levels
        nl = int(r.n_levels)
        nodes = [int(v) for v in per[0][:nl]]
        starts = np.concatenate([[0], np.cumsum(nodes)]).astype(np.int64)
        return dict(levels=[flat[starts[l]:starts[l + 1]].copy() for l in range(nl)], nodes=nodes, communities=[int(v) for v in per[1][:nl]],
                    rounds=[int(v) for v in per[2][:nl]], S=[int(v) for v in per[3][:nl]], level_ms=[float(v) for v in per[4][:nl]], M=int(r.M), level0=level0, final=final, nnz=int(r.nnz),
                    fit_ms=r.fit_ms, union_ms=r.union_ms, rounds_ms=r.rounds_ms, aggregate_ms=r.aggregate_ms, wave_deg_max=int(r.wave_deg_max),
                    lds_deg_max=int(r.lds_deg_max), batch=int(r.batch))

    def batch_correct(self, projection, steps, sigma=_lib.CBC_SIGMA, num_pcs=None, want_corr=False, pair_tile=0, row_tile=0, slab_rows=0):
        """a merge schedule of CORRECT_CHEMISTRY_BATCH with the matrix resident on the device (crgpu_batch_correct_dev,
        csrc/batch_correction.hip).  steps: a list of dict(cur_rows, mnn_cur, mnn_ref) (or such triples): per step corr =
        correction_vector(x, cur_rows, mnn_cur, mnn_ref, sigma) from the matrix as it stands, then x[cur_rows] += corr.  No step: the
        matrix comes back bit for bit.  A cur row whose weights all underflow gets NaN, as numpy gives.  pair_tile / row_tile /
        slab_rows: test seams, no result depends on them
        -> dict(aligned f64[n, d], corr (want_corr: a list of f64[n_cur, d]), step_ms f64[steps, 4] = gather, accumulate, finish, apply,
        fit_ms, upload_ms, download_ms, gather_ms, accumulate_ms, finish_ms, apply_ms, pairs_evaluated, chunks, zero_den_rows, pair_tile,
        row_tile)"""
        x = np.ascontiguousarray(projection, dtype=np.float64)
        if x.ndim != 2:
            raise ValueError("batch_correct: the projection is cells x PCs")
        n, ld = x.shape
        d = ld if num_pcs is None else int(num_pcs)
        if not 1 <= d <= ld:
            raise ValueError("batch_correct: %d of %d columns" % (d, ld))
        lists = []
        for s in steps:
            cur, mc, mr = (s["cur_rows"], s["mnn_cur"], s["mnn_ref"]) if isinstance(s, dict) else s
            cur, mc, mr = (np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (cur, mc, mr))
            if len(mc) != len(mr):
                raise ValueError("batch_correct: mnn_cur and mnn_ref pair up")
            lists.append((cur, mc, mr, np.zeros((len(cur), d)) if want_corr else None))
        arr = (_lib.BcStep * max(len(lists), 1))()
        for i, (cur, mc, mr, corr) in enumerate(lists):
            arr[i] = _lib.BcStep(cur_rows=ptr(cur), mnn_cur=ptr(mc), mnn_ref=ptr(mr), corr_out=ptr(corr), n_cur=len(cur), n_mnn=len(mc))
        aligned, step_ms = np.zeros((n, d)), np.zeros((max(len(lists), 1), 4))
        a = _lib.BcArgs(pair_tile=int(pair_tile), row_tile=int(row_tile), slab_rows=int(slab_rows))
        r = _lib.BcResult(step_ms_out=ptr(step_ms))
        self._check(self.L.crgpu_batch_correct_dev(self.h, ptr(x), n, d, ld, float(sigma), arr, len(lists), ptr(aligned), C.byref(a), C.byref(r)))
        o = dict(aligned=aligned, step_ms=step_ms[:len(lists)], fit_ms=r.fit_ms, upload_ms=r.upload_ms, download_ms=r.download_ms, gather_ms=r.gather_ms,
                 accumulate_ms=r.accumulate_ms, finish_ms=r.finish_ms, apply_ms=r.apply_ms, pairs_evaluated=int(r.pairs_evaluated), chunks=int(r.chunks),
                 zero_den_rows=int(r.zero_den_rows), pair_tile=int(r.pair_tile), row_tile=int(r.row_tile))
        if want_corr:
            o["corr"] = [c for _, _, _, c in lists]
        return o

    def pca(self, m, n_components=10, pca_features=None, pca_bc_indices=None, seed=0, min_count_threshold=0, start=None, n_features=None,
            wave_block=0, dot_parts_per_block=0, want_projection=True):
        """run_pca of the filtered MatrixDev `m` (features x barcodes, one feature type: select_features_dev) at ONE threshold on the device
        (csrc/pca.hip): thresholding, the dispersion order of the features, IRLBA on the centred and scaled log matrix, the projection of
        every barcode -> dict(transformed_pca_matrix = projection f64[barcodes, n_components], components f64[n_components, features],
        variance_explained, dispersion (NaN = removed by the threshold), features_selected (rows of m in the order of org_cols_used), d, it,
        mprod, m_b, n_components (reduced to min(features, barcodes) when the threshold is not 2), the counts and the times).
        pca_features None = every thresholded feature; pca_bc_indices: ascending positions among the thresholded barcodes, None = all;
        start: the first Lanczos vector before normalisation (None: RandomState(seed).randn).  MatrixRankTooSmall / NullAxisMatrix as the
        reference raises them.  wave_block / dot_parts_per_block: seams, no result depends on them.  The sign of a component is the
        library's (include/crgpu.h, SIGN OF A COMPONENT), not LAPACK's"""
        if n_features is None:
            n_features = getattr(m, "n_features", None) or getattr(self, "n_features", None)
            if n_features is None:
                raise ValueError("pca: pass n_features")
        G, V, nc = int(n_features), int(m.n_barcodes), int(n_components)
        if not 1 <= nc <= _lib.PCA_MAX_COMPONENTS:      # the output arrays need a shape; the library refuses the rest
            raise ValueError("pca: n_components = %d, 1 to %d" % (nc, _lib.PCA_MAX_COMPONENTS))
        bcs = None if pca_bc_indices is None else np.ascontiguousarray(pca_bc_indices, dtype=np.uint64)
        st = None if start is None else np.ascontiguousarray(start, dtype=np.float64)
        o = dict(transformed_pca_matrix=np.zeros((V, nc)) if want_projection else None, components=np.zeros((nc, G)), variance_explained=np.zeros(nc),
                 dispersion=np.zeros(G), features_selected=np.zeros(G, np.int32), d=np.zeros(nc))
        a = _lib.PcaArgs(pca_bc_indices=ptr(bcs), n_pca_bcs=0 if bcs is None else len(bcs), start=ptr(st), n_start=0 if st is None else len(st),
                         n_components=nc, pca_features=int(pca_features or 0), min_count_threshold=int(min_count_threshold), seed=int(seed),
                         wave_block=int(wave_block), dot_parts_per_block=int(dot_parts_per_block))
        r = _lib.PcaResult(**{k + "_out": ptr(v) for k, v in o.items() if k != "transformed_pca_matrix"})
        r.transformed_out = ptr(o["transformed_pca_matrix"])
        self._check(self.L.crgpu_pca_dev(self.h, m._mv, G, C.byref(a), C.byref(r)))
        if r.status == _lib.PCA_NULL_AXIS:
            raise NullAxisMatrix("pca: no barcode or no feature with a sum above %d" % min_count_threshold)
        if r.status == _lib.PCA_RANK_TOO_SMALL:
            raise MatrixRankTooSmall("Matrix rank is too small")
        nu = int(r.n_components)
        if want_projection:      # the rows were written with the stride of the components used
            o["transformed_pca_matrix"] = np.ascontiguousarray(o["transformed_pca_matrix"].ravel()[:V * nu].reshape(V, nu))
        o["components"] = np.ascontiguousarray(o["components"].ravel()[:nu * G].reshape(nu, G))
        o["variance_explained"], o["d"] = o["variance_explained"][:nu], o["d"][:nu]
        o["features_selected"] = o["features_selected"][:int(r.n_used_features)]
        o.update(projection=o["transformed_pca_matrix"], n_components=nu, it=int(r.it), mprod=int(r.mprod), m_b=int(r.m_b),
                 n_used_features=int(r.n_used_features), n_thresholded_features=int(r.n_thresholded_features),
                 n_thresholded_barcodes=int(r.n_thresholded_barcodes), n_pca_barcodes=int(r.n_pca_barcodes), min_count_threshold=int(min_count_threshold),
                 fit_ms=r.fit_ms, prepare_ms=r.prepare_ms, lanczos_ms=r.lanczos_ms, project_ms=r.project_ms)
        return o

    def sseq_params(self, m, n_features=None):
        """compute_sseq_params of the MatrixDev `m` (features x cells, one feature type: select_features_dev) on the device
        (csrc/sseq.h) -> SseqParams; n_features = the rows of m (default: what select_features_dev left, else the context's n_features)"""
        if n_features is None:
            n_features = getattr(m, "n_features", None) or getattr(self, "n_features", None)
            if n_features is None:
                raise ValueError("sseq_params: pass n_features")
        a = _lib.SseqArgs(n_features=int(n_features))
        h = C.c_void_p()
        self._check(self.L.crgpu_sseq_params_dev(self.h, m._mv, C.byref(a), C.byref(h)))
        self.sseq_params_computed = getattr(self, "sseq_params_computed", 0) + 1
        return SseqParams(self, h, m.n_barcodes, int(n_features))

    def sseq_diffexp(self, m, params, clusters, n_clusters=None, wave_min=0, wg_min=0):
        """sseq_differential_expression of every cluster (1-based labels i32[cells]) against all other cells -> dict of [K, G] arrays
        sums_in, sums_out (u64), norm_mean_in, norm_mean_out, log2_fold_change, p_values, adjusted_p_values (f64), below_median (u8: the
        side of the median an asymptotic test took, 255 = none), per cluster s_a, s_b, n_exact, n_asymptotic, the counts n_terms, n_short,
        n_wave, n_workgroup, the times ms_*, and data f64[G, 3 K] = per cluster norm_mean_in, log2_fold_change, adjusted_p_values.
        wave_min / wg_min: the class thresholds of the exact tests (0 = default); no result depends on them"""
        lab = np.ascontiguousarray(clusters, dtype=np.int32)
        if lab.ndim != 1 or len(lab) != m.n_barcodes:
            raise ValueError("sseq_diffexp: one label per cell")
        K = int(lab.max()) if n_clusters is None and len(lab) else int(n_clusters or 0)
        G = params.n_features
        Ka = max(K, 1)
        o = dict(sums_in=np.zeros((Ka, G), np.uint64), sums_out=np.zeros((Ka, G), np.uint64), norm_mean_in=np.zeros((Ka, G)),
                 norm_mean_out=np.zeros((Ka, G)), log2_fold_change=np.zeros((Ka, G)), p_values=np.zeros((Ka, G)),
                 adjusted_p_values=np.zeros((Ka, G)), below_median=np.zeros((Ka, G), np.uint8), s_a=np.zeros(Ka), s_b=np.zeros(Ka),
                 n_exact=np.zeros(Ka, np.uint64), n_asymptotic=np.zeros(Ka, np.uint64))
        r = _lib.SseqResult(**{("below_median_out" if k == "below_median" else k + "_out"): ptr(v) for k, v in o.items()})
        a = _lib.SseqArgs(n_features=G, wave_min=int(wave_min), wg_min=int(wg_min))
        self._check(self.L.crgpu_sseq_diffexp_dev(self.h, m._mv, params._h, ptr(lab), K, C.byref(a), C.byref(r)))
        o.update(n_clusters=K, n_terms=int(r.n_terms), n_short=int(r.n_short), n_wave=int(r.n_wave), n_workgroup=int(r.n_workgroup),
                 ms_sums=r.ms_sums, ms_exact=r.ms_exact, ms_asymptotic=r.ms_asymptotic, ms_bh=r.ms_bh)
        data = np.zeros((G, 3 * K))
        data[:, 0::3], data[:, 1::3], data[:, 2::3] = o["norm_mean_in"].T, o["log2_fold_change"].T, o["adjusted_p_values"].T
        o["data"] = data
        return o

    def sseq_pairs(self, m, groups, n_groups=None, n_features=None):
        """The plan of the local sSeq tests of one MatrixDev and one grouping of its cells (crgpu_sseq_pairs_create_dev, csrc/sseq_pair.h):
        groups i32[cells], -1 = a cell in no group, else 0 .. n_groups - 1 (default: the largest + 1), every group with a cell.  The
        entries of the grouped cells are sorted into (gene, group, cell) order once -> SseqPairs; n_features as Context.sseq_params"""
        if n_features is None:
            n_features = getattr(m, "n_features", None) or getattr(self, "n_features", None)
            if n_features is None:
                raise ValueError("sseq_pairs: pass n_features")
        g = np.ascontiguousarray(groups, dtype=np.int32)
        if g.ndim != 1 or len(g) != m.n_barcodes:
            raise ValueError("sseq_pairs: one group per cell")
        K = (int(g.max()) + 1 if len(g) else 0) if n_groups is None else int(n_groups)
        a = _lib.SseqPairArgs(n_features=int(n_features))
        h = C.c_void_p()
        self._check(self.L.crgpu_sseq_pairs_create_dev(self.h, m._mv, ptr(g), max(K, 0), C.byref(a), C.byref(h)))
        return SseqPairs(self, h, K, int(n_features))

    def cluster_medians(self, projection, labels, n_clusters=None, num_pcs=None):
        """np.median of every column of the f64 projection [rows x PCs] over the rows of every cluster (labels 0 .. n_clusters - 1, every
        cluster with a row) by an exact radix select on the device (crgpu_cluster_medians_dev, csrc/merge_clusters.hip): the medoids of
        MERGE_CLUSTERS -> dict(medians f64[K, d], sizes u64[K])"""
        x = np.ascontiguousarray(projection, dtype=np.float64)
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if x.ndim != 2 or lab.ndim != 1 or len(lab) != x.shape[0]:
            raise ValueError("cluster_medians: the projection is rows x PCs, one label per row")
        n, ld = x.shape
        d = ld if num_pcs is None else int(num_pcs)
        K = (int(lab.max()) + 1 if n else 0) if n_clusters is None else int(n_clusters)
        if not 1 <= K <= _lib.SSEQ_MAX_K or not 1 <= d <= ld:      # the output needs a shape; the library refuses the rest
            raise ValueError("cluster_medians: %d clusters (1 to %d), %d of %d columns" % (K, _lib.SSEQ_MAX_K, d, ld))
        med, sizes = np.zeros((K, d)), np.zeros(K, np.uint64)
        self._check(self.L.crgpu_cluster_medians_dev(self.h, ptr(x), n, d, ld, ptr(lab), K, ptr(med), ptr(sizes)))
        return dict(medians=med, sizes=sizes)

    def tag_moments(self, m, tag_rows, n_features=None):
        """the exact sums over the cells of x, x^2 and x y for the listed tag rows (at most 16) -> (u64[n], u64[n], u64[n, n])"""
        rows = np.ascontiguousarray(tag_rows, dtype=np.uint32)
        if n_features is None:
            n_features = getattr(self, "n_features", None)
            if n_features is None:
                raise ValueError("tag_moments: pass n_features")
        n = len(rows)
        sx, sxx, sxy = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros((n, n), np.uint64)
        self._check(self.L.crgpu_tag_moments_dev(self.h, m._mv, ptr(rows), n, int(n_features), ptr(sx), ptr(sxx), ptr(sxy)))
        return sx, sxx, sxy

    def jibes_fit(self, y, bg, fg, sd, n_gems=N_G, estimated_cells=None, blank_prob=0.04, freqs=None, max_k_lets=3, max_reps=50000, abs_tol=1e-2,
                  rel_tol=1e-7, confidence=JIBES_MIN_CONFIDENCE, exclude_blanks_from_posterior=False, apply_confidence=True, want_posterior=False):
        """perform_EM of jibes_o3 and get_assignment_df on the device: y f64[n, k] = log10(count + 1), (bg, fg, sd) the initial model.
        -> dict(bg, fg, sd, LL, iterations, converged, n_states, k_let_limited, fit_ms, states u8[z, k], prior, estimated_cells,
        probs f64[n, k + 2] (tags, Multiplet, Blank), assignment i32[n] (a tag, k = Multiplet, k + 1 = Blank, k + 2 = Unassigned),
        assignment_prob, ml_state (index of the most likely Multiplet state); want_posterior adds posterior f64[n, z] (tests)."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.ndim != 2:
            raise ValueError("jibes_fit: y is n x k")
        n, k = y.shape
        m0 = [np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (bg, fg, sd)]
        if any(len(a) != k for a in m0):
            raise ValueError("jibes_fit: the initial model has one value per tag")
        fr = None if freqs is None else np.ascontiguousarray(freqs, dtype=np.float64)
        if estimated_cells is None:
            estimated_cells = jibes_expected_cells(n, n_gems)
        a = _lib.JibesFitArgs(bg=ptr(m0[0]), fg=ptr(m0[1]), sd=ptr(m0[2]), freqs=ptr(fr), blank_prob=blank_prob, estimated_cells=estimated_cells,
                              abs_tol=abs_tol, rel_tol=rel_tol, confidence=confidence, n_gems=n_gems, max_k_lets=max_k_lets, max_reps=max_reps,
                              flags=(_lib.JIBES_EXCLUDE_BLANKS if exclude_blanks_from_posterior else 0) | (0 if apply_confidence else _lib.JIBES_NO_CONFIDENCE),
                              reserved=0)
        res = _lib.JibesFitResult()
        post = None
        lat = jibes_latent_states(n, k, n_gems, max_k_lets, estimated_cells, blank_prob, fr)      # refuses k > 16 and max_k_lets > 3 as the fit would
        z = len(lat["states"])
        probs, asst, aprob, ml = np.zeros((n, k + 2)), np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.uint32)
        if want_posterior:
            post = np.zeros((n, z))
        if n:
            a.probs_out, a.assignment_out, a.assignment_prob_out, a.ml_state_out, a.posterior_out = ptr(probs), ptr(asst), ptr(aprob), ptr(ml), ptr(post)
        self._check(self.L.crgpu_jibes_fit_dev(self.h, ptr(y) if n else None, n, k, C.byref(a), C.byref(res)))
        out = dict(bg=np.array(res.bg[:k]), fg=np.array(res.fg[:k]), sd=np.array(res.sd[:k]), LL=res.ll, iterations=int(res.iterations),
                   converged=bool(res.converged), n_states=int(res.n_states), k_let_limited=bool(res.k_let_limited), fit_ms=res.fit_ms,
                   states=lat["states"], prior=lat["prior"], estimated_cells=estimated_cells, probs=probs, assignment=asst, assignment_prob=aprob,
                   ml_state=ml)
        if want_posterior:
            out["posterior"] = post
        return out

    def multigenome_jibes(self, counts0, counts1, n_gems=N_G):
        """JIBESMultiGenome._infer_multiplets (analysis/jibes.py:396-442): the two count vectors as log10(count + 1), the initial
        calls from the device classify_gems, the fit with its defaults and no confidence rule
        -> (observed multiplets, infer_multiplets_from_observed, calls u8 per barcode as _lib.MG_*)"""
        c0, c1 = (np.ascontiguousarray(x.to_host(x.size) if isinstance(x, DeviceArray) else x, dtype=np.uint32) for x in (counts0, counts1))
        if len(c0) != len(c1):
            raise ValueError("multigenome_jibes: counts0 and counts1 differ in length")
        first = self.multigenome(c0, c1, bootstraps=1).call
        if len(set(first.tolist())) <= 1:
            return 0, 0.0, first
        y = np.stack((np.log10(c0 + 1.0), np.log10(c1 + 1.0)), axis=1)
        calls = np.where(first == _lib.MG_GENOME0, 0, np.where(first == _lib.MG_GENOME1, 1, -1)).astype(np.int32)
        bg, fg, sd = jibes_initial_parameters(y, calls)
        fit = self.jibes_fit(y, bg, fg, sd, n_gems=n_gems, apply_confidence=False)
        a = fit["assignment"]
        m, g0, g1 = int((a == 2).sum()), int((a == 0).sum()), int((a == 1).sum())
        call = np.where(a == 0, _lib.MG_GENOME0, np.where(a == 1, _lib.MG_GENOME1, np.where(a == 2, _lib.MG_MULTIPLET, 255))).astype(np.uint8)
        return m, float(multigenome_summary(np.array([[m, g0, g1]], np.int64), len(c0))[0][0]), call

    def call_additional_cells(self, m, call, low, high, emptydrops_minimum_umis=500, num_sims=10000, max_adj_pvalue=0.01, seed=0,
                              feature_mask=None, sim_table=None, keep_sim_table=False, keep_profile=True):
        """find_nonambient_barcodes (cell_calling.py:144-263) behind the initial call `call` (CellCall) on the MatrixDev `m`:
        the ambient profile from places [low, high) of the descending totals (get_empty_drops_range), the candidates above
        max(emptydrops_minimum_umis, 1 + max_background_umis), their p-values from num_sims simulations on the device (seed:
        the Philox key) or from sim_table = (sim_n, sim_loglk) of the reference's simulate_multinomial_loglikelihoods, BH and
        the merged call -> AdditionalCells.  feature_mask: the rows of one genome / library type (crgpu.h)."""
        mask = None if feature_mask is None else np.ascontiguousarray(np.asarray(feature_mask) != 0, dtype=np.uint8)
        d_counts = self.column_sums(m, mask)
        sim_n = sim_ll = None
        if sim_table is not None:
            sim_n = np.ascontiguousarray(sim_table[0], dtype=np.int64)
            sim_ll = np.ascontiguousarray(sim_table[1], dtype=np.float64)
            if sim_ll.shape != (len(sim_n), num_sims):
                raise ValueError("sim_table: sim_loglk must be len(sim_n) x num_sims")
        flags = (_lib.ED_KEEP_PROFILE if keep_profile else 0) | (_lib.ED_KEEP_SIM_TABLE if keep_sim_table and sim_table is None else 0)
        res, arr = _lib.EmptydropsResult(), _lib.EmptydropsArrays()
        self._check(self.L.crgpu_emptydrops_dev(self.h, m._mv, ptr(mask), 0 if mask is None else len(mask), _p(d_counts), _p(call.cols),
                                                call.n_cells, low, high, emptydrops_minimum_umis, num_sims, max_adj_pvalue, seed,
                                                ptr(sim_n), 0 if sim_n is None else len(sim_n), ptr(sim_ll), flags, C.byref(res),
                                                C.byref(arr)))
        return AdditionalCells(self, res, arr, call, m)

    def ambient_pvalues(self, umis, obs_loglk, sim_n, sim_loglk, max_adj_pvalue=0.01):
        """compute_ambient_pvalues (stats.py:205-231) + adjust_pvalue_bh + the calls against a simulated table ->
        (n_lower, pvalues, pvalues_adj, is_nonambient) as numpy arrays"""
        umis, obs = np.ascontiguousarray(umis, dtype=np.uint32), np.ascontiguousarray(obs_loglk, dtype=np.float64)
        sim_n, tab = np.ascontiguousarray(sim_n, dtype=np.int64), np.ascontiguousarray(sim_loglk, dtype=np.float64)
        assert tab.ndim == 2 and tab.shape[0] == len(sim_n) and len(umis) == len(obs)
        n = len(umis)
        d_nl, d_p, d_q, d_c = self.empty(n, np.uint32), self.empty(n, np.float64), self.empty(n, np.float64), self.empty(n, np.uint8)
        d_umis, d_obs, d_tab = self.upload(umis), self.upload(obs), self.upload(tab.ravel())    # named: alive until the call is over
        called = C.c_uint64()
        self._check(self.L.crgpu_ambient_pvalues_dev(self.h, _p(d_umis), _p(d_obs), n, ptr(sim_n), len(sim_n), _p(d_tab), tab.shape[1],
                                                     max_adj_pvalue, _p(d_nl), _p(d_p), _p(d_q), _p(d_c), C.byref(called)))
        return d_nl.to_host(n), d_p.to_host(n), d_q.to_host(n), d_c.to_host(n).astype(bool)

    def emptydrops_simulate(self, profile_p, umis, num_sims, seed=0, obs_loglk=None, keep_table=True):
        """the simulation kernel of call_additional_cells on its own (test and measurement hook): -> (sim_n, sim_loglk or
        None, n_lower or None, kernel milliseconds)"""
        p = np.ascontiguousarray(profile_p, dtype=np.float64)
        u = np.ascontiguousarray(umis, dtype=np.uint32)
        obs = None if obs_loglk is None else np.ascontiguousarray(obs_loglk, dtype=np.float64)
        d = len(np.unique(u))
        sim_n, tab = np.zeros(len(u), np.int64), (np.zeros((d, num_sims), np.float64) if keep_table else None)
        nl = None if obs is None else np.zeros(len(u), np.uint32)
        nd, ms = C.c_uint32(), C.c_double()
        self._check(self.L.crgpu_emptydrops_simulate_dev(self.h, ptr(p), len(p), ptr(u), ptr(obs), len(u), num_sims, seed, ptr(sim_n),
                                                         C.byref(nd), ptr(tab), ptr(nl), C.byref(ms)))
        assert nd.value == d
        return sim_n[:d].copy(), tab, nl, ms.value

    def mt19937_stream(self, seed, n_words):
        """the generator kernel of the cell call on its own: (DeviceArray of the first n_words outputs of
        np.random.RandomState(seed)'s raw stream, rounded down to whole chunks; kernel milliseconds)"""
        out = self.empty(max(n_words, 1), np.uint32)
        n, ms = C.c_uint64(), C.c_double()
        self._check(self.L.crgpu_mt19937_stream_dev(self.h, seed, n_words, _p(out), C.byref(n), C.byref(ms)))
        out.shape = (n.value,)
        return out, ms.value

    def trim_molecule_barcodes(self, d_barcode_idx, n_molecules, n_barcodes, pass_filter_idx=None, pass_only=False, offset=0):
        """MERGE_MOLECULES on barcode_idx (crgpu.h): rewrites the device column in place; returns (retained old indices,
        rewritten pass_filter indices)"""
        pf = np.zeros(0, np.uint64) if pass_filter_idx is None else np.ascontiguousarray(pass_filter_idx, dtype=np.uint64).copy()
        retained = np.zeros(n_barcodes, np.uint64)
        n = C.c_uint64()
        self._check(self.L.crgpu_trim_molecule_barcodes_dev(self.h, _p(d_barcode_idx), n_molecules, n_barcodes, ptr(pf) if len(pf) else None,
                                                            len(pf), int(pass_only), offset, ptr(retained), C.byref(n)))
        return retained[: n.value], pf

    def concat_matrices(self, mats, gem_groups):
        """merged matrix of several GEM wells: column concatenation in (gem_group, barcode) order"""
        arr = (C.c_void_p * len(mats))(*[C.cast(m._mv, C.c_void_p) for m in mats])
        gg = np.ascontiguousarray(gem_groups, dtype=np.uint16)
        mv = C.POINTER(MatrixView)()
        self._check(self.L.crgpu_concat_matrices(self.h, arr, ptr(gg), len(mats), C.byref(mv)))
        return Matrix(self, mv)

    def assemble_matrix(self, bc, feature, count, n_features):
        bc = np.ascontiguousarray(bc, np.uint32)
        ft = np.ascontiguousarray(feature, np.uint32)
        ct = np.ascontiguousarray(count, np.uint32)
        mv = C.POINTER(MatrixView)()
        self._check(self.L.crgpu_assemble_matrix(self.h, ptr(bc), ptr(ft), ptr(ct), len(bc), n_features, C.byref(mv)))
        return Matrix(self, mv)

    def assemble_matrix_dev(self, d_bc, d_feature, d_count, n_triplets):
        mv = C.POINTER(_lib.MatrixDevView)()
        self._check(self.L.crgpu_assemble_matrix_dev(self.h, _p(d_bc), _p(d_feature), _p(d_count), n_triplets, C.byref(mv)))
        return MatrixDev(self, mv)

    def count(self, recs, n_features):
        mv = C.POINTER(MatrixView)()
        self._check(self.L.crgpu_count(self.h, C.byref(recs), n_features, C.byref(mv)))
        return Matrix(self, mv)

    # ---- feature barcodes ----------------------------------------------------------------------------
    def set_feature_pattern(self, pattern, feat_seqs, feat_index, feat_dist=None):
        s = ascii_matrix(feat_seqs)
        ix = np.ascontiguousarray(feat_index, dtype=np.uint32)
        d = None if feat_dist is None else np.ascontiguousarray(feat_dist, dtype=np.float64)
        self._check(self.L.crgpu_set_feature_pattern(self.h, pattern, s.tobytes(), s.shape[0], s.shape[1], ptr(ix), ptr(d)))

    def match_features(self, pattern, d_seq, d_qualn, n, d_feature_out):
        self._check(self.L.crgpu_match_features_dev(self.h, pattern, _p(d_seq), _p(d_qualn), n, _p(d_feature_out)))

    # ---- segmented barcode constructs (GelBeadAndProbe) ---------------------------------------------------
    def set_barcode_segments(self, lib, seg_seqs, seg_lens):
        """seg_seqs: per segment the packed sequences, ascending (a segment context's canonical list)"""
        k = len(seg_seqs)
        keep = [np.ascontiguousarray(a, dtype=np.uint32) for a in seg_seqs]
        n = (C.c_uint32 * k)(*[len(a) for a in keep])
        ln = (C.c_uint32 * k)(*seg_lens)
        pp = (C.c_void_p * k)(*[a.ctypes.data for a in keep])
        self._check(self.L.crgpu_set_barcode_segments(self.h, lib, k, n, ln, pp))
        self.cb_len, self.n_canon = int(sum(seg_lens)), int(np.prod([len(a) for a in keep], dtype=np.int64))
        self.rtl_n_probe = len(keep[-1]) if k >= 2 else 0  # the probe segment of a GelBeadAndProbe construct

    def combine_segments(self, lib, d_seg_idx, n, d_idx_inout, after_correction=False):
        pp = (C.c_void_p * len(d_seg_idx))(*[_p(a) for a in d_seg_idx])
        self._check(self.L.crgpu_combine_segments_dev(self.h, lib, pp, len(d_seg_idx), n, int(after_correction), _p(d_idx_inout)))

    # whole reads, every pattern form (FeatureExtractor::match_read)
    def set_feature_extractor(self, extractor, defs, feat_dist=None):
        """defs: [(pattern, sequence, FeatureDef::index, read)] of ONE feature type, read 0 = R1, 1 = R2"""
        keep = [(p.encode(), s.encode()) for p, s, _, _ in defs]
        arr = (_lib.FeatureDef * len(defs))()
        for k, (_, _, index, read) in enumerate(defs):
            arr[k] = _lib.FeatureDef(keep[k][0], keep[k][1], index, read)
        d = None if feat_dist is None else np.ascontiguousarray(feat_dist, dtype=np.float64)
        self._check(self.L.crgpu_set_feature_extractor(self.h, extractor, arr, len(defs), ptr(d), 0 if d is None else len(d)))

    def feature_extractor_regexes(self, extractor):
        n = C.c_uint32(0)
        self._check(self.L.crgpu_feature_extractor_regex(self.h, extractor, 0, None, 0, C.byref(n)))
        out = []
        for p in range(n.value):
            buf = C.create_string_buffer(1 << 20)
            self._check(self.L.crgpu_feature_extractor_regex(self.h, extractor, p, buf, 1 << 20, None))
            out.append(buf.value.decode())
        return out

    def extract_features(self, extractor, n, d_feature_out, r1=None, r2=None, d_n_ids_out=None, d_capture_out=None):
        """r1 / r2: (d_seq_rows, d_qual_rows, d_len or None, stride) or None"""
        a = r1 or (None, None, None, 0)
        b = r2 or (None, None, None, 0)
        self._check(self.L.crgpu_extract_features_dev(self.h, extractor, _p(a[0]), _p(a[1]), _p(a[2]), a[3], _p(b[0]), _p(b[1]),
                                                      _p(b[2]), b[3], n, _p(d_feature_out), _p(d_n_ids_out), _p(d_capture_out)))

    def feature_counts(self, d_feature, n, n_features, counts=None):
        """MAKE_SHARD's feature_counts (make_shard_metrics.rs:336-345): counts[f] += reads whose feature is f"""
        counts = np.zeros(n_features, np.int64) if counts is None else counts
        self._check(self.L.crgpu_feature_counts_dev(self.h, _p(d_feature), n, n_features, ptr(counts)))
        return counts

    def synth_rows(self, seed, first, n, d_feature, feat_seq, L, offset, row_stride, d_seq_rows, d_qual_rows, err=0.005, n_rate=0.0005):
        """Feature Barcoding read rows on the device (crgpu_synth_rows_dev); feat_seq: packed u64 sequences"""
        fs = np.ascontiguousarray(feat_seq, dtype=np.uint64)
        self._check(self.L.crgpu_synth_rows_dev(self.h, seed, first, n, _p(d_feature), ptr(fs), len(fs), L, offset, row_stride,
                                                int(round(err * 65536)), int(round(n_rate * (1 << 20))), _p(d_seq_rows), _p(d_qual_rows)))

    # ---- synthetic data --------------------------------------------------------------------------------
    def synth(self, params, first, n, cb=None, cb_qualn=None, umi=None, umi_qualn=None, feature=None, flags=None):
        o = SynthOut()
        o.cb, o.cb_qualn, o.umi, o.umi_qualn = _p(cb), _p(cb_qualn), _p(umi), _p(umi_qualn)
        o.feature, o.flags = _p(feature), _p(flags)
        self._check(self.L.crgpu_synth_dev(self.h, C.byref(params.c), first, n, C.byref(o)))
