"""ctypes binding of libcrgpu.so (include/crgpu.h).

There is no CPU fallback: if the HIP library is missing or no gfx950 device is visible, loading or
`Context()` raises.  Nothing here imports the oracle.
"""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
# CRGPU_LIB_PATH: load another build of the same library (A/B timing of kernel variants on one box)
LIB_PATH = os.environ.get("CRGPU_LIB_PATH") or os.path.join(PKG, "libcrgpu.so")

MISS = 0xFFFFFFFF
NO_FEATURE = 0xFFFFFFFF
MAX_LIB = 16
FLAG_LIB_MASK = 0x0F
FLAG_CB_HAS_N = 0x10
FLAG_NONTXOMIC = 0x20

COUNTS_VALID, COUNTS_CORRECTED, COUNTS_PRIOR = 0, 1, 2
T_NAMES = ["pack", "match", "correct", "keys", "sort_scatter", "dedup", "matrix", "synth", "sort_hist", "scan", "comm", "feature"]
UNIQUE_ID_BYTES = 128
OPT_BUFFERS_UNCHANGED_BETWEEN_CALLS = 0
STAT_SORT_REFINISHED = 1
STAT_RL_COUNTS_FROM_FINISH = 15


class CrgpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("crgpu error %d: %s" % (code, msg))
        self.code = code


class Records(C.Structure):
    _fields_ = [
        ("n", C.c_uint64),
        ("umi_len", C.c_uint32),
        ("d_bc_idx", C.c_void_p),
        ("d_umi", C.c_void_p),
        ("d_umi_qualn", C.c_void_p),
        ("d_feature", C.c_void_p),
        ("d_flags", C.c_void_p),
        ("d_umi_len", C.c_void_p),
        ("d_probe_idx", C.c_void_p),
    ]


class MatrixView(C.Structure):
    _fields_ = [
        ("n_barcodes", C.c_uint64),
        ("nnz", C.c_uint64),
        ("n_features", C.c_uint32),
        ("cb_len", C.c_uint32),
        ("barcode_rank", C.c_void_p),
        ("barcode_seq", C.c_void_p),
        ("indptr", C.c_void_p),
        ("indices", C.c_void_p),
        ("data", C.c_void_p),
        ("gem_group", C.c_void_p),
        ("barcode_seq_hi", C.c_void_p),
    ]


class MatrixDevView(C.Structure):
    _fields_ = [
        ("n_barcodes", C.c_uint64),
        ("nnz", C.c_uint64),
        ("d_barcode_rank", C.c_void_p),
        ("d_indptr", C.c_void_p),
        ("d_indices", C.c_void_p),
        ("d_data", C.c_void_p),
    ]


SHARD_METRIC_FIELDS = ["sequenced_reads", "bc_n_bases", "bc_bases", "umi_n_bases", "umi_bases", "bc_q30_bases", "bc_q30_den",
                       "umi_q30_bases", "umi_q30_den", "good_umi", "has_n_barcode", "has_n_umi", "homopolymer_barcode",
                       "homopolymer_umi", "low_min_qual_barcode", "low_min_qual_umi", "miss_whitelist_barcode", "polyt_suffix_umi"]


class ShardMetrics(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in SHARD_METRIC_FIELDS]


class RowsMetrics(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("n_bases", "bases", "q30_bases", "q30_den")]


# crgpu_dupinfo (crgpu_count_host's per-read output) as a numpy record
DUPINFO_DTYPE = np.dtype([("processed_umi", np.uint32), ("read_count", np.uint32), ("flags", np.uint8), ("reserved", np.uint8, (3,))])
NO_PROBE = -1
ABI_VERSION = 3

# crgpu_barcode_summary_row as a numpy record
BARCODE_SUMMARY_DTYPE = np.dtype([("barcode_rank", np.uint32), ("library", np.uint32), ("reads", np.uint64), ("umis", np.uint64),
                                  ("candidate_dup_reads", np.uint64), ("umi_corrected_reads", np.uint64)])


class SynthParams(C.Structure):
    _fields_ = [
        ("seed", C.c_uint64),
        ("cb_len", C.c_uint32),
        ("umi_len", C.c_uint32),
        ("n_wl", C.c_uint32),
        ("wl_packed", C.c_void_p),
        ("n_cells", C.c_uint32),
        ("cell_wl_pos", C.c_void_p),
        ("cell_cdf", C.c_void_p),
        ("n_ambient", C.c_uint32),
        ("ambient_wl_pos", C.c_void_p),
        ("n_genes", C.c_uint32),
        ("gene_cdf", C.c_void_p),
        ("ambient_per_2_16", C.c_uint32),
        ("cb_err_per_2_16", C.c_uint32),
        ("umi_err_per_2_16", C.c_uint32),
        ("n_per_2_20", C.c_uint32),
        ("no_feature_per_2_16", C.c_uint32),
        ("reads_per_umi", C.c_uint32),
        ("n_total", C.c_uint64),
        ("n_libs", C.c_uint32),
    ]


class SynthOut(C.Structure):
    _fields_ = [
        ("cb", C.c_void_p),
        ("cb_qualn", C.c_void_p),
        ("umi", C.c_void_p),
        ("umi_qualn", C.c_void_p),
        ("feature", C.c_void_p),
        ("flags", C.c_void_p),
    ]


class BcCorrectionMetrics(C.Structure):
    _fields_ = [("valid_reads", C.c_uint64), ("corrected_reads", C.c_uint64), ("barcodes_detected", C.c_uint64),
                ("effective_barcode_diversity", C.c_double)]


ORDMAG_SAMPLES = 100


class OrdmagResult(C.Structure):
    """crgpu_ordmag_result"""
    _fields_ = [
        ("n_nonzero", C.c_uint64),
        ("recovered_cells", C.c_int64),
        ("recovered_boot", C.c_int64 * ORDMAG_SAMPLES),
        ("loss_boot", C.c_double * ORDMAG_SAMPLES),
        ("baseline_bc_idx", C.c_int64),
        ("top_n_boot", C.c_int64 * ORDMAG_SAMPLES),
        ("filtered_bcs_mean", C.c_double),
        ("filtered_bcs_var", C.c_double),
        ("filtered_bcs_cv", C.c_double),
        ("filtered_bcs_lb", C.c_double),
        ("filtered_bcs_ub", C.c_double),
        ("filtered_bcs", C.c_int64),
        ("filtered_bcs_cutoff", C.c_int64),
        ("filtered_bcs_cutoff_set", C.c_int32),
        ("estimated", C.c_int32),
    ]


class EmptydropsResult(C.Structure):
    """crgpu_emptydrops_result"""
    _fields_ = [
        ("status", C.c_int32),
        ("sim_in_lds", C.c_int32),
        ("n_ambient_used", C.c_uint64),
        ("max_background_umis", C.c_uint64),
        ("emptydrops_minimum_umis", C.c_uint64),
        ("n_eval_features", C.c_uint64),
        ("n_candidates", C.c_uint64),
        ("n_distinct_n", C.c_uint64),
        ("n_nonambient", C.c_uint64),
        ("sgt_slope", C.c_double),
        ("sgt_p0", C.c_double),
        ("sim_ms", C.c_double),
    ]


class EmptydropsArrays(C.Structure):
    """crgpu_emptydrops_arrays"""
    _fields_ = [(n, C.c_uint64) for n in ("n_candidates", "n_called", "n_eval_features", "n_distinct_n", "num_sims")] + [
        (n, C.c_void_p) for n in ("d_eval_cols", "d_umis", "d_obs_loglk", "d_n_lower", "d_pvalues", "d_pvalues_adj", "d_is_nonambient",
                                  "d_called_cols", "d_eval_features", "d_profile_p", "d_sim_n", "d_sim_loglk")]


class SubsampleArgs(C.Structure):
    """crgpu_subsample_args"""
    _fields_ = [(n, C.c_uint32) for n in ("n_tasks", "n_genomes", "n_libs", "n_features")] + [("n_cells", C.c_uint64), ("seed", C.c_uint64)] + [
        (n, C.c_void_p) for n in ("rates", "task_type", "d_cell_ranks", "cell_genome_mask", "feature_genome", "feature_mask", "umis_per_bc",
                                  "read_pairs_per_bc", "features_det_per_bc", "read_pairs", "umis", "total_features_det", "any_reads")]


class SubsampleResult(C.Structure):
    """crgpu_subsample_result"""
    _fields_ = [(n, C.c_uint64) for n in ("n_molecules", "n_groups", "n_lane", "n_wave", "n_workgroup")] + [
        ("n_active_tasks", C.c_uint32), ("n_batches", C.c_uint32), ("draw_ms", C.c_double)]


class NormalizeDepthArgs(C.Structure):
    """crgpu_normalize_depth_args"""
    _fields_ = [(n, C.c_uint32) for n in ("n_libs", "n_features", "n_classes", "reserved")] + [("n_cells", C.c_uint64), ("seed", C.c_uint64)] + [
        (n, C.c_void_p) for n in ("frac_reads_kept", "feature_class", "d_cell_ranks", "cell_class_mask", "matrix", "raw_mapped_reads",
                                  "flt_mapped_reads", "reads_per_lib", "kept_reads_per_lib", "kept_molecules_per_lib", "kept_out")]


class NormalizeDepthResult(C.Structure):
    """crgpu_normalize_depth_result"""
    _fields_ = [(n, C.c_uint64) for n in ("n_molecules", "n_lane", "n_wave", "n_workgroup", "n_kept_molecules", "n_triplets")] + [
        ("draw_ms", C.c_double), ("tally_ms", C.c_double)]


class MultigenomeResult(C.Structure):
    """crgpu_multigenome_result"""
    _fields_ = [("n", C.c_uint64), ("obs_thresh0", C.c_double), ("obs_thresh1", C.c_double)] + [
        (n, C.c_int64) for n in ("observed_multiplets", "observed_genome0", "observed_genome1")] + [
        (n, C.c_uint64) for n in ("sum_c0_genome0", "sum_all_genome0", "sum_c1_genome1", "sum_all_genome1", "sum_max_single", "sum_all_single")] + [
        (n, C.c_double) for n in ("purity0", "purity1", "purity_overall", "boot_mean")] + [("inferred_multiplets", C.c_int64)] + [
        (n, C.c_double) for n in ("multiplet_rate", "normalized_multiplet_rate", "multiplet_rate_lb", "multiplet_rate_ub")] + [
        ("generator_words", C.c_uint64), ("obs_branch", C.c_int32), ("rate_bounds_set", C.c_int32)]


class RtlGemRuns(C.Structure):
    """crgpu_rtl_gem_runs"""
    _fields_ = [("gems_per_tag", C.c_uint64 * 64), ("common", C.c_uint64 * 4096), ("cells_per_tag", C.c_uint64 * 64),
                ("cells_per_gem_hist", C.c_uint64 * 257), ("cells_per_probe", C.c_uint64 * 256),
                ("first_cell_col_per_probe", C.c_uint64 * 256), ("gems_with_cells", C.c_uint64), ("n_gems", C.c_uint64),
                ("n_cells", C.c_uint64), ("n_probe", C.c_uint32), ("n_tags", C.c_uint32), ("present", C.c_uint8 * 64)]


class RtlOverlapRow(C.Structure):
    """crgpu_rtl_overlap_row"""
    _fields_ = [("tag1", C.c_uint32), ("tag2", C.c_uint32), ("gems1", C.c_int64), ("gems2", C.c_int64), ("common_gems", C.c_int64),
                ("overlap", C.c_double)]


class RtlHighOccupancy(C.Structure):
    """crgpu_rtl_high_occupancy"""
    _fields_ = [(n, C.c_uint64) for n in ("n_cells", "n_kept", "gems_with_cells", "high_occupancy_gems", "cells_in_high_occupancy_gems")] + [
        ("fraction_cell_gems_high_occupancy", C.c_double), ("fraction_cells_in_high_occupancy_gems", C.c_double),
        ("threshold", C.c_uint32), ("reserved", C.c_uint32)]


class MatrixSummaryClass(C.Structure):
    """crgpu_matrix_summary_class"""
    _fields_ = [(n, C.c_uint64) for n in ("n_features_class", "n_cells", "raw_total_counts", "union_total_counts", "union_nnz", "cells_total_counts",
                                          "cells_nnz", "genes_detected", "counts_sum", "counts_sumsq_hi", "counts_sumsq_lo", "genes_sum",
                                          "genes_sumsq_hi", "genes_sumsq_lo", "reads_cells")] + [
        ("top_counts_value", C.c_uint64 * 5), ("top_cells_value", C.c_uint64 * 5), ("counts_q", C.c_uint32 * 6), ("genes_q", C.c_uint32 * 6),
        ("top_counts_feature", C.c_uint32 * 5), ("top_cells_feature", C.c_uint32 * 5), ("n_top", C.c_uint32), ("reserved", C.c_uint32)]


class MatrixSummaryFloats(C.Structure):
    """crgpu_matrix_summary_floats"""
    _fields_ = [(n, C.c_double) for n in ("counts_mean", "counts_median", "counts_cv", "counts_iqr", "counts_std", "genes_mean", "genes_median",
                                          "genes_cv", "genes_iqr", "genes_std", "density", "cum_frac", "dupe_frac", "reads_per_cell",
                                          "reads_cum_frac")]


class AggregatesInfo(C.Structure):
    """crgpu_aggregates_info"""
    _fields_ = [(n, C.c_uint32) for n in ("n_antibodies", "n_signal", "top_k", "n_candidates", "min_antibodies", "n_aggregates", "n_slices",
                                          "rows_per_slice")] + [("in_lds", C.c_int32), ("reserved", C.c_uint32), ("rank_ms", C.c_double)]


class RpuStats(C.Structure):
    """crgpu_rpu_stats: index 0 on-target in cells, 1 on-target all barcodes, 2 off-target in cells, 3 off-target all barcodes;
    the gene counts: 0 on target, 1 off target"""
    _fields_ = [(n, C.c_double * 4) for n in ("mean", "cv", "median", "iqrnorm", "perc80")] + [("pcr_dupe_reads_frac_on_target", C.c_double)] + [
        (n, C.c_uint64 * 2) for n in ("n_genes", "n_not_detected", "n_detected", "n_not_quantifiable", "n_quantifiable")] + [
        ("n_quantifiable_total", C.c_uint64)]


class RpuGmmArgs(C.Structure):
    """crgpu_rpu_gmm_args"""
    _fields_ = [("start_lk_out", C.c_void_p), ("start_iters_out", C.c_void_p), ("enriched_out", C.c_void_p), ("reserved", C.c_uint64)]


class RpuGmmResult(C.Structure):
    """crgpu_rpu_gmm_result"""
    _fields_ = [(n, C.c_double) for n in ("log_rpu_threshold", "mu_high", "mu_low", "sd_high", "sd_low", "alpha_high", "alpha_low",
                                          "n_targeted_enriched", "n_targeted_not_enriched", "n_offtgt_enriched", "n_offtgt_not_enriched",
                                          "max_lk", "fit_ms")] + [(n, C.c_uint32) for n in ("winner", "n_starts", "fitted", "in_lds")]


class JibesSetup(C.Structure):
    """crgpu_jibes_setup"""
    _fields_ = [("estimated_cells", C.c_double)] + [(n, C.c_uint32) for n in ("n_states", "k_let_limited", "max_multiplets", "max_modeled_k_let")]


class JibesFitArgs(C.Structure):
    """crgpu_jibes_fit_args"""
    _fields_ = [(n, C.c_void_p) for n in ("bg", "fg", "sd", "freqs")] + [
        (n, C.c_double) for n in ("blank_prob", "estimated_cells", "abs_tol", "rel_tol", "confidence")] + [
        (n, C.c_uint32) for n in ("n_gems", "max_k_lets", "max_reps", "flags")] + [
        (n, C.c_void_p) for n in ("probs_out", "assignment_out", "assignment_prob_out", "ml_state_out", "posterior_out")] + [("reserved", C.c_uint64)]


class JibesFitResult(C.Structure):
    """crgpu_jibes_fit_result"""
    _fields_ = [(n, C.c_double * 16) for n in ("bg", "fg", "sd")] + [("ll", C.c_double), ("fit_ms", C.c_double)] + [
        (n, C.c_uint32) for n in ("iterations", "converged", "n_states", "k_let_limited")]


class MarginalRow(C.Structure):
    """crgpu_marginal_row"""
    _fields_ = [("status", C.c_uint32), ("in_lds", C.c_uint32), ("total_umis", C.c_uint64), ("cells_assigned", C.c_uint64),
                ("umi_threshold_observed", C.c_int64)] + [
        (n, C.c_double) for n in ("mean_low", "mean_high", "weight_low", "weight_high", "covariance", "lower_bound")] + [
        (n, C.c_uint32) for n in ("winner", "n_iter", "n_distinct", "reserved")]


class MarginalCalls(C.Structure):
    """crgpu_marginal_calls"""
    _fields_ = [("rows", C.POINTER(MarginalRow)), ("n_rows", C.c_uint32), ("reserved", C.c_uint32), ("n_barcodes", C.c_uint64),
                ("n_assigned", C.c_uint64)] + [
        (n, C.c_void_p) for n in ("d_indptr", "d_columns", "d_features_per_cell", "d_hist_offsets", "d_hist_values", "d_hist_counts")] + [
        (n, C.c_uint64) for n in ("n_hist_slots", "cells_with_0", "cells_with_1", "cells_with_many", "cells_without_umis")] + [
        (n, C.c_double) for n in ("ms_extract", "ms_histogram", "ms_fit", "ms_assign")]


class KmeansArgs(C.Structure):
    """crgpu_kmeans_args"""
    _fields_ = [("init", C.POINTER(C.c_void_p)), ("tol_factor", C.c_double), ("seed", C.c_uint32), ("max_iter", C.c_uint32)]


class KmeansResult(C.Structure):
    """crgpu_kmeans_result"""
    _fields_ = [(n, C.c_void_p) for n in ("labels_out", "clusters_out", "centers_out", "sizes_out", "wss_out")] + [
        (n, C.c_double) for n in ("inertia", "db_score", "fit_ms")] + [
        (n, C.c_uint32) for n in ("n_iter", "strict", "relocations", "in_lds")]


class SseqArgs(C.Structure):
    """crgpu_sseq_args"""
    _fields_ = [(n, C.c_uint32) for n in ("n_features", "wave_min", "wg_min", "reserved")]


class SseqParamsInfo(C.Structure):
    """crgpu_sseq_params_info"""
    _fields_ = [(n, C.c_void_p) for n in ("size_factors_out", "mean_out", "var_out", "phi_mm_out", "phi_out", "use_out")] + [
        ("zeta_hat", C.c_double), ("delta", C.c_double), ("n_cells", C.c_uint64), ("n_features", C.c_uint32), ("n_used", C.c_uint32)]


class SseqResult(C.Structure):
    """crgpu_sseq_result"""
    _fields_ = [(n, C.c_void_p) for n in ("sums_in_out", "sums_out_out", "norm_mean_in_out", "norm_mean_out_out", "log2_fold_change_out", "p_values_out",
                                           "adjusted_p_values_out", "below_median_out", "s_a_out", "s_b_out", "n_exact_out", "n_asymptotic_out")] + [
        (n, C.c_uint64) for n in ("n_terms", "n_short", "n_wave", "n_workgroup")] + [
        (n, C.c_double) for n in ("ms_sums", "ms_exact", "ms_asymptotic", "ms_bh")]


class SseqPairArgs(C.Structure):
    """crgpu_sseq_pair_args"""
    _fields_ = [(n, C.c_uint32) for n in ("n_features", "wave_min", "wg_min", "reserved")] + [("de_threshold", C.c_double)]


class SseqPairResult(C.Structure):
    """crgpu_sseq_pair_result"""
    _fields_ = [(n, C.c_void_p) for n in ("use_out", "mean_out", "phi_mm_out", "phi_out", "sums_a_out", "sums_b_out", "norm_mean_a_out", "norm_mean_b_out",
                                           "log2_fold_change_out", "p_values_out", "adjusted_p_values_out", "below_median_out")] + [
        (n, C.c_double) for n in ("zeta_hat", "delta", "s_a", "s_b")] + [
        (n, C.c_uint64) for n in ("n_cells_a", "n_cells_b", "n_exact", "n_asymptotic", "n_terms", "n_de")] + [
        (n, C.c_uint32) for n in ("n_used", "n_runs")] + [
        (n, C.c_double) for n in ("ms_median", "ms_sums", "ms_exact", "ms_asymptotic", "ms_bh")]


class PbItem(C.Structure):
    """crgpu_pb_item"""
    _fields_ = [(n, C.c_uint32) for n in ("gene", "group_a", "group_b", "stream")]


class PbArgs(C.Structure):
    """crgpu_pb_args"""
    _fields_ = [(n, C.c_uint32) for n in ("n_bootstraps", "lds_cells", "draws_per_wg", "reserved")] + [("seed", C.c_uint64)]


class KnnArgs(C.Structure):
    """crgpu_knn_args"""
    _fields_ = [("query_start", C.c_uint64), ("n_queries", C.c_uint64)] + [
        (n, C.c_uint32) for n in ("capacity", "force_device", "cand_tile", "reserved")]


class KnnResult(C.Structure):
    """crgpu_knn_result"""
    _fields_ = [(n, C.c_void_p) for n in ("indices_out", "distances_out", "sorted_out")] + [
        (n, C.c_double) for n in ("fit_ms", "select_ms", "sort_ms")] + [
        (n, C.c_uint64) for n in ("compactions", "selections", "survivors", "pairs_evaluated")] + [
        (n, C.c_uint32) for n in ("in_lds", "capacity", "query_tiles", "cand_tile")]


class KnnCrossArgs(C.Structure):
    """crgpu_knn_cross_args"""
    _fields_ = [(n, C.c_uint64) for n in ("query_start", "n_queries", "cand_start", "n_cands")] + [
        (n, C.c_uint32) for n in ("capacity", "force_device", "cand_tile", "reserved")]


class BcStep(C.Structure):
    """crgpu_bc_step"""
    _fields_ = [(n, C.c_void_p) for n in ("cur_rows", "mnn_cur", "mnn_ref", "corr_out")] + [("n_cur", C.c_uint64), ("n_mnn", C.c_uint64)]


class BcArgs(C.Structure):
    """crgpu_bc_args"""
    _fields_ = [(n, C.c_uint32) for n in ("pair_tile", "row_tile", "slab_rows", "reserved")]


class BcResult(C.Structure):
    """crgpu_bc_result"""
    _fields_ = [("step_ms_out", C.c_void_p)] + [
        (n, C.c_double) for n in ("fit_ms", "upload_ms", "download_ms", "gather_ms", "accumulate_ms", "finish_ms", "apply_ms")] + [
        (n, C.c_uint64) for n in ("pairs_evaluated", "chunks", "zero_den_rows")] + [(n, C.c_uint32) for n in ("pair_tile", "row_tile")]


class PcaArgs(C.Structure):
    """crgpu_pca_args"""
    _fields_ = [("pca_bc_indices", C.c_void_p), ("n_pca_bcs", C.c_uint64), ("start", C.c_void_p), ("n_start", C.c_uint64)] + [
        (n, C.c_uint32) for n in ("n_components", "pca_features", "min_count_threshold", "seed", "wave_block", "dot_parts_per_block", "reserved0",
                                  "reserved1")]


class PcaResult(C.Structure):
    """crgpu_pca_result"""
    _fields_ = [(n, C.c_void_p) for n in ("transformed_out", "components_out", "variance_explained_out", "dispersion_out", "features_selected_out",
                                           "d_out")] + [
        (n, C.c_double) for n in ("fit_ms", "prepare_ms", "lanczos_ms", "project_ms")] + [
        (n, C.c_uint64) for n in ("n_thresholded_barcodes", "n_pca_barcodes")] + [
        (n, C.c_uint32) for n in ("status", "n_components", "n_used_features", "n_thresholded_features", "it", "mprod", "m_b", "reserved")]


class TsneArgs(C.Structure):
    """crgpu_tsne_args"""
    _fields_ = [("eta", C.c_double)] + [
        (n, C.c_uint32) for n in ("first_iter", "n_iters", "max_iter", "stop_lying_iter", "mom_switch_iter", "row_tile", "cand_tile", "slab_rows",
                                  "wave_row_len", "reserved")]


class TsneResult(C.Structure):
    """crgpu_tsne_result"""
    _fields_ = [(n, C.c_void_p) for n in ("beta_out", "steps_out", "cond_out", "indptr_out", "indices_out", "values_out", "grad_out")] + [
        (n, C.c_double) for n in ("sum_q", "kl", "p_total", "fit_ms", "search_ms", "csr_ms", "loop_ms", "repulse_ms")] + [
        (n, C.c_uint64) for n in ("nnz", "pairs_evaluated")] + [
        (n, C.c_uint32) for n in ("row_tile", "cand_tile", "slab_rows", "wave_row_len", "n_chunks", "n_groups", "max_steps", "reserved")]


class UmapArgs(C.Structure):
    """crgpu_umap_args"""
    _fields_ = [(n, C.c_double) for n in ("a", "b", "gamma", "initial_alpha")] + [("seed", C.c_uint64)] + [
        (n, C.c_uint32) for n in ("first_epoch", "n_run", "n_epochs", "negative_sample_rate", "wave_row_len", "rows_per_wg", "reserved0", "reserved1")]


class UmapResult(C.Structure):
    """crgpu_umap_result"""
    _fields_ = [(n, C.c_void_p) for n in ("rho_out", "sigma_out", "steps_out", "indptr_out", "indices_out", "values_out", "delta_out")] + [
        (n, C.c_double) for n in ("wmax", "fit_ms", "search_ms", "csr_ms", "loop_ms")] + [
        (n, C.c_uint64) for n in ("nnz", "n_active", "n_negative")] + [
        (n, C.c_uint32) for n in ("wave_row_len", "rows_per_wg", "max_steps", "reserved")]


class LouvainArgs(C.Structure):
    """crgpu_louvain_args"""
    _fields_ = [(n, C.c_uint32) for n in ("symmetrize", "max_rounds", "wave_deg_max", "lds_deg_max", "batch", "reserved0")] + [("levels_capacity", C.c_uint64)]


class LouvainResult(C.Structure):
    """crgpu_louvain_result"""
    _fields_ = [(n, C.c_void_p) for n in ("levels_out", "level0_out", "final_out", "level_nodes_out", "level_communities_out", "level_rounds_out",
                                          "level_S_out", "level_ms_out")] + [("M", C.c_int64)] + [(n, C.c_uint64) for n in ("levels_needed", "nnz")] + [
        (n, C.c_double) for n in ("fit_ms", "union_ms", "rounds_ms", "aggregate_ms")] + [
        (n, C.c_uint32) for n in ("n_levels", "wave_deg_max", "lds_deg_max", "batch")]


KM_MAX_K, KM_MAX_D, KM_MAX_LIST = 64, 128, 64
TSNE_CAND_CHUNK, TSNE_MAX_FEATURES = 4096, 128
TSNE_PERPLEXITY, TSNE_THETA, TSNE_MAX_ITER, TSNE_STOP_LYING_ITER, TSNE_MOM_SWITCH_ITER, TSNE_ETA = 30, 0.5, 1000, 250, 250, 200.0
UMAP_SLOTS, UMAP_MAX_RATE, UMAP_MAX_FEATURES = 16, 8, 128
LOUVAIN_MAX_LEVELS, LOUVAIN_MAX_ROUNDS, LOUVAIN_WAVE_DEG_MAX, LOUVAIN_LDS_DEG_MAX, LOUVAIN_BATCH = 64, 1000, 127, 2047, 8
UMAP_N_NEIGHBORS, UMAP_MIN_DIST, UMAP_SPREAD, UMAP_NEGATIVE_SAMPLE_RATE, UMAP_METRICS = 30, 0.3, 1.0, 5, ("correlation", "pearson", "cosine", "euclidean")
PCA_MAX_COMPONENTS, PCA_DEFAULT_THRESHOLD, PCA_OK, PCA_NULL_AXIS, PCA_RANK_TOO_SMALL = 128, 2, 0, 1, 2
KNN_MAX_K, KNN_MAX_CAPACITY = 1024, 4096
BC_PAIR_CHUNK, BC_LDS_BYTES, BC_MAX_PAIR_TILE = 2048, 73728, 64
CBC_KNN, CBC_ALPHA, CBC_SIGMA, CBC_REALIGN_PANORAMA = 10, 0.1, 150.0, False
GRAPHCLUST_NEIGHBORS_DEFAULT, GRAPHCLUST_NEIGHBOR_A_DEFAULT, GRAPHCLUST_NEIGHBOR_B_DEFAULT = 1, -230.0, 120.0
NN_QUERIES_PER_CHUNK = 15000
SSEQ_MAX_K, SSEQ_BIG_COUNT = 4096, 900
MC_INITS, MC_SKIPPED, MC_FITTED = 10, 0, 1
JIBES_MAX_TAGS, JIBES_MAX_K_LETS, JIBES_MAX_STATES, JIBES_NEAR_ZERO, JIBES_CANT_CONVERGE = 16, 3, 970, 12, 1
JIBES_EXCLUDE_BLANKS, JIBES_NO_CONFIDENCE = 1, 2
MS_MAX_CLASSES, MS_NO_CLASS, MS_TOP_N = 32, 255, 5
TARGETED_MIN_UMIS, GMM_STARTS = 10, 5152
AGG_KIND_OTHER, AGG_KIND_ANTIBODY, AGG_KIND_ANTIGEN = 0, 1, 2
AGG_COUNTS, AGG_HIGHLY_CORRECTED, AGG_ANTIGEN = 1, 2, 4
RTL_MAX_TAGS, RTL_MAX_PROBES, RTL_MAX_TYPES = 64, 256, 8
RTL_KIND_RTL, RTL_KIND_ANTIBODY, RTL_KIND_OTHER = 0, 1, 2
RTL_NONE = 0xFF
MG_MAX_BOOTSTRAPS = 65536
MG_BRANCH_DEFAULT, MG_BRANCH_PERCENTILES, MG_BRANCH_DEFAULT_SUM, MG_BRANCH_PERCENTILES_SUM = 0, 1, 2, 3
MG_GENOME0, MG_GENOME1, MG_MULTIPLET = 0, 1, 2
SS_PER_CELL, SS_CELLS_ONLY, SS_BULK = 0, 1, 2
SS_PLAN_RAW, SS_PLAN_MAPPED, SS_PLAN_RAW_CELLS, SS_PLAN_BULK = 0, 1, 2, 3
SS_NUM_ADDITIONAL_DEPTHS = 10
SS_FIXED_DEPTHS = (3000, 5000, 10000, 20000, 30000, 50000)
SS_TARGETED_FIXED_DEPTHS = (100, 250, 500, 1000, 2500, 3000, 5000, 10000, 15000, 20000, 30000, 40000, 50000)
SS_BULK_FIXED_DEPTHS = (10000, 50000, 100000, 250000, 500000, 1000000, 2500000, 5000000, 7500000, 10000000, 50000000, 100000000, 1000000000)
SS_SUMMARY_COLS = ("mean_read_pairs", "median_read_pairs", "mean_umis", "median_umis", "mean_features", "median_features", "duplication_frac")

ED_STATUS = {0: "ok", 1: "no usable ambient barcode", 2: "SGT not applicable", 3: "no initial cell", 4: "no candidate"}
ED_KEEP_PROFILE, ED_KEEP_SIM_TABLE = 1, 2
SGT_TOO_FEW, SGT_SLOPE = 1, 2

# every symbol include/crgpu.h declares: (restype, argtypes)
_vp, _u8p, _u32, _u64, _i, _dbl = C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_double
SYMBOLS = {
    "crgpu_abi_version": (_i, []),
    "crgpu_abi_layout": (_i, [C.c_char_p, _vp, _u32]),
    "crgpu_count_host": (_i, [_vp, C.POINTER(Records), _u32, C.POINTER(C.POINTER(MatrixView)), _vp, C.POINTER(_vp)]),
    "crgpu_counts_probe_idx": (_i, [_vp, _vp, _vp]),
    "crgpu_counts_probe_triplets_dev": (_i, [_vp, _vp, _u32, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64)]),
    "crgpu_counts_probe_triplets": (_i, [_vp, _vp, _u32, _vp, _vp, _vp, C.POINTER(_u64)]),
    "crgpu_assemble_probe_matrix_dev": (_i, [_vp, _vp, _u32, _vp, _u64, C.POINTER(C.POINTER(MatrixDevView))]),
    "crgpu_probe_metrics_dev": (_i, [_vp, _vp, _u32, _vp, _u64, _vp, _vp]),
    "crgpu_get_unique_id": (_i, [_vp]),
    "crgpu_local_group_id": (_i, [_u32, _vp]),
    "crgpu_create": (_i, [C.POINTER(_vp), _i, _i, _i, _vp]),
    "crgpu_comm_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "crgpu_set_option": (_i, [_vp, _i, C.c_int64]),
    "crgpu_invalidate": (_i, [_vp]),
    "crgpu_get_stat": (_i, [_vp, _i, C.POINTER(_u64)]),
    "crgpu_barrier": (_i, [_vp]),
    "crgpu_allreduce_counts": (_i, [_vp, _i, _i]),
    "crgpu_exchange_keys_dev": (_i, [_vp, _vp, _u64, C.POINTER(_vp), C.POINTER(_u64), _vp]),
    "crgpu_gatherv_dev": (_i, [_vp, _vp, _u64, _i, C.POINTER(_vp), _vp]),
    "crgpu_gather_triplets_dev": (_i, [_vp, _vp, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64)]),
    "crgpu_allreduce_max_f64": (_i, [_vp, C.POINTER(_dbl)]),
    "crgpu_allreduce_sum_i64": (_i, [_vp, _vp, _u32]),
    "crgpu_destroy": (None, [_vp]),
    "crgpu_last_error": (C.c_char_p, [_vp]),
    "crgpu_synchronize": (_i, [_vp]),
    "crgpu_stream": (_vp, [_vp]),
    "crgpu_malloc": (_i, [_vp, C.POINTER(_vp), _u64]),
    "crgpu_free": (_i, [_vp, _vp]),
    "crgpu_trim": (_i, [_vp]),
    "crgpu_memcpy_h2d": (_i, [_vp, _vp, _vp, _u64]),
    "crgpu_memcpy_d2h": (_i, [_vp, _vp, _vp, _u64]),
    "crgpu_memset": (_i, [_vp, _vp, _i, _u64]),
    "crgpu_timing_enable": (_i, [_vp, _i]),
    "crgpu_timing_reset": (_i, [_vp]),
    "crgpu_timing_get": (_i, [_vp, _vp, _vp, _vp]),
    "crgpu_set_whitelist": (_i, [_vp, _i, C.c_char_p, _u32, _u32, C.c_char_p, _u32, _vp]),
    "crgpu_set_whitelist_packed": (_i, [_vp, _i, _vp, _u32, _u32, _vp, _u32, _vp]),
    "crgpu_whitelist_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "crgpu_get_canon_order": (_i, [_vp, _vp, _vp]),
    "crgpu_pack_dev": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp]),
    "crgpu_pack_rows_dev": (_i, [_vp, _vp, _vp, _u64, _u32, _u32, _u32, _vp, _vp, _vp]),
    "crgpu_shard_metrics_dev": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, C.POINTER(ShardMetrics)]),
    "crgpu_rows_metrics_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _u32, C.POINTER(RowsMetrics)]),
    "crgpu_homopolymer_metrics_dev": (_i, [_vp, _vp, _u32, _vp, _vp, _u32, _vp, _u64, _u32, _vp]),
    "crgpu_fastq_to_rows_dev": (_i, [_vp, _vp, _u64, _u32, _u64, _vp, _vp, _vp, C.POINTER(_u64)]),
    "crgpu_match_and_count_dev": (_i, [_vp, _vp, _vp, _u64, _vp]),
    "crgpu_set_posterior": (_i, [_vp, _dbl, _dbl]),
    "crgpu_correct_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "crgpu_get_counts": (_i, [_vp, _i, _i, _vp]),
    "crgpu_set_counts": (_i, [_vp, _i, _i, _vp]),
    "crgpu_reset_counts": (_i, [_vp]),
    "crgpu_counts_dev": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "crgpu_barcode_correction_metrics": (_i, [_vp, _i, C.POINTER(BcCorrectionMetrics)]),
    "crgpu_total_barcode_counts": (_i, [_vp, C.c_int64, _vp, _vp, _u64, C.POINTER(_u64)]),
    "crgpu_match_and_count": (_i, [_vp, _i, _vp, _vp, _u64, _vp]),
    "crgpu_correct": (_i, [_vp, _i, _vp, _vp, _u64, _vp, _vp]),
    "crgpu_set_key_layout": (_i, [_vp, _u32, _u32, _u32, _u32]),
    "crgpu_set_umi_min_len": (_i, [_vp, _u32]),
    "crgpu_pack_rows_var_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "crgpu_set_target_filter": (_i, [_vp, _vp, _u32, _u64]),
    "crgpu_build_keys_dev": (_i, [_vp, C.POINTER(Records), _vp, C.POINTER(_u64)]),
    "crgpu_partition_keys_dev": (_i, [_vp, _vp, _u64, _u32, _vp, _vp, _vp]),
    "crgpu_balanced_bounds": (_i, [_vp, _u32, _vp]),
    "crgpu_count_keys_dev": (_i, [_vp, _vp, _u64, C.POINTER(_vp)]),
    "crgpu_count_records_dev": (_i, [_vp, C.POINTER(Records), C.POINTER(_vp), _vp, _vp, _vp]),
    "crgpu_count_records_sharded_dev": (_i, [_vp, C.POINTER(Records), C.POINTER(_vp), _vp, _vp, _vp]),
    "crgpu_counts_info": (_i, [_vp, _vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "crgpu_counts_triplets_dev": (_i, [_vp, _vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "crgpu_counts_triplets": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "crgpu_counts_molecules": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "crgpu_counts_molecule_info": (_i, [_vp, _vp, C.c_uint16, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "crgpu_enable_barcode_summary": (_i, [_vp, _i]),
    "crgpu_counts_barcode_summary": (_i, [_vp, _vp, _u32, _u32, _vp, _u64, C.POINTER(_u64)]),
    "crgpu_write_barcode_summary_csv": (_i, [_vp, _vp, _u64, C.c_uint16, _vp, C.POINTER(C.c_char_p), _u32, C.c_char_p]),
    "crgpu_counts_free": (None, [_vp, _vp]),
    "crgpu_assemble_matrix": (_i, [_vp, _vp, _vp, _vp, _u64, _u32, C.POINTER(C.POINTER(MatrixView))]),
    "crgpu_matrix_free": (None, [_vp, C.POINTER(MatrixView)]),
    "crgpu_sum_matrices": (_i, [_vp, C.POINTER(MatrixView), C.POINTER(MatrixView), C.POINTER(C.POINTER(MatrixView))]),
    "crgpu_select_barcodes": (_i, [_vp, C.POINTER(MatrixView), _vp, _u64, C.POINTER(C.POINTER(MatrixView))]),
    "crgpu_trim_molecule_barcodes_dev": (_i, [_vp, _vp, _u64, _u64, _vp, _u64, _i, _u64, _vp, C.POINTER(_u64)]),
    "crgpu_concat_matrices": (_i, [_vp, _vp, _vp, _u32, C.POINTER(C.POINTER(MatrixView))]),
    "crgpu_write_mtx": (_i, [_vp, C.POINTER(MatrixView), C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint16]),
    "crgpu_assemble_matrix_dev": (_i, [_vp, _vp, _vp, _vp, _u64, C.POINTER(C.POINTER(MatrixDevView))]),
    "crgpu_sum_matrices_dev": (_i, [_vp, C.POINTER(MatrixDevView), C.POINTER(MatrixDevView), C.POINTER(C.POINTER(MatrixDevView))]),
    "crgpu_select_barcodes_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u64, C.POINTER(C.POINTER(MatrixDevView))]),
    "crgpu_matrix_dev_free": (None, [_vp, C.POINTER(MatrixDevView)]),
    "crgpu_matrix_dev_column_sums": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, _vp]),
    "crgpu_ordmag_candidates": (_i, [C.c_int64, _vp, _u32, C.POINTER(_u32)]),
    "crgpu_call_cells_ordmag_dev": (_i, [_vp, _vp, _u64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(OrdmagResult), C.POINTER(_vp),
                                         C.POINTER(_u64)]),
    "crgpu_cell_ranks_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u64, _vp]),
    "crgpu_select_barcodes_cols_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u64, C.POINTER(C.POINTER(MatrixDevView))]),
    "crgpu_mt19937_stream_dev": (_i, [_vp, _u32, _u64, _vp, C.POINTER(_u64), C.POINTER(_dbl)]),
    "crgpu_sgt_proportions": (_i, [_vp, _u64, _vp, C.POINTER(_dbl), C.POINTER(_dbl)]),
    "crgpu_emptydrops_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, _vp, _vp, _u64, _u64, _u64, _u64, _u32, _dbl, _u64, _vp, _u32,
                                  _vp, _u32, C.POINTER(EmptydropsResult), C.POINTER(EmptydropsArrays)]),
    "crgpu_ambient_pvalues_dev": (_i, [_vp, _vp, _vp, _u64, _vp, _u32, _vp, _u32, _dbl, _vp, _vp, _vp, _vp, C.POINTER(_u64)]),
    "crgpu_emptydrops_arrays_free": (None, [_vp, C.POINTER(EmptydropsArrays)]),
    "crgpu_emptydrops_simulate_dev": (_i, [_vp, _vp, _u32, _vp, _vp, _u64, _u32, _u64, _vp, C.POINTER(_u32), _vp, _vp, C.POINTER(_dbl)]),
    "crgpu_subsample_dev": (_i, [_vp, _vp, C.POINTER(SubsampleArgs), C.POINTER(SubsampleResult)]),
    "crgpu_subsample_plan": (_i, [_i, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _u32, C.POINTER(_u32)]),
    "crgpu_subsample_summary": (_i, [_u32, _u32, _u64, _u32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "crgpu_normalize_depth_dev": (_i, [_vp, _vp, C.POINTER(NormalizeDepthArgs), C.POINTER(NormalizeDepthResult)]),
    "crgpu_select_features_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, C.POINTER(C.POINTER(MatrixDevView))]),
    "crgpu_normalize_depth_plan": (_i, [_u32, _vp, _vp, _vp, _i, _i, _vp, _dbl, _vp]),
    "crgpu_matrix_dev_genome_totals": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, _u32, _vp]),
    "crgpu_multigenome_dev": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, C.POINTER(MultigenomeResult)]),
    "crgpu_multigenome_summary": (_i, [_vp, _u32, _u64, _vp, C.POINTER(MultigenomeResult)]),
    "crgpu_rtl_tags_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, _vp, _u32, _u32, _vp, _vp, _vp]),
    "crgpu_rtl_sample_columns_dev": (_i, [_vp, _vp, _u64, _vp, _u32, _u32, _i, _vp, _u64, _vp, _vp]),
    "crgpu_rtl_gem_runs_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, _vp, _u64, _vp, _vp, _vp, C.POINTER(RtlGemRuns)]),
    "crgpu_rtl_medians_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _vp, _u64, _vp, _vp]),
    "crgpu_rtl_overlap_rows": (_i, [_vp, _vp, _vp, _u32, C.POINTER(RtlOverlapRow), _u32, _vp]),
    "crgpu_rtl_ab_thresholds": (_i, [_vp, _vp, _vp, _u32, _vp, _u32, _vp]),
    "crgpu_rtl_suspicious_pairings": (_i, [C.POINTER(RtlOverlapRow), _u32, _vp, _vp, _u32, C.POINTER(RtlOverlapRow), _vp]),
    "crgpu_rtl_occupancy_summary": (_i, [_vp, _u32, _u64, _vp, C.c_int64, _dbl, _vp, _vp, _vp]),
    "crgpu_rtl_remove_high_occupancy_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u64, _u32, _vp, C.POINTER(RtlHighOccupancy)]),
    "crgpu_matrix_summary_dev": (_i, [_vp, C.POINTER(MatrixDevView), _u32, _u32, _vp, _vp, _u64, _vp, _vp, _vp, _vp, C.POINTER(MatrixSummaryClass),
                                      C.POINTER(_u64), C.POINTER(_u64), _vp, _vp]),
    "crgpu_matrix_dev_reads_per_column": (_i, [_vp, C.POINTER(MatrixDevView), _u32, _vp]),
    "crgpu_matrix_summary_stats": (_i, [C.POINTER(MatrixSummaryClass), _u64, _u64, C.POINTER(MatrixSummaryFloats)]),
    "crgpu_feature_metrics_dev": (_i, [_vp, _vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _vp]),
    "crgpu_targeted_rpu_stats": (_i, [_u32, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(RpuStats), _vp, _vp, _vp]),
    "crgpu_rpu_gmm_dev": (_i, [_vp, _vp, _vp, _u32, C.POINTER(RpuGmmArgs), C.POINTER(RpuGmmResult)]),
    "crgpu_jibes_expected_cells": (_i, [_u64, _u32, C.POINTER(_dbl)]),
    "crgpu_jibes_latent_states": (_i, [_u64, _u32, _u32, _u32, _dbl, _vp, C.POINTER(JibesSetup)]),
    "crgpu_jibes_log_prior": (_i, [_vp, _u32, _u32, _dbl, _u32, _u32, _u32, _u32, _dbl, _vp, _vp]),
    "crgpu_jibes_initial_parameters": (_i, [_vp, _u64, _u32, _vp, _vp, _vp, _vp]),
    "crgpu_jibes_tag_counts_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u64), _vp]),
    "crgpu_jibes_fit_dev": (_i, [_vp, _vp, _u64, _u32, C.POINTER(JibesFitArgs), C.POINTER(JibesFitResult)]),
    "crgpu_marginal_calls_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, _u32, _u32, _u32, C.POINTER(C.POINTER(MarginalCalls))]),
    "crgpu_marginal_calls_free": (None, [_vp, C.POINTER(MarginalCalls)]),
    "crgpu_tag_moments_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, _u32, _vp, _vp, _vp]),
    "crgpu_tag_contaminants": (_i, [_u32, _u64, _vp, _vp, _vp, _vp, _u64, _dbl, _dbl, _vp, _vp]),
    "crgpu_marginal_seed_draws": (_i, [_u64, _vp, _vp]),
    "crgpu_kmeans_dev": (_i, [_vp, _vp, _u64, _u32, _u64, _vp, _u32, C.POINTER(KmeansArgs), C.POINTER(KmeansResult)]),
    "crgpu_kmeans_db_index": (_i, [_u32, _u32, _vp, _vp, _vp, C.POINTER(_dbl)]),
    "crgpu_kmeans_seed_draws": (_i, [_u32, _u64, _u32, _vp, C.POINTER(_u64)]),
    "crgpu_sseq_params_dev": (_i, [_vp, C.POINTER(MatrixDevView), C.POINTER(SseqArgs), C.POINTER(_vp)]),
    "crgpu_sseq_params_free": (None, [_vp, _vp]),
    "crgpu_sseq_params_get": (_i, [_vp, _vp, C.POINTER(SseqParamsInfo)]),
    "crgpu_sseq_diffexp_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _vp, _u32, C.POINTER(SseqArgs), C.POINTER(SseqResult)]),
    "crgpu_sseq_adjust_bh": (_i, [_vp, _u64, _vp]),
    "crgpu_sseq_pairs_create_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, C.POINTER(SseqPairArgs), C.POINTER(_vp)]),
    "crgpu_sseq_pairs_free": (None, [_vp, _vp]),
    "crgpu_sseq_pair_dev": (_i, [_vp, _vp, _vp, _u32, _vp, _u32, C.POINTER(SseqPairArgs), C.POINTER(SseqPairResult)]),
    "crgpu_sseq_pair_bootstrap_dev": (_i, [_vp, _vp, _vp, _u32, C.POINTER(PbArgs), _vp, _vp]),
    "crgpu_perturbation_ci": (_i, [_vp, _vp, _u32, C.c_double, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp]),
    "crgpu_cluster_medians_dev": (_i, [_vp, _vp, _u64, _u32, _u64, _vp, _u32, _vp, _vp]),
    "crgpu_linkage_complete": (_i, [_vp, _u32, _u32, _vp]),
    "crgpu_knn_dev": (_i, [_vp, _vp, _u64, _u32, _u64, _u32, C.POINTER(KnnArgs), C.POINTER(KnnResult)]),
    "crgpu_graphclust_num_neighbors": (_i, [_u64, _u32, _dbl, _dbl, C.POINTER(_u32)]),
    "crgpu_knn_cross_dev": (_i, [_vp, _vp, _u64, _u32, _u64, _u32, C.POINTER(KnnCrossArgs), C.POINTER(KnnResult)]),
    "crgpu_mnn_pairs": (_i, [_vp, _u64, _u64, _vp, _u64, _u64, _u32, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "crgpu_batch_correct_dev": (_i, [_vp, _vp, _u64, _u32, _u64, _dbl, C.POINTER(BcStep), _u32, _vp, C.POINTER(BcArgs), C.POINTER(BcResult)]),
    "crgpu_pca_dev": (_i, [_vp, C.POINTER(MatrixDevView), _u32, C.POINTER(PcaArgs), C.POINTER(PcaResult)]),
    "crgpu_legacy_randn": (_i, [_u32, _u64, _vp]),
    "crgpu_normalized_dispersion": (_i, [_vp, _vp, _u64, _u32, _vp]),
    "crgpu_small_svd": (_i, [_vp, _u32, _vp, _vp, _vp]),
    "crgpu_tsne_affinities_dev": (_i, [_vp, _vp, _vp, _u64, _u32, _dbl, C.POINTER(TsneArgs), C.POINTER(TsneResult)]),
    "crgpu_tsne_gradient_dev": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _u32, _dbl, C.POINTER(TsneArgs), C.POINTER(TsneResult)]),
    "crgpu_tsne_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, C.POINTER(TsneArgs), C.POINTER(TsneResult)]),
    "crgpu_umap_ab": (_i, [_dbl, _dbl, C.POINTER(_dbl), C.POINTER(_dbl)]),
    "crgpu_umap_graph_dev": (_i, [_vp, _vp, _vp, _u64, _u32, _u32, C.POINTER(UmapResult)]),
    "crgpu_umap_epochs_dev": (_i, [_vp, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, C.POINTER(UmapArgs), C.POINTER(UmapResult)]),
    "crgpu_louvain_dev": (_i, [_vp, _vp, _vp, _vp, _u64, C.POINTER(LouvainArgs), C.POINTER(LouvainResult)]),
    "crgpu_modularity": (_i, [_vp, _vp, _vp, _u64, _vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "crgpu_aggregate_min_antibodies": (_i, [_u32, C.POINTER(_u32)]),
    "crgpu_antigen_outlier_threshold": (_i, [_vp, _u32, C.POINTER(_dbl), C.POINTER(_dbl), C.POINTER(_dbl)]),
    "crgpu_aggregates_by_counts_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, _u32, _vp, _vp, _u32, C.POINTER(_u32),
                                            C.POINTER(AggregatesInfo)]),
    "crgpu_aggregates_highly_corrected_dev": (_i, [_vp, _vp, _vp, _u64, _vp, C.POINTER(_u64)]),
    "crgpu_counts_corrected_reads_per_column": (_i, [_vp, _vp, C.POINTER(MatrixDevView), _u32, _vp]),
    "crgpu_aggregates_antigen_outliers_dev": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _u32, _vp, _vp, _u32, C.POINTER(_u32), C.POINTER(_dbl)]),
    "crgpu_aggregates_partition_dev": (_i, [_vp, _vp, _u64, C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_vp), C.POINTER(_u64)]),
    "crgpu_take_columns_dev": (_i, [_vp, _vp, _u32, _u64, _vp, _u64, _vp]),
    "crgpu_sum_u32_dev": (_i, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "crgpu_filter_cells_min_umis_dev": (_i, [_vp, _vp, _u64, _vp, _u64, _u64, C.POINTER(_vp), C.POINTER(_u64)]),
    "crgpu_filter_cells_mito_dev": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _dbl, C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_vp), C.POINTER(_u64)]),
    "crgpu_matrix_dev_download": (_i, [_vp, C.POINTER(MatrixDevView), _vp, _vp, _vp, _vp]),
    "crgpu_count": (_i, [_vp, C.POINTER(Records), _u32, C.POINTER(C.POINTER(MatrixView))]),
    "crgpu_set_feature_pattern": (_i, [_vp, _i, C.c_char_p, _u32, _u32, _vp, _vp]),
    "crgpu_match_features_dev": (_i, [_vp, _i, _vp, _vp, _u64, _vp]),
    "crgpu_set_barcode_segments": (_i, [_vp, _i, _u32, _vp, _vp, _vp]),
    "crgpu_combine_segments_dev": (_i, [_vp, _i, _vp, _u32, _u64, _i, _vp]),
    "crgpu_set_feature_extractor": (_i, [_vp, _i, _vp, _u32, _vp, _u32]),
    "crgpu_compile_feature_pattern": (_i, [C.c_char_p, _u32, C.c_char_p, _u64]),
    "crgpu_feature_extractor_regex": (_i, [_vp, _i, _u32, C.c_char_p, _u64, _vp]),
    "crgpu_extract_features_dev": (_i, [_vp, _i, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _u64, _vp, _vp, _vp]),
    "crgpu_feature_counts_dev": (_i, [_vp, _vp, _u64, _u32, _vp]),
    "crgpu_compute_feature_dist": (_i, [_vp, _vp, _u32, _vp]),
    "crgpu_synth_rows_dev": (_i, [_vp, _u64, _u64, _u64, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "crgpu_synth_rows_host": (_i, [_u64, _u64, _u64, _vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp]),
    "crgpu_synth_dev": (_i, [_vp, C.POINTER(SynthParams), _u64, _u64, C.POINTER(SynthOut)]),
    "crgpu_synth_host": (_i, [C.POINTER(SynthParams), _u64, _u64, C.POINTER(SynthOut)]),
}

_lib = None


def load():
    """Load libcrgpu.so and bind every symbol of include/crgpu.h (raises if one is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CrgpuError(-2, "%s not found: build it with `python -m cellranger_amd.build` "
                             "(there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    missing = [name for name in SYMBOLS if not hasattr(L, name)]
    if missing:
        raise CrgpuError(-2, "libcrgpu.so does not export: %s" % ", ".join(missing))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def ptr(a):
    """numpy array / int / None -> c_void_p"""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data_as(C.c_void_p)
    return C.c_void_p(int(a))


class FeatureDef(C.Structure):
    """crgpu_feature_def"""
    _fields_ = [("pattern", C.c_char_p), ("sequence", C.c_char_p), ("index", C.c_uint32), ("read", C.c_uint32)]


NO_CAPTURE = 0xFFFFFFFF
