// ctx.hip -- context, memory helpers and the HIP-event timing ledger of libcrgpu.
#include <cmath>

#include <cstdio>
#include <cstdlib>

#include "common.h"

static thread_local std::string g_thread_err;

void cr_set_thread_error(const char *msg) { g_thread_err = msg; }

int cr_fail(crgpu_ctx *ctx, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->err = buf;
    else
        g_thread_err = buf;
    return code;
}

extern "C" int crgpu_abi_version(void) { return CRGPU_ABI_VERSION; }

// ---- layout of the public structs, for bindings to check their own declarations against (include/crgpu.h) -------------
#include <cstddef>
namespace {
struct AbiField {
    uint32_t offset, size;
};
struct AbiStruct {
    const char *name;
    uint32_t size, align;
    std::vector<AbiField> fields;
};
#define ABI_F(T, f) AbiField{(uint32_t)offsetof(T, f), (uint32_t)sizeof(((T *)nullptr)->f)}
#define ABI_S(T, ...) AbiStruct{#T, (uint32_t)sizeof(T), (uint32_t)alignof(T), {__VA_ARGS__}}
const std::vector<AbiStruct> &abi_table() {
    static const std::vector<AbiStruct> t = {
        ABI_S(crgpu_records, ABI_F(crgpu_records, n), ABI_F(crgpu_records, umi_len), ABI_F(crgpu_records, d_bc_idx),
              ABI_F(crgpu_records, d_umi), ABI_F(crgpu_records, d_umi_qualn), ABI_F(crgpu_records, d_feature),
              ABI_F(crgpu_records, d_flags), ABI_F(crgpu_records, d_umi_len), ABI_F(crgpu_records, d_probe_idx)),
        ABI_S(crgpu_matrix, ABI_F(crgpu_matrix, n_barcodes), ABI_F(crgpu_matrix, nnz), ABI_F(crgpu_matrix, n_features),
              ABI_F(crgpu_matrix, cb_len), ABI_F(crgpu_matrix, barcode_rank), ABI_F(crgpu_matrix, barcode_seq),
              ABI_F(crgpu_matrix, indptr), ABI_F(crgpu_matrix, indices), ABI_F(crgpu_matrix, data), ABI_F(crgpu_matrix, gem_group),
              ABI_F(crgpu_matrix, barcode_seq_hi)),
        ABI_S(crgpu_matrix_dev, ABI_F(crgpu_matrix_dev, n_barcodes), ABI_F(crgpu_matrix_dev, nnz),
              ABI_F(crgpu_matrix_dev, d_barcode_rank), ABI_F(crgpu_matrix_dev, d_indptr), ABI_F(crgpu_matrix_dev, d_indices),
              ABI_F(crgpu_matrix_dev, d_data)),
        ABI_S(crgpu_dupinfo, ABI_F(crgpu_dupinfo, processed_umi), ABI_F(crgpu_dupinfo, read_count), ABI_F(crgpu_dupinfo, flags),
              ABI_F(crgpu_dupinfo, reserved)),
        ABI_S(crgpu_barcode_summary_row, ABI_F(crgpu_barcode_summary_row, barcode_rank), ABI_F(crgpu_barcode_summary_row, library),
              ABI_F(crgpu_barcode_summary_row, reads), ABI_F(crgpu_barcode_summary_row, umis),
              ABI_F(crgpu_barcode_summary_row, candidate_dup_reads), ABI_F(crgpu_barcode_summary_row, umi_corrected_reads)),
        ABI_S(crgpu_bc_correction_metrics, ABI_F(crgpu_bc_correction_metrics, valid_reads),
              ABI_F(crgpu_bc_correction_metrics, corrected_reads), ABI_F(crgpu_bc_correction_metrics, barcodes_detected),
              ABI_F(crgpu_bc_correction_metrics, effective_barcode_diversity)),
        ABI_S(crgpu_shard_metrics, ABI_F(crgpu_shard_metrics, sequenced_reads), ABI_F(crgpu_shard_metrics, bc_n_bases),
              ABI_F(crgpu_shard_metrics, bc_bases), ABI_F(crgpu_shard_metrics, umi_n_bases), ABI_F(crgpu_shard_metrics, umi_bases),
              ABI_F(crgpu_shard_metrics, bc_q30_bases), ABI_F(crgpu_shard_metrics, bc_q30_den), ABI_F(crgpu_shard_metrics, umi_q30_bases),
              ABI_F(crgpu_shard_metrics, umi_q30_den), ABI_F(crgpu_shard_metrics, good_umi), ABI_F(crgpu_shard_metrics, has_n_barcode),
              ABI_F(crgpu_shard_metrics, has_n_umi), ABI_F(crgpu_shard_metrics, homopolymer_barcode),
              ABI_F(crgpu_shard_metrics, homopolymer_umi), ABI_F(crgpu_shard_metrics, low_min_qual_barcode),
              ABI_F(crgpu_shard_metrics, low_min_qual_umi), ABI_F(crgpu_shard_metrics, miss_whitelist_barcode),
              ABI_F(crgpu_shard_metrics, polyt_suffix_umi)),
        ABI_S(crgpu_rows_metrics, ABI_F(crgpu_rows_metrics, n_bases), ABI_F(crgpu_rows_metrics, bases),
              ABI_F(crgpu_rows_metrics, q30_bases), ABI_F(crgpu_rows_metrics, q30_den)),
        ABI_S(crgpu_feature_def, ABI_F(crgpu_feature_def, pattern), ABI_F(crgpu_feature_def, sequence),
              ABI_F(crgpu_feature_def, index), ABI_F(crgpu_feature_def, read)),
        ABI_S(crgpu_synth_params, ABI_F(crgpu_synth_params, seed), ABI_F(crgpu_synth_params, cb_len), ABI_F(crgpu_synth_params, umi_len),
              ABI_F(crgpu_synth_params, n_wl), ABI_F(crgpu_synth_params, wl_packed), ABI_F(crgpu_synth_params, n_cells),
              ABI_F(crgpu_synth_params, cell_wl_pos), ABI_F(crgpu_synth_params, cell_cdf), ABI_F(crgpu_synth_params, n_ambient),
              ABI_F(crgpu_synth_params, ambient_wl_pos), ABI_F(crgpu_synth_params, n_genes), ABI_F(crgpu_synth_params, gene_cdf),
              ABI_F(crgpu_synth_params, ambient_per_2_16), ABI_F(crgpu_synth_params, cb_err_per_2_16),
              ABI_F(crgpu_synth_params, umi_err_per_2_16), ABI_F(crgpu_synth_params, n_per_2_20),
              ABI_F(crgpu_synth_params, no_feature_per_2_16), ABI_F(crgpu_synth_params, reads_per_umi),
              ABI_F(crgpu_synth_params, n_total), ABI_F(crgpu_synth_params, n_libs)),
        ABI_S(crgpu_synth_out, ABI_F(crgpu_synth_out, cb), ABI_F(crgpu_synth_out, cb_qualn), ABI_F(crgpu_synth_out, umi),
              ABI_F(crgpu_synth_out, umi_qualn), ABI_F(crgpu_synth_out, feature), ABI_F(crgpu_synth_out, flags)),
        ABI_S(crgpu_ordmag_result, ABI_F(crgpu_ordmag_result, n_nonzero), ABI_F(crgpu_ordmag_result, recovered_cells),
              ABI_F(crgpu_ordmag_result, recovered_boot), ABI_F(crgpu_ordmag_result, loss_boot),
              ABI_F(crgpu_ordmag_result, baseline_bc_idx), ABI_F(crgpu_ordmag_result, top_n_boot),
              ABI_F(crgpu_ordmag_result, filtered_bcs_mean), ABI_F(crgpu_ordmag_result, filtered_bcs_var),
              ABI_F(crgpu_ordmag_result, filtered_bcs_cv), ABI_F(crgpu_ordmag_result, filtered_bcs_lb),
              ABI_F(crgpu_ordmag_result, filtered_bcs_ub), ABI_F(crgpu_ordmag_result, filtered_bcs),
              ABI_F(crgpu_ordmag_result, filtered_bcs_cutoff), ABI_F(crgpu_ordmag_result, filtered_bcs_cutoff_set),
              ABI_F(crgpu_ordmag_result, estimated)),
        ABI_S(crgpu_emptydrops_result, ABI_F(crgpu_emptydrops_result, status), ABI_F(crgpu_emptydrops_result, sim_in_lds),
              ABI_F(crgpu_emptydrops_result, n_ambient_used), ABI_F(crgpu_emptydrops_result, max_background_umis),
              ABI_F(crgpu_emptydrops_result, emptydrops_minimum_umis), ABI_F(crgpu_emptydrops_result, n_eval_features),
              ABI_F(crgpu_emptydrops_result, n_candidates), ABI_F(crgpu_emptydrops_result, n_distinct_n),
              ABI_F(crgpu_emptydrops_result, n_nonambient), ABI_F(crgpu_emptydrops_result, sgt_slope),
              ABI_F(crgpu_emptydrops_result, sgt_p0), ABI_F(crgpu_emptydrops_result, sim_ms)),
        ABI_S(crgpu_emptydrops_arrays, ABI_F(crgpu_emptydrops_arrays, n_candidates), ABI_F(crgpu_emptydrops_arrays, n_called),
              ABI_F(crgpu_emptydrops_arrays, n_eval_features), ABI_F(crgpu_emptydrops_arrays, n_distinct_n),
              ABI_F(crgpu_emptydrops_arrays, num_sims), ABI_F(crgpu_emptydrops_arrays, d_eval_cols),
              ABI_F(crgpu_emptydrops_arrays, d_umis), ABI_F(crgpu_emptydrops_arrays, d_obs_loglk),
              ABI_F(crgpu_emptydrops_arrays, d_n_lower), ABI_F(crgpu_emptydrops_arrays, d_pvalues),
              ABI_F(crgpu_emptydrops_arrays, d_pvalues_adj), ABI_F(crgpu_emptydrops_arrays, d_is_nonambient),
              ABI_F(crgpu_emptydrops_arrays, d_called_cols), ABI_F(crgpu_emptydrops_arrays, d_eval_features),
              ABI_F(crgpu_emptydrops_arrays, d_profile_p), ABI_F(crgpu_emptydrops_arrays, d_sim_n),
              ABI_F(crgpu_emptydrops_arrays, d_sim_loglk)),
        ABI_S(crgpu_subsample_args, ABI_F(crgpu_subsample_args, n_tasks), ABI_F(crgpu_subsample_args, n_genomes),
              ABI_F(crgpu_subsample_args, n_libs), ABI_F(crgpu_subsample_args, n_features),
              ABI_F(crgpu_subsample_args, n_cells), ABI_F(crgpu_subsample_args, seed), ABI_F(crgpu_subsample_args, rates),
              ABI_F(crgpu_subsample_args, task_type), ABI_F(crgpu_subsample_args, d_cell_ranks),
              ABI_F(crgpu_subsample_args, cell_genome_mask), ABI_F(crgpu_subsample_args, feature_genome),
              ABI_F(crgpu_subsample_args, feature_mask), ABI_F(crgpu_subsample_args, umis_per_bc),
              ABI_F(crgpu_subsample_args, read_pairs_per_bc), ABI_F(crgpu_subsample_args, features_det_per_bc),
              ABI_F(crgpu_subsample_args, read_pairs), ABI_F(crgpu_subsample_args, umis),
              ABI_F(crgpu_subsample_args, total_features_det), ABI_F(crgpu_subsample_args, any_reads)),
        ABI_S(crgpu_subsample_result, ABI_F(crgpu_subsample_result, n_molecules), ABI_F(crgpu_subsample_result, n_groups),
              ABI_F(crgpu_subsample_result, n_lane), ABI_F(crgpu_subsample_result, n_wave),
              ABI_F(crgpu_subsample_result, n_workgroup), ABI_F(crgpu_subsample_result, n_active_tasks),
              ABI_F(crgpu_subsample_result, n_batches), ABI_F(crgpu_subsample_result, draw_ms)),
        ABI_S(crgpu_normalize_depth_args, ABI_F(crgpu_normalize_depth_args, n_libs),
              ABI_F(crgpu_normalize_depth_args, n_features), ABI_F(crgpu_normalize_depth_args, n_classes),
              ABI_F(crgpu_normalize_depth_args, reserved), ABI_F(crgpu_normalize_depth_args, n_cells),
              ABI_F(crgpu_normalize_depth_args, seed), ABI_F(crgpu_normalize_depth_args, frac_reads_kept),
              ABI_F(crgpu_normalize_depth_args, feature_class), ABI_F(crgpu_normalize_depth_args, d_cell_ranks),
              ABI_F(crgpu_normalize_depth_args, cell_class_mask), ABI_F(crgpu_normalize_depth_args, matrix),
              ABI_F(crgpu_normalize_depth_args, raw_mapped_reads), ABI_F(crgpu_normalize_depth_args, flt_mapped_reads),
              ABI_F(crgpu_normalize_depth_args, reads_per_lib), ABI_F(crgpu_normalize_depth_args, kept_reads_per_lib),
              ABI_F(crgpu_normalize_depth_args, kept_molecules_per_lib), ABI_F(crgpu_normalize_depth_args, kept_out)),
        ABI_S(crgpu_normalize_depth_result, ABI_F(crgpu_normalize_depth_result, n_molecules),
              ABI_F(crgpu_normalize_depth_result, n_lane), ABI_F(crgpu_normalize_depth_result, n_wave),
              ABI_F(crgpu_normalize_depth_result, n_workgroup), ABI_F(crgpu_normalize_depth_result, n_kept_molecules),
              ABI_F(crgpu_normalize_depth_result, n_triplets), ABI_F(crgpu_normalize_depth_result, draw_ms),
              ABI_F(crgpu_normalize_depth_result, tally_ms)),
        ABI_S(crgpu_multigenome_result, ABI_F(crgpu_multigenome_result, n),
              ABI_F(crgpu_multigenome_result, obs_thresh0),
              ABI_F(crgpu_multigenome_result, obs_thresh1),
              ABI_F(crgpu_multigenome_result, observed_multiplets),
              ABI_F(crgpu_multigenome_result, observed_genome0),
              ABI_F(crgpu_multigenome_result, observed_genome1),
              ABI_F(crgpu_multigenome_result, sum_c0_genome0),
              ABI_F(crgpu_multigenome_result, sum_all_genome0),
              ABI_F(crgpu_multigenome_result, sum_c1_genome1),
              ABI_F(crgpu_multigenome_result, sum_all_genome1),
              ABI_F(crgpu_multigenome_result, sum_max_single),
              ABI_F(crgpu_multigenome_result, sum_all_single),
              ABI_F(crgpu_multigenome_result, purity0),
              ABI_F(crgpu_multigenome_result, purity1),
              ABI_F(crgpu_multigenome_result, purity_overall),
              ABI_F(crgpu_multigenome_result, boot_mean),
              ABI_F(crgpu_multigenome_result, inferred_multiplets),
              ABI_F(crgpu_multigenome_result, multiplet_rate),
              ABI_F(crgpu_multigenome_result, normalized_multiplet_rate),
              ABI_F(crgpu_multigenome_result, multiplet_rate_lb),
              ABI_F(crgpu_multigenome_result, multiplet_rate_ub),
              ABI_F(crgpu_multigenome_result, generator_words),
              ABI_F(crgpu_multigenome_result, obs_branch),
              ABI_F(crgpu_multigenome_result, rate_bounds_set)),
        ABI_S(crgpu_rtl_gem_runs, ABI_F(crgpu_rtl_gem_runs, gems_per_tag),
              ABI_F(crgpu_rtl_gem_runs, common),
              ABI_F(crgpu_rtl_gem_runs, cells_per_tag),
              ABI_F(crgpu_rtl_gem_runs, cells_per_gem_hist),
              ABI_F(crgpu_rtl_gem_runs, cells_per_probe),
              ABI_F(crgpu_rtl_gem_runs, first_cell_col_per_probe),
              ABI_F(crgpu_rtl_gem_runs, gems_with_cells),
              ABI_F(crgpu_rtl_gem_runs, n_gems),
              ABI_F(crgpu_rtl_gem_runs, n_cells),
              ABI_F(crgpu_rtl_gem_runs, n_probe),
              ABI_F(crgpu_rtl_gem_runs, n_tags),
              ABI_F(crgpu_rtl_gem_runs, present)),
        ABI_S(crgpu_rtl_overlap_row, ABI_F(crgpu_rtl_overlap_row, tag1),
              ABI_F(crgpu_rtl_overlap_row, tag2),
              ABI_F(crgpu_rtl_overlap_row, gems1),
              ABI_F(crgpu_rtl_overlap_row, gems2),
              ABI_F(crgpu_rtl_overlap_row, common_gems),
              ABI_F(crgpu_rtl_overlap_row, overlap)),
        ABI_S(crgpu_rtl_high_occupancy, ABI_F(crgpu_rtl_high_occupancy, n_cells),
              ABI_F(crgpu_rtl_high_occupancy, n_kept),
              ABI_F(crgpu_rtl_high_occupancy, gems_with_cells),
              ABI_F(crgpu_rtl_high_occupancy, high_occupancy_gems),
              ABI_F(crgpu_rtl_high_occupancy, cells_in_high_occupancy_gems),
              ABI_F(crgpu_rtl_high_occupancy, fraction_cell_gems_high_occupancy),
              ABI_F(crgpu_rtl_high_occupancy, fraction_cells_in_high_occupancy_gems),
              ABI_F(crgpu_rtl_high_occupancy, threshold),
              ABI_F(crgpu_rtl_high_occupancy, reserved)),
        ABI_S(crgpu_matrix_summary_class, ABI_F(crgpu_matrix_summary_class, n_features_class),
              ABI_F(crgpu_matrix_summary_class, n_cells),
              ABI_F(crgpu_matrix_summary_class, raw_total_counts),
              ABI_F(crgpu_matrix_summary_class, union_total_counts),
              ABI_F(crgpu_matrix_summary_class, union_nnz),
              ABI_F(crgpu_matrix_summary_class, cells_total_counts),
              ABI_F(crgpu_matrix_summary_class, cells_nnz),
              ABI_F(crgpu_matrix_summary_class, genes_detected),
              ABI_F(crgpu_matrix_summary_class, counts_sum),
              ABI_F(crgpu_matrix_summary_class, counts_sumsq_hi),
              ABI_F(crgpu_matrix_summary_class, counts_sumsq_lo),
              ABI_F(crgpu_matrix_summary_class, genes_sum),
              ABI_F(crgpu_matrix_summary_class, genes_sumsq_hi),
              ABI_F(crgpu_matrix_summary_class, genes_sumsq_lo),
              ABI_F(crgpu_matrix_summary_class, reads_cells),
              ABI_F(crgpu_matrix_summary_class, top_counts_value),
              ABI_F(crgpu_matrix_summary_class, top_cells_value),
              ABI_F(crgpu_matrix_summary_class, counts_q),
              ABI_F(crgpu_matrix_summary_class, genes_q),
              ABI_F(crgpu_matrix_summary_class, top_counts_feature),
              ABI_F(crgpu_matrix_summary_class, top_cells_feature),
              ABI_F(crgpu_matrix_summary_class, n_top),
              ABI_F(crgpu_matrix_summary_class, reserved)),
        ABI_S(crgpu_matrix_summary_floats, ABI_F(crgpu_matrix_summary_floats, counts_mean),
              ABI_F(crgpu_matrix_summary_floats, counts_median),
              ABI_F(crgpu_matrix_summary_floats, counts_cv),
              ABI_F(crgpu_matrix_summary_floats, counts_iqr),
              ABI_F(crgpu_matrix_summary_floats, counts_std),
              ABI_F(crgpu_matrix_summary_floats, genes_mean),
              ABI_F(crgpu_matrix_summary_floats, genes_median),
              ABI_F(crgpu_matrix_summary_floats, genes_cv),
              ABI_F(crgpu_matrix_summary_floats, genes_iqr),
              ABI_F(crgpu_matrix_summary_floats, genes_std),
              ABI_F(crgpu_matrix_summary_floats, density),
              ABI_F(crgpu_matrix_summary_floats, cum_frac),
              ABI_F(crgpu_matrix_summary_floats, dupe_frac),
              ABI_F(crgpu_matrix_summary_floats, reads_per_cell),
              ABI_F(crgpu_matrix_summary_floats, reads_cum_frac)),
        ABI_S(crgpu_rpu_stats, ABI_F(crgpu_rpu_stats, mean),
              ABI_F(crgpu_rpu_stats, cv),
              ABI_F(crgpu_rpu_stats, median),
              ABI_F(crgpu_rpu_stats, iqrnorm),
              ABI_F(crgpu_rpu_stats, perc80),
              ABI_F(crgpu_rpu_stats, pcr_dupe_reads_frac_on_target),
              ABI_F(crgpu_rpu_stats, n_genes),
              ABI_F(crgpu_rpu_stats, n_not_detected),
              ABI_F(crgpu_rpu_stats, n_detected),
              ABI_F(crgpu_rpu_stats, n_not_quantifiable),
              ABI_F(crgpu_rpu_stats, n_quantifiable),
              ABI_F(crgpu_rpu_stats, n_quantifiable_total)),
        ABI_S(crgpu_rpu_gmm_args, ABI_F(crgpu_rpu_gmm_args, start_lk_out),
              ABI_F(crgpu_rpu_gmm_args, start_iters_out),
              ABI_F(crgpu_rpu_gmm_args, enriched_out),
              ABI_F(crgpu_rpu_gmm_args, reserved)),
        ABI_S(crgpu_rpu_gmm_result, ABI_F(crgpu_rpu_gmm_result, log_rpu_threshold),
              ABI_F(crgpu_rpu_gmm_result, mu_high),
              ABI_F(crgpu_rpu_gmm_result, mu_low),
              ABI_F(crgpu_rpu_gmm_result, sd_high),
              ABI_F(crgpu_rpu_gmm_result, sd_low),
              ABI_F(crgpu_rpu_gmm_result, alpha_high),
              ABI_F(crgpu_rpu_gmm_result, alpha_low),
              ABI_F(crgpu_rpu_gmm_result, n_targeted_enriched),
              ABI_F(crgpu_rpu_gmm_result, n_targeted_not_enriched),
              ABI_F(crgpu_rpu_gmm_result, n_offtgt_enriched),
              ABI_F(crgpu_rpu_gmm_result, n_offtgt_not_enriched),
              ABI_F(crgpu_rpu_gmm_result, max_lk),
              ABI_F(crgpu_rpu_gmm_result, fit_ms),
              ABI_F(crgpu_rpu_gmm_result, winner),
              ABI_F(crgpu_rpu_gmm_result, n_starts),
              ABI_F(crgpu_rpu_gmm_result, fitted),
              ABI_F(crgpu_rpu_gmm_result, in_lds)),
        ABI_S(crgpu_aggregates_info, ABI_F(crgpu_aggregates_info, n_antibodies),
              ABI_F(crgpu_aggregates_info, n_signal),
              ABI_F(crgpu_aggregates_info, top_k),
              ABI_F(crgpu_aggregates_info, n_candidates),
              ABI_F(crgpu_aggregates_info, min_antibodies),
              ABI_F(crgpu_aggregates_info, n_aggregates),
              ABI_F(crgpu_aggregates_info, n_slices),
              ABI_F(crgpu_aggregates_info, rows_per_slice),
              ABI_F(crgpu_aggregates_info, in_lds),
              ABI_F(crgpu_aggregates_info, reserved),
              ABI_F(crgpu_aggregates_info, rank_ms)),
        ABI_S(crgpu_jibes_setup, ABI_F(crgpu_jibes_setup, estimated_cells),
              ABI_F(crgpu_jibes_setup, n_states),
              ABI_F(crgpu_jibes_setup, k_let_limited),
              ABI_F(crgpu_jibes_setup, max_multiplets),
              ABI_F(crgpu_jibes_setup, max_modeled_k_let)),
        ABI_S(crgpu_jibes_fit_args, ABI_F(crgpu_jibes_fit_args, bg),
              ABI_F(crgpu_jibes_fit_args, fg),
              ABI_F(crgpu_jibes_fit_args, sd),
              ABI_F(crgpu_jibes_fit_args, freqs),
              ABI_F(crgpu_jibes_fit_args, blank_prob),
              ABI_F(crgpu_jibes_fit_args, estimated_cells),
              ABI_F(crgpu_jibes_fit_args, abs_tol),
              ABI_F(crgpu_jibes_fit_args, rel_tol),
              ABI_F(crgpu_jibes_fit_args, confidence),
              ABI_F(crgpu_jibes_fit_args, n_gems),
              ABI_F(crgpu_jibes_fit_args, max_k_lets),
              ABI_F(crgpu_jibes_fit_args, max_reps),
              ABI_F(crgpu_jibes_fit_args, flags),
              ABI_F(crgpu_jibes_fit_args, probs_out),
              ABI_F(crgpu_jibes_fit_args, assignment_out),
              ABI_F(crgpu_jibes_fit_args, assignment_prob_out),
              ABI_F(crgpu_jibes_fit_args, ml_state_out),
              ABI_F(crgpu_jibes_fit_args, posterior_out),
              ABI_F(crgpu_jibes_fit_args, reserved)),
        ABI_S(crgpu_jibes_fit_result, ABI_F(crgpu_jibes_fit_result, bg),
              ABI_F(crgpu_jibes_fit_result, fg),
              ABI_F(crgpu_jibes_fit_result, sd),
              ABI_F(crgpu_jibes_fit_result, ll),
              ABI_F(crgpu_jibes_fit_result, fit_ms),
              ABI_F(crgpu_jibes_fit_result, iterations),
              ABI_F(crgpu_jibes_fit_result, converged),
              ABI_F(crgpu_jibes_fit_result, n_states),
              ABI_F(crgpu_jibes_fit_result, k_let_limited)),
        ABI_S(crgpu_marginal_row, ABI_F(crgpu_marginal_row, status),
              ABI_F(crgpu_marginal_row, in_lds),
              ABI_F(crgpu_marginal_row, total_umis),
              ABI_F(crgpu_marginal_row, cells_assigned),
              ABI_F(crgpu_marginal_row, umi_threshold_observed),
              ABI_F(crgpu_marginal_row, mean_low),
              ABI_F(crgpu_marginal_row, mean_high),
              ABI_F(crgpu_marginal_row, weight_low),
              ABI_F(crgpu_marginal_row, weight_high),
              ABI_F(crgpu_marginal_row, covariance),
              ABI_F(crgpu_marginal_row, lower_bound),
              ABI_F(crgpu_marginal_row, winner),
              ABI_F(crgpu_marginal_row, n_iter),
              ABI_F(crgpu_marginal_row, n_distinct),
              ABI_F(crgpu_marginal_row, reserved)),
        ABI_S(crgpu_marginal_calls, ABI_F(crgpu_marginal_calls, rows),
              ABI_F(crgpu_marginal_calls, n_rows),
              ABI_F(crgpu_marginal_calls, reserved),
              ABI_F(crgpu_marginal_calls, n_barcodes),
              ABI_F(crgpu_marginal_calls, n_assigned),
              ABI_F(crgpu_marginal_calls, d_indptr),
              ABI_F(crgpu_marginal_calls, d_columns),
              ABI_F(crgpu_marginal_calls, d_features_per_cell),
              ABI_F(crgpu_marginal_calls, d_hist_offsets),
              ABI_F(crgpu_marginal_calls, d_hist_values),
              ABI_F(crgpu_marginal_calls, d_hist_counts),
              ABI_F(crgpu_marginal_calls, n_hist_slots),
              ABI_F(crgpu_marginal_calls, cells_with_0),
              ABI_F(crgpu_marginal_calls, cells_with_1),
              ABI_F(crgpu_marginal_calls, cells_with_many),
              ABI_F(crgpu_marginal_calls, cells_without_umis),
              ABI_F(crgpu_marginal_calls, ms_extract),
              ABI_F(crgpu_marginal_calls, ms_histogram),
              ABI_F(crgpu_marginal_calls, ms_fit),
              ABI_F(crgpu_marginal_calls, ms_assign)),
        ABI_S(crgpu_kmeans_args, ABI_F(crgpu_kmeans_args, init),
              ABI_F(crgpu_kmeans_args, tol_factor),
              ABI_F(crgpu_kmeans_args, seed),
              ABI_F(crgpu_kmeans_args, max_iter)),
        ABI_S(crgpu_kmeans_result, ABI_F(crgpu_kmeans_result, labels_out),
              ABI_F(crgpu_kmeans_result, clusters_out),
              ABI_F(crgpu_kmeans_result, centers_out),
              ABI_F(crgpu_kmeans_result, sizes_out),
              ABI_F(crgpu_kmeans_result, wss_out),
              ABI_F(crgpu_kmeans_result, inertia),
              ABI_F(crgpu_kmeans_result, db_score),
              ABI_F(crgpu_kmeans_result, fit_ms),
              ABI_F(crgpu_kmeans_result, n_iter),
              ABI_F(crgpu_kmeans_result, strict),
              ABI_F(crgpu_kmeans_result, relocations),
              ABI_F(crgpu_kmeans_result, in_lds)),
        ABI_S(crgpu_sseq_args, ABI_F(crgpu_sseq_args, n_features),
              ABI_F(crgpu_sseq_args, wave_min),
              ABI_F(crgpu_sseq_args, wg_min),
              ABI_F(crgpu_sseq_args, reserved)),
        ABI_S(crgpu_sseq_params_info, ABI_F(crgpu_sseq_params_info, size_factors_out),
              ABI_F(crgpu_sseq_params_info, mean_out),
              ABI_F(crgpu_sseq_params_info, var_out),
              ABI_F(crgpu_sseq_params_info, phi_mm_out),
              ABI_F(crgpu_sseq_params_info, phi_out),
              ABI_F(crgpu_sseq_params_info, use_out),
              ABI_F(crgpu_sseq_params_info, zeta_hat),
              ABI_F(crgpu_sseq_params_info, delta),
              ABI_F(crgpu_sseq_params_info, n_cells),
              ABI_F(crgpu_sseq_params_info, n_features),
              ABI_F(crgpu_sseq_params_info, n_used)),
        ABI_S(crgpu_sseq_result, ABI_F(crgpu_sseq_result, sums_in_out),
              ABI_F(crgpu_sseq_result, sums_out_out),
              ABI_F(crgpu_sseq_result, norm_mean_in_out),
              ABI_F(crgpu_sseq_result, norm_mean_out_out),
              ABI_F(crgpu_sseq_result, log2_fold_change_out),
              ABI_F(crgpu_sseq_result, p_values_out),
              ABI_F(crgpu_sseq_result, adjusted_p_values_out),
              ABI_F(crgpu_sseq_result, below_median_out),
              ABI_F(crgpu_sseq_result, s_a_out),
              ABI_F(crgpu_sseq_result, s_b_out),
              ABI_F(crgpu_sseq_result, n_exact_out),
              ABI_F(crgpu_sseq_result, n_asymptotic_out),
              ABI_F(crgpu_sseq_result, n_terms),
              ABI_F(crgpu_sseq_result, n_short),
              ABI_F(crgpu_sseq_result, n_wave),
              ABI_F(crgpu_sseq_result, n_workgroup),
              ABI_F(crgpu_sseq_result, ms_sums),
              ABI_F(crgpu_sseq_result, ms_exact),
              ABI_F(crgpu_sseq_result, ms_asymptotic),
              ABI_F(crgpu_sseq_result, ms_bh)),
        ABI_S(crgpu_sseq_pair_args, ABI_F(crgpu_sseq_pair_args, n_features),
              ABI_F(crgpu_sseq_pair_args, wave_min),
              ABI_F(crgpu_sseq_pair_args, wg_min),
              ABI_F(crgpu_sseq_pair_args, reserved),
              ABI_F(crgpu_sseq_pair_args, de_threshold)),
        ABI_S(crgpu_sseq_pair_result, ABI_F(crgpu_sseq_pair_result, use_out),
              ABI_F(crgpu_sseq_pair_result, mean_out),
              ABI_F(crgpu_sseq_pair_result, phi_mm_out),
              ABI_F(crgpu_sseq_pair_result, phi_out),
              ABI_F(crgpu_sseq_pair_result, sums_a_out),
              ABI_F(crgpu_sseq_pair_result, sums_b_out),
              ABI_F(crgpu_sseq_pair_result, norm_mean_a_out),
              ABI_F(crgpu_sseq_pair_result, norm_mean_b_out),
              ABI_F(crgpu_sseq_pair_result, log2_fold_change_out),
              ABI_F(crgpu_sseq_pair_result, p_values_out),
              ABI_F(crgpu_sseq_pair_result, adjusted_p_values_out),
              ABI_F(crgpu_sseq_pair_result, below_median_out),
              ABI_F(crgpu_sseq_pair_result, zeta_hat),
              ABI_F(crgpu_sseq_pair_result, delta),
              ABI_F(crgpu_sseq_pair_result, s_a),
              ABI_F(crgpu_sseq_pair_result, s_b),
              ABI_F(crgpu_sseq_pair_result, n_cells_a),
              ABI_F(crgpu_sseq_pair_result, n_cells_b),
              ABI_F(crgpu_sseq_pair_result, n_exact),
              ABI_F(crgpu_sseq_pair_result, n_asymptotic),
              ABI_F(crgpu_sseq_pair_result, n_terms),
              ABI_F(crgpu_sseq_pair_result, n_de),
              ABI_F(crgpu_sseq_pair_result, n_used),
              ABI_F(crgpu_sseq_pair_result, n_runs),
              ABI_F(crgpu_sseq_pair_result, ms_median),
              ABI_F(crgpu_sseq_pair_result, ms_sums),
              ABI_F(crgpu_sseq_pair_result, ms_exact),
              ABI_F(crgpu_sseq_pair_result, ms_asymptotic),
              ABI_F(crgpu_sseq_pair_result, ms_bh)),
        ABI_S(crgpu_pb_item, ABI_F(crgpu_pb_item, gene),
              ABI_F(crgpu_pb_item, group_a),
              ABI_F(crgpu_pb_item, group_b),
              ABI_F(crgpu_pb_item, stream)),
        ABI_S(crgpu_pb_args, ABI_F(crgpu_pb_args, n_bootstraps),
              ABI_F(crgpu_pb_args, lds_cells),
              ABI_F(crgpu_pb_args, draws_per_wg),
              ABI_F(crgpu_pb_args, reserved),
              ABI_F(crgpu_pb_args, seed)),
        ABI_S(crgpu_knn_args, ABI_F(crgpu_knn_args, query_start),
              ABI_F(crgpu_knn_args, n_queries),
              ABI_F(crgpu_knn_args, capacity),
              ABI_F(crgpu_knn_args, force_device),
              ABI_F(crgpu_knn_args, cand_tile),
              ABI_F(crgpu_knn_args, reserved)),
        ABI_S(crgpu_knn_result, ABI_F(crgpu_knn_result, indices_out),
              ABI_F(crgpu_knn_result, distances_out),
              ABI_F(crgpu_knn_result, sorted_out),
              ABI_F(crgpu_knn_result, fit_ms),
              ABI_F(crgpu_knn_result, select_ms),
              ABI_F(crgpu_knn_result, sort_ms),
              ABI_F(crgpu_knn_result, compactions),
              ABI_F(crgpu_knn_result, selections),
              ABI_F(crgpu_knn_result, survivors),
              ABI_F(crgpu_knn_result, pairs_evaluated),
              ABI_F(crgpu_knn_result, in_lds),
              ABI_F(crgpu_knn_result, capacity),
              ABI_F(crgpu_knn_result, query_tiles),
              ABI_F(crgpu_knn_result, cand_tile)),
        ABI_S(crgpu_knn_cross_args, ABI_F(crgpu_knn_cross_args, query_start),
              ABI_F(crgpu_knn_cross_args, n_queries),
              ABI_F(crgpu_knn_cross_args, cand_start),
              ABI_F(crgpu_knn_cross_args, n_cands),
              ABI_F(crgpu_knn_cross_args, capacity),
              ABI_F(crgpu_knn_cross_args, force_device),
              ABI_F(crgpu_knn_cross_args, cand_tile),
              ABI_F(crgpu_knn_cross_args, reserved)),
        ABI_S(crgpu_bc_step, ABI_F(crgpu_bc_step, cur_rows),
              ABI_F(crgpu_bc_step, mnn_cur),
              ABI_F(crgpu_bc_step, mnn_ref),
              ABI_F(crgpu_bc_step, corr_out),
              ABI_F(crgpu_bc_step, n_cur),
              ABI_F(crgpu_bc_step, n_mnn)),
        ABI_S(crgpu_bc_args, ABI_F(crgpu_bc_args, pair_tile),
              ABI_F(crgpu_bc_args, row_tile),
              ABI_F(crgpu_bc_args, slab_rows),
              ABI_F(crgpu_bc_args, reserved)),
        ABI_S(crgpu_bc_result, ABI_F(crgpu_bc_result, step_ms_out),
              ABI_F(crgpu_bc_result, fit_ms),
              ABI_F(crgpu_bc_result, upload_ms),
              ABI_F(crgpu_bc_result, download_ms),
              ABI_F(crgpu_bc_result, gather_ms),
              ABI_F(crgpu_bc_result, accumulate_ms),
              ABI_F(crgpu_bc_result, finish_ms),
              ABI_F(crgpu_bc_result, apply_ms),
              ABI_F(crgpu_bc_result, pairs_evaluated),
              ABI_F(crgpu_bc_result, chunks),
              ABI_F(crgpu_bc_result, zero_den_rows),
              ABI_F(crgpu_bc_result, pair_tile),
              ABI_F(crgpu_bc_result, row_tile)),
        ABI_S(crgpu_tsne_args, ABI_F(crgpu_tsne_args, eta),
              ABI_F(crgpu_tsne_args, first_iter),
              ABI_F(crgpu_tsne_args, n_iters),
              ABI_F(crgpu_tsne_args, max_iter),
              ABI_F(crgpu_tsne_args, stop_lying_iter),
              ABI_F(crgpu_tsne_args, mom_switch_iter),
              ABI_F(crgpu_tsne_args, row_tile),
              ABI_F(crgpu_tsne_args, cand_tile),
              ABI_F(crgpu_tsne_args, slab_rows),
              ABI_F(crgpu_tsne_args, wave_row_len),
              ABI_F(crgpu_tsne_args, reserved)),
        ABI_S(crgpu_tsne_result, ABI_F(crgpu_tsne_result, beta_out),
              ABI_F(crgpu_tsne_result, steps_out),
              ABI_F(crgpu_tsne_result, cond_out),
              ABI_F(crgpu_tsne_result, indptr_out),
              ABI_F(crgpu_tsne_result, indices_out),
              ABI_F(crgpu_tsne_result, values_out),
              ABI_F(crgpu_tsne_result, grad_out),
              ABI_F(crgpu_tsne_result, sum_q),
              ABI_F(crgpu_tsne_result, kl),
              ABI_F(crgpu_tsne_result, p_total),
              ABI_F(crgpu_tsne_result, fit_ms),
              ABI_F(crgpu_tsne_result, search_ms),
              ABI_F(crgpu_tsne_result, csr_ms),
              ABI_F(crgpu_tsne_result, loop_ms),
              ABI_F(crgpu_tsne_result, repulse_ms),
              ABI_F(crgpu_tsne_result, nnz),
              ABI_F(crgpu_tsne_result, pairs_evaluated),
              ABI_F(crgpu_tsne_result, row_tile),
              ABI_F(crgpu_tsne_result, cand_tile),
              ABI_F(crgpu_tsne_result, slab_rows),
              ABI_F(crgpu_tsne_result, wave_row_len),
              ABI_F(crgpu_tsne_result, n_chunks),
              ABI_F(crgpu_tsne_result, n_groups),
              ABI_F(crgpu_tsne_result, max_steps),
              ABI_F(crgpu_tsne_result, reserved)),
        ABI_S(crgpu_umap_args, ABI_F(crgpu_umap_args, a),
              ABI_F(crgpu_umap_args, b),
              ABI_F(crgpu_umap_args, gamma),
              ABI_F(crgpu_umap_args, initial_alpha),
              ABI_F(crgpu_umap_args, seed),
              ABI_F(crgpu_umap_args, first_epoch),
              ABI_F(crgpu_umap_args, n_run),
              ABI_F(crgpu_umap_args, n_epochs),
              ABI_F(crgpu_umap_args, negative_sample_rate),
              ABI_F(crgpu_umap_args, wave_row_len),
              ABI_F(crgpu_umap_args, rows_per_wg),
              ABI_F(crgpu_umap_args, reserved0),
              ABI_F(crgpu_umap_args, reserved1)),
        ABI_S(crgpu_umap_result, ABI_F(crgpu_umap_result, rho_out),
              ABI_F(crgpu_umap_result, sigma_out),
              ABI_F(crgpu_umap_result, steps_out),
              ABI_F(crgpu_umap_result, indptr_out),
              ABI_F(crgpu_umap_result, indices_out),
              ABI_F(crgpu_umap_result, values_out),
              ABI_F(crgpu_umap_result, delta_out),
              ABI_F(crgpu_umap_result, wmax),
              ABI_F(crgpu_umap_result, fit_ms),
              ABI_F(crgpu_umap_result, search_ms),
              ABI_F(crgpu_umap_result, csr_ms),
              ABI_F(crgpu_umap_result, loop_ms),
              ABI_F(crgpu_umap_result, nnz),
              ABI_F(crgpu_umap_result, n_active),
              ABI_F(crgpu_umap_result, n_negative),
              ABI_F(crgpu_umap_result, wave_row_len),
              ABI_F(crgpu_umap_result, rows_per_wg),
              ABI_F(crgpu_umap_result, max_steps),
              ABI_F(crgpu_umap_result, reserved)),
        ABI_S(crgpu_louvain_args, ABI_F(crgpu_louvain_args, symmetrize),
              ABI_F(crgpu_louvain_args, max_rounds),
              ABI_F(crgpu_louvain_args, wave_deg_max),
              ABI_F(crgpu_louvain_args, lds_deg_max),
              ABI_F(crgpu_louvain_args, batch),
              ABI_F(crgpu_louvain_args, reserved0),
              ABI_F(crgpu_louvain_args, levels_capacity)),
        ABI_S(crgpu_louvain_result, ABI_F(crgpu_louvain_result, levels_out),
              ABI_F(crgpu_louvain_result, level0_out),
              ABI_F(crgpu_louvain_result, final_out),
              ABI_F(crgpu_louvain_result, level_nodes_out),
              ABI_F(crgpu_louvain_result, level_communities_out),
              ABI_F(crgpu_louvain_result, level_rounds_out),
              ABI_F(crgpu_louvain_result, level_S_out),
              ABI_F(crgpu_louvain_result, level_ms_out),
              ABI_F(crgpu_louvain_result, M),
              ABI_F(crgpu_louvain_result, levels_needed),
              ABI_F(crgpu_louvain_result, nnz),
              ABI_F(crgpu_louvain_result, fit_ms),
              ABI_F(crgpu_louvain_result, union_ms),
              ABI_F(crgpu_louvain_result, rounds_ms),
              ABI_F(crgpu_louvain_result, aggregate_ms),
              ABI_F(crgpu_louvain_result, n_levels),
              ABI_F(crgpu_louvain_result, wave_deg_max),
              ABI_F(crgpu_louvain_result, lds_deg_max),
              ABI_F(crgpu_louvain_result, batch)),
        ABI_S(crgpu_pca_args, ABI_F(crgpu_pca_args, pca_bc_indices),
              ABI_F(crgpu_pca_args, n_pca_bcs),
              ABI_F(crgpu_pca_args, start),
              ABI_F(crgpu_pca_args, n_start),
              ABI_F(crgpu_pca_args, n_components),
              ABI_F(crgpu_pca_args, pca_features),
              ABI_F(crgpu_pca_args, min_count_threshold),
              ABI_F(crgpu_pca_args, seed),
              ABI_F(crgpu_pca_args, wave_block),
              ABI_F(crgpu_pca_args, dot_parts_per_block),
              ABI_F(crgpu_pca_args, reserved0),
              ABI_F(crgpu_pca_args, reserved1)),
        ABI_S(crgpu_pca_result, ABI_F(crgpu_pca_result, transformed_out),
              ABI_F(crgpu_pca_result, components_out),
              ABI_F(crgpu_pca_result, variance_explained_out),
              ABI_F(crgpu_pca_result, dispersion_out),
              ABI_F(crgpu_pca_result, features_selected_out),
              ABI_F(crgpu_pca_result, d_out),
              ABI_F(crgpu_pca_result, fit_ms),
              ABI_F(crgpu_pca_result, prepare_ms),
              ABI_F(crgpu_pca_result, lanczos_ms),
              ABI_F(crgpu_pca_result, project_ms),
              ABI_F(crgpu_pca_result, n_thresholded_barcodes),
              ABI_F(crgpu_pca_result, n_pca_barcodes),
              ABI_F(crgpu_pca_result, status),
              ABI_F(crgpu_pca_result, n_components),
              ABI_F(crgpu_pca_result, n_used_features),
              ABI_F(crgpu_pca_result, n_thresholded_features),
              ABI_F(crgpu_pca_result, it),
              ABI_F(crgpu_pca_result, mprod),
              ABI_F(crgpu_pca_result, m_b),
              ABI_F(crgpu_pca_result, reserved)),
    };
    return t;
}
}  // namespace

extern "C" int crgpu_abi_layout(const char *struct_name, uint32_t *out, uint32_t cap) {
    if (!struct_name) return CRGPU_EINVAL;
    for (const AbiStruct &s : abi_table()) {
        if (strcmp(s.name, struct_name) != 0) continue;
        std::vector<uint32_t> w = {s.size, s.align, (uint32_t)s.fields.size()};
        for (const AbiField &f : s.fields) {
            w.push_back(f.offset);
            w.push_back(f.size);
        }
        for (uint32_t i = 0; i < w.size() && i < cap && out; i++) out[i] = w[i];
        return (int)w.size();
    }
    return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_abi_layout: no public struct named %s", struct_name);
}

extern "C" const char *crgpu_last_error(const crgpu_ctx *ctx) {
    return ctx ? ctx->err.c_str() : g_thread_err.c_str();
}

extern "C" int crgpu_create(crgpu_ctx **out, int device_id, int n_ranks, int rank, const void *unique_id) {
    if (!out) return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_create: out is NULL");
    *out = nullptr;
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_create: rank %d of %d ranks", rank, n_ranks);
    if (n_ranks > 1 && !unique_id)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_create: %d ranks need a unique_id (crgpu_get_unique_id / crgpu_local_group_id)",
                       n_ranks);
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return cr_fail(nullptr, CRGPU_ENODEV,
                       "crgpu_create: no HIP device visible (%s); libcrgpu has no CPU fallback",
                       e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
    if (device_id < 0 || device_id >= n_dev)
        return cr_fail(nullptr, CRGPU_EINVAL, "crgpu_create: device_id %d out of range [0,%d)", device_id, n_dev);
    e = hipSetDevice(device_id);
    if (e != hipSuccess) return cr_fail(nullptr, CRGPU_ENODEV, "hipSetDevice(%d): %s", device_id, hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess) return cr_fail(nullptr, CRGPU_ENODEV, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return cr_fail(nullptr, CRGPU_ENODEV, "device %d is %s; libcrgpu is built for gfx950 (MI355X) only", device_id,
                       prop.gcnArchName);

    crgpu_ctx *ctx = new (std::nothrow) crgpu_ctx();
    if (!ctx) return cr_fail(nullptr, CRGPU_ENOMEM, "crgpu_create: out of host memory");
    ctx->device = device_id;
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete ctx;
        return cr_fail(nullptr, CRGPU_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    // the second stream carries the branch of the count stage that is NOT the critical path (candidate filter + hash sort beside
    // the UMI correction): lowest priority, so that its kernels fill what the main stream leaves
    int prio_least = 0, prio_greatest = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, prio_least) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();  // the count stage then stays on the one stream
        if (ctx->stream2) hipStreamDestroy(ctx->stream2);
        ctx->stream2 = nullptr;
    }
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b) ctx->pool_budget = (uint64_t)total_b / 2;
    }
    if (const char *cap = getenv("CRGPU_PROBE_SEG_CAP")) ctx->probe_seg_cap = (uint32_t)strtoul(cap, nullptr, 10);  // tests: force the global route
    if (const char *b = getenv("CRGPU_MG_BATCH")) ctx->mg_batch = (uint32_t)strtoul(b, nullptr, 10);  // tests: small batches of the multi-genome bootstrap
    if (const char *b = getenv("CRGPU_JIBES_BATCH")) ctx->jibes_batch = (uint32_t)strtoul(b, nullptr, 10);  // tests: EM rounds between two reads of the stop latch
    if (const char *b = getenv("CRGPU_MG_LDS_CELLS")) {  // tests: the LDS / device-memory seam
        const unsigned long v = strtoul(b, nullptr, 10);
        ctx->mg_lds_cells = v < 32768ul ? (uint32_t)v : 32768u;
    }
    if (const char *b = getenv("CRGPU_ORDMAG_BATCH")) ctx->ordmag_batch = (uint32_t)strtoul(b, nullptr, 10);  // tests: small batches of the cell call
    if (const char *f = getenv("CRGPU_ED_LDS_FEATURES")) ctx->ed_lds_features = (uint32_t)strtoul(f, nullptr, 10);  // tests: 0 = counters in global memory
    if (const char *f = getenv("CRGPU_MS_LDS_FEATURES")) ctx->ms_lds_features = (uint32_t)strtoul(f, nullptr, 10);  // tests: several slices on a small matrix; 0 = counters in device memory
    if (const char *f = getenv("CRGPU_FM_LDS_FEATURES")) ctx->fm_lds_features = (uint32_t)strtoul(f, nullptr, 10);  // tests: several slices on a small feature set; 0 = counters in device memory
    if (const char *f = getenv("CRGPU_GMM_LDS_VALUES")) ctx->gmm_lds_values = (uint32_t)strtoul(f, nullptr, 10);    // tests: 0 = the mixture fit reads its values from device memory
    if (const char *f = getenv("CRGPU_MC_LDS_VALUES")) ctx->mc_lds_values = (uint32_t)strtoul(f, nullptr, 10);      // tests: 0 = the marginal caller reads its histograms from device memory
    if (const char *f = getenv("CRGPU_KM_LDS_CENTERS")) ctx->km_lds_centers = std::min<uint32_t>((uint32_t)strtoul(f, nullptr, 10), 4096u);  // tests: 0 = the k-means assign pass reads its centres from device memory
    if (const char *b = getenv("CRGPU_KM_BATCH")) ctx->km_batch = (uint32_t)strtoul(b, nullptr, 10);                // tests: Lloyd rounds between two reads of the stop latches
    if (const char *r = getenv("CRGPU_AGG_LDS_ROWS")) ctx->agg_lds_rows = (uint32_t)strtoul(r, nullptr, 10);  // tests: several slices of signal rows; 0 = the rank table in device memory
    if (const char *v = getenv("CRGPU_SS_WAVE_MIN")) ctx->ss_wave_min = (uint32_t)strtoul(v, nullptr, 10);  // tests: reach the wave path of the subsampling draw
    if (const char *v = getenv("CRGPU_SS_WG_MIN")) ctx->ss_wg_min = (uint32_t)strtoul(v, nullptr, 10);      // ... and its workgroup path
    if (const char *v = getenv("CRGPU_SS_TASK_BATCH")) ctx->ss_task_batch = (uint32_t)strtoul(v, nullptr, 10);  // tests: small task batches
    // probability(q) = 10^(-(q-33)/10) computed on the HOST with libm pow, exactly as the
    // reference does per call (corrector.rs:167-171), for every 7-bit quality character.
    double ptab[128];
    for (int q = 0; q < 128; q++) ptab[q] = std::pow(10.0, -((double)q - 33.0) / 10.0);
    if (hipMalloc(&ctx->d_ptab, sizeof(ptab)) != hipSuccess ||
        hipMemcpy(ctx->d_ptab, ptab, sizeof(ptab), hipMemcpyHostToDevice) != hipSuccess ||
        hipMalloc(&ctx->d_scalars, 4096) != hipSuccess || hipMemset(ctx->d_scalars, 0, 4096) != hipSuccess ||
        hipMalloc(&ctx->d_sort_hist, sizeof(uint32_t) * (256 * 2048 + 512)) != hipSuccess) {
        crgpu_destroy(ctx);
        return cr_fail(nullptr, CRGPU_ENOMEM, "crgpu_create: device allocation failed");
    }
    if (unique_id) {
        // blocks until every rank has arrived; the message of a failure is kept for crgpu_last_error(NULL)
        const int rc = cr_comm_init(ctx, n_ranks, rank, unique_id);
        if (rc != CRGPU_OK) {
            const std::string msg = ctx->err;
            crgpu_destroy(ctx);
            return cr_fail(nullptr, rc, "%s", msg.c_str());
        }
    }
    *out = ctx;
    return CRGPU_OK;
}

extern "C" int crgpu_comm_info(crgpu_ctx *ctx, uint32_t *n_ranks_out, uint32_t *rank_out) {
    if (!ctx) return CRGPU_EINVAL;
    if (n_ranks_out) *n_ranks_out = (uint32_t)ctx->n_ranks;
    if (rank_out) *rank_out = (uint32_t)ctx->rank;
    return CRGPU_OK;
}

extern "C" int crgpu_set_option(crgpu_ctx *ctx, int option, int64_t value) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    switch (option) {
        case CRGPU_OPT_BUFFERS_UNCHANGED_BETWEEN_CALLS:
            ctx->trust_buffers = value != 0;
            cr_invalidate(ctx);
            return CRGPU_OK;
        case CRGPU_OPT_DENSE_BARCODE_KEYS:
            cr_invalidate(ctx);
            cr_dense_drop(ctx);
            ctx->dense.on = value != 0;
            return CRGPU_OK;
        default:
            return cr_fail(ctx, CRGPU_EINVAL, "crgpu_set_option: unknown option %d", option);
    }
}

extern "C" int crgpu_get_stat(crgpu_ctx *ctx, int which, uint64_t *value_out) {
    if (!ctx || !value_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    switch (which) {
        case CRGPU_STAT_SORT_FALLBACKS:
            *value_out = ctx->sort_fallbacks;
            return CRGPU_OK;
        case CRGPU_STAT_SORT_REFINISHED:
            *value_out = ctx->sort_refinished;
            return CRGPU_OK;
        case CRGPU_STAT_RL_COUNTS_FROM_FINISH:
            *value_out = ctx->rl_counts_from_finish;
            return CRGPU_OK;
        case CRGPU_STAT_K1_SPLIT_ROUNDS:
            *value_out = ctx->k1_split_rounds;
            return CRGPU_OK;
        case CRGPU_STAT_K2_SORTED_READS:
            *value_out = ctx->k2_sorted_reads;
            return CRGPU_OK;
        case CRGPU_STAT_K2_RECORD_READS:
            *value_out = ctx->k2_record_reads;
            return CRGPU_OK;
        case CRGPU_STAT_COMM_BYTES_C1:
        case CRGPU_STAT_COMM_BYTES_C2:
        case CRGPU_STAT_COMM_BYTES_C3:
            *value_out = ctx->comm_bytes[which - CRGPU_STAT_COMM_BYTES_C1];
            return CRGPU_OK;
        case CRGPU_STAT_FEATURE_RESUMED_READS:
            *value_out = ctx->feature_resumed_reads;
            return CRGPU_OK;
        case CRGPU_STAT_FEATURE_FAST_LAUNCHES:
            *value_out = ctx->feature_fast_launches;
            return CRGPU_OK;
        case CRGPU_STAT_MISS_RECORD_SETS: {
            uint64_t k = 0;
            for (const MissRecords &r : ctx->recs) k += r.valid ? 1u : 0u;
            *value_out = k;
            return CRGPU_OK;
        }
        case CRGPU_STAT_DISTINCT_KEYS:
            *value_out = ctx->last_distinct_keys;
            return CRGPU_OK;
        case CRGPU_STAT_LOW_SUPPORT_CANDIDATES:
            *value_out = ctx->last_low_support_candidates;
            return CRGPU_OK;
        case CRGPU_STAT_FEATURE_READS_REQUEUED:
            *value_out = ctx->feature_reads_requeued;
            return CRGPU_OK;
        case CRGPU_STAT_PROBE_SEGMENTS_WAVE:
        case CRGPU_STAT_PROBE_SEGMENTS_WORKGROUP:
        case CRGPU_STAT_PROBE_SEGMENTS_GLOBAL:
            *value_out = ctx->probe_segments[which - CRGPU_STAT_PROBE_SEGMENTS_WAVE];
            return CRGPU_OK;
        default:
            return cr_fail(ctx, CRGPU_EINVAL, "crgpu_get_stat: unknown counter %d", which);
    }
}

void cr_invalidate(crgpu_ctx *ctx) {
    cr_drop_miss_records(ctx);
    cr_drop_feature_pending(ctx);
    ctx->ghist.valid = false;
}
// the same for a call that writes [p, p + bytes) of the caller's memory and nothing else: only the by-products that describe
// (a buffer overlapping) that range go -- the feature extraction between pass A and pass B writes the feature indices, not the
// barcodes pass A's miss records are about
void cr_invalidate_range(crgpu_ctx *ctx, const void *p, uint64_t bytes) {
    if (!p || !bytes) return;
    const uintptr_t a = (uintptr_t)p, b = a + bytes;
    auto hits = [&](const void *q, uint64_t len) { return q && (uintptr_t)q < b && (uintptr_t)q + len > a; };
    for (MissRecords &r : ctx->recs)
        if (r.valid && (hits(r.d_cb, r.n * 4) || hits(r.d_flags, r.n) || hits(r.d_idx, r.n * 4))) cr_drop_miss_records(ctx, r);
    const FxPendingSet &f = ctx->fxp;
    // (rows: at most stride bytes each; the outputs: 4 bytes per read and id / capture -- bounded generously)
    if (f.valid && (hits(f.d_seq, f.n * (uint64_t)(f.stride ? f.stride : 1)) || hits(f.d_qual, f.n * (uint64_t)(f.stride ? f.stride : 1)) ||
                    hits(f.d_len, f.n * 4) || hits(f.d_feature_out, f.n * 4) || hits(f.d_n_ids_out, f.n * 4) ||
                    hits(f.d_capture_out, f.n * 4)))
        cr_drop_feature_pending(ctx);
    const KeyHistograms &g = ctx->ghist;
    if (g.valid && hits(g.d_keys, g.n * 8)) ctx->ghist.valid = false;
}
void cr_dense_drop(crgpu_ctx *ctx) {
    if (!ctx->dense.valid) return;
    ctx->dense.valid = false;
    ctx->dense.V = 0;
    if (ctx->layout.set) ctx->layout.bits_bc = ctx->dense.canon_bits;
    ctx->ghist.valid = false;
}
void cr_dense_free(crgpu_ctx *ctx) {
    cr_dense_drop(ctx);
    (void)hipFree(ctx->dense.d_fwd);
    (void)hipFree(ctx->dense.d_back);
    ctx->dense.d_fwd = nullptr;
    ctx->dense.d_back = nullptr;
}

extern "C" int crgpu_invalidate(crgpu_ctx *ctx) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    cr_invalidate(ctx);
    cr_dense_drop(ctx);  // the host may have written a histogram table through crgpu_counts_dev (rebuilt from the tables on demand)
    return CRGPU_OK;
}

static void free_wl(WlTables &w) {
    hipFree(w.d_offA);
    hipFree(w.d_tailA);
    hipFree(w.d_valA);
    hipFree(w.d_offB);
    hipFree(w.d_offE);
    hipFree(w.d_headB);
    hipFree(w.d_valB);
    hipFree(w.d_key_of_rank);
    hipFree(w.d_valid);
    hipFree(w.d_corrected);
    hipFree(w.d_prior_override);
    w = WlTables();
}

void cr_free_wl(WlTables &w) { free_wl(w); }

extern "C" void crgpu_destroy(crgpu_ctx *ctx) {
    if (!ctx) return;
    int prev_dev = -1;
    (void)hipGetDevice(&prev_dev);
    hipSetDevice(ctx->device);
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    cr_comm_destroy(ctx);
    for (auto &w : ctx->wl) free_wl(w);
    for (auto &p : ctx->pat) {
        hipFree(p.d_seq);
        hipFree(p.d_index);
        hipFree(p.d_dist);
    }
    cr_feature_extractors_free(ctx);
    cr_dense_free(ctx);
    hipFree(ctx->d_on_target);
    hipFree(ctx->d_canon_keys);
    hipFree(ctx->d_hot_image);
    hipFree(ctx->d_ptab);
    hipFree(ctx->d_scalars);
    hipFree(ctx->d_sort_hist);
    hipFree(ctx->d_scratch);
    cr_pool_release_all(ctx);
    for (auto &s : ctx->spans) {
        hipEventDestroy(s.start);
        hipEventDestroy(s.stop);
    }
    for (auto ev : ctx->event_pool) hipEventDestroy(ev);
    if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) hipEventDestroy(ctx->ev_join);
    if (ctx->stream2) hipStreamDestroy(ctx->stream2);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
}

extern "C" int crgpu_synchronize(crgpu_ctx *ctx) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRGPU_OK;
}

extern "C" void *crgpu_stream(crgpu_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }

extern "C" int crgpu_malloc(crgpu_ctx *ctx, void **d_out, uint64_t bytes) {
    if (!ctx || !d_out) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    return cr_pool_alloc(ctx, d_out, bytes);
}

extern "C" int crgpu_free(crgpu_ctx *ctx, void *d_ptr) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    cr_invalidate(ctx);  // a by-product must not outlive the buffer it describes (the pool hands the address out again)
    cr_pool_free(ctx, d_ptr);
    return CRGPU_OK;
}

extern "C" int crgpu_trim(crgpu_ctx *ctx) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < ctx->pool.size();) {
        if (!ctx->pool[i].in_use) {
            (void)hipFree(ctx->pool[i].p);
            ctx->pool.erase(ctx->pool.begin() + i);
        } else {
            i++;
        }
    }
    return CRGPU_OK;
}

extern "C" int crgpu_memcpy_h2d(crgpu_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    if (!bytes) return CRGPU_OK;
    cr_invalidate_range(ctx, d_dst, bytes);  // the destination may be a buffer a kept by-product describes
    CR_HIP(ctx, hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream));
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRGPU_OK;
}

extern "C" int crgpu_memcpy_d2h(crgpu_ctx *ctx, void *h_dst, const void *d_src, uint64_t bytes) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    if (!bytes) return CRGPU_OK;
    CR_HIP(ctx, hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return CRGPU_OK;
}

extern "C" int crgpu_memset(crgpu_ctx *ctx, void *d_dst, int value, uint64_t bytes) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    if (!bytes) return CRGPU_OK;
    cr_invalidate_range(ctx, d_dst, bytes);
    CR_HIP(ctx, hipMemsetAsync(d_dst, value, bytes, ctx->stream));
    return CRGPU_OK;
}

int cr_scratch(crgpu_ctx *ctx, uint64_t bytes, void **out) {
    if (bytes > ctx->scratch_bytes) {
        CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_scratch) CR_HIP(ctx, hipFree(ctx->d_scratch));
        ctx->d_scratch = nullptr;
        ctx->scratch_bytes = 0;
        uint64_t want = bytes + bytes / 8 + 4096;
        hipError_t e = hipMalloc(&ctx->d_scratch, want);
        if (e != hipSuccess)
            return cr_fail(ctx, CRGPU_ENOMEM, "workspace hipMalloc(%llu): %s", (unsigned long long)want, hipGetErrorString(e));
        ctx->scratch_bytes = want;
    }
    *out = ctx->d_scratch;
    return CRGPU_OK;
}

// ---- caching pool ----------------------------------------------------------------------------------

int cr_pool_alloc(crgpu_ctx *ctx, void **out, uint64_t bytes) {
    *out = nullptr;
    if (bytes == 0) bytes = 8;
    bytes = (bytes + 255) & ~255ull;
    // A free block of exactly this size if there is one.  Otherwise a new block, as long as the pool stays below
    // its budget: a step asks for the same sizes in the same order every time, so after ONE step every request
    // finds its own block (with a waste-tolerant best fit a request could take the block a later request needed,
    // and the second and third steps still paid multi-millisecond hipMallocs).  Above the budget: best fit among
    // the free blocks that waste at most 25 %.
    int best = -1;
    uint64_t pooled = 0;
    for (size_t i = 0; i < ctx->pool.size(); i++) {
        const auto &b = ctx->pool[i];
        pooled += b.bytes;
        if (!b.in_use && b.bytes == bytes && best < 0) best = (int)i;
    }
    if (best < 0 && pooled + bytes > ctx->pool_budget) {
        for (size_t i = 0; i < ctx->pool.size(); i++) {
            const auto &b = ctx->pool[i];
            if (b.in_use || b.bytes < bytes || b.bytes - bytes > bytes / 4 + 4096) continue;
            if (best < 0 || b.bytes < ctx->pool[best].bytes) best = (int)i;
        }
    }
    if (best >= 0) {
        ctx->pool[best].in_use = true;
        *out = ctx->pool[best].p;
        return CRGPU_OK;
    }
    void *p = nullptr;
    static const bool pool_debug = getenv("CRGPU_POOL_DEBUG") != nullptr;
    if (pool_debug) fprintf(stderr, "[crgpu pool] hipMalloc %llu bytes (%zu blocks cached)\n", (unsigned long long)bytes, ctx->pool.size());
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        // memory pressure: drop every cached free block and retry once
        (void)hipGetLastError();
        (void)hipStreamSynchronize(ctx->stream);
        for (size_t i = 0; i < ctx->pool.size();) {
            if (!ctx->pool[i].in_use) {
                (void)hipFree(ctx->pool[i].p);
                ctx->pool.erase(ctx->pool.begin() + i);
            } else {
                i++;
            }
        }
        e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess)
        return cr_fail(ctx, CRGPU_ENOMEM, "device pool hipMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e));
    ctx->pool.push_back({p, bytes, true});
    *out = p;
    return CRGPU_OK;
}

void cr_pool_free(crgpu_ctx *ctx, void *p) {
    if (!p || !ctx) return;
    for (auto &b : ctx->pool)
        if (b.p == p) {
            b.in_use = false;
            return;
        }
    (void)hipFree(p);  // not from the pool
}

void cr_pool_release_all(crgpu_ctx *ctx) {
    for (auto &b : ctx->pool) (void)hipFree(b.p);
    ctx->pool.clear();
}

// ---- timing ------------------------------------------------------------------------------------

hipEvent_t cr_take_event(crgpu_ctx *ctx) {
    if (!ctx->event_pool.empty()) {
        hipEvent_t e = ctx->event_pool.back();
        ctx->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}

CrTimer::CrTimer(crgpu_ctx *c, int s, uint64_t u) : ctx(c), slot(s), units(u) {
    if (!ctx->timing) return;
    start = cr_take_event(ctx);
    stop = cr_take_event(ctx);
    hipEventRecord(start, ctx->stream);
}

CrTimer::~CrTimer() {
    if (!start) return;
    hipEventRecord(stop, ctx->stream);
    ctx->spans.push_back({slot, start, stop, units});
}

static int drain_spans(crgpu_ctx *ctx) {
    CR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (auto &s : ctx->spans) {
        float ms = 0.f;
        CR_HIP(ctx, hipEventElapsedTime(&ms, s.start, s.stop));
        ctx->acc_ms[s.slot] += ms;
        ctx->acc_launches[s.slot] += 1;
        ctx->acc_units[s.slot] += s.units;
        ctx->event_pool.push_back(s.start);
        ctx->event_pool.push_back(s.stop);
    }
    ctx->spans.clear();
    return CRGPU_OK;
}

extern "C" int crgpu_timing_enable(crgpu_ctx *ctx, int on) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_TRY(drain_spans(ctx));
    ctx->timing = on != 0;
    return CRGPU_OK;
}

extern "C" int crgpu_timing_reset(crgpu_ctx *ctx) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_TRY(drain_spans(ctx));
    for (int i = 0; i < CRGPU_T_NSLOTS; i++) {
        ctx->acc_ms[i] = 0;
        ctx->acc_launches[i] = 0;
        ctx->acc_units[i] = 0;
    }
    return CRGPU_OK;
}

extern "C" int crgpu_timing_get(crgpu_ctx *ctx, double *ms_out, uint64_t *launches_out, uint64_t *units_out) {
    if (!ctx) return CRGPU_EINVAL;
    CR_ENTER(ctx);
    CR_TRY(drain_spans(ctx));
    for (int i = 0; i < CRGPU_T_NSLOTS; i++) {
        if (ms_out) ms_out[i] = ctx->acc_ms[i];
        if (launches_out) launches_out[i] = ctx->acc_launches[i];
        if (units_out) units_out[i] = ctx->acc_units[i];
    }
    return CRGPU_OK;
}
