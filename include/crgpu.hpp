// crgpu.hpp -- header-only C++17 host layer over the C ABI (include/crgpu.h), mirroring the
// reference's Rust interface for this path (names, argument meaning, error behaviour), in batch form:
//
//   crgpu::Whitelist        barcode/src/whitelist.rs:453-546       Whitelist::{Plain, Trans}
//   crgpu::Posterior        barcode/src/corrector.rs:92-109        thresholds, Default
//   crgpu::BarcodeCorrector barcode/src/corrector.rs:14-71         new(whitelist, bc_counts, strategy), correct_barcode
//   crgpu::DupBuilder       tx_annotation/src/mark_dups.rs:118-169 observe(...), build(...)
//   crgpu::BarcodeDupMarker tx_annotation/src/mark_dups.rs:171-363 -> UmiCount stream + feature_counts()
//   crgpu::FeatureExtractor cr_types/src/reference/feature_extraction.rs:176-470  new(feature defs, feat_dist), match_read,
//                           compile_pattern
//   crgpu::BarcodeIndex     cr_types/src/barcode_index.rs:14-53
//   crgpu::CountMatrix      cr_h5/src/count_matrix.rs:382-448, cr_lib/src/stages/write_matrix_market.rs:80-122
//   crgpu::filter_cellular_barcodes_ordmag / _fixed_cutoff  lib/python/cellranger/cell_calling_helpers.py:864-964 (Python there)
//   crgpu::find_nonambient_barcodes / compute_ambient_pvalues / sgt_proportions
//                           lib/python/cellranger/cell_calling.py:144-263, stats.py:205-231, sgt.py:97-132 (Python there)
//   crgpu::multigenome_analysis / multigenome_top_two  lib/python/cellranger/analysis/multigenome.py:80-335 (Python there)
//   crgpu::rtl_tags / rtl_sample_columns / rtl_gem_runs / rtl_medians / rtl_ab_thresholds / rtl_overlap_rows /
//   rtl_suspicious_pairings / rtl_occupancy_summary / remove_high_occupancy_gems
//                           lib/rust/cr_lib/src/stages/call_tags_rtl.rs:143-498, barcode_overlap.rs; cell_calling_helpers.py:315-424
//
// Errors are C++ exceptions carrying crgpu_last_error (the Rust returns anyhow::Result); nothing here
// computes on the CPU: every result comes from libcrgpu, and construction fails without a gfx950 device.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "crgpu.h"

namespace crgpu {

class Error : public std::runtime_error {
   public:
    Error(int code, const std::string &msg) : std::runtime_error("crgpu error " + std::to_string(code) + ": " + msg), code(code) {}
    int code;
};

class Context {
   public:
    // one GPU: Context(device); one rank of a multi-GPU well: Context(device, n_ranks, rank, id) with the id of
    // crgpu_get_unique_id (processes) or crgpu_local_group_id (threads of this process)
    explicit Context(int device_id = 0, int n_ranks = 1, int rank = 0, const void *unique_id = nullptr) {
        const int rc = crgpu_create(&h_, device_id, n_ranks, rank, unique_id);
        if (rc != CRGPU_OK) throw Error(rc, crgpu_last_error(nullptr));
    }
    ~Context() { crgpu_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    crgpu_ctx *get() const { return h_; }
    void check(int rc) const {
        if (rc != CRGPU_OK) throw Error(rc, crgpu_last_error(h_));
    }

   private:
    crgpu_ctx *h_ = nullptr;
};

/// SimpleHistogram<BcSegSeq> (metric/src/histogram.rs:26-32): sequence -> count, 0 when absent.
using SimpleHistogram = std::map<std::string, int64_t>;

/// Whitelist::{Plain, Trans}.  `translation` empty => Plain.
struct Whitelist {
    std::vector<std::string> sequences;    // raw sequences (file column 1)
    std::vector<std::string> translation;  // translated sequences (file column 2) or empty
    static Whitelist plain(std::vector<std::string> seqs) { return Whitelist{std::move(seqs), {}}; }
    static Whitelist trans(std::vector<std::string> raw, std::vector<std::string> translated) {
        return Whitelist{std::move(raw), std::move(translated)};
    }
};

/// Posterior (corrector.rs:92-109).
struct Posterior {
    double max_expected_barcode_errors = DBL_MAX;  // Default: f64::MAX
    double bc_confidence_threshold = 0.975;        // BARCODE_CONFIDENCE_THRESHOLD
};

/// BarcodeCorrector::new(whitelist, bc_counts, strategy) for one library type of a context.
/// `canon` is the canonical (matrix column) list of the GEM well; empty => the whitelist itself.
class BarcodeCorrector {
   public:
    BarcodeCorrector(Context &ctx, int lib, const Whitelist &wl, const SimpleHistogram &bc_counts, Posterior strategy = {},
                     const std::vector<std::string> &canon = {})
        : ctx_(ctx), lib_(lib) {
        if (wl.sequences.empty()) throw Error(CRGPU_EINVAL, "empty whitelist");
        len_ = (uint32_t)wl.sequences[0].size();
        const std::vector<std::string> &cn = !canon.empty() ? canon : (wl.translation.empty() ? wl.sequences : wl.translation);
        // canonical list: unique sequences in first-seen order
        std::map<std::string, uint32_t> canon_pos;
        std::string canon_flat;
        for (const auto &s : cn)
            if (canon_pos.emplace(s, (uint32_t)canon_pos.size()).second) canon_flat += s;
        std::string keys_flat;
        std::vector<uint32_t> translate_to;
        for (size_t i = 0; i < wl.sequences.size(); i++) {
            keys_flat += wl.sequences[i];
            if (!wl.translation.empty()) {
                auto it = canon_pos.find(wl.translation[i]);
                if (it == canon_pos.end()) throw Error(CRGPU_EINVAL, "translated sequence is not in the canonical list");
                translate_to.push_back(it->second);
            }
        }
        ctx_.check(crgpu_set_whitelist(ctx_.get(), lib, keys_flat.data(), (uint32_t)wl.sequences.size(), len_, canon_flat.data(),
                                       (uint32_t)canon_pos.size(), translate_to.empty() ? nullptr : translate_to.data()));
        // rank <-> sequence of the canonical space
        const uint32_t n = (uint32_t)canon_pos.size();
        std::vector<uint32_t> order(n);
        ctx_.check(crgpu_get_canon_order(ctx_.get(), order.data(), nullptr));
        rank_seq_.resize(n);
        std::vector<std::string> by_pos(n);
        for (const auto &kv : canon_pos) by_pos[kv.second] = kv.first;
        for (uint32_t r = 0; r < n; r++) rank_seq_[r] = by_pos[order[r]];
        for (uint32_t r = 0; r < n; r++) seq_rank_[rank_seq_[r]] = r;
        // prior = bc_counts keyed by the (translated) sequence
        std::vector<uint32_t> prior(n, 0);
        for (const auto &kv : bc_counts) {
            auto it = seq_rank_.find(kv.first);
            if (it != seq_rank_.end()) prior[it->second] = (uint32_t)kv.second;
        }
        ctx_.check(crgpu_set_counts(ctx_.get(), lib, CRGPU_COUNTS_PRIOR, prior.data()));
        ctx_.check(crgpu_set_posterior(ctx_.get(), strategy.max_expected_barcode_errors, strategy.bc_confidence_threshold));
    }

    /// Batch form of correct_barcode for Invalid segments: the corrected (translated) sequence, or
    /// nullopt when no correction is made.  quals may be empty (Option<BcSegQual> = None).
    std::vector<std::optional<std::string>> correct_barcodes(const std::vector<std::string> &seqs,
                                                             const std::vector<std::vector<uint8_t>> &quals) const {
        const size_t n = seqs.size();
        std::string flat;
        std::vector<uint8_t> q;
        for (size_t i = 0; i < n; i++) {
            if (seqs[i].size() != len_) throw Error(CRGPU_EINVAL, "barcode length differs from the whitelist's");
            flat += seqs[i];
            if (!quals.empty()) q.insert(q.end(), quals[i].begin(), quals[i].end());
        }
        std::vector<uint32_t> idx(n, CRGPU_MISS);
        std::vector<uint8_t> flag(n, 0);
        ctx_.check(crgpu_correct(ctx_.get(), lib_, reinterpret_cast<const uint8_t *>(flat.data()), quals.empty() ? nullptr : q.data(), n,
                                 idx.data(), flag.data()));
        std::vector<std::optional<std::string>> out(n);
        for (size_t i = 0; i < n; i++)
            if (flag[i]) out[i] = rank_seq_[idx[i]];
        return out;
    }
    std::optional<std::string> correct_barcode(const std::string &seq, const std::vector<uint8_t> &qual) const {
        return correct_barcodes({seq}, qual.empty() ? std::vector<std::vector<uint8_t>>{} : std::vector<std::vector<uint8_t>>{qual})[0];
    }
    /// Whitelist::check_and_update for a batch: translated sequence on a hit.
    std::vector<std::optional<std::string>> check_and_update(const std::vector<std::string> &seqs) const {
        std::string flat;
        for (const auto &s : seqs) flat += s;
        std::vector<uint32_t> idx(seqs.size(), CRGPU_MISS);
        ctx_.check(crgpu_match_and_count(ctx_.get(), lib_, reinterpret_cast<const uint8_t *>(flat.data()), nullptr, seqs.size(), idx.data()));
        std::vector<std::optional<std::string>> out(seqs.size());
        for (size_t i = 0; i < seqs.size(); i++)
            if (idx[i] != CRGPU_MISS) out[i] = rank_seq_[idx[i]];
        return out;
    }
    uint32_t rank_of(const std::string &seq) const { return seq_rank_.at(seq); }
    const std::string &sequence_of(uint32_t rank) const { return rank_seq_[rank]; }
    uint32_t barcode_length() const { return len_; }

   private:
    Context &ctx_;
    int lib_;
    uint32_t len_ = 0;
    std::vector<std::string> rank_seq_;
    std::map<std::string, uint32_t> seq_rank_;
};

/// UmiCount (cr_types/src/types.rs:152-160) without probe_idx (BarcodeDupMarker::probe_counts carries the histogram of it).
struct UmiCount {
    uint32_t barcode_rank;
    uint16_t library_idx;
    uint32_t feature_idx, umi, read_count;
    uint8_t utype;  // 0 Txomic, 1 NonTxomic
};
/// FeatureBarcodeCount (types.rs:121-137), BarcodeThenFeatureOrder.
struct FeatureBarcodeCount {
    uint32_t barcode_rank, feature_idx, umi_count;
};

/// ProbeBarcodeCount (types.rs:141-146), ordered by (barcode, probe_idx) as its derived Ord.
struct ProbeBarcodeCount {
    uint32_t barcode, probe_idx, umi_count;  // barcode = canonical rank
};

/// Result of DupBuilder::build: what BarcodeDupMarker::process + BcUmiInfo::feature_counts yield for all
/// barcodes of the batch.
/// DupInfo (mark_dups.rs:61-72): what BarcodeDupMarker::process returns for one read.
struct DupInfo {
    uint32_t processed_umi;  // 2-bit packed corrected UMI
    uint32_t read_count;     // reads of the read's molecule (UmiCount::read_count)
    bool is_corrected, is_low_support_umi, is_umi_count;
};

/// BarcodeSummary (cr_lib/src/aligner.rs:33-68) with the barcode as its canonical rank and the library id in place of
/// the LibraryType; `reads` comes from the context's histograms (the reads check_and_update / correct_barcodes saw).
struct BarcodeSummary {
    uint32_t barcode_rank, library;
    uint64_t reads, umis, candidate_dup_reads, umi_corrected_reads;
};

struct BarcodeDupMarker {
    std::vector<BarcodeSummary> barcode_summaries;    // ordered by (library, barcode), one per barcode with a read
    std::vector<UmiCount> umi_counts;                 // sorted per barcode as align_and_count.rs:314
    std::vector<FeatureBarcodeCount> feature_counts;  // sorted by (barcode, feature)
    /// BcUmiInfo::probe_counts (types.rs:190-204) of every barcode: filled when a read was observed with a probe
    std::vector<ProbeBarcodeCount> probe_counts;      // sorted by (barcode, probe_idx)
    /// process(read): one entry per observe() call, in call order (the order stands in for the qname
    /// rank: observe reads in read-header order).  nullopt = process() returned None.
    std::vector<std::optional<DupInfo>> dup_infos;
};

/// DupBuilder: observe() every annotated read of a batch (any number of barcodes / library types), then
/// build().  umi: ASCII; umi_qual: FASTQ quality bytes; feature: conf_mapped_feature or CRGPU_NO_FEATURE.
class DupBuilder {
   public:
    DupBuilder(Context &ctx, uint32_t n_features, uint32_t umi_len, uint32_t n_libs = 1, uint32_t multiplexing_lib_mask = 0)
        : ctx_(ctx), n_features_(n_features), umi_len_(umi_len) {
        ctx_.check(crgpu_set_key_layout(ctx_.get(), n_features, umi_len, n_libs, multiplexing_lib_mask));
    }
    /// probe_idx: the read's confidently mapped LHS probe (RTL / Flex reads, mark_dups.rs:332-342) or CRGPU_NO_PROBE
    void observe(uint32_t barcode_rank, int lib, const std::string &umi, const std::vector<uint8_t> &umi_qual, uint32_t feature,
                 bool is_txomic = true, int32_t probe_idx = CRGPU_NO_PROBE) {
        if (umi.size() != umi_len_ || umi_qual.size() != umi_len_) throw Error(CRGPU_EINVAL, "UMI length differs from the layout's");
        uint32_t packed = 0;
        for (uint32_t j = 0; j < umi_len_; j++) {
            const char c = umi[j];
            const uint32_t code = c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
            packed = (packed << 2) | (code & 3u);
            qualn_.push_back((uint8_t)((umi_qual[j] > 127 ? 127 : umi_qual[j]) | (code == 4u ? 0x80u : 0u)));
        }
        bc_.push_back(barcode_rank);
        umi_.push_back(packed);
        feature_.push_back(feature);
        flags_.push_back((uint8_t)((lib & 0x0F) | (is_txomic ? 0 : CRGPU_FLAG_NONTXOMIC)));
        if (probe_idx < CRGPU_NO_PROBE) throw Error(CRGPU_ERANGE, "probe_idx below CRGPU_NO_PROBE");
        probe_.push_back(probe_idx);
        if (probe_idx >= 0 && (uint32_t)probe_idx + 1u > n_probes_) n_probes_ = (uint32_t)probe_idx + 1u;
    }
    /// keep (nullable): receives the crgpu_counts of the batch (what crgpu::run_subsampling takes) instead of their being freed;
    /// release them with crgpu_counts_free.  *keep stays NULL for an empty batch.
    BarcodeDupMarker build(crgpu_counts **keep = nullptr) {
        if (keep) *keep = nullptr;
        const uint64_t n = bc_.size();
        struct Dev {
            const Context &c;
            void *p = nullptr;
            Dev(const Context &c, const void *h, uint64_t bytes) : c(c) {
                c.check(crgpu_malloc(c.get(), &p, bytes));
                c.check(crgpu_memcpy_h2d(c.get(), p, h, bytes));
            }
            ~Dev() { crgpu_free(c.get(), p); }
        };
        BarcodeDupMarker out;
        if (n == 0) return out;
        Dev d_bc(ctx_, bc_.data(), n * 4), d_umi(ctx_, umi_.data(), n * 4), d_q(ctx_, qualn_.data(), n * umi_len_),
            d_f(ctx_, feature_.data(), n * 4), d_fl(ctx_, flags_.data(), n);
        std::vector<uint32_t> pu(n), rc32(n);
        std::vector<uint8_t> df(n);
        Dev d_pu(ctx_, pu.data(), n * 4), d_rc(ctx_, rc32.data(), n * 4), d_df(ctx_, df.data(), n);
        Dev d_pr(ctx_, probe_.data(), n * 4);
        crgpu_records recs{n, umi_len_, (const uint32_t *)d_bc.p, (const uint32_t *)d_umi.p, (const uint8_t *)d_q.p,
                           (const uint32_t *)d_f.p, (const uint8_t *)d_fl.p};
        if (n_probes_) recs.d_probe_idx = (const int32_t *)d_pr.p;
        crgpu_counts *c = nullptr;
        ctx_.check(crgpu_count_records_dev(ctx_.get(), &recs, &c, (uint32_t *)d_pu.p, (uint32_t *)d_rc.p, (uint8_t *)d_df.p));
        uint64_t nt = 0, nm = 0;
        ctx_.check(crgpu_counts_info(ctx_.get(), c, &nt, &nm));
        std::vector<uint32_t> tb(nt), tf(nt), tc(nt), mb(nm), mf(nm), mu(nm), mr(nm);
        std::vector<uint8_t> ml(nm), mt(nm);
        int rc = crgpu_counts_triplets(ctx_.get(), c, tb.data(), tf.data(), tc.data());
        if (rc == CRGPU_OK) rc = crgpu_counts_molecules(ctx_.get(), c, mb.data(), ml.data(), mf.data(), mu.data(), mr.data(), mt.data());
        std::vector<crgpu_barcode_summary_row> rows;
        if (rc == CRGPU_OK) {
            uint64_t n_rows = 0;
            rc = crgpu_counts_barcode_summary(ctx_.get(), c, 0, 0xFFFFFFFFu, nullptr, 0, &n_rows);
            rows.resize(n_rows);
            if (rc == CRGPU_OK && n_rows)
                rc = crgpu_counts_barcode_summary(ctx_.get(), c, 0, 0xFFFFFFFFu, rows.data(), n_rows, &n_rows);
        }
        std::vector<uint32_t> pb, pp, pc;
        if (rc == CRGPU_OK && n_probes_) {
            uint64_t np = 0;
            rc = crgpu_counts_probe_triplets(ctx_.get(), c, n_probes_, nullptr, nullptr, nullptr, &np);
            pb.resize(np), pp.resize(np), pc.resize(np);
            if (rc == CRGPU_OK && np) rc = crgpu_counts_probe_triplets(ctx_.get(), c, n_probes_, pb.data(), pp.data(), pc.data(), &np);
        }
        if (keep && rc == CRGPU_OK)
            *keep = c;
        else
            crgpu_counts_free(ctx_.get(), c);
        ctx_.check(rc);
        ctx_.check(crgpu_memcpy_d2h(ctx_.get(), pu.data(), d_pu.p, n * 4));
        ctx_.check(crgpu_memcpy_d2h(ctx_.get(), rc32.data(), d_rc.p, n * 4));
        ctx_.check(crgpu_memcpy_d2h(ctx_.get(), df.data(), d_df.p, n));
        out.dup_infos.resize(n);
        for (uint64_t i = 0; i < n; i++)
            if (df[i] & CRGPU_DUP_HAS)
                out.dup_infos[i] = DupInfo{pu[i], rc32[i], (df[i] & CRGPU_DUP_CORRECTED) != 0, (df[i] & CRGPU_DUP_LOW_SUPPORT) != 0,
                                           (df[i] & CRGPU_DUP_UMI_COUNT) != 0};
        for (const auto &r : rows)
            out.barcode_summaries.push_back({r.barcode_rank, r.library, r.reads, r.umis, r.candidate_dup_reads, r.umi_corrected_reads});
        for (uint64_t i = 0; i < nt; i++) out.feature_counts.push_back({tb[i], tf[i], tc[i]});
        for (size_t i = 0; i < pb.size(); i++) out.probe_counts.push_back({pb[i], pp[i], pc[i]});
        for (uint64_t i = 0; i < nm; i++) out.umi_counts.push_back({mb[i], ml[i], mf[i], mu[i], mr[i], mt[i]});
        return out;
    }

   private:
    Context &ctx_;
    uint32_t n_features_, umi_len_;
    std::vector<uint32_t> bc_, umi_, feature_;
    std::vector<uint8_t> qualn_, flags_;
    std::vector<int32_t> probe_;
    uint32_t n_probes_ = 0;  // largest probe_idx observed + 1 (0: no read carried a probe)
};

/// FeatureDef (cr_types/src/reference/feature_reference.rs): the columns FeatureExtractor reads.
struct FeatureDef {
    uint32_t index;        // position in the feature reference (and in feat_dist)
    std::string pattern;   // "5PNNNNNNNNNN(BC)", "^(BC)", "(BC)GTTTAAG...", bare "(BC)"
    std::string sequence;  // A/C/G/T
    int read;              // WhichRead: 0 = R1, 1 = R2
};

/// FeatureData (feature_extraction.rs:163-173) of one read: ids as feature indices, barcode / qual as a span of the read.
struct FeatureData {
    std::vector<uint32_t> ids;        // one id when the read is counted; its value is ids[0] (more ids: only the count is kept)
    uint32_t n_ids = 0;
    int read = 0;
    uint32_t start = 0, len = 0;
    bool corrected = false;           // corrected_barcode is Some
};

/// FeatureExtractor of ONE feature type (match_read skips the definitions of other types, :376-378): new() compiles the
/// patterns (errors as the reference's: invalid pattern / sequence, duplicate definition), match_read runs on the GPU.
class FeatureExtractor {
   public:
    FeatureExtractor(Context &ctx, int slot, const std::vector<FeatureDef> &defs, const std::vector<double> *feat_dist = nullptr)
        : ctx_(ctx), slot_(slot) {
        std::vector<crgpu_feature_def> d(defs.size());
        for (size_t k = 0; k < defs.size(); k++)
            d[k] = crgpu_feature_def{defs[k].pattern.c_str(), defs[k].sequence.c_str(), defs[k].index, (uint32_t)defs[k].read};
        ctx_.check(crgpu_set_feature_extractor(ctx_.get(), slot_, d.data(), (uint32_t)d.size(), feat_dist ? feat_dist->data() : nullptr,
                                               feat_dist ? (uint32_t)feat_dist->size() : 0u));
    }
    /// compile_pattern (:307-343): the regular expression as text; throws for a pattern the reference rejects
    static std::string compile_pattern(const std::string &pattern, uint32_t length) {
        char buf[4096];
        const int rc = crgpu_compile_feature_pattern(pattern.c_str(), length, buf, sizeof(buf));
        if (rc != CRGPU_OK) throw Error(rc, "Invalid pattern: '" + pattern + "'");
        return buf;
    }
    /// regex_str of every compiled pattern (tethered ones as compile_pattern gives them, bare groups as compile_bare_patterns)
    std::vector<std::string> regexes() const {
        uint32_t n = 0;
        ctx_.check(crgpu_feature_extractor_regex(ctx_.get(), slot_, 0, nullptr, 0, &n));
        std::vector<std::string> out;
        std::vector<char> buf(1 << 20);
        for (uint32_t p = 0; p < n; p++) {
            ctx_.check(crgpu_feature_extractor_regex(ctx_.get(), slot_, p, buf.data(), buf.size(), nullptr));
            out.emplace_back(buf.data());
        }
        return out;
    }
    /// match_read (:358-441) for a batch of read pairs (either read may be absent: empty vectors); nullopt = None
    std::vector<std::optional<FeatureData>> match_reads(const std::vector<std::string> &r1_seq, const std::vector<std::string> &r1_qual,
                                                        const std::vector<std::string> &r2_seq,
                                                        const std::vector<std::string> &r2_qual) const {
        const size_t n = r1_seq.empty() ? r2_seq.size() : r1_seq.size();
        Rows a = upload(r1_seq, r1_qual), b = upload(r2_seq, r2_qual);
        DevBuf f(ctx_, n * 4), ni(ctx_, n * 4), cap(ctx_, n * 4);
        ctx_.check(crgpu_extract_features_dev(ctx_.get(), slot_, a.seq.u8(), a.qual.u8(), a.len.u32(), a.stride, b.seq.u8(), b.qual.u8(),
                                              b.len.u32(), b.stride, n, f.u32(), ni.u32(), cap.u32()));
        std::vector<uint32_t> hf(n), hn(n), hc(n);
        ctx_.check(crgpu_memcpy_d2h(ctx_.get(), hf.data(), f.p, n * 4));
        ctx_.check(crgpu_memcpy_d2h(ctx_.get(), hn.data(), ni.p, n * 4));
        ctx_.check(crgpu_memcpy_d2h(ctx_.get(), hc.data(), cap.p, n * 4));
        std::vector<std::optional<FeatureData>> out(n);
        for (size_t i = 0; i < n; i++) {
            if (hc[i] == CRGPU_NO_CAPTURE) continue;
            FeatureData d;
            d.corrected = (hc[i] >> 31) != 0;
            d.read = (int)((hc[i] >> 30) & 1u);
            d.start = (hc[i] >> 8) & 0x3FFFFFu;
            d.len = hc[i] & 0xFFu;
            d.n_ids = hn[i];
            if (hn[i] == 1) d.ids.push_back(hf[i]);
            out[i] = d;
        }
        return out;
    }

   private:
    struct DevBuf {
        Context &c;
        void *p = nullptr;
        DevBuf(Context &ctx, size_t bytes) : c(ctx) {
            if (bytes) c.check(crgpu_malloc(c.get(), &p, bytes));
        }
        ~DevBuf() {
            if (p) crgpu_free(c.get(), p);
        }
        DevBuf(const DevBuf &) = delete;
        DevBuf(DevBuf &&o) noexcept : c(o.c), p(o.p) { o.p = nullptr; }
        uint8_t *u8() const { return (uint8_t *)p; }
        uint32_t *u32() const { return (uint32_t *)p; }
    };
    struct Rows {
        DevBuf seq, qual, len;
        uint32_t stride;
    };
    Rows upload(const std::vector<std::string> &seq, const std::vector<std::string> &qual) const {
        uint32_t stride = 0;
        for (const auto &s : seq) stride = s.size() > stride ? (uint32_t)s.size() : stride;
        stride = (stride + 3u) & ~3u;
        const size_t n = seq.size();
        Rows r{DevBuf(ctx_, n * stride), DevBuf(ctx_, n * stride), DevBuf(ctx_, n * 4), stride};
        if (n == 0) return r;
        std::vector<uint8_t> s(n * stride, 0), q(n * stride, 0);
        std::vector<uint32_t> l(n);
        for (size_t i = 0; i < n; i++) {
            std::copy(seq[i].begin(), seq[i].end(), s.begin() + i * stride);
            std::copy(qual[i].begin(), qual[i].end(), q.begin() + i * stride);
            l[i] = (uint32_t)seq[i].size();
        }
        ctx_.check(crgpu_memcpy_h2d(ctx_.get(), r.seq.p, s.data(), s.size()));
        ctx_.check(crgpu_memcpy_h2d(ctx_.get(), r.qual.p, q.data(), q.size()));
        ctx_.check(crgpu_memcpy_h2d(ctx_.get(), r.len.p, l.data(), n * 4));
        return r;
    }
    Context &ctx_;
    int slot_;
};

/// CountMatrix: the arrays write_matrix_h5 stores (count_matrix.rs:382-448) + write_matrix_mtx.
class CountMatrix {
   public:
    CountMatrix(Context &ctx, const std::vector<FeatureBarcodeCount> &counts, uint32_t n_features) : ctx_(ctx) {
        std::vector<uint32_t> b, f, c;
        for (const auto &x : counts) {
            b.push_back(x.barcode_rank);
            f.push_back(x.feature_idx);
            c.push_back(x.umi_count);
        }
        ctx_.check(crgpu_assemble_matrix(ctx_.get(), b.data(), f.data(), c.data(), counts.size(), n_features, &m_));
    }
    ~CountMatrix() { crgpu_matrix_free(ctx_.get(), m_); }
    CountMatrix(const CountMatrix &) = delete;
    CountMatrix &operator=(const CountMatrix &) = delete;
    const crgpu_matrix &arrays() const { return *m_; }
    /// BarcodeIndex::sorted_barcodes as canonical ranks
    std::vector<uint32_t> barcode_ranks() const { return {m_->barcode_rank, m_->barcode_rank + m_->n_barcodes}; }
    void write_matrix_mtx(const std::string &mtx_path, const std::string &barcodes_tsv_path, const std::string &metadata_line,
                          uint16_t gem_group = 1) const {
        ctx_.check(crgpu_write_mtx(ctx_.get(), m_, metadata_line.c_str(), mtx_path.c_str(),
                                   barcodes_tsv_path.empty() ? nullptr : barcodes_tsv_path.c_str(), gem_group));
    }

   private:
    Context &ctx_;
    crgpu_matrix *m_ = nullptr;
};

/// filter_cellular_barcodes_ordmag (lib/python/cellranger/cell_calling_helpers.py:864-955) of one GEM group: bc_counts = the
/// UMI total of every matrix column, recovered_cells = std::nullopt to estimate it (the grid then ends at max_expected_cells).
/// Returns (top_bc_idx: the called columns, ascending; metrics: BarcodeFilterResults plus the bootstrap's per-sample values,
/// the C struct itself).  The third element of the reference's tuple, the warning for all-zero counts, is
/// `metrics.n_nonzero == 0`.
static_assert(sizeof(crgpu_ordmag_result) == 2488, "crgpu_ordmag_result changed: bump CRGPU_ABI_VERSION and every binding");
struct CellCall {
    std::vector<uint64_t> top_bc_idx;
    crgpu_ordmag_result metrics;
};
namespace detail {
inline CellCall call_cells(Context &ctx, const std::vector<uint32_t> &bc_counts, int64_t recovered_cells, int64_t max_expected_cells,
                           int64_t force_cells) {
    CellCall out{};
    void *d_counts = nullptr;
    uint64_t *d_cols = nullptr, n = 0;
    const size_t bytes = bc_counts.size() * sizeof(uint32_t);
    if (bytes) {
        ctx.check(crgpu_malloc(ctx.get(), &d_counts, bytes));
        int rc = crgpu_memcpy_h2d(ctx.get(), d_counts, bc_counts.data(), bytes);
        if (rc == CRGPU_OK)
            rc = crgpu_call_cells_ordmag_dev(ctx.get(), (const uint32_t *)d_counts, bc_counts.size(), recovered_cells, max_expected_cells,
                                             force_cells, &out.metrics, &d_cols, &n);
        if (rc == CRGPU_OK && n) {
            out.top_bc_idx.resize(n);
            rc = crgpu_memcpy_d2h(ctx.get(), out.top_bc_idx.data(), d_cols, n * sizeof(uint64_t));
        }
        crgpu_free(ctx.get(), d_counts);
        if (d_cols) crgpu_free(ctx.get(), d_cols);
        ctx.check(rc);
    }
    return out;
}
}  // namespace detail
inline CellCall filter_cellular_barcodes_ordmag(Context &ctx, const std::vector<uint32_t> &bc_counts, std::optional<int64_t> recovered_cells,
                                                int64_t max_expected_cells = 1 << 18) {
    return detail::call_cells(ctx, bc_counts, recovered_cells ? std::max<int64_t>(*recovered_cells, 1) : 0, max_expected_cells, 0);
}
/// filter_cellular_barcodes_fixed_cutoff (:958-964): the top min(cutoff, non-zero barcodes) columns
inline CellCall filter_cellular_barcodes_fixed_cutoff(Context &ctx, const std::vector<uint32_t> &bc_counts, int64_t cutoff) {
    if (cutoff <= 0) throw Error(CRGPU_EINVAL, "filter_cellular_barcodes_fixed_cutoff: cutoff must be positive");
    return detail::call_cells(ctx, bc_counts, 0, 1 << 18, cutoff);
}

/// sgt_proportions (lib/python/cellranger/sgt.py:97-132), host code: nullopt for the reference's SimpleGoodTuringError
/// (*status_out, nullable: CRGPU_SGT_TOO_FEW or CRGPU_SGT_SLOPE), else (pstar, p0).
inline std::optional<std::pair<std::vector<double>, double>> sgt_proportions(const std::vector<uint64_t> &frequencies, int *status_out = nullptr) {
    std::vector<double> pstar(frequencies.size());
    double p0 = 0.0, slope = 0.0;
    const int rc = crgpu_sgt_proportions(frequencies.data(), frequencies.size(), pstar.data(), &p0, &slope);
    if (rc < 0) throw Error(rc, crgpu_last_error(nullptr));
    if (status_out) *status_out = rc;
    if (rc != CRGPU_OK) return std::nullopt;
    return std::make_pair(std::move(pstar), p0);
}

/// find_nonambient_barcodes (lib/python/cellranger/cell_calling.py:144-263) of one genome / GEM group behind the initial call:
/// NonAmbientBarcodeResult's arrays per candidate (ascending columns), `metrics` = the C struct itself (metrics.status != 0 is
/// the reference's `return None`: no candidate rows, called == the initial cells) and `called` = the sorted union of the
/// initial cells and the non-ambient candidates.
static_assert(sizeof(crgpu_emptydrops_result) == 88, "crgpu_emptydrops_result changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_emptydrops_arrays) == 136, "crgpu_emptydrops_arrays changed: bump CRGPU_ABI_VERSION and every binding");
struct NonAmbientBarcodeResult {
    std::vector<uint64_t> eval_bcs;
    std::vector<uint32_t> umis;
    std::vector<double> log_likelihood, pvalues, pvalues_adj;
    std::vector<uint8_t> is_nonambient;
    std::vector<uint64_t> called;
    crgpu_emptydrops_result metrics;
};
namespace detail {
template <typename T>
inline int fetch(Context &ctx, std::vector<T> &out, const T *d, uint64_t n) {
    out.resize(n);
    return n ? crgpu_memcpy_d2h(ctx.get(), out.data(), d, n * sizeof(T)) : CRGPU_OK;
}
}  // namespace detail
/// raw: the device matrix; d_bc_counts: its column sums under feature_mask (crgpu_matrix_dev_column_sums); orig_cells: the
/// initially-called columns, ascending; low / high: get_empty_drops_range (cell_calling.py:122-141); feature_mask empty = all rows.
inline NonAmbientBarcodeResult find_nonambient_barcodes(Context &ctx, const crgpu_matrix_dev *raw, const uint32_t *d_bc_counts,
                                                        const std::vector<uint64_t> &orig_cells, uint64_t low, uint64_t high,
                                                        uint64_t emptydrops_minimum_umis = 500, uint32_t num_sims = 10000,
                                                        double max_adj_pvalue = 0.01, uint64_t seed = 0,
                                                        const std::vector<uint8_t> &feature_mask = {}) {
    NonAmbientBarcodeResult out{};
    crgpu_emptydrops_arrays a{};
    void *d_cells = nullptr;
    if (!orig_cells.empty()) {
        ctx.check(crgpu_malloc(ctx.get(), &d_cells, orig_cells.size() * sizeof(uint64_t)));
        const int rc = crgpu_memcpy_h2d(ctx.get(), d_cells, orig_cells.data(), orig_cells.size() * sizeof(uint64_t));
        if (rc != CRGPU_OK) {
            crgpu_free(ctx.get(), d_cells);
            ctx.check(rc);
        }
    }
    int rc = crgpu_emptydrops_dev(ctx.get(), raw, feature_mask.empty() ? nullptr : feature_mask.data(), (uint32_t)feature_mask.size(),
                                  d_bc_counts, (const uint64_t *)d_cells, orig_cells.size(), low, high, emptydrops_minimum_umis, num_sims,
                                  max_adj_pvalue, seed, nullptr, 0, nullptr, 0, &out.metrics, &a);
    if (d_cells) crgpu_free(ctx.get(), d_cells);
    ctx.check(rc);
    const uint64_t n = a.n_candidates;
    rc = detail::fetch(ctx, out.eval_bcs, a.d_eval_cols, n);
    if (rc == CRGPU_OK) rc = detail::fetch(ctx, out.umis, a.d_umis, n);
    if (rc == CRGPU_OK) rc = detail::fetch(ctx, out.log_likelihood, a.d_obs_loglk, n);
    if (rc == CRGPU_OK) rc = detail::fetch(ctx, out.pvalues, a.d_pvalues, n);
    if (rc == CRGPU_OK) rc = detail::fetch(ctx, out.pvalues_adj, a.d_pvalues_adj, n);
    if (rc == CRGPU_OK) rc = detail::fetch(ctx, out.is_nonambient, a.d_is_nonambient, n);
    if (rc == CRGPU_OK) rc = detail::fetch(ctx, out.called, a.d_called_cols, a.n_called);
    crgpu_emptydrops_arrays_free(ctx.get(), &a);
    ctx.check(rc);
    return out;
}

/// compute_ambient_pvalues (lib/python/cellranger/stats.py:205-231) + adjust_pvalue_bh (analysis/diffexp.py:88-97) against a
/// simulated table (sim_n ascending, sim_loglk = sim_n.size() rows of num_sims values): (pvalues, pvalues_adj).
inline std::pair<std::vector<double>, std::vector<double>> compute_ambient_pvalues(Context &ctx, const std::vector<uint32_t> &umis_per_bc,
                                                                                  const std::vector<double> &obs_loglk,
                                                                                  const std::vector<int64_t> &sim_n,
                                                                                  const std::vector<double> &sim_loglk) {
    const size_t n = umis_per_bc.size();
    if (obs_loglk.size() != n || sim_n.empty() || sim_loglk.size() % sim_n.size()) throw Error(CRGPU_EINVAL, "compute_ambient_pvalues: shapes");
    std::vector<double> p(n), q(n);
    if (!n) return {p, q};
    const size_t b_umis = n * sizeof(uint32_t), b_obs = n * sizeof(double), b_tab = sim_loglk.size() * sizeof(double);
    void *d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const size_t bytes[5] = {b_umis, b_obs, b_tab, b_obs, b_obs};
    int rc = CRGPU_OK;
    for (int i = 0; i < 5 && rc == CRGPU_OK; i++) rc = crgpu_malloc(ctx.get(), &d[i], bytes[i]);
    if (rc == CRGPU_OK) rc = crgpu_memcpy_h2d(ctx.get(), d[0], umis_per_bc.data(), b_umis);
    if (rc == CRGPU_OK) rc = crgpu_memcpy_h2d(ctx.get(), d[1], obs_loglk.data(), b_obs);
    if (rc == CRGPU_OK) rc = crgpu_memcpy_h2d(ctx.get(), d[2], sim_loglk.data(), b_tab);
    if (rc == CRGPU_OK)
        rc = crgpu_ambient_pvalues_dev(ctx.get(), (const uint32_t *)d[0], (const double *)d[1], n, sim_n.data(), (uint32_t)sim_n.size(),
                                       (const double *)d[2], (uint32_t)(sim_loglk.size() / sim_n.size()), 1.0, nullptr, (double *)d[3],
                                       (double *)d[4], nullptr, nullptr);
    if (rc == CRGPU_OK) rc = crgpu_memcpy_d2h(ctx.get(), p.data(), d[3], b_obs);
    if (rc == CRGPU_OK) rc = crgpu_memcpy_d2h(ctx.get(), q.data(), d[4], b_obs);
    for (void *x : d)
        if (x) crgpu_free(ctx.get(), x);
    ctx.check(rc);
    return {p, q};
}

/// SUBSAMPLE_READS (lib/python/cellranger/subsample.py).  SubsamplingDef (:161-168) of one depth: the rates per library and the
/// task type (CRGPU_SS_PER_CELL / CRGPU_SS_CELLS_ONLY / CRGPU_SS_BULK).
static_assert(sizeof(crgpu_subsample_args) == 136, "crgpu_subsample_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_subsample_result) == 56, "crgpu_subsample_result changed: bump CRGPU_ABI_VERSION and every binding");
struct SubsamplingDef {
    int64_t target_read_pairs_per_cell;
    uint8_t task_type;
    std::vector<double> library_subsample_rates;
};
/// make_subsamplings (:222-309) for the libraries `lib_indices` of one library type; subsample_type: CRGPU_SS_PLAN_*.
inline std::vector<SubsamplingDef> make_subsamplings(int subsample_type, const std::vector<uint32_t> &lib_indices,
                                                     const std::vector<double> &num_cells_per_lib, const std::vector<double> &raw_reads_per_lib,
                                                     const std::vector<double> &usable_reads_per_lib, const std::vector<int64_t> &fixed_depths,
                                                     uint32_t num_additional_depths = CRGPU_SS_NUM_ADDITIONAL_DEPTHS) {
    const uint32_t n_libs = (uint32_t)num_cells_per_lib.size();
    if (raw_reads_per_lib.size() != n_libs || usable_reads_per_lib.size() != n_libs) throw Error(CRGPU_EINVAL, "make_subsamplings: shapes");
    const uint32_t cap = (uint32_t)fixed_depths.size() + num_additional_depths + 1;
    std::vector<int64_t> depths(cap);
    std::vector<double> rates((size_t)cap * n_libs);
    uint32_t n = 0;
    const int rc = crgpu_subsample_plan(subsample_type, lib_indices.data(), (uint32_t)lib_indices.size(), n_libs, num_cells_per_lib.data(),
                                        raw_reads_per_lib.data(), usable_reads_per_lib.data(), fixed_depths.data(), (uint32_t)fixed_depths.size(),
                                        num_additional_depths, depths.data(), rates.data(), cap, &n);
    if (rc != CRGPU_OK) throw Error(rc, crgpu_last_error(nullptr));
    const uint8_t type = subsample_type == CRGPU_SS_PLAN_BULK ? CRGPU_SS_BULK : subsample_type == CRGPU_SS_PLAN_RAW_CELLS ? CRGPU_SS_CELLS_ONLY : CRGPU_SS_PER_CELL;
    std::vector<SubsamplingDef> out;
    for (uint32_t d = 0; d < n; d++) out.push_back({depths[d], type, {rates.begin() + (size_t)d * n_libs, rates.begin() + (size_t)(d + 1) * n_libs}});
    return out;
}
/// SubsampleDataDict (:406-415): [task][genome][cell], [task][genome], [task][genome][feature]; any_reads [library][genome]
struct SubsampleData {
    uint32_t n_tasks = 0, n_genomes = 0, n_libs = 0, n_features = 0;
    uint64_t n_cells = 0;
    std::vector<int64_t> umis_per_bc, read_pairs_per_bc, features_det_per_bc, read_pairs, umis, total_features_det;
    std::vector<uint8_t> any_reads;
    crgpu_subsample_result info{};
};
/// run_subsampling (:430-569) on the molecule table of `counts` (DupBuilder::build(&counts)); cell_ranks: strictly ascending
/// canonical ranks; feature_genome / cell_genome_mask / feature_mask: empty = genome 0 / cells of every genome / all features.
inline SubsampleData run_subsampling(Context &ctx, crgpu_counts *counts, const std::vector<SubsamplingDef> &tasks, uint32_t n_libs,
                                     uint32_t n_features, const std::vector<uint32_t> &cell_ranks, uint32_t n_genomes = 1,
                                     const std::vector<uint8_t> &feature_genome = {}, const std::vector<uint32_t> &cell_genome_mask = {},
                                     const std::vector<uint8_t> &feature_mask = {}, uint64_t seed = 1) {
    SubsampleData out;
    out.n_tasks = (uint32_t)tasks.size(), out.n_genomes = n_genomes, out.n_libs = n_libs, out.n_features = n_features, out.n_cells = cell_ranks.size();
    if ((!feature_genome.empty() && feature_genome.size() != n_features) || (!feature_mask.empty() && feature_mask.size() != n_features) ||
        (!cell_genome_mask.empty() && cell_genome_mask.size() != cell_ranks.size()))
        throw Error(CRGPU_EINVAL, "run_subsampling: shapes");
    std::vector<double> rates;
    std::vector<uint8_t> types;
    for (const auto &t : tasks) {
        if (t.library_subsample_rates.size() != n_libs) throw Error(CRGPU_EINVAL, "run_subsampling: a task with another number of libraries");
        rates.insert(rates.end(), t.library_subsample_rates.begin(), t.library_subsample_rates.end());
        types.push_back(t.task_type);
    }
    const size_t T = tasks.size(), G = n_genomes, NC = cell_ranks.size();
    out.umis_per_bc.assign(T * G * NC, 0), out.read_pairs_per_bc.assign(T * G * NC, 0), out.features_det_per_bc.assign(T * G * NC, 0);
    out.read_pairs.assign(T * G, 0), out.umis.assign(T * G, 0), out.total_features_det.assign(T * G * n_features, 0);
    out.any_reads.assign((size_t)n_libs * G, 0);
    void *d_cells = nullptr;
    if (NC) {
        ctx.check(crgpu_malloc(ctx.get(), &d_cells, NC * sizeof(uint32_t)));
        const int rc = crgpu_memcpy_h2d(ctx.get(), d_cells, cell_ranks.data(), NC * sizeof(uint32_t));
        if (rc != CRGPU_OK) {
            crgpu_free(ctx.get(), d_cells);
            ctx.check(rc);
        }
    }
    crgpu_subsample_args a{};
    a.n_tasks = out.n_tasks, a.n_genomes = n_genomes, a.n_libs = n_libs, a.n_features = n_features, a.n_cells = NC, a.seed = seed;
    a.rates = rates.data(), a.task_type = types.data(), a.d_cell_ranks = (const uint32_t *)d_cells;
    a.cell_genome_mask = cell_genome_mask.empty() ? nullptr : cell_genome_mask.data();
    a.feature_genome = feature_genome.empty() ? nullptr : feature_genome.data();
    a.feature_mask = feature_mask.empty() ? nullptr : feature_mask.data();
    a.umis_per_bc = out.umis_per_bc.data(), a.read_pairs_per_bc = out.read_pairs_per_bc.data(), a.features_det_per_bc = out.features_det_per_bc.data();
    a.read_pairs = out.read_pairs.data(), a.umis = out.umis.data(), a.total_features_det = out.total_features_det.data();
    a.any_reads = out.any_reads.data();
    const int rc = crgpu_subsample_dev(ctx.get(), counts, &a, &out.info);
    if (d_cells) crgpu_free(ctx.get(), d_cells);
    ctx.check(rc);
    return out;
}
/// the per-task, per-genome numbers of calculate_subsampling_metrics (:719-845): [task][genome][CRGPU_SS_SUMMARY_COLS] and the
/// whole-dataset duplication fraction per task
inline std::pair<std::vector<double>, std::vector<double>> subsampling_summary(const SubsampleData &d, const std::vector<SubsamplingDef> &tasks,
                                                                              const std::vector<uint32_t> &cell_genome_mask = {}) {
    std::vector<uint8_t> types;
    for (const auto &t : tasks) types.push_back(t.task_type);
    if (types.size() != d.n_tasks) throw Error(CRGPU_EINVAL, "subsampling_summary: shapes");
    std::vector<double> out((size_t)d.n_tasks * d.n_genomes * CRGPU_SS_SUMMARY_COLS), all(d.n_tasks);
    const int rc = crgpu_subsample_summary(d.n_tasks, d.n_genomes, d.n_cells, d.n_features, types.data(),
                                           cell_genome_mask.empty() ? nullptr : cell_genome_mask.data(), d.umis_per_bc.data(),
                                           d.read_pairs_per_bc.data(), d.features_det_per_bc.data(), d.read_pairs.data(), d.umis.data(),
                                           d.total_features_det.data(), out.data(), all.data());
    if (rc != CRGPU_OK) throw Error(rc, crgpu_last_error(nullptr));
    return {out, all};
}

/// NORMALIZE_DEPTH of aggr (mro/rna/stages/aggregator/normalize_depth/__init__.py) for one GEM well; the draw is the Philox
/// stream of run_subsampling (crgpu.h), not the reference's serial np.random.binomial.
static_assert(sizeof(crgpu_normalize_depth_args) == 120, "crgpu_normalize_depth_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_normalize_depth_result) == 64, "crgpu_normalize_depth_result changed: bump CRGPU_ABI_VERSION and every binding");
/// frac_reads_kept of split() (:139-176): library_type = a small integer id per library; is_targeted_lib empty = none.
inline std::vector<double> normalize_depth_plan(const std::vector<uint32_t> &library_type, const std::vector<double> &usable_reads,
                                                const std::vector<double> &num_cells, bool downsample = true, bool targeted_aggr = false,
                                                const std::vector<uint8_t> &is_targeted_lib = {}, double targeted_depth_factor = 1.0) {
    const size_t n = library_type.size();
    if (usable_reads.size() != n || num_cells.size() != n || (!is_targeted_lib.empty() && is_targeted_lib.size() != n))
        throw Error(CRGPU_EINVAL, "normalize_depth_plan: shapes");
    std::vector<double> frac(n);
    const int rc = crgpu_normalize_depth_plan((uint32_t)n, library_type.data(), usable_reads.data(), num_cells.data(), downsample, targeted_aggr,
                                              is_targeted_lib.empty() ? nullptr : is_targeted_lib.data(), targeted_depth_factor, frac.data());
    if (rc != CRGPU_OK) throw Error(rc, crgpu_last_error(nullptr));
    return frac;
}
/// a device-resident CSC (crgpu_matrix_dev), released with its owner
class MatrixDev {
   public:
    MatrixDev(Context &ctx, crgpu_matrix_dev *m) : ctx_(&ctx), m_(m) {}
    ~MatrixDev() {
        if (m_) crgpu_matrix_dev_free(ctx_->get(), m_);
    }
    MatrixDev(MatrixDev &&o) noexcept : ctx_(o.ctx_), m_(o.m_) { o.m_ = nullptr; }
    MatrixDev(const MatrixDev &) = delete;
    MatrixDev &operator=(const MatrixDev &) = delete;
    const crgpu_matrix_dev *get() const { return m_; }
    uint64_t n_barcodes() const { return m_->n_barcodes; }
    uint64_t nnz() const { return m_->nnz; }
    struct Host {
        std::vector<uint32_t> barcode_rank;
        std::vector<int64_t> indptr;
        std::vector<int32_t> indices, data;
    };
    Host download() const {
        Host h;
        h.barcode_rank.resize(m_->n_barcodes), h.indptr.resize(m_->n_barcodes + 1), h.indices.resize(m_->nnz), h.data.resize(m_->nnz);
        ctx_->check(crgpu_matrix_dev_download(ctx_->get(), m_, h.barcode_rank.data(), h.indptr.data(), h.indices.data(), h.data.data()));
        return h;
    }

   private:
    Context *ctx_;
    crgpu_matrix_dev *m_;
};
/// what main() (:481-532) computes: the raw UMI matrix after the draw, summarize_read_matrix's sums per class, the per-library sums
struct NormalizedDepth {
    MatrixDev matrix;
    std::vector<int64_t> raw_mapped_reads, flt_mapped_reads;                          // [class]
    std::vector<int64_t> reads_per_lib, kept_reads_per_lib, kept_molecules_per_lib;   // [library]
    std::vector<uint32_t> kept;                                                       // per molecule in table order (want_kept)
    crgpu_normalize_depth_result info{};
};
/// `counts` = DupBuilder::build(&counts) of the well; cell_ranks: strictly ascending canonical ranks; feature_class empty = one
/// class; cell_class_mask empty = every cell is a cell of every class.
inline NormalizedDepth normalize_depth(Context &ctx, crgpu_counts *counts, const std::vector<double> &frac_reads_kept, uint32_t n_features,
                                       const std::vector<uint32_t> &cell_ranks = {}, const std::vector<uint8_t> &feature_class = {},
                                       uint32_t n_classes = 1, const std::vector<uint32_t> &cell_class_mask = {}, uint64_t seed = 0,
                                       bool want_kept = false) {
    if ((!feature_class.empty() && feature_class.size() != n_features) || (!cell_class_mask.empty() && cell_class_mask.size() != cell_ranks.size()))
        throw Error(CRGPU_EINVAL, "normalize_depth: shapes");
    const size_t NL = frac_reads_kept.size(), NC = cell_ranks.size();
    crgpu_matrix_dev *mv = nullptr;
    std::vector<int64_t> raw(n_classes, 0), flt(n_classes, 0), reads(NL, 0), kept_reads(NL, 0), kept_mols(NL, 0);
    std::vector<uint32_t> kept;
    if (want_kept && counts) {
        uint64_t nm = 0;
        ctx.check(crgpu_counts_info(ctx.get(), counts, nullptr, &nm));
        kept.assign(nm, 0);
    }
    void *d_cells = nullptr;
    if (NC) {
        ctx.check(crgpu_malloc(ctx.get(), &d_cells, NC * sizeof(uint32_t)));
        const int rc = crgpu_memcpy_h2d(ctx.get(), d_cells, cell_ranks.data(), NC * sizeof(uint32_t));
        if (rc != CRGPU_OK) {
            crgpu_free(ctx.get(), d_cells);
            ctx.check(rc);
        }
    }
    crgpu_normalize_depth_args a{};
    a.n_libs = (uint32_t)NL, a.n_features = n_features, a.n_classes = n_classes, a.n_cells = NC, a.seed = seed;
    a.frac_reads_kept = frac_reads_kept.data(), a.d_cell_ranks = (const uint32_t *)d_cells;
    a.feature_class = feature_class.empty() ? nullptr : feature_class.data();
    a.cell_class_mask = cell_class_mask.empty() ? nullptr : cell_class_mask.data();
    a.matrix = &mv;
    a.raw_mapped_reads = raw.data(), a.flt_mapped_reads = flt.data(), a.reads_per_lib = reads.data();
    a.kept_reads_per_lib = kept_reads.data(), a.kept_molecules_per_lib = kept_mols.data();
    a.kept_out = kept.empty() ? nullptr : kept.data();
    crgpu_normalize_depth_result info{};
    const int rc = crgpu_normalize_depth_dev(ctx.get(), counts, &a, &info);
    if (d_cells) crgpu_free(ctx.get(), d_cells);
    ctx.check(rc);
    return NormalizedDepth{MatrixDev(ctx, mv), raw, flt, reads, kept_reads, kept_mols, kept, info};
}
/// CountMatrix.select_features (lib/python/cellranger/matrix.py:886-894) for the ascending indices whose mask byte is non-zero
inline MatrixDev select_features(Context &ctx, const MatrixDev &m, const std::vector<uint8_t> &feature_mask) {
    crgpu_matrix_dev *out = nullptr;
    ctx.check(crgpu_select_features_dev(ctx.get(), m.get(), feature_mask.data(), (uint32_t)feature_mask.size(), &out));
    return MatrixDev(ctx, out);
}

/// MultiGenomeAnalysis.run_all (lib/python/cellranger/analysis/multigenome.py:251-335) behind the filtered matrix: classify_gems,
/// the multiplet bootstrap (np.random.seed(0) / np.random.choice, reproduced on the device) and the mean count purities.  The
/// purity-outlier diagnostics (scipy's beta.fit) are not covered (crgpu.h).
static_assert(sizeof(crgpu_multigenome_result) == 184, "crgpu_multigenome_result changed: bump CRGPU_ABI_VERSION and every binding");
struct MultigenomeAnalysis {
    std::vector<uint8_t> call;                 // per barcode: 0 genome0, 1 genome1, 2 Multiplet
    std::vector<int64_t> boot_counts;          // [3 * bootstraps]: (Multiplets, genome0, genome1) per sample
    std::vector<double> boot_thresholds;       // [2 * bootstraps]
    std::vector<int32_t> boot_branch;          // [bootstraps]: CRGPU_MG_BRANCH_*
    std::vector<double> boot;                  // [bootstraps]: inferred multiplets per sample
    crgpu_multigenome_result result{};         // the C struct itself
};
/// counts0 / counts1: the UMI totals of the filtered barcodes over the features of the two top genomes
inline MultigenomeAnalysis multigenome_analysis(Context &ctx, const std::vector<uint32_t> &counts0, const std::vector<uint32_t> &counts1,
                                                uint32_t bootstraps = 1000) {
    if (counts0.size() != counts1.size()) throw Error(CRGPU_EINVAL, "multigenome_analysis: shapes");
    const size_t n = counts0.size(), bytes = n * sizeof(uint32_t);
    MultigenomeAnalysis out;
    out.call.assign(n, 0), out.boot_counts.assign((size_t)3 * bootstraps, 0), out.boot_thresholds.assign((size_t)2 * bootstraps, 0.0);
    out.boot_branch.assign(bootstraps, 0), out.boot.assign(bootstraps, 0.0);
    void *d0 = nullptr, *d1 = nullptr, *dc = nullptr;
    int rc = CRGPU_OK;
    if (n) {
        rc = crgpu_malloc(ctx.get(), &d0, bytes);
        if (rc == CRGPU_OK) rc = crgpu_malloc(ctx.get(), &d1, bytes);
        if (rc == CRGPU_OK) rc = crgpu_malloc(ctx.get(), &dc, n);
        if (rc == CRGPU_OK) rc = crgpu_memcpy_h2d(ctx.get(), d0, counts0.data(), bytes);
        if (rc == CRGPU_OK) rc = crgpu_memcpy_h2d(ctx.get(), d1, counts1.data(), bytes);
    }
    if (rc == CRGPU_OK)
        rc = crgpu_multigenome_dev(ctx.get(), (const uint32_t *)d0, (const uint32_t *)d1, n, bootstraps, (uint8_t *)dc, out.boot_counts.data(),
                                   out.boot_thresholds.data(), out.boot_branch.data(), &out.result);
    if (rc == CRGPU_OK && n) rc = crgpu_memcpy_d2h(ctx.get(), out.call.data(), dc, n);
    for (void *p : {d0, d1, dc})
        if (p) crgpu_free(ctx.get(), p);
    ctx.check(rc);
    if (n) {
        crgpu_multigenome_result again = out.result;  // the per-sample values come from the summary (host code, no context)
        if (crgpu_multigenome_summary(out.boot_counts.data(), bootstraps, n, out.boot.data(), &again) != CRGPU_OK)
            throw Error(CRGPU_EINVAL, crgpu_last_error(nullptr));
    }
    return out;
}
/// sorted(np.argsort(totals)[::-1][:2]) of :260: among equal totals the larger index first
inline std::vector<uint32_t> multigenome_top_two(const std::vector<uint64_t> &totals) {
    std::vector<uint32_t> idx(totals.size());
    for (uint32_t i = 0; i < idx.size(); i++) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return totals[a] < totals[b]; });
    std::vector<uint32_t> top(idx.rbegin(), idx.rbegin() + std::min<size_t>(2, idx.size()));
    std::sort(top.begin(), top.end());
    return top;
}

/// CALL_TAGS_RTL (lib/rust/cr_lib/src/stages/call_tags_rtl.rs:143-498, barcode_overlap.rs, read_level_multiplexing.rs:22-68) and
/// remove_bcs_from_high_occupancy_gems (lib/python/cellranger/cell_calling_helpers.py:315-424) on the raw device matrix of a
/// multiplexed Flex well.  Tags index the caller's probe-barcode identifiers in ascending order.
static_assert(sizeof(crgpu_rtl_gem_runs) == 40040, "crgpu_rtl_gem_runs changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_rtl_overlap_row) == 40, "crgpu_rtl_overlap_row changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_rtl_high_occupancy) == 64, "crgpu_rtl_high_occupancy changed: bump CRGPU_ABI_VERSION and every binding");
namespace detail {
struct DeviceCols {  // an ascending column list on the device for the length of a call
    Context &ctx;
    void *d = nullptr;
    DeviceCols(Context &c, const std::vector<uint64_t> &cols) : ctx(c) {
        if (cols.empty()) return;
        ctx.check(crgpu_malloc(ctx.get(), &d, cols.size() * sizeof(uint64_t)));
        const int rc = crgpu_memcpy_h2d(ctx.get(), d, cols.data(), cols.size() * sizeof(uint64_t));
        if (rc != CRGPU_OK) {
            crgpu_free(ctx.get(), d);
            d = nullptr;
            ctx.check(rc);
        }
    }
    ~DeviceCols() {
        if (d) crgpu_free(ctx.get(), d);
    }
    DeviceCols(const DeviceCols &) = delete;
    const uint64_t *get() const { return (const uint64_t *)d; }
};
}  // namespace detail
struct RtlTags {
    std::vector<uint8_t> tags;                 // per column of the raw matrix
    std::vector<uint64_t> barcodes_per_tag;    // [n_tags]
    std::vector<uint64_t> umi_per_tag;         // [n_types * n_tags]
};
/// get_barcodes_per_multiplexing_identifier / get_umi_per_multiplexing_identifier; tag_of_probe[p] = 0xFF: not on the map
inline RtlTags rtl_tags(Context &ctx, const crgpu_matrix_dev *raw, const std::vector<uint8_t> &tag_of_probe, uint32_t n_tags,
                        const std::vector<uint8_t> &feature_type = {}, uint32_t n_types = 0) {
    RtlTags out;
    out.tags.assign(raw->n_barcodes, 0), out.barcodes_per_tag.assign(n_tags, 0), out.umi_per_tag.assign((size_t)n_types * n_tags, 0);
    void *d_tags = nullptr;
    ctx.check(crgpu_malloc(ctx.get(), &d_tags, raw->n_barcodes ? raw->n_barcodes : 1));
    int rc = crgpu_rtl_tags_dev(ctx.get(), raw, tag_of_probe.data(), n_tags, feature_type.empty() ? nullptr : feature_type.data(),
                                (uint32_t)feature_type.size(), n_types, (uint8_t *)d_tags, out.barcodes_per_tag.data(),
                                n_types ? out.umi_per_tag.data() : nullptr);
    if (rc == CRGPU_OK && raw->n_barcodes) rc = crgpu_memcpy_d2h(ctx.get(), out.tags.data(), d_tags, raw->n_barcodes);
    crgpu_free(ctx.get(), d_tags);
    ctx.check(rc);
    return out;
}
namespace detail {
template <typename T>
struct DeviceCopy {  // a host vector on the device for the length of a call (one byte when the vector is empty)
    Context &ctx;
    void *d = nullptr;
    DeviceCopy(Context &c, const std::vector<T> &h) : ctx(c) {
        ctx.check(crgpu_malloc(ctx.get(), &d, h.empty() ? 1 : h.size() * sizeof(T)));
        const int rc = h.empty() ? CRGPU_OK : crgpu_memcpy_h2d(ctx.get(), d, h.data(), h.size() * sizeof(T));
        if (rc != CRGPU_OK) {
            crgpu_free(ctx.get(), d);
            d = nullptr;
            ctx.check(rc);
        }
    }
    ~DeviceCopy() {
        if (d) crgpu_free(ctx.get(), d);
    }
    DeviceCopy(const DeviceCopy &) = delete;
    const T *get() const { return (const T *)d; }
};
}  // namespace detail
/// the antibody part of detect_suspicious_rtl_ab_pairings: the reverse-translated tag of every probe rank, the Antibody sum of
/// every raw column (crgpu_matrix_dev_column_sums under the Antibody mask) and the thresholds of rtl_ab_thresholds
struct RtlAntibody {
    std::vector<uint8_t> ab_tag_of_probe;
    std::vector<uint32_t> ab_sums;
    std::vector<uint64_t> ab_min_count;   // UINT64_MAX: the tag is removed
};
/// ProbeBarcodeGelBeadGrouper::group_all + calculate_barcode_overlap_counts of the filtered barcodes `cells` (ascending columns of
/// the raw matrix), and the GEM occupancy of the same pass; with `ab` the combined map of detect_suspicious_rtl_ab_pairings
inline crgpu_rtl_gem_runs rtl_gem_runs(Context &ctx, const crgpu_matrix_dev *raw, const std::vector<uint8_t> &tags, uint32_t n_tags,
                                       const std::vector<uint64_t> &cells, const RtlAntibody *ab = nullptr) {
    crgpu_rtl_gem_runs res{};
    if (tags.size() != raw->n_barcodes || (ab && (ab->ab_sums.size() != raw->n_barcodes || ab->ab_min_count.size() != n_tags)))
        throw Error(CRGPU_EINVAL, "rtl_gem_runs: shapes");
    detail::DeviceCols d_cells(ctx, cells);
    detail::DeviceCopy<uint8_t> d_tags(ctx, tags);
    if (ab) {
        detail::DeviceCopy<uint32_t> d_sums(ctx, ab->ab_sums);
        ctx.check(crgpu_rtl_gem_runs_dev(ctx.get(), raw, d_tags.get(), n_tags, d_cells.get(), cells.size(), ab->ab_tag_of_probe.data(),
                                         d_sums.get(), ab->ab_min_count.data(), &res));
    } else {
        ctx.check(crgpu_rtl_gem_runs_dev(ctx.get(), raw, d_tags.get(), n_tags, d_cells.get(), cells.size(), nullptr, nullptr, nullptr, &res));
    }
    return res;
}
/// sample_barcodes (cells == nullptr: all columns) / sample_cell_barcodes (the called columns, ascending): per sample its columns,
/// ascending -- with crgpu_cell_ranks_dev what crgpu_assemble_probe_matrix_dev takes as d_sample_ranks.  sample_of_tag[t] = 0xFF:
/// the tag belongs to no sample
inline std::vector<std::vector<uint64_t>> rtl_sample_columns(Context &ctx, const crgpu_matrix_dev *raw, const std::vector<uint8_t> &tags,
                                                             const std::vector<uint8_t> &sample_of_tag, uint32_t n_samples,
                                                             const std::vector<uint64_t> *cells = nullptr) {
    if (tags.size() != raw->n_barcodes) throw Error(CRGPU_EINVAL, "rtl_sample_columns: one tag per column");
    detail::DeviceCopy<uint8_t> d_tags(ctx, tags);
    detail::DeviceCols d_cells(ctx, cells ? *cells : std::vector<uint64_t>{});
    std::vector<uint64_t> off(n_samples + 1, 0), all;
    uint64_t *d_out = nullptr;
    ctx.check(crgpu_rtl_sample_columns_dev(ctx.get(), d_tags.get(), raw->n_barcodes, sample_of_tag.data(), (uint32_t)sample_of_tag.size(),
                                           n_samples, cells != nullptr, d_cells.get(), cells ? cells->size() : 0, &d_out, off.data()));
    const int rc = detail::fetch(ctx, all, (const uint64_t *)d_out, off[n_samples]);
    if (d_out) crgpu_free(ctx.get(), d_out);
    ctx.check(rc);
    std::vector<std::vector<uint64_t>> out(n_samples);
    for (uint32_t s = 0; s < n_samples; s++) out[s].assign(all.begin() + off[s], all.begin() + off[s + 1]);
    return out;
}
struct RtlMedians {
    std::vector<uint64_t> n_nonzero, median;   // per probe rank
};
/// get_median_umi_per_cell for one feature type: sums = the column sums of the raw matrix under that type's mask
inline RtlMedians rtl_medians(Context &ctx, const crgpu_matrix_dev *raw, const std::vector<uint32_t> &sums, const std::vector<uint64_t> &cells,
                              uint32_t n_probe) {
    if (sums.size() != raw->n_barcodes || n_probe > CRGPU_RTL_MAX_PROBES) throw Error(CRGPU_EINVAL, "rtl_medians: shapes");
    detail::DeviceCopy<uint32_t> d_sums(ctx, sums);
    detail::DeviceCols d_cells(ctx, cells);
    RtlMedians out;
    out.n_nonzero.assign(CRGPU_RTL_MAX_PROBES, 0), out.median.assign(CRGPU_RTL_MAX_PROBES, 0);
    ctx.check(crgpu_rtl_medians_dev(ctx.get(), raw, d_sums.get(), d_cells.get(), cells.size(), out.n_nonzero.data(), out.median.data()));
    out.n_nonzero.resize(n_probe), out.median.resize(n_probe);
    return out;
}
/// the Antibody thresholds of detect_suspicious_rtl_ab_pairings: round(0.1 * median), UINT64_MAX = removed
inline std::vector<uint64_t> rtl_ab_thresholds(const RtlMedians &med, const std::vector<uint8_t> &ab_tag_of_probe,
                                               const std::vector<uint8_t> &tag_kind) {
    if (med.median.size() != ab_tag_of_probe.size() || med.n_nonzero.size() != ab_tag_of_probe.size()) throw Error(CRGPU_EINVAL, "rtl_ab_thresholds: shapes");
    std::vector<uint64_t> out(tag_kind.size());
    const int rc = crgpu_rtl_ab_thresholds(med.median.data(), med.n_nonzero.data(), ab_tag_of_probe.data(), (uint32_t)ab_tag_of_probe.size(),
                                           tag_kind.data(), (uint32_t)tag_kind.size(), out.data());
    if (rc != CRGPU_OK) throw Error(rc, crgpu_last_error(nullptr));
    return out;
}
/// the tail of detect_suspicious_rtl_ab_pairings: RTL + Antibody rows that are no configured pairing, RTL first, sorted
inline std::vector<crgpu_rtl_overlap_row> rtl_suspicious_pairings(const std::vector<crgpu_rtl_overlap_row> &rows, const std::vector<uint8_t> &tag_kind,
                                                                  const std::vector<int32_t> &paired_with) {
    if (paired_with.size() != tag_kind.size()) throw Error(CRGPU_EINVAL, "rtl_suspicious_pairings: shapes");
    std::vector<crgpu_rtl_overlap_row> out(rows.size() ? rows.size() : 1);
    uint32_t n = 0;
    const int rc = crgpu_rtl_suspicious_pairings(rows.data(), (uint32_t)rows.size(), tag_kind.data(), paired_with.data(), (uint32_t)tag_kind.size(),
                                                 out.data(), &n);
    if (rc != CRGPU_OK) throw Error(rc, crgpu_last_error(nullptr));
    out.resize(n);
    return out;
}
struct RtlOccupancy {
    uint64_t zero_bin = 0;               // GEMs without a cell: max(0, int(partitions * recovery_factor - gems_with_cells))
    double estimated_lambda = 0.0;
    uint32_t total_probe_barcodes = 0;
};
/// the head of remove_bcs_from_high_occupancy_gems from the occupancy outputs of rtl_gem_runs
inline RtlOccupancy rtl_occupancy_summary(const crgpu_rtl_gem_runs &r, int64_t total_instrument_partitions = 115000,
                                          double recovery_factor = 1 / 1.65) {
    RtlOccupancy out;
    const int rc = crgpu_rtl_occupancy_summary(r.cells_per_gem_hist, r.n_probe, r.gems_with_cells, r.cells_per_probe, total_instrument_partitions,
                                               recovery_factor, &out.zero_bin, &out.estimated_lambda, &out.total_probe_barcodes);
    if (rc != CRGPU_OK) throw Error(rc, crgpu_last_error(nullptr));
    return out;
}
/// calculate_frp_gem_barcode_overlap: one row per pair of present tags
inline std::vector<crgpu_rtl_overlap_row> rtl_overlap_rows(const crgpu_rtl_gem_runs &r) {
    uint32_t n = 0;
    if (crgpu_rtl_overlap_rows(r.gems_per_tag, r.common, r.present, r.n_tags, nullptr, 0, &n) != CRGPU_OK)
        throw Error(CRGPU_EINVAL, crgpu_last_error(nullptr));
    std::vector<crgpu_rtl_overlap_row> rows(n);
    if (n && crgpu_rtl_overlap_rows(r.gems_per_tag, r.common, r.present, r.n_tags, rows.data(), n, &n) != CRGPU_OK)
        throw Error(CRGPU_EINVAL, crgpu_last_error(nullptr));
    return rows;
}
struct HighOccupancyRemoval {
    std::vector<uint64_t> kept;           // the kept cell columns, ascending
    crgpu_rtl_high_occupancy summary{};
};
/// remove_bcs_from_high_occupancy_gems behind its threshold (the host's: _get_high_occupancy_gem_threshold needs numpy's stream)
inline HighOccupancyRemoval remove_high_occupancy_gems(Context &ctx, const crgpu_matrix_dev *raw, const std::vector<uint64_t> &cells,
                                                       uint32_t threshold) {
    HighOccupancyRemoval out;
    detail::DeviceCols d_cells(ctx, cells);
    uint64_t *d_kept = nullptr;
    ctx.check(crgpu_rtl_remove_high_occupancy_dev(ctx.get(), raw, d_cells.get(), cells.size(), threshold, &d_kept, &out.summary));
    const int rc = detail::fetch(ctx, out.kept, (const uint64_t *)d_kept, out.summary.n_kept);
    crgpu_free(ctx.get(), d_kept);
    ctx.check(rc);
    return out;
}

// ---- the summary metrics of the filtered matrix (report_matrix.py: _report / _report_genome_agnostic_metrics) ------------------------
static_assert(sizeof(crgpu_matrix_summary_class) == 296, "crgpu_matrix_summary_class changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_matrix_summary_floats) == 120, "crgpu_matrix_summary_floats changed: bump CRGPU_ABI_VERSION and every binding");
struct MatrixSummary {
    std::vector<uint64_t> counts_per_feature, cells_ge2_per_feature;  // [n_features], over the cells of the feature's own class
    std::vector<crgpu_matrix_summary_class> classes;                  // [n_classes]
    uint64_t reads_all = 0, reads_union = 0;                          // 0 without a read table
    std::vector<uint32_t> counts_per_cell, genes_per_cell;            // [n_classes * n_cells] when asked for
};
/// the counted reads (VALID + CORRECTED) of every column, the libraries of lib_mask added up
inline std::vector<uint32_t> reads_per_column(Context &ctx, const crgpu_matrix_dev *raw, uint32_t lib_mask = 1u) {
    std::vector<uint32_t> out(raw->n_barcodes);
    void *d = nullptr;
    ctx.check(crgpu_malloc(ctx.get(), &d, out.empty() ? 1 : out.size() * sizeof(uint32_t)));
    int rc = crgpu_matrix_dev_reads_per_column(ctx.get(), raw, lib_mask, (uint32_t *)d);
    if (rc == CRGPU_OK && !out.empty()) rc = crgpu_memcpy_d2h(ctx.get(), out.data(), d, out.size() * sizeof(uint32_t));
    crgpu_free(ctx.get(), d);
    ctx.check(rc);
    return out;
}
/// crgpu_matrix_summary_dev on the raw matrix: cells = the ascending called columns; feature_class empty = every feature in class 0
/// (n_features then counts); cell_class_mask empty = a cell of every class; reads empty = no read table
inline MatrixSummary matrix_summary(Context &ctx, const crgpu_matrix_dev *raw, const std::vector<uint64_t> &cells, uint32_t n_features,
                                    const std::vector<uint8_t> &feature_class = {}, uint32_t n_classes = 1,
                                    const std::vector<uint32_t> &cell_class_mask = {}, const std::vector<uint32_t> &reads = {},
                                    bool per_cell = false) {
    if ((!feature_class.empty() && feature_class.size() != n_features) || (!cell_class_mask.empty() && cell_class_mask.size() != cells.size()) ||
        (!reads.empty() && reads.size() != raw->n_barcodes) || n_classes < 1 || n_classes > CRGPU_MS_MAX_CLASSES)
        throw Error(CRGPU_EINVAL, "matrix_summary: shapes");
    MatrixSummary out;
    out.counts_per_feature.assign(n_features, 0), out.cells_ge2_per_feature.assign(n_features, 0);
    out.classes.resize(n_classes);
    detail::DeviceCols d_cells(ctx, cells);
    detail::DeviceCopy<uint32_t> d_reads(ctx, reads);
    const size_t n_pc = per_cell ? (size_t)n_classes * cells.size() : 0;
    detail::DeviceCopy<uint32_t> d_cpc(ctx, std::vector<uint32_t>(n_pc, 0)), d_gpc(ctx, std::vector<uint32_t>(n_pc, 0));
    ctx.check(crgpu_matrix_summary_dev(ctx.get(), raw, n_features, n_classes, feature_class.empty() ? nullptr : feature_class.data(), d_cells.get(),
                                       cells.size(), cell_class_mask.empty() ? nullptr : cell_class_mask.data(), reads.empty() ? nullptr : d_reads.get(),
                                       out.counts_per_feature.data(), out.cells_ge2_per_feature.data(), out.classes.data(), &out.reads_all,
                                       &out.reads_union, per_cell ? (uint32_t *)d_cpc.d : nullptr, per_cell ? (uint32_t *)d_gpc.d : nullptr));
    if (n_pc) {
        ctx.check(detail::fetch(ctx, out.counts_per_cell, d_cpc.get(), n_pc));
        ctx.check(detail::fetch(ctx, out.genes_per_cell, d_gpc.get(), n_pc));
    }
    return out;
}
/// the floats of _report from the integers of one class; reads_cells / reads_all: the class's own and the well's by default
inline crgpu_matrix_summary_floats matrix_summary_stats(const crgpu_matrix_summary_class &c, uint64_t reads_cells, uint64_t reads_all) {
    crgpu_matrix_summary_floats out;
    const int rc = crgpu_matrix_summary_stats(&c, reads_cells, reads_all, &out);
    if (rc != CRGPU_OK) throw Error(rc, crgpu_last_error(nullptr));
    return out;
}
inline crgpu_matrix_summary_floats matrix_summary_stats(const MatrixSummary &s, uint32_t k) {
    return matrix_summary_stats(s.classes.at(k), s.classes.at(k).reads_cells, s.reads_all);
}

// ---- a targeted well (CALCULATE_TARGETED_METRICS): tallies, reads-per-UMI statistics, the enrichment call --------------------------------
static_assert(sizeof(crgpu_rpu_stats) == 256, "crgpu_rpu_stats changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_rpu_gmm_args) == 32, "crgpu_rpu_gmm_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_rpu_gmm_result) == 120, "crgpu_rpu_gmm_result changed: bump CRGPU_ABI_VERSION and every binding");
struct FeatureMetrics {  // pandas_utils.collapse_feature_counts: per feature
    std::vector<uint64_t> num_umis, num_reads, num_umis_cells, num_reads_cells;
};
/// crgpu_feature_metrics_dev on `counts` (DupBuilder::build(&counts)): lib_mask = filter_library_idx as bits; cell_ranks: strictly
/// ascending canonical ranks, the union of the pass-filter barcodes of those libraries
inline FeatureMetrics feature_metrics(Context &ctx, crgpu_counts *counts, uint32_t n_features, const std::vector<uint32_t> &cell_ranks = {},
                                      uint32_t lib_mask = 1u) {
    FeatureMetrics out;
    out.num_umis.assign(n_features, 0), out.num_reads.assign(n_features, 0), out.num_umis_cells.assign(n_features, 0), out.num_reads_cells.assign(n_features, 0);
    detail::DeviceCopy<uint32_t> d_cells(ctx, cell_ranks);
    ctx.check(crgpu_feature_metrics_dev(ctx.get(), counts, n_features, lib_mask, cell_ranks.empty() ? nullptr : d_cells.get(), cell_ranks.size(),
                                        out.num_umis.data(), out.num_reads.data(), out.num_umis_cells.data(), out.num_reads_cells.data()));
    return out;
}
struct TargetedRpuStats {
    crgpu_rpu_stats stats;
    std::vector<uint32_t> q_feature;  // the quantifiable features, ascending ...
    std::vector<double> q_value;      // ... log10(num_reads_cells / num_umis_cells) ...
    std::vector<uint8_t> q_label;     // ... 1 = targeted: the input of rpu_gmm
};
/// crgpu_targeted_rpu_stats (host): is_gex empty = every feature is Gene Expression
inline TargetedRpuStats targeted_rpu_stats(const FeatureMetrics &t, const std::vector<uint8_t> &is_targeted, const std::vector<uint8_t> &is_gex = {}) {
    const size_t F = t.num_umis.size();
    if (t.num_reads.size() != F || t.num_umis_cells.size() != F || t.num_reads_cells.size() != F || is_targeted.size() != F || (!is_gex.empty() && is_gex.size() != F))
        throw Error(CRGPU_EINVAL, "targeted_rpu_stats: shapes");
    TargetedRpuStats out;
    out.q_feature.resize(F), out.q_value.resize(F), out.q_label.resize(F);
    const int rc = crgpu_targeted_rpu_stats((uint32_t)F, t.num_umis.data(), t.num_reads.data(), t.num_umis_cells.data(), t.num_reads_cells.data(), is_targeted.data(),
                                            is_gex.empty() ? nullptr : is_gex.data(), &out.stats, out.q_feature.data(), out.q_value.data(), out.q_label.data());
    if (rc != CRGPU_OK) throw Error(rc, crgpu_last_error(nullptr));
    const size_t nq = out.stats.n_quantifiable_total;
    out.q_feature.resize(nq), out.q_value.resize(nq), out.q_label.resize(nq);
    return out;
}
struct RpuGmm {
    crgpu_rpu_gmm_result result;       // sd_high / sd_low: the tied PRECISION, as the reference reports it (gmm.py:86-90)
    std::vector<uint8_t> enriched;     // per gene: value >= log_rpu_threshold
    std::vector<double> start_lk;      // [CRGPU_GMM_STARTS] when asked for
    std::vector<uint32_t> start_iters;
};
/// crgpu_rpu_gmm_dev: fit_enrichments(labels, values, method = BOTH_TIED)
inline RpuGmm rpu_gmm(Context &ctx, const std::vector<double> &values, const std::vector<uint8_t> &labels, bool want_starts = false) {
    if (values.size() != labels.size() || values.size() > 0xFFFFFFFFull) throw Error(CRGPU_EINVAL, "rpu_gmm: one label per value");
    RpuGmm out;
    out.enriched.assign(values.size(), 0);
    if (want_starts) out.start_lk.assign(CRGPU_GMM_STARTS, 0.0), out.start_iters.assign(CRGPU_GMM_STARTS, 0);
    crgpu_rpu_gmm_args a{want_starts ? out.start_lk.data() : nullptr, want_starts ? out.start_iters.data() : nullptr,
                         values.empty() ? nullptr : out.enriched.data(), 0};
    ctx.check(crgpu_rpu_gmm_dev(ctx.get(), values.empty() ? nullptr : values.data(), labels.empty() ? nullptr : labels.data(), (uint32_t)values.size(), &a,
                                &out.result));
    return out;
}

// ---- a cell-multiplexed (CMO) well: the JIBES tag caller (CALL_TAGS_JIBES) ---------------------------------------------------------------
static_assert(sizeof(crgpu_jibes_setup) == 24, "crgpu_jibes_setup changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_jibes_fit_args) == 136, "crgpu_jibes_fit_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_jibes_fit_result) == 416, "crgpu_jibes_fit_result changed: bump CRGPU_ABI_VERSION and every binding");
/// crgpu_jibes_expected_cells: throws Error(CRGPU_JIBES_CANT_CONVERGE, ...) where the reference raises CellEstimateCantConvergeException
inline double jibes_expected_cells(uint64_t n, uint32_t n_gems) {
    double out = 0.0;
    const int rc = crgpu_jibes_expected_cells(n, n_gems, &out);
    if (rc != CRGPU_OK) throw Error(rc, rc == CRGPU_JIBES_CANT_CONVERGE ? "Could not converge on an accurate cell estimate." : "jibes_expected_cells");
    return out;
}
struct JibesLatentStates {
    crgpu_jibes_setup setup;
    std::vector<uint8_t> states;  // [n_states x k]
    std::vector<double> prior;    // [n_states]
};
/// crgpu_jibes_latent_states + crgpu_jibes_log_prior with the uniform tag frequencies
inline JibesLatentStates jibes_latent_states(uint64_t n, uint32_t k, uint32_t n_gems, double estimated_cells, uint32_t max_k_lets = 3, double blank_prob = 0.04) {
    JibesLatentStates out;
    out.states.assign((size_t)CRGPU_JIBES_MAX_STATES * (k ? k : 1), 0);
    int rc = crgpu_jibes_latent_states(n, k, n_gems, max_k_lets, estimated_cells, out.states.data(), &out.setup);
    if (rc != CRGPU_OK) throw Error(rc, "jibes_latent_states: 1 .. 16 tags, max_k_lets 1 .. 3");
    out.states.resize((size_t)out.setup.n_states * k);
    out.prior.assign(out.setup.n_states, 0.0);
    rc = crgpu_jibes_log_prior(out.states.data(), out.setup.n_states, k, estimated_cells, n_gems, max_k_lets, out.setup.k_let_limited,
                               out.setup.max_modeled_k_let, blank_prob, nullptr, out.prior.data());
    if (rc != CRGPU_OK) throw Error(rc, "jibes_latent_states: the prior");
    return out;
}
struct JibesFit {
    crgpu_jibes_fit_result result;
    std::vector<double> probs;             // [n x (k + 2)]: the tags, Multiplet, Blank
    std::vector<int32_t> assignment;       // a tag, k = Multiplet, k + 1 = Blank, k + 2 = Unassigned
    std::vector<double> assignment_prob;
    std::vector<uint32_t> ml_state;        // the most likely Multiplet state, as a state index
};
/// crgpu_jibes_fit_dev: y [n x k] = log10(count + 1); (bg, fg, sd) the initial model; the reference's defaults otherwise
inline JibesFit jibes_fit(Context &ctx, const std::vector<double> &y, uint32_t k, const std::vector<double> &bg, const std::vector<double> &fg,
                          const std::vector<double> &sd, uint32_t n_gems, double estimated_cells, double abs_tol = 1e-2, double rel_tol = 1e-7,
                          uint32_t max_reps = 50000, double confidence = 0.9, uint32_t flags = 0) {
    if (!k || y.size() % k || bg.size() != k || fg.size() != k || sd.size() != k) throw Error(CRGPU_EINVAL, "jibes_fit: shapes");
    const size_t n = y.size() / k;
    JibesFit out;
    out.probs.assign(n * (k + 2), 0.0), out.assignment.assign(n, 0), out.assignment_prob.assign(n, 0.0), out.ml_state.assign(n, 0);
    crgpu_jibes_fit_args a{};
    a.bg = bg.data(), a.fg = fg.data(), a.sd = sd.data(), a.blank_prob = 0.04, a.estimated_cells = estimated_cells;
    a.abs_tol = abs_tol, a.rel_tol = rel_tol, a.confidence = confidence, a.n_gems = n_gems, a.max_k_lets = 3, a.max_reps = max_reps, a.flags = flags;
    if (n) a.probs_out = out.probs.data(), a.assignment_out = out.assignment.data(), a.assignment_prob_out = out.assignment_prob.data(), a.ml_state_out = out.ml_state.data();
    ctx.check(crgpu_jibes_fit_dev(ctx.get(), n ? y.data() : nullptr, n, k, &a, &out.result));
    return out;
}

// ---- marginal calls of guides, antibodies and tags ------------------------------------------------------------------------------------------
static_assert(sizeof(crgpu_marginal_row) == 96, "crgpu_marginal_row changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_marginal_calls) == 152, "crgpu_marginal_calls changed: bump CRGPU_ABI_VERSION and every binding");
struct MarginalCalls {
    std::vector<crgpu_marginal_row> rows;   // one per listed feature row
    std::vector<int64_t> indptr;            // the assignment matrix as CSR over the listed rows
    std::vector<uint32_t> columns;          // ascending inside a row
    std::vector<uint32_t> features_per_cell;
    uint64_t cells_with_0 = 0, cells_with_1 = 0, cells_with_many = 0, cells_without_umis = 0;
};
/// crgpu_marginal_calls_dev with everything brought to the host: feature_rows strictly ascending; umi_threshold 3 for guides, 1 otherwise
inline MarginalCalls marginal_calls(Context &ctx, const crgpu_matrix_dev *filtered, const std::vector<uint32_t> &feature_rows, uint32_t n_features,
                                    uint32_t umi_threshold = 1) {
    crgpu_marginal_calls *r = nullptr;
    ctx.check(crgpu_marginal_calls_dev(ctx.get(), filtered, feature_rows.data(), (uint32_t)feature_rows.size(), n_features, umi_threshold, 0, &r));
    MarginalCalls out;
    out.rows.assign(r->rows, r->rows + r->n_rows);
    out.cells_with_0 = r->cells_with_0, out.cells_with_1 = r->cells_with_1, out.cells_with_many = r->cells_with_many;
    out.cells_without_umis = r->cells_without_umis;
    int rc = detail::fetch(ctx, out.indptr, r->d_indptr, (uint64_t)r->n_rows + 1);
    if (rc == CRGPU_OK) rc = detail::fetch(ctx, out.columns, r->d_columns, r->n_assigned);
    if (rc == CRGPU_OK) rc = detail::fetch(ctx, out.features_per_cell, r->d_features_per_cell, r->n_barcodes);
    crgpu_marginal_calls_free(ctx.get(), r);
    ctx.check(rc);
    return out;
}
struct TagContaminants {
    std::vector<uint8_t> flags;                  // 0 kept, 1 contaminant, 2 dropped for zero UMIs
    std::vector<std::vector<uint32_t>> sources;  // per tag its source tags in the order met
};
/// crgpu_tag_moments_dev + crgpu_tag_contaminants with the reference's constants: order = the tags sorted by id, as a permutation
inline TagContaminants tag_contaminants(Context &ctx, const crgpu_matrix_dev *filtered, const std::vector<uint32_t> &tag_rows, uint32_t n_features,
                                        const std::vector<uint32_t> &order) {
    const uint32_t n = (uint32_t)tag_rows.size();
    if (order.size() != n) throw Error(CRGPU_EINVAL, "tag_contaminants: one place per tag");
    std::vector<uint64_t> sx(n), sxx(n), sxy((size_t)n * n);
    ctx.check(crgpu_tag_moments_dev(ctx.get(), filtered, tag_rows.data(), n, n_features, sx.data(), sxx.data(), sxy.data()));
    TagContaminants out;
    out.flags.assign(n, 0), out.sources.assign(n, {});
    std::vector<int32_t> src((size_t)n * n, -1);
    const int rc = crgpu_tag_contaminants(n, filtered->n_barcodes, sx.data(), sxx.data(), sxy.data(), order.data(), 1000, 50.0, 0.5, out.flags.data(), src.data());
    if (rc != CRGPU_OK) throw Error(rc, "tag_contaminants");
    for (uint32_t t = 0; t < n; t++)
        for (uint32_t j = 0; j < n && src[(size_t)t * n + j] >= 0; j++) out.sources[t].push_back((uint32_t)src[(size_t)t * n + j]);
    return out;
}

// ---- k-means clustering of a dense projection (RUN_KMEANS) -----------------------------------------------------------------------------------
static_assert(sizeof(crgpu_kmeans_args) == 24, "crgpu_kmeans_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_kmeans_result) == 80, "crgpu_kmeans_result changed: bump CRGPU_ABI_VERSION and every binding");
struct KmeansFit {
    uint32_t n_clusters = 0, n_iter = 0, relocations = 0;
    bool strict = false, in_lds = false;
    double inertia = 0.0, db_score = 0.0, fit_ms = 0.0;
    std::vector<int32_t> labels;     // scikit-learn's labels_
    std::vector<int32_t> clusters;   // 1-based, the largest cluster first (relabel_by_size)
    std::vector<double> centers;     // n_clusters x d
    std::vector<uint64_t> sizes;
    std::vector<double> wss;
};
/// crgpu_kmeans_dev for a list of distinct K on x (n rows of stride ld, the first d columns); inits: empty, or per K an empty vector
/// (k-means++) or K x d centres (scikit-learn's init = array)
inline std::vector<KmeansFit> kmeans(Context &ctx, const double *x, uint64_t n, uint32_t d, uint64_t ld, const std::vector<uint32_t> &ks, uint32_t seed = 0,
                                     const std::vector<std::vector<double>> &inits = {}, uint32_t max_iter = 300, double tol_factor = 1e-4) {
    const size_t m = ks.size();
    if (!inits.empty() && inits.size() != m) throw Error(CRGPU_EINVAL, "kmeans: one init (or an empty vector) per K");
    std::vector<const double *> ip(m, nullptr);
    for (size_t p = 0; p < inits.size(); p++) {
        if (inits[p].empty()) continue;
        if (inits[p].size() != (size_t)ks[p] * d) throw Error(CRGPU_EINVAL, "kmeans: an init is K x d");
        ip[p] = inits[p].data();
    }
    crgpu_kmeans_args a = {inits.empty() ? nullptr : ip.data(), tol_factor, seed, max_iter};
    std::vector<KmeansFit> out(m);
    std::vector<crgpu_kmeans_result> res(m);
    for (size_t p = 0; p < m; p++) {
        KmeansFit &f = out[p];
        f.n_clusters = ks[p];
        f.labels.assign(n, 0), f.clusters.assign(n, 0), f.centers.assign((size_t)ks[p] * d, 0.0), f.sizes.assign(ks[p], 0), f.wss.assign(ks[p], 0.0);
        res[p] = crgpu_kmeans_result{f.labels.data(), f.clusters.data(), f.centers.data(), f.sizes.data(), f.wss.data(), 0.0, 0.0, 0.0, 0, 0, 0, 0};
    }
    ctx.check(crgpu_kmeans_dev(ctx.get(), x, n, d, ld, ks.data(), (uint32_t)m, &a, res.data()));
    for (size_t p = 0; p < m; p++) {
        KmeansFit &f = out[p];
        f.inertia = res[p].inertia, f.db_score = res[p].db_score, f.fit_ms = res[p].fit_ms;
        f.n_iter = res[p].n_iter, f.relocations = res[p].relocations, f.strict = res[p].strict != 0, f.in_lds = res[p].in_lds != 0;
    }
    return out;
}
/// compute_db_index from the per-cluster sums
inline double kmeans_db_index(uint32_t k, uint32_t d, const std::vector<double> &centers, const std::vector<double> &wss, const std::vector<uint64_t> &counts) {
    double score = 0.0;
    if (centers.size() != (size_t)k * d || wss.size() != k || counts.size() != k) throw Error(CRGPU_EINVAL, "kmeans_db_index: centers is k x d, wss and counts k");
    const int rc = crgpu_kmeans_db_index(k, d, centers.data(), wss.data(), counts.data(), &score);
    if (rc != CRGPU_OK) throw Error(rc, "kmeans_db_index");
    return score;
}

// ---- sSeq differential expression of clusters (RUN_DIFFERENTIAL_EXPRESSION) -----------------------------------------------------------------
static_assert(sizeof(crgpu_sseq_args) == 16, "crgpu_sseq_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_sseq_params_info) == 80, "crgpu_sseq_params_info changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_sseq_result) == 160, "crgpu_sseq_result changed: bump CRGPU_ABI_VERSION and every binding");
/// adjust_pvalue_bh on the host
inline std::vector<double> sseq_adjust_bh(const std::vector<double> &p) {
    std::vector<double> q(p.size());
    const int rc = crgpu_sseq_adjust_bh(p.data(), p.size(), q.data());
    if (rc != CRGPU_OK) throw Error(rc, "sseq_adjust_bh");
    return q;
}
struct SseqParamValues {
    std::vector<double> size_factors, mean, var, phi_mm, phi;  // phi: NaN for a gene that is not used
    std::vector<uint8_t> use;
    double zeta_hat = 0.0, delta = 0.0;
    uint32_t n_used = 0;
};
/// crgpu_sseq_params of one matrix (features x cells, one feature type), resident on the device
class SseqParams {
public:
    SseqParams(Context &ctx, const crgpu_matrix_dev *m, uint32_t n_features) : ctx_(ctx), n_cells_(m ? m->n_barcodes : 0), n_features_(n_features) {
        crgpu_sseq_args a = {n_features, 0, 0, 0};
        ctx.check(crgpu_sseq_params_dev(ctx.get(), m, &a, &p_));
    }
    ~SseqParams() { crgpu_sseq_params_free(ctx_.get(), p_); }
    SseqParams(const SseqParams &) = delete;
    SseqParams &operator=(const SseqParams &) = delete;
    const crgpu_sseq_params *get() const { return p_; }
    uint64_t n_cells() const { return n_cells_; }
    uint32_t n_features() const { return n_features_; }
    SseqParamValues download() const {
        SseqParamValues v;
        v.size_factors.assign(n_cells_, 0.0), v.mean.assign(n_features_, 0.0), v.var.assign(n_features_, 0.0), v.phi_mm.assign(n_features_, 0.0);
        v.phi.assign(n_features_, 0.0), v.use.assign(n_features_, 0);
        crgpu_sseq_params_info info = {v.size_factors.data(), v.mean.data(), v.var.data(), v.phi_mm.data(), v.phi.data(), v.use.data(), 0.0, 0.0, 0, 0, 0};
        ctx_.check(crgpu_sseq_params_get(ctx_.get(), p_, &info));
        v.zeta_hat = info.zeta_hat, v.delta = info.delta, v.n_used = info.n_used;
        return v;
    }

private:
    Context &ctx_;
    crgpu_sseq_params *p_ = nullptr;
    uint64_t n_cells_;
    uint32_t n_features_;
};
struct SseqDiffexp {
    uint32_t n_clusters = 0, n_features = 0;
    std::vector<uint64_t> sums_in, sums_out;  // [K][G]
    std::vector<double> norm_mean_in, norm_mean_out, log2_fold_change, p_values, adjusted_p_values;  // [K][G]
    std::vector<uint8_t> below_median;        // [K][G]: 1 / 0 = the side an asymptotic test took, 255 = none
    std::vector<double> s_a, s_b;             // [K]
    std::vector<uint64_t> n_exact, n_asymptotic;
    uint64_t n_terms = 0, n_short = 0, n_wave = 0, n_workgroup = 0;
};
/// crgpu_sseq_diffexp_dev: every cluster of the 1-based labels against all other cells; wave_min / wg_min = the class thresholds of the
/// exact tests (0 = default), which change no result
inline SseqDiffexp sseq_diffexp(Context &ctx, const crgpu_matrix_dev *m, const SseqParams &params, const std::vector<int32_t> &labels, uint32_t n_clusters,
                                uint32_t wave_min = 0, uint32_t wg_min = 0) {
    if (!m || labels.size() != m->n_barcodes) throw Error(CRGPU_EINVAL, "sseq_diffexp: one label per cell");
    SseqDiffexp o;
    o.n_clusters = n_clusters, o.n_features = params.n_features();
    const size_t K = n_clusters ? n_clusters : 1, KG = K * params.n_features();
    o.sums_in.assign(KG, 0), o.sums_out.assign(KG, 0), o.norm_mean_in.assign(KG, 0.0), o.norm_mean_out.assign(KG, 0.0), o.log2_fold_change.assign(KG, 0.0);
    o.p_values.assign(KG, 0.0), o.adjusted_p_values.assign(KG, 0.0), o.below_median.assign(KG, 0), o.s_a.assign(K, 0.0), o.s_b.assign(K, 0.0);
    o.n_exact.assign(K, 0), o.n_asymptotic.assign(K, 0);
    crgpu_sseq_result r = {o.sums_in.data(), o.sums_out.data(), o.norm_mean_in.data(), o.norm_mean_out.data(), o.log2_fold_change.data(), o.p_values.data(),
                           o.adjusted_p_values.data(), o.below_median.data(), o.s_a.data(), o.s_b.data(), o.n_exact.data(), o.n_asymptotic.data(),
                           0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0};
    crgpu_sseq_args a = {params.n_features(), wave_min, wg_min, 0};
    ctx.check(crgpu_sseq_diffexp_dev(ctx.get(), m, params.get(), labels.data(), n_clusters, &a, &r));
    o.n_terms = r.n_terms, o.n_short = r.n_short, o.n_wave = r.n_wave, o.n_workgroup = r.n_workgroup;
    return o;
}

// ---- MERGE_CLUSTERS: medoids, complete linkage, local sSeq tests of sibling leaves ------------------------------------------------------
static_assert(sizeof(crgpu_sseq_pair_args) == 24, "crgpu_sseq_pair_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_sseq_pair_result) == 224, "crgpu_sseq_pair_result changed: bump CRGPU_ABI_VERSION and every binding");
struct SseqPair {
    std::vector<uint8_t> use, below_median;   // [G]
    std::vector<double> mean, phi_mm, phi, norm_mean_a, norm_mean_b, log2_fold_change, p_values, adjusted_p_values;  // [G]
    std::vector<uint64_t> sums_a, sums_b;     // [G]
    double zeta_hat = 0.0, delta = 0.0, s_a = 0.0, s_b = 0.0;
    uint64_t n_cells_a = 0, n_cells_b = 0, n_exact = 0, n_asymptotic = 0, n_terms = 0, n_de = 0;
    uint32_t n_used = 0;
};
/// crgpu_sseq_pairs: one matrix and one grouping of its cells (group_of_cell: -1 = in no group), transposed once for every pair test
class SseqPairs {
public:
    SseqPairs(Context &ctx, const crgpu_matrix_dev *m, const std::vector<int32_t> &group_of_cell, uint32_t n_groups, uint32_t n_features)
        : ctx_(ctx), n_features_(n_features) {
        if (!m || group_of_cell.size() != m->n_barcodes) throw Error(CRGPU_EINVAL, "SseqPairs: one group per cell");
        crgpu_sseq_pair_args a = {n_features, 0, 0, 0, 0.0};
        ctx.check(crgpu_sseq_pairs_create_dev(ctx.get(), m, group_of_cell.data(), n_groups, &a, &p_));
    }
    ~SseqPairs() { crgpu_sseq_pairs_free(ctx_.get(), p_); }
    SseqPairs(const SseqPairs &) = delete;
    SseqPairs &operator=(const SseqPairs &) = delete;
    /// crgpu_sseq_pair_dev: the groups of side a against those of side b (ascending, distinct, disjoint); de_threshold 0 = 0.05
    SseqPair compare(const std::vector<uint32_t> &groups_a, const std::vector<uint32_t> &groups_b, double de_threshold = 0.0, uint32_t wave_min = 0,
                     uint32_t wg_min = 0) const {
        SseqPair o;
        const size_t G = n_features_;
        o.use.assign(G, 0), o.below_median.assign(G, 0), o.mean.assign(G, 0.0), o.phi_mm.assign(G, 0.0), o.phi.assign(G, 0.0);
        o.norm_mean_a.assign(G, 0.0), o.norm_mean_b.assign(G, 0.0), o.log2_fold_change.assign(G, 0.0), o.p_values.assign(G, 0.0);
        o.adjusted_p_values.assign(G, 0.0), o.sums_a.assign(G, 0), o.sums_b.assign(G, 0);
        crgpu_sseq_pair_result r = {};
        r.use_out = o.use.data(), r.mean_out = o.mean.data(), r.phi_mm_out = o.phi_mm.data(), r.phi_out = o.phi.data();
        r.sums_a_out = o.sums_a.data(), r.sums_b_out = o.sums_b.data(), r.norm_mean_a_out = o.norm_mean_a.data(), r.norm_mean_b_out = o.norm_mean_b.data();
        r.log2_fold_change_out = o.log2_fold_change.data(), r.p_values_out = o.p_values.data(), r.adjusted_p_values_out = o.adjusted_p_values.data();
        r.below_median_out = o.below_median.data();
        crgpu_sseq_pair_args a = {n_features_, wave_min, wg_min, 0, de_threshold};
        ctx_.check(crgpu_sseq_pair_dev(ctx_.get(), p_, groups_a.data(), (uint32_t)groups_a.size(), groups_b.data(), (uint32_t)groups_b.size(), &a, &r));
        o.zeta_hat = r.zeta_hat, o.delta = r.delta, o.s_a = r.s_a, o.s_b = r.s_b, o.n_cells_a = r.n_cells_a, o.n_cells_b = r.n_cells_b;
        o.n_exact = r.n_exact, o.n_asymptotic = r.n_asymptotic, o.n_terms = r.n_terms, o.n_de = r.n_de, o.n_used = r.n_used;
        return o;
    }
    /// crgpu_sseq_pair_bootstrap_dev: per item and draw the sum of the item's gene over a resample of group_a / of group_b
    /// -> (sums_a, sums_b), u64[items x B] each (B = n_bootstraps, 0 = 500); the stream is Philox, not the reference's np.random
    std::pair<std::vector<uint64_t>, std::vector<uint64_t>> bootstrap(const std::vector<crgpu_pb_item> &items, uint32_t n_bootstraps = 0, uint64_t seed = 0,
                                                                      uint32_t lds_cells = 0, uint32_t draws_per_wg = 0) const {
        const size_t B = n_bootstraps ? n_bootstraps : 500;
        std::vector<uint64_t> sa(items.size() * B), sb(items.size() * B);
        crgpu_pb_args a = {n_bootstraps, lds_cells, draws_per_wg, 0, seed};
        ctx_.check(crgpu_sseq_pair_bootstrap_dev(ctx_.get(), p_, items.data(), (uint32_t)items.size(), &a, sa.data(), sb.data()));
        return {std::move(sa), std::move(sb)};
    }

private:
    Context &ctx_;
    crgpu_sseq_pairs *p_ = nullptr;
    uint32_t n_features_;
};
// ---- MEASURE_PERTURBATIONS: the bootstrap sums (SseqPairs::bootstrap above) and the confidence interval --------------------------------
static_assert(sizeof(crgpu_pb_item) == 16, "crgpu_pb_item changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_pb_args) == 24, "crgpu_pb_args changed: bump CRGPU_ABI_VERSION and every binding");
/// crgpu_perturbation_ci (host only): the percentiles ci_lower / ci_upper of the draws' log2 fold changes; s_a, s_b = those of the pair
inline std::pair<double, double> perturbation_ci(const uint64_t *sums_a, const uint64_t *sums_b, uint32_t n_bootstraps, double s_a, double s_b,
                                                 double ci_lower = 5.0, double ci_upper = 95.0, std::vector<double> *log2fc = nullptr) {
    if (log2fc) log2fc->assign(n_bootstraps, 0.0);
    double lo = 0.0, hi = 0.0;
    const int rc = crgpu_perturbation_ci(sums_a, sums_b, n_bootstraps, s_a, s_b, ci_lower, ci_upper, log2fc ? log2fc->data() : nullptr, &lo, &hi);
    if (rc != CRGPU_OK) throw Error(rc, "crgpu_perturbation_ci");
    return {lo, hi};
}
/// crgpu_cluster_medians_dev: np.median of every dimension over the rows of every cluster (labels 0 .. n_clusters - 1) -> [n_clusters][d]
inline std::vector<double> cluster_medians(Context &ctx, const std::vector<double> &x, uint64_t n, uint32_t d, const std::vector<int32_t> &labels,
                                           uint32_t n_clusters) {
    if (x.size() != n * d || labels.size() != n) throw Error(CRGPU_EINVAL, "cluster_medians: x is n x d, one label per row");
    std::vector<double> med((size_t)n_clusters * d);
    ctx.check(crgpu_cluster_medians_dev(ctx.get(), x.data(), n, d, d, labels.data(), n_clusters, med.data(), nullptr));
    return med;
}
/// crgpu_linkage_complete (host only): scipy's linkage(points, "complete") -> Z [k - 1][4]
inline std::vector<double> linkage_complete(const std::vector<double> &points, uint32_t k, uint32_t d) {
    if (points.size() != (size_t)k * d || k < 2) throw Error(CRGPU_EINVAL, "linkage_complete: points is k x d, k >= 2");
    std::vector<double> z((size_t)(k - 1) * 4);
    const int rc = crgpu_linkage_complete(points.data(), k, d, z.data());
    if (rc != CRGPU_OK) throw Error(rc, "linkage_complete");
    return z;
}

// ---- exact k-nearest-neighbour graph of a dense projection: the query of RUN_GRAPH_CLUSTERING -----------------------------------------
static_assert(sizeof(crgpu_knn_args) == 32, "crgpu_knn_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_knn_result) == 96, "crgpu_knn_result changed: bump CRGPU_ABI_VERSION and every binding");
/// split()'s rule: int(max(num_neighbors, np.round(a + b * log10(n)))) clamped to [1, n - 1]
inline uint32_t graphclust_num_neighbors(uint64_t n, uint32_t num_neighbors = 1, double a = -230.0, double b = 120.0) {
    uint32_t k = 0;
    const int rc = crgpu_graphclust_num_neighbors(n, num_neighbors, a, b, &k);
    if (rc != CRGPU_OK) throw Error(rc, "graphclust_num_neighbors");
    return k;
}
struct Knn {
    uint64_t n_queries = 0;
    uint32_t k = 0;
    std::vector<int32_t> indices, sorted_indices;  // [n_queries][k]: by rank; ascending (the CSR row of merge_nearest_neighbors)
    std::vector<double> distances;                 // [n_queries][k]
    crgpu_knn_result info{};                       // the counters and times; its pointers are those of the vectors above
};
/// crgpu_knn_dev on x (n rows of stride ld, the first d columns): BallTree.query(rows, k + 1)[:, 1:] for the rows query_start ..
/// query_start + n_queries (0, 0 = all); capacity / force_device / cand_tile = the test seams (0 = default), which change no result
inline Knn knn(Context &ctx, const double *x, uint64_t n, uint32_t d, uint64_t ld, uint32_t k, uint64_t query_start = 0, uint64_t n_queries = 0,
               uint32_t capacity = 0, uint32_t force_device = 0, uint32_t cand_tile = 0) {
    Knn o;
    o.n_queries = (query_start == 0 && n_queries == 0) ? n : n_queries, o.k = k;
    const size_t m = (size_t)o.n_queries * k;
    o.indices.assign(m, 0), o.sorted_indices.assign(m, 0), o.distances.assign(m, 0.0);
    crgpu_knn_args a = {query_start, n_queries, capacity, force_device, cand_tile, 0};
    o.info = crgpu_knn_result{o.indices.data(), o.distances.data(), o.sorted_indices.data(), 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0, 0};
    ctx.check(crgpu_knn_dev(ctx.get(), x, n, d, ld, k, &a, &o.info));
    return o;
}

// ---- RUN_TSNE: the perplexity search, the symmetrised sparse P, the exact gradient and the descent -------------------------------------
static_assert(sizeof(crgpu_tsne_args) == 48, "crgpu_tsne_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_tsne_result) == 168, "crgpu_tsne_result changed: bump CRGPU_ABI_VERSION and every binding");
struct TsneAffinities {
    std::vector<double> beta, values;              // [n]; [nnz]
    std::vector<uint32_t> steps;                   // [n]
    std::vector<int64_t> indptr;                   // [n + 1]
    std::vector<int32_t> indices;                  // [nnz], ascending within a row
    crgpu_tsne_result info{};
};
/// crgpu_tsne_affinities_dev on the neighbours knn() delivers at k = floor(3 * perplexity): the symmetrised P as CSR, its values add to 1
inline TsneAffinities tsne_affinities(Context &ctx, const int32_t *nn_indices, const double *nn_distances, uint64_t n, uint32_t k, double perplexity) {
    TsneAffinities o;
    const size_t room = (size_t)2 * n * k;
    o.beta.assign(n, 0.0), o.steps.assign(n, 0), o.indptr.assign(n + 1, 0), o.indices.assign(room, 0), o.values.assign(room, 0.0);
    crgpu_tsne_args a{};
    o.info.beta_out = o.beta.data(), o.info.steps_out = o.steps.data(), o.info.indptr_out = o.indptr.data();
    o.info.indices_out = o.indices.data(), o.info.values_out = o.values.data();
    ctx.check(crgpu_tsne_affinities_dev(ctx.get(), nn_indices, nn_distances, n, k, perplexity, &a, &o.info));
    o.indices.resize(o.info.nnz), o.values.resize(o.info.nnz);
    return o;
}
/// crgpu_tsne_dev: the iterations first_iter .. first_iter + n_iters of max_iter on y, uY, gains ([n][dims], in and out); returns the
/// counters, info.kl the cost at the y the call ends on
inline crgpu_tsne_result tsne_run(Context &ctx, const TsneAffinities &p, uint32_t dims, std::vector<double> &y, std::vector<double> &uY,
                                  std::vector<double> &gains, uint32_t first_iter, uint32_t n_iters, uint32_t max_iter = 1000,
                                  uint32_t stop_lying_iter = 250, uint32_t mom_switch_iter = 250) {
    crgpu_tsne_args a{};
    a.first_iter = first_iter, a.n_iters = n_iters, a.max_iter = max_iter, a.stop_lying_iter = stop_lying_iter, a.mom_switch_iter = mom_switch_iter;
    crgpu_tsne_result r{};
    ctx.check(crgpu_tsne_dev(ctx.get(), p.indptr.data(), p.indices.data(), p.values.data(), p.indptr.size() - 1, dims, y.data(), uY.data(), gains.data(),
                             &a, &r));
    return r;
}

// ---- RUN_UMAP: the fuzzy kNN graph and the sampled epochs of the layout ---------------------------------------------------------------
static_assert(sizeof(crgpu_umap_args) == 72, "crgpu_umap_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_umap_result) == 136, "crgpu_umap_result changed: bump CRGPU_ABI_VERSION and every binding");
struct UmapGraph {
    std::vector<double> rho, sigma, values;        // [n]; [n]; [nnz]
    std::vector<uint32_t> steps;                   // [n]
    std::vector<int64_t> indptr;                   // [n + 1]
    std::vector<int32_t> indices;                  // [nnz], ascending within a row
    crgpu_umap_result info{};
};
/// crgpu_umap_graph_dev on the neighbours knn() delivers at k = n_neighbors - 1: the pruned fuzzy union as CSR, twin entries equal bit for bit
inline UmapGraph umap_graph(Context &ctx, const int32_t *nn_indices, const double *nn_distances, uint64_t n, uint32_t k, uint32_t n_epochs) {
    UmapGraph o;
    const size_t room = (size_t)2 * n * k;
    o.rho.assign(n, 0.0), o.sigma.assign(n, 0.0), o.steps.assign(n, 0), o.indptr.assign(n + 1, 0), o.indices.assign(room, 0), o.values.assign(room, 0.0);
    o.info.rho_out = o.rho.data(), o.info.sigma_out = o.sigma.data(), o.info.steps_out = o.steps.data(), o.info.indptr_out = o.indptr.data();
    o.info.indices_out = o.indices.data(), o.info.values_out = o.values.data();
    ctx.check(crgpu_umap_graph_dev(ctx.get(), nn_indices, nn_distances, n, k, n_epochs, &o.info));
    o.indices.resize(o.info.nnz), o.values.resize(o.info.nnz);
    return o;
}
/// crgpu_umap_epochs_dev: the epochs first_epoch .. first_epoch + n_run of n_epochs on y ([n][dims]) and the two schedule states ([nnz]),
/// all in and out; a, b from crgpu_umap_ab; returns the counters
inline crgpu_umap_result umap_run(Context &ctx, const UmapGraph &g, uint32_t dims, std::vector<double> &y, std::vector<double> &next_sample,
                                  std::vector<double> &next_negative, double a, double b, uint64_t seed, uint32_t first_epoch, uint32_t n_run,
                                  uint32_t n_epochs) {
    crgpu_umap_args args{};
    args.a = a, args.b = b, args.seed = seed, args.first_epoch = first_epoch, args.n_run = n_run, args.n_epochs = n_epochs;
    next_sample.resize(g.values.size()), next_negative.resize(g.values.size());
    crgpu_umap_result r{};
    ctx.check(crgpu_umap_epochs_dev(ctx.get(), g.indptr.data(), g.indices.data(), g.values.data(), g.indptr.size() - 1, dims, y.data(), next_sample.data(),
                                    next_negative.data(), &args, &r));
    return r;
}

// ---- RUN_GRAPH_CLUSTERING: Louvain in exact integer rounds -------------------------------------------------------------------------------
static_assert(sizeof(crgpu_louvain_args) == 32, "crgpu_louvain_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_louvain_result) == 136, "crgpu_louvain_result changed: bump CRGPU_ABI_VERSION and every binding");
struct LouvainClusters {
    std::vector<std::vector<int32_t>> levels;      // the partition of every level, level l over the nodes of level l
    std::vector<int32_t> level0, final_labels;     // [n]; [n]: level 0 composed through every level
    std::vector<uint32_t> nodes, communities, rounds;  // per level
    std::vector<int64_t> S;                        // per level: Q = S / M^2
    std::vector<double> ms;                        // per level: host time of its rounds
    crgpu_louvain_result info{};
};
/// crgpu_louvain_dev on a CSR (symmetrize: the union of both directions of an unweighted neighbour matrix, weights NULL): the published
/// algorithm in synchronous integer rounds, no parity with bin/louvain
inline LouvainClusters louvain(Context &ctx, const int64_t *indptr, const int32_t *indices, const uint32_t *weights, uint64_t n, bool symmetrize = true,
                               uint32_t max_rounds = 0) {
    LouvainClusters o;
    std::vector<int32_t> flat((size_t)4 * n + 64);
    o.level0.assign(n, 0), o.final_labels.assign(n, 0);
    o.nodes.assign(CRGPU_LOUVAIN_MAX_LEVELS, 0), o.communities.assign(CRGPU_LOUVAIN_MAX_LEVELS, 0), o.rounds.assign(CRGPU_LOUVAIN_MAX_LEVELS, 0);
    o.S.assign(CRGPU_LOUVAIN_MAX_LEVELS, 0), o.ms.assign(CRGPU_LOUVAIN_MAX_LEVELS, 0.0);
    crgpu_louvain_args args{};
    args.symmetrize = symmetrize ? 1u : 0u, args.max_rounds = max_rounds;
    for (;;) {
        args.levels_capacity = flat.size();
        o.info = crgpu_louvain_result{};
        o.info.levels_out = flat.data(), o.info.level0_out = o.level0.data(), o.info.final_out = o.final_labels.data();
        o.info.level_nodes_out = o.nodes.data(), o.info.level_communities_out = o.communities.data(), o.info.level_rounds_out = o.rounds.data();
        o.info.level_S_out = o.S.data(), o.info.level_ms_out = o.ms.data();
        ctx.check(crgpu_louvain_dev(ctx.get(), indptr, indices, weights, n, &args, &o.info));
        if (o.info.levels_needed <= flat.size()) break;
        flat.assign(o.info.levels_needed, 0);      // the run is a pure function of its input: the second call gives the same levels
    }
    o.nodes.resize(o.info.n_levels), o.communities.resize(o.info.n_levels), o.rounds.resize(o.info.n_levels), o.S.resize(o.info.n_levels), o.ms.resize(o.info.n_levels);
    size_t at = 0;
    for (uint32_t l = 0; l < o.info.n_levels; at += o.nodes[l++]) o.levels.emplace_back(flat.begin() + at, flat.begin() + at + o.nodes[l]);
    return o;
}

// ---- CORRECT_CHEMISTRY_BATCH: batch-balanced neighbours, mutual nearest neighbours, the correction of the merged batches ---------------
static_assert(sizeof(crgpu_knn_cross_args) == 48, "crgpu_knn_cross_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_bc_step) == 48, "crgpu_bc_step changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_bc_args) == 16, "crgpu_bc_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_bc_result) == 96, "crgpu_bc_result changed: bump CRGPU_ABI_VERSION and every binding");
/// crgpu_knn_cross_dev: find_knn(cur, ref, k) = BallTree(ref).query(cur, k) for the query rows query_start .. + n_queries against the
/// candidate rows cand_start .. + n_cands ALONE; nothing dropped, global indices; capacity / force_device / cand_tile = the test seams
inline Knn knn_cross(Context &ctx, const double *x, uint64_t n, uint32_t d, uint64_t ld, uint32_t k, uint64_t query_start, uint64_t n_queries,
                     uint64_t cand_start, uint64_t n_cands, uint32_t capacity = 0, uint32_t force_device = 0, uint32_t cand_tile = 0) {
    Knn o;
    o.n_queries = n_queries, o.k = k;
    const size_t m = (size_t)n_queries * k;
    o.indices.assign(m, 0), o.sorted_indices.assign(m, 0), o.distances.assign(m, 0.0);
    crgpu_knn_cross_args a = {query_start, n_queries, cand_start, n_cands, capacity, force_device, cand_tile, 0};
    o.info = crgpu_knn_result{o.indices.data(), o.distances.data(), o.sorted_indices.data(), 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0, 0};
    ctx.check(crgpu_knn_cross_dev(ctx.get(), x, n, d, ld, k, &a, &o.info));
    return o;
}
struct MnnPairs {
    std::vector<int32_t> pairs;                    // [n][2]: (row of batch i, row of batch j), ascending
    uint64_t n_first = 0, n_second = 0;            // distinct rows of i, of j: the numerators of overlap_percentage
};
/// crgpu_mnn_pairs (host only): a = [n_i][k] neighbours in batch j of the rows start_i .., b = [n_j][k] the other direction, global indices
inline MnnPairs mnn_pairs(const std::vector<int32_t> &a, uint64_t start_i, const std::vector<int32_t> &b, uint64_t start_j, uint32_t k) {
    MnnPairs o;
    uint64_t n = 0;
    o.pairs.assign(2 * a.size() + 2, 0);
    const int rc = k ? crgpu_mnn_pairs(a.data(), a.size() / k, start_i, b.data(), b.size() / k, start_j, k, o.pairs.data(), a.size(), &n, &o.n_first, &o.n_second)
                     : CRGPU_EINVAL;
    if (rc != CRGPU_OK) throw Error(rc, "mnn_pairs");
    o.pairs.resize(2 * n);
    return o;
}
struct BcStep {
    std::vector<int32_t> cur_rows, mnn_cur, mnn_ref;
};
struct BatchCorrect {
    std::vector<double> aligned;                   // [n][d]
    std::vector<std::vector<double>> corr;         // per step [n_cur][d] (want_corr)
    std::vector<double> step_ms;                   // [steps][4]: gather, accumulate, finish, apply
    crgpu_bc_result info{};
};
/// crgpu_batch_correct_dev: the steps in order, corr from the matrix as it stands at a step's start, then x[cur_rows] += corr;
/// pair_tile / row_tile / slab_rows = the test seams (0 = default), which change no result
inline BatchCorrect batch_correct(Context &ctx, const double *x, uint64_t n, uint32_t d, uint64_t ld, double sigma, const std::vector<BcStep> &steps,
                                  bool want_corr = false, uint32_t pair_tile = 0, uint32_t row_tile = 0, uint32_t slab_rows = 0) {
    BatchCorrect o;
    o.aligned.assign((size_t)n * d, 0.0), o.step_ms.assign(4 * steps.size() + 4, 0.0), o.corr.resize(want_corr ? steps.size() : 0);
    std::vector<crgpu_bc_step> st(steps.size() + 1);
    for (size_t i = 0; i < steps.size(); i++) {
        if (want_corr) o.corr[i].assign(steps[i].cur_rows.size() * d, 0.0);
        st[i] = crgpu_bc_step{steps[i].cur_rows.data(), steps[i].mnn_cur.data(), steps[i].mnn_ref.data(), want_corr ? o.corr[i].data() : nullptr,
                              steps[i].cur_rows.size(), std::min(steps[i].mnn_cur.size(), steps[i].mnn_ref.size())};
    }
    crgpu_bc_args a = {pair_tile, row_tile, slab_rows, 0};
    o.info.step_ms_out = o.step_ms.data();
    ctx.check(crgpu_batch_correct_dev(ctx.get(), x, n, d, ld, sigma, st.data(), (uint32_t)steps.size(), o.aligned.data(), &a, &o.info));
    o.step_ms.resize(4 * steps.size());
    return o;
}

// ---- RUN_PCA: the dispersion order of the features, IRLBA, the projection ----------------------------------------------------------------
static_assert(sizeof(crgpu_pca_args) == 64, "crgpu_pca_args changed: bump CRGPU_ABI_VERSION and every binding");
static_assert(sizeof(crgpu_pca_result) == 128, "crgpu_pca_result changed: bump CRGPU_ABI_VERSION and every binding");
struct Pca {
    std::vector<double> transformed;               // [n_barcodes][n_components]
    std::vector<double> components;                // [n_components][n_features], 0 outside the used features
    std::vector<double> variance_explained, d;     // [n_components]
    std::vector<double> dispersion;                // [n_features], NaN for the features the threshold removed
    std::vector<int32_t> features_selected;        // the rows of org_cols_used, in that order
    crgpu_pca_result info{};                       // status (CRGPU_PCA_*), n_components as used, it, mprod, the times
};
/// crgpu_pca_dev on a filtered matrix of one feature type: run_pca at ONE threshold.  info.status != CRGPU_PCA_OK: nothing was computed
/// (the stage then calls again with min_count_threshold = 0).  wave_block / dot_parts_per_block = the test seams, which change no result
inline Pca pca(Context &ctx, const crgpu_matrix_dev *m, uint32_t n_features, uint32_t n_components = 10, uint32_t pca_features = 0,
               const std::vector<uint64_t> &pca_bc_indices = {}, uint32_t seed = 0, uint32_t min_count_threshold = CRGPU_PCA_DEFAULT_THRESHOLD,
               const std::vector<double> &start = {}, uint32_t wave_block = 0, uint32_t dot_parts_per_block = 0) {
    Pca o;
    const uint32_t nc = n_components ? n_components : 1u;
    o.transformed.assign((size_t)m->n_barcodes * nc, 0.0), o.components.assign((size_t)nc * n_features, 0.0);
    o.variance_explained.assign(nc, 0.0), o.d.assign(nc, 0.0), o.dispersion.assign(n_features, 0.0), o.features_selected.assign(n_features, 0);
    crgpu_pca_args a = {pca_bc_indices.empty() ? nullptr : pca_bc_indices.data(), pca_bc_indices.size(), start.empty() ? nullptr : start.data(), start.size(),
                        n_components, pca_features, min_count_threshold, seed, wave_block, dot_parts_per_block, 0, 0};
    o.info = crgpu_pca_result{o.transformed.data(), o.components.data(), o.variance_explained.data(), o.dispersion.data(), o.features_selected.data(),
                              o.d.data(), 0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    ctx.check(crgpu_pca_dev(ctx.get(), m, n_features, &a, &o.info));
    const uint32_t nu = o.info.status == CRGPU_PCA_OK ? o.info.n_components : 0u;
    o.transformed.resize((size_t)m->n_barcodes * nu), o.components.resize((size_t)nu * n_features);
    o.variance_explained.resize(nu), o.d.resize(nu), o.features_selected.resize(o.info.status == CRGPU_PCA_OK ? o.info.n_used_features : 0u);
    return o;
}
/// np.random.RandomState(seed).randn(n), bit for bit (host only)
inline std::vector<double> legacy_randn(uint32_t seed, uint64_t n) {
    std::vector<double> out(n);
    if (crgpu_legacy_randn(seed, n, out.data()) != CRGPU_OK) throw Error(CRGPU_EINVAL, "legacy_randn");
    return out;
}

// ---- protein aggregates of an antibody / antigen well; the closing filters of a cell call ---------------------------------------------
static_assert(sizeof(crgpu_aggregates_info) == 48, "crgpu_aggregates_info changed: bump CRGPU_ABI_VERSION and every binding");
/// int(np.round(n_signal * _calculate_fraction_to_use(n_signal)))
inline uint32_t aggregate_min_antibodies(uint32_t n_signal) {
    uint32_t out = 0;
    const int rc = crgpu_aggregate_min_antibodies(n_signal, &out);
    if (rc != CRGPU_OK) throw Error(rc, crgpu_last_error(nullptr));
    return out;
}
struct Aggregates {
    std::vector<uint64_t> removed;   // ascending
    std::vector<uint8_t> reasons;    // CRGPU_AGG_COUNTS | CRGPU_AGG_HIGHLY_CORRECTED | CRGPU_AGG_ANTIGEN per removed column
    std::vector<uint64_t> kept;      // ascending: what select_barcodes takes
    crgpu_aggregates_info info{};
    double antigen_threshold = 0.0;  // NaN without a column
};
/// remove_antibody_antigen_aggregates on the raw matrix up to the column lists: feature_kind = CRGPU_AGG_KIND_* per feature; reads /
/// corrected_reads = the Antibody library's per column (both empty: no highly-corrected detection)
inline Aggregates detect_aggregates(Context &ctx, const crgpu_matrix_dev *raw, const std::vector<uint8_t> &feature_kind, uint32_t num_probe_barcodes = 0,
                                    const std::vector<uint32_t> &reads = {}, const std::vector<uint32_t> &corrected_reads = {}) {
    const uint64_t V = raw->n_barcodes;
    if (reads.size() != corrected_reads.size() || (!reads.empty() && reads.size() != V)) throw Error(CRGPU_EINVAL, "detect_aggregates: shapes");
    Aggregates out;
    detail::DeviceCopy<uint8_t> d_reason(ctx, std::vector<uint8_t>(V, 0));
    if (!reads.empty()) {
        detail::DeviceCopy<uint32_t> d_reads(ctx, reads), d_corr(ctx, corrected_reads);
        ctx.check(crgpu_aggregates_highly_corrected_dev(ctx.get(), d_reads.get(), d_corr.get(), V, (uint8_t *)d_reason.d, nullptr));
    }
    uint32_t n = 0;
    ctx.check(crgpu_aggregates_by_counts_dev(ctx.get(), raw, feature_kind.data(), (uint32_t)feature_kind.size(), num_probe_barcodes,
                                             (uint8_t *)d_reason.d, nullptr, 0, &n, &out.info));
    ctx.check(crgpu_aggregates_antigen_outliers_dev(ctx.get(), raw, feature_kind.data(), (uint32_t)feature_kind.size(), (uint8_t *)d_reason.d, nullptr, 0,
                                                    &n, &out.antigen_threshold));
    uint64_t *d_kept = nullptr, *d_removed = nullptr, n_kept = 0, n_removed = 0;
    ctx.check(crgpu_aggregates_partition_dev(ctx.get(), d_reason.get(), V, &d_kept, &n_kept, &d_removed, &n_removed));
    int rc = detail::fetch(ctx, out.kept, (const uint64_t *)d_kept, n_kept);
    if (rc == CRGPU_OK) rc = detail::fetch(ctx, out.removed, (const uint64_t *)d_removed, n_removed);
    if (rc == CRGPU_OK && n_removed) {
        detail::DeviceCopy<uint8_t> d_why(ctx, std::vector<uint8_t>(n_removed, 0));
        rc = crgpu_take_columns_dev(ctx.get(), d_reason.get(), 1, V, d_removed, n_removed, d_why.d);
        if (rc == CRGPU_OK) rc = detail::fetch(ctx, out.reasons, d_why.get(), n_removed);
    }
    crgpu_free(ctx.get(), d_kept);
    crgpu_free(ctx.get(), d_removed);
    ctx.check(rc);
    return out;
}
/// apply_global_minimum_umis_threshold: the cells (ascending columns) whose entry of umis_per_col is >= minimum_umis
inline std::vector<uint64_t> apply_minimum_umis(Context &ctx, const std::vector<uint32_t> &umis_per_col, const std::vector<uint64_t> &cells,
                                                uint64_t minimum_umis) {
    detail::DeviceCopy<uint32_t> d_umis(ctx, umis_per_col);
    detail::DeviceCols d_cells(ctx, cells);
    uint64_t *d_kept = nullptr, n = 0;
    ctx.check(crgpu_filter_cells_min_umis_dev(ctx.get(), d_umis.get(), umis_per_col.size(), d_cells.get(), cells.size(), minimum_umis, &d_kept, &n));
    std::vector<uint64_t> out;
    const int rc = detail::fetch(ctx, out, (const uint64_t *)d_kept, n);
    crgpu_free(ctx.get(), d_kept);
    ctx.check(rc);
    return out;
}
struct MitoFilter {
    std::vector<uint64_t> kept, removed;  // in the order of the call
};
/// apply_mitochondrial_threshold: cells with 100.0 * mito / total > max_mito_percent leave (0 / 0 stays)
inline MitoFilter apply_mito_threshold(Context &ctx, const std::vector<uint32_t> &mito_per_col, const std::vector<uint32_t> &total_per_col,
                                       const std::vector<uint64_t> &cells, double max_mito_percent) {
    if (mito_per_col.size() != total_per_col.size()) throw Error(CRGPU_EINVAL, "apply_mito_threshold: shapes");
    detail::DeviceCopy<uint32_t> d_mito(ctx, mito_per_col), d_total(ctx, total_per_col);
    detail::DeviceCols d_cells(ctx, cells);
    uint64_t *d_kept = nullptr, *d_removed = nullptr, n_kept = 0, n_removed = 0;
    ctx.check(crgpu_filter_cells_mito_dev(ctx.get(), d_mito.get(), d_total.get(), total_per_col.size(), d_cells.get(), cells.size(), max_mito_percent,
                                          &d_kept, &n_kept, &d_removed, &n_removed));
    MitoFilter out;
    int rc = detail::fetch(ctx, out.kept, (const uint64_t *)d_kept, n_kept);
    if (rc == CRGPU_OK) rc = detail::fetch(ctx, out.removed, (const uint64_t *)d_removed, n_removed);
    crgpu_free(ctx.get(), d_kept);
    crgpu_free(ctx.get(), d_removed);
    ctx.check(rc);
    return out;
}

}  // namespace crgpu
