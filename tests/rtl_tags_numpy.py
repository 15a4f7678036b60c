"""Restatement of CALL_TAGS_RTL (lib/rust/cr_lib/src/stages/call_tags_rtl.rs:143-498, barcode_overlap.rs,
read_level_multiplexing.rs:22-68, cr_types/src/utils.rs:57-70, barcode/src/whitelist.rs:181-192) and of
remove_bcs_from_high_occupancy_gems with its threshold simulation (lib/python/cellranger/cell_calling_helpers.py:273-424, without the
read fractions), with plain dicts and sets over (gel bead, probe) pairs.  Deliberately not vectorised: it is what the device code and
the engine's host functions are compared against, with equality.

A well is described by
    cols          list of (gel, probe) per matrix column, ascending
    counts        list of {feature: count} per column (no explicit zeros)
    feature_type  list: the type name of every feature
    probe_id      list: the identifier string of every probe rank (the translated identifier, as as_translation_seq_to_id gives)
    cells         ascending list of column indices: the filtered barcodes
"""
import math
from collections import Counter

import numpy as np

ANTIBODY = "Antibody Capture"


def categorize(bc_id):
    """categorize_multiplexing_barcode_id: 'RTL', 'Antibody', 'Crispr', 'Overhang' or 'CMO'"""
    head, tail = bc_id[:2], bc_id[2:]
    num = int(tail) if tail.isdigit() else None
    if head == "BC" and num is not None and num <= 24:
        return "RTL"
    if head == "BC" and num is None and bc_id[-1:] in ("A", "B", "C", "D"):
        return "RTL"
    if (head == "BC" and num is not None and num >= 25) or (head == "AB" and num is not None):
        return "Antibody"
    if head == "CR" and num is not None:
        return "Crispr"
    if head == "OH" and num is not None:
        return "Overhang"
    return "CMO"


def rust_round(x):
    """f64::round: half away from zero"""
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


def median_of_sorted(xs):
    n = len(xs)
    if n == 0:
        return None
    if n % 2 == 0:
        return (xs[n // 2 - 1] + xs[n // 2]) // 2
    return xs[n // 2]


def barcodes_per_id(cols, probe_id):
    out = {}
    for c, (_, p) in enumerate(cols):
        out.setdefault(probe_id[p], []).append(c)
    return out


def umi_per_id(cols, counts, feature_type, probe_id):
    out = {}
    for (_, p), col in zip(cols, counts):
        for f, n in col.items():
            per = out.setdefault(feature_type[f], {})
            per[probe_id[p]] = per.get(probe_id[p], 0) + n
    return out


def group(constructs, seq_to_id, weights=None):
    """ProbeBarcodeGelBeadGrouper: id -> {gel: observations}"""
    out = {}
    for k, (gel, p) in enumerate(constructs):
        per = out.setdefault(seq_to_id[p], {})
        per[gel] = per.get(gel, 0) + (1 if weights is None else weights[k])
    return out


def overlap_counts(groups):
    ids = sorted(groups)
    out = {}
    for a in range(len(ids)):
        for b in range(a + 1, len(ids)):
            out[(ids[a], ids[b])] = sum(1 for gel in groups[ids[a]] if gel in groups[ids[b]])
    return out


def overlap_rows(groups):
    """calculate_frp_gem_barcode_overlap: [(id1, id2, gems1, gems2, common, overlap)]"""
    rows = []
    for (a, b), common in sorted(overlap_counts(groups).items()):
        g1, g2 = len(groups[a]), len(groups[b])
        low = min(g1, g2)
        rows.append((a, b, g1, g2, common, float(common) / float(low) if low else float("nan")))   # Rust: 0.0 / 0.0 = NaN
    return rows


def median_umi_per_cell(cols, counts, feature_type, cells):
    sums = {}
    for c in cells:
        for f, n in counts[c].items():
            key = (feature_type[f], c)
            sums[key] = sums.get(key, 0) + n
    per = {}
    for (ty, c), n in sums.items():
        if n > 0:
            per.setdefault((ty, cols[c][1]), []).append(n)
    return {key: median_of_sorted(sorted(v)) for key, v in per.items()}


def suspicious_pairings(cols, counts, feature_type, probe_id, pairings, medians, gex_groups):
    """detect_suspicious_rtl_ab_pairings; pairings: RTL identifier -> its antibody identifier"""
    reverse = [pairings.get(i, i) for i in probe_id]
    constructs, weights = [], []
    for (gel, p), col in zip(cols, counts):
        for f, n in col.items():
            if feature_type[f] == ANTIBODY:
                constructs.append((gel, p))
                weights.append(n)
    ab = group(constructs, reverse, weights)
    med = {}
    for (ty, p), m in medians.items():
        if ty == ANTIBODY:
            med[reverse[p]] = m
    for ident in list(ab):
        if ident not in med:
            del ab[ident]
            continue
        assert categorize(ident) == "Antibody", ident
        low = int(rust_round(0.1 * float(med[ident])))
        ab[ident] = {gel: n for gel, n in ab[ident].items() if n >= low}
    combined = ab
    for ident, gels in gex_groups.items():
        per = combined.setdefault(ident, {})
        for gel, n in gels.items():
            per[gel] = per.get(gel, 0) + n
    return filter_suspicious(overlap_rows(combined), pairings)


def filter_suspicious(all_rows, pairings):
    """the tail of detect_suspicious_rtl_ab_pairings: RTL + Antibody rows that are no configured pairing, RTL first, sorted"""
    ignore = set(pairings.items())
    rows = []
    for a, b, g1, g2, common, ov in all_rows:
        kinds = (categorize(a), categorize(b))
        if kinds == ("RTL", "Antibody"):
            pair = (a, b)
        elif kinds == ("Antibody", "RTL"):
            pair = (b, a)
        else:
            continue
        if pair in ignore:
            continue
        rows.append((a, b, g1, g2, common, ov) if kinds[0] == "RTL" else (b, a, g2, g1, common, ov))
    return sorted(rows, key=lambda r: (r[0], r[1]))


def call_tags_rtl(cols, counts, feature_type, probe_id, cells, pairings=None):
    """the join of the stage -> (barcodes_per_tag, rows, metrics, umi_per_probe_barcode)"""
    gex = group([cols[c] for c in cells], probe_id)
    rows = overlap_rows(gex)
    if pairings:
        med = median_umi_per_cell(cols, counts, feature_type, cells)
        rows = rows + suspicious_pairings(cols, counts, feature_type, probe_id, pairings, med, gex)
    gels = set()
    for per in gex.values():
        gels.update(per)
    metrics = dict(filtered_gel_bead_barcodes_count=len(gels),
                   filtered_barcodes_per_probe_barcode={i: len(per) for i, per in gex.items()},
                   probe_barcode_overlap_coefficients={"%s_%s" % (r[0], r[1]): r[5] for r in rows})
    return barcodes_per_id(cols, probe_id), rows, metrics, umi_per_id(cols, counts, feature_type, probe_id)


# ---- high-occupancy GEMs ---------------------------------------------------------------------------------------------------------
def occupancy(cell_constructs, partitions=115000, recovery_factor=1 / 1.65):
    """the head of remove_bcs_from_high_occupancy_gems -> (histogram dict, estimated_lambda, total_probe_barcodes, per_gem Counter)"""
    per_gem = Counter(gel for gel, _ in cell_constructs)
    hist = Counter(per_gem.values())
    hist[0] = max(0, int((partitions * recovery_factor) - len(per_gem)))
    lam = float(np.average(list(hist.keys()), weights=list(hist.values())))
    return dict(hist), lam, len(set(p for _, p in cell_constructs)), per_gem


def threshold(estimated_lambda, probes_observed, total_simulated_gems=1000000):
    """_get_high_occupancy_gem_threshold with numpy's legacy global stream"""
    if estimated_lambda == 0:
        return 0
    np.random.seed(0)
    draws = np.random.poisson(estimated_lambda, total_simulated_gems)
    sizes = list(draws[draws > 0])
    widest = np.max(sizes)
    freq = np.array(list(Counter(probes_observed).values())) / len(probes_observed)
    sim = np.random.choice(list(range(len(freq))), size=(len(sizes), widest), p=freq)
    distinct = [len(set(sim[i, :k])) for i, k in enumerate(sizes)]
    return int(np.ceil(np.quantile(distinct, 0.999)))


def remove_high_occupancy(cell_constructs, thr):
    """-> (kept positions in the cell list, high GEMs, cells in them, fraction of cell GEMs, fraction of cells)"""
    per_gem = Counter(gel for gel, _ in cell_constructs)
    high = [k for k, (gel, _) in enumerate(cell_constructs) if per_gem[gel] > thr]
    n_high = sum(1 for n in per_gem.values() if n > thr)
    drop = set(high)
    kept = [k for k in range(len(cell_constructs)) if k not in drop]

    def div(a, b):
        return float(a) / float(b) if b else float("nan")

    return kept, n_high, len(high), div(n_high, len(per_gem)), div(len(high), len(cell_constructs))
