"""MEASURE_PERTURBATIONS restated in numpy: the specification of csrc/perturbations.h and engine.measure_perturbations (include/crgpu.h,
section MEASURE_PERTURBATIONS).  It follows lib/python/cellranger/feature/crispr/measure_perturbations.py of the reference: the grouping
of the cells (_get_ps_clusters), the loop of _analyze_transcriptome around a pair test that is handed in, the bootstrap of
_get_fold_change_cis with the project's Philox stream in place of the unseeded np.random, the summary and the top genes.

The stream: position q of draw b of side z (0 = a, 1 = b) of the item with stream number t takes the cell at index (w * n) >> 64 of the
side's n cells, w = element q of np.random.Philox(counter=[0, s, 0, 0], key=[seed, 0]).random_raw(), s = (t << 33) | (z << 32) | b."""
import collections

import numpy as np

FILTER_LIST = ("None", "Non-Targeting", "Ignore")
CONTROL = "Non-Targeting"
MIN_CELLS = 10
SUMMARY_COLUMNS = ["Perturbation", "target_string", "Log2 Fold Change", "p Value", "Log2 Fold Change Lower Bound", "Log2 Fold Change Upper Bound",
                   "Cells with Perturbation", "Mean UMI Count Among Cells with Perturbation", "Cells with Non-Targeting Guides",
                   "Mean UMI Count Among Cells with Non-Targeting Guides"]

# ---- hand cases of the grouping, written from the reference's statements ------------------------------------------------------------
FEATURE_REF = [dict(id="G1", target_gene_id="ENSG01", target_gene_name="GENEA"),      # a target whose name differs from its id
               dict(id="G2", target_gene_id="ENSG02", target_gene_name="GENEB"),
               dict(id="G3", target_gene_id="ENSG02", target_gene_name="GENEB"),      # a second guide of the same target
               dict(id="NT1", target_gene_id="Non-Targeting", target_gene_name="Non-Targeting"),
               dict(id="NT2", target_gene_id="Non-Targeting", target_gene_name="Non-Targeting")]
FEATURE_REF_NO_NAMES = [dict(id=r["id"], target_gene_id=r["target_gene_id"]) for r in FEATURE_REF]
BARCODES = ["bc%d-1" % i for i in range(8)]
CALLS = {"bc0-1": ("G1", 1),          # a single guide
         "bc1-1": ("G1|G2", 2),       # two guides with different targets
         "bc2-1": ("NT1|NT2", 2),     # two Non-Targeting guides: a control cell
         "bc3-1": ("NT1|G2", 2),      # Non-Targeting plus a target: the target
         "bc4-1": ("NT1", 1),
         # bc5-1: no call
         "bc6-1": ("G2|G3", 2),       # two guides of one target
         "bc7-1": ("G2", 1)}
# (feature_ref, by_feature, ignore_multiples) -> (cluster per barcode, names in cluster order)
HAND_CASES = {
    "by_target": (FEATURE_REF, False, False, [1, 2, 4, 3, 4, 5, 3, 3], ["GENEA", "GENEA|GENEB", "GENEB", "Non-Targeting", "None"]),
    "by_target_ignore_multiples": (FEATURE_REF, False, True, [1, 3, 3, 3, 4, 5, 3, 2], ["GENEA", "GENEB", "Ignore", "Non-Targeting", "None"]),
    "by_feature": (FEATURE_REF, True, False, [1, 2, 7, 6, 7, 5, 4, 3], ["G1", "G1|G2", "G2", "G2|G3", "Ignore", "NT1|G2", "Non-Targeting"]),
    "by_feature_ignore_multiples": (FEATURE_REF, True, True, [1, 3, 3, 3, 4, 3, 3, 2], ["G1", "G2", "Ignore", "Non-Targeting"]),
    "by_target_without_names": (FEATURE_REF_NO_NAMES, False, False, [1, 2, 4, 3, 4, 5, 3, 3], ["ENSG01", "ENSG01|ENSG02", "ENSG02", "Non-Targeting", "None"]),
}


def target_info(feature_ref):
    return {r["id"]: dict(target_id=r["target_gene_id"], target_name=r.get("target_gene_name", r["target_gene_id"])) for r in feature_ref}


def clusters(feature_ref, calls, barcodes, by_feature=False, ignore_multiples=False):
    """-> (cluster_per_bc, {cluster: name}); a multi-guide cell's targets are joined in sorted order"""
    info = target_info(feature_ref)
    target_of, feature_of = {}, {}
    for bc in barcodes:
        if bc not in calls:
            target_of[bc], feature_of[bc] = "None", "None"
            continue
        call, n = calls[bc]
        tid = info[call]["target_id"] if call in info else call
        if n > 1:
            ids = set(info[f]["target_id"] for f in call.split("|"))
            if ignore_multiples:
                tid = "Ignore"
            elif ids == {CONTROL}:
                tid = CONTROL
            else:
                tid = "|".join(sorted(ids - set(FILTER_LIST))) or "Ignore"
        target_of[bc], feature_of[bc] = tid, call
    if by_feature:
        def key(bc):
            if target_of[bc] not in FILTER_LIST:
                return feature_of[bc]
            return "Ignore" if target_of[bc] == "None" else target_of[bc]
        per_bc = [key(bc) for bc in barcodes]
        uniq = sorted(set(per_bc))
        names = {i + 1: u for i, u in enumerate(uniq)}
    else:
        name_of = {v["target_id"]: v["target_name"] for v in info.values()}
        per_bc = [target_of[bc] for bc in barcodes]
        uniq = sorted(set(per_bc))
        names = {i + 1: "|".join(name_of.get(p, p) for p in u.split("|")) for i, u in enumerate(uniq)}
    return np.array([uniq.index(v) + 1 for v in per_bc], np.int64), names


# ---- the stream -----------------------------------------------------------------------------------------------------------------------
def stream_id(stream, z, b):
    return (int(stream) << 33) | (int(z) << 32) | int(b)


def raw_words(seed, stream, z, b, n):
    return np.random.Philox(counter=[0, stream_id(stream, z, b), 0, 0], key=[int(seed), 0]).random_raw(int(n))


def mulhi(w, n):
    """the specification: Python integers"""
    return (int(w) * int(n)) >> 64


def mulhi_u64(w, n):
    """(w * n) >> 64 for n < 2^32 in u64 arithmetic: w = wh 2^32 + wl, (wh n + (wl n >> 32)) >> 32 -- no term reaches 2^64"""
    w = np.asarray(w, np.uint64)
    n = np.uint64(n)
    wh, wl = w >> np.uint64(32), w & np.uint64(0xFFFFFFFF)
    return (wh * n + ((wl * n) >> np.uint64(32))) >> np.uint64(32)


def draw_indices(seed, stream, z, b, n):
    return mulhi_u64(raw_words(seed, stream, z, b, n), n).astype(np.int64)


def bootstrap_sums(column, seed, stream, z, B):
    """column: the gene's counts over the side's cells in (group, cell) order -> u64[B]"""
    col = np.asarray(column, np.uint64)
    return np.array([col[draw_indices(seed, stream, z, b, len(col))].sum(dtype=np.uint64) for b in range(B)], np.uint64)


def log_terms(sums_a, sums_b, s_a, s_b):
    ta = np.log2((1 + np.asarray(sums_a).astype(np.int64)) / (1 + s_a))
    tb = np.log2((1 + np.asarray(sums_b).astype(np.int64)) / (1 + s_b))
    return ta, tb


def ci(sums_a, sums_b, s_a, s_b, lower=5.0, upper=95.0):
    """_get_fold_change_cis on given sums: s_a, s_b = the size factor sums of the ORIGINAL cells -> (lower, upper, log2fc[B])"""
    ta, tb = log_terms(sums_a, sums_b, s_a, s_b)
    fc = ta - tb
    return float(np.percentile(fc, lower)), float(np.percentile(fc, upper)), fc


# ---- the stage around a pair test that is handed in -----------------------------------------------------------------------------------
def top_genes(r, gene_ids, gene_names, keep=10):
    rows = [g for g in range(len(gene_ids)) if r["sums_b"][g] > 0 and (r["sums_a"][g] >= 5 or r["sums_b"][g] >= 5)]
    rows.sort(key=lambda g: (-abs(float(r["log2_fold_change"][g])), float(r["adjusted_p_values"][g]), gene_names[g]))
    return [(gene_names[g], gene_ids[g], float(r["log2_fold_change"][g]), float(r["adjusted_p_values"][g])) for g in rows[:keep]]


def measure(x, gene_ids, gene_names, feature_ref, calls, barcodes, compare, by_feature=False, ignore_multiples=False, B=500, seed=0, bounds=(5.0, 95.0)):
    """x int[G, cells]; compare(cells_a, cells_b) -> the pair's dict (sums_a, sums_b, log2_fold_change, p_values, adjusted_p_values, s_a,
    s_b).  None where the reference returns None"""
    if any("target_gene_id" not in r for r in feature_ref) or CONTROL not in [r["target_gene_id"] for r in feature_ref]:
        return None
    info = target_info(feature_ref)
    id_of = {f: v["target_id"] for f, v in info.items()} if by_feature else {v["target_name"]: v["target_id"] for v in info.values()}
    per_bc, names = clusters(feature_ref, calls, barcodes, by_feature, ignore_multiples)
    num_cells = {name: int((per_bc == c).sum()) for c, name in names.items()}
    control = [c for c, name in names.items() if name == CONTROL]
    if not control:
        return None
    cells_b = np.flatnonzero(per_bc == control[0])
    fold, fold_ci, per, order, skipped, stream = {}, {}, collections.OrderedDict(), [], [], 0
    columns = []
    for c in sorted(names):
        name = names[c]
        if name in FILTER_LIST:
            continue
        parts = name.split("|")
        ids = [id_of[p] for p in parts]
        cells_a = np.flatnonzero(per_bc == c)
        if all(i in FILTER_LIST for i in ids) or len(cells_a) < MIN_CELLS:
            skipped.append(name)
            continue
        r = compare(cells_a, cells_b)
        per[name] = r
        order.append(name)
        columns += [np.asarray(r["sums_a"]) / len(cells_a), r["log2_fold_change"], r["adjusted_p_values"]]
        fold[name], fold_ci[name] = {}, {}
        for part, target in zip(parts, ids):
            if target in FILTER_LIST or target not in gene_ids:
                continue
            g = gene_ids.index(target)
            fold[name][part] = (float(r["log2_fold_change"][g]), float(r["p_values"][g]), int(r["sums_a"][g]), int(r["sums_b"][g]))
            sa, sb = bootstrap_sums(x[g, cells_a], seed, stream, 0, B), bootstrap_sums(x[g, cells_b], seed, stream, 1, B)
            lo, hi, _ = ci(sa, sb, r["s_a"], r["s_b"], *bounds)
            fold_ci[name][part] = (lo, hi, sa, sb)
            stream += 1
    rows = []
    for name in sorted(fold):
        for part, res in fold[name].items():
            n, nc = num_cells[name], num_cells[CONTROL]
            rows.append((name, part, res[0], res[1], fold_ci[name][part][0], fold_ci[name][part][1], n, res[2] / n if n else float("nan"), nc,
                         res[3] / nc if nc else float("nan")))
    rows.sort(key=lambda row: row[2])
    header = list(SUMMARY_COLUMNS)
    header[1] = "Target Guide" if by_feature else "Target Gene"
    table = np.stack(columns, axis=1) if columns else np.zeros((len(gene_ids), 0))
    return dict(log2_fold_change=fold, log2_fold_change_ci=fold_ci, num_cells_per_perturbation=num_cells, results_per_perturbation=per, names=order,
                skipped=skipped, results_all_perturbations=table, summary=rows, summary_columns=header,
                top_perturbed_genes={n: top_genes(r, gene_ids, gene_names) for n, r in per.items()}, cluster_per_bc=per_bc, perturbation_keys=names)
