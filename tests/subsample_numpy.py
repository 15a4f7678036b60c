"""numpy restatement of the read subsampling (the reference for cellranger_amd's crgpu_subsample_dev / _plan / _summary).

Written after lib/python/cellranger/subsample.py: compute_target_depths / _subsampling_for_depth / make_subsamplings (:140-309),
_run_subsample_task (:572-654) for ONE chunk that holds the whole table, and the per-task numbers of
calculate_subsampling_metrics (:719-845).  The reference module itself needs compiled extensions and h5py, so nothing here is
pinned against its output; the hand-computed cases of tests/test_subsample_restatement.py are the anchor.

The one deliberate difference: np.random.seed(1); np.random.binomial(count, rate) is replaced by the counter-based draw `kept`
below, which the device reproduces bit for bit."""
import numpy as np

PER_CELL, CELLS_ONLY, BULK = 0, 1, 2
PLAN_RAW, PLAN_MAPPED, PLAN_RAW_CELLS, PLAN_BULK = 0, 1, 2, 3
FIXED_DEPTHS = [3000, 5000, 10000, 20000, 30000, 50000]
TARGETED_FIXED_DEPTHS = [100, 250, 500, 1000, 2500, 3000, 5000, 10000, 15000, 20000, 30000, 40000, 50000]
BULK_FIXED_DEPTHS = [int(x) for x in (1e4, 5e4, 1e5, 2.5e5, 5e5, 1e6, 2.5e6, 5e6, 7.5e6, 1e7, 5e7, 1e8, 1e9)]
NUM_ADDITIONAL_DEPTHS = 10


# ---- the draw ---------------------------------------------------------------------------------------------------------------------
def thresholds(rates):
    """floor(rate * 2^53) as python ints (exact: the product is a power-of-two scaling)"""
    return [int(np.floor(np.ldexp(float(r), 53))) if not np.isnan(r) else 0 for r in rates]


def read_words(m, count, seed=1):
    """u of the reads 0 .. count - 1 of molecule m: the first `count` raw words of Philox stream m, shifted right by 11"""
    if count == 0:
        return np.zeros(0, np.uint64)
    return np.random.Philox(counter=[0, int(m), 0, 0], key=[int(seed), 0]).random_raw(int(count)) >> np.uint64(11)


def kept(counts, libs, rates, seed=1, positions=None):
    """kept[m] = #{j < counts[m] : u(m, j) < floor(rates[libs[m]] * 2^53)}; positions[m] = the stream of molecule m (default m:
    its place in the molecule table)"""
    thr = thresholds(rates)
    out = np.zeros(len(counts), np.int64)
    for i in range(len(counts)):
        m = i if positions is None else int(positions[i])
        out[i] = int(np.count_nonzero(read_words(m, int(counts[i]), seed) < np.uint64(thr[int(libs[i])])))
    return out


def kept_all_tasks(counts, libs, rates, seed=1, positions=None):
    """the same for rates[task][lib]: one generation of the words serves every task"""
    rates = np.asarray(rates, np.float64)
    thr = [thresholds(r) for r in rates]
    out = np.zeros((len(rates), len(counts)), np.int64)
    for i in range(len(counts)):
        m = i if positions is None else int(positions[i])
        u = read_words(m, int(counts[i]), seed)
        for t in range(len(rates)):
            out[t, i] = int(np.count_nonzero(u < np.uint64(thr[t][int(libs[i])])))
    return out


_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mul_hi_lo(a, b):
    """the 128-bit product of the constant a and the uint64 array b as (high, low) words, from 32-bit limbs"""
    a_lo, a_hi = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    b_lo, b_hi = b & _M32, b >> _S32
    ll, lh, hl, hh = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    mid = (ll >> _S32) + (lh & _M32) + (hl & _M32)
    return hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32), (mid << _S32) | (ll & _M32)


def philox4x64_10(c0, c1, seed):
    """Philox4x64-10 of the counters (c0, c1, 0, 0) (uint64 arrays) under the key (seed, 0): four uint64 arrays"""
    c0, c1 = np.asarray(c0, np.uint64), np.asarray(c1, np.uint64)
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = int(seed) & (2 ** 64 - 1), 0
    for _ in range(10):
        hi0, lo0 = _mul_hi_lo(0xD2E7470EE14C6C93, c0)
        hi1, lo1 = _mul_hi_lo(0xCA5A826395121157, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + 0x9E3779B97F4A7C15) & (2 ** 64 - 1), (k1 + 0xBB67AE8584CAA73B) & (2 ** 64 - 1)
    return c0, c1, c2, c3


def kept_vectorised(counts, libs, rates, seed=1, positions=None):
    """`kept` without a python loop over the molecules (the CPU yardstick of scripts/bench_subsample.py)"""
    counts = np.asarray(counts).astype(np.int64)
    n = len(counts)
    thr = np.array(thresholds(rates), np.uint64)[np.asarray(libs).astype(np.int64)]
    pos = np.arange(n, dtype=np.uint64) if positions is None else np.asarray(positions).astype(np.uint64)
    n_blocks = (counts + 3) // 4
    mol = np.repeat(np.arange(n), n_blocks)                      # the molecule of every Philox block
    blk = np.arange(len(mol)) - np.repeat(np.cumsum(n_blocks) - n_blocks, n_blocks)
    words = philox4x64_10((blk + 1).astype(np.uint64), pos[mol], seed)
    keep = np.zeros(len(mol), np.int64)
    for k in range(4):
        keep += ((4 * blk + k < counts[mol]) & ((words[k] >> np.uint64(11)) < thr[mol])).astype(np.int64)
    return np.bincount(mol, weights=keep, minlength=n).astype(np.int64)


# ---- one task, group by group -----------------------------------------------------------------------------------------------------
def run_task(task_type, rates, bc, lib, feature, kept_reads, cell_ranks, cell_genome_mask, feature_genome, n_genomes, n_features):
    """Tallies of one task on a table ordered by barcode (bc = canonical ranks), `kept_reads` already drawn.  Returns
    (umis_per_bc, read_pairs_per_bc, features_det_per_bc [genome][cell], read_pairs, umis [genome], total_features_det
    [genome][feature])."""
    n_cells = len(cell_ranks)
    upb, rpb, fpb = (np.zeros((n_genomes, n_cells), np.int64) for _ in range(3))
    rp_task, um_task = np.zeros(n_genomes, np.int64), np.zeros(n_genomes, np.int64)
    tfd = np.zeros((n_genomes, n_features), np.int64)
    rates = np.asarray(rates, np.float64)
    if np.count_nonzero(rates) == 0:
        return upb, rpb, fpb, rp_task, um_task, tfd
    if len(lib) and np.isnan(rates[lib]).any():
        return upb, rpb, fpb, rp_task, um_task, tfd
    if len(lib) and (np.any(rates[lib] < 0) or np.any(rates[lib] > 1)):
        raise ValueError("subsampling probabilities cannot be < 0 or > 1")
    genome = np.asarray(feature_genome)[feature] if len(feature) else np.zeros(0, np.int64)
    cell_index = {int(r): i for i, r in enumerate(cell_ranks)}
    if task_type == BULK:
        groups = [np.arange(len(bc))] if len(bc) else []
    else:
        edges = np.flatnonzero(np.concatenate(([True], bc[1:] != bc[:-1], [True]))) if len(bc) else []
        groups = [np.arange(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]
    for idx in groups:
        ci = cell_index.get(int(bc[idx[0]])) if task_type != BULK else None
        for g in range(n_genomes):
            is_cell = ci is not None and (cell_genome_mask is None or (int(cell_genome_mask[ci]) >> g) & 1 == 1)
            if task_type == CELLS_ONLY and not is_cell:
                continue
            mine = genome[idx] == g
            surv = idx[(kept_reads[idx] > 0) & mine]
            reads = int(kept_reads[idx][mine].sum())
            if task_type == BULK:
                upb[g, :] = len(surv)
                rpb[g, :] = reads
                fpb[g, :] = 0
                tfd[g, :] = np.bincount(feature[surv], minlength=n_features)
            elif is_cell:
                upb[g, ci] = len(surv)
                rpb[g, ci] = reads
                fpb[g, ci] = len(set(feature[surv].tolist()))
                tfd[g, :] += np.bincount(feature[surv], minlength=n_features)
            rp_task[g] += reads
            um_task[g] += len(surv)
    return upb, rpb, fpb, rp_task, um_task, tfd


def run(task_types, rates, mol, cell_ranks, n_genomes=1, feature_genome=None, cell_genome_mask=None, feature_mask=None, seed=1,
        n_features=None, n_libs=None, kept_reads=None):
    """All tasks on a molecule table `mol` (dict of bc, lib, feature, read_count in table order): the dict the device returns.
    The streams are numbered by the position in the table BEFORE the feature mask."""
    rates = np.asarray(rates, np.float64)
    T, n_libs = len(rates), rates.shape[1] if n_libs is None else n_libs
    bc, lib, feature, count = (np.asarray(mol[k]).astype(np.int64) for k in ("bc", "lib", "feature", "read_count"))
    if n_features is None:
        n_features = len(feature_genome) if feature_genome is not None else len(feature_mask)
    fg = np.zeros(n_features, np.int64) if feature_genome is None else np.asarray(feature_genome).astype(np.int64)
    pos = np.arange(len(bc))
    if feature_mask is not None:
        keep = np.asarray(feature_mask).astype(bool)[feature]
        bc, lib, feature, count, pos = bc[keep], lib[keep], feature[keep], count[keep], pos[keep]
        if kept_reads is not None:
            kept_reads = np.asarray(kept_reads)[:, keep]
    if kept_reads is None:
        kept_reads = kept_all_tasks(count, lib, np.where(np.isnan(rates), 0.0, rates), seed, pos)
    n_cells = len(cell_ranks)
    out = dict(umis_per_bc=np.zeros((T, n_genomes, n_cells), np.int64), features_det_per_bc=np.zeros((T, n_genomes, n_cells), np.int64),
               read_pairs_per_bc=np.zeros((T, n_genomes, n_cells), np.int64), read_pairs=np.zeros((T, n_genomes), np.int64),
               umis=np.zeros((T, n_genomes), np.int64), total_features_det=np.zeros((T, n_genomes, n_features), np.int64))
    any_reads = np.zeros((n_libs, n_genomes), bool)
    for l, g in set(zip(lib[count > 0].tolist(), fg[feature[count > 0]].tolist())):
        any_reads[l, g] = True
    out["any_reads"] = any_reads
    for t in range(T):
        r = run_task(int(task_types[t]), rates[t], bc, lib, feature, kept_reads[t], cell_ranks, cell_genome_mask, fg, n_genomes, n_features)
        for k, v in zip(("umis_per_bc", "read_pairs_per_bc", "features_det_per_bc", "read_pairs", "umis", "total_features_det"), r):
            out[k][t] = v
    return out


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def compute_target_depths(max_target, num_targets):
    d = np.unique(np.linspace(start=0, stop=max_target, num=num_targets + 1, dtype=int))
    return d[d > 0]


def plan(subsample_type, lib_indices, num_cells_per_lib, raw_reads_per_lib, usable_reads_per_lib, fixed_depths,
         num_additional_depths=NUM_ADDITIONAL_DEPTHS):
    """(depths, rates[depth][library])"""
    idx = np.asarray(lib_indices, np.int64)
    cells, raw, usable = (np.asarray(x).astype(float) for x in (num_cells_per_lib, raw_reads_per_lib, usable_reads_per_lib))
    with np.errstate(divide="ignore", invalid="ignore"):
        raw_rppc, usable_rppc, usable_frac = raw / cells, usable / cells, usable / raw
    if subsample_type == PLAN_BULK:
        max_target = np.min(raw[idx])
    else:
        max_target = np.min((usable_rppc if subsample_type == PLAN_MAPPED else raw_rppc)[idx])
    computed = compute_target_depths(max_target, num_additional_depths)
    max_computed = np.max(computed) if len(computed) else None
    depths = np.unique(np.concatenate([computed, np.asarray(fixed_depths, int)]).astype(int))
    rows = []
    for depth in depths:
        if subsample_type == PLAN_BULK:
            target = np.full(cells.shape, float(depth))
        elif subsample_type == PLAN_MAPPED:
            target = depth * cells
        else:
            target = depth * cells * usable_frac
        den = raw if subsample_type == PLAN_BULK else usable
        r = np.zeros(len(cells))
        for i in idx:
            if den[i] != 0.0:
                r[i] = target[i] / den[i]
        if max_computed is not None and depth == max_computed:
            mx = np.max(r)
            if mx != 0.0:
                r = r / mx
        r[r > 1.0] = 0.0
        rows.append(r)
    return depths.astype(np.int64), np.array(rows, np.float64).reshape(len(depths), len(cells))


# ---- the summary ------------------------------------------------------------------------------------------------------------------
def dup_frac(read_pairs, umis):
    return float(read_pairs - umis) / float(read_pairs) if read_pairs > 0 else 0.0


def summary(data, task_types, cell_genome_mask=None):
    """([task][genome][mean reads, median reads, mean umis, median umis, mean features, median features, dup frac], [task])"""
    T, G, n_cells = data["umis_per_bc"].shape
    out, allf = np.zeros((T, G, 7)), np.zeros(T)
    for t in range(T):
        for g in range(G):
            cells = np.arange(n_cells) if cell_genome_mask is None else np.flatnonzero((np.asarray(cell_genome_mask) >> g) & 1)
            with np.errstate(all="ignore"):
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    for k, name in enumerate(("read_pairs_per_bc", "umis_per_bc", "features_det_per_bc")):
                        out[t, g, 2 * k] = np.mean(data[name][t, g, cells])
                        out[t, g, 2 * k + 1] = np.median(data[name][t, g, cells])
            if task_types[t] == BULK:
                out[t, g, 4] = out[t, g, 5] = np.count_nonzero(data["total_features_det"][t, g])
            out[t, g, 6] = dup_frac(int(data["read_pairs"][t, g]), int(data["umis"][t, g]))
        allf[t] = dup_frac(int(np.sum(data["read_pairs"][t])), int(np.sum(data["umis"][t])))
    return out, allf
