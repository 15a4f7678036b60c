"""Constructed inputs for the feature stage: captures, read rows and feature lists that sit on chosen sides of the boundaries
of feature.hip (k_match_features, k_match_features_lds) and feature_extract.hip (k_extract_features and its queue,
k_extract_tethered_lds, k_feature_counts).

Host only: numpy, no device, no oracle.  The constants the cases turn on are read out of the source text, so a changed
constant moves the cases with it and a vanished line fails loudly.  A case is the definitions (or the pre-cut pattern table),
the reads as a handful of distinct rows plus the row every read repeats, an optional distribution, and a list of claims about
its own structure; describe() recomputes the structure (which kernel the dispatch chooses and with what window, what every
read is to that kernel, how many candidates a capture has, how many captures wait in a workgroup's queue per batch) from the
arrays alone and check_claims() asserts every claim.

Expected results come from a plain restatement of correct_feature_barcode / find_closest / match_read
(cr_types/src/reference/feature_extraction.rs:34-117, :358-470) in Python floats: the patterns as the regular expressions the
reference compiles, candidates in position-major A<C<G<T order, the map with replacement and likelihood_sum += like - old,
u8-wrapping quality arithmetic and p_edit = 10 ** (-qv / 10).  Nothing is compared with a tolerance."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_FEATURE = NO_CAPTURE = 0xFFFFFFFF
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
ACGT = b"ACGT"
FEATURE_CONF_THRESHOLD = 0.975
FEATURE_MAX_QV = 33
Q0 = 60                                        # the quality of a base nothing is said about (phred 27)
EDGE_QUALS = (32, 33, 34, 65, 66, 67, 126)     # 32 wraps to 255 (capped), 66 is the cap, 67 and 126 lie above it


# ---- constants from the source ------------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(ROOT, "cellranger_amd", "csrc", name)) as f:
        return f.read()


def _define(text, name, where):
    m = re.search(r"^#define\s+%s\s+\(?\s*(0x[0-9a-fA-F]+|\d+)u?\s*\)?\s*(?://.*)?$" % name, text, re.M)
    if not m:
        raise RuntimeError("feature_cases: #define %s not found in %s" % (name, where))
    return int(m.group(1), 0)


def _find(text, pattern, what, where):
    m = re.search(pattern, text)
    if not m:
        raise RuntimeError("feature_cases: %s not found in %s" % (what, where))
    return m


def _read_constants():
    fx, fm, cm = _source("feature_extract.hip"), _source("feature.hip"), _source("common.h")
    X, M = "feature_extract.hip", "feature.hip"
    k = {}
    k["FX_LOCAL_ENTRIES"] = _define(fx, "FX_LOCAL_ENTRIES", X)
    k["FC_SLOTS"] = _define(fx, "FC_SLOTS", X)
    k["FM_MAX_FEATURES"] = _define(fm, "FM_MAX_FEATURES", M)
    k["FXT_MAXC"] = int(_find(fx, r"constexpr uint32_t FXT_MAXC = (\d+);", "FXT_MAXC", X).group(1))
    _find(fx, r"#define FXT_EMPTY 0xFFFFFFFFFFFFFFFFull", "FXT_EMPTY", X)
    m = _find(fx, r"cur == FC_EMPTY && s_used < FC_SLOTS \* (\d+)u / (\d+)u", "the fill rule of k_feature_counts", X)
    k["FC_FILL"] = k["FC_SLOTS"] * int(m.group(1)) // int(m.group(2))
    k["FC_PROBES"] = int(_find(fx, r"probe < (\d+) && !placed; probe\+\+, t = \(t \+ 1u\) & \(FC_SLOTS - 1u\)", "the probe bound of k_feature_counts", X).group(1))
    m = _find(fx, r"uint32_t t = \(f \* (0x[0-9A-Fa-f]+)u\) >> (\d+);", "the hash of k_feature_counts", X)
    k["FC_MUL"], k["FC_SHIFT"] = int(m.group(1), 16), int(m.group(2))
    assert (1 << (32 - k["FC_SHIFT"])) == k["FC_SLOTS"]
    m = _find(fx, r"fxt_hash\(unsigned long long key, uint32_t mask\) \{\s*return \(uint32_t\)\(\(key \* (0x[0-9A-Fa-f]+)ull\) >> (\d+)\) & mask;", "fxt_hash", X)
    k["FXT_MUL"], k["FXT_SHIFT"] = int(m.group(1), 16), int(m.group(2))
    m = _find(fm, r"fm_hash\(uint32_t key, uint32_t mask\) \{ return \(\(key \* (0x[0-9A-Fa-f]+)u\) >> (\d+)\) & mask; \}", "fm_hash", M)
    k["FM_MUL"], k["FM_SHIFT"] = int(m.group(1), 16), int(m.group(2))
    _find(cm, r"cr_grid\(uint64_t n, uint32_t block, uint32_t max_blocks = 256u \* 8u\) \{\s*uint64_t g = \(n \+ block - 1\) / block;\s*"
              r"if \(g < 1\) g = 1;\s*if \(g > max_blocks\) g = max_blocks;", "cr_grid", "common.h")
    # the launches: (threads, largest grid) of either size of both LDS kernels
    for text, kern, var, where in ((fm, "k_match_features_lds", "n", M), (fx, "k_extract_tethered_lds", "work", X)):
        for m in re.finditer(kern + r"<(\d+)>, dim3\(cr_grid\(%s, (\d+), (\d+)u(?: \* (\d+)u)?\)\), dim3\((\d+)\)" % var, text):
            assert m.group(1) == m.group(2) == m.group(5)
            k[kern, int(m.group(1))] = int(m.group(3)) * int(m.group(4) or 1)
        if (kern, 256) not in k or (kern, 1024) not in k:
            raise RuntimeError("feature_cases: the launches of %s not found in %s" % (kern, where))
    m = _find(fx, r"k_feature_counts, dim3\(cr_grid\(n, (\d+) \* (\d+), (\d+)u \* (\d+)u\)\), dim3\((\d+)\)", "the launch of k_feature_counts", X)
    k["FC_PER_BLOCK"], k["FC_GRID"], k["FC_THREADS"] = int(m.group(1)) * int(m.group(2)), int(m.group(3)) * int(m.group(4)), int(m.group(5))
    # the switches of crgpu_match_features_dev
    _find(fm, r"P\.n <= FM_MAX_FEATURES && \(uintptr_t\)d_qualn % 4 == 0 && !getenv\(\"CRGPU_FEATURES_GLOBAL\"\)", "the LDS condition", M)
    k["FM_SMALL"] = int(_find(fm, r"if \(P\.n <= (\d+)u\) \{", "the 256 / 1024 thread switch", M).group(1))
    k["SLOTS_MIN"] = int(_find(fm, r"uint32_t slots = (\d+);\s*while \(slots < 2u \* P\.n\) slots <<= 1;", "the slot rule", M).group(1))
    assert k["SLOTS_MIN"] == int(_find(fx, r"uint32_t slots = (\d+);\s*while \(slots < 2u \* X\.t_n_feat\) slots <<= 1;", "the slot rule", X).group(1))
    # ... and of crgpu_extract_features_dev
    k["FXT_MAX_FEATURES"] = int(_find(fx, r"X\.one_tethered && X\.t_n_feat <= (\d+)u && !X\.t_has_empty_key && !getenv\(\"CRGPU_FEATURES_GLOBAL\"\)",
                                      "the LDS condition", X).group(1))
    k["FXT_SMALL"] = int(_find(fx, r"if \(X\.t_n_feat <= (\d+)u\) \{", "the 256 / 1024 thread switch", X).group(1))
    assert k["FXT_SMALL"] == int(_find(fx, r"const bool halves = X\.has_dist && X\.t_n_feat <= (\d+)u && X\.t_L >= 2;", "the halves rule", X).group(1))
    m = _find(fx, r"aligned && win_dw >= 1 && win_dw <= (\d+)u && R\.stride >= 4 && X\.t_pre_len \+ X\.t_suf_len <= (\d+)u", "the window condition", X)
    k["WIN_DW_MAX"], k["PAT_MAX"] = int(m.group(1)), int(m.group(2))
    m = _find(fx, r"#define FXT_LDS_BYTES \((\d+)u \* (\d+)u - (\d+)u\)", "FXT_LDS_BYTES", X)
    k["FXT_LDS_BYTES"] = int(m.group(1)) * int(m.group(2)) - int(m.group(3))
    _find(fx, r"\? \(size_t\)slots \* 12 \+ \(halves \? \(size_t\)X\.t_n_feat \* 24 : 0\) \+ \(size_t\)4 \* 64 \* \(win_dw \| 1u\) \* 4 \+ 8 \+ 2 \* 256 \* sizeof\(FxtPending\)\s*"
              r": \(size_t\)slots \* 12 \+ \(size_t\)16 \* 64 \* \(win_dw \| 1u\) \* 4 \+ 8 \+ 2 \* 1024 \* sizeof\(FxtPending\);", "the LDS need of the tethered kernel", X)
    _find(fx, r"struct FxtPending \{\s*unsigned long long key;\s*uint32_t i_lo, i_hi, start, npos;", "FxtPending (24 bytes)", X)
    _find(fx, r"X\.t_pre_len \+ X\.t_suf_len <= \d+u && lds <= FXT_LDS_BYTES\)", "the LDS limit in the window condition", X)
    k["QUAD_MIN_STRIDE"] = int(_find(fx, r"if \(R\.stride >= (\d+)\) \{", "the quad condition", X).group(1))
    _find(fx, r"P\.prefetch = P\.quad_lanes == 1u \|\| P\.quad_lanes == 2u;", "the prefetch rule", X)
    _find(fx, r"P\.pitch = win_dw \| 1u;", "the pitch", X)
    _find(fx, r"if \(X\.t_pre_dots\) win_lo = X\.t_pre_len & ~3u;", "win_lo of a wildcard prefix", X)
    _find(fx, r"else if \(X\.t_anchor3 && !R\.len && need <= R\.stride\) win_lo = \(R\.stride - need\) & ~3u;", "win_lo of a 3' anchor", X)
    _find(fx, r"win_hi = std::min\(R\.stride, \(need \+ 3u\) & ~3u\);", "win_hi of a 5' anchor", X)
    k["REC_MIN_N"] = int(_find(fx, r"!X\.has_dist && !resume\.valid && n >= (\d+);", "the smallest recording call", X).group(1))
    m = _find(fx, r"rec_cap = n / (\d+) \+ (\d+);", "rec_cap", X)
    k["REC_DIV"], k["REC_ADD"] = int(m.group(1)), int(m.group(2))
    return k


K = _read_constants()
FX_LOCAL_ENTRIES, FXT_MAXC, FM_MAX_FEATURES, FXT_MAX_FEATURES = K["FX_LOCAL_ENTRIES"], K["FXT_MAXC"], K["FM_MAX_FEATURES"], K["FXT_MAX_FEATURES"]
FC_SLOTS, FC_FILL, FC_PROBES = K["FC_SLOTS"], K["FC_FILL"], K["FC_PROBES"]
FM_SMALL, FXT_SMALL, REC_MIN_N = K["FM_SMALL"], K["FXT_SMALL"], K["REC_MIN_N"]
# reads one sweep of the grid takes: a workgroup sees a second batch only in a longer call
N_GRID = {(kern, t): t * K[kern, t] for kern in ("k_match_features_lds", "k_extract_tethered_lds") for t in (256, 1024)}


def cr_grid(n, block, cap):
    return max(1, min((n + block - 1) // block, cap))


def rec_cap(n):
    return n // K["REC_DIV"] + K["REC_ADD"]


def slots_for(n_feat):
    s = K["SLOTS_MIN"]
    while s < 2 * n_feat:
        s <<= 1
    return s


def fm_hash(key, mask):
    return (((key * K["FM_MUL"]) & M32) >> K["FM_SHIFT"]) & mask


def fxt_hash(key, mask):
    return (((key * K["FXT_MUL"]) & M64) >> K["FXT_SHIFT"]) & mask


def fc_hash(f):
    return ((f * K["FC_MUL"]) & M32) >> K["FC_SHIFT"]


# ---- sequences ----------------------------------------------------------------------------------------------------------
_DIGITS = bytes.maketrans(b"ACGTN", b"01230")


def B(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def key_of(s):
    """packed value of a sequence, first base in the most significant pair; N packs as A"""
    return int(B(s).translate(_DIGITS), 4)


def seq_of(key, L):
    return bytes(ACGT[(key >> (2 * (L - 1 - j))) & 3] for j in range(L))


def with_base(seq, pos, base):
    s = bytearray(B(seq))
    s[pos] = base if isinstance(base, int) else ord(base)
    return bytes(s)


def other(seq, pos, k=1):
    """seq with the base at pos replaced by the k-th next one"""
    seq = B(seq)
    return with_base(seq, pos, ACGT[(ACGT.index(seq[pos]) + k) & 3])


def neighbours(seq):
    """the 3 L sequences one substitution away, in position-major A<C<G<T order"""
    seq = B(seq)
    return [with_base(seq, p, b) for p in range(len(seq)) for b in ACGT if b != seq[p]]


def hamming(a, b):
    return sum(1 for x, y in zip(B(a), B(b)) if x != y)


def random_seq(rng, L):
    return bytes(ACGT[k] for k in rng.integers(0, 4, L))


def far_seqs(k, L, rng, min_dist, avoid=()):
    """k sequences of L bases at pairwise Hamming distance >= min_dist, and as far from `avoid`"""
    out = [B(a) for a in avoid]
    n0 = len(out)
    tries = 0
    while len(out) < k + n0:
        c = random_seq(rng, L)
        tries += 1
        if tries > 200000:
            raise RuntimeError("feature_cases: no %d sequences of %d bases %d apart" % (k, L, min_dist))
        if all(hamming(c, o) >= min_dist for o in out):
            out.append(c)
    return out[n0:]


# ---- the reference, restated --------------------------------------------------------------------------------------------
def p_edit(q):
    """feature_extraction.rs:43-45: qv = min(qual - 33, 33) in u8 arithmetic"""
    qv = min((int(q) - 33) & 0xFF, FEATURE_MAX_QV)
    return 10.0 ** (-float(qv) / 10.0)


def _confident(mx, total):
    """(mx / total) >= FEATURE_CONF_THRESHOLD in IEEE doubles: x / 0 is an infinity of x's sign, 0 / 0 is NaN"""
    if total == 0.0:
        return mx > 0.0
    return (mx / total) >= FEATURE_CONF_THRESHOLD


def compute_feature_dist(counts, types=None):
    """compute_feature_dist (feature_checker.rs:8-50): proportions within a feature type; all zero: uniform over all features"""
    types = [0] * len(counts) if types is None else [int(t) for t in types]
    total = {}
    for c, t in zip(counts, types):
        total[t] = total.get(t, 0) + int(c)
    d = [float(int(c)) / float(total[t]) if total[t] > 0 else 0.0 for c, t in zip(counts, types)]
    if all(x == 0.0 for x in d):
        d = [1.0 / float(len(d))] * len(d)
    return d


def correct_feature_barcode(caps, feats, dist, info=None):
    """correct_feature_barcode (:34-117).  caps: [(sequence, qualities)]; feats: {sequence: feature index}.  Returns
    (number of the capture, whitelist sequence) or None."""
    wl = {}          # whitelist_likelihoods: sequence -> [likelihood, capture]
    total = 0.0

    def insert_hit(like, test_seq, c):
        nonlocal total
        e = wl.get(test_seq)
        if e is not None:
            if like > e[0]:
                old = e[0]
                e[0], e[1] = like, c
                total += like - old
        else:
            wl[test_seq] = [like, c]
            total += like

    for c, (seq, qual) in enumerate(caps):
        f = feats.get(seq)
        if f is not None:
            insert_hit(dist[f], seq, c)
            continue
        t = bytearray(seq)
        for i in range(len(t)):
            orig = t[i]
            for base in ACGT:
                if base != orig:
                    t[i] = base
                    f = feats.get(bytes(t))
                    if f is not None:
                        insert_hit(dist[f] * p_edit(qual[i]), bytes(t), c)
            t[i] = orig
    mx, best = -1.0, None
    for s, (like, c) in wl.items():      # (two equal maxima give a ratio of at most one half: the order cannot decide)
        if like > mx:
            mx, best = like, (c, s)
    if info is not None:
        info["map"] = len(wl)
    return best if _confident(mx, total) else None


def find_closest(caps, feats, dist, info=None):
    """find_closest (:443-470)"""
    if not caps:
        return None
    if len(caps) == 1 and caps[0][0] in feats:
        return 0, caps[0][0]
    if dist is not None:
        return correct_feature_barcode(caps, feats, dist, info)
    return None


def compile_pattern(orig, L):
    """compile_pattern (:306-342): the regular expression as the reference writes it, None for a rejected pattern"""
    pat = re.sub(r"^5[Pp]?[-_]?", "^", orig, count=1)
    pat = re.sub(r"[-_]?3[Pp]?$", "$", pat, count=1)
    check = pat.replace("(BC)", "", 1)
    if not re.match(r"^\^?[ACGTN]*\$?$", check) or orig.count("(BC)") != 1:
        return None
    return pat.replace("N", ".").replace("(BC)", "(.{%d,%d})" % (L, L), 1)


def compile_bare_patterns(seqs):
    """compile_bare_patterns (:291-304)"""
    return "(" + "|".join(s[:i] + "." + s[i + 1:] for s in seqs for i in range(len(s))) + ")"


class Pattern:
    def __init__(self, read, regex_str, tethered, L):
        self.read, self.regex_str, self.tethered, self.L = read, regex_str, tethered, L
        py = regex_str[:-1] + r"\Z" if regex_str.endswith("$") else regex_str
        self.rx = re.compile(py.encode(), re.S)
        self.feats = {}

    @property
    def least(self):
        return min(self.feats.values())


class Extractor:
    """FeatureExtractor of one feature type (:183-266): defs = [(pattern, sequence, index, read)]"""

    def __init__(self, defs, dist=None):
        self.dist = dist
        pats, bare = {}, {}
        for pattern, seq, index, read in defs:
            assert re.match(r"^[ACGTN]+$", seq)
            if pattern == "(BC)":
                bare.setdefault((read, len(seq)), []).append((seq, index))
                continue
            rs = compile_pattern(pattern, len(seq))
            assert rs is not None, pattern
            p = pats.setdefault((read, rs), Pattern(read, rs, True, len(seq)))
            assert B(seq) not in p.feats
            p.feats[B(seq)] = index
        for (read, L), fds in bare.items():
            rs = compile_bare_patterns([s for s, _ in fds])
            p = pats.setdefault((read, rs), Pattern(read, rs, False, L))
            for s, index in fds:
                assert B(s) not in p.feats
                p.feats[B(s)] = index
        self.patterns = list(pats.values())

    def match_read(self, r1=None, q1=None, r2=None, q2=None, info=None):
        """match_read (:358-445) -> (feature where ids holds one id else NO_FEATURE, ids.len(), the span of
        FeatureData::barcode as crgpu.h packs it).  info: a list that receives one dict per pattern with captures"""
        wl, pm = [], []
        for pat in self.patterns:
            s, q = (r1, q1) if pat.read == 0 else (r2, q2)
            if s is None:
                continue
            caps, offset = [], 0
            while offset <= len(s):
                m = pat.rx.search(s[offset:])
                if not m:
                    break
                a, b = m.start(1) + offset, m.end(1) + offset
                caps.append((s[a:b], q[a:b], a))
                offset += m.start(1) + 1        # "just after this match" (:392-394)
                if pat.tethered:
                    break
            if not caps:
                continue
            d = dict(pattern=pat, starts=[c[2] for c in caps], map=0)
            hit = find_closest([(c[0], c[1]) for c in caps], pat.feats, self.dist, d)
            d["hit"] = hit
            if info is not None:
                info.append(d)
            if hit is not None:
                wl.append((pat.L, pat.feats[hit[1]], caps[hit[0]][2], pat.read))
            else:
                for c in caps:
                    pm.append((len(c[0]), pat.least, c[2], pat.read))
        best = None
        for x in wl or pm:                       # max_by_key((len, Reverse(index))) keeps the last of equal keys
            if best is None or (x[0], -x[1]) >= (best[0], -best[1]):
                best = x
        if best is None:
            return NO_FEATURE, 0, NO_CAPTURE
        span = (best[3] << 30) | (best[2] << 8) | best[0]
        if wl:
            return (wl[0][1] if len(wl) == 1 else NO_FEATURE), len(wl), 0x80000000 | span
        return NO_FEATURE, 0, span


# ---- group A: pre-cut captures ------------------------------------------------------------------------------------------
EXACT, PENDING, NOTHING = 0, 1, 2     # what a read is to an LDS kernel: answered at once, queued for the posterior, or neither


class MatchCase:
    """crgpu_match_features_dev: feats (ASCII, in definition order) with their indices and counts (None: no distribution);
    the distinct captures (sequence with N, L quality bytes) and `which`: the distinct capture every read repeats.
    offset: bytes the quality array is shifted from a dword boundary."""
    group = "A"

    def __init__(self, name, L, feats, index, counts, rows, which, offset=0):
        self.name, self.L, self.offset = name, L, offset
        self.feats, self.index = [B(f) for f in feats], np.asarray(index, np.uint32)
        assert len(set(self.feats)) == len(self.feats) == len(self.index) and all(len(f) == L for f in self.feats)
        self.counts = counts
        self.dist = None if counts is None else compute_feature_dist(counts)
        self.rows = [(B(s), bytes(bytearray(q))) for s, q in rows]
        assert all(len(s) == L and len(q) == L for s, q in self.rows)
        self.which = np.asarray(which, np.int64)
        self.n = len(self.which)
        self.claims, self.tags = [], {}
        self._d = self._e = None

    def arrays(self):
        """(packed captures, quality bytes with bit 7 = N) as crgpu_pack_dev makes them"""
        key = np.array([key_of(s) for s, _ in self.rows], np.uint32)
        qn = np.array([[q[j] | (0x80 if s[j] not in ACGT else 0) for j in range(self.L)] for s, q in self.rows], np.uint8).reshape(len(self.rows), self.L)
        return key[self.which], qn[self.which]

    def row_expected(self):
        pos = {f: k for k, f in enumerate(self.feats)}
        out = []
        for s, q in self.rows:
            hit = find_closest([(s, q)], pos, self.dist)
            out.append(NO_FEATURE if hit is None else int(self.index[pos[hit[1]]]))
        return np.array(out, np.uint32)

    def expected(self):
        if self._e is None:
            self._e = self.row_expected()[self.which]
        return self._e


class Described:
    pass


def _queue(counts, threads):
    """the pending-capture queue of one workgroup over its batches: (captures waiting after each batch's drain, drains)"""
    left, kept, drains = 0, [], 0
    for c in counts:
        left += int(c)
        assert left < 2 * threads
        if left >= threads:
            left -= threads
            drains += 1
        kept.append(left)
    return kept, drains


def _batches(state_of_read, n, threads, grid):
    """pending captures per (workgroup, batch) of a grid-stride LDS kernel"""
    tile = np.arange(n) // threads
    n_batch = (int(tile[-1]) // grid) + 1
    out = np.zeros((grid, n_batch), np.int64)
    np.add.at(out, (tile % grid, tile // grid), state_of_read == PENDING)
    return out


def _describe_match(case, env_global=False):
    d = Described()
    nf = len(case.feats)
    d.n_feat, d.slots = nf, slots_for(nf)
    if nf > FM_MAX_FEATURES or case.offset % 4 or env_global:
        d.kernel, d.threads = "global", 256
    else:
        d.kernel, d.threads = ("lds256", 256) if nf <= FM_SMALL else ("lds1024", 1024)
    d.tail = (case.n * case.L) % 4
    member = set(case.feats)
    d.state, d.n_cand, d.n_n = [], [], []
    for s, q in case.rows:
        n_n = sum(1 for b in s if b not in ACGT)
        cand = [t for t in (neighbours(s) if n_n == 0 else [with_base(s, p, b) for p in range(case.L) if s[p] not in ACGT for b in ACGT])
                if t in member] if n_n <= 1 else []
        exact = n_n == 0 and s in member
        d.state.append(EXACT if exact else PENDING if (case.dist is not None and n_n <= 1) else NOTHING)
        d.n_cand.append(0 if exact else len(cand))
        d.n_n.append(n_n)
    d.state, d.n_cand, d.n_n = np.array(d.state), np.array(d.n_cand), np.array(d.n_n)
    if d.kernel != "global":
        d.grid = cr_grid(case.n, d.threads, K["k_match_features_lds", d.threads])
        d.pending = _batches(d.state[case.which], case.n, d.threads, d.grid)
        d.batches = d.pending.shape[1]
    d.last_slot = sum(1 for f in case.feats if fm_hash(key_of(f), d.slots - 1) == d.slots - 1)
    return d


# ---- groups B and C: read rows ------------------------------------------------------------------------------------------
class Rows:
    """distinct rows of one read: sequence and quality bytes of `stride` bytes each (zero behind what was given) and, unless
    every row is full, the length the call is told"""

    def __init__(self, stride, with_len=True):
        self.stride, self.with_len = stride, with_len
        self.seq, self.qual, self.len = [], [], []

    def add(self, seq, qual=None, length=None):
        """qual: None (Q0 everywhere), one value, or one per base.  length: what d_len says; the bytes behind it stay in the row"""
        seq = B(seq)
        assert len(seq) <= self.stride
        if qual is None or isinstance(qual, int):
            qual = [Q0 if qual is None else qual] * len(seq)
        assert len(qual) == len(seq)
        if not self.with_len:
            assert len(seq) == self.stride and length is None
        self.seq.append(seq + bytes(self.stride - len(seq)))
        self.qual.append(bytes(bytearray(qual)) + bytes(self.stride - len(seq)))
        self.len.append(len(seq) if length is None else length)
        return len(self.seq) - 1

    def read(self, k):
        ln = min(self.len[k], self.stride) if self.with_len else self.stride
        return self.seq[k][:ln], self.qual[k][:ln]

    def arrays(self, which):
        s = np.frombuffer(b"".join(self.seq), np.uint8).reshape(len(self.seq), self.stride)
        q = np.frombuffer(b"".join(self.qual), np.uint8).reshape(len(self.qual), self.stride)
        ln = np.array(self.len, np.uint32)[which] if self.with_len else None
        return np.ascontiguousarray(s[which]), np.ascontiguousarray(q[which]), ln


class ExtractCase:
    """crgpu_extract_features_dev: defs = [(pattern, sequence, index, read)], counts per feature index (the distribution is
    compute_feature_dist of them; the runs without one drop it), r1 / r2: Rows or None, which: the distinct row every read
    repeats.  group "B": one tethered pattern; "C": the generic kernel."""

    def __init__(self, name, group, defs, counts, r1, r2, which):
        self.name, self.group, self.defs = name, group, list(defs)
        self.counts = list(counts)
        assert max(d[2] for d in defs) < len(self.counts)
        self.dist = compute_feature_dist(self.counts)
        self.r1, self.r2 = r1, r2
        self.which = np.asarray(which, np.int64)
        self.n = len(self.which)
        self.n_rows = len((r1 or r2).seq)
        assert r1 is None or r2 is None or len(r1.seq) == len(r2.seq)
        self.claims, self.tags = [], {}
        self._x, self._e, self._i = {}, {}, {}

    def extractor(self, with_dist=True):
        if with_dist not in self._x:
            self._x[with_dist] = Extractor(self.defs, self.dist if with_dist else None)
        return self._x[with_dist]

    def row_reads(self, k):
        a = self.r1.read(k) if self.r1 else (None, None)
        b = self.r2.read(k) if self.r2 else (None, None)
        return a[0], a[1], b[0], b[1]

    def row_expected(self, with_dist=True):
        """(feature, n_ids, capture) of every distinct row, and what the restatement saw on the way"""
        if with_dist not in self._e:
            x = self.extractor(with_dist)
            out, infos = np.zeros((self.n_rows, 3), np.uint32), []
            for k in range(self.n_rows):
                info = []
                out[k] = x.match_read(*self.row_reads(k), info=info)
                infos.append(info)
            self._e[with_dist], self._i[with_dist] = out, infos
        return self._e[with_dist]

    def row_info(self, with_dist=True):
        self.row_expected(with_dist)
        return self._i[with_dist]

    def expected(self, with_dist=True):
        e = self.row_expected(with_dist)[self.which]
        return e[:, 0].copy(), e[:, 1].copy(), e[:, 2].copy()


def _tethered_parts(regex_str):
    """(anchor5, prefix, suffix, anchor3) of a tethered expression, '.' = any"""
    m = re.match(r"^(\^?)([ACGT.]*)\(\.\{\d+,\d+\}\)([ACGT.]*)(\$?)$", regex_str)
    assert m, regex_str
    return bool(m.group(1)), m.group(2), m.group(3), bool(m.group(4))


def dispatch(case, with_dist=True, env_global=False):
    """what crgpu_extract_features_dev decides from the extractor and the rows: the kernel and, for the LDS kernel, the staged
    window, its load plan and the needle of a floating pattern"""
    x = case.extractor(with_dist)
    d = dict(kernel="generic")
    if len(x.patterns) != 1 or not x.patterns[0].tethered:
        return d
    p = x.patterns[0]
    a5, pre, suf, a3 = _tethered_parts(p.regex_str)
    R = case.r2 if p.read else case.r1
    need = len(pre) + p.L + len(suf)
    nf = len(p.feats)
    d.update(anchor5=a5, anchor3=a3, pre=pre, suf=suf, need=need, L=p.L, n_feat=nf, read=p.read, stride=R.stride)
    pre_dots, suf_dots = pre.strip(".") == "", suf.strip(".") == ""
    empty_key = any(len(f) == 32 and key_of(f) == M64 for f in p.feats)
    d.update(empty_key=empty_key)
    if nf > FXT_MAX_FEATURES or empty_key or env_global:
        return d
    win_lo, win_hi = 0, R.stride
    if a5:
        win_hi = min(R.stride, (need + 3) & ~3)
        if pre_dots:
            win_lo = len(pre) & ~3
    elif a3 and not R.with_len and need <= R.stride:
        win_lo = (R.stride - need) & ~3
    win_dw = ((win_hi - win_lo) & M32) // 4
    threads = 256 if nf <= FXT_SMALL else 1024
    halves = with_dist and nf <= FXT_SMALL and p.L >= 2
    # what the workgroup needs of LDS: the set, the half tables, the row windows of its waves, the queue of 2 * threads captures
    lds = slots_for(nf) * 12 + (nf * 24 if halves else 0) + (threads // 64) * 64 * (win_dw | 1) * 4 + 8 + 2 * threads * 24
    d.update(lds=lds)
    if not (R.stride % 4 == 0 and 1 <= win_dw <= K["WIN_DW_MAX"] and R.stride >= 4 and len(pre) + len(suf) <= K["PAT_MAX"] and lds <= K["FXT_LDS_BYTES"]):
        return d
    quad_lanes = 0
    if R.stride >= K["QUAD_MIN_STRIDE"]:
        quad_lanes = 1
        while quad_lanes < (win_dw + 3) // 4:
            quad_lanes <<= 1
    src = suf if (suf and suf[0] != ".") else pre
    needle_len = 0
    if src and src[0] != "." and not a5 and not a3:
        while needle_len < 4 and needle_len < len(src) and src[needle_len] != ".":
            needle_len += 1
    # a quad that would run past its row starts earlier: its leading dwords then lie in front of the window
    q_stride_dw, q_lo_dw, quads = R.stride // 4, win_lo // 4, (win_dw + 3) // 4
    early = quad_lanes != 0 and any(q_lo_dw + 4 * c + 4 > q_stride_dw and q_stride_dw - 4 < q_lo_dw for c in range(quads))
    d.update(kernel="lds%d" % threads, threads=threads, win_lo=win_lo, win_dw=win_dw, quad_lanes=quad_lanes,
             prefetch=quad_lanes in (1, 2), pitch=win_dw | 1, needle_len=needle_len,
             needle_off=(len(pre) + p.L if src is suf and needle_len else 0), halves=halves,
             slots=slots_for(nf), quad_in_front=early, grid_cap=K["k_extract_tethered_lds", threads])
    return d


def _describe_extract(case, with_dist=True, env_global=False, recording=False):
    """recording: a call without a distribution that keeps its captures for the one with (two-pass flow)"""
    d = Described()
    d.dispatch = dispatch(case, with_dist, env_global)
    d.kernel = d.dispatch["kernel"]
    infos = case.row_info(with_dist)
    exp = case.row_expected(with_dist)
    x = case.extractor(with_dist)
    d.n_caps = np.array([sum(len(i["starts"]) for i in info) for info in infos])
    # the widest map a pattern of the read fills: the generic kernel redoes the read when one outgrows its local array
    d.map = np.array([max([i["map"] for i in info] or [0]) for info in infos])
    d.requeued = int((d.map[case.which] > FX_LOCAL_ENTRIES).sum()) if with_dist else 0
    if d.kernel != "generic":
        p = x.patterns[0]
        state, n_cand, start = [], [], []
        for k, info in enumerate(infos):
            if not info:
                state.append(NOTHING), n_cand.append(0), start.append(-1)
                continue
            st = info[0]["starts"][0]
            s = (case.row_reads(k)[2 if p.read else 0])[st:st + p.L]
            n_n = sum(1 for b in s if b not in ACGT)
            exact = s in p.feats
            cand = [t for t in (neighbours(s) if n_n == 0 else [with_base(s, j, b) for j in range(p.L) if s[j] not in ACGT for b in ACGT])
                    if t in p.feats] if n_n <= 1 else []
            state.append(EXACT if exact else PENDING if ((with_dist or recording) and n_n <= 1) else NOTHING)
            n_cand.append(0 if exact else len(cand))
            start.append(st)
        d.state, d.n_cand, d.start = np.array(state), np.array(n_cand), np.array(start)
        t = d.dispatch["threads"]
        d.grid = cr_grid(case.n, t, d.dispatch["grid_cap"])
        d.pending = _batches(d.state[case.which], case.n, t, d.grid)
        d.batches = d.pending.shape[1]
        d.n_pending = int(d.pending.sum())
        d.last_slot = sum(1 for f in p.feats if fxt_hash(key_of(f), d.dispatch["slots"] - 1) == d.dispatch["slots"] - 1)
    d.exp = exp
    return d


# ---- group D: feature counts --------------------------------------------------------------------------------------------
class CountCase:
    group = "D"

    def __init__(self, name, feature, n_features, counts_in=None):
        self.name, self.n_features = name, n_features
        self.feature = np.ascontiguousarray(feature, np.uint32)
        self.n = len(self.feature)
        self.counts_in = np.zeros(n_features, np.int64) if counts_in is None else np.asarray(counts_in, np.int64)
        self.claims = []

    def expected(self):
        f = self.feature[self.feature < self.n_features].astype(np.int64)
        return self.counts_in + np.bincount(f, minlength=self.n_features)


def _describe_counts(case):
    """per workgroup of k_feature_counts: the distinct features it sees, and whether some feature must find its 16 probes taken"""
    d = Described()
    T = K["FC_THREADS"]
    d.grid = cr_grid(case.n, K["FC_PER_BLOCK"], K["FC_GRID"])
    f = case.feature
    pad = (-case.n) % (d.grid * T)
    g = np.concatenate([f, np.full(pad, NO_FEATURE, np.uint32)]).reshape(-1, d.grid, T).transpose(1, 0, 2).reshape(d.grid, -1)
    g = np.sort(g, axis=1)
    ok = g < case.n_features
    d.distinct = (ok & np.concatenate([np.ones((d.grid, 1), bool), g[:, 1:] != g[:, :-1]], axis=1)).sum(axis=1)
    # a feature is surely counted in global memory when more features of its workgroup want one of the FC_PROBES slots it can
    # reach than there are such slots; here: more than FC_PROBES features of one workgroup share one home slot
    d.same_home = 0
    for b in range(min(d.grid, 4)):
        u = np.unique(g[b][ok[b]])
        if len(u):
            h = ((u.astype(np.uint64) * np.uint64(K["FC_MUL"])) & np.uint64(M32)) >> np.uint64(K["FC_SHIFT"])
            d.same_home = max(d.same_home, int(np.bincount(h.astype(np.int64)).max()))
    return d


def describe(case, **kw):
    if isinstance(case, MatchCase):
        return _describe_match(case, **kw)
    if isinstance(case, CountCase):
        return _describe_counts(case)
    return _describe_extract(case, **kw)


# ---- claims -------------------------------------------------------------------------------------------------------------
def check_claims(case, **kw):
    """assert every claim of the case against describe(); returns the description"""
    d = describe(case, **kw)
    for c in case.claims:
        kind, what = c["kind"], "%s: %r" % (case.name, c)
        if c.get("queued") and not (kw.get("with_dist", True) or kw.get("recording", False)):
            continue      # a claim about the runs that queue captures: with a distribution, or recording for the run that has one
        if "with_dist" in c and c["with_dist"] != kw.get("with_dist", True):
            continue      # a claim about another run of the case
        if kw.get("env_global") and kind in ("kernel", "dispatch", "states", "batches", "pending_plan", "pending_total", "rows_in_batch",
                                             "no_nothing", "last_slot", "slots", "n_cand_occurs", "records"):
            continue      # a claim about the LDS kernel, which this run does not take
        if kind == "kernel":
            assert d.kernel == c["kernel"], what
        elif kind == "dispatch":
            for k, v in c["values"].items():
                assert d.dispatch.get(k) == v, (what, k, d.dispatch.get(k))
        elif kind == "tail":
            assert d.tail == c["tail"], what
        elif kind == "states":          # every listed state occurs among the reads
            assert d.kernel != "generic" and set(c["states"]) <= set(d.state[case.which].tolist()), (what, set(d.state.tolist()))
        elif kind == "row":             # one tagged row
            k = case.tags[c["tag"]]
            if not hasattr(d, "state"):      # the generic kernel: what a read is to the LDS kernel's queue does not apply
                c = {x: v for x, v in c.items() if x not in ("state", "n_cand", "start")}
            if "state" in c:
                assert d.state[k] == c["state"], (what, d.state[k])
            if "n_cand" in c:
                assert d.n_cand[k] == c["n_cand"], (what, d.n_cand[k])
            if "start" in c:
                assert d.start[k] == c["start"], (what, d.start[k])
            if "n_caps" in c:
                assert d.n_caps[k] == c["n_caps"], (what, d.n_caps[k])
            if "map" in c:
                assert d.map[k] == c["map"], (what, d.map[k])
            if "feature" in c:
                assert _row_feature(case, k, kw) == c["feature"], (what, _row_feature(case, k, kw))
            if "capture" in c:
                got = int(d.exp[k][2])
                assert got == c["capture"], (what, hex(got))
        elif kind == "batches":
            assert d.batches == c["batches"], (what, d.batches)
        elif kind == "pending_plan":    # pending captures of a workgroup per batch, and what that does to its queue
            got = d.pending[c["block"]].tolist()
            assert got == c["counts"], (what, got)
            kept, drains = _queue(got, d.threads if isinstance(case, MatchCase) else d.dispatch["threads"])
            assert kept == c["kept"] and drains == c["drains"], (what, kept, drains)
        elif kind == "pending_total":
            assert int(d.pending.sum()) == c["total"], (what, int(d.pending.sum()))
        elif kind == "rows_in_batch":   # reads of a workgroup's batch
            t = d.threads if isinstance(case, MatchCase) else d.dispatch["threads"]
            first = (c["batch"] * d.grid + c["block"]) * t
            assert max(0, min(case.n - first, t)) == c["rows"], what
        elif kind == "no_nothing":      # apart from the planned pending captures every read is answered at once
            assert not (d.state[case.which] == NOTHING).any(), what
        elif kind == "last_slot":       # features whose home is the last slot of the set: the probe sequence wraps
            assert d.last_slot >= c["at_least"], (what, d.last_slot)
        elif kind == "slots":
            got = d.slots if isinstance(case, MatchCase) else d.dispatch["slots"]
            assert got == c["slots"], (what, got)
        elif kind == "n_cand_occurs":
            assert set(c["values"]) <= set(d.n_cand[d.state == PENDING].tolist()), (what, sorted(set(d.n_cand.tolist())))
        elif kind == "both_sides":      # among the tagged rows some are corrected and some are not
            got = [_row_feature(case, case.tags[t], kw) != NO_FEATURE for t in c["tags"]]
            assert any(got) and not all(got), (what, got)
        elif kind == "map_occurs":
            assert set(c["values"]) <= set(d.map.tolist()), (what, sorted(set(d.map.tolist())))
        elif kind == "requeued":
            assert d.requeued == c["count"], (what, d.requeued)
        elif kind == "records":         # captures a recording call keeps
            assert d.n_pending == c["count"], (what, d.n_pending)
        elif kind == "distinct_per_block":
            assert int(d.distinct.min()) > c["more_than"], (what, int(d.distinct.min()))
        elif kind == "same_home":
            assert d.same_home > c["more_than"], (what, d.same_home)
        elif kind == "grid":
            assert d.grid == c["grid"], (what, d.grid)
        else:
            raise AssertionError("unknown claim %r" % (c,))
    return d


def _row_feature(case, k, kw):
    if isinstance(case, MatchCase):
        return int(case.row_expected()[k])
    return int(case.row_expected(kw.get("with_dist", True))[k][0])


# ---- building blocks ----------------------------------------------------------------------------------------------------
def split_positions(L):
    """position 0, both sides of the half split (the last half holds L >> 1 bases), the last position"""
    h = L - (L >> 1)
    return sorted(set(p for p in (0, h - 1, h, L - 1) if 0 <= p < L))


def q_at(L, **kw):
    q = [Q0] * L
    for k, v in kw.items():
        q[int(k[1:])] = v
    return q


def random_feats(rng, L, k):
    """k distinct sequences of L bases (at most five eighths of all there are)"""
    k = max(1, min(k, 4 ** L * 5 // 8))
    keys = set()
    while len(keys) < k:
        keys.update(int(x) for x in rng.integers(0, 4 ** L, 2 * (k - len(keys)), dtype=np.uint64))
        while len(keys) > k:
            keys.pop()
    return [seq_of(x, L) for x in sorted(keys)]


def capture_variants(L, feats, rng):
    """captures around a feature list: exact ones; one substitution and one N at position 0, on both sides of the half split
    and at the last position; an N where the feature has an A; two Ns; an N and a substitution; every edge quality under one
    substitution; noise.  -> [(tag, sequence, qualities)]"""
    member, out = set(feats), []
    qs = EDGE_QUALS + (40, 50)
    nq = [0]

    def nextq():
        nq[0] += 1
        return qs[nq[0] % len(qs)]
    out.append(("exact_first", feats[0], [Q0] * L))
    out.append(("exact_last", feats[-1], [nextq()] * L))
    for j, p in enumerate(split_positions(L)):
        f = feats[(1 + j) % len(feats)]
        for k in (1, 2, 3):
            if other(f, p, k) not in member:
                out.append(("mm_p%d" % p, other(f, p, k), q_at(L, **{"p%d" % p: nextq()})))
                break
        out.append(("n_p%d" % p, with_base(f, p, "N"), q_at(L, **{"p%d" % p: nextq()})))
    for f in feats:
        if ord("A") in f:
            p = f.index(b"A")
            out.append(("n_on_a", with_base(f, p, "N"), q_at(L, **{"p%d" % p: nextq()})))
            break
    if L >= 2:
        out.append(("two_n", with_base(with_base(feats[0], 0, "N"), L - 1, "N"), [Q0] * L))
        out.append(("n_and_mm", with_base(other(feats[0], L - 1), 0, "N"), [nextq()] * L))
    f, p = feats[len(feats) // 2], L // 2
    for q in EDGE_QUALS:
        out.append(("q%d" % q, other(f, p, 1 + q % 3), q_at(L, **{"p%d" % p: q})))
    out.append(("noise", random_seq(rng, L), [int(x) for x in rng.integers(33, 75, L)]))
    return out


def posterior_set(L, rng):
    """Feature families around far-apart centres (no centre is a feature) and the captures that sit on the decisions of the
    posterior.  -> (feats, counts, [(tag, sequence, qualities)], claims about the tagged rows)"""
    C = far_seqs(40, L, rng, 5)
    nc = [0]

    def centre():
        nc[0] += 1
        return C[nc[0] - 1]
    feats, counts, rows, claims = [], [], [], []

    def add(seq, count):
        assert seq not in feats
        feats.append(seq)
        counts.append(count)
        return seq

    def row(tag, seq, qual=None, **claim):
        rows.append((tag, seq, [Q0] * L if qual is None else qual))
        if claim:
            claims.append(dict(kind="row", tag=tag, queued=True, **claim))
    # two candidates whose counts put max / sum at and next to 0.975, at equal and at different qualities
    ratio_tags = []
    for a, b in ((39, 1), (38, 1), (40, 1), (78, 2), (77, 2)):
        c = centre()
        add(other(c, 2), a), add(other(c, L - 3), b)
        row("ratio_%d_%d_eq" % (a, b), c, state=PENDING, n_cand=2)
        row("ratio_%d_%d_dq" % (a, b), c, q_at(L, p2=36, **{"p%d" % (L - 3): 37}), state=PENDING, n_cand=2)
        ratio_tags += ["ratio_%d_%d_eq" % (a, b), "ratio_%d_%d_dq" % (a, b)]
    claims.append(dict(kind="both_sides", tags=ratio_tags, with_dist=True))
    claims.append(dict(kind="both_sides", tags=[t for t in ratio_tags if t.endswith("_eq")], with_dist=True))
    # every candidate with count 0: 0 / 0
    c = centre()
    add(other(c, 1), 0), add(other(c, L - 2), 0)
    row("zero_over_zero", c, state=PENDING, n_cand=2, feature=NO_FEATURE)
    # the edge qualities: a candidate under quality q against one under the cap
    c = centre()
    add(other(c, 4), 10), add(other(c, 9), 10)
    for q in EDGE_QUALS:
        row("qual_%d" % q, c, q_at(L, p4=q, p9=66), state=PENDING, n_cand=2)
    claims.append(dict(kind="both_sides", tags=["qual_%d" % q for q in EDGE_QUALS], with_dist=True))
    # one N: at position 0, on both sides of the half split, at the last position; where the feature has an A
    f = add(centre(), 7)
    for p in split_positions(L):
        row("n_p%d" % p, with_base(f, p, "N"), q_at(L, **{"p%d" % p: 35}), state=PENDING, n_cand=1)
    fa = add(with_base(centre(), 3, "A"), 5)
    row("n_on_a", with_base(fa, 3, "N"), state=PENDING, n_cand=1)
    row("two_n", with_base(with_base(f, 1, "N"), L - 2, "N"), state=NOTHING, n_cand=0, feature=NO_FEATURE)
    row("n_and_mm", with_base(other(f, 5), 0, "N"), state=PENDING, n_cand=0, feature=NO_FEATURE)
    # four completions of one N
    c = centre()
    for k, b in enumerate(ACGT):
        add(with_base(c, 6, b), (1, 0, 900, 3)[k])
    row("n_four", with_base(c, 6, "N"), state=PENDING, n_cand=4)
    # FXT_MAXC and one more candidates; an N in such a family leaves the (at most four) candidates of its position
    for total in (FXT_MAXC, FXT_MAXC + 1):
        c = centre()
        spots = [(p, k) for p in (2, L - (L >> 1), L - 2) for k in (1, 2, 3)][:total]
        assert len(spots) == total
        for j, (p, k) in enumerate(spots):
            add(other(c, p, k), 4000 if j == total - 1 else 1)
        row("cand%d" % total, c, state=PENDING, n_cand=total)
        row("cand%d_low" % total, c, q_at(L, **{"p%d" % spots[-1][0]: 75}), state=PENDING, n_cand=total)
        cn = with_base(c, 2, "A")
        row("cand%d_n" % total, with_base(cn, 2, "N"), state=PENDING, n_cand=sum(1 for p, k in spots if p == 2))
    # features nobody is near, and exact captures
    for _ in range(6):
        add(centre(), int(rng.integers(1, 50)))
    row("exact", feats[-1], state=EXACT)
    row("exact_low_quality", feats[-2], [33] * L, state=EXACT)
    row("lone", other(feats[-3], L // 2), state=PENDING, n_cand=1)
    row("far", centre(), state=PENDING, n_cand=0, feature=NO_FEATURE)
    return feats, counts, rows, claims


# ---- group A ------------------------------------------------------------------------------------------------------------
A_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 15, 16)
A_SIZES = (1, 63, 64, 65, 255, 256, 257)


def match_case(name, L, n, n_feat, seed, with_dist=True, offset=0, kernel=None):
    rng = np.random.default_rng(seed)
    feats = random_feats(rng, L, n_feat)
    order = rng.permutation(len(feats))
    feats = [feats[k] for k in order]
    counts = [int(x) for x in rng.integers(0, 60, len(feats))] if with_dist else None
    rows = [(s, q) for _, s, q in capture_variants(L, feats, rng)]
    which = (np.arange(n) + seed) % len(rows) if n < len(rows) else np.arange(n) % len(rows)
    case = MatchCase(name, L, feats, 100 + rng.permutation(len(feats)), counts, rows, which, offset)
    case.claims.append(dict(kind="kernel", kernel=kernel or ("lds256" if len(feats) <= FM_SMALL else "lds1024")))
    case.claims.append(dict(kind="tail", tail=(n * L) % 4))
    return case


def posterior_match_case():
    L = 16
    feats, counts, rows, claims = posterior_set(L, np.random.default_rng(23))
    case = MatchCase("a_posterior", L, feats, np.arange(len(feats)) + 3, counts, [(s, q) for _, s, q in rows], np.arange(len(rows)))
    case.tags = {t: k for k, (t, _, _) in enumerate(rows)}
    case.claims = claims + [dict(kind="kernel", kernel="lds256")]
    return case


def wrap_match_case(n_feat):
    """features whose home is the last slot of the set (probing wraps to slot 0), n_feat features in all"""
    L, rng = 12, np.random.default_rng(29 + n_feat)
    slots = slots_for(n_feat)
    last = []
    key = 0
    while len(last) < 4:
        key += 1
        if fm_hash(key, slots - 1) == slots - 1:
            last.append(seq_of(key, L))
    feats = last + [f for f in random_feats(rng, L, n_feat) if f not in last][:n_feat - len(last)]
    rows = [(s, q) for _, s, q in capture_variants(L, feats, rng)]
    rows += [(f, [Q0] * L) for f in last] + [(other(f, 7), q_at(L, p7=40)) for f in last]
    case = MatchCase("a_wrap_%d" % n_feat, L, feats, np.arange(len(feats)), [3] * len(feats), rows, np.arange(len(rows)))
    case.claims += [dict(kind="last_slot", at_least=4), dict(kind="slots", slots=slots), dict(kind="kernel", kernel="lds256")]
    return case


def _plan(threads):
    """pending captures of the first workgroups in their two batches, what stays queued after each batch, and the drains inside
    the loop: drained at np == THREADS; THREADS - 1 stay and the newest THREADS go; THREADS reached by the second batch"""
    s = threads // 256
    return {0: ([threads, 0], [0, 0], 1), 1: ([threads - 1, threads], [threads - 1, threads - 1], 1), 2: ([100 * s, 156 * s], [100 * s, 0], 1),
            3: ([0, 0], [0, 0], 0)}


def _planned_which(n, threads, grid, n_pending_rows):
    """row 0 (an exact hit) everywhere but where the plan puts pending captures: rows 1 .. n_pending_rows in turn"""
    which = np.zeros(n, np.int64)
    j = 0
    for block, (counts, _, _) in _plan(threads).items():
        for batch, c in enumerate(counts):
            first = (batch * grid + block) * threads
            for k in range(c):
                which[first + k] = 1 + j % n_pending_rows
                j += 1
    return which


def _plan_claims(threads, n):
    cl = [dict(kind="batches", batches=2, queued=True), dict(kind="no_nothing", queued=True),
          dict(kind="rows_in_batch", block=3, batch=1, rows=37, queued=True), dict(kind="rows_in_batch", block=2, batch=1, rows=threads, queued=True),
          dict(kind="pending_total", total=sum(sum(c) for c, _, _ in _plan(threads).values()), queued=True)]
    for block, (counts, kept, drains) in _plan(threads).items():
        cl.append(dict(kind="pending_plan", block=block, counts=counts, kept=kept, drains=drains, queued=True))
    return cl


def grid_match_case(n_feat):
    """one sweep of the grid and three full tiles and 37 reads more: the workgroups 0 .. 3 take a second batch"""
    L, rng = 15, np.random.default_rng(31)
    threads = 256 if n_feat <= FM_SMALL else 1024
    n = N_GRID["k_match_features_lds", threads] + 3 * threads + 37
    feats = far_seqs(40, L, rng, 4)
    feats += [f for f in random_feats(rng, L, n_feat) if all(hamming(f, g) > 2 for g in feats[:40])][:n_feat - 40]
    assert len(feats) == n_feat
    counts = [int(x) for x in rng.integers(1, 60, n_feat)]
    a, b = feats[1], feats[2]
    counts[3] = 0
    rows = [(feats[0], [Q0] * L), (other(a, 0), q_at(L, p0=40)), (other(a, 7), q_at(L, p7=32)), (with_base(b, L - 1, "N"), q_at(L, **{"p%d" % (L - 1): 67})),
            (other(b, 8, 2), [Q0] * L), (with_base(b, 0, "N"), [Q0] * L), (other(feats[3], 5), [Q0] * L)]
    grid = cr_grid(n, threads, K["k_match_features_lds", threads])
    case = MatchCase("a_grid_%d" % n_feat, L, feats, np.arange(n_feat) + 1, counts, rows, _planned_which(n, threads, grid, len(rows) - 1))
    case.claims = [dict(kind="kernel", kernel="lds%d" % threads)] + _plan_claims(threads, n)
    return case


# ---- group B ------------------------------------------------------------------------------------------------------------
def _literal(rng, s):
    return bytes(ACGT[int(rng.integers(0, 4))] if c == "." else ord(c) for c in s)


def _build_read(rng, total, start, pre, cap, suf, cap_qual, fill=None):
    """a read of `total` bases with prefix + capture + suffix at `start`; the other bases random (or `fill`)"""
    s = bytearray(random_seq(rng, total) if fill is None else B(fill) * total)
    q = [Q0] * total
    at = start + len(pre)
    s[start:at] = _literal(rng, pre)
    s[at:at + len(cap)] = cap
    q[at:at + len(cap)] = cap_qual
    s[at + len(cap):at + len(cap) + len(suf)] = _literal(rng, suf)
    assert len(s) == total
    return bytes(s), q


def tethered_case(name, pattern, L, stride, with_len=True, n=None, n_feat=24, read=1, seed=1, values=None, kernel="lds256"):
    """one tethered pattern over rows of `stride` bytes: the capture variants at every start the pattern allows (floating: the
    first eight and the last), at several read lengths, with the lengths 0, need - 1, need, stride and stride + 5 over a row
    that holds the whole pattern twice (once behind every shorter length)"""
    rng = np.random.default_rng(seed)
    rs = compile_pattern(pattern, L)
    a5, pre, suf, a3 = _tethered_parts(rs)
    need = len(pre) + L + len(suf)
    feats = random_feats(rng, L, n_feat)
    feats = [feats[k] for k in rng.permutation(len(feats))]
    caps = capture_variants(L, feats, rng)
    R = Rows(stride, with_len)
    totals = [t for t in sorted(set([need, need + 1, need + 2, need + 3, stride])) if need <= t <= stride] if with_len else [stride] * (need <= stride)
    combo = 0
    for total in totals:
        starts = [0] if a5 else [total - need] if a3 else sorted(set(range(0, min(8, total - need + 1))) | {total - need})
        if a5 and a3 and total != need:
            starts = [0]        # (cannot match: the restatement says so too)
        for st in starts:
            for c in range(4 if len(totals) * len(starts) > 12 else len(caps)):
                _, cs, cq = caps[(4 * combo + c) % len(caps)]
                R.add(*_build_read(rng, total, st, pre, cs, suf, cq))
            combo += 1
    if with_len and 2 * need <= stride:
        s1, q1 = _build_read(rng, need, 0, pre, feats[0], suf, [Q0] * L)
        s2, q2 = _build_read(rng, stride - need, stride - 2 * need, pre, feats[1 % len(feats)], suf, [Q0] * L, fill="C" if "C" not in pre + suf else "A")
        for length in (0, need - 1, need, need + 1, stride - 1, stride, stride + 5):
            R.add(s1 + s2, q1 + q2, length)
        s3, q3 = _build_read(rng, stride, stride - need, pre, feats[2 % len(feats)], suf, [Q0] * L, fill="C" if "C" not in pre + suf else "A")
        for length in (need - 1, need, stride - 1, stride):
            R.add(s3, q3, length)
    if not R.seq:      # rows shorter than the pattern: nothing can match
        R.add(random_seq(rng, stride), None, None if not with_len else stride)
    which = np.arange(len(R.seq) if n is None else n) % len(R.seq)
    idx = 2 + rng.permutation(len(feats))
    counts = [int(x) for x in rng.integers(0, 60, len(feats) + 2)]
    case = ExtractCase(name, "B", [(pattern, f.decode(), int(idx[k]), read) for k, f in enumerate(feats)], counts,
                       None if read else R, R if read else None, which)
    case.claims.append(dict(kind="kernel", kernel=kernel))
    if values:
        case.claims.append(dict(kind="dispatch", values=values))
    if kernel != "generic" and need <= stride and case.n >= len(R.seq):
        case.claims.append(dict(kind="states", states=[EXACT, PENDING], with_dist=True))
    return case


def floating_case(stride):
    """"GA(BC)TTC" over rows of C: the needle TTC of the suffix in front of the true start, below p_lo and behind p_hi; two valid
    starts; the start at s_hi; the first valid start at every byte alignment of two dwords"""
    L, rng = 8, np.random.default_rng(37)
    pattern, pre, suf = "GA(BC)TTC", "GA", "TTC"
    need, off = 2 + L + 3, 2 + L
    feats = [f for f in far_seqs(60, L, rng, 3) if b"TT" not in f and b"GA" not in f][:8]
    assert len(feats) == 8
    f0, f1 = feats[0], feats[1]
    R = Rows(stride, True)
    tags, claims = {}, []

    def put(tag, s, length=None, **claim):
        tags[tag] = R.add(bytes(s), None, length)
        claims.append(dict(kind="row", tag=tag, **claim))

    def base(total):
        return bytearray(b"C" * total)

    def at(s, st, f):
        s[st:st + need] = b"GA" + f + b"TTC"
    for st in range(0, 9):                       # every alignment, across the first dword edge
        s = base(stride)
        at(s, st, f0)
        put("align_%d" % st, s, start=st + 2, state=EXACT)
    s = base(stride)
    at(s, 14, f0)
    s[off:off + 3] = b"TTC"                      # the needle where start 0 would have it; no GA there
    put("needle_fails_in_front", s, start=16, state=EXACT)
    s = base(stride)
    at(s, 13, f0)
    s[off - 2:off + 1] = b"TTC"                  # the needle two bytes below p_lo, in the dword the scan starts with
    put("needle_below_p_lo", s, start=15, state=EXACT)
    s = base(stride)
    at(s, 3, f0), at(s, 3 + need, f1)
    put("two_starts", s, start=5, state=EXACT)
    s = base(stride)
    at(s, stride - need, f1)
    put("start_at_s_hi", s, start=stride - need + 2, state=EXACT)
    s = base(stride)
    at(s, stride - need, f1)
    put("cut_by_len", s, stride - 1, n_caps=0)   # the needle hit lies one behind p_hi: the pattern is whole only behind len
    s = base(stride)
    at(s, 2, f1)
    put("len_need_minus_1", s, need - 1, n_caps=0)
    s = base(stride)
    at(s, 0, f1)
    put("len_need", s, need, start=2, state=EXACT)
    s = base(stride)
    at(s, 5, other(f1, 3))
    put("pending", s, start=7, state=PENDING, n_cand=1, queued=True)
    case = ExtractCase("b_floating_%d" % stride, "B", [(pattern, f.decode(), k, 1) for k, f in enumerate(feats)], [5] * 8, None, R, np.arange(len(R.seq)))
    case.tags = tags
    case.claims = claims + [dict(kind="dispatch", values=dict(kernel="lds256", win_lo=0, win_dw=stride // 4, needle_len=3, needle_off=off, pitch=(stride // 4) | 1))]
    return case


def posterior_extract_case(n_feat_extra=0, name="b_posterior", narrow=False):
    """the posterior set behind "5PNN(BC)": 16-base captures at byte 2 of 32-byte rows (a window of five dwords); narrow: 12-base
    captures behind "5PNNNN(BC)" in 16-byte rows, a window of three dwords, all the 1024-thread kernel has room for beside a set
    of 8192 slots.  n_feat_extra: more features, far from the set, to move the extractor across the 1024 / 1025 and 4096 / 4097
    switches"""
    L, stride, pattern, lead = (12, 16, "5PNNNN(BC)", b"GTAC") if narrow else (16, 32, "5PNN(BC)", b"GT")
    rng = np.random.default_rng(41)
    feats, counts, rows, claims = posterior_set(L, rng)
    if n_feat_extra:
        have = list(feats)
        for f in random_feats(rng, L, n_feat_extra + 64):
            if len(feats) - len(have) < n_feat_extra and all(hamming(f, g) > 2 for g in have):
                feats.append(f)
                counts.append(int(rng.integers(1, 9)))
        assert len(feats) == len(have) + n_feat_extra
    R = Rows(stride, False)
    tags = {}
    pad = stride - len(lead) - L
    for tag, s, q in rows:
        tags[tag] = R.add(lead + s + b"C" * pad, [Q0] * len(lead) + list(q) + [Q0] * pad)
    nf = len(feats)
    case = ExtractCase(name, "B", [(pattern, f.decode(), k, 1) for k, f in enumerate(feats)], counts, None, R, np.arange(len(R.seq)))
    case.tags = tags
    wide = not narrow and nf > 2048        # a set of 8192 slots leaves the 1024-thread kernel no room for windows of five dwords
    kernel = "generic" if nf > FXT_MAX_FEATURES or wide else "lds256" if nf <= FXT_SMALL else "lds1024"
    case.claims = [dict(kind="kernel", kernel=kernel)]
    if kernel != "generic":
        case.claims += claims + [dict(kind="n_cand_occurs", values=[FXT_MAXC, FXT_MAXC + 1], with_dist=True),
                                 dict(kind="dispatch", values=dict(halves=nf <= FXT_SMALL, win_dw=3 if narrow else 5), with_dist=True)]
    return case


def all_t_case():
    """a feature of 32 T packs to the value an empty slot of the LDS set holds: as an exact capture, as the target of one
    substitution among few candidates, and among more than FXT_MAXC of them"""
    L, rng = 32, np.random.default_rng(43)
    t = b"T" * L
    feats, counts = [t], [500]
    few = other(t, 5)                            # not a feature; candidates: all T and one more
    feats.append(other(few, 20)), counts.append(1)
    many = other(t, 9)                           # not a feature; candidates: all T and FXT_MAXC more
    spots = [(p, k) for p in (1, 17, 30) for k in (1, 2, 3)][:FXT_MAXC]
    for p, k in spots:
        feats.append(other(many, p, k)), counts.append(1)
    for f in far_seqs(6, L, rng, 8, avoid=[t]):
        feats.append(f), counts.append(int(rng.integers(1, 20)))
    R = Rows(32, False)
    tags = dict(exact=R.add(t), few=R.add(few, q_at(L, p5=40)), many=R.add(many, q_at(L, p9=40)), n=R.add(with_base(t, 31, "N")),
                other=R.add(feats[-1]), other_mm=R.add(other(feats[-1], 16)))
    case = ExtractCase("b_all_t", "B", [("^(BC)", f.decode(), k + 1, 0) for k, f in enumerate(feats)], [0] + counts, R, None, np.arange(len(R.seq)) % len(R.seq))
    case.tags = tags
    case.claims = [dict(kind="kernel", kernel="generic"), dict(kind="dispatch", values=dict(empty_key=True)),
                   dict(kind="row", tag="exact", feature=1), dict(kind="row", tag="few", feature=1, map=2, with_dist=True),
                   dict(kind="row", tag="many", feature=1, map=FXT_MAXC + 1, with_dist=True), dict(kind="row", tag="n", feature=1, with_dist=True)]
    return case


def last_slot_extract_case():
    """features whose fxt_hash is the last slot of a 64-slot set: inserting and probing wrap to slot 0"""
    L, rng = 12, np.random.default_rng(47)
    last, key = [], 0
    while len(last) < 4:
        key += 7
        if fxt_hash(key, 63) == 63:
            last.append(seq_of(key, L))
    feats = last + [f for f in random_feats(rng, L, 20) if f not in last]
    R = Rows(16, False)
    for f in feats[:8]:
        R.add(b"A" + f + b"CCC")
        R.add(b"A" + other(f, 6) + b"CCC", [Q0] * 7 + [36] + [Q0] * 8)
    case = ExtractCase("b_last_slot", "B", [("5PN(BC)", f.decode(), k, 1) for k, f in enumerate(feats)], [4] * len(feats), None, R, np.arange(len(R.seq)))
    case.claims = [dict(kind="last_slot", at_least=4), dict(kind="slots", slots=64), dict(kind="kernel", kernel="lds256")]
    return case


GRID_SHAPES = {16: ("5PNN(BC)", 8, dict(quad_lanes=1, prefetch=True, win_dw=3)), 32: ("5PNN(BC)", 20, dict(quad_lanes=2, prefetch=True, win_dw=6)),
               64: ("(BC)GTTTAAGAGC", 20, dict(quad_lanes=4, prefetch=False, win_dw=16))}


def grid_extract_case(stride, n_feat=40):
    """the plan of grid_match_case for k_extract_tethered_lds, over rows of `stride` bytes without lengths"""
    pattern, L, values = GRID_SHAPES[stride]
    rng = np.random.default_rng(53 + stride)
    threads = 256 if n_feat <= FXT_SMALL else 1024
    n = N_GRID["k_extract_tethered_lds", threads] + 3 * threads + 37
    feats = far_seqs(40, L, rng, 3 if L <= 8 else 5)
    if n_feat > 40:
        feats += [f for f in random_feats(rng, L, 2 * n_feat) if all(hamming(f, g) > 2 for g in feats[:40])][:n_feat - 40]
    assert len(feats) == n_feat
    counts = [int(x) for x in rng.integers(1, 60, n_feat)]
    counts[3] = 0
    _, pre, suf, _ = _tethered_parts(compile_pattern(pattern, L))
    a, b = feats[1], feats[2]
    R = Rows(stride, False)
    st = 0 if pattern.startswith("5P") else 5
    for cap, q in ((feats[0], [Q0] * L), (other(a, 0), q_at(L, p0=40)), (other(a, L // 2), q_at(L, **{"p%d" % (L // 2): 32})),
                   (with_base(b, L - 1, "N"), q_at(L, **{"p%d" % (L - 1): 67})), (other(b, 3, 2), [Q0] * L), (with_base(b, 0, "N"), [Q0] * L),
                   (other(feats[3], 5), [Q0] * L)):
        R.add(*_build_read(rng, stride, st, pre, cap, suf, q, fill="C"))
    grid = cr_grid(n, threads, K["k_extract_tethered_lds", threads])
    case = ExtractCase("b_grid_%d_%d" % (stride, n_feat), "B", [(pattern, f.decode(), k + 1, 1) for k, f in enumerate(feats)], [0] + counts, None, R,
                       _planned_which(n, threads, grid, len(R.seq) - 1))
    case.claims = [dict(kind="dispatch", values=dict(kernel="lds%d" % threads, **values))] + _plan_claims(threads, n)
    return case


def two_pass_case(n, n_missing, n_two_n=5):
    """`n_missing` captures without an exact feature (at most one N) and n_two_n with two Ns among exact hits: what a call
    without a distribution records for the call with one"""
    L, rng = 8, np.random.default_rng(59)
    feats = far_seqs(30, L, rng, 3)
    counts = [int(x) for x in rng.integers(1, 60, len(feats))]
    R = Rows(16, False)
    for cap, q in ((feats[0], [Q0] * L), (other(feats[1], 2), q_at(L, p2=40)), (with_base(feats[2], 7, "N"), [Q0] * L), (other(feats[4], 0, 3), [Q0] * L),
                   (with_base(with_base(feats[5], 0, "N"), 4, "N"), [Q0] * L)):
        R.add(*_build_read(rng, 16, 0, "..", cap, "", q, fill="C"))
    which = np.zeros(n, np.int64)
    spots = rng.permutation(n)
    which[spots[:n_missing]] = 1 + np.arange(n_missing) % 3
    which[spots[n_missing:n_missing + n_two_n]] = 4
    case = ExtractCase("b_two_pass_%d_%d" % (n, n_missing), "B", [("5PNN(BC)", f.decode(), k, 1) for k, f in enumerate(feats)], counts, None, R, which)
    case.claims = [dict(kind="kernel", kernel="lds256"), dict(kind="records", count=n_missing, queued=True)]
    return case


# ---- group C ------------------------------------------------------------------------------------------------------------
def _generic_case(name, defs, counts, r1, r2, n=None):
    rows = len((r1 or r2).seq)
    case = ExtractCase(name, "C", defs, counts, r1, r2, np.arange(rows if n is None else n) % rows)
    case.claims.append(dict(kind="kernel", kernel="generic"))
    return case


def wide_map_case():
    """two bare groups: windows of 8 bases around a centre with FX_LOCAL_ENTRIES of its neighbours listed, windows of 9 around one
    with FX_LOCAL_ENTRIES + 1.  A read with the first centre fills the local map exactly, one with the second outgrows it, one
    with both overflows in its second pattern only."""
    rng = np.random.default_rng(61)
    c8, c9 = b"ACGTTGCA", b"TGCATCAGT"
    f8 = neighbours(c8)[:FX_LOCAL_ENTRIES]
    f9 = neighbours(c9)[:FX_LOCAL_ENTRIES + 1]
    defs = [("(BC)", f.decode(), k, 1) for k, f in enumerate(f8 + f9)]
    counts = [int(x) for x in rng.integers(1, 50, len(defs))]
    R = Rows(40, True)
    tags = dict(fits=R.add(b"GGGGGG" + c8 + b"GGGGGGG", [int(x) for x in rng.integers(34, 70, 21)]),
                over=R.add(b"GGGGG" + c9 + b"GGGGGGG", [int(x) for x in rng.integers(34, 70, 21)]),
                second_over=R.add(b"GGG" + c8 + b"GGGGGGGGGG" + c9 + b"GGG", [int(x) for x in rng.integers(34, 70, 33)]),
                exact=R.add(b"GGGG" + f8[3] + b"GGGGGGGGGGGGG"), nothing=R.add(b"G" * 30))
    case = _generic_case("c_wide_map", defs, counts, None, R, n=5 * 40 + 2)
    case.tags = tags
    case.claims += [dict(kind="row", tag="fits", map=FX_LOCAL_ENTRIES, with_dist=True), dict(kind="row", tag="over", map=FX_LOCAL_ENTRIES + 1, with_dist=True),
                    dict(kind="row", tag="second_over", map=FX_LOCAL_ENTRIES + 1, with_dist=True),
                    dict(kind="map_occurs", values=[FX_LOCAL_ENTRIES, FX_LOCAL_ENTRIES + 1], with_dist=True),
                    dict(kind="requeued", count=int(np.isin(case.which, [tags["over"], tags["second_over"]]).sum()), with_dist=True)]
    return case


def captures_case():
    """several captures of one bare pattern: the same feature reached twice with the better capture second (replacement, the sum
    updated by the difference, the winner's start), windows one base apart, a window at the very end; len < L and len == L"""
    rng = np.random.default_rng(67)
    L = 8
    feats = [b"ACGTACGG", b"AAAAAAAA"] + far_seqs(5, L, rng, 4, avoid=[b"ACGTACGG", b"AAAAAAAA"])
    defs = [("(BC)", f.decode(), k + 2, 1) for k, f in enumerate(feats)]
    counts = [0, 0] + [int(x) for x in rng.integers(1, 50, len(feats))]
    R = Rows(37, True)           # an odd stride
    f = feats[0]
    tags = {}
    s = b"CC" + other(f, 1) + b"CCCC" + other(f, 6) + b"CC"
    q = [Q0] * len(s)
    q[2 + 1], q[14 + 6] = 70, 36                  # the second capture weighs more
    tags["better_second"] = R.add(s, q)
    q[2 + 1], q[14 + 6] = 36, 70
    tags["better_first"] = R.add(s, q)
    tags["one_apart"] = R.add(b"C" + b"A" * 9 + b"CC")
    tags["two_apart"] = R.add(b"GG" + b"A" * 10 + b"GG")
    tags["at_end"] = R.add(b"CCCCC" + feats[2])
    tags["len_below_L"] = R.add(feats[2] + b"CC", None, L - 1)
    tags["len_is_L"] = R.add(feats[2] + b"CC", None, L)
    tags["len_above_stride"] = R.add(b"C" * 29 + feats[3], None, 50)
    tags["len_0"] = R.add(feats[3], None, 0)
    case = _generic_case("c_captures", defs, counts, None, R)
    case.tags = tags
    idx = 2
    case.claims += [dict(kind="row", tag="better_second", n_caps=2, map=1, feature=idx, capture=0x80000000 | (1 << 30) | (14 << 8) | L, with_dist=True),
                    dict(kind="row", tag="better_first", n_caps=2, map=1, feature=idx, capture=0x80000000 | (1 << 30) | (2 << 8) | L, with_dist=True),
                    dict(kind="row", tag="better_second", n_caps=2, feature=NO_FEATURE, capture=(1 << 30) | (14 << 8) | L, with_dist=False),
                    dict(kind="row", tag="one_apart", n_caps=4, feature=3, with_dist=True),
                    dict(kind="row", tag="len_below_L", n_caps=0), dict(kind="row", tag="len_is_L", n_caps=1, feature=4),
                    dict(kind="row", tag="len_above_stride", n_caps=1, feature=5), dict(kind="row", tag="len_0", n_caps=0)]
    return case


def ties_case():
    """patterns of one capture length on both reads: whitelist matches of equal length are told apart by the feature index,
    raw captures by the least index of their pattern; a longer capture beats both"""
    rng = np.random.default_rng(71)
    L = 8
    fs = far_seqs(8, L, rng, 4)
    long = far_seqs(2, 12, rng, 5)
    defs = [("5P(BC)", fs[0].decode(), 6, 1), ("5P(BC)", fs[1].decode(), 7, 1),          # anchored, R2
            ("(BC)", fs[2].decode(), 2, 1), ("(BC)", fs[3].decode(), 9, 1),              # bare, R2
            ("GG(BC)", fs[4].decode(), 0, 0), ("GG(BC)", fs[5].decode(), 11, 0),         # floating, R1
            ("(BC)AC3P", long[0].decode(), 12, 0), ("(BC)AC3P", long[1].decode(), 13, 0)]    # 3' anchored and longer, R1
    counts = [int(x) for x in rng.integers(1, 50, 14)]
    R1, R2 = Rows(32, True), Rows(32, True)
    tags = {}

    def put(tag, a, b):
        R1.add(a)
        tags[tag] = R2.add(b)
    t = b"T" * 6
    put("wl_bare_wins", t, fs[0] + t + fs[2])            # indices 6 and 2: the bare pattern's capture is reported
    put("wl_anchored_wins", t, fs[0] + t + fs[3])        # 6 and 9
    put("wl_r1_wins", b"GG" + fs[4] + t, fs[0] + t)      # 0 on R1 against 6 on R2
    put("wl_r2_wins", b"GG" + fs[5] + t, fs[0] + t)      # 11 against 6
    put("pm_tie", b"GG" + other(other(fs[4], 1), 5) + t, other(other(fs[0], 2), 6) + t)     # raw captures: least indices 0 and 6
    put("pm_bare", t, other(other(fs[1], 2), 6) + t + other(fs[2], 3) + t)
    put("longer_wins", b"GG" + fs[4] + long[0] + b"AC", fs[0] + t)
    put("longer_raw", b"GG" + fs[4] + other(other(long[0], 1), 7) + b"AC", t)
    put("only_r1", b"GG" + fs[4], t)
    put("nothing", t, t)
    case = _generic_case("c_ties", defs, counts, R1, R2)
    case.tags = tags
    W = 0x80000000
    case.claims += [dict(kind="row", tag="wl_bare_wins", capture=W | (1 << 30) | (14 << 8) | L, feature=NO_FEATURE),
                    dict(kind="row", tag="wl_anchored_wins", capture=W | (1 << 30) | (0 << 8) | L, feature=NO_FEATURE),
                    dict(kind="row", tag="wl_r1_wins", capture=W | (0 << 30) | (2 << 8) | L), dict(kind="row", tag="wl_r2_wins", capture=W | (1 << 30) | L),
                    dict(kind="row", tag="pm_tie", capture=(0 << 30) | (2 << 8) | L, with_dist=False),
                    dict(kind="row", tag="longer_wins", capture=W | (10 << 8) | 12), dict(kind="row", tag="only_r1", feature=0)]
    return case


def bare_length_case(L):
    rng = np.random.default_rng(73 + L)
    feats = random_feats(rng, L, 6) if L > 3 else [seq_of(k, L) for k in range(0, 4 ** L, 3)][:max(1, 4 ** L // 3)]
    if L == 32:
        feats.append(b"T" * 32)
    defs = [("(BC)", f.decode(), k, 1) for k, f in enumerate(feats)]
    counts = [int(x) for x in rng.integers(0, 50, len(feats))]
    stride = 40 if L == 32 else 12
    R = Rows(stride, True)
    for f in feats[:6] + feats[-1:]:
        for st in (0, 1, stride - L):
            R.add(*_build_read(rng, stride - (st == 1), st, "", f, "", [int(x) for x in rng.integers(33, 70, L)]))
            m = other(f, L // 2)
            R.add(*_build_read(rng, stride - 2 * (st == 1), st, "", m, "", [int(x) for x in rng.integers(33, 70, L)]))
        R.add(with_base(f, L - 1, "N") + b"C", None)
        R.add(f, None, L - 1)
    return _generic_case("c_bare_L%d" % L, defs, counts, None, R)


# ---- group D ------------------------------------------------------------------------------------------------------------
def count_same_home_case():
    """more features than probes on one home slot, in one workgroup; NO_FEATURE and n_features skipped, n_features - 1 counted"""
    n_features = 1 << 18
    home, fs, f = fc_hash(12345), [], 0
    while len(fs) < FC_PROBES + 4:
        if fc_hash(f) == home:
            fs.append(f)
        f += 1
    rng = np.random.default_rng(79)
    feature = np.array(fs, np.uint32)[rng.integers(0, len(fs), 200)]
    feature[:len(fs)] = fs
    feature = np.concatenate([feature, np.array([NO_FEATURE, n_features, n_features - 1, n_features - 1, n_features + 7, 0], np.uint32)])
    case = CountCase("d_same_home", feature, n_features, counts_in=rng.integers(0, 5, n_features))
    case.claims = [dict(kind="same_home", more_than=FC_PROBES), dict(kind="grid", grid=1)]
    return case


def count_full_table_case():
    """13 sweeps of the full grid, every workgroup meeting 13 x 256 distinct features: more than the table may hold"""
    T, G = K["FC_THREADS"], K["FC_GRID"]
    sweeps = FC_FILL // T + 1
    n = G * T * sweeps
    i = np.arange(n, dtype=np.int64)
    feature = ((i // (G * T)) * T + i % T).astype(np.uint32) * np.uint32(5) + np.uint32(1)
    case = CountCase("d_full_table", feature, 5 * sweeps * T + 2)
    case.claims = [dict(kind="distinct_per_block", more_than=FC_FILL), dict(kind="grid", grid=G)]
    return case


def count_one_case():
    return CountCase("d_one", np.array([3], np.uint32), 4, counts_in=np.array([9, 0, 0, 2]))


# ---- the cases ----------------------------------------------------------------------------------------------------------
STRIDE_SHAPES = [
    # (stride, pattern, L, lengths given, dispatch values that must come out)
    (4, "5PN(BC)", 3, False, dict(kernel="lds256", win_dw=1, quad_lanes=0)), (4, "(BC)3P", 2, True, dict(kernel="lds256", quad_lanes=0)),
    (8, "5PNNN(BC)", 4, True, dict(kernel="lds256", win_lo=0, win_dw=2, quad_lanes=0)), (8, "A(BC)C", 3, True, dict(kernel="lds256", needle_len=1, needle_off=4)),
    (12, "5PNNNN(BC)", 8, False, dict(kernel="lds256", win_lo=4, win_dw=2, quad_lanes=0)), (12, "(BC)GT3P", 7, False, dict(kernel="lds256", win_lo=0, win_dw=3)),
    (16, "5PNNN(BC)", 12, True, dict(kernel="lds256", win_lo=0, win_dw=4, quad_lanes=1, prefetch=True)),
    (16, "TTN(BC)GNA", 9, True, dict(kernel="lds256", win_dw=4, needle_len=1, needle_off=12)),
    (20, "5PNNNNNNNNNN(BC)", 8, True, dict(kernel="lds256", win_lo=8, win_dw=3, quad_lanes=1, quad_in_front=True)),
    (32, "5PNNNNNNNNNNNN(BC)", 15, False, dict(kernel="lds256", win_lo=12, win_dw=4, quad_lanes=1)),
    (32, "(BC)GTTTAAGAGC", 20, True, dict(kernel="lds256", win_dw=8, quad_lanes=2, prefetch=True, needle_len=4, needle_off=20, pitch=9)),
    (36, "5PACGT(BC)", 15, True, dict(kernel="lds256", win_lo=0, win_dw=5, quad_lanes=2)), (36, "ACGN(BC)", 12, True, dict(kernel="lds256", win_dw=9, needle_len=3, needle_off=0, pitch=9)),
    (36, "NA(BC)", 10, True, dict(kernel="lds256", needle_len=0)), (36, "AC(BC)", 10, True, dict(kernel="lds256", needle_len=2, needle_off=0)),
    (36, "A(BC)", 10, True, dict(kernel="lds256", needle_len=1, needle_off=0)), (36, "ACGTA(BC)", 10, True, dict(kernel="lds256", needle_len=4, needle_off=0)),
    (36, "(BC)GTTNA", 10, True, dict(kernel="lds256", needle_len=3, needle_off=10)), (36, "(BC)GT", 10, True, dict(kernel="lds256", needle_len=2, needle_off=10)),
    (64, "(BC)AC3P", 7, True, dict(kernel="lds256", win_lo=0, win_dw=16, quad_lanes=4, prefetch=False)),
    (64, "(BC)AC3P", 7, False, dict(kernel="lds256", win_lo=52, win_dw=3, quad_lanes=1, quad_in_front=True)),
    (64, "^NN(BC)NNC$", 10, True, dict(kernel="lds256", win_lo=0, win_dw=4, quad_lanes=1)),
    (256, "(BC)GTTTAAGAGCTAAGCTGGAA", 20, True, dict(kernel="lds256", win_dw=64, quad_lanes=16, prefetch=False)),
    (256, "5PNNNNNNNNNN(BC)", 15, True, dict(kernel="lds256", win_lo=8, win_dw=5, quad_lanes=2)),
    (260, "(BC)GTTTAAGAGCTAAGCTGGAA", 20, True, dict(kernel="generic")), (260, "5PNNNNNNNNNN(BC)", 15, True, dict(kernel="lds256", win_dw=5)),
]
B_LENGTHS = (1, 2, 3, 31, 32)
BUILDERS = {}


def _register():
    for L in A_LENGTHS:
        for j, n in enumerate(A_SIZES):
            BUILDERS["a_L%d_n%d" % (L, n)] = (lambda L=L, n=n, j=j: match_case("a_L%d_n%d" % (L, n), L, n, 40, 100 * L + j))
    BUILDERS["a_posterior"] = posterior_match_case
    for nf in (FM_SMALL, FM_SMALL + 1, FM_MAX_FEATURES, FM_MAX_FEATURES + 1):
        BUILDERS["a_nfeat_%d" % nf] = (lambda nf=nf: match_case("a_nfeat_%d" % nf, 16, 301, nf, nf, kernel="global" if nf > FM_MAX_FEATURES else None))
    BUILDERS["a_unaligned"] = lambda: match_case("a_unaligned", 15, 259, 40, 5, offset=1, kernel="global")
    BUILDERS["a_no_dist"] = lambda: match_case("a_no_dist", 15, 259, 40, 6, with_dist=False)
    BUILDERS["a_wrap_32"] = lambda: wrap_match_case(32)
    BUILDERS["a_wrap_33"] = lambda: wrap_match_case(33)
    BUILDERS["a_grid_40"] = lambda: grid_match_case(40)
    BUILDERS["a_grid_%d" % (FM_SMALL + 1)] = lambda: grid_match_case(FM_SMALL + 1)
    for k, (stride, pattern, L, with_len, values) in enumerate(STRIDE_SHAPES):
        name = "b_s%d_%s_%s" % (stride, re.sub(r"\W", "", pattern.replace("(BC)", "_")), "len" if with_len else "full")
        BUILDERS[name] = (lambda name=name, k=k, stride=stride, pattern=pattern, L=L, with_len=with_len, values=values:
                          tethered_case(name, pattern, L, stride, with_len, seed=200 + k, values=values, kernel=values["kernel"]))
    for j, n in enumerate(A_SIZES):
        BUILDERS["b_n%d" % n] = (lambda n=n, j=j: tethered_case("b_n%d" % n, "5PNNNNNNNNNN(BC)", 15, 28, j % 2 == 0, n=n, seed=300 + j,
                                                               values=dict(kernel="lds256", win_lo=8, win_dw=5, quad_lanes=2)))
    for L in B_LENGTHS:
        BUILDERS["b_L%d" % L] = (lambda L=L: tethered_case("b_L%d" % L, "5PN(BC)C", L, 36, True, seed=400 + L, values=dict(kernel="lds256")))
    BUILDERS["b_floating_32"] = lambda: floating_case(32)
    BUILDERS["b_floating_36"] = lambda: floating_case(36)
    BUILDERS["b_posterior"] = posterior_extract_case
    base = len(posterior_set(16, np.random.default_rng(41))[0])
    for nf in (FXT_SMALL, FXT_SMALL + 1, FXT_MAX_FEATURES, FXT_MAX_FEATURES + 1):
        BUILDERS["b_nfeat_%d" % nf] = (lambda nf=nf: posterior_extract_case(nf - base, "b_nfeat_%d" % nf))
    for nf in (FXT_MAX_FEATURES, FXT_MAX_FEATURES + 1):
        BUILDERS["b_nfeat_%d_narrow" % nf] = (lambda nf=nf: posterior_extract_case(nf - base, "b_nfeat_%d_narrow" % nf, narrow=True))
    BUILDERS["b_all_t"] = all_t_case
    BUILDERS["b_last_slot"] = last_slot_extract_case
    for stride in GRID_SHAPES:
        BUILDERS["b_grid_%d_40" % stride] = (lambda stride=stride: grid_extract_case(stride))
    BUILDERS["b_grid_16_%d" % (FXT_SMALL + 1)] = lambda: grid_extract_case(16, FXT_SMALL + 1)
    BUILDERS["b_two_pass_%d_100" % (REC_MIN_N - 1)] = lambda: two_pass_case(REC_MIN_N - 1, 100)
    BUILDERS["b_two_pass_%d_%d" % (REC_MIN_N, rec_cap(REC_MIN_N))] = lambda: two_pass_case(REC_MIN_N, rec_cap(REC_MIN_N))
    BUILDERS["b_two_pass_%d_%d" % (REC_MIN_N, rec_cap(REC_MIN_N) + 1)] = lambda: two_pass_case(REC_MIN_N, rec_cap(REC_MIN_N) + 1)
    BUILDERS["c_wide_map"] = wide_map_case
    BUILDERS["c_captures"] = captures_case
    BUILDERS["c_ties"] = ties_case
    for L in (1, 2, 3, 32):
        BUILDERS["c_bare_L%d" % L] = (lambda L=L: bare_length_case(L))
    BUILDERS["d_same_home"] = count_same_home_case
    BUILDERS["d_full_table"] = count_full_table_case
    BUILDERS["d_one"] = count_one_case


_register()
_cases = {}


def get_case(name):
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
        assert _cases[name].name == name, (_cases[name].name, name)
    return _cases[name]


def names(group):
    return [n for n in BUILDERS if n.startswith(group.lower() + "_")]
