"""Constructed inputs for the read ingest: FASTQ text -> rows (k_nl_count, k_nl_write, k_fastq_rows in metrics.hip), the
packing of barcode / UMI slices (k_pack, k_pack_rows, k_pack_rows_var in barcode.hip) and the MAKE_SHARD metrics
(k_shard_metrics, k_rows_metrics, k_homopolymer_metrics).

Host only: numpy and the standard library, no device, no oracle.  The constants the cases turn on (FQ_TILE, the plan of
crgpu_fastq_to_rows_dev, the windows of row_homopolymers, the grid cap) are read out of the source text, so a changed plan
either moves the cases with it or fails here.  A case carries claims about itself ("a line feed on the last byte of tile
0"); describe_*() recomputes the structure from the bytes alone and check_claims() asserts every claim against it, so a case
that no longer hits its edge fails instead of passing.  The restatements are exact: integers, no tolerance anywhere."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG_CB_HAS_N = 0x10
MISS = 0xFFFFFFFF
LF, CR = 10, 13


# ---- constants from the source -----------------------------------------------------------------------------------------
def _source(name):
    with open(os.path.join(ROOT, "cellranger_amd", "csrc", name)) as f:
        return f.read()


def _need(text, pattern, what):
    m = re.search(pattern, text, re.M)
    if not m:
        raise RuntimeError("ingest_cases: %s no longer reads as the cases assume" % what)
    return m


def _read_constants():
    mh, ch = _source("metrics.hip"), _source("common.h")
    k = {}
    m = re.search(r"^#define\s+FQ_TILE\s+(\d+)u?\b", mh, re.M)
    assert m, "ingest_cases: #define FQ_TILE not found in metrics.hip"
    k["FQ_TILE"] = int(m.group(1))
    # the plan of crgpu_fastq_to_rows_dev: 4 * FQ_TILE bytes per workgroup, at most 4096 workgroups, tiles of whole 256-byte rounds
    _need(mh, r"nb\s*=\s*\(n_bytes\s*\+\s*4\s*\*\s*FQ_TILE\s*-\s*1\)\s*/\s*\(4\s*\*\s*FQ_TILE\);", "the 4 * FQ_TILE bytes per workgroup")
    _need(mh, r"nb\s*=\s*nb\s*<\s*1\s*\?\s*1\s*:\s*\(nb\s*>\s*4096\s*\?\s*4096\s*:\s*nb\);", "the cap of 4096 workgroups")
    _need(mh, r"tile\s*=\s*\(n_bytes\s*\+\s*nb\s*-\s*1\)\s*/\s*nb;", "the tile of the plan")
    _need(mh, r"tile\s*=\s*\(tile\s*\+\s*255\)\s*/\s*256\s*\*\s*256;", "the tile rounded up to 256")
    _need(mh, r"nb\s*=\s*\(n_bytes\s*\+\s*tile\s*-\s*1\)\s*/\s*tile;", "the workgroups of the rounded tile")
    _need(mh, r"for\s*\(uint64_t base = lo;\s*base < hi;\s*base \+= 256\)", "the 256-byte rounds of k_nl_write")
    # row_homopolymers: windows of 64 bytes (one per lane of the ballot), a step of 64 - (run_len - 1), w + run_len <= L
    _need(mh, r"const uint32_t step\s*=\s*64u\s*-\s*\(run_len\s*-\s*1u\);", "the window step of row_homopolymers")
    _need(mh, r"for\s*\(uint32_t w = 0;\s*w \+ run_len <= L;\s*w \+= step\)", "the window loop of row_homopolymers")
    _need(mh, r"const uint32_t p = w \+ lane;", "the 64-byte window of row_homopolymers")
    _need(mh, r"run_len >= 2 && run_len <= 64", "the run lengths 2..64")
    # the grids: at most 256 * 8 workgroups, a thread per read (256 a workgroup) or a wave per row (4 a workgroup)
    _need(ch, r"cr_grid\(uint64_t n, uint32_t block, uint32_t max_blocks\s*=\s*256u \* 8u\)", "the 256u * 8u grid cap of cr_grid")
    for kern, per in (("k_shard_metrics", r"n, 256"), ("k_rows_metrics", r"n, 4"), ("k_homopolymer_metrics", r"n, 4"),
                      ("k_fastq_rows", r"n_rec \* 64, 256")):
        _need(mh, r"%s, dim3\(cr_grid\(%s, 256u \* 8u\)\), dim3\(256\)" % (kern, per), "the grid of " + kern)
    bh = _source("barcode.hip")
    for kern in ("k_pack", "k_pack_rows", "k_pack_rows_var"):
        _need(bh, r"%s, dim3\(cr_grid\(n, 256\)\), dim3\(256\)" % kern, "the grid of " + kern)
    k["GRID_CAP"] = 256 * 8
    return k


K = _read_constants()
FQ_TILE, GRID_CAP = K["FQ_TILE"], K["GRID_CAP"]
THREAD_WRAP = GRID_CAP * 256     # reads beyond which a thread-per-read grid wraps
WAVE_WRAP = GRID_CAP * 4         # rows beyond which a wave-per-row grid wraps
HP_WINDOW = 64


def fastq_plan(n_bytes):
    """(workgroups before the rounding, workgroups, tile) of crgpu_fastq_to_rows_dev -- for the placement of the cases only"""
    nb0 = (n_bytes + 4 * FQ_TILE - 1) // (4 * FQ_TILE)
    nb0c = min(max(nb0, 1), 4096)
    tile = (n_bytes + nb0c - 1) // nb0c
    tile = (tile + 255) // 256 * 256
    return nb0c, (n_bytes + tile - 1) // tile, tile


def hp_step(run_len):
    return HP_WINDOW - (run_len - 1)


# ---- FASTQ: builder, restatement, description ----------------------------------------------------------------------------
class FastqRefused(ValueError):
    pass


def fastq_text(records, eol=b"\n", final=True):
    """records: (header, sequence, separator, quality) as bytes"""
    lines = [x for r in records for x in r]
    return eol.join(lines) + (eol if final and lines else b"")


def fastq_lines(text):
    lines = bytes(text).split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()                                    # the piece behind a final line feed
    return [l[:-1] if l.endswith(b"\r") else l for l in lines]


def fastq_rows(text, stride):
    """what crgpu.h says of crgpu_fastq_to_rows_dev: (sequence rows, quality rows, lengths in the file) or FastqRefused"""
    lines = fastq_lines(text) if len(text) else []
    if len(lines) % 4:
        raise FastqRefused("%d lines" % len(lines))
    n = len(lines) // 4
    seq, qual, lens = np.zeros((n, stride), np.uint8), np.zeros((n, stride), np.uint8), np.zeros(n, np.uint32)
    for r in range(n):
        h, s, p, q = lines[4 * r:4 * r + 4]
        if not h.startswith(b"@"):
            raise FastqRefused("record %d: header" % r)
        if not p.startswith(b"+"):
            raise FastqRefused("record %d: separator" % r)
        if len(s) != len(q):
            raise FastqRefused("record %d: %d bases, %d qualities" % (r, len(s), len(q)))
        lens[r] = len(s)
        k = min(len(s), stride)
        seq[r, :k] = np.frombuffer(s[:k], np.uint8)
        qual[r, :k] = np.frombuffer(q[:k], np.uint8)
    return seq, qual, lens


def describe_text(text):
    """the structure of a FASTQ text from its bytes alone"""
    t = np.frombuffer(bytes(text), np.uint8)
    n = len(t)
    lf = np.flatnonzero(t == LF)
    d = dict(n_bytes=n, n_lf=len(lf), final_lf=bool(n and t[-1] == LF))
    crlf = lf[(lf > 0)]
    crlf = crlf[t[crlf - 1] == CR]
    d["n_crlf"] = len(crlf)
    d["all_crlf"] = len(lf) > 0 and len(crlf) == len(lf)
    d["n_cr"] = int((t == CR).sum())
    d["ends_with_cr"] = bool(n and t[-1] == CR)
    nb0, nb, tile = fastq_plan(max(n, 1))
    d.update(nb0=nb0, nb=nb, tile=tile, nb_uncapped=(n + 4 * FQ_TILE - 1) // (4 * FQ_TILE))
    in_tile = lf % tile
    d["lf_last_of_tile"] = lf[(in_tile == tile - 1) & (lf + 1 < n)]          # a next tile exists
    d["lf_first_of_tile"] = lf[(in_tile == 0) & (lf > 0)]
    d["crlf_across_tiles"] = crlf[(crlf % tile == 0)]                          # CR on the last byte of the tile before
    inner = (in_tile != 0) & (in_tile != tile - 1)
    d["lf_last_of_round"] = lf[inner & (in_tile % 256 == 255)]
    d["lf_first_of_round"] = lf[inner & (in_tile % 256 == 0)]
    ci = crlf % tile
    d["crlf_across_rounds"] = crlf[(ci != 0) & (ci % 256 == 0)]
    d["len_mod_tile"] = n % tile
    # line feeds per 256-byte round (rounds start at the tile's first byte) and per wave of a round
    rounds = (lf // tile) * (tile // 256) + in_tile // 256
    d["max_lf_per_round"] = int(np.bincount(rounds).max()) if len(lf) else 0
    waves = (lf // tile) * (tile // 64) + in_tile // 64
    d["max_lf_per_wave"] = int(np.bincount(waves).max()) if len(lf) else 0
    lines = fastq_lines(text) if n else []
    d["n_lines"] = len(lines)
    d["seq_lens"] = [len(l) for l in lines[1::4]]
    d["qual_first"] = set(l[:1] for l in lines[3::4])
    d["headers_with"] = set(ch for l in lines[0::4] for ch in (b"@", b"+") if ch in l[1:])
    d["sep_repeats_name"] = sum(1 for h, p in zip(lines[0::4], lines[2::4]) if len(p) > 1 and p[1:] == h[1:])
    return d


class Case:
    def __init__(self, name, claims, **kw):
        self.name, self.claims = name, claims
        self.__dict__.update(kw)


def _check_text_claims(name, d, claims):
    assert claims, name
    for key, want in claims.items():
        if key == "n_bytes_below":
            ok = d["n_bytes"] < want
        elif key == "seq_lens_include":
            ok = set(want) <= set(d["seq_lens"])
        elif key == "qual_first_include":
            ok = set(want) <= d["qual_first"]
        elif key == "headers_with":
            ok = set(want) <= d["headers_with"]
        elif key == "sep_repeats_name_min":
            ok = d["sep_repeats_name"] >= want
        elif key == "max_lf_per_round_min":
            ok = d["max_lf_per_round"] >= want
        elif key == "n_records":
            ok = d["n_lines"] == 4 * want
        elif key == "lines_mod_4":
            ok = d["n_lines"] % 4 == want
        elif key.endswith("_nonempty"):
            ok = len(d[key[:-9]]) > 0
        else:
            ok = d[key] == want
        assert ok, "%s: claim %s = %r does not hold (%r)" % (name, key, want, d.get(key))


def _rec(i, seq, qual, name=None, sep=b"+"):
    return (b"@" + (name if name is not None else b"r%d" % i), seq, sep, qual)


def _rand_seq(rng, L, alphabet=b"ACGTN", p=None):
    return rng.choice(np.frombuffer(alphabet, np.uint8), size=L, p=p).tobytes()


def _rand_qual(rng, L):
    return rng.integers(33, 127, size=L, dtype=np.uint8).tobytes()      # every printable quality, '@' and '+' among them


def small_fastq_cases():
    """group A: (name, text, stride, claims)"""
    cases = []
    one = [_rec(0, b"ACGTNACGTTGCA", b"IIII#5?@+IIII")]
    for name, eol, final in (("one_lf", b"\n", True), ("one_lf_nofinal", b"\n", False), ("one_crlf", b"\r\n", True),
                             ("one_crlf_nofinal", b"\r\n", False)):
        cases.append(Case(name, dict(n_bytes_below=256, n_records=1, final_lf=final, all_crlf=eol == b"\r\n", nb=1,
                                     ends_with_cr=False), text=fastq_text(one, eol, final), stride=64))
    cases.append(Case("one_crlf_ends_in_cr", dict(n_bytes_below=256, n_records=1, final_lf=False, ends_with_cr=True),
                      text=fastq_text(one, b"\r\n", False) + b"\r", stride=64))
    empties = [_rec(0, b"", b""), _rec(1, b"ACGT", b"IIII"), _rec(2, b"", b""), _rec(3, b"", b"")]
    for name, eol, final in (("empty_reads_lf", b"\n", True), ("empty_reads_crlf", b"\r\n", True), ("empty_reads_nofinal", b"\n", False)):
        recs = empties if final else empties[::-1][1:] + empties[1:2]     # an empty last line needs its line end to exist at all
        cases.append(Case(name, dict(n_records=4, seq_lens_include=[0, 4], final_lf=final),
                          text=fastq_text(recs, eol, final), stride=8))
    # the classic trap: quality lines that begin with '@' and with '+', headers that hold them, separators with the name
    trap = [_rec(0, b"ACGTACGT", b"@IIIIIII", name=b"a@b+c 1:N:0"), _rec(1, b"TTTTACGT", b"+IIIIII@", name=b"+plus"),
            _rec(2, b"GG", b"@+", name=b"@at", sep=b"+@at"), _rec(3, b"C", b"@", name=b"x y", sep=b"+x y"),
            _rec(4, b"A", b"+", name=b"z", sep=b"+z"), _rec(5, b"ACGTN", b"@@@@@"), _rec(6, b"ACGTN", b"+++++")]
    for name, eol, final in (("trap_lf", b"\n", True), ("trap_crlf_nofinal", b"\r\n", False)):
        cases.append(Case(name, dict(n_records=7, qual_first_include=[b"@", b"+"], headers_with=[b"@", b"+"], sep_repeats_name_min=3,
                                     all_crlf=eol == b"\r\n"), text=fastq_text(trap, eol, final), stride=16))
    rng = np.random.default_rng(501)
    for stride in (1, 63, 64, 65, 100, 200):
        lens = [stride - 1, stride, stride + 1, 3 * stride, 0, 1, 2 * stride + 1]
        recs = [_rec(i, _rand_seq(rng, L), _rand_qual(rng, L)) for i, L in enumerate(lens)]
        for eol in (b"\n", b"\r\n"):
            cases.append(Case("stride_%d_%s" % (stride, "crlf" if eol != b"\n" else "lf"),
                              dict(n_records=len(lens), seq_lens_include=[stride - 1, stride, stride + 1, 3 * stride], all_crlf=eol != b"\n"),
                              text=fastq_text(recs, eol, True), stride=stride))
    cases.append(Case("no_len_out", dict(n_records=7), text=fastq_text(trap), stride=16, no_len=True))
    dense = b"@\n\n+\n\n" * 3000
    cases.append(Case("dense", dict(n_records=3000, max_lf_per_round_min=171, max_lf_per_wave=43, nb=2, final_lf=True), text=dense, stride=4))
    cases.append(Case("dense_nofinal", dict(n_records=3001, max_lf_per_round_min=171, final_lf=False), text=dense + b"@\nA\n+\nI", stride=4))
    return cases


def check_small_case(case):
    d = describe_text(case.text)
    _check_text_claims(case.name, d, case.claims)
    return d


# ---- group B: the sweep ----------------------------------------------------------------------------------------------------
SWEEP_D = 512
SWEEP_STRIDE = 48
_sweep = {}


def sweep_records():
    """records of 0..90 bases (some cut at SWEEP_STRIDE), qualities over the whole printable range.  About 1.5 times 4 * FQ_TILE bytes: two
    workgroups at every d, so that the tile is half the length rounded up to 256 and every 512 consecutive lengths hold a
    multiple of the tile and one fewer."""
    if "recs" not in _sweep:
        rng = np.random.default_rng(502)
        recs = []
        while sum(len(r[0]) + len(r[1]) + len(r[2]) + len(r[3]) + 4 for r in recs) < 4 * FQ_TILE + 2 * FQ_TILE:
            L = int(rng.integers(0, 91))
            recs.append(_rec(len(recs), _rand_seq(rng, L, p=[0.24, 0.24, 0.24, 0.24, 0.04]), _rand_qual(rng, L),
                             sep=b"+" if len(recs) % 3 else b"+r%d" % len(recs)))
        _sweep["recs"] = recs
    return _sweep["recs"]


SWEEP_VARIANTS = {"lf": (b"\n", True), "crlf": (b"\r\n", True), "lf_nofinal": (b"\n", False), "crlf_nofinal": (b"\r\n", False)}


def sweep_text(variant, d):
    """the sweep's text with d bytes more in the header of record 0: every later byte moves by d"""
    eol, final = SWEEP_VARIANTS[variant]
    key = ("tail", variant)
    if key not in _sweep:
        recs = sweep_records()
        _sweep[key] = eol.join([recs[0][1], recs[0][2], recs[0][3]] + [x for r in recs[1:] for x in r]) + (eol if final else b"")
    return sweep_records()[0][0] + b"p" * d + eol + _sweep[key]


SWEEP_CLAIMS = {
    "lf": ["lf_last_of_tile", "lf_first_of_tile", "lf_last_of_round", "lf_first_of_round", "len_multiple", "len_one_fewer"],
    "crlf": ["lf_last_of_tile", "lf_first_of_tile", "crlf_across_tiles", "crlf_across_rounds", "lf_last_of_round", "len_multiple",
             "len_one_fewer"],
    "lf_nofinal": ["lf_last_of_tile", "lf_first_of_tile", "len_multiple", "len_one_fewer"],
    "crlf_nofinal": ["lf_last_of_tile", "crlf_across_tiles", "crlf_across_rounds", "len_multiple", "len_one_fewer"],
}


def describe_sweep(variant):
    """{event: the d at which it happens}, from the bytes of all SWEEP_D texts"""
    key = ("events", variant)
    if key in _sweep:
        return _sweep[key]
    ev = {k: [] for k in ("lf_last_of_tile", "lf_first_of_tile", "crlf_across_tiles", "crlf_across_rounds", "lf_last_of_round",
                          "lf_first_of_round", "len_multiple", "len_one_fewer", "len_one_more")}
    tiles = set()
    for dd in range(SWEEP_D):
        d = describe_text(sweep_text(variant, dd))
        assert d["n_bytes"] >= 4 * FQ_TILE + 1 and d["nb0"] == 2 and d["nb"] == 2 and d["n_lines"] == 4 * len(sweep_records())
        tiles.add(d["tile"])
        for k in ev:
            if k.startswith("len_"):
                want = {"len_multiple": 0, "len_one_fewer": d["tile"] - 1, "len_one_more": 1}[k]
                if d["len_mod_tile"] == want:
                    ev[k].append(dd)
            elif len(d[k]):
                ev[k].append(dd)
    ev["tiles"] = sorted(tiles)
    _sweep[key] = ev
    return ev


def check_sweep(variant):
    ev = describe_sweep(variant)
    for k in SWEEP_CLAIMS[variant]:
        assert ev[k], "sweep %s: no text with %s" % (variant, k)
    return ev


def one_byte_tile_text():
    """A text whose last tile holds exactly one byte (its length is one more than a multiple of the tile).  The plan derives
    the tile from the length, so no text of two or three tiles can have that; the shortest length at which the plan allows
    it is found here by search, and the records are made to fit it."""
    if "one_more" not in _sweep:
        n = 4 * FQ_TILE + 1
        while n % fastq_plan(n)[2] != 1:
            n += 1
            assert n < (1 << 24), "no length with a one-byte tile below 16 MiB"
        rng = np.random.default_rng(503)
        recs, size = [], 0
        while True:
            L = int(rng.integers(20, 200))
            r = _rec(len(recs), _rand_seq(rng, L), _rand_qual(rng, L))
            sz = sum(len(x) + 1 for x in r)
            if size + sz + 16 > n:
                break
            recs.append(r)
            size += sz
        pad = n - size - 8                              # the last record "@" + pad + LF, "A", "+", "I": pad + 8 bytes
        recs.append((b"@" + b"q" * pad, b"A", b"+", b"I"))
        _sweep["one_more"] = fastq_text(recs)
        assert len(_sweep["one_more"]) == n
    return _sweep["one_more"]


# ---- group C: the grid wrap and the workgroup cap ------------------------------------------------------------------------------
def wrap_fastq_case():
    """WAVE_WRAP + 5 short records: the wave-per-record loop of k_fastq_rows goes round"""
    rng = np.random.default_rng(504)
    n = WAVE_WRAP + 5
    recs = []
    for i in range(n):
        L = int(rng.integers(0, 20))
        recs.append(_rec(i, _rand_seq(rng, L), _rand_qual(rng, L)))
    return Case("wrap", dict(n_records=n, final_lf=True), text=fastq_text(recs), stride=16, n=n)


LARGE_STRIDE = 48
_large = {}


def large_fastq_case():
    """One text just above 4096 x 4 x FQ_TILE bytes: a block of 61 records of 0..3000 bases, tiled with numpy, and its
    reference rows tiled the same way.  Returns (text as a uint8 array, seq rows, qual rows, lens, claims)."""
    if "case" in _large:
        return _large["case"]
    rng = np.random.default_rng(505)
    recs = []
    for i in range(61):
        L = int(rng.integers(0, 3001)) if i % 4 else int(rng.integers(0, 60))
        recs.append(_rec(i, _rand_seq(rng, L), _rand_qual(rng, L)))
    block = fastq_text(recs)
    assert len(block) % 256 not in (0, 1, 255)                     # the block moves against the tiles from copy to copy
    need = 4096 * 4 * FQ_TILE + 1
    reps = (need + len(block) - 1) // len(block)
    text = np.tile(np.frombuffer(block, np.uint8), reps)
    s, q, l = fastq_rows(block, LARGE_STRIDE)
    case = Case("large", dict(nb0=4096), text=text, seq=np.tile(s, (reps, 1)), qual=np.tile(q, (reps, 1)),
                lens=np.tile(l, reps), stride=LARGE_STRIDE, n=61 * reps, block=block, reps=reps)
    _large["case"] = case
    return case


def check_large_case(case):
    n = len(case.text)
    nb0, nb, tile = fastq_plan(n)
    assert (n + 4 * FQ_TILE - 1) // (4 * FQ_TILE) > 4096 and nb0 == 4096, "the text does not reach the cap of 4096 workgroups"
    assert tile > 4 * FQ_TILE and nb <= 4096 and n < 0xFFFFFFFF
    assert n - len(case.block) < 4096 * 4 * FQ_TILE + 1 <= n       # just above: no whole block to spare
    lf = np.flatnonzero(case.text == LF)
    assert len(lf) == 4 * case.n and case.text[-1] == LF
    in_tile = lf % tile
    assert ((in_tile == tile - 1) & (lf + 1 < n)).any() and (in_tile == 0).any(), "no line feed on a tile edge"
    return dict(nb0=nb0, nb=nb, tile=tile)


# ---- group D: refusals -----------------------------------------------------------------------------------------------------------
def refusal_cases():
    """(name, text, why): texts the FASTQ restatement refuses; the long ones put the fault in a later tile"""
    rng = np.random.default_rng(506)
    good = [_rec(i, _rand_seq(rng, 60), _rand_qual(rng, 60)) for i in range(300)]       # about 2.4 times 4 * FQ_TILE bytes
    base = fastq_text(good)
    assert len(base) > 2 * 4 * FQ_TILE
    out = []
    out.append(Case("lines_4k+1", dict(lines_mod_4=1), text=base + b"@r\n"))
    out.append(Case("lines_4k+2", dict(lines_mod_4=2), text=base + b"@r\nACGT\n"))
    out.append(Case("lines_4k+3", dict(lines_mod_4=3), text=base + b"@r\nACGT\n+\n"))
    out.append(Case("lines_4k+3_nofinal", dict(lines_mod_4=3, final_lf=False), text=base + b"@r\nACGT\n+"))

    def with_record(i, rec):
        r = list(good)
        r[i] = rec
        return fastq_text(r)
    mid = 200
    assert len(fastq_text(good[:mid])) > 4 * FQ_TILE                                       # record 200 starts in a later tile
    for where, i in (("first", 0), ("middle", mid), ("last", len(good) - 1)):
        h, s, p, q = good[i]
        out.append(Case("header_without_at_" + where, dict(lines_mod_4=0, bad_record=i), text=with_record(i, (h[1:], s, p, q))))
    h, s, p, q = good[mid]
    out.append(Case("empty_header", dict(lines_mod_4=0, bad_record=mid), text=with_record(mid, (b"", s, p, q))))
    out.append(Case("separator_without_plus", dict(lines_mod_4=0, bad_record=mid), text=with_record(mid, (h, s, b"-", q))))
    out.append(Case("empty_separator", dict(lines_mod_4=0, bad_record=mid), text=with_record(mid, (h, s, b"", q))))
    h, s, p, q = good[-1]
    out.append(Case("quality_one_short_last", dict(lines_mod_4=0, bad_record=len(good) - 1), text=with_record(len(good) - 1, (h, s, p, q[:-1]))))
    out.append(Case("quality_one_long_last", dict(lines_mod_4=0, bad_record=len(good) - 1), text=with_record(len(good) - 1, (h, s, p, q + b"I"))))
    out.append(Case("line_feeds_only", dict(lines_mod_4=0, n_lf=1024, n_bytes=1024, bad_record=0), text=b"\n" * 1024))
    return out, base, len(good)


def check_refusal_case(case):
    d = describe_text(case.text)
    claims = dict(case.claims)
    bad = claims.pop("bad_record", None)
    _check_text_claims(case.name, d, claims)
    refused = None
    try:
        fastq_rows(case.text, 8)
    except FastqRefused as e:
        refused = str(e)
    assert refused is not None, "%s: the restatement accepts the text" % case.name
    if bad is not None:
        assert refused.startswith("record %d:" % bad), "%s: refused for %s" % (case.name, refused)
    return d


# ---- pack ------------------------------------------------------------------------------------------------------------------------
_CODE = np.zeros(256, np.uint32)
_IS_N = np.ones(256, bool)
for _i, _b in enumerate(b"ACGT"):
    _CODE[_b] = _i
    _IS_N[_b] = False


def pack_ref(seq, qual):
    """(n, L) ASCII bases and qualities -> (packed words, qualn rows, a base was N): codes 0..3 for A C G T, every other byte
    an N with code 0, the first base in the highest bits, qualn = min(q, 127) | 0x80 for an N"""
    seq, qual = np.asarray(seq, np.uint8), np.asarray(qual, np.uint8)
    n, L = seq.shape
    key = np.zeros(n, np.uint32)
    for j in range(L):
        key = (key << np.uint32(2)) | _CODE[seq[:, j]]
    is_n = _IS_N[seq]
    qualn = (np.minimum(qual, 127) | np.where(is_n, 0x80, 0)).astype(np.uint8)
    return key, qualn, is_n.any(axis=1)


def pack_rows_ref(seq_rows, qual_rows, offset, length):
    return pack_ref(seq_rows[:, offset:offset + length], qual_rows[:, offset:offset + length])


def pack_rows_var_ref(seq_rows, qual_rows, read_len, offset, length, min_length):
    """the comment above k_pack_rows_var: a read that ends early keeps max(min(read_len - offset, length), min_length) bases,
    none when that range passes the end of the read; the word holds the L bases, quality bytes beyond L are 0"""
    n, stride = seq_rows.shape
    rl = np.minimum(np.asarray(read_len, np.int64), stride)
    L = np.maximum(np.minimum(np.maximum(rl - offset, 0), length), min_length)
    L[offset + L > rl] = 0
    key, qualn = np.zeros(n, np.uint32), np.zeros((n, length), np.uint8)
    for j in range(length):
        b, q = seq_rows[:, offset + j], qual_rows[:, offset + j]
        on = j < L
        key = np.where(on, (key << np.uint32(2)) | _CODE[b], key).astype(np.uint32)
        qualn[:, j] = np.where(on, np.minimum(q, 127) | np.where(_IS_N[b], 0x80, 0), 0)
    return key, qualn, L.astype(np.uint8)


PACK_ALPHABET = b"ACGTNacgtn.-RYKM\0\xff*"


def pack_reads(n, L, seed):
    rng = np.random.default_rng(seed)
    p = np.full(len(PACK_ALPHABET), 0.1 / (len(PACK_ALPHABET) - 4))
    p[:4] = 0.9 / 4
    seq = rng.choice(np.frombuffer(PACK_ALPHABET, np.uint8), size=(n, L), p=p)
    qual = rng.integers(0, 256, size=(n, L), dtype=np.uint8)
    return seq, qual


def byte_value_blocks(L, what):
    """256 reads per base position whose byte at that position (of the bases, or of the qualities) runs through 0..255"""
    n = 256 * L
    seq = np.tile(np.frombuffer(b"ACGT", np.uint8), (n, (L + 3) // 4))[:, :L].copy()
    qual = np.full((n, L), ord("I"), np.uint8)
    tgt = seq if what == "base" else qual
    for p in range(L):
        tgt[256 * p:256 * (p + 1), p] = np.arange(256, dtype=np.uint8)
    for p in range(L):                                   # the claim: every value at every position
        assert len(np.unique(tgt[:, p])) == 256
    return seq, qual


PACK_VAR_STRIDE = 40


def pack_var_triples(stride=PACK_VAR_STRIDE):
    return [(16, 12, 10), (16, 12, 12), (0, 16, 1), (20, 8, 8), (stride - 16, 16, 3)]


def pack_var_rows(stride=PACK_VAR_STRIDE, per_len=6, seed=507):
    """rows for every read_len in 0..stride + 2; the bytes behind the read's end hold bases too, so a kernel that reads past
    the end packs something other than nothing"""
    seq, qual = pack_reads((stride + 3) * per_len, stride, seed)
    read_len = np.repeat(np.arange(stride + 3, dtype=np.uint32), per_len)
    assert set(read_len.tolist()) == set(range(stride + 3))
    return seq, qual, read_len


# ---- shard metrics ----------------------------------------------------------------------------------------------------------------
def _filler(L, shift=0):
    return bytes(b"ACGT"[(i + shift) % 4] for i in range(L))


def shard_reads(cb_len, umi_len):
    """(cb, cb_qual, umi, umi_qual as (n, L) ASCII arrays, classes): the read classes of group F at one length pair; every class
    shapes the barcode and the UMI alike, each at its own length"""
    reads, classes = [], {}

    def add(klass, cb, cbq, umi, uq):
        assert len(cb) == len(cbq) == cb_len and len(umi) == len(uq) == umi_len
        classes[klass] = classes.get(klass, 0) + 1
        reads.append((cb, cbq, umi, uq))

    def both(klass, f, fq=None):
        fq = fq or (lambda L: b"I" * L)
        add(klass, f(cb_len), fq(cb_len), f(umi_len), fq(umi_len))
    hi = max(cb_len, umi_len)
    both("all_n", lambda L: b"N" * L)
    for p in range(hi):
        both("one_n", lambda L: _filler(L)[:p] + b"N" + _filler(L)[p + 1:] if p < L else _filler(L, 1))
    for b in b"ACGT":
        both("homopolymer", lambda L: bytes([b]) * L)
        o = b"ACGT"[(b"ACGT".index(b) + 1) % 4]
        for p in range(hi):
            both("broken_homopolymer", lambda L: (bytes([b]) * p + bytes([o]) + bytes([b]) * L)[:L] if p < L else bytes([b]) * L)
    for q in [33 + x for x in (0, 1, 2, 3, 9, 10, 29, 30)] + [32, 127]:
        both("quality_%d" % q, _filler, lambda L: bytes([q]) * L)
    for q in (42, 43, 32, 34, 36):
        for p in range(hi):
            both("min_quality_at", _filler, lambda L: (b"I" * p + bytes([q]) + b"I" * L)[:L] if p < L else b"I" * L)
    for p in range(hi):                                  # Q30: one base below 63 among bases at 63
        both("q30_at", _filler, lambda L: (b"?" * p + b">" + b"?" * L)[:L] if p < L else b"?" * L)

    def umi_tail(klass, tail, head=b"A"):
        u = (head * 16 + tail)[-umi_len:]
        add(klass, _filler(cb_len), b"I" * cb_len, u, b"I" * umi_len)
    umi_tail("polyt", b"TTTTT")
    umi_tail("polyt", b"TTTTT", head=b"T")
    umi_tail("polyt", b"TTTTT", head=b"G")
    for k in range(5):
        for o in b"ACG":
            umi_tail("polyt_four", b"TTTTT"[:k] + bytes([o]) + b"TTTTT"[k + 1:], head=b"T")
        umi_tail("polyt_n", b"TTTTT"[:k] + b"N" + b"TTTTT"[k + 1:], head=b"T")
    umi_tail("polyt_n_before", b"NTTTTT", head=b"T")
    want = {"all_n": 1, "one_n": hi, "homopolymer": 4, "broken_homopolymer": 4 * hi, "min_quality_at": 5 * hi, "q30_at": hi,
            "polyt": 3, "polyt_four": 15, "polyt_n": 5, "polyt_n_before": 1}
    for k, v in want.items():
        assert classes[k] == v, (k, classes[k], v)
    arr = [np.frombuffer(b"".join(r[k] for r in reads), np.uint8).reshape(len(reads), -1) for k in range(4)]
    return arr[0], arr[1], arr[2], arr[3], classes


def shard_idx(n):
    """pass A's output with misses: every third read"""
    idx = np.arange(n, dtype=np.uint32) * 7 + 1
    idx[::3] = MISS
    return idx


def shard_zero_reads(n=300):
    """reads that leave eight counters at exactly 0 (the `if (t)` skip of k_shard_metrics): no N, no homopolymer, high
    qualities, no T suffix, every barcode on the list"""
    cb = np.frombuffer(_filler(16) * n, np.uint8).reshape(n, 16).copy()
    umi = np.frombuffer(_filler(12, 1) * n, np.uint8).reshape(n, 12).copy()
    umi[:, 0] = np.frombuffer(b"ACGT", np.uint8)[np.arange(n) % 4]
    return cb, np.full((n, 16), ord("I"), np.uint8), umi, np.full((n, 12), ord("I"), np.uint8)


SHARD_ZERO_FIELDS = ("bc_n_bases", "umi_n_bases", "has_n_barcode", "has_n_umi", "homopolymer_barcode", "homopolymer_umi",
                     "low_min_qual_barcode", "low_min_qual_umi", "miss_whitelist_barcode", "polyt_suffix_umi")


def shard_random_reads(n, cb_len, umi_len, seed=508):
    rng = np.random.default_rng(seed)
    al = np.frombuffer(b"ACGTN", np.uint8)
    p = [0.245, 0.245, 0.245, 0.245, 0.02]
    cb, umi = rng.choice(al, size=(n, cb_len), p=p), rng.choice(al, size=(n, umi_len), p=p)
    qs = np.array([32, 33, 35, 36, 42, 43, 62, 63, 73, 127], np.uint8)
    pq = [0.005, 0.005, 0.01, 0.01, 0.01, 0.02, 0.04, 0.1, 0.79, 0.01]
    cbq, uq = rng.choice(qs, size=(n, cb_len), p=pq), rng.choice(qs, size=(n, umi_len), p=pq)
    k = n // 50
    umi[:k, -5:] = ord("T")                              # T suffixes and homopolymers are too rare by chance
    cb[k:2 * k] = cb[k:2 * k, :1]
    umi[2 * k:3 * k] = umi[2 * k:3 * k, :1]
    return cb, cbq, umi, uq


# ---- rows metrics and homopolymers ---------------------------------------------------------------------------------------------
_LOW_Q = bytes(range(0, 36))        # q > 2 + 33 fails
_BELOW_Q30 = bytes(range(0, 63))    # q >= 30 + 33 fails


def rows_metrics_ref(seq_rows, qual_rows, lens, stride):
    """Python counting over the bytes of every row: only the letter N counts as an N base"""
    out = dict(n_bases=0, bases=0, q30_bases=0, q30_den=0)
    for r in range(len(seq_rows)):
        L = stride if lens is None else min(int(lens[r]), stride)
        s, q = seq_rows[r, :L].tobytes(), qual_rows[r, :L].tobytes()
        out["n_bases"] += s.count(b"N")
        out["bases"] += len(s)
        out["q30_den"] += len(q.translate(None, _LOW_Q))
        out["q30_bases"] += len(q.translate(None, _BELOW_Q30))
    return out


def homopolymer_ref(r1, l1, s1, run_len, r2=None, l2=None, s2=0):
    """reads whose R1 or R2 holds run_len equal bases in a row, per base: the `in` operator on bytes"""
    out = dict.fromkeys("ACGT", 0)
    for r in range(len(r1)):
        a = r1[r, :s1 if l1 is None else min(int(l1[r]), s1)].tobytes()
        b = b"" if r2 is None else r2[r, :s2 if l2 is None else min(int(l2[r]), s2)].tobytes()
        for ch in "ACGT":
            pat = ch.encode() * run_len
            out[ch] += (pat in a) or (pat in b)
    return out


ROWS_LENGTHS = (0, 1, 63, 64, 65, 127, 128, 129)
ROWS_STRIDE = 160


def rows_metrics_rows(n_random=0, stride=ROWS_STRIDE, seed=509):
    """rows of the named lengths, of the stride and of a length above it; behind a row's end the buffer holds N and high
    qualities, which count only when the lengths are ignored"""
    rng = np.random.default_rng(seed)
    lens = list(ROWS_LENGTHS) + [stride, stride + 40] + [int(x) for x in rng.integers(0, stride + 20, size=n_random)]
    n = len(lens)
    seq = rng.choice(np.frombuffer(b"ACGTNn.", np.uint8), size=(n, stride), p=[0.2, 0.2, 0.2, 0.2, 0.1, 0.05, 0.05])
    qual = rng.choice(np.array([0, 33, 35, 36, 37, 62, 63, 64, 73, 126, 127, 200, 255], np.uint8), size=(n, stride))
    lens = np.array(lens, np.uint32)
    for r in range(n):
        seq[r, min(int(lens[r]), stride):] = ord("N")
        qual[r, min(int(lens[r]), stride):] = ord("I")
    return seq, qual, lens


HP_RUN_LENS = (2, 3, 15, 16, 17, 32, 33, 63, 64)


def _hp_row(L, base, start, run, stride, fill=0):
    """a row of L bytes cycling over the three other bases, `run` bytes of `base` from `start`; `fill` behind L"""
    others = bytes(b for b in b"ACGT" if b != base)
    row = bytearray(others[i % 3] for i in range(L))
    row[start:start + run] = bytes([base]) * run
    assert len(row) == L
    return bytes(row) + bytes([fill]) * (stride - L)


def hp_positive_case(run_len, exact_end):
    """one row per base and per start 0..L - run_len; L spans three windows, and with exact_end the third window holds exactly
    the start of the run that ends at L.  Every row counts for its base alone."""
    step = hp_step(run_len)
    L = 2 * step + run_len + (0 if exact_end else 5)
    stride = L + 3
    rows, starts = [], list(range(L - run_len + 1))
    for base in b"ACGT":
        rows += [_hp_row(L, base, s, run_len, stride) for s in starts]
    claims = dict(windows_min=3, last_start_of_window0=HP_WINDOW - run_len, first_start_of_window1=step, run_ends_at_L=True)
    if exact_end:
        claims["last_window_starts_at"] = L - run_len
    return Case("hp_pos_%d_%d" % (run_len, exact_end), claims, rows=np.frombuffer(b"".join(rows), np.uint8).reshape(-1, stride),
                lens=np.full(len(rows), L, np.uint32), stride=stride, L=L, run_len=run_len, expect=dict.fromkeys("ACGT", len(starts)))


def check_hp_positive(case):
    """from the bytes: every row holds exactly one run of its base, of exactly run_len, and the starts are all of 0..L - run_len"""
    L, k = case.L, case.run_len
    step = hp_step(k)
    windows = list(range(0, L - k + 1, step))
    per_base = {}
    for row in case.rows:
        s = row[:L].tobytes()
        hits = [(ch, s.find(bytes([ch]) * k)) for ch in b"ACGT" if bytes([ch]) * k in s]
        assert len(hits) == 1
        ch, at = hits[0]
        assert bytes([ch]) * (k + 1) not in s and s.count(bytes([ch])) == k
        per_base.setdefault(ch, []).append(at)
    for ch in b"ACGT":
        assert per_base[ch] == list(range(L - k + 1))
    c = case.claims
    assert len(windows) >= c["windows_min"]
    assert c["last_start_of_window0"] == max(s for s in per_base[65] if s + k <= HP_WINDOW)
    assert c["first_start_of_window1"] == windows[1] == min(s for s in per_base[65] if s + k > HP_WINDOW)
    assert (L - k in per_base[65]) == c["run_ends_at_L"]
    if "last_window_starts_at" in c:
        assert windows[-1] == c["last_window_starts_at"] == L - k
    if k == 15:
        assert c["last_start_of_window0"] == 49 and c["first_start_of_window1"] == 50
    return windows


def hp_near_miss_case(run_len):
    """rows that must count 0: runs of run_len - 1 at every start; runs of run_len + 1 broken in the middle by an N and by
    another base; a run that only bytes behind the row's length would complete (the buffer holds the base there)"""
    step = hp_step(run_len)
    L = 2 * step + run_len + 5
    stride = L + run_len + 3
    rows, lens = [], []
    for base in b"ACGT":
        if run_len > 2:
            for s in range(L - run_len + 2):
                rows.append(_hp_row(L, base, s, run_len - 1, stride))
                lens.append(L)
        for s in sorted(set([0, step - 1, step, L - run_len - 1]) if run_len < 63 else set(range(L - run_len))):
            for breaker in (ord("N"), b"ACGT"[(b"ACGT".index(base) + 2) % 4]):
                r = bytearray(_hp_row(L, base, s, run_len + 1, stride))
                r[s + run_len // 2] = breaker
                if run_len == 2:                             # X b X: runs of 1
                    r[s:s + 3] = bytes([base, breaker, base])
                rows.append(bytes(r))
                lens.append(L)
        for s in sorted(set([0, step - 1, step, 2 * step, L - run_len])):
            cut = s + run_len - 1                            # the row ends one byte before the run does
            r = bytearray(_hp_row(cut, base, s, run_len - 1, stride, fill=base))
            rows.append(bytes(r))
            lens.append(cut)
    return Case("hp_miss_%d" % run_len, dict(beyond_len_completes=True), rows=np.frombuffer(b"".join(rows), np.uint8).reshape(-1, stride),
                lens=np.array(lens, np.uint32), stride=stride, L=L, run_len=run_len, expect=dict.fromkeys("ACGT", 0))


def check_hp_near_miss(case):
    k = case.run_len
    n_beyond = 0
    for row, L in zip(case.rows, case.lens):
        s, whole = row[:L].tobytes(), row.tobytes()
        for ch in b"ACGT":
            assert bytes([ch]) * k not in s
            n_beyond += bytes([ch]) * k in whole
    assert n_beyond >= 4 * 4, "no row whose run completes behind its length"
    assert homopolymer_ref(case.rows, None, case.stride, k) != case.expect      # ignoring the lengths would count
    longest = max(len(m.group(0)) for row, L in zip(case.rows, case.lens) for m in re.finditer(rb"A+|C+|G+|T+", row[:L].tobytes()))
    assert longest == k - 1
    return n_beyond


def hp_edge_rows(run_len):
    """(rows, lens, stride, expected): L == run_len (counts), L == run_len - 1 (does not), a length above the stride (clamped)"""
    stride = run_len + 2
    rows = [b"G" * run_len + b"\0\0", b"G" * (run_len - 1) + b"\0\0\0", b"C" * stride, b"T" * stride, b"A" * run_len + b"AA"]
    lens = [run_len, run_len - 1, stride + 9, run_len, run_len - 1]
    exp = dict(A=0, C=1, G=1, T=1)
    return np.frombuffer(b"".join(rows), np.uint8).reshape(-1, stride), np.array(lens, np.uint32), stride, exp


def hp_pair_case(run_len=15, s1=70, s2=45):
    """R1 / R2 with the run in R2 only, in both, in R1 only and in neither; R2's stride differs from R1's"""
    r1, r2, l1, l2 = [], [], [], []
    for k, (in1, in2) in enumerate([(0, 1), (1, 1), (1, 0), (0, 0)] * 5):
        base = b"ACGT"[(k // 4) % 4]
        L1, L2 = 60 + k % 7, 30 + k % 11
        r1.append(_hp_row(L1, base, 3 + k, run_len if in1 else run_len - 1, s1))
        r2.append(_hp_row(L2, base, k % 9, run_len if in2 else run_len - 1, s2))
        l1.append(L1)
        l2.append(L2)
    return (np.frombuffer(b"".join(r1), np.uint8).reshape(-1, s1), np.array(l1, np.uint32),
            np.frombuffer(b"".join(r2), np.uint8).reshape(-1, s2), np.array(l2, np.uint32))
