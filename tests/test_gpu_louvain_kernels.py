"""Builds and runs tests/cpp/test_louvain_kernels.hip: the kernels of cellranger_amd/csrc/louvain.hip by direct launch into guarded
buffers at constructed shapes.

The program includes louvain.hip inside a namespace and is compiled with cellranger_amd.build.FLAGS: it runs the same text under the
same flags, not the library's object code.  The context, the pool, the scan and the radix sort come from libcrgpu.so.

Everything in louvain.hip is an integer, so every comparison with the program's host order model is bit for bit: the labels, tot, size
and the count of moves a round writes, both sums of S, the decision and the latch, the class lists, the union, the structure check,
the degrees, the dense renumbering, the composition and the aggregation."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cellranger_amd")


def _build(out_dir):
    from cellranger_amd import build

    exe = os.path.join(str(out_dir), "test_louvain_kernels")
    cmd = [build.HIPCC] + build.FLAGS + ["-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"),
                                         os.path.join(ROOT, "tests", "cpp", "test_louvain_kernels.hip"), "-L" + PKG, "-lcrgpu", "-pthread",
                                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The program, built once for all groups."""
    from cellranger_amd import build

    build.build()
    return _build(tmp_path_factory.mktemp("louvain_kernels"))


def _run(exe, args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "all tests passed" in r.stdout, "\n".join(out.splitlines()[-40:])
    print("\n".join(line for line in r.stdout.splitlines() if not line.startswith("ok ")))
    return r.stdout


# the extern "C" entry points of louvain.hip keep their names inside the namespace, libcrgpu.so defines them too, so the linker exports
# the program's copies (the same text; the program calls none of them)
_EXPORTED = {"crgpu_louvain_dev", "crgpu_modularity"}


def test_louvain_kernels_compile_and_the_order_model_holds():
    """CPU: louvain.hip compiles inside the namespace for gfx950 and links against the library as built from this tree; on every case
    the host order model gives the hand-computed values (two triangles: S = 70 after two rounds, a third is discarded; both ties; the
    singleton rule on one edge), its tot add up to M and its S is the dense matrix's; every branch was taken.  The program's dynamic
    symbol table holds no k_lv_* symbol that could interpose the library's kernels, and of the library's crgpu_* / cr_* names exactly
    the two entry points of louvain.hip."""
    import tempfile

    from cellranger_amd import build

    build.build()
    with tempfile.TemporaryDirectory() as d:
        exe = _build(d)
        out = _run(exe, ["--host-only"])
        assert out.count("(host only)") >= 40
        counts = [int(v) for v in __import__("re").search(r"branches: (\d+) ties of own and another, (\d+) ties of two others, (\d+) dropped proposals, "
                                                            r"(\d+) rows with one label", out).groups()]
        assert all(c > 0 for c in counts), counts
        nm = subprocess.run(["nm", "-D", "--defined-only", exe], capture_output=True, text=True, check=True).stdout
        names = [line.split()[-1] for line in nm.splitlines() if line.strip()]
        assert names and not [n for n in names if "k_lv_" in n]
        assert {n for n in names if n.startswith(("crgpu_", "cr_"))} == _EXPORTED


@pytest.mark.gpu
def test_louvain_kernels_round(exe):
    """k_lv_prep, k_lv_round in its three classes, k_lv_inside, k_lv_squares and k_lv_decide from crafted labels: two triangles through
    their three rounds; a tie on G between the own community and another and between two others; the singleton rule; a star whose
    leaves share one label; a hub row of n - 1 entries at n = 63 / 65 / 257 under the thresholds 127 / 2047, 4 / 16 and 4 / 2; weights
    near 2^28 (M = 2^31 - 2); rows of exactly 127, 128, 2047 and 2048 entries (and 5, 6, 9, 10; 63, 64, 65) at the class boundaries;
    the class lists by the compaction; fewer device tables than rows that need one; a latched round and decision write nothing."""
    _run(exe, ["--group", "round"])


@pytest.mark.gpu
def test_louvain_kernels_levels(exe):
    """k_lv_keys, the library's sort, the run heads and k_keys_to_csr (the union, with rows that name themselves) at n = 63 / 64 / 65 / 255 /
    257 / 300 / 1100; k_lv_check on the union and on a swapped pair, a weight of 0, an unequal twin; k_lv_degrees; k_lv_identity and
    k_lv_begin; the dense renumbering with unused ids, k_lv_compose; k_lv_agg_keys, the sort with its payload, k_lv_run_sums and the
    CSR of the aggregated graph, down to two communities (runs of tens of thousands of keys)."""
    _run(exe, ["--group", "levels"])


@pytest.mark.gpu
def test_louvain_kernels_csr(exe):
    """k_keys_to_csr of graph_common.h, the kernel tsne.hip, umap.hip and louvain.hip share, through its launch helper on hand-made sorted
    distinct keys against a host loop, exact integers, guarded buffers, each with and without the weights pointer: n = 5 with entries in
    rows 1 and 3 only (empty rows at the start, in the middle and at the end; 3 entries, so the grid is sized by n + 1); n = 2 with
    every cell; n = 300 with one row of 257 entries and one entry in every other row (more entries than n + 1 and than a workgroup has
    threads)."""
    _run(exe, ["--group", "csr"])
