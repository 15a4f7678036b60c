"""Builds and runs tests/cpp/test_merge_kernels.hip: the two kernels of MERGE_CLUSTERS by direct launch into guarded buffers.

The program includes csrc/sseq_pair.h and csrc/merge_clusters.hip inside namespaces and is compiled with cellranger_amd.build.FLAGS: it
runs the same text under the same flags, not the library's object code.  The context and the pool come from libcrgpu.so.

k_sq_pair_row_sums: side a of 1, 2 and 3 groups holding exactly 0, 1, 63, 64, 65, 127, 128 and 129 entries of a gene, a gene in no cell,
a gene only outside the pair, the first and the last gene and group.  Bit for bit against a host order model (lane = concatenated index
% 64, ascending within a lane, the butterfly 32 .. 1); against a long double sum within gamma(n / 64 + 7) * sum |terms| (the derivation
stands beside the check in the program); x_a and x_b equal as integers.
k_mc_median: segments of 1, 2, 3, 255, 256, 257 and 4097 values that are all equal, differ in the lowest byte only, in the sign only,
are negative, denormal, -0 / +0 or normal: equal to std::nth_element."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cellranger_amd")


def _build(out_dir):
    from cellranger_amd import build

    exe = os.path.join(str(out_dir), "test_merge_kernels")
    cmd = [build.HIPCC] + build.FLAGS + ["-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"),
                                         os.path.join(ROOT, "tests", "cpp", "test_merge_kernels.hip"), "-L" + PKG, "-lcrgpu", "-pthread",
                                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The program, built once for both groups."""
    return _build(tmp_path_factory.mktemp("merge_kernels"))


def _run(exe, args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "all tests passed" in r.stdout, "\n".join(out.splitlines()[-40:])
    print("\n".join(line for line in r.stdout.splitlines() if not line.startswith("ok ")))
    return r.stdout


# the extern "C" functions of the included text keep their names inside the namespaces, libcrgpu.so defines them too, so the linker
# exports the program's copies (the same text; the program calls none of them).  The entry points that take the opaque types the
# included text defines are renamed by the program and are not among them
_EXPORTED = {"crgpu_sseq_adjust_bh", "crgpu_cluster_medians_dev", "crgpu_linkage_complete"}


def test_merge_kernels_compile_and_the_references_agree(tmp_path):
    """CPU: the two files compile inside the namespaces for gfx950 and link against the library as built from this tree; on every case
    the order model lies within the derived bound of the long double reference and the host twin of the radix select equals
    std::nth_element.  The program's dynamic symbol table holds no kernel that could interpose the library's."""
    from cellranger_amd import build

    build.build()
    exe = _build(tmp_path)
    out = _run(exe, ["--host-only"])
    assert out.count("(host only)") == 9 + 8 and "group pair" in out
    nm = subprocess.run(["nm", "-D", "--defined-only", exe], capture_output=True, text=True, check=True).stdout
    names = [line.split()[-1] for line in nm.splitlines() if line.strip()]
    assert names and not [n for n in names if "k_sq_" in n or "k_mc_" in n]
    assert {n for n in names if n.startswith(("crgpu_", "cr_"))} == _EXPORTED


@pytest.mark.gpu
def test_merge_kernels_pair(exe):
    """k_sq_pair_row_sums at the constructed run lengths: the device equals the order model bit for bit and lies within the bound."""
    out = _run(exe, ["--group", "pair"])
    assert out.count("ok   k_sq_pair_row_sums") == 9


@pytest.mark.gpu
def test_merge_kernels_select(exe):
    """k_mc_median at the constructed segment sizes and value kinds: the device equals std::nth_element."""
    out = _run(exe, ["--group", "select"])
    assert out.count("ok   k_mc_median") == 7
