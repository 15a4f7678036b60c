"""Builds and runs tests/cpp/test_pca_kernels.hip: the kernels of cellranger_amd/csrc/pca.hip and the host functions that launch
them (pca_prepare, pca_scale, PcaLanczos), called directly at constructed shapes.

The program includes pca.hip inside a namespace and is compiled with cellranger_amd.build.FLAGS: it runs the same text under the
same flags, not the library's object code.  The context, the pool and the radix sort come from libcrgpu.so.

Every f64 output has two references: a host loop that takes the device's steps in its order (a lane's chain, the butterfly
32 .. 1, the partials ascending), which must agree bit for bit, and a long double sum in index order written from the definition,
from which the device may differ by gamma(d + 1) * sum |terms| for d additions on the longest path (plus the reference's own
2^-64 part); the derivations stand beside the checks.  Case sizes hang on PCA_WG, PCA_PART_ROWS and PCA_PROJ_CHUNK, which the
program reads through the include.

The one value that cannot be bit-equal is log2(1 + count * factor) of k_pca_fill (OCML's log2, not libm's); count * factor itself
is checked bit for bit in the unlogged mode.  Measured on the CPU over every logged preparation of the program (--host-only asserts
both figures on every entry):
    libm's log2(1.0 + x) lies at most 86 ulps from the rounded log2l(1.0L + x)   -> the device may lie 4 * 86 = 344 ulps from it.
        (The 86 are the rounding of the f64 sum 1.0 + x, which numpy and the device both do: about 2^-53 / (x ln 2) of a
        small logarithm.)
    libm's log2(1.0 + x) lies at most 1 ulp from the rounded log2l of that f64 sum -> the device may lie 4 ulps from it.
A float intermediate is 2^29 ulps off, log1p or log2 of the wrong argument more.  Every later check starts from the device's own
downloaded values, so these ulps reach no other comparison.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cellranger_amd")


def _build(out_dir):
    from cellranger_amd import build

    exe = os.path.join(str(out_dir), "test_pca_kernels")
    cmd = [build.HIPCC] + build.FLAGS + ["-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"),
                                         os.path.join(ROOT, "tests", "cpp", "test_pca_kernels.hip"), "-L" + PKG, "-lcrgpu", "-pthread",
                                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The program, built once for all groups."""
    return _build(tmp_path_factory.mktemp("pca_kernels"))


def _run(exe, args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "all tests passed" in r.stdout, "\n".join(out.splitlines()[-40:])
    print("\n".join(line for line in r.stdout.splitlines() if not line.startswith("ok ")))  # the worst deviation-to-bound ratios
    return r.stdout


# the extern "C" host functions of pca.hip: they keep their names inside the namespace, libcrgpu.so defines them too, so the linker
# exports the program's copies (the same text; the program calls none of them)
_EXPORTED = {"crgpu_legacy_randn", "crgpu_normalized_dispersion", "crgpu_pca_dev", "crgpu_small_svd"}


def test_pca_kernels_compile_and_the_references_agree(tmp_path):
    """CPU: pca.hip compiles inside the namespace for gfx950 and links against the library as built from this tree; on every
    case the order model lies within the derived bound of the long double reference, and libm's log2 within the two figures of
    the module docstring.  The program's dynamic symbol table holds no k_pca_* symbol that could interpose the library's
    kernels, and of the library's crgpu_* / cr_* names exactly the four host functions of pca.hip."""
    from cellranger_amd import build

    build.build()
    exe = _build(tmp_path)
    out = _run(exe, ["--host-only"])
    assert out.count("(host only)") >= 70 and "group project" in out
    nm = subprocess.run(["nm", "-D", "--defined-only", exe], capture_output=True, text=True, check=True).stdout
    names = [line.split()[-1] for line in nm.splitlines() if line.strip()]
    assert names and not [n for n in names if "k_pca_" in n]
    assert {n for n in names if n.startswith(("crgpu_", "cr_"))} == _EXPORTED


@pytest.mark.gpu
def test_pca_kernels_prepare(exe):
    """pca_prepare and pca_scale at 64, 128 and 256 threads, then each kernel of the preparation by direct launch of two
    workgroups into guarded buffers: column lengths around 64 and its multiples, a feature map with holes inside a chunk of the
    compaction, a column subset, F on 255 / 256 / 257, F * N on and beside a power of two, medians with ties, of an even count
    and of mostly empty columns, and more columns than the grid has waves.  k_pca_feature_counts against the host's histogram
    over a column subset, with rows at and above G, sums above 2^32 and 1, 2 and the stage's number of workgroups."""
    _run(exe, ["--group", "prepare"])


@pytest.mark.gpu
def test_pca_kernels_operator(exe):
    """k_pca_av and k_pca_atw through PcaLanczos (the scalars from the dot kernels) and by direct launch of 1 and 3 workgroups:
    normal, twelve-decade and unit vectors, rows and features without entries, <A v, w> = <v, A^T w>."""
    _run(exe, ["--group", "operator"])


@pytest.mark.gpu
def test_pca_kernels_dense(exe):
    """k_pca_dots + k_pca_dots_finish for n = 1 .. 769, 1 .. PCA_MAX_MB columns, 1, 2, 3 and 64 partials a workgroup, ld = n + 7
    with NaN in the padding; k_pca_update, k_pca_axpy, k_pca_scal, k_pca_fill_ones; k_pca_small_product in place and direct."""
    _run(exe, ["--group", "dense"])


@pytest.mark.gpu
def test_pca_kernels_project(exe):
    """k_pca_project for 1 .. 128 components, rows of 0, 1, 64, 65 and 200 entries, a feature map with holes and a row with
    nothing mapped, 64 and 256 threads, the stage's grid and one workgroup."""
    _run(exe, ["--group", "project"])
