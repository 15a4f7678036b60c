"""Builds and runs tests/cpp/test_perturbation_kernels.hip: the two kernels of the MEASURE_PERTURBATIONS bootstrap by direct launch into
guarded buffers.

The program includes csrc/perturbations.h inside a namespace and is compiled with cellranger_amd.build.FLAGS: it runs the same text
under the same flags, not the library's object code.  The context and the pool come from libcrgpu.so.  The sums are integers, so the
device must equal the host model; there is no bound.

k_pb_draws: columns of 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, lds_cells and lds_cells + 1 cells, a column of zeros, a column with a
count in every cell, five cells of 2^31 - 1; each launch through the LDS path (lds_cells = 300) and through the global path (lds_cells
= 1); B in {1, 2, 9} with 1, 4 and 8 draws per workgroup.  The host model walks the positions in order with a host Philox4x64-10 that is
checked against words recorded from numpy.
k_pb_gather: a gene with 0, 1, 64, 65 and 130 entries in the group, the first and last gene and group, a gene present only outside the
group; the pool is filled with 0xFF first, so a word left unwritten shows."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cellranger_amd")


def _build(out_dir):
    from cellranger_amd import build

    exe = os.path.join(str(out_dir), "test_perturbation_kernels")
    cmd = [build.HIPCC] + build.FLAGS + ["-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"),
                                         os.path.join(ROOT, "tests", "cpp", "test_perturbation_kernels.hip"), "-L" + PKG, "-lcrgpu", "-pthread",
                                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The program, built once for both groups."""
    return _build(tmp_path_factory.mktemp("perturbation_kernels"))


def _run(exe, args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "all tests passed" in r.stdout, "\n".join(out.splitlines()[-40:])
    return r.stdout


# the extern "C" functions of the included text keep their names inside the namespace, libcrgpu.so defines them too, so the linker
# exports the program's copies (the same text; the program calls none of them).  The entry points that take the opaque types the
# included text defines are renamed by the program and are not among them
_EXPORTED = {"crgpu_sseq_adjust_bh", "crgpu_perturbation_ci"}


def test_perturbation_kernels_compile_and_the_host_model_agrees_with_numpy(tmp_path):
    """CPU: the text compiles inside the namespace for gfx950 and links against the library as built from this tree; the host Philox
    gives the words numpy recorded, every constructed shape is what it is for.  The program's dynamic symbol table holds no kernel
    that could interpose the library's."""
    from cellranger_amd import build

    build.build()
    exe = _build(tmp_path)
    out = _run(exe, ["--host-only"])
    assert out.count("(host only)") == 1 + 18 + 1
    nm = subprocess.run(["nm", "-D", "--defined-only", exe], capture_output=True, text=True, check=True).stdout
    names = [line.split()[-1] for line in nm.splitlines() if line.strip()]
    assert names and not [n for n in names if "k_sq_" in n or "k_pb_" in n]
    assert {n for n in names if n.startswith(("crgpu_", "cr_"))} == _EXPORTED


@pytest.mark.gpu
def test_perturbation_kernels_draws(exe):
    """k_pb_draws at the constructed sizes, both paths, every (B, draws per workgroup): the device equals the host model."""
    out = _run(exe, ["--group", "draws"])
    assert out.count("ok   k_pb_draws") == 18 and "(host only)" not in out


@pytest.mark.gpu
def test_perturbation_kernels_gather(exe):
    """k_pb_gather at the constructed run lengths: every word of every column equals the dense column built on the host."""
    out = _run(exe, ["--group", "gather"])
    assert out.count("ok   k_pb_gather") == 1 and "(host only)" not in out
