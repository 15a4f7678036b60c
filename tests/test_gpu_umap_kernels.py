"""Builds and runs tests/cpp/test_umap_kernels.hip: the kernels of cellranger_amd/csrc/umap.hip by direct launch into guarded buffers
at constructed shapes.

The program includes umap.hip inside a namespace and is compiled with cellranger_amd.build.FLAGS: it runs the same text under the same
flags, not the library's object code.  The context, the pool, the scan and the radix sort come from libcrgpu.so.

What holds + - * /, floor and integers only (rho, the row sums and their total, the steps and the mid of the search, the keys, the
union from the device's own memberships, wmax, the prune, the CSR; in an epoch both schedule states, the two counters and the sampled
vertices) must equal a host order model bit for bit.  exp (the memberships, psum at the device's own sigma) and pow (delta, Y') are
OCML's: they are compared against long double with bounds derived in the program from OCML's documented 1 ulp and Higham's gamma; the
program prints the worst ratio (the README quotes the device's).  On the host the order model's delta comes to 0.145 of its bound at
the worst (--host-only)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cellranger_amd")


def _build(out_dir):
    from cellranger_amd import build

    exe = os.path.join(str(out_dir), "test_umap_kernels")
    cmd = [build.HIPCC] + build.FLAGS + ["-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"),
                                         os.path.join(ROOT, "tests", "cpp", "test_umap_kernels.hip"), "-L" + PKG, "-lcrgpu", "-pthread",
                                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The program, built once for all groups."""
    from cellranger_amd import build

    build.build()
    return _build(tmp_path_factory.mktemp("umap_kernels"))


def _run(exe, args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "all tests passed" in r.stdout, "\n".join(out.splitlines()[-40:])
    print("\n".join(line for line in r.stdout.splitlines() if not line.startswith("ok ")))  # the worst deviation-to-bound ratios
    return r.stdout


# the extern "C" entry points of umap.hip keep their names inside the namespace, libcrgpu.so defines them too, so the linker exports
# the program's copies (the same text; the program calls none of them)
_EXPORTED = {"crgpu_umap_ab", "crgpu_umap_graph_dev", "crgpu_umap_epochs_dev"}


def test_umap_kernels_compile_and_the_order_model_is_within_its_bound(exe):
    """CPU: umap.hip compiles inside the namespace for gfx950 and links against the library as built from this tree; on every case the
    order model lies within the derived bound of the long double reference and every branch (d2 = 0, a self-sample, a clipped term,
    n_neg of 0, of 15 and held to 16) was taken.  The program's dynamic symbol table holds no k_umap_* symbol that could interpose the
    library's kernels, and of the library's crgpu_* / cr_* names exactly the three entry points of umap.hip."""
    out = _run(exe, ["--host-only"])
    assert out.count("(host only)") >= 28 and "branches: d2 = 0" in out
    nm = subprocess.run(["nm", "-D", "--defined-only", exe], capture_output=True, text=True, check=True).stdout
    names = [line.split()[-1] for line in nm.splitlines() if line.strip()]
    assert names and not [n for n in names if "k_umap_" in n]
    assert {n for n in names if n.startswith(("crgpu_", "cr_"))} == _EXPORTED


@pytest.mark.gpu
def test_umap_kernels_graph(exe):
    """k_umap_rows, the 256-row partials, k_umap_search, k_pair_keys, the library's sort, the union, wmax, the prune and k_keys_to_csr at
    N = 63 / 64 / 65 / 255 / 257 with K = 3, at K = 29 and at K = 1024: a row of zeros (rho 0, 64 steps, the all-distances floor), a row
    with leading zeros, a row that is named by none it names; psum and every membership in long double at the device's own sigma."""
    _run(exe, ["--group", "graph"])


@pytest.mark.gpu
def test_umap_kernels_epoch(exe):
    """k_umap_epoch from a crafted state (entries that are not active, n_neg of 0, 1, 5, 15 and a state that asks for more than the 16
    words an entry owns) at N = 63 / 64 / 65 / 255 / 257, 2 and 3 dimensions: a hub row of N - 1 entries beside rows of 2 and 3; rows
    of 0 and 1 entries; rows of T - 1, T and T + 1 entries under wave thresholds of T - 1 .. T + 2, 1 and beyond every row, workgroups
    of 64, 128 and 256 threads; coincident rows; every setting equal bit for bit; umap_sample against the host's Philox; the schedule's
    start."""
    _run(exe, ["--group", "epoch"])
