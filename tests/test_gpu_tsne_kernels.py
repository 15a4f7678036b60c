"""Builds and runs tests/cpp/test_tsne_kernels.hip: the kernels of cellranger_amd/csrc/tsne.hip by direct launch into guarded buffers
at constructed shapes.

The program includes tsne.hip inside a namespace and is compiled with cellranger_amd.build.FLAGS: it runs the same text under the same
flags, not the library's object code.  The context, the pool, the scan and the radix sort come from libcrgpu.so.

The descent holds + - * / only, so its outputs (the repulsion partials added in order, Z, the gradient, gains, uY, the new Y, the
centred Y, the CSR structure, the merged values before and after the normalisation, their total) must equal a host loop that takes
the device's steps in its order, bit for bit; the sums are also held to a long double reference within gamma(roundings + path) * sum
|terms| (derived in the program).  exp (the conditional rows) and log (the cost) are OCML's: they are compared against long double at
the device's own beta / P / Y with bounds from OCML's 1 ulp; the program prints the worst ratio.  The order model's sums come to 0.249 of
their bound at the worst (--host-only); the exp and log ratios are printed by the groups on the device (the README quotes them).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cellranger_amd")


def _build(out_dir):
    from cellranger_amd import build

    exe = os.path.join(str(out_dir), "test_tsne_kernels")
    cmd = [build.HIPCC] + build.FLAGS + ["-I" + os.path.join(PKG, "csrc"), "-I" + os.path.join(ROOT, "include"),
                                         os.path.join(ROOT, "tests", "cpp", "test_tsne_kernels.hip"), "-L" + PKG, "-lcrgpu", "-pthread",
                                         "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The program, built once for all groups."""
    from cellranger_amd import build

    build.build()
    return _build(tmp_path_factory.mktemp("tsne_kernels"))


def _run(exe, args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "all tests passed" in r.stdout, "\n".join(out.splitlines()[-40:])
    print("\n".join(line for line in r.stdout.splitlines() if not line.startswith("ok ")))  # the worst deviation-to-bound ratios
    return r.stdout


# the extern "C" entry points of tsne.hip keep their names inside the namespace, libcrgpu.so defines them too, so the linker exports
# the program's copies (the same text; the program calls none of them)
_EXPORTED = {"crgpu_tsne_affinities_dev", "crgpu_tsne_gradient_dev", "crgpu_tsne_dev"}


def test_tsne_kernels_compile_and_the_order_model_is_within_its_bound(exe):
    """CPU: tsne.hip compiles inside the namespace for gfx950 and links against the library as built from this tree; on every case the
    order model lies within the derived gamma bound of the long double reference.  The program's dynamic symbol table holds no
    k_tsne_* symbol that could interpose the library's kernels, and of the library's crgpu_* / cr_* names exactly the three entry
    points of tsne.hip."""
    out = _run(exe, ["--host-only"])
    assert out.count("(host only)") >= 30
    nm = subprocess.run(["nm", "-D", "--defined-only", exe], capture_output=True, text=True, check=True).stdout
    names = [line.split()[-1] for line in nm.splitlines() if line.strip()]
    assert names and not [n for n in names if "k_tsne_" in n]
    assert {n for n in names if n.startswith(("crgpu_", "cr_"))} == _EXPORTED


@pytest.mark.gpu
def test_tsne_kernels_repulse(exe):
    """k_tsne_repulse + k_tsne_finish + the column sums at N = 63 / 64 / 65, 127 .. 129, 255 .. 257 (the row tiles +- 1), CAND_CHUNK - 1,
    CAND_CHUNK, CAND_CHUNK + 1 and 2 CAND_CHUNK + 1, 2 and 3 dimensions, normal Y, Y over twelve decades and coincident rows (q = 1);
    row tiles of 64, 128, 256, candidate tiles of 1 (3 beyond a chunk), 333, 512, 1024 and slab groups of 64, 128, 256 rows and of all:
    every setting bit-equal to the order model."""
    _run(exe, ["--group", "repulse"])


@pytest.mark.gpu
def test_tsne_kernels_attract(exe):
    """k_tsne_attract (gradient only and with the update), the column sums, k_tsne_centre and k_tsne_kl: K = 3, 90 and 1024, a hub row
    of N - 1 entries and more beside rows of K, two neighbouring rows with threshold - 1 and threshold entries, the wave threshold at
    that value, at 1 (every row a wave), beyond every row (every row a lane) and one above; zero velocities (sign 0) and gains at the
    floor."""
    _run(exe, ["--group", "attract"])


@pytest.mark.gpu
def test_tsne_kernels_affinities(exe):
    """k_tsne_search at K = 3, 90 and 1024 with a row of zeros (200 steps, uniform): the entropy and every p in long double at the
    device's own beta; k_pair_keys, the library's sort, the merge, k_keys_to_csr, the total and k_tsne_divide against a host merge."""
    _run(exe, ["--group", "affinities"])
