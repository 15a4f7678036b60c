"""Builds and runs tests/cpp/test_block_utils.hip: the wave and workgroup primitives of cellranger_amd/csrc/block_utils.h, called
directly, one launch of at most a few workgroups per case.

The header needs nothing from the library, so the program links the HIP runtime alone.  Every comparison is exact: integers as
they are, f64 as bit patterns against host loops that take the steps of the device code in its order (wave_incl_scan: distances
1, 2, 4, ...; wave_sum / wave_max: the butterfly 32, 16, ... 1, the result of all 64 lanes).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cellranger_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _build(out_dir):
    exe = os.path.join(str(out_dir), "test_block_utils")
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.join(PKG, "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_block_utils.hip"), "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def _run(exe, args=()):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all tests passed" in r.stdout, "\n".join((r.stdout + r.stderr).splitlines()[-40:])
    return r.stdout


def test_block_utils_compiles_and_the_host_models_hold(tmp_path):
    """CPU: the header and every instantiation the device cases use compile for gfx950, and the host models of the scan and of
    the butterfly agree with plain serial loops (on integers, where every order is exact), the butterfly's lane 0 with a tree of
    downward shifts bit for bit."""
    out = _run(_build(tmp_path), ["--host-only"])
    assert "0 failed (host only)" in out


@pytest.mark.gpu
def test_block_utils_on_the_device(tmp_path):
    """wave_incl_scan<2 .. 64> for u32 and f64 inside `if (lane < W)` with the other lanes busy and one wave gone; every
    wave_sum / wave_or / wave_min / wave_max overload in all 64 lanes; block_excl_scan<64 | 256 | 1024> twice in a row, with and
    without the trailing barrier, total_out given and NULL; block_reserve_256 of three workgroups on one counter; the count tail
    for 4 and 16 waves; the write tail for 4, 32 and 64 words."""
    out = _run(_build(tmp_path))
    assert " 0 failed" in out and "host only" not in out
