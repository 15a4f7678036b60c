"""Builds and runs the C++ host-mirror test of CORRECT_CHEMISTRY_BATCH (include/crgpu.hpp over the C ABI)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "test_batch_correction")
    pkg = os.path.join(ROOT, "cellranger_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_batch_correction.cpp"), "-L" + pkg, "-lcrgpu",
           "-Wl,-rpath," + pkg, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_cpp_batch_correction_compiles_and_the_host_functions_hold(tmp_path):
    """CPU: the mirrors of crgpu.hpp compile and link against libcrgpu.so; the host half of the test needs no device."""
    from cellranger_amd import build

    build.build()
    r = subprocess.run([_build(tmp_path), "--host-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_batch_correction_on_the_device(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all tests passed" in r.stdout
