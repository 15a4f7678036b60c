"""Builds and runs the C++ host-mirror test of RUN_PCA (include/crgpu.hpp over the C ABI): the host functions on the CPU, and on the GPU
the `thr` fixture of tests/golden/pca_reference.npz written out as raw arrays, with the bounds of tests/test_gpu_pca.py."""
import os
import subprocess

import numpy as np
import pytest

import pca_numpy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = "thr"


def _build(tmp_path):
    exe = str(tmp_path / "test_pca")
    pkg = os.path.join(ROOT, "cellranger_amd")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_pca.cpp"), "-L" + pkg, "-lcrgpu",
           "-Wl,-rpath," + pkg, "-Wl,-rpath-link,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


def test_cpp_pca_compiles_and_the_host_functions_hold(tmp_path):
    """CPU: the mirrors of crgpu.hpp compile and link against libcrgpu.so; the host half of the test needs no device."""
    from cellranger_amd import build

    build.build()
    r = subprocess.run([_build(tmp_path), "--host-only"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all tests passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_pca_on_the_device(tmp_path):
    exe = _build(tmp_path)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "pca_reference.npz"))
    dense = np.ascontiguousarray(P.FIXTURES[FIXTURE]["make"](), dtype=np.int32)
    d = tmp_path / "fixture"
    d.mkdir()
    dense.tofile(str(d / "dense.i32"))
    gold[FIXTURE + "_features_selected"].astype(np.int32).tofile(str(d / "features.i32"))
    gold[FIXTURE + "_d"].astype(np.float64).tofile(str(d / "d.f64"))
    np.ascontiguousarray(gold[FIXTURE + "_components"], dtype=np.float64).tofile(str(d / "components.f64"))
    with open(str(d / "meta.txt"), "w") as f:
        f.write("%d %d %d %d %d %d %.17g %.17g\n" % (dense.shape[0], dense.shape[1], int(gold[FIXTURE + "_n_components"]), int(gold[FIXTURE + "_it"]),
                                                    int(gold[FIXTURE + "_mprod"]), len(gold[FIXTURE + "_features_selected"]),
                                                    16.0 * float(gold[FIXTURE + "_mov_d"]), 16.0 * float(gold[FIXTURE + "_mov_components"])))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all tests passed" in r.stdout
