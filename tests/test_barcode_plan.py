"""Builds and runs tests/cpp/test_barcode_plan.cpp: the sizing arithmetic of the barcode stage's host side
(cellranger_amd/csrc/barcode_plan.h) at pinned values.  Host code only: a plain g++ program, no GPU and no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_barcode_plan_values(tmp_path):
    exe = str(tmp_path / "test_barcode_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "cellranger_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_barcode_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all tests passed" in r.stdout
