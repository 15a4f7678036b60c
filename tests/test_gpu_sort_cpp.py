"""Builds and runs tests/cpp/test_sort.hip: the device sort of cellranger_amd/csrc/sort.hip, entry point by entry point,
against std::stable_sort on the host.

The program links libcrgpu.so and calls the exported cr_* functions of sort.hip directly (the radix sorts on 32- and 64-bit
keys, the finishing step behind a sort on the top bits, the partition by owner, the small scan), with the context kept opaque.
All data are integers, every comparison is exact.  The payload of a case is the input index, so for the radix passes and the
partition the expected payload is the stable order itself.  The finishing step is different ON PURPOSE: among EQUAL whole keys
it promises no order (or_flag_permute is an in-place American-flag permutation), so there the test asserts the set of payloads
of every range of equal keys, and the exact order only for runs that held no descent and must not be rewritten.

The case sizes hang on the tuning constants of sort.hip (the chunk of the scatter, the look-back width, the run-length classes
of the repair kernels ...).  They live in the source, not in a header: they are read out of the text here, each one asserted
to be found, and handed to the program, which derives every size from them.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cellranger_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

_DEFINES = ["SORT_BLOCK", "SORT_ITEMS", "SORT_ITEMS_KV64", "SORT_LB", "SORT_MAX_BLOCKS", "OS_GROUP", "OR_MAX_LOW_BITS", "OR_CAP",
            "OR_MAX", "FD_ITEMS", "RR_SHORT", "RR_WORDS", "RL_CAP"]


def sort_constants():
    with open(os.path.join(PKG, "csrc", "sort.hip")) as f:
        text = f.read()
    c = {}
    for name in _DEFINES:
        m = re.search(r"^#define\s+%s\s+\(?\s*(0x[0-9a-fA-F]+|\d+)u?\s*\)?\s*(?://.*)?$" % name, text, re.M)
        assert m, "#define %s not found in sort.hip" % name
        c[name] = int(m.group(1), 0)
    # the chunk of a scatter workgroup is composed in SortCfg; make sure it still is before composing it here
    assert re.search(r"ITEMS\s*=\s*\(sizeof\(K\)\s*==\s*8\s*&&\s*HAS_VALS\)\s*\?\s*SORT_ITEMS_KV64\s*:\s*SORT_ITEMS;", text), "SortCfg::ITEMS"
    assert re.search(r"CHUNK\s*=\s*SORT_BLOCK\s*\*\s*ITEMS;", text), "SortCfg::CHUNK"
    c["CHUNK"] = c["SORT_BLOCK"] * c["SORT_ITEMS"]
    c["CHUNK_KV64"] = c["SORT_BLOCK"] * c["SORT_ITEMS_KV64"]
    return c


def _const_args():
    args = []
    for k, v in sorted(sort_constants().items()):
        args += ["--const", "%s=%d" % (k, v)]
    return args


def _build(out_dir):
    exe = os.path.join(str(out_dir), "test_sort")
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(PKG, "csrc"),
           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_sort.hip"), "-L" + PKG, "-lcrgpu",
           "-pthread", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The program, built once for all device groups."""
    return _build(tmp_path_factory.mktemp("sort_cpp"))


def _tail(r, lines=40):
    return "\n".join((r.stdout + r.stderr).splitlines()[-lines:])


def _run_group(exe, group, env=None, timeout=300):
    e = dict(os.environ)
    for k in ("CRGPU_SORT", "CRGPU_SORT_FINISH", "CRGPU_SORT_STATUS64", "CRGPU_SORT_FORCE_ABORT"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([exe, "--group", group] + _const_args(), capture_output=True, text=True, timeout=timeout, env=e)
    assert r.returncode == 0 and "all tests passed" in r.stdout, _tail(r)
    return r.stdout


def test_cpp_sort_compiles_and_the_digit_plans_hold(tmp_path):
    """CPU: the program compiles and links against libcrgpu.so; cr_sweep_plan for every 0 <= lo < hi <= 64 and
    cr_sort_low_bits for every key width need no device."""
    from cellranger_amd import build

    build.build()
    c = sort_constants()
    assert c["CHUNK"] > c["CHUNK_KV64"] > 64 and c["OR_CAP"] > c["RR_SHORT"] and c["OR_MAX"] > c["RL_CAP"] > 65
    r = subprocess.run([_build(tmp_path), "--host-only"] + _const_args(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all tests passed" in r.stdout, _tail(r)
    assert "2080 plans" in r.stdout


@pytest.mark.gpu
def test_cpp_sort_u32(exe):
    """cr_radix_sort_u32 (the classic three-kernel passes), with and without payload: chunk and workgroup borders, 8- and 9-bit
    digits, bit ranges off bit 0."""
    _run_group(exe, "u32")


@pytest.mark.gpu
def test_cpp_sort_u64(exe):
    """cr_radix_sort_u64 and _full by the onesweep scatter: look-back rounds, per-XCD ticket groups, 32- and 64-bit status words."""
    _run_group(exe, "u64")


@pytest.mark.gpu
def test_cpp_sort_u64_classic(exe):
    """The same cases with CRGPU_SORT=classic (latched once per process, hence a process of its own)."""
    _run_group(exe, "u64", env={"CRGPU_SORT": "classic"})


@pytest.mark.gpu
def test_cpp_sort_finish(exe):
    """A sort on the top bits and cr_order_runs: every class of run length on every border of the repair kernels' shares,
    the run heads per tile, the fall-back beyond OR_MAX keys.  Payload order among equal keys is not asserted (see above)."""
    _run_group(exe, "finish")


@pytest.mark.gpu
def test_cpp_sort_finish_without_the_low_bits_switch(exe):
    """CRGPU_SORT_FINISH=0 only changes what cr_sort_low_bits proposes; the program composes the two steps itself, so the same
    expectations hold."""
    _run_group(exe, "finish", env={"CRGPU_SORT_FINISH": "0"})


@pytest.mark.gpu
def test_cpp_sort_partition(exe):
    """cr_partition_by_owner[_kv]: equal widths and explicit bounds with empty ranges, barcodes on and right below every bound,
    the refused inputs."""
    _run_group(exe, "partition")


@pytest.mark.gpu
def test_cpp_sort_scan(exe):
    _run_group(exe, "scan")


@pytest.mark.gpu
def test_cpp_sort_large(exe):
    """More keys than SORT_MAX_BLOCKS tiles of four chunks: the block count is capped, k_scan_digits runs several rounds."""
    _run_group(exe, "large")
