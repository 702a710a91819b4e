"""The workspace arena (bevgen_amd/csrc/arena.h) on the CPU: the metering mode sizes exactly what real carving takes, and Arena::carve keeps the two runs of a layout equal.

tests/host/arena_check.cpp is built for the host only - no HIP header, the arena's reserve / release backed by malloc - with the address and undefined-behaviour sanitizers,
and run directly: no GPU and no HIP call."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

CHECKS = [
    "same_offsets", "aligned_256", "metered_total_is_real_off", "metering_pointer_non_null", "one_byte_less_is_exhausted", "exact_size_fits", "measure",
    "carve_runs_layout_twice_reserves_once", "carve_keeps_a_sufficient_slab", "carve_grows", "carve_rejects_a_smaller_second_run", "carve_rejects_a_larger_second_run",
]


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("arena") / "arena_check")
    r = subprocess.run([HIPCC, "-std=c++17", "-x", "c++", "-O1", "-g", "-I", os.path.join(ROOT, "bevgen_amd", "csrc"), "-Xarch_host", "-fsanitize=address,undefined",
                        os.path.join(ROOT, "tests", "host", "arena_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert not p.stderr, p.stderr[-3000:]   # (a sanitizer report goes to stderr)
    out = {d["check"]: d for d in map(json.loads, p.stdout.splitlines())}
    assert p.returncode == sum(not d["ok"] for d in out.values()), (p.returncode, out)
    return out


def test_every_check_ran(results):
    assert sorted(results) == sorted(CHECKS)
    assert results["same_offsets"]["detail"].startswith("300 sequences, ")


@pytest.mark.parametrize("check", CHECKS)
def test_arena(results, check):
    assert results[check]["ok"], results[check]


def test_arena_header_needs_no_hip_header():
    for name in ("arena.h", "error.h"):
        with open(os.path.join(ROOT, "bevgen_amd", "csrc", name)) as f:
            includes = [l.split()[1] for l in f if l.startswith("#include")]
        assert all("hip" not in i and i not in ('"common.h"', '"kernels.h"', '"model.h"') for i in includes), (name, includes)
