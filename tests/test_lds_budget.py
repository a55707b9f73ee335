"""Builds and runs tests/cpp/test_lds_budget.cpp: the LDS of a workgroup as csrc/search_kernels.hpp adds it up (one-query search
launches, the descent, the literal-heap kernel, the pair pass, the construction kernels) against numbers worked out by hand -- the
table of long rows (54 016 / 56 064 bytes at d = 4096, 69 632 / 71 680 at d = 8000), the six configurations of bench.py as the
driver sized them before these functions existed --, the clamp of the visited table as a function of an assumed limit (64 KiB and
160 KiB), and the refusal of rows whose tile fits no launch.  The functions are pure host code; the program needs no device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp_lds") / "test_lds_budget"
    cmd = [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "hnswlib-rs_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "test_lds_budget.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return subprocess.run([str(out)], capture_output=True, text=True, timeout=60)


def test_sums_clamp_and_bench_shapes(run):
    assert run.returncode == 0 and "lds budget OK" in run.stdout and "FAILED" not in run.stdout, run.stdout + run.stderr


def test_refusal_message_names_d_the_bytes_needed_and_the_limit(run):
    """d = 39 713 (stride 39 744) against 160 KiB: 4 x 39 744 + 256 + 32 + 2560 + 2048 = 163 872 > 163 840"""
    msg = re.search(r"^message: (.*)$", run.stdout, re.M).group(1)
    assert "d = 39713" in msg and "163872 bytes" in msg and "163840 bytes" in msg and "too long for this device" in msg, msg
