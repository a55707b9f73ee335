"""Builds and runs tests/cpp/test_scratch_layout.cpp: the layout of a call's scratch block (csrc/scratch_layout.hpp) -- size and
carving agree, 256-byte boundaries, no overlap, spans between marks, counts of 0 and 1 and whole lines, a list that grew after the
sizing is refused, a host form's uploads with two arrays absent -- and the blocks of dendrogram_of_edges, forest_init and the StagedGraph against the byte counts those units
summed by hand before, at n, m, k in {1, 2, 63, 64, 65, 1000}.  Plain arithmetic under AddressSanitizer and UBSan; no device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp_layout") / "test_scratch_layout"
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "hnswlib-rs_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "test_scratch_layout.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return subprocess.run([str(out)], capture_output=True, text=True, timeout=120)


def test_layout_sizes_carves_and_refuses(run):
    assert run.returncode == 0 and "scratch layout OK" in run.stdout and "FAILED" not in run.stdout, run.stdout + run.stderr
