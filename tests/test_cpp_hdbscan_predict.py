"""Builds and runs tests/cpp/test_hdbscan_predict.cpp: hnswhdp_assign of include/hnsw_mi355x_hdbscan_predict.h called from C++."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def binary(native, tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp_hdbscan_predict") / "test_hdbscan_predict"
    lib_dir = os.path.dirname(native.LIB_PATH)
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_hdbscan_predict.cpp"), "-o", str(out), native.LIB_PATH, f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def test_cpp_hdbscan_predict_host_side(binary):
    r = subprocess.run([binary, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cpu mode OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_hdbscan_predict_on_the_device(binary):
    r = subprocess.run([binary, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gpu mode OK" in r.stdout, r.stdout + r.stderr
