"""Builds and runs tests/cpp/test_dbscan.cpp: hnswdbs_csr of include/hnsw_mi355x_dbscan.h called from C++; and the header as C."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def binary(native, tmp_path_factory):
    out = tmp_path_factory.mktemp("cpp_dbscan") / "test_dbscan"
    lib_dir = os.path.dirname(native.LIB_PATH)
    cmd = ["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "test_dbscan.cpp"), "-o", str(out), native.LIB_PATH, f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "as_c.c"
    src.write_text('#include "hnsw_mi355x_dbscan.h"\n'
                   "int (*const p_exact)(const hnswgpu_index*, float, uint64_t, int32_t*, uint8_t*, uint32_t*, uint32_t*, uint64_t*) = hnswdbs_exact;\n"
                   "int (*const p_csr)(int, uint64_t, const uint64_t*, const uint32_t*, const float*, float, uint64_t, uint32_t, int32_t*, uint8_t*, uint32_t*,\n"
                   "                   uint32_t*, uint64_t*) = hnswdbs_csr;\n")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "as_c.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cpp_dbscan_host_side(binary):
    r = subprocess.run([binary, "cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cpu mode OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_dbscan_on_the_device(binary):
    r = subprocess.run([binary, "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "gpu mode OK" in r.stdout, r.stdout + r.stderr
