#!/usr/bin/env python3
"""Wall time of hnswgpu_graph_dendrogram next to hnswgpu_graph_spanning_forest on the same index (k = 16, ef = 64, UNION, core_k 0;
both host entries through the Python methods), of the forest form alone on its device entry (hnswgpu_forest_dendrogram_device, the
forest already in HBM), and of what a caller did before: the forest's ends downloaded (timed on their own, from HBM into pageable
host arrays) and run through a sequential union-find on ONE host core -- compiled C++ (g++ -O2, built into a temporary directory
when the tool starts), or numpy-free Python where no compiler is found; the line says which.  n x 128 DistL2 (clustered, the data
of tools/spanning_forest_rate.py), the index built in the process (GPU-assisted, M = 16, ef_construction 64).
    dendrogram_rate.py --n 100000
    dendrogram_rate.py --n 1000000
One warm-up call, then the median of --repeats.  The number of levels is ceil(log2 m), a function of the edge count alone.  The
three answers (index form, device form, host pass) are compared byte for byte before anything is reported.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIM, DIST, K, EF = 128, "DistL2", 16, 64

HOST_PASS = r"""
#include <cstdint>
#include <vector>
extern "C" int host_dendrogram(uint32_t n, uint32_t m, const uint32_t* a, const uint32_t* b, uint32_t* left, uint32_t* right, uint32_t* size) {
    std::vector<uint32_t> parent(n), last(n, 0xFFFFFFFFu), count(n, 1u);
    for (uint32_t v = 0; v < n; ++v) parent[v] = v;
    auto find = [&](uint32_t v) {
        while (parent[v] != v) v = parent[v] = parent[parent[v]];
        return v;
    };
    for (uint32_t e = 0; e < m; ++e) {
        const uint32_t ra = find(a[e]), rb = find(b[e]);
        if (ra == rb) return 1;
        left[e] = last[ra] == 0xFFFFFFFFu ? a[e] : n + last[ra];
        right[e] = last[rb] == 0xFFFFFFFFu ? b[e] : n + last[rb];
        const uint32_t lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
        parent[hi] = lo;
        count[lo] += count[hi];
        last[lo] = e;
        size[e] = count[lo];
    }
    return 0;
}
"""


def clustered(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.random((256, d), dtype=np.float32)
    return (centres[rng.integers(0, 256, n)] + np.float32(0.05) * rng.standard_normal((n, d), dtype=np.float32)).astype(np.float32)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(median=statistics.median(ts), min=min(ts), max=max(ts))


def python_pass(n, a, b):
    """the same pass without numpy in the loop"""
    a, b = a.tolist(), b.tolist()
    parent, last, count = list(range(n)), [-1] * n, [1] * n
    left, right, size = [0] * len(a), [0] * len(a), [0] * len(a)
    for e in range(len(a)):
        x, y = a[e], b[e]
        ra = x
        while parent[ra] != ra:
            parent[ra] = parent[parent[ra]]
            ra = parent[ra]
        rb = y
        while parent[rb] != rb:
            parent[rb] = parent[parent[rb]]
            rb = parent[rb]
        left[e] = x if last[ra] < 0 else n + last[ra]
        right[e] = y if last[rb] < 0 else n + last[rb]
        lo, hi = (ra, rb) if ra < rb else (rb, ra)
        parent[hi] = lo
        count[lo] += count[hi]
        last[lo] = e
        size[e] = count[lo]
    return np.array(left, np.uint32), np.array(right, np.uint32), np.array(size, np.uint32)


def host_pass(tmp):
    """(name, fn(n, a, b) -> left, right, size)"""
    src, lib = os.path.join(tmp, "host_dendrogram.cpp"), os.path.join(tmp, "host_dendrogram.so")
    with open(src, "w") as f:
        f.write(HOST_PASS)
    try:
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", lib], check=True, capture_output=True)
        fn = C.CDLL(lib).host_dendrogram
    except (OSError, subprocess.CalledProcessError):
        return "python", python_pass
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 5

    def run(n, a, b):
        out = [np.empty(len(a), np.uint32) for _ in range(3)]
        rc = fn(n, len(a), a.ctypes.data, b.ctypes.data, *[x.ctypes.data for x in out])
        assert rc == 0
        return out
    return "c++ (g++ -O2)", run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import hnsw_rs_amd as H
    H.build_native()
    L = H.lib()
    n = a.n
    X = clustered(n, DIM, 1)
    h = H.Hnsw(16, n, 16, 64, DIST)
    h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
    t0 = time.perf_counter()
    h.parallel_insert(X)
    h.upload(0)
    out = dict(n=n, d=DIM, dist=DIST, k=K, ef=EF, mode="union", core_k=0, repeats=a.repeats, warmup=a.warmup,
               build_and_upload_s=time.perf_counter() - t0)
    out["forest_s"] = timed(lambda: h.knn_graph_spanning_forest(K, EF), a.warmup, a.repeats)
    out["dendrogram_s"] = timed(lambda: h.knn_graph_dendrogram(K, EF), a.warmup, a.repeats)
    f, d = h.knn_graph_spanning_forest(K, EF), h.knn_graph_dendrogram(K, EF)
    assert d.a.tobytes() == f.a.tobytes() and d.b.tobytes() == f.b.tobytes() and d.weights.tobytes() == f.weights.tobytes()
    m = f.n_edges
    out["edges"], out["levels"], out["roots"] = m, max(m - 1, 0).bit_length(), int(len(d.roots()))
    # the forest form alone, the forest in HBM
    d_a, d_b = (torch.from_numpy(x.view(np.int32).copy()).cuda() for x in (f.a, f.b))
    d_out = [torch.zeros(m, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()

    def device_form():
        rc = L.hnswgpu_forest_dendrogram_device(0, n, m, *[C.c_void_p(t.data_ptr()) for t in (d_a, d_b, *d_out)], None)
        assert rc == 0, H._native.last_error()
    out["forest_dendrogram_device_s"] = timed(device_form, a.warmup, a.repeats)
    got = [t.cpu().numpy().view(np.uint32) for t in d_out]
    assert all(np.array_equal(x, y) for x, y in zip(got, (d.left, d.right, d.sizes)))
    # what a caller did before: the ends downloaded, then one host core
    host_a, host_b = np.empty(m, np.uint32), np.empty(m, np.uint32)

    def download():
        host_a[:] = d_a.cpu().numpy().view(np.uint32)
        host_b[:] = d_b.cpu().numpy().view(np.uint32)
    out["download_ends_s"] = timed(download, a.warmup, a.repeats)
    with tempfile.TemporaryDirectory() as tmp:
        name, run = host_pass(tmp)
        out["host_pass"] = name
        out["host_pass_s"] = timed(lambda: run(n, host_a, host_b), a.warmup, a.repeats if name != "python" else 1)
        ref = run(n, host_a, host_b)
    assert all(np.array_equal(x, y) for x, y in zip(ref, (d.left, d.right, d.sizes)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
