#!/usr/bin/env python3
"""Wall time of hnswgpu_graph_components (k = 16, ef = 64, UNION and MUTUAL) next to hnswgpu_symmetric_graph -- the nearest path
before the components existed: the symmetrised graph, downloaded, then a union-find on the host -- and next to the source call of D
itself, on n x 128 DistL2 (clustered, the data of tools/knn_graph_rate.py and tools/symmetric_graph_rate.py), the index built in the
process (GPU-assisted, M = 16, ef_construction 64).
    graph_components_rate.py --n 100000
    graph_components_rate.py --n 1000000
    ... --csr            also hnswgpu_csr_components on the symmetrised graph's own CSR (host arrays: the upload is in the time)
Host-buffer entries through the Python methods; one warm-up call, then the median of --repeats.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIM, DIST, K, EF = 128, "DistL2", 16, 64


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--csr", action="store_true")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import hnsw_rs_amd as H
    H.build_native()
    n = a.n
    X = clustered(n, DIM, 1)
    h = H.Hnsw(16, n, 16, 64, DIST)
    h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
    t0 = time.perf_counter()
    h.parallel_insert(X)
    h.upload(0)
    out = dict(n=n, d=DIM, dist=DIST, k=K, ef=EF, repeats=a.repeats, warmup=a.warmup, build_and_upload_s=time.perf_counter() - t0)
    out["graph_search_s"] = timed(lambda: h.knn_graph_flat(K, EF), a.warmup, a.repeats)
    for mode in ("union", "mutual"):
        out[f"symmetric_{mode}_s"] = timed(lambda: h.symmetric_knn_graph_flat(K, EF, mode), a.warmup, a.repeats)
        out[f"components_{mode}_s"] = timed(lambda: h.knn_graph_components(K, EF, mode), a.warmup, a.repeats)
        g = h.symmetric_knn_graph_flat(K, EF, mode)
        c = h.knn_graph_components(K, EF, mode)
        cut = float(np.median(g.dists)) if len(g.dists) else 0.0
        out[f"components_{mode}_cut_at_median_s"] = timed(lambda: h.knn_graph_components(K, EF, mode, cut), a.warmup, a.repeats)
        out[f"{mode}_total"], out[f"{mode}_components"], out[f"{mode}_largest"] = int(g.offsets[-1]), c.n_components, int(c.sizes.max())
        out[f"{mode}_components_cut_at_median"] = h.knn_graph_components(K, EF, mode, cut).n_components
        if a.csr:
            out[f"csr_components_{mode}_s"] = timed(lambda: H.csr_components(g.offsets, g.pos), a.warmup, a.repeats)
            assert np.array_equal(H.csr_components(g.offsets, g.pos).labels, c.labels)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
