#!/usr/bin/env python3
"""Wall time of hnswgpu_symmetric_graph (UNION, k = 16) next to its own source call, on n x 128 DistL2 (clustered, the data of
tools/knn_graph_rate.py), the index built in the process (GPU-assisted, M = 16, ef_construction 64).
    symmetric_graph_rate.py --n 100000 --exact --approx     the symmetrised graph from the exact graph and from the graph at ef = 64,
                                                            each beside hnswgpu_exact_graph_batch / hnswgpu_graph_search_batch of
                                                            every point at the same k (and ef)
    symmetric_graph_rate.py --n 1000000 --approx            at 1M the exact graph of every point is not run
    ... --package-root DIR                                  the source calls alone through the package of another checkout (the
                                                            parent commit, built there), which has no symmetrised graph
    ... --once                                              one symmetrised call at ef = 64 and nothing else (for a kernel trace)
Host-buffer entries through the Python methods; one warm-up call, then the median of --repeats.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--package-root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--package-root") + 1])
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
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--approx", action="store_true")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--package-root", default=None)
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
    out = dict(package_root=a.package_root or "this tree", n=n, d=DIM, dist=DIST, k=K, mode="union", repeats=a.repeats, warmup=a.warmup,
               build_and_upload_s=time.perf_counter() - t0)
    have = hasattr(h, "symmetric_knn_graph_flat")
    if a.once:
        g = h.symmetric_knn_graph_flat(K, EF, "union")
        out.update(ef=EF, total=int(g.offsets[-1]), longest_row=int(g.counts.max()))
        print(json.dumps(out), flush=True)
        return
    if a.exact:
        out["exact_graph_s"] = timed(lambda: h.exact_knn_graph_flat(K), a.warmup, a.repeats)
        if have:
            out["symmetric_from_exact_s"] = timed(lambda: h.symmetric_knn_graph_flat(K, None, "union"), a.warmup, a.repeats)
            g = h.symmetric_knn_graph_flat(K, None, "union")
            out["exact_total"], out["exact_longest_row"] = int(g.offsets[-1]), int(g.counts.max())
    if a.approx:
        out["ef"] = EF
        out["graph_search_s"] = timed(lambda: h.knn_graph_flat(K, EF), a.warmup, a.repeats)
        if have:
            out["symmetric_from_graph_search_s"] = timed(lambda: h.symmetric_knn_graph_flat(K, EF, "union"), a.warmup, a.repeats)
            g = h.symmetric_knn_graph_flat(K, EF, "union")
            out["approx_total"], out["approx_longest_row"] = int(g.offsets[-1]), int(g.counts.max())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
