#!/usr/bin/env python3
"""Wall time of hnswgpu_graph_spanning_forest (k = 16, ef = 64, UNION and MUTUAL, core_k 0 and 5) next to hnswgpu_graph_components
and hnswgpu_symmetric_graph on the same D -- the nearest paths before the forest existed: the components at ONE radius, or the
symmetrised graph, downloaded, then sorted and run through Kruskal on the host -- on n x 128 DistL2 (clustered, the data of
tools/graph_components_rate.py), the index built in the process (GPU-assisted, M = 16, ef_construction 64).
    spanning_forest_rate.py --n 100000
    spanning_forest_rate.py --n 1000000
    ... --csr            also hnswgpu_csr_spanning_forest on the symmetrised graph's own CSR (host arrays: the upload is in the time)
Host-buffer entries through the Python methods; one warm-up call, then the median of --repeats.  The number of Boruvka rounds is a
function of the edge list alone: it is counted on the host, by the same rule (every component picks its lightest outgoing edge in
the order (weight, lo, hi); the round that picks nothing is counted, as the device runs it).  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIM, DIST, K, EF, CORE_K = 128, "DistL2", 16, 64, 5


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


def boruvka_rounds(n, lo, hi, w):
    """the rounds Boruvka takes on the pairs (lo < hi, w >= 0) under the order (w, lo, hi), the last one, which picks nothing, included"""
    order = np.lexsort((hi, lo, w))
    lo, hi = lo[order].astype(np.int64), hi[order].astype(np.int64)
    comp = np.arange(n, dtype=np.int64)
    rounds = 0
    while True:
        rounds += 1
        ca, cb = comp[lo], comp[hi]
        out = np.flatnonzero(ca != cb)
        if len(out) == 0:
            return rounds
        best = np.full(n, len(lo), np.int64)
        np.minimum.at(best, ca[out], out)
        np.minimum.at(best, cb[out], out)
        picked = np.unique(best[best < len(lo)])
        # the picked edges have no cycle: join their ends' components, the smaller number winning, until nothing moves
        x, y = comp[lo[picked]], comp[hi[picked]]
        root = np.arange(n, dtype=np.int64)
        while True:
            rx, ry = root[x], root[y]
            if (rx == ry).all():
                break
            np.minimum.at(root, np.maximum(rx, ry), np.minimum(rx, ry))
            while True:
                nxt = root[root]
                if (nxt == root).all():
                    break
                root = nxt
        comp = root[comp]
        lo, hi = lo[out], hi[out]                               # (an edge inside a component stays inside)


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
    out = dict(n=n, d=DIM, dist=DIST, k=K, ef=EF, core_k=CORE_K, repeats=a.repeats, warmup=a.warmup, build_and_upload_s=time.perf_counter() - t0)
    D = h.knn_graph_flat(K, EF)
    core = np.where(D.counts > 0, D.dists[np.arange(n), np.minimum(D.counts, CORE_K) - 1], np.float32(0)).astype(np.float32)
    for mode in ("union", "mutual"):
        out[f"symmetric_{mode}_s"] = timed(lambda: h.symmetric_knn_graph_flat(K, EF, mode), a.warmup, a.repeats)
        out[f"components_{mode}_s"] = timed(lambda: h.knn_graph_components(K, EF, mode), a.warmup, a.repeats)
        g = h.symmetric_knn_graph_flat(K, EF, mode)
        c = h.knn_graph_components(K, EF, mode)
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(g.offsets.astype(np.int64)))
        up = rows < g.pos                                       # (DistL2: both directions of a pair carry the same bits)
        lo, hi, w = rows[up], g.pos[up].astype(np.int64), g.dists[up]
        out[f"{mode}_pairs"], out[f"{mode}_components"] = int(up.sum()), c.n_components
        for core_k in (0, CORE_K):
            tag = f"{mode}_core{core_k}"
            out[f"forest_{tag}_s"] = timed(lambda: h.knn_graph_spanning_forest(K, EF, mode, core_k), a.warmup, a.repeats)
            f = h.knn_graph_spanning_forest(K, EF, mode, core_k)
            assert f.n_edges == n - c.n_components and (f.a < f.b).all()
            ww = w if core_k == 0 else np.maximum(w, np.maximum(core[lo], core[hi]))
            out[f"rounds_{tag}"] = boruvka_rounds(n, lo, hi, ww)
            out[f"forest_{tag}_edges"], out[f"forest_{tag}_weight"] = f.n_edges, float(f.weights.astype(np.float64).sum())
        if a.csr:
            out[f"csr_forest_{mode}_s"] = timed(lambda: H.csr_spanning_forest(g.offsets, g.pos, g.dists), a.warmup, a.repeats)
            f0, f1 = h.knn_graph_spanning_forest(K, EF, mode), H.csr_spanning_forest(g.offsets, g.pos, g.dists)
            assert np.array_equal(f0.a, f1.a) and np.array_equal(f0.b, f1.b) and np.array_equal(f0.weights, f1.weights)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
