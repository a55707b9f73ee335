#!/usr/bin/env python3
"""Rates of the queries by stored point (hnswgpu_exact_graph_batch, hnswgpu_graph_search_batch) on 1M x 128 DistL2, k = 10.
    knn_graph_rate.py --dump-dir DIR --build          builds the index and dumps it into DIR (one JSON line: the build)
    knn_graph_rate.py --dump-dir DIR --exact          loads the dump; the exact graph of 10 000 named points against the yardstick:
                                                      exact_search_flat fed the same 10 000 vectors as host queries; then the
                                                      existing one-filter exact call (30 % allowed).  With --package-root DIR2
                                                      through the package of another checkout (the parent commit, built there),
                                                      which has the yardstick and the one-filter call only: run the two in
                                                      alternation
    knn_graph_rate.py --dump-dir DIR --approx         loads the dump; the approximate graph of ALL points at ef = 64 against
                                                      parallel_search_flat of the same vectors uploaded in calls of 100 000, and
                                                      its recall against the exact graph on the 10 000-point sample
Warm-up calls first, then the median and the spread of --repeats calls.  Every mode prints one JSON line."""
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
N_POINTS, DIM, DIST, BASENAME, K, EF, SAMPLE = 1_000_000, 128, "DistL2", "graph_rate", 10, 64, 10_000


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
    ap.add_argument("--dump-dir", required=True)
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--exact", action="store_true")
    ap.add_argument("--approx", action="store_true")
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--efc", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--package-root", default=None)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import hnsw_rs_amd as H
    H.build_native()
    n, d = N_POINTS, DIM
    X = clustered(n, d, 1)                                   # (ids are 0 .. n-1: point i carries id i)
    out = dict(package_root=a.package_root or "this tree", n=n, d=d, dist=DIST, k=K, repeats=a.repeats, warmup=a.warmup)
    if a.build:
        h = H.Hnsw(a.m, n, 16, a.efc, DIST)
        h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
        t0 = time.perf_counter()
        h.parallel_insert(X)
        h.upload(0)
        out.update(mode="build", m=a.m, ef_construction=a.efc, build_and_upload_s=time.perf_counter() - t0)
        h.file_dump(a.dump_dir, BASENAME)
        print(json.dumps(out), flush=True)
        return
    h = H.HnswIo(a.dump_dir, BASENAME).load_hnsw(DIST)
    h.upload(0)
    pts = np.sort(np.random.default_rng(5).choice(n, SAMPLE, replace=False)).astype(np.uint64)
    Q = np.ascontiguousarray(X[pts.astype(np.int64)])
    if a.exact:
        out.update(mode="exact", points=SAMPLE)
        out["yardstick_exact_search_flat_s"] = timed(lambda: h.exact_search_flat(Q, K), a.warmup, a.repeats)
        if hasattr(h, "exact_knn_graph_flat"):
            g = h.exact_knn_graph_flat(K, pts)
            wide = h.exact_search_flat(Q, K + 1)
            # the same work: without exact copies in the data a point's graph row is its (k + 1)-NN answer behind the point itself
            out["rows_equal_the_knn_answer_behind_the_point"] = bool(np.array_equal(wide.ids[:, 0], pts) and np.array_equal(g.ids, wide.ids[:, 1:]) and
                                                                     np.array_equal(g.dists.view(np.uint32), wide.dists[:, 1:].view(np.uint32)))
            out["exact_graph_s"] = timed(lambda: h.exact_knn_graph_flat(K, pts), a.warmup, a.repeats)
        allowed = np.flatnonzero(np.random.default_rng(7).random(n) < 0.3).astype(np.uint64)
        out["one_filter_allowed"] = len(allowed)
        out["one_filter_exact_search_flat_s"] = timed(lambda: h.exact_search_flat(Q, K, allowed), a.warmup, a.repeats)
    if a.approx:
        out.update(mode="approx", ef=EF, points=n)
        out["graph_all_points_s"] = timed(lambda: h.knn_graph_flat(K, EF), a.warmup, a.repeats)

        def uploaded():
            for c0 in range(0, n, 100_000):
                h.parallel_search_flat(X[c0:c0 + 100_000], K, EF)
        out["parallel_search_flat_calls_of_100000_s"] = timed(uploaded, a.warmup, a.repeats)
        out["graph_sample_points_s"] = timed(lambda: h.knn_graph_flat(K, EF, pts), a.warmup, a.repeats)
        out["recall_by_id_on_the_sample"] = h.knn_graph_recall(K, EF, pts)
        whole = h.knn_graph_flat(K, EF)
        part = h.knn_graph_flat(K, EF, pts)
        out["sample_rows_equal_the_whole_graphs"] = bool(np.array_equal(whole.ids[pts.astype(np.int64)], part.ids))
        out["mean_count"] = float(whole.counts.mean())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
