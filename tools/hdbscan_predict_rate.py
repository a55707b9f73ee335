#!/usr/bin/env python3
"""Wall time of HDBSCAN's prediction stage on the device, next to the search it is built on (the sibling of tools/hdbscan_rate.py,
same data and index: n x 128 DistL2, clustered, GPU-assisted build, M = 16, ef_construction 64; clustered with k = 16, ef = 64,
UNION, core_k = 5, min_cluster_size = 10, excess of mass, GLOSH on).  Per batch of --nq new vectors from the same distribution
(knbn = 10, ef = 64, core_k = 5), every buffer in HBM, in one process:
  * hnswgpu_search_batch_device alone;
  * hnswhdp_predict_device on the same queries (the search, the positions, the assignment);
  * hnswhdp_assign_device alone, on the rows the search left in HBM (DataIds are 0 .. n - 1 here, so a row's positions are its ids);
and once per index hnswhdp_core_distances_device.  One warm-up call, then the median of --repeats.  Before anything is reported the
assign form's answer on the search's rows is compared with the index form's, byte for byte.  One JSON line.
    hdbscan_predict_rate.py --n 1000000 --nq 10000 100000
Per-kernel times: run the tool under `rocprofv3 --kernel-trace --stats -- python tools/hdbscan_predict_rate.py --n N --nq NQ`."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from hdbscan_rate import CORE_K, DIM, DIST, EF, K, MCS, timed  # noqa: E402

KNBN = 10


def clustered(n, d, seed):
    """hdbscan_rate.clustered, and the centres besides"""
    rng = np.random.default_rng(seed)
    centres = rng.random((256, d), dtype=np.float32)
    return (centres[rng.integers(0, 256, n)] + np.float32(0.05) * rng.standard_normal((n, d), dtype=np.float32)).astype(np.float32), centres


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--nq", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import hnsw_rs_amd as H
    H.build_native()
    L = H.lib()
    n = a.n
    X, centres = clustered(n, DIM, 1)
    h = H.Hnsw(16, n, 16, 64, DIST)
    h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
    t0 = time.perf_counter()
    h.parallel_insert(X)
    h.upload(0)
    out = dict(n=n, d=DIM, dist=DIST, k=K, ef=EF, mode="union", core_k=CORE_K, min_cluster_size=MCS, method="eom", knbn=KNBN, repeats=a.repeats,
               warmup=a.warmup, build_and_upload_s=time.perf_counter() - t0)
    r = h.hdbscan(MCS, K, EF, "union", CORE_K, outlier_scores=True)
    out["clusters"], out["labels"] = r.n_clusters, r.n_labels
    kk = r.n_clusters
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()  # noqa: E731
    as_i32 = lambda x: dev(np.ascontiguousarray(x).view(np.int32))  # noqa: E731
    d_core = torch.zeros(n, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def core_form():
        rc = L.hnswhdp_core_distances_device(h.handle, K, EF, CORE_K, ptr(d_core), None)
        assert rc == 0, H._native.last_error()
    out["core_distances_device_s"] = timed(core_form, a.warmup, a.repeats)
    d_tree = [as_i32(r.cluster_parent), dev(r.cluster_birth_w), as_i32(r.point_cluster), dev(r.point_w), dev(r.selected.astype(np.uint8))]
    d_death = dev(r.cluster_death_lambda)
    tree = [ptr(d_core), kk] + [ptr(t) for t in d_tree] + [0.0, ptr(d_death)]
    out["batches"] = []
    rng = np.random.default_rng(2)
    for nq in a.nq:
        Q = (centres[rng.integers(0, 256, nq)] + np.float32(0.05) * rng.standard_normal((nq, DIM), dtype=np.float32)).astype(np.float32)
        d_q = dev(Q)
        ids = torch.zeros(nq * KNBN, dtype=torch.int64, device="cuda")
        dists = torch.zeros(nq * KNBN, dtype=torch.float32, device="cuda")
        layers = torch.zeros(nq * KNBN, dtype=torch.uint8, device="cuda")
        ranks, counts = torch.zeros(nq * KNBN, dtype=torch.int32, device="cuda"), torch.zeros(nq, dtype=torch.int32, device="cuda")
        outs = [[torch.zeros(nq, dtype=torch.int32, device="cuda") for _ in range(6)] for _ in range(2)]
        torch.cuda.synchronize()

        def search_form():
            rc = L.hnswgpu_search_batch_device(h.handle, ptr(d_q), nq, DIM, KNBN, EF, ptr(ids), ptr(dists), ptr(layers), ptr(ranks), ptr(counts), None, None)
            assert rc == 0, H._native.last_error()

        def predict_form():
            rc = L.hnswhdp_predict_device(h.handle, ptr(d_q), nq, DIM, KNBN, EF, CORE_K, *tree, *[ptr(t) for t in outs[0]], None)
            assert rc == 0, H._native.last_error()
        b = dict(nq=nq)
        b["search_batch_device_s"] = timed(search_form, a.warmup, a.repeats)
        b["predict_device_s"] = timed(predict_form, a.warmup, a.repeats)
        pos = ids.to(torch.int32)                               # DataIds 0 .. n - 1: a point's position is its id
        torch.cuda.synchronize()

        def assign_form():
            rc = L.hnswhdp_assign_device(0, nq, KNBN, ptr(pos), ptr(dists), ptr(counts), CORE_K, n, *tree, *[ptr(t) for t in outs[1]], None)
            assert rc == 0, H._native.last_error()
        b["assign_device_s"] = timed(assign_form, a.warmup, a.repeats)
        for x, y in zip(outs[0], outs[1]):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        labels = outs[0][0].cpu().numpy()
        b["noise"] = int((labels < 0).sum())
        b["added_over_search"] = b["predict_device_s"]["median"] / b["search_batch_device_s"]["median"] - 1.0
        out["batches"].append(b)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
