#!/usr/bin/env python3
"""Wall time of DBSCAN on the device next to the count pass it is made of (the sibling of tools/hdbscan_predict_rate.py, same data and
index: n x 128 DistL2, clustered, GPU-assisted build, M = 16, ef_construction 64), every buffer in HBM, in one process:
  * hnswgpu_exact_range_search_batch_device, count only (cap = 0), on --nq stored vectors as queries, every radius the eps -- and that
    time scaled to n queries: what one pass over all pairs costs;
  * hnswdbs_exact_device at min_samples = 10 and three eps: the 10th-nearest distance (the point itself included) that --core of a
    sample of the points reach -- few points core, about half, nearly all;
  * hnswdbs_csr_device on the symmetric graph at k = 10 (ef = 64, UNION, add_self 1), eps the middle one.
One warm-up call, then the median of --repeats.  One JSON line.
    dbscan_rate.py --n 1000000
Per-kernel times: run the tool under `rocprofv3 --kernel-trace --stats -- python tools/dbscan_rate.py --n N`."""
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
from hdbscan_rate import DIM, DIST, clustered, timed  # noqa: E402

MIN_SAMPLES, K, EF = 10, 10, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--core", type=float, nargs="+", default=[0.05, 0.5, 0.98])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import hnsw_rs_amd as H
    H.build_native()
    L = H.lib()
    N = H._native
    n, nq = a.n, min(a.nq, a.n)
    X = clustered(n, DIM, 1)
    h = H.Hnsw(16, n, 16, 64, DIST)
    h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
    t0 = time.perf_counter()
    h.parallel_insert(X)
    h.upload(0)
    out = dict(n=n, d=DIM, dist=DIST, min_samples=MIN_SAMPLES, nq_count_pass=nq, repeats=a.repeats, warmup=a.warmup,
               build_and_upload_s=time.perf_counter() - t0)
    rng = np.random.default_rng(2)
    sample = X[rng.choice(n, min(n, 2000), replace=False)]
    tenth = np.sort(h.exact_search_flat(sample, MIN_SAMPLES).dists[:, MIN_SAMPLES - 1])
    eps_of = [float(tenth[min(len(tenth) - 1, int(c * len(tenth)))]) for c in a.core]
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()  # noqa: E731
    d_q = dev(X[rng.choice(n, nq, replace=False)])
    d_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
    label, count, anchor = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    core = torch.zeros(n, dtype=torch.uint8, device="cuda")
    c = np.zeros(1, np.uint64)
    torch.cuda.synchronize()
    out["cases"] = []
    for share, eps in zip(a.core, eps_of):
        d_rad = torch.full((nq,), eps, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        def count_form():
            rc = L.hnswgpu_exact_range_search_batch_device(h.handle, ptr(d_q), nq, DIM, ptr(d_rad), None, 0, 0, ptr(d_off), None, None, None, None, None)
            assert rc in (N.OK, N.ERR_CAPACITY), N.last_error()    # (count only: "the answers need more than 0 slots" is the answer)

        def dbscan_form():
            rc = L.hnswdbs_exact_device(h.handle, eps, MIN_SAMPLES, ptr(label), ptr(core), ptr(count), ptr(anchor), c.ctypes.data, None)
            assert rc == 0, N.last_error()
        b = dict(core_share_asked=share, eps=eps)
        b["count_only_s"] = timed(count_form, a.warmup, a.repeats)
        b["answers_per_query"] = float(d_off[-1].item()) / nq
        b["count_pass_scaled_to_n_s"] = b["count_only_s"]["median"] * n / nq
        b["dbscan_exact_device_s"] = timed(dbscan_form, a.warmup, a.repeats)
        b["clusters"], b["core"], b["noise"] = int(c[0]), int(core.sum().item()), int((label < 0).sum().item())
        b["ratio_to_one_count_pass"] = b["dbscan_exact_device_s"]["median"] / b["count_pass_scaled_to_n_s"]
        out["cases"].append(b)
    g = h.symmetric_knn_graph_flat(K, EF, "union")
    d_offs, d_cols, d_dists = dev(g.offsets.view(np.int64)), dev(g.pos.astype(np.uint32).view(np.int32)), dev(g.dists)
    eps = eps_of[len(eps_of) // 2]
    torch.cuda.synchronize()

    def csr_form():
        rc = L.hnswdbs_csr_device(0, n, ptr(d_offs), ptr(d_cols), ptr(d_dists), eps, MIN_SAMPLES, 1, ptr(label), ptr(core), ptr(count), ptr(anchor),
                                  c.ctypes.data, None)
        assert rc == 0, N.last_error()
    out["csr"] = dict(k=K, ef=EF, mode="union", add_self=1, eps=eps, entries=int(g.offsets[-1]), csr_device_s=timed(csr_form, a.warmup, a.repeats),
                      clusters=int(c[0]), core=int(core.sum().item()))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
