#!/usr/bin/env python3
"""Rate of the approximate range search (hnswgpu_range_search_batch_device) on BASELINE config 2's shape: 1M x 128 DistL2, 10 000
queries, ef_first = 64, ef_max = 1024, at three radii -- one radius per case for all queries, chosen from the exact answers so that
the median ball holds about 0, 10 and 100 points (the exact range search's median count is reported next to it).  Per case:
  the call's queries/s (device entry, every buffer in HBM, cap = the total), and the host entry through Hnsw.range_search_flat;
  hnswgpu_search_batch_device's rate at the modal settling ef with knbn = ef on the same queries (existing code: the comparator),
  and at ef_first;
  the exact range search's rate on the same queries (host entry);
  range_recall_flat: recall by id against the exact range search, and the share of saturated queries;
  the histogram of out_ef;
  the rounds taken apart with existing code: hnswgpu_search_batch_device at every ef of the sequence on the queries pending in that
  round (their sum is what the call spends in searches) and on the queries settling there (their sum is every query searched once,
  at its final ef): the second ratio is what restarting costs.
Nothing is asserted.  Warm-up calls first, then the median and the spread of --repeats calls.  One JSON line."""
import argparse
import collections
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_POINTS, DIM, DIST = 1_000_000, 128, "DistL2"


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
    ap.add_argument("--n", type=int, default=N_POINTS)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--efc", type=int, default=64)
    ap.add_argument("--ef-first", type=int, default=64)
    ap.add_argument("--ef-max", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import hnsw_rs_amd as H
    H.build_native()
    L = H.lib()
    n, d, nq = a.n, DIM, a.nq
    X, Q = clustered(n, d, 1), clustered(nq, d, 2)
    h = H.Hnsw(a.m, n, 16, a.efc, DIST)
    h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
    t0 = time.perf_counter()
    h.parallel_insert(X)
    h.upload(0)
    out = dict(n=n, d=d, dist=DIST, nq=nq, m=a.m, ef_construction=a.efc, ef_first=a.ef_first, ef_max=a.ef_max, repeats=a.repeats, warmup=a.warmup,
               build_and_upload_s=time.perf_counter() - t0)
    knn = h.exact_search_flat(Q, 100)
    # one radius per case: 40 % of the queries have their nearest point inside (median ball: 0 points), the median 10th / 100th distance
    radius = {"0": float(np.quantile(knn.dists[:, 0], 0.4)), "10": float(np.median(knn.dists[:, 9])), "100": float(np.median(knn.dists[:, 99]))}
    stream = torch.cuda.Stream()
    dq = torch.from_numpy(Q).cuda()

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    def search_rate(ef, rows=None):
        """hnswgpu_search_batch_device with knbn = ef on all queries, or on the rows named"""
        sub = dq if rows is None else torch.from_numpy(np.ascontiguousarray(Q[rows])).cuda()
        m = len(sub)
        o = (torch.zeros((m, ef), dtype=torch.int64, device="cuda"), torch.zeros((m, ef), dtype=torch.float32, device="cuda"),
             torch.zeros((m, ef), dtype=torch.uint8, device="cuda"), torch.zeros((m, ef), dtype=torch.int32, device="cuda"),
             torch.zeros(m, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()

        def call():
            rc = L.hnswgpu_search_batch_device(h.handle, ptr(sub), m, d, ef, ef, *[ptr(t) for t in o], None, C.c_void_p(stream.cuda_stream))
            assert rc == 0, H._native.last_error()
        t = timed(call, a.warmup, a.repeats)
        return dict(ef=ef, queries=m, seconds=t, queries_per_s=m / t["median"])

    def rounds_of(got):
        """what the rounds are made of, from existing code alone: per ef of the sequence the search of the queries PENDING in that
        round (what the call runs) and of the queries that SETTLE there (what a search that never restarted would run)"""
        out_rounds, e = [], a.ef_first
        while True:
            pending, settling = np.flatnonzero(got.ef >= e), np.flatnonzero(got.ef == e)
            r = dict(ef=e, pending=len(pending), settling=len(settling))
            if len(pending):
                r["search_pending_s"] = search_rate(e, pending)["seconds"]["median"]
            if len(settling):
                r["search_settling_s"] = search_rate(e, settling)["seconds"]["median"]
            out_rounds.append(r)
            if e >= a.ef_max:
                break
            e = min(2 * e, a.ef_max)
        return out_rounds

    out["search_batch_device_at_ef_first"] = search_rate(a.ef_first)
    for case, r in radius.items():
        radii = np.full(nq, r, np.float32)
        exact = h.exact_range_search_flat(Q, radii)
        got = h.range_search_flat(Q, radii, a.ef_first, a.ef_max)
        total = int(got.offsets[-1])
        hist = collections.Counter(got.ef.tolist())
        modal = max(hist, key=lambda e: (hist[e], -e))
        dr = torch.from_numpy(radii).cuda()
        o_off = torch.zeros(nq + 1, dtype=torch.int64, device="cuda")
        o = (torch.zeros(max(total, 1), dtype=torch.int64, device="cuda"), torch.zeros(max(total, 1), dtype=torch.float32, device="cuda"),
             torch.zeros(max(total, 1), dtype=torch.uint8, device="cuda"), torch.zeros(max(total, 1), dtype=torch.int32, device="cuda"))
        o_ef, o_fl = torch.zeros(nq, dtype=torch.int32, device="cuda"), torch.zeros(nq, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def call():
            rc = L.hnswgpu_range_search_batch_device(h.handle, ptr(dq), nq, d, ptr(dr), a.ef_first, a.ef_max, None, 0, max(total, 1), ptr(o_off),
                                                     *[ptr(t) for t in o], ptr(o_ef), ptr(o_fl), C.c_void_p(stream.cuda_stream))
            assert rc == 0, H._native.last_error()
        t = timed(call, a.warmup, a.repeats)
        same = bool(np.array_equal(o_off.cpu().numpy().astype(np.uint64), got.offsets) and np.array_equal(o[0][:total].cpu().numpy().astype(np.uint64), got.ids))
        comparator = search_rate(modal)
        recall, saturated = h.range_recall_flat(Q, radii, a.ef_first, a.ef_max)
        c = dict(radius=r, exact_median_count=float(np.median(exact.counts)), exact_mean_count=float(exact.counts.mean()), exact_total=int(exact.offsets[-1]),
                 answers=total, device_entry_s=t, queries_per_s=nq / t["median"], device_entry_equals_host_entry=same,
                 host_entry_python_s=timed(lambda: h.range_search_flat(Q, radii, a.ef_first, a.ef_max), a.warmup, a.repeats),
                 ef_histogram={str(e): hist[e] for e in sorted(hist)}, modal_ef=modal, search_batch_device_at_modal_ef=comparator,
                 ratio_to_search_at_modal_ef=t["median"] / comparator["seconds"]["median"],
                 ratio_to_search_at_ef_first=t["median"] / out["search_batch_device_at_ef_first"]["seconds"]["median"],
                 exact_range_search_python_s=timed(lambda: h.exact_range_search_flat(Q, radii), a.warmup, a.repeats),
                 recall_by_id=recall, saturated_share=saturated)
        c["exact_range_queries_per_s"] = nq / c["exact_range_search_python_s"]["median"]
        c["rounds"] = rounds_of(got)
        c["sum_search_pending_s"] = sum(r.get("search_pending_s", 0.0) for r in c["rounds"])      # the searches the call makes
        c["sum_search_settling_s"] = sum(r.get("search_settling_s", 0.0) for r in c["rounds"])    # every query once, at its final ef
        c["call_over_its_searches"] = t["median"] / c["sum_search_pending_s"]
        c["restart_cost"] = c["sum_search_pending_s"] / c["sum_search_settling_s"]
        out["median_ball_" + case] = c
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
