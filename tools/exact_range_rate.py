#!/usr/bin/env python3
"""Rate of the exact range search (hnswgpu_exact_range_search_batch) on 1M x 128 DistL2 with 10 000 queries, two radius cases:
  (a) each query's own 10th-nearest distance (about 10 answers per query),
  (b) one radius for all, the median 1000th-nearest distance of a sample of queries (about 1000 answers per query),
against the yardstick hnswgpu_exact_search_batch at k = 10 of the same build on the same inputs (host entries all).
    exact_range_rate.py --dump-dir DIR                  builds the index, dumps it and the radii into DIR, prints one JSON line
    exact_range_rate.py --dump-dir DIR --trace-run      loads that dump and makes one warm and one measured call per case: to be run
                                                        under `rocprofv3 --kernel-trace --output-format csv -d OUT -- python ...`
    exact_range_rate.py --parse-trace OUT               the count / fill / sort / decode split of the measured calls from that trace
    exact_range_rate.py --dump-dir DIR --one-filter     times the existing one-filter exact k-NN call (30 % allowed, k = 10) on the
                                                        dumped index; with --package-root DIR2 through the package of another checkout
                                                        (the parent commit, built there): the regression check
Warm-up calls first, then the median and the spread of --repeats calls."""
import argparse
import csv
import ctypes as C
import glob
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
N_POINTS, DIM, DIST, BASENAME = 1_000_000, 128, "DistL2", "range_rate"


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


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def range_call(H, h, Q, radii, cap, outs):
    """the host entry itself with `cap` slots (0: count only); returns (rc, offsets)"""
    nq, d = Q.shape
    offs = np.zeros(nq + 1, np.uint64)
    ptrs = [_p(o) for o in outs] if cap else [None] * 4
    rc = H.lib().hnswgpu_exact_range_search_batch(h.handle, _p(Q), nq, d, _p(radii), None, 0, cap, _p(offs), *ptrs)
    return rc, offs


def load(H, a):
    h = H.HnswIo(a.dump_dir, BASENAME).load_hnsw(DIST)
    h.upload(0)
    return h


def parse_trace(out_dir):
    """per call of the entry (batches of one chunk of tiles): milliseconds in the count pass, the fill pass, the sort and the decoding.
    A slab kernel followed by the scan kernel is a count pass, any other a fill pass; prep + slab + scan open a call."""
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    calls, cur = [], None
    for i, (t0, t1, name) in enumerate(rows):
        ms = (t1 - t0) / 1e6
        after = [rows[j][2] for j in range(i + 1, min(i + 3, len(rows)))] + ["", ""]
        if "exact_knn_prep_kernel" in name and "exact_range_slab_kernel" in after[0] and "exact_range_scan_kernel" in after[1]:
            cur = dict(count_ms=0.0, scan_ms=0.0, fill_ms=0.0, sort_ms=0.0, decode_ms=0.0, prep_ms=0.0, start=t0, end=t1)   # a call's count pass
            calls.append(cur)
        if cur is None:
            continue
        if "exact_range_slab_kernel" in name:
            cur["count_ms" if "exact_range_scan_kernel" in after[0] else "fill_ms"] += ms
        elif "exact_range_scan_kernel" in name:
            cur["scan_ms"] += ms
        elif "exact_range_decode_kernel" in name:
            cur["decode_ms"] += ms
        elif "rocprim" in name:
            cur["sort_ms"] += ms
        elif "exact_knn_prep_kernel" in name:
            cur["prep_ms"] += ms
        else:
            continue
        cur["end"] = t1
    return [c for c in calls if c["count_ms"] > 0.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump-dir")
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--parse-trace")
    ap.add_argument("--one-filter", action="store_true")
    ap.add_argument("--package-root", default=None)
    a = ap.parse_args()
    if a.parse_trace:
        calls = parse_trace(a.parse_trace)
        # the trace run makes, per case, a count-only call and two full calls: the last of each triple is the warm one
        out = dict(mode="trace", calls=[{k: round(v, 3) for k, v in c.items() if k.endswith("_ms")} | dict(span_ms=round((c["end"] - c["start"]) / 1e6, 3))
                                        for c in calls])
        print(json.dumps(out), flush=True)
        return
    import torch
    torch.cuda.init()
    import hnsw_rs_amd as H
    H.build_native()
    n, d, nq = N_POINTS, DIM, a.nq
    Q = clustered(nq, d, 2)
    if a.one_filter:
        h = load(H, a)
        allowed = np.flatnonzero(np.random.default_rng(7).random(n) < 0.3).astype(np.uint64)
        t = timed(lambda: h.exact_search_flat(Q, 10, allowed), a.warmup, a.repeats)
        print(json.dumps(dict(mode="one_filter", package_root=ROOT, n=n, d=d, nq=nq, k=10, allowed=len(allowed), seconds=t)), flush=True)
        return
    if a.trace_run:
        h = load(H, a)
        for case in ("a", "b"):
            radii = np.load(os.path.join(a.dump_dir, f"radii_{case}.npy"))
            rc, offs = range_call(H, h, Q, radii, 0, None)
            total = int(offs[-1])
            outs = [np.zeros(total, t) for t in (np.uint64, np.float32, np.uint8, np.int32)]
            for _ in range(2):
                rc, offs = range_call(H, h, Q, radii, total, outs)
                assert rc == 0
        return
    X = clustered(n, d, 1)
    h = H.Hnsw(8, n, 16, 16, DIST)   # (the graph plays no part in an exhaustive search: a cheap one)
    h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
    t0 = time.perf_counter()
    h.parallel_insert(X)
    h.upload(0)
    print(f"== built and uploaded in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    out = dict(mode="rate", n=n, d=d, dist=DIST, nq=nq, repeats=a.repeats, warmup=a.warmup)
    knn = h.exact_search_flat(Q, 10)
    out["exact_knn_k10_s"] = timed(lambda: h.exact_search_flat(Q, 10), a.warmup, a.repeats)
    sample = h.exact_search_flat(Q[:64], 1000)
    cases = {"a": np.ascontiguousarray(knn.dists[:, 9]), "b": np.full(nq, np.median(sample.dists[:, 999]), np.float32)}
    for case, radii in cases.items():
        rc, offs = range_call(H, h, Q, radii, 0, None)
        total = int(offs[-1])
        outs = [np.zeros(total, t) for t in (np.uint64, np.float32, np.uint8, np.int32)]
        rc, offs = range_call(H, h, Q, radii, total, outs)
        assert rc == 0, H._native.last_error()
        counts = np.diff(offs).astype(np.int64)
        r = dict(answers=total, answers_per_query_mean=float(counts.mean()), answers_per_query_max=int(counts.max()),
                 call_s=timed(lambda: range_call(H, h, Q, radii, total, outs), a.warmup, a.repeats),
                 count_only_call_s=timed(lambda: range_call(H, h, Q, radii, 0, None), a.warmup, a.repeats),
                 python_method_s=timed(lambda: h.exact_range_search_flat(Q, radii), a.warmup, a.repeats))
        r["pairs_per_s"] = n * nq / r["call_s"]["median"]                      # pairs answered; each is evaluated twice
        r["pair_evaluations_per_s"] = 2 * n * nq / r["call_s"]["median"]
        r["ratio_to_exact_knn_k10"] = r["call_s"]["median"] / out["exact_knn_k10_s"]["median"]
        if case == "a":  # equal work: the first 10 answers of every query are the k-NN answer
            r["first_10_are_the_knn_answer"] = bool(all(np.array_equal(outs[0][int(offs[q]):int(offs[q]) + 10], knn.ids[q]) for q in range(nq)))
        out["case_" + case] = r
        if a.dump_dir:
            np.save(os.path.join(a.dump_dir, f"radii_{case}.npy"), radii)
    if a.dump_dir:
        h.file_dump(a.dump_dir, BASENAME)
    print(json.dumps(out), flush=True)
    if out["case_a"].get("first_10_are_the_knn_answer") is False:
        sys.exit(1)


if __name__ == "__main__":
    main()
