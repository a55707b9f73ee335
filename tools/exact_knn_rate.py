#!/usr/bin/env python3
"""Rate of the exhaustive exact k-NN entry (hnswgpu_exact_search_batch_device) on the index shapes of BASELINE configs 2, 3 and 5,
with two comparators measured on the same box and inputs:
  (a) the only exact path there was before: hnswgpu_eval_distance_matrix in row slices + selection on the host, on a query count
      small enough to finish -- the new entry (host buffers, like (a)) is timed on the same queries;
  (b) bench.py's ground_truth (torch GEMM shortlist + f64 re-evaluation): context only -- not exact, not the index's arithmetic.
    tools/gpu_call.sh exact_rate OUTDIR [--shapes sift1m,glove25,mnist784] [--nq 10000]      -> OUTDIR/rate.json
One JSON line per shape on stdout, progress on stderr.  Warm-up calls first, then the median and the spread of `--repeats` calls.

Filter-set mode (--filter-set): hnswgpu_exact_search_batch_filter_set through Hnsw.exact_search_filters_flat on the first shape,
with --filters F filters of --selectivity LO[,HI] (fractions of the points, spread evenly from LO to HI) named by the queries
--naming random | same (every query names filter 0) | own (query q names filter q: F = nq), against the host loop it replaces
(one Hnsw.exact_search_flat per filter on that filter's queries) and against the one-filter call with filter 0 for every query.
--package-root DIR measures the package of another checkout (the parent commit, built there): what that package lacks -- the set
call before it existed -- is left out of the line, so both commits are timed by the same code on the same inputs."""
import argparse
import ctypes as C
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

SHAPES = {  # BASELINE configs 2, 3, 5
    "sift1m": dict(n=1_000_000, d=128, dist="DistL2"),
    "glove25": dict(n=1_200_000, d=25, dist="DistCosine"),
    "mnist784": dict(n=60_000, d=784, dist="DistL2"),
}
# A NOMINAL model of the inner loop of exact_knn_slab_kernel: three vector-ALU operations per (query, element) -- DistL2: subtract,
# multiply, add; DistCosine: multiply, widen, add in f64.  The loop as compiled for DistL2 packs the multiplies and adds of two
# queries (per 2 queries x 4 elements: 8 v_sub_f32, 4 v_pk_mul_f32, 4 v_pk_add_f32, about 6 v_mov_b32 to pair the lanes), so the
# "fraction of the VALU bound" below is a fraction of this model, not of the issue slots of the compiled loop.
VALU_PER_ELEMENT = {"DistL2": 3, "DistCosine": 3}
HBM_PEAK = 8.0e12  # bytes / s, MI355X data sheet


def clustered(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = rng.random((256, d), dtype=np.float32)
    return (centres[rng.integers(0, 256, n)] + np.float32(0.05) * rng.standard_normal((n, d), dtype=np.float32)).astype(np.float32)


def gpu_clock_hz():
    """the maximum engine clock rocminfo reports for the first gfx950 agent of this box (2.4 GHz, the data sheet's, if it cannot be read)"""
    import re
    import subprocess
    try:
        text = subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True, timeout=60).stdout
        for agent in text.split("Agent ")[1:]:
            if re.search(r"Name:\s+gfx950", agent):
                m = re.search(r"Max Clock Freq\. \(MHz\):\s+(\d+)", agent)
                if m:
                    return int(m.group(1)) * 1e6
    except (OSError, subprocess.SubprocessError):
        pass
    return 2.4e9


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts), max(ts)


def filter_set_mode(a):
    import torch
    torch.cuda.init()
    import hnsw_rs_amd as H
    H.build_native()
    name = a.shapes.split(",")[0]
    s = SHAPES[name]
    n, d, dist, k, nq = s["n"], s["d"], s["dist"], a.k, a.nq
    sel = [float(x) for x in a.selectivity.split(",")]
    nf = nq if a.naming == "own" else a.filters
    fracs = np.linspace(sel[0], sel[-1], nf)
    rng = np.random.default_rng(7)
    X, Q = clustered(n, d, 1), clustered(nq, d, 2)
    h = H.Hnsw(8, n, 16, 16, dist)
    h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
    t0 = time.perf_counter()
    h.parallel_insert(X)
    h.upload(0)
    print(f"== {name}: built and uploaded in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    filters = [np.flatnonzero(rng.random(n) < f).astype(np.uint64) for f in fracs]   # origin ids are the row numbers
    filter_of = {"random": rng.integers(0, nf, nq), "same": np.zeros(nq, np.int64), "own": np.arange(nq)}[a.naming].astype(np.uint32)
    out = dict(mode="filter_set", shape=name, n=n, d=d, dist=dist, nq=nq, k=k, filters=nf, selectivity=[float(fracs[0]), float(fracs[-1])],
               naming=a.naming, repeats=a.repeats, warmup=a.warmup, package_root=ROOT)

    def loop():   # what a caller had to do before: one call per filter with the queries that name it
        res = {}
        for f in np.unique(filter_of):
            qs = np.flatnonzero(filter_of == f)
            res[int(f)] = (qs, h.exact_search_flat(Q[qs], k, filters[int(f)]))
        return res
    med, lo, hi = timed(lambda: h.exact_search_flat(Q, k, filters[0]), a.warmup, a.repeats)
    out["one_filter_call_filter0_s"] = dict(median=med, min=lo, max=hi)
    med, lo, hi = timed(loop, min(a.warmup, 1), a.repeats)
    out["host_loop_s"] = dict(median=med, min=lo, max=hi, calls=int(len(np.unique(filter_of))))
    if hasattr(h, "exact_search_filters_flat"):
        med, lo, hi = timed(lambda: h.exact_search_filters_flat(Q, k, filters, filter_of), a.warmup, a.repeats)
        out["set_call_s"] = dict(median=med, min=lo, max=hi)
        out["host_loop_over_set_call"] = out["host_loop_s"]["median"] / med
        got, same = h.exact_search_filters_flat(Q, k, filters, filter_of), True
        for f, (qs, r) in loop().items():   # equal work: the set call's rows are the loop's
            same = same and np.array_equal(got.ids[qs], r.ids) and np.array_equal(got.dists[qs].view(np.uint32), r.dists.view(np.uint32)) \
                and np.array_equal(got.counts[qs], r.counts)
        out["same_answers_as_host_loop"] = bool(same)
    print(json.dumps(out), flush=True)
    if out.get("same_answers_as_host_loop") is False:
        sys.exit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sift1m,glove25,mnist784")
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq-small", type=int, default=64, help="queries of comparator (a)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-torch-comparator", action="store_true")
    ap.add_argument("--filter-set", action="store_true")
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--selectivity", default="0.01,0.5")
    ap.add_argument("--naming", choices=("random", "same", "own"), default="random")
    ap.add_argument("--package-root", default=None)
    a = ap.parse_args()
    if a.filter_set:
        return filter_set_mode(a)
    import torch
    torch.cuda.init()
    import hnsw_rs_amd as H
    import hnsw_rs_amd._native as N
    H.build_native()
    L = H.lib()
    prop = torch.cuda.get_device_properties(0)
    clock_hz = gpu_clock_hz()
    cus = prop.multi_processor_count
    failed = []
    for name in a.shapes.split(","):
        s = SHAPES[name]
        n, d, dist, k, nq = s["n"], s["d"], s["dist"], a.k, a.nq
        print(f"== {name}: data", file=sys.stderr)
        X, Q = clustered(n, d, 1), clustered(nq, d, 2)
        h = H.Hnsw(8, n, 16, 16, dist)  # (the graph plays no part in an exhaustive search: a cheap one)
        h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
        t0 = time.perf_counter()
        h.parallel_insert(X)
        h.upload(0)
        print(f"== {name}: built and uploaded in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
        dq = torch.from_numpy(Q).cuda()
        ids = torch.zeros((nq, k), dtype=torch.int64, device="cuda")
        dd = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(nq, dtype=torch.int32, device="cuda")

        def call():
            rc = L.hnswgpu_exact_search_batch_device(h.handle, C.c_void_p(dq.data_ptr()), nq, d, k, None, 0, C.c_void_p(ids.data_ptr()),
                                                     C.c_void_p(dd.data_ptr()), None, None, C.c_void_p(cnt.data_ptr()), None)
            assert rc == 0, N.last_error()
        med, lo, hi = timed(call, a.warmup, a.repeats)
        stride = (d + 31) // 32 * 32
        tiles = (nq + 15) // 16
        out = dict(shape=name, n=n, d=d, dist=dist, nq=nq, k=k, seconds_median=med, seconds_min=lo, seconds_max=hi, repeats=a.repeats,
                   pair_evaluations_per_s=n * nq / med, ms_per_10000_queries=med * 1e3 * 10_000 / nq,
                   valu_bound_pairs_per_s=cus * 64 * clock_hz / (VALU_PER_ELEMENT[dist] * 4 * ((d + 3) // 4)), clock_hz=clock_hz, cus=cus,
                   bytes_read_per_query=n * stride * 4 * tiles / nq, )
        out["fraction_of_valu_bound"] = out["pair_evaluations_per_s"] / out["valu_bound_pairs_per_s"]
        out["fraction_of_hbm_peak"] = out["bytes_read_per_query"] * nq / med / HBM_PEAK
        # (a) eval_distance_matrix in slices of rows + host selection, and the new entry (host buffers) on the same few queries
        ns = min(a.nq_small, nq)
        Qs = np.ascontiguousarray(Q[:ns])

        def old_path():
            best_d = np.full((ns, 0), np.inf, np.float32)
            best_i = np.zeros((ns, 0), np.int64)
            for r0 in range(0, n, 100_000):
                D = H.eval_distance_matrix(dist, Qs, X[r0:r0 + 100_000], 64)
                best_d = np.concatenate([best_d, D], 1)
                best_i = np.concatenate([best_i, np.broadcast_to(np.arange(r0, r0 + D.shape[1]), D.shape)], 1)
                keep = np.argsort(best_d, 1, kind="stable")[:, :k]
                best_d, best_i = np.take_along_axis(best_d, keep, 1), np.take_along_axis(best_i, keep, 1)
            return best_i, best_d
        ta = timed(old_path, 1, 3)
        tn = timed(lambda: h.exact_search_flat(Qs, k), 1, 3)
        oi, od = old_path()
        nw = h.exact_search_flat(Qs, k)
        out["comparator_a"] = dict(nq=ns, eval_matrix_plus_host_selection_s=ta[0], new_entry_host_buffers_s=tn[0], speedup=ta[0] / tn[0],
                                   same_distance_bits=bool(np.array_equal(od.view(np.uint32), nw.dists.view(np.uint32))),
                                   same_ids=bool(np.array_equal(oi, nw.ids.astype(np.int64))))
        ca = out["comparator_a"]
        if ca["speedup"] < 1.0 or not ca["same_distance_bits"] or not ca["same_ids"]:  # the one condition on speed, and on equal work
            failed.append(name)
        if not a.no_torch_comparator:
            import bench
            Xd = torch.from_numpy(X).cuda()
            tb = timed(lambda: (bench.ground_truth(torch, Xd, dq, k, dist), torch.cuda.synchronize()), 1, 3)
            out["comparator_b_bench_ground_truth_s"] = tb[0]
            del Xd
        print(json.dumps(out), flush=True)
        del h, dq, ids, dd, cnt
        torch.cuda.empty_cache()
    if failed:
        print(f"FAILED against comparator (a): {failed}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
