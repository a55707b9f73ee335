#!/usr/bin/env python3
"""Rates of the filter-set search (hnswgpu_search_batch_filter_set_device) beside the one-filter call
(hnswgpu_search_batch_filtered_device) on the cached bench index of a config: 10 000 queries, ef 64, ~30 % of the points allowed
per filter, with 1, 16 and 10 000 distinct filters -- device-resident buffers on a stream, warm-up calls, then timed calls, the
median with its range.  Run bench.py for the config first (it builds and caches the index).  One JSON line per setting.
HNSW_MI355X_LIB=<another build's library> measures that build (the parent commit: `--only-one-filter`)."""
import argparse
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="sift1m")
ap.add_argument("--cache-dir", default=os.environ.get("HNSW_BENCH_CACHE", "/tmp/hnsw_mi355x_bench_cache"))
ap.add_argument("--nq", type=int, default=10000)
ap.add_argument("--ef", type=int, default=64)
ap.add_argument("--allowed", type=float, default=0.3)
ap.add_argument("--filters", default="1,16,10000")
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--only-one-filter", action="store_true", help="only hnswgpu_search_batch_filtered_device (a build without the set entries)")
args = ap.parse_args()
import torch  # noqa: E402  (first: see INTEGRATION.md, loading order)
import hnsw_rs_amd as H  # noqa: E402

cfg = bench.CONFIGS[args.config]
marks = sorted(f for f in glob.glob(os.path.join(args.cache_dir, f"bench_{args.config}_*.done"))
               if len(os.path.basename(f)) == len(f"bench_{args.config}_") + 12 + 5)
if not marks:
    raise SystemExit("run bench.py for this config first (it builds and caches the index)")
index = H.HnswIo(args.cache_dir, os.path.basename(marks[-1])[:-5]).load_hnsw(cfg["dist"])
index.upload(0)
L = H.lib()
dev = torch.device("cuda", 0)
n, d, k, nq = cfg["n"], cfg["d"], cfg["k"], args.nq
stream = torch.cuda.Stream(dev)
gen = torch.Generator(device=dev)
gen.manual_seed(0xF117)
with torch.cuda.stream(stream):
    q = torch.from_numpy(bench.synth(nq, d, 0x5EED0002, "clustered")).to(dev)
    ids = torch.zeros((nq, k), dtype=torch.int64, device=dev)
    dists = torch.zeros((nq, k), dtype=torch.float32, device=dev)
    counts = torch.zeros((nq,), dtype=torch.int32, device=dev)


def make_set(n_filters):
    """n_filters sorted id vectors (origin ids of the bench index are 0..n-1), each ~args.allowed of the points, on the device"""
    parts, offsets = [], [0]
    with torch.cuda.stream(stream):
        for _ in range(n_filters):
            v = torch.nonzero(torch.rand(n, device=dev, generator=gen) < args.allowed).flatten()
            parts.append(v)
            offsets.append(offsets[-1] + int(v.numel()))
        flat = torch.cat(parts)
        off = torch.tensor(offsets, dtype=torch.int64, device=dev)
        of = (torch.arange(nq, device=dev) % n_filters).to(torch.int32)
    stream.synchronize()
    return flat, off, of, offsets


def timed(call):
    ms = []
    for i in range(args.warmup + args.calls):
        stream.synchronize()
        t0 = time.perf_counter()
        rc = call()
        stream.synchronize()
        assert rc == 0, H._native.last_error()
        if i >= args.warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return ms


def report(what, n_filters, ms):
    med = ms[len(ms) // 2]
    print(json.dumps({"call": what, "config": args.config, "nq": nq, "ef": args.ef, "allowed": args.allowed, "filters": n_filters,
                      "ms_median": round(med, 3), "ms_min": round(ms[0], 3), "ms_max": round(ms[-1], 3),
                      "queries_per_s": round(nq / med * 1e3), "full_answers": float((counts == k).float().mean())}), flush=True)


flat, off, of, offsets = make_set(1)
report("hnswgpu_search_batch_filtered_device", 1, timed(lambda: L.hnswgpu_search_batch_filtered_device(
    index.handle, q.data_ptr(), nq, d, k, args.ef, flat.data_ptr(), offsets[1], ids.data_ptr(), dists.data_ptr(), None, None, counts.data_ptr(),
    None, stream.cuda_stream, None)))
if not args.only_one_filter:
    for nf in [int(x) for x in args.filters.split(",")]:
        if nf != 1:
            del flat, off, of
            flat, off, of, offsets = make_set(nf)
        report("hnswgpu_search_batch_filter_set_device", nf, timed(lambda: L.hnswgpu_search_batch_filter_set_device(
            index.handle, q.data_ptr(), nq, d, k, args.ef, flat.data_ptr(), off.data_ptr(), nf, of.data_ptr(), ids.data_ptr(), dists.data_ptr(),
            None, None, counts.data_ptr(), None, stream.cuda_stream, None)))
