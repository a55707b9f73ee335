#!/usr/bin/env python3
"""What half-precision storage (Hnsw.set_storage("f16")) does to the search rate and to the replica's bytes, on the index shapes of
BASELINE configs 2, 3 and 5 (the last at 240 000 points: out of the Infinity Cache):
    python tools/storage_rate.py [--shapes sift1m,glove25,mnist784_hbm] [--steps 7] [--warmup 3]
Per shape: ONE index built GPU-assisted from round_to_f16 data; the same batch (device-resident queries, the device entry) on
the same handle at F32 and at F16, ALTERNATING in one process -- warm-up, then the median of --steps timed steps each, with the
spread; call rate and hnswgpu_last_search_kernel_ms; the two answer sets must be bit-equal (exit status 1 otherwise);
device_bytes of both.  And, so that the effect of the data change (coarser values, more ties) is not taken for an effect of the
storage, the plain F32 rate of an index built the same way from the UNROUNDED data.  One JSON line per shape on stdout, progress on
stderr."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {  # bench.py's configs: n, d, dist, M, ef_c, ef, batch sizes
    "sift1m": dict(n=1_000_000, d=128, dist="DistL2", M=16, efc=200, ef=64, nqs=(10_000, 100_000)),
    "glove25": dict(n=1_200_000, d=25, dist="DistCosine", M=24, efc=400, ef=128, nqs=(10_000,)),
    "mnist784_hbm": dict(n=240_000, d=784, dist="DistL2", M=32, efc=400, ef=200, nqs=(10_000,)),
}
K = 10


def log(*a):
    print("[storage_rate]", *a, file=sys.stderr, flush=True)


class DeviceCall:
    """hnswgpu_search_batch_device on torch buffers: what bench.py times"""

    def __init__(self, torch, H, h, Q):
        self.torch, self.L, self.h, self.nq, self.d = torch, H.lib(), h, Q.shape[0], Q.shape[1]
        self.q = torch.from_numpy(Q).cuda()
        self.ids = torch.zeros((self.nq, K), dtype=torch.int64, device="cuda")
        self.dd = torch.zeros((self.nq, K), dtype=torch.float32, device="cuda")
        self.lay = torch.zeros((self.nq, K), dtype=torch.uint8, device="cuda")
        self.rk = torch.zeros((self.nq, K), dtype=torch.int32, device="cuda")
        self.cnt = torch.zeros(self.nq, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def __call__(self, ef):
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        rc = self.L.hnswgpu_search_batch_device(self.h.handle, p(self.q), self.nq, self.d, K, ef, p(self.ids), p(self.dd), p(self.lay), p(self.rk),
                                                p(self.cnt), None, None)
        assert rc == 0, rc

    def answers(self):
        self.torch.cuda.synchronize()
        return tuple(t.cpu().numpy() for t in (self.ids, self.dd.view(self.torch.int32), self.lay, self.rk, self.cnt))


def step(call, h, ef):
    t0 = time.perf_counter()
    call(ef)
    dt = time.perf_counter() - t0
    return dt, h.last_search_kernel_ms()


def summary(samples, nq):
    ts, ks = [s[0] for s in samples], [s[1] for s in samples]
    med = statistics.median(ts)
    return dict(queries_per_s=nq / med, queries_per_s_min=nq / max(ts), queries_per_s_max=nq / min(ts), call_ms=med * 1e3,
                search_kernel_ms=statistics.median(ks), search_kernel_ms_min=min(ks), search_kernel_ms_max=max(ks), steps=len(ts))


def build(H, s, X):
    h = H.Hnsw(s["M"], s["n"], 16, s["efc"], s["dist"])
    h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
    t0 = time.perf_counter()
    h.parallel_insert(X)
    return h, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="sift1m,glove25,mnist784_hbm")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lean", action="store_true", help="strict ties off, like a plain bench.py run")
    ap.add_argument("--no-unrounded", action="store_true", help="skip the second index (unrounded data)")
    a = ap.parse_args()
    assert a.steps >= 7, "the median of at least 7 timed steps"
    import torch
    torch.cuda.init()
    import bench
    import hnsw_rs_amd as H
    H.build_native()
    ok = True
    for name in a.shapes.split(","):
        s = SHAPES[name]
        n, d, ef = s["n"], s["d"], s["ef"]
        raw = bench.synth(n, d, 0x5EED0001, "clustered")
        X = H.round_to_f16(raw)
        h, t_build = build(H, s, X)
        if a.lean:
            h.set_strict_ties(False)
        log(f"{name}: built from rounded data in {t_build:.1f} s")
        out = dict(shape=name, n=n, d=d, dist=s["dist"], M=s["M"], ef=ef, k=K, strict_ties=not a.lean, build_s=t_build, batches={})
        Qall = bench.synth(max(s["nqs"]), d, 0x5EED0002, "clustered")
        for storage in ("f32", "f16"):
            h.set_storage(storage)
            h.upload(0)
            out[f"device_bytes_{storage}"] = h.device_bytes(0)
        for nq in s["nqs"]:
            call = DeviceCall(torch, H, h, np.ascontiguousarray(Qall[:nq]))
            samples, answers, same = {"f32": [], "f16": []}, {}, True
            # alternating in one process: every round re-uploads the replica of the other kind (untimed), warms it up, times one step
            for rnd in range(a.steps):
                for storage in ("f32", "f16"):
                    h.set_storage(storage)
                    h.upload(0)
                    for _ in range(a.warmup):
                        call(ef)
                    samples[storage].append(step(call, h, ef))
                    answers[storage] = call.answers()
                same = same and all(np.array_equal(x, y) for x, y in zip(answers["f32"], answers["f16"]))   # every round's answers
            ok = ok and same
            b = dict(f32=summary(samples["f32"], nq), f16=summary(samples["f16"], nq), answers_bit_equal=bool(same))
            b["f16_over_f32_rate"] = b["f16"]["queries_per_s"] / b["f32"]["queries_per_s"]
            b["f16_over_f32_kernel_ms"] = b["f16"]["search_kernel_ms"] / b["f32"]["search_kernel_ms"]
            out["batches"][str(nq)] = b
            log(f"{name} nq {nq}: f32 {b['f32']['queries_per_s']:.0f} q/s (kernel {b['f32']['search_kernel_ms']:.3f} ms), "
                f"f16 {b['f16']['queries_per_s']:.0f} q/s (kernel {b['f16']['search_kernel_ms']:.3f} ms), bit-equal {same}")
            del call
        del h
        torch.cuda.empty_cache()
        if not a.no_unrounded:
            h, t_build = build(H, s, raw)
            if a.lean:
                h.set_strict_ties(False)
            h.upload(0)
            out["unrounded_f32"] = {}
            for nq in s["nqs"]:
                call = DeviceCall(torch, H, h, np.ascontiguousarray(Qall[:nq]))
                for _ in range(a.warmup):
                    call(ef)
                out["unrounded_f32"][str(nq)] = summary([step(call, h, ef) for _ in range(a.steps)], nq)
                del call
            del h
            torch.cuda.empty_cache()
        print(json.dumps(out), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
