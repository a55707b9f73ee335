#!/usr/bin/env python3
"""Wall time of HDBSCAN on the device (k = 16, ef = 64, UNION, core_k = 5, min_cluster_size = 10, excess of mass):
  * hnswhdb_graph next to hnswgpu_graph_dendrogram on the same index (both host entries through the Python methods);
  * the forest form alone on its device entry (hnswhdb_forest_device, the forest already in HBM; it builds the dendrogram
    itself) next to what a caller did before: hnswgpu_forest_dendrogram_device, the dendrogram and the weights downloaded (timed on
    their own, from HBM into pageable host arrays) and one pass of the SAME definitions on ONE host core -- compiled C++ (g++ -O2,
    built into a temporary directory when the tool starts; without a compiler the tool says so and leaves the pass out);
  * the selection alone (hnswhds_select_device) on the condensed tree that the device form left in HBM: at the defaults, checked
    byte for byte against the first stage's own selection, and with allow_single_cluster, an epsilon at the median birth weight and
    max_cluster_size = n / 100.
n x 128 DistL2 (clustered, the data of tools/spanning_forest_rate.py), the index built in the process (GPU-assisted, M = 16,
ef_construction 64).
    hdbscan_rate.py --n 100000
    hdbscan_rate.py --n 1000000
One warm-up call, then the median of --repeats.  K, L and the depth of the cluster tree are reported.  The index form, the device form
and the host pass are compared before anything is reported: integers, weights, labels and probabilities byte for byte, stabilities
within rows 2^-53 (the host pass sums in row order).  One JSON line.  Per-kernel times: run the tool under
`rocprofv3 --kernel-trace --stats -- python tools/hdbscan_rate.py --n N`."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DIM, DIST, K, EF, CORE_K, MCS = 128, "DistL2", 16, 64, 5, 10

HOST_PASS = r"""
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>
static double lambda_of(float w) {
    if (w != w || w == std::numeric_limits<float>::infinity()) return 0.0;
    if (w <= 0.0f) return std::numeric_limits<double>::infinity();
    return 1.0 / (double)w;
}
static double term(double row, double birth, uint32_t size) { return row == birth ? 0.0 : (row - birth) * (double)size; }
// the definitions of hnsw_mi355x_hdbscan.h, one after the other, over a dendrogram in host memory; excess of mass
extern "C" int host_hdbscan(uint32_t n, uint32_t m, const uint32_t* left, const uint32_t* right, const uint32_t* sizes, const float* w, uint32_t mcs,
                            int32_t* labels, float* prob, uint32_t* point_cluster, float* point_w, uint32_t* cparent, float* cbirth, uint32_t* csize,
                            double* stability, uint8_t* selected, uint32_t* counts) {
    const uint32_t nodes = n + m, none = 0xFFFFFFFFu;
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<uint32_t> par(nodes, none), cluster(nodes, 0), top(nodes);
    auto size_of = [&](uint32_t x) { return x < n ? 1u : sizes[x - n]; };
    for (uint32_t e = 0; e < m; ++e) par[left[e]] = par[right[e]] = n + e;
    uint32_t big_roots = 0;
    for (uint32_t x = 0; x < nodes; ++x) big_roots += par[x] == none && size_of(x) >= mcs;
    uint32_t k = 1;
    cparent[0] = none, cbirth[0] = inf, csize[0] = n;
    for (uint32_t x = nodes; x-- > 0;) {  // a parent's id is above its children's
        top[x] = x;
        if (size_of(x) >= mcs) {
            const uint32_t p = par[x];
            const bool head = p == none ? big_roots >= 2 : (size_of(left[p - n]) >= mcs && size_of(right[p - n]) >= mcs);
            if (head) {
                cluster[x] = k;
                cparent[k] = p == none ? 0 : cluster[p];
                cbirth[k] = p == none ? inf : w[p - n];
                csize[k] = size_of(x);
                ++k;
            } else {
                cluster[x] = p == none ? 0 : cluster[p];
            }
        } else if (par[x] != none && size_of(par[x]) < mcs) {
            top[x] = top[par[x]];
        }
    }
    std::vector<double> maxlam(k, 0.0), s_of(k, 0.0), below(k, 0.0);
    std::vector<uint32_t> kids(k, 0), best(k, none), label_of(k, 0), depth(k, 0);
    for (uint32_t c = 0; c < k; ++c) stability[c] = 0.0;
    for (uint32_t v = 0; v < n; ++v) {
        const uint32_t p = par[top[v]];
        point_cluster[v] = p == none ? 0 : cluster[p];
        point_w[v] = p == none ? inf : w[p - n];
        const double lam = lambda_of(point_w[v]);
        stability[point_cluster[v]] += term(lam, lambda_of(cbirth[point_cluster[v]]), 1);
        if (lam > maxlam[point_cluster[v]]) maxlam[point_cluster[v]] = lam;
    }
    for (uint32_t c = 1; c < k; ++c) {
        const double lam = lambda_of(cbirth[c]);
        stability[cparent[c]] += term(lam, lambda_of(cbirth[cparent[c]]), csize[c]);
        if (lam > maxlam[cparent[c]]) maxlam[cparent[c]] = lam;
        ++kids[cparent[c]];
    }
    std::vector<uint8_t> wins(k, 0);
    for (uint32_t c = k; c-- > 1;) {
        wins[c] = kids[c] == 0 || stability[c] >= below[c];
        s_of[c] = stability[c] >= below[c] || kids[c] == 0 ? stability[c] : below[c];
        below[cparent[c]] += s_of[c];
    }
    uint32_t n_labels = 0, deepest = 0;
    selected[0] = 0;
    for (uint32_t c = 1; c < k; ++c) {
        const uint32_t p = cparent[c];
        depth[c] = depth[p] + 1;
        if (depth[c] > deepest) deepest = depth[c];
        best[c] = p != 0 && best[p] != none ? best[p] : (wins[c] ? c : none);
        selected[c] = best[c] == c;
        if (selected[c]) label_of[c] = n_labels++;
    }
    for (uint32_t v = 0; v < n; ++v) {
        const uint32_t q = best[point_cluster[v]];
        if (q == none) {
            labels[v] = -1, prob[v] = 0.0f;
            continue;
        }
        labels[v] = (int32_t)label_of[q];
        const double lam = lambda_of(point_w[v]);
        prob[v] = maxlam[q] == 0.0 || lam >= maxlam[q] ? 1.0f : (float)(lam / maxlam[q]);
    }
    counts[0] = k, counts[1] = n_labels, counts[2] = deepest;
    return 0;
}
"""


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


def host_pass(tmp):
    """fn(n, left, right, sizes, w, mcs) -> dict of arrays, or None where no compiler is found"""
    src, lib = os.path.join(tmp, "host_hdbscan.cpp"), os.path.join(tmp, "host_hdbscan.so")
    with open(src, "w") as f:
        f.write(HOST_PASS)
    try:
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", lib], check=True, capture_output=True)
        fn = C.CDLL(lib).host_hdbscan
    except (OSError, subprocess.CalledProcessError):
        return None
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint32] + [C.c_void_p] * 10

    def run(n, left, right, sizes, w, mcs, slots):
        o = dict(labels=np.empty(n, np.int32), prob=np.empty(n, np.float32), point_cluster=np.empty(n, np.uint32), point_w=np.empty(n, np.float32),
                 cparent=np.empty(slots, np.uint32), cbirth=np.empty(slots, np.float32), csize=np.empty(slots, np.uint32),
                 stability=np.empty(slots, np.float64), selected=np.empty(slots, np.uint8), counts=np.zeros(3, np.uint32))
        rc = fn(n, len(left), left.ctypes.data, right.ctypes.data, sizes.ctypes.data, w.ctypes.data, mcs, *[x.ctypes.data for x in o.values()])
        assert rc == 0
        return o
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, required=True)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import hnsw_rs_amd as H
    H.build_native()
    L = H.lib()
    n = a.n
    X = clustered(n, DIM, 1)
    h = H.Hnsw(16, n, 16, 64, DIST)
    h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
    t0 = time.perf_counter()
    h.parallel_insert(X)
    h.upload(0)
    out = dict(n=n, d=DIM, dist=DIST, k=K, ef=EF, mode="union", core_k=CORE_K, min_cluster_size=MCS, method="eom", repeats=a.repeats, warmup=a.warmup,
               build_and_upload_s=time.perf_counter() - t0)
    out["dendrogram_s"] = timed(lambda: h.knn_graph_dendrogram(K, EF, "union", CORE_K), a.warmup, a.repeats)
    out["hdbscan_s"] = timed(lambda: h.hdbscan(MCS, K, EF, "union", CORE_K), a.warmup, a.repeats)
    d, r = h.knn_graph_dendrogram(K, EF, "union", CORE_K), h.hdbscan(MCS, K, EF, "union", CORE_K)
    for x, y in ((r.forest.a, d.a), (r.forest.b, d.b), (r.forest.weights, d.weights), (r.dendrogram.left, d.left), (r.dendrogram.right, d.right),
                 (r.dendrogram.sizes, d.sizes)):
        assert x.tobytes() == y.tobytes()
    m = d.n_edges
    slots = int(L.hnswhdb_max_clusters(n, MCS))
    out["edges"], out["roots"], out["clusters"], out["labels"], out["noise"] = m, int(len(d.roots())), r.n_clusters, r.n_labels, int((r.labels < 0).sum())
    # the forest form alone, the forest in HBM
    as_i32 = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32).copy()).cuda()  # noqa: E731
    d_a, d_b, d_w = as_i32(d.a), as_i32(d.b), as_i32(d.weights)
    d_den = [torch.zeros(max(m, 1), dtype=torch.int32, device="cuda") for _ in range(3)]
    d_out = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(4)] + [torch.zeros(slots, dtype=torch.int32, device="cuda") for _ in range(3)]
    d_out += [torch.zeros(slots, dtype=torch.float64, device="cuda"), torch.zeros(slots, dtype=torch.uint8, device="cuda")]
    counts = np.zeros(2, np.uint64)
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def device_form():
        rc = L.hnswhdb_forest_device(0, n, m, ptr(d_a), ptr(d_b), ptr(d_w), MCS, 0, *[ptr(t) for t in d_out], counts[0:1].ctypes.data,
                                             counts[1:2].ctypes.data, None)
        assert rc == 0, H._native.last_error()

    def dendrogram_form():
        rc = L.hnswgpu_forest_dendrogram_device(0, n, m, ptr(d_a), ptr(d_b), *[ptr(t) for t in d_den], None)
        assert rc == 0, H._native.last_error()
    out["forest_hdbscan_device_s"] = timed(device_form, a.warmup, a.repeats)
    out["forest_dendrogram_device_s"] = timed(dendrogram_form, a.warmup, a.repeats)
    # the selection alone on the condensed tree that the device form left in HBM (hnswhds_select_device): at the defaults, where it
    # must give the first stage's own bytes, and with the three options set
    kk = r.n_clusters
    s_out = [torch.zeros(slots, dtype=torch.uint8, device="cuda")] + [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3)]
    s_out += [torch.zeros(slots, dtype=torch.float64, device="cuda")]
    n_labels = np.zeros(1, np.uint64)
    births = r.cluster_birth_w[np.isfinite(r.cluster_birth_w)]
    eps = float(np.float32(np.median(births)) * np.float32(1.0001)) if len(births) else 1.0
    tree = [ptr(d_out[i]) for i in (4, 5, 6, 7, 2, 3)]
    torch.cuda.synchronize()

    def select_form(allow, e, max_size):
        rc = L.hnswhds_select_device(0, n, kk, *tree, 0, allow, e, max_size, *[ptr(t) for t in s_out], n_labels.ctypes.data, None)
        assert rc == 0, H._native.last_error()
    out["select_options"] = dict(allow_single_cluster=1, cluster_selection_epsilon=eps, max_cluster_size=n // 100)
    out["select_device_options_s"] = timed(lambda: select_form(1, eps, n // 100), a.warmup, a.repeats)
    out["select_options_labels"] = int(n_labels[0])
    out["select_device_s"] = timed(lambda: select_form(0, 0.0, 0), a.warmup, a.repeats)
    sel = [t.cpu().numpy() for t in s_out]
    assert int(n_labels[0]) == r.n_labels and sel[0][:kk].tobytes() == r.selected.astype(np.uint8).tobytes() and sel[1].tobytes() == r.labels.tobytes()
    assert sel[2].view(np.float32).tobytes() == r.probabilities.tobytes()
    got = [t.cpu().numpy() for t in d_out]
    assert (int(counts[0]), int(counts[1])) == (r.n_clusters, r.n_labels)
    for x, y in ((got[0], r.labels), (got[1].view(np.float32), r.probabilities), (got[2].view(np.uint32), r.point_cluster),
                 (got[3].view(np.float32), r.point_w), (got[4].view(np.uint32)[:kk], r.cluster_parent), (got[5].view(np.float32)[:kk], r.cluster_birth_w),
                 (got[6].view(np.uint32)[:kk], r.cluster_size), (got[7][:kk], r.stability), (got[8][:kk], r.selected.astype(np.uint8))):
        assert x.tobytes() == y.tobytes()
    # what a caller did before: the dendrogram and the weights downloaded, then one host core
    host = [np.empty(m, np.uint32) for _ in range(3)] + [np.empty(m, np.float32)]

    def download():
        for dst, t in zip(host[:3], d_den):
            dst[:] = t.cpu().numpy().view(np.uint32)[:m]
        host[3][:] = d_w.cpu().numpy().view(np.float32)
    out["download_dendrogram_s"] = timed(download, a.warmup, a.repeats)
    with tempfile.TemporaryDirectory() as tmp:
        run = host_pass(tmp)
        out["host_pass"] = "c++ (g++ -O2)" if run else "none: no compiler"
        if run:
            out["host_pass_s"] = timed(lambda: run(n, *host, MCS, slots), a.warmup, a.repeats)
            ref = run(n, *host, MCS, slots)
            assert (int(ref["counts"][0]), int(ref["counts"][1])) == (r.n_clusters, r.n_labels), (ref["counts"], r.n_clusters, r.n_labels)
            out["cluster_tree_depth"] = int(ref["counts"][2])
            for x, y in ((ref["point_cluster"], r.point_cluster), (ref["point_w"], r.point_w), (ref["cparent"][:kk], r.cluster_parent),
                         (ref["cbirth"][:kk], r.cluster_birth_w), (ref["csize"][:kk], r.cluster_size)):
                assert x.tobytes() == y.tobytes()
            # (the selection hangs on the stabilities, which the host pass sums in another order: a near-tie may fall the other way)
            out["host_pass_differs"] = dict(selected=int((ref["selected"][:kk] != r.selected).sum()), labels=int((ref["labels"] != r.labels).sum()),
                                            prob=int((ref["prob"].view(np.uint32) != r.probabilities.view(np.uint32)).sum()))
            rows = np.bincount(r.point_cluster, minlength=kk) + np.bincount(r.cluster_parent[1:], minlength=kk)
            assert (np.abs(ref["stability"][:kk] - r.stability) <= 2 * rows * 2.0 ** -53 * np.maximum(ref["stability"][:kk], r.stability)).all()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
