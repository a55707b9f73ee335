"""The exhaustive exact k-NN entries (hnswgpu_exact_search_batch / _device, csrc/exact_knn.hip) as far as a box without a GPU can
see them: the ABI, the argument checks, the "no device" answer, the sanitizer build's source list, and a numpy emulation of the
selection (sorted lists per slab with a running threshold) and of the merge of the slabs' lists.  CPU only."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("hnswgpu_exact_search_batch", "hnswgpu_exact_search_batch_device")


def _N():
    import hnsw_rs_amd._native as N
    return N


def _has_gpu(native):
    return native.lib().hnswgpu_device_count() > 0


def _small(native, n=50, d=8, dist="DistL2"):
    X = np.random.default_rng(1).random((n, d), dtype=np.float32)
    h = native.Hnsw(8, n, 16, 32, dist)
    h.set_build_options(nthreads=1)
    h.parallel_insert(X)
    return X, h


def _bufs(nq, k):
    return (np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint8), np.zeros((nq, k), np.int32),
            np.zeros(nq, np.uint32))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_both_prototypes_are_in_the_header_and_exported(native):
    protos = _N().HEADER.prototypes
    for name in ENTRIES:
        assert name in protos, name
        res, args, names, _ = protos[name]
        assert res is C.c_int
        assert names[:5] == ["idx", "queries" if name.endswith("batch") else "d_queries", "nq", "d", "k"]
        assert getattr(native.lib(), name) is not None
    assert protos[ENTRIES[1]][2][-1] == "stream"
    assert len(protos[ENTRIES[0]][1]) == 12 and len(protos[ENTRIES[1]][1]) == 13


def test_argument_errors(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    Q = X[:3].copy()
    ids, dists, layers, ranks, counts = _bufs(3, 5)
    host = lambda idx, q, nq, d, k, al, na, oi=ids, od=dists, oc=counts: L.hnswgpu_exact_search_batch(
        idx, _p(q), nq, d, k, _p(al), na, _p(oi), _p(od), _p(layers), _p(ranks), _p(oc))
    dev = lambda idx, q, nq, d, k, al, na, oi=ids, od=dists, oc=counts: L.hnswgpu_exact_search_batch_device(
        idx, _p(q), nq, d, k, _p(al), na, _p(oi), _p(od), _p(layers), _p(ranks), _p(oc), None)
    for call in (host, dev):
        assert call(None, Q, 3, 8, 5, None, 0) == N.ERR_ARG
        assert call(h.handle, Q, 3, 8, 0, None, 0) == N.ERR_ARG and "knbn" in N.last_error()          # k == 0
        assert call(h.handle, Q, 3, 7, 5, None, 0) == N.ERR_ARG and "dimension" in N.last_error()     # wrong d
        assert call(h.handle, None, 3, 8, 5, None, 0) == N.ERR_ARG
        assert call(h.handle, Q, 3, 8, 5, None, 0, oi=None) == N.ERR_ARG
        assert call(h.handle, Q, 3, 8, 5, None, 0, oc=None) == N.ERR_ARG
        assert call(h.handle, Q, 3, 8, 5, None, 4) == N.ERR_ARG and "filter" in N.last_error()        # ids announced, none given
        assert call(h.handle, Q, 3, 8, 4097, None, 0) == N.ERR_ARG
    unsorted = np.array([5, 3, 9], np.uint64)
    assert host(h.handle, Q, 3, 8, 5, unsorted, 3) == N.ERR_ARG and "sorted" in N.last_error()
    # an index set to the SIMD-order arithmetic is refused, never answered in the other arithmetic
    h.set_arithmetic("simd8")
    try:
        for call in (host, dev):
            rc = call(h.handle, Q, 3, 8, 5, None, 0)
            assert rc == N.ERR_ARG and "SIMD8" in N.last_error()
    finally:
        h.set_arithmetic("scalar")


def test_without_a_device_a_well_formed_call_reports_no_device(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    Q = X[:3].copy()
    ids, dists, layers, ranks, counts = _bufs(3, 5)
    if _has_gpu(native):  # a box with a GPU answers the call (tests/test_gpu_exact_knn.py checks the answer)
        assert h.exact_search_flat(Q, 5).counts.tolist() == [5, 5, 5]
        return
    rc = L.hnswgpu_exact_search_batch(h.handle, _p(Q), 3, 8, 5, None, 0, _p(ids), _p(dists), _p(layers), _p(ranks), _p(counts))
    assert rc == N.ERR_DEVICE and N.last_error()
    rc = L.hnswgpu_exact_search_batch_device(h.handle, _p(Q), 3, 8, 5, None, 0, _p(ids), _p(dists), None, None, _p(counts), None)
    assert rc == N.ERR_DEVICE and N.last_error()
    for fn in (lambda: h.exact_search_flat(Q, 5), lambda: h.exact_search(Q, 5, allowed_ids=[1, 2, 3]), lambda: h.recall_flat(Q, 5, 16)):
        with pytest.raises(native.HnswError) as e:
            fn()
        assert e.value.code == N.ERR_DEVICE
    with pytest.raises(native.HnswError) as e:
        h.exact_search_flat(Q, 0)
    assert e.value.code == N.ERR_ARG
    with pytest.raises(native.HnswError) as e:
        h.exact_search_flat(Q[:, :5], 3)
    assert e.value.code == N.ERR_ARG


def test_the_sanitizer_scripts_source_list_links_without_undefined_symbols(tmp_path):
    """what tools/asan_host_suite.sh compiles (read from the script), linked with -Wl,-z,defs and no sanitizer: the stand-ins
    define every device entry of the host sources, and the library exports every symbol the header declares"""
    script = open(os.path.join(ROOT, "tools", "asan_host_suite.sh")).read()
    srcs = re.findall(r"\$(C|ROOT)(/[\w/.\-]+\.cpp)", script)
    paths = [os.path.join(ROOT, "hnswlib-rs_amd", "csrc") + p if v == "C" else ROOT + p for v, p in srcs]
    assert any(p.endswith("stub_exact_knn.cpp") for p in paths) and any(p.endswith("stub_device.cpp") for p in paths), paths
    assert len(paths) == len(set(paths)) == 6, paths
    c = os.path.join(ROOT, "hnswlib-rs_amd", "csrc")
    out = tmp_path / "libhnsw_stub.so"
    cmd = ["g++", "-O0", "-std=c++17", "-fPIC", "-ffp-contract=off", "-pthread", "-I" + c, "-I" + os.path.join(ROOT, "include"), "-shared",
           "-Wl,-z,defs", "-o", str(out)] + paths
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(str(out))
    N = _N()
    for name in N.SYMBOLS:
        assert hasattr(lib, name), name


# ----------------------------------------------------------------------------------------------------- selection emulation
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def _order_bits(d):
    """dist_order_bits of dist_order.hpp: u32 whose unsigned order is the order of the f32 values, NaN behind everything"""
    b = d.view(np.uint32).copy()
    b[b == 0x80000000] = 0
    neg = (b & 0x80000000) != 0
    out = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    out[np.isnan(d)] = 0xFFFFFFFF
    return out


class SlabList:
    """list_insert: a sorted list of at most cap keys; the threshold is KEY_NONE until it is full, then its last key"""

    def __init__(self, cap):
        self.cap, self.keys, self.thr, self.inserts = cap, [], KEY_NONE, 0

    def offer_wave(self, keys, ok):
        """64 rows at a time: the ballot against the threshold as it stood, then the passing lanes one by one (each checked again)"""
        mask = [i for i in range(len(keys)) if ok[i] and keys[i] < self.thr]
        for i in mask:
            kb = keys[i]
            if not kb < self.thr:
                continue
            # chunks of 64 from the tail: entries above kb move up one slot, the one that falls off a full list is dropped
            lst, pos = self.keys, 0
            n = len(lst)
            new = list(lst) + [None]
            for c in range((n + 63) // 64 - 1, -1, -1):
                below = 0
                for j in range(c * 64, min(n, c * 64 + 64)):
                    if lst[j] < kb:
                        below += 1
                    else:
                        new[j + 1] = lst[j]
                if below:
                    pos = c * 64 + below
                    break
            new[pos] = kb
            self.keys = new[:min(n + 1, self.cap)]
            self.inserts += 1
            if len(self.keys) == self.cap:
                self.thr = self.keys[-1]


def _emulate(dist, rank, k, slab_rows, allow=None):
    """the device's plan for one query: per slab a SlabList fed 64 rows at a time, then the merge by smallest head"""
    n = len(dist)
    cap = min(k, n)
    keys = (_order_bits(dist).astype(np.uint64) << np.uint64(32)) | rank.astype(np.uint64)
    ok = np.ones(n, bool) if allow is None else allow
    lists = []
    for lo in range(0, n, slab_rows):
        hi = min(n, lo + slab_rows)
        sl = SlabList(cap)
        for r0 in range(lo, hi, 64):
            r1 = min(hi, r0 + 64)
            if ok[r0:r1].any():
                sl.offer_wave([keys[r] for r in range(r0, r1)], ok[r0:r1])
        assert sl.keys == sorted(sl.keys)
        lists.append(sl.keys)
    heads = [0] * len(lists)
    out = []
    cnt = min(k, sum(len(x) for x in lists))
    for _ in range(cnt):
        cur = [lst[h] if h < len(lst) else KEY_NONE for lst, h in zip(lists, heads)]
        s = int(np.argmin(np.array(cur, np.uint64)))
        out.append(cur[s])
        heads[s] += 1
    return np.array(out, np.uint64)


@pytest.mark.parametrize("n,k,slab_rows,levels", [(1000, 10, 256, 7), (1000, 100, 256, 3), (777, 64, 320, 2), (300, 1024, 64, 5),
                                                 (65, 65, 64, 1), (1, 5, 64, 1), (2000, 200, 512, 4000)])
def test_selection_and_merge_emulation_against_lexsort(n, k, slab_rows, levels):
    """random keys with heavy duplication (`levels` distinct distances; 1 = everything ties): tie groups straddle position k and
    the slab boundaries, and the answer is the lexsort by (distance, DataId rank) all the same -- with and without a filter"""
    rng = np.random.default_rng(n * 31 + k)
    for trial in range(3):
        dist = (rng.integers(0, levels, n) / np.float32(levels)).astype(np.float32)
        if trial == 2 and n > 10:
            dist[rng.choice(n, 5, replace=False)] = np.nan      # NaN orders behind every number
            dist[rng.choice(n, 5, replace=False)] = np.inf
        rank = rng.permutation(n).astype(np.uint32)             # position in ascending DataId order: not the row order
        for allow in (None, rng.random(n) < 0.3, np.zeros(n, bool)):
            got = _emulate(dist, rank, k, slab_rows, allow)
            rows = np.arange(n) if allow is None else np.flatnonzero(allow)
            want_rows = rows[np.lexsort((rank[rows], dist[rows]))][:k]   # (np.lexsort puts NaN last, like the keys)
            want = (_order_bits(dist[want_rows]).astype(np.uint64) << np.uint64(32)) | rank[want_rows].astype(np.uint64)
            assert np.array_equal(got, want), (n, k, slab_rows, levels, trial)
            if len(want_rows) == k and k < len(rows):               # the cut goes through a tie group: DataId decides
                nxt = rows[np.lexsort((rank[rows], dist[rows]))][k]
                if dist[nxt] == dist[want_rows[-1]]:
                    assert rank[nxt] > rank[want_rows[-1]]


def test_order_bits_are_monotone_and_reversible():
    v = np.array([0.0, -0.0, 1e-45, 1.0, 1.0000001, 3e38, np.inf, np.nan], np.float32)
    u = _order_bits(v)
    assert u[0] == u[1] and np.all(np.diff(u[1:].astype(np.int64)) > 0)
    back = np.where((u & 0x80000000) != 0, u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)
    assert np.array_equal(back[:7], np.abs(v[:7]))
