"""The minimum-spanning-forest entries (hnswgpu_graph_spanning_forest / _device, hnswgpu_csr_spanning_forest / _device,
csrc/spanning_forest.hip) as far as a box without a GPU can see them: the ABI, every refusal that is answered before a device is
needed, the empty index -- and the contract restated in Python: `spanning_forest`, Kruskal over the edges sorted by (order bits, lo,
hi), and `pair_weights`, the min / max / core rule over any directed graph D.  tests/test_gpu_spanning_forest.py imports both to
build its expected answers from the existing public graph calls, never from the code under test.  Here the model is checked on
hand-made graphs, and against `components` / `cut_and_join` of tests/test_graph_components_abi.py at every cut.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from test_exact_knn_abi import _order_bits
from test_graph_components_abi import components, cut_and_join

ENTRIES = ("hnswgpu_graph_spanning_forest", "hnswgpu_graph_spanning_forest_device", "hnswgpu_csr_spanning_forest",
           "hnswgpu_csr_spanning_forest_device")
A, B, W, COUNT = 0xA5A5A5A5, 0x5A5A5A5A, 0x7FC01234, 0x7777      # (W: a NaN with a payload, compared as bits)


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------- the model
def spanning_forest(n, edges):
    """(a u32[m], b u32[m], w f32[m]) of the minimum spanning forest of the undirected graph on 0 .. n - 1 whose edges are
    (x, y, weight) triples: Kruskal over the edges with x != y, as (lo, hi), sorted by (order bits of the weight, lo, hi) -- a stable
    sort, so of copies that tie the first one listed gives its bits.  The answer is in that order."""
    e = [(min(int(x), int(y)), max(int(x), int(y)), np.float32(w)) for x, y, w in edges if int(x) != int(y)]
    if e:
        key = _order_bits(np.array([w for _, _, w in e], np.float32))
        e = [e[i] for i in sorted(range(len(e)), key=lambda i: (int(key[i]), e[i][0], e[i][1]))]
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    out = []
    for lo, hi, w in e:
        ra, rb = find(lo), find(hi)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            out.append((lo, hi, w))
    return (np.array([x[0] for x in out], np.uint32), np.array([x[1] for x in out], np.uint32), np.array([x[2] for x in out], np.float32))


def pair_weights(n, counts, pos, dists, mode, core_k=0):
    """The contract of the index entries over ANY directed graph D (rows of neighbour positions and f32 distances): the (lo, hi, w)
    triples of the undirected pairs.  union: a pair exists iff either direction is in D and weighs the min of those present; mutual:
    iff both are, and weighs the max.  Compared by order bits; a tie keeps lo -> hi.  core_k >= 1: w = max(w, core(lo), core(hi)),
    core(v) = dists[v, min(core_k, counts[v]) - 1], +0 for an empty row; a tie keeps the earlier of the three."""
    seen = {}

    def ob(x):
        bits = int(np.float32(x).view(np.uint32))
        if bits not in seen:
            seen[bits] = int(_order_bits(np.array([x], np.float32))[0])
        return seen[bits]
    slot = {}
    for i in range(n):
        for s in range(int(counts[i])):
            slot.setdefault((i, int(pos[i, s])), np.float32(dists[i, s]))
    core = [np.float32(dists[v, min(core_k, int(counts[v])) - 1]) if core_k and counts[v] else np.float32(0) for v in range(n)]
    out = []
    for lo, hi in sorted({(min(i, j), max(i, j)) for (i, j) in slot if i != j}):
        fwd, back = slot.get((lo, hi)), slot.get((hi, lo))
        if mode == "mutual" and (fwd is None or back is None):
            continue
        if fwd is None or back is None:
            w = fwd if back is None else back
        elif mode == "mutual":
            w = back if ob(back) > ob(fwd) else fwd
        else:
            w = back if ob(back) < ob(fwd) else fwd
        if core_k:
            for c in (core[lo], core[hi]):
                if ob(c) > ob(w):
                    w = c
        out.append((lo, hi, w))
    return out


def forest_labels(n, a, b, w, cut):
    """`components` of the forest edges whose weight is <= cut (None: all of them)"""
    keep = np.ones(len(a), bool) if cut is None else (np.asarray(w, np.float32) <= np.float32(cut))
    return components(n, zip(np.asarray(a)[keep].tolist(), np.asarray(b)[keep].tolist()))


HAND = dict(counts=np.array([2, 1, 1, 0]), pos=np.array([[1, 2], [0, 0], [3, 0], [0, 0]]),
            d=np.array([[0.5, -0.0], [0.75, 0], [np.nan, 0], [0, 0]], np.float32))


def test_model_on_the_hand_made_graph():
    """the graph of test_graph_components_abi: 0 -> 1 (0.5), 0 -> 2 (-0); 1 -> 0 (0.75); 2 -> 3 (NaN)"""
    a, b, w = spanning_forest(4, pair_weights(4, HAND["counts"], HAND["pos"], HAND["d"], "union"))
    assert list(zip(a.tolist(), b.tolist())) == [(0, 2), (0, 1), (2, 3)]
    assert _bits(w).tolist() == _bits([-0.0, 0.5, np.nan]).tolist()              # the stored bits: the -0 stays a -0
    a, b, w = spanning_forest(4, pair_weights(4, HAND["counts"], HAND["pos"], HAND["d"], "mutual"))
    assert list(zip(a.tolist(), b.tolist())) == [(0, 1)] and w.tolist() == [0.75]
    # core distances: core = (0.5, 0.75, NaN, +0) at core_k = 1; (-0, 0.75, NaN, +0) at 2 (row 0 ascends in the ORDER: 0.5, -0 is a
    # hand-made row, the rule reads the slot whatever it holds)
    got = pair_weights(4, HAND["counts"], HAND["pos"], HAND["d"], "union", 1)
    assert [(lo, hi) for lo, hi, _ in got] == [(0, 1), (0, 2), (2, 3)]
    assert _bits([x[2] for x in got]).tolist() == _bits([0.75, np.nan, np.nan]).tolist()
    got = pair_weights(4, HAND["counts"], HAND["pos"], HAND["d"], "mutual", 2)
    assert [(lo, hi, float(w)) for lo, hi, w in got] == [(0, 1, 0.75)]
    # ties: equal weights go by (lo, hi); of copies of one pair the lighter one, and of equal copies the first, gives the bits
    a, b, w = spanning_forest(3, [(2, 1, 1.0), (1, 0, 1.0), (0, 2, 1.0)])
    assert list(zip(a.tolist(), b.tolist())) == [(0, 1), (0, 2)]
    a, b, w = spanning_forest(2, [(0, 1, 2.0), (1, 0, 0.0), (0, 1, -0.0), (0, 0, -5.0)])
    assert list(zip(a.tolist(), b.tolist())) == [(0, 1)] and _bits(w).tolist() == [0]
    a, b, w = spanning_forest(3, [(0, 1, np.nan), (1, 2, np.inf), (0, 2, -1.0)])
    assert list(zip(a.tolist(), b.tolist())) == [(0, 2), (1, 2)]                 # the NaN is behind +inf
    assert [len(x) for x in spanning_forest(0, [])] == [0, 0, 0] and [len(x) for x in spanning_forest(1, [(0, 0, 1.0)])] == [0, 0, 0]


def test_model_agrees_with_the_components_at_every_cut():
    """for every cut, the components of the forest edges <= cut are `cut_and_join` of D -- on the hand-made graph and on random
    directed graphs whose two directions differ"""
    cases = [(4, HAND["counts"], HAND["pos"], HAND["d"])]
    rng = np.random.default_rng(3)
    for n, k in ((12, 2), (40, 3)):
        counts = rng.integers(0, k + 1, n)
        pos = np.stack([rng.permutation(np.setdiff1d(np.arange(n), [i]))[:k] for i in range(n)])
        d = rng.integers(0, 6, (n, k)).astype(np.float32) / 4
        d[rng.random((n, k)) < 0.1] = np.nan
        d[rng.random((n, k)) < 0.1] = -0.0
        cases.append((n, counts, pos, d))
    for n, counts, pos, d in cases:
        for mode in ("union", "mutual"):
            a, b, w = spanning_forest(n, pair_weights(n, counts, pos, d, mode))
            assert (a < b).all()
            for cut in (None, np.inf, 0.0, -0.0, 0.25, 0.5, 0.75, 1.0, -np.inf):
                want = cut_and_join(n, counts, pos, d, mode, cut)
                got = forest_labels(n, a, b, w, cut)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, mode, cut)
            assert len(a) == n - len(cut_and_join(n, counts, pos, d, mode, None)[1])


# ----------------------------------------------------------------------------------------------------- the ABI
def _small(native, n=50, d=8, f16=False):
    X = np.random.default_rng(1).random((n, d), dtype=np.float32)
    if f16:
        X = native.round_to_f16(X)
    h = native.Hnsw(8, n, 16, 32, "DistL2")
    h.set_build_options(nthreads=1)
    h.parallel_insert(X)
    return X, h


def test_header_declares_the_four_symbols(native):
    N = _N()
    protos = N.HEADER.prototypes
    for name in ENTRIES:
        assert name in protos and name in N.SYMBOLS, name
        assert protos[name][0] is C.c_int
        assert getattr(native.lib(), name) is not None
    assert protos[ENTRIES[0]][2] == ["idx", "k", "ef", "mode", "core_k", "out_a", "out_b", "out_w", "out_n_edges"]
    assert protos[ENTRIES[1]][2] == ["idx", "k", "ef", "mode", "core_k", "d_out_a", "d_out_b", "d_out_w", "out_n_edges", "stream"]
    assert protos[ENTRIES[2]][2] == ["device", "n", "offsets", "cols", "dists", "out_a", "out_b", "out_w", "out_n_edges"]
    assert protos[ENTRIES[3]][2] == ["device", "n", "d_offsets", "d_cols", "d_dists", "d_out_a", "d_out_b", "d_out_w", "out_n_edges", "stream"]
    assert protos[ENTRIES[0]][1][3] is C.c_uint32 and protos[ENTRIES[0]][1][4] is C.c_uint64 and protos[ENTRIES[2]][1][0] is C.c_int
    text = open(N.HEADER_PATH).read()
    doc = text[text.index("minimum spanning forest ---"):text.index("int hnswgpu_csr_spanning_forest_device")]
    for word in ("POSITIONS", "min", "max", "unique", "core_k", "Out of scope", "STORED", "lo -> hi", "-0 equal to +0", "behind +inf", "n - c",
                 "ceil(log2 n) + 1", "2^31 - 1", "2^32", "ONE word", "hnswgpu_symmetric_graph_device", "dendrogram", "F16 storage",
                 "sharding over GPUs"):
        assert word in doc, word
    assert hasattr(native.Hnsw, "knn_graph_spanning_forest") and callable(native.csr_spanning_forest)
    r = native.SpanningForestResult(np.array([0, 2], np.uint32), np.array([1, 3], np.uint32), np.array([0.5, np.nan], np.float32), 2, 5)
    assert r.n_edges == 2 and r.n_vertices == 5
    got = r.labels_at()
    assert isinstance(got, native.ComponentsResult) and got.labels.tolist() == [0, 0, 1, 1, 2] and got.sizes.tolist() == [2, 2, 1]
    got = r.labels_at(float("inf"))                                             # a NaN weight passes no cut
    assert got.labels.tolist() == [0, 0, 1, 2, 3] and got.n_components == 4 and got.labels.dtype == np.uint32
    assert r.labels_at(0.25).n_components == 5


class _Outs:
    """out arrays at their sentinels"""

    def __init__(self, n):
        m = max(n - 1, 1)
        self.a, self.b, self.w = np.full(m, A, np.uint32), np.full(m, B, np.uint32), np.full(m, W, np.uint32).view(np.float32)
        self.count = np.full(1, COUNT, np.uint64)

    def untouched(self):
        return bool((self.a == A).all() and (self.b == B).all() and (self.w.view(np.uint32) == W).all() and self.count[0] == COUNT)


def test_index_entries_answer_every_refusal_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    o = _Outs(50)

    def host(idx=h.handle, k=3, ef=0, mode=0, core_k=0, a=o.a, b=o.b, w=o.w, count=o.count):
        return L.hnswgpu_graph_spanning_forest(idx, k, ef, mode, core_k, _p(a), _p(b), _p(w), _p(count))

    def dev(idx=h.handle, k=3, ef=0, mode=0, core_k=0, a=o.a, b=o.b, w=o.w, count=o.count):
        return L.hnswgpu_graph_spanning_forest_device(idx, k, ef, mode, core_k, _p(a), _p(b), _p(w), _p(count), None)

    for call in (host, dev):
        def refused(word, **kw):
            rc = call(**kw)
            assert rc == N.ERR_ARG, (kw.keys(), rc, N.last_error())
            assert word in N.last_error(), (word, N.last_error())
            assert o.untouched(), kw.keys()
        refused("null", idx=None)
        refused("out_n_edges", count=None)
        for name in ("a", "b", "w"):
            refused("out_a, out_b or out_w", **{name: None})
        for ef in (0, 32):
            refused("knbn", k=0, ef=ef)
            refused("mode", mode=2, ef=ef)
            refused("mode", mode=0xFFFFFFFF, ef=ef)
            big = (1 << 30) // 50 + 1                           # 50 points x 21474837 = 1073741850 slots
            refused(str(50 * big), k=big, ef=ef)
            refused("2^30", k=1 << 40, ef=ef)
            refused("knbn must be", k=0, mode=7, ef=ef)         # two faults at once: knbn is looked at first ...
            refused("out_n_edges", k=0, count=None, ef=ef)      # ... and the answer's slots before either
            refused("core_k", core_k=4, ef=ef)                  # core_k > k
            refused("core_k", core_k=1 << 63, ef=ef)
            refused("mode", core_k=4, mode=2, ef=ef)            # the shape of D first
            refused("core_k", core_k=big + 1, k=big, ef=ef)     # ... and core_k before the source of D
        refused("4096", k=4097)                                # the exact graph's own limit, and not the approximate one's
        h.set_arithmetic("simd8")
        try:
            refused("SIMD8")                                   # ef == 0 only: the graph search serves either arithmetic
            refused("4096", k=4097)                            # two faults at once, in the symmetrised graph's order
        finally:
            h.set_arithmetic("scalar")
    Xh, hh = _small(native, f16=True)
    hh.set_storage("f16")
    for ef in (0, 32):
        for call in (host, dev):
            rc = call(idx=hh.handle, ef=ef)
            assert rc == N.ERR_ARG and "HNSWGPU_STORAGE_F16" in N.last_error() and "HNSWGPU_STORAGE_F32" in N.last_error(), N.last_error()
    assert o.untouched()
    for bad in (dict(knbn=0), dict(knbn=3, mode="both"), dict(knbn=3, ef=0), dict(knbn=3, core_k=4), dict(knbn=3, core_k=-1)):
        with pytest.raises(native.HnswError) as err:           # the Python method hands the refusals on
            h.knn_graph_spanning_forest(**bad)
        assert err.value.code == N.ERR_ARG


def test_csr_entries_answer_every_refusal_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    offs, cols = np.array([0, 1, 2, 2], np.uint64), np.array([1, 2], np.uint32)
    o = _Outs(3)

    def host(n=3, of=offs, co=cols, di=None, a=o.a, b=o.b, w=o.w, count=o.count):
        return L.hnswgpu_csr_spanning_forest(0, n, _p(of), _p(co), _p(di), _p(a), _p(b), _p(w), _p(count))

    def dev(n=3, of=offs, co=cols, di=None, a=o.a, b=o.b, w=o.w, count=o.count):
        return L.hnswgpu_csr_spanning_forest_device(0, n, _p(of), _p(co), _p(di), _p(a), _p(b), _p(w), _p(count), None)

    def refused(call, word, **kw):
        rc = call(**kw)
        assert rc == N.ERR_ARG, (kw.keys(), rc, N.last_error())
        assert word in N.last_error(), (word, N.last_error())
        assert o.untouched(), kw.keys()
    for call in (host, dev):                                   # what either form sees without reading an array
        refused(call, "out_n_edges", count=None)
        for name in ("a", "b", "w"):
            refused(call, "out_a, out_b or out_w", **{name: None})
        refused(call, "2^31", n=1 << 31)
        refused(call, "2^31", n=(1 << 63) + 5)
        refused(call, "offsets", of=None)
        refused(call, "out_n_edges", count=None, n=1 << 31)    # two faults at once
        refused(call, "out_a, out_b or out_w", a=None, of=None)
    # the graph itself: the host form reads its arrays (the device form's validation kernels need a device:
    # tests/test_gpu_spanning_forest.py)
    refused(host, "offsets[0]", of=np.array([1, 1, 2, 2], np.uint64))
    refused(host, "descend", of=np.array([0, 2, 1, 2], np.uint64))
    refused(host, "not below n", co=np.array([1, 3], np.uint32))
    refused(host, "not below n", co=np.array([0xFFFFFFFF, 0], np.uint32))
    refused(host, "2^32", of=np.array([0, 1, 2, 1 << 32], np.uint64))
    refused(host, "2^32", of=np.array([0, 1, 2, (1 << 64) - 1], np.uint64))
    refused(host, "null cols", co=None)
    refused(host, "offsets[0]", of=np.array([3, 2, 1, 0], np.uint64), co=np.array([9, 9], np.uint32))      # two faults at once
    assert "csr spanning forest" in N.last_error()
    # n <= 1: no edge, nothing else written -- whatever the other pointers are
    for call in (host, dev):
        for n in (0, 1):
            count = np.full(1, COUNT, np.uint64)
            assert call(n=n, of=np.zeros(2, np.uint64), co=None, a=None, b=None, w=None, count=count) == N.OK and count[0] == 0
            count[0] = COUNT
            assert call(n=n, of=np.array([0, 1], np.uint64), co=np.zeros(1, np.uint32), count=count) == N.OK and count[0] == 0
        o.count[0] = COUNT
        assert o.untouched()
    for bad in (dict(offsets=[0, 1, 1], cols=[2]), dict(offsets=[0, 2, 2], cols=[0]), dict(offsets=[0, 1, 1], cols=[1], dists=[1.0, 2.0]),
                dict(offsets=[], cols=[])):
        with pytest.raises(native.HnswError) as err:           # the Python function hands the refusals on
            native.csr_spanning_forest(**bad)
        assert err.value.code == N.ERR_ARG
    for offsets, cols in (([0], []), ([0, 0], []), ([0, 1], [0])):
        got = native.csr_spanning_forest(offsets, cols)
        assert got.n_edges == 0 and len(got.a) == 0 and len(got.b) == 0 and len(got.weights) == 0
        assert got.labels_at().n_components == len(offsets) - 1


def test_empty_and_one_point_indexes_have_no_edge_and_need_no_device(native):
    N = _N()
    L = native.lib()
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    for mode in ("union", "mutual"):
        for ef in (None, 16):
            for core_k in (0, 2):
                res = e.knn_graph_spanning_forest(5, ef, mode, core_k)
                assert res.n_edges == 0 and len(res.a) == 0 and len(res.b) == 0 and len(res.weights) == 0
                assert res.a.dtype == np.uint32 and res.b.dtype == np.uint32 and res.weights.dtype == np.float32
                assert res.labels_at().n_components == 0
    e.parallel_insert(np.zeros((0, 8), np.float32))            # (a handle exists from the first insertion on)
    assert e.handle
    one = native.Hnsw(8, 10, 16, 32, "DistL2")
    one.parallel_insert(np.ones((1, 8), np.float32))
    o = _Outs(1)
    for h in (e, one):
        for mode in (0, 1):
            o.count[0] = COUNT
            assert L.hnswgpu_graph_spanning_forest(h.handle, 5, 0, mode, 0, None, None, None, _p(o.count)) == N.OK and o.count[0] == 0
            o.count[0] = COUNT
            assert L.hnswgpu_graph_spanning_forest_device(h.handle, 5, 32, mode, 5, _p(o.a), _p(o.b), _p(o.w), _p(o.count), None) == N.OK
            assert o.count[0] == 0
        o.count[0] = COUNT
        assert o.untouched()
        assert L.hnswgpu_graph_spanning_forest(h.handle, 0, 0, 0, 0, None, None, None, _p(o.count)) == N.ERR_ARG        # still refused
        assert L.hnswgpu_graph_spanning_forest(h.handle, 5, 0, 0, 6, None, None, None, _p(o.count)) == N.ERR_ARG
        assert o.untouched()
    got = one.knn_graph_spanning_forest(5)
    assert got.n_edges == 0 and got.labels_at().labels.tolist() == [0]


def test_without_a_device_a_well_formed_call_reports_no_device(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    offs, cols = np.array([0, 1, 2, 2], np.uint64), np.array([1, 2], np.uint32)
    if L.hnswgpu_device_count() > 0:                           # a box with a GPU answers (tests/test_gpu_spanning_forest.py checks the answers)
        got = h.knn_graph_spanning_forest(3)
        assert 25 <= got.n_edges <= 49 and (got.a < got.b).all()     # (every point has a neighbour: components of two at least)
        got = native.csr_spanning_forest(offs, cols)
        assert got.a.tolist() == [0, 1] and got.b.tolist() == [1, 2]
        return
    with pytest.raises(native.HnswError) as e:
        h.knn_graph_spanning_forest(3)
    assert e.value.code == N.ERR_DEVICE
    with pytest.raises(native.HnswError) as e:
        native.csr_spanning_forest(offs, cols)
    assert e.value.code == N.ERR_DEVICE
    o = _Outs(50)
    rc = L.hnswgpu_graph_spanning_forest_device(h.handle, 3, 0, 0, 0, _p(o.a), _p(o.b), _p(o.w), _p(o.count), None)
    assert rc == N.ERR_DEVICE and N.last_error() and o.untouched()
    o = _Outs(3)
    rc = L.hnswgpu_csr_spanning_forest_device(0, 3, _p(offs), _p(cols), None, _p(o.a), _p(o.b), _p(o.w), _p(o.count), None)
    assert rc == N.ERR_DEVICE and N.last_error() and o.untouched()
