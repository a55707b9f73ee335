"""The connected-components entries (hnswgpu_graph_components / _device, hnswgpu_csr_components / _device,
csrc/graph_components.hip) as far as a box without a GPU can see them: the ABI, every refusal that is answered before a device is
needed, the empty index -- and the contract restated in Python: `components`, a plain union-find over lists with the numbering rule,
and `cut_and_join`, the cut applied to a directed graph D and then UNION / MUTUAL exactly as `symmetrise` of
tests/test_symmetric_graph_abi.py joins.  tests/test_gpu_graph_components.py imports both to build its expected answers from the
existing public graph calls, never from the code under test.  Here the model is checked on hand-made graphs.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from test_symmetric_graph_abi import symmetrise

ENTRIES = ("hnswgpu_graph_components", "hnswgpu_graph_components_device", "hnswgpu_csr_components", "hnswgpu_csr_components_device")
LABEL, SIZE, COUNT = 0xA5A5A5A5, 0x5A5A5A5A, 0x7777


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ----------------------------------------------------------------------------------------------------- the model
def components(n, edges):
    """(labels u32[n], sizes u32[c]) of the undirected graph on 0 .. n - 1 with the given (a, b) pairs: a union-find over a list,
    the smaller root wins; components numbered by their smallest vertex, ascending"""
    parent = list(range(n))

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    for a, b in edges:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    labels, sizes, number = [], [], {}
    for v in range(n):
        r = find(v)
        if r not in number:                                     # (v == r: a root is the smallest vertex of its tree)
            assert r == v
            number[r] = len(sizes)
            sizes.append(0)
        labels.append(number[r])
        sizes[number[r]] += 1
    return np.array(labels, np.uint32), np.array(sizes, np.uint32)


def cut_and_join(n, counts, pos, dists, mode, max_dist):
    """The contract of the index entries over ANY directed graph D (rows of neighbour positions and f32 distances, as `symmetrise`
    takes it): the cut is applied to D first -- a slot stays iff max_dist is None or its f32 distance <= max_dist, an ordered
    comparison: a NaN never stays --, `symmetrise` joins what is left under `mode`, and `components` labels the result."""
    k = pos.shape[1] if n else 0
    kept_counts, kept_pos, kept_dists = np.zeros(n, np.int64), np.zeros((n, max(k, 1)), np.int64), np.zeros((n, max(k, 1)), np.float32)
    for i in range(n):
        for s in range(int(counts[i])):
            d = np.float32(dists[i, s])
            if max_dist is None or bool(d <= np.float32(max_dist)):
                kept_pos[i, kept_counts[i]], kept_dists[i, kept_counts[i]] = pos[i, s], d
                kept_counts[i] += 1
    offsets, cols, _, _, _ = symmetrise(n, kept_counts, kept_pos, kept_dists, mode)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets.astype(np.int64)))
    return components(n, zip(rows.tolist(), cols.tolist()))


def csr_edges(offsets, cols, dists=None, max_dist=None):
    """the (row, col) pairs of a CSR that survive the cut"""
    offsets = np.asarray(offsets, np.int64)
    rows = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))
    keep = np.ones(len(rows), bool) if max_dist is None else (np.asarray(dists, np.float32)[:len(rows)] <= np.float32(max_dist))
    return list(zip(rows[keep].tolist(), np.asarray(cols, np.int64)[:len(rows)][keep].tolist()))


def test_components_numbers_by_smallest_vertex():
    lab, sizes = components(1, [])
    assert lab.tolist() == [0] and sizes.tolist() == [1]
    lab, sizes = components(0, [])
    assert lab.tolist() == [] and sizes.tolist() == []
    lab, sizes = components(6, [(5, 1), (4, 2), (2, 2), (1, 5), (3, 5)])         # {0} {1, 3, 5} {2, 4}; a self-loop, a repeat
    assert lab.tolist() == [0, 1, 2, 1, 2, 1] and sizes.tolist() == [1, 3, 2]
    lab, sizes = components(5, [(4, 3), (3, 2), (2, 1), (1, 0)])                 # a path named from its far end
    assert lab.tolist() == [0] * 5 and sizes.tolist() == [5]
    lab, sizes = components(4, [(3, 0)])
    assert lab.tolist() == [0, 1, 2, 0] and sizes.tolist() == [2, 1, 1]


def test_model_on_the_hand_made_graph_under_every_cut():
    """the graph of test_symmetric_graph_abi.test_model_on_a_hand_made_graph: 0 -> 1 (0.5), 0 -> 2 (-0); 1 -> 0 (0.75); 2 -> 3 (NaN)"""
    counts = np.array([2, 1, 1, 0])
    pos = np.array([[1, 2], [0, 0], [3, 0], [0, 0]])
    d = np.array([[0.5, -0.0], [0.75, 0], [np.nan, 0], [0, 0]], np.float32)

    def got(mode, cut):
        lab, sizes = cut_and_join(4, counts, pos, d, mode, cut)
        return lab.tolist(), sizes.tolist()
    # no cut: every slot counts, the NaN one too
    assert got("union", None) == ([0, 0, 0, 0], [4])
    assert got("mutual", None) == ([0, 0, 1, 2], [2, 1, 1])                      # only 0 <-> 1 is named both ways
    # +inf: everything but the NaN
    assert got("union", np.inf) == ([0, 0, 0, 1], [3, 1])
    assert got("mutual", np.inf) == ([0, 0, 1, 2], [2, 1, 1])
    # 0.5: 0 -> 1 stays, 1 -> 0 (0.75) goes -- the pair is no longer mutual; -0 <= 0.5
    assert got("union", 0.5) == ([0, 0, 0, 1], [3, 1])
    assert got("mutual", 0.5) == ([0, 1, 2, 3], [1, 1, 1, 1])
    # 0.0: only the -0 slot is left, since -0 == +0
    assert got("union", 0.0) == ([0, 1, 0, 2], [2, 1, 1])
    assert got("mutual", 0.0) == ([0, 1, 2, 3], [1, 1, 1, 1])
    assert got("union", -0.0) == got("union", 0.0)
    assert csr_edges([0, 2, 3, 4, 4], [1, 2, 0, 3], d[[0, 0, 1, 2], [0, 1, 0, 0]], 0.5) == [(0, 1), (0, 2)]
    assert csr_edges([0, 2, 3, 4, 4], [1, 2, 0, 3]) == [(0, 1), (0, 2), (1, 0), (2, 3)]


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
    assert protos[ENTRIES[0]][2] == ["idx", "k", "ef", "mode", "max_dist", "out_label", "out_sizes", "out_n_components"]
    assert protos[ENTRIES[1]][2] == ["idx", "k", "ef", "mode", "max_dist", "d_out_label", "d_out_sizes", "out_n_components", "stream"]
    assert protos[ENTRIES[2]][2] == ["device", "n", "offsets", "cols", "dists", "max_dist", "out_label", "out_sizes", "out_n_components"]
    assert protos[ENTRIES[3]][2] == ["device", "n", "d_offsets", "d_cols", "d_dists", "max_dist", "d_out_label", "d_out_sizes", "out_n_components",
                                     "stream"]
    assert protos[ENTRIES[0]][1][3] is C.c_uint32 and protos[ENTRIES[2]][1][0] is C.c_int
    text = open(N.HEADER_PATH).read()
    doc = text[text.index("connected components, cut optional"):text.index("int hnswgpu_csr_components_device")]
    for word in ("POSITIONS", "HOST pointer", "never counts", "-0 equals +0", "smallest position", "WEAKLY", "2^31 - 1", "2^32", "ONE word",
                 "hnswgpu_symmetric_graph_device", "12 n bytes", "Out of scope"):
        assert word in doc, word
    assert hasattr(native.Hnsw, "knn_graph_components") and callable(native.csr_components)
    r = native.ComponentsResult(np.zeros(3, np.uint32), np.array([3], np.uint32), 1)
    assert r.n_components == 1 and r.labels.tolist() == [0, 0, 0] and r.sizes.tolist() == [3]


class _Outs:
    """out arrays at their sentinels"""

    def __init__(self, n):
        self.label, self.sizes, self.count = np.full(max(n, 1), LABEL, np.uint32), np.full(max(n, 1), SIZE, np.uint32), np.full(1, COUNT, np.uint64)

    def untouched(self):
        return bool((self.label == LABEL).all() and (self.sizes == SIZE).all() and self.count[0] == COUNT)


def test_index_entries_answer_every_refusal_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    o = _Outs(50)
    nan, one = np.array([np.nan], np.float32), np.array([1.0], np.float32)

    def host(idx=h.handle, k=3, ef=0, mode=0, cut=None, label=o.label, count=o.count):
        return L.hnswgpu_graph_components(idx, k, ef, mode, _p(cut), _p(label), _p(o.sizes), _p(count))

    def dev(idx=h.handle, k=3, ef=0, mode=0, cut=None, label=o.label, count=o.count):
        return L.hnswgpu_graph_components_device(idx, k, ef, mode, _p(cut), _p(label), _p(o.sizes), _p(count), None)

    for call in (host, dev):
        def refused(word, **kw):
            rc = call(**kw)
            assert rc == N.ERR_ARG, (kw.keys(), rc, N.last_error())
            assert word in N.last_error(), (word, N.last_error())
            assert o.untouched(), kw.keys()
        refused("null", idx=None)
        refused("out_n_components", count=None)
        refused("out_label", label=None)
        refused("NaN", cut=nan)
        for ef in (0, 32):
            refused("knbn", k=0, ef=ef)
            refused("knbn", k=0, ef=ef, cut=one)
            refused("mode", mode=2, ef=ef)
            refused("mode", mode=0xFFFFFFFF, ef=ef)
            big = (1 << 30) // 50 + 1                           # 50 points x 21474837 = 1073741850 slots
            refused(str(50 * big), k=big, ef=ef)
            refused("2^30", k=1 << 40, ef=ef)
            refused("knbn must be", k=0, mode=7, ef=ef)         # two faults at once: knbn is looked at first ...
            refused("NaN", k=0, cut=nan, ef=ef)                 # ... and the cut before either
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
    for bad in (dict(knbn=0), dict(knbn=3, mode="both"), dict(knbn=3, ef=0), dict(knbn=3, max_dist=float("nan"))):
        with pytest.raises(native.HnswError) as err:           # the Python method hands the refusals on
            h.knn_graph_components(**bad)
        assert err.value.code == N.ERR_ARG


def test_csr_entries_answer_every_refusal_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    offs, cols = np.array([0, 1, 2, 2], np.uint64), np.array([1, 2], np.uint32)
    dists = np.array([0.5, 0.25], np.float32)
    o = _Outs(3)
    nan, one = np.array([np.nan], np.float32), np.array([1.0], np.float32)

    def host(n=3, of=offs, co=cols, di=None, cut=None, label=o.label, count=o.count):
        return L.hnswgpu_csr_components(0, n, _p(of), _p(co), _p(di), _p(cut), _p(label), _p(o.sizes), _p(count))

    def dev(n=3, of=offs, co=cols, di=None, cut=None, label=o.label, count=o.count):
        return L.hnswgpu_csr_components_device(0, n, _p(of), _p(co), _p(di), _p(cut), _p(label), _p(o.sizes), _p(count), None)

    def refused(call, word, **kw):
        rc = call(**kw)
        assert rc == N.ERR_ARG, (kw.keys(), rc, N.last_error())
        assert word in N.last_error(), (word, N.last_error())
        assert o.untouched(), kw.keys()
    for call in (host, dev):                                   # what either form sees without reading an array
        refused(call, "out_n_components", count=None)
        refused(call, "out_label", label=None)
        refused(call, "NaN", cut=nan, di=dists)
        refused(call, "dists", cut=one)
        refused(call, "2^31", n=1 << 31)
        refused(call, "2^31", n=(1 << 63) + 5)
        refused(call, "offsets", of=None)
        refused(call, "out_n_components", count=None, cut=nan)  # two faults at once
        refused(call, "NaN", cut=nan, n=1 << 31)
    # the graph itself: the host form reads its arrays (the device form's validation kernels need a device:
    # tests/test_gpu_graph_components.py)
    refused(host, "offsets[0]", of=np.array([1, 1, 2, 2], np.uint64))
    refused(host, "descend", of=np.array([0, 2, 1, 2], np.uint64))
    refused(host, "not below n", co=np.array([1, 3], np.uint32))
    refused(host, "not below n", co=np.array([0xFFFFFFFF, 0], np.uint32))
    refused(host, "2^32", of=np.array([0, 1, 2, 1 << 32], np.uint64))
    refused(host, "2^32", of=np.array([0, 1, 2, (1 << 64) - 1], np.uint64))
    refused(host, "null cols", co=None)
    refused(host, "offsets[0]", of=np.array([3, 2, 1, 0], np.uint64), co=np.array([9, 9], np.uint32))      # two faults at once
    # n == 0: no vertex, no component, nothing else written -- whatever the other pointers are
    for call in (host, dev):
        count = np.full(1, COUNT, np.uint64)
        assert call(n=0, of=np.zeros(1, np.uint64), co=None, label=None, count=count) == N.OK and count[0] == 0
        assert (o.label == LABEL).all() and (o.sizes == SIZE).all()
    for bad in (dict(offsets=[0, 1], cols=[0], dists=None, max_dist=1.0), dict(offsets=[0, 1], cols=[0], dists=[1.0], max_dist=float("nan")),
                dict(offsets=[0, 1], cols=[1]), dict(offsets=[0, 2], cols=[0])):
        with pytest.raises(native.HnswError) as err:           # the Python function hands the refusals on
            native.csr_components(**bad)
        assert err.value.code == N.ERR_ARG
    got = native.csr_components([0], [])
    assert got.n_components == 0 and len(got.labels) == 0 and len(got.sizes) == 0


def test_empty_index_has_no_component_and_needs_no_device(native):
    N = _N()
    L = native.lib()
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    for mode in ("union", "mutual"):
        for ef in (None, 16):
            for cut in (None, 0.5):
                res = e.knn_graph_components(5, ef, mode, cut)
                assert res.n_components == 0 and len(res.labels) == 0 and len(res.sizes) == 0
                assert res.labels.dtype == np.uint32 and res.sizes.dtype == np.uint32
    e.parallel_insert(np.zeros((0, 8), np.float32))            # (a handle exists from the first insertion on)
    assert e.handle
    o = _Outs(1)
    for mode in (0, 1):
        o.count[0] = COUNT
        assert L.hnswgpu_graph_components(e.handle, 5, 0, mode, None, None, None, _p(o.count)) == N.OK and o.count[0] == 0
        o.count[0] = COUNT
        assert L.hnswgpu_graph_components_device(e.handle, 5, 32, mode, None, None, None, _p(o.count), None) == N.OK and o.count[0] == 0
    assert (o.label == LABEL).all() and (o.sizes == SIZE).all()
    assert L.hnswgpu_graph_components(e.handle, 0, 0, 0, None, None, None, _p(o.count)) == N.ERR_ARG           # still refused
    assert e.knn_graph_components(5).n_components == 0


def test_without_a_device_a_well_formed_call_reports_no_device(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    offs, cols = np.array([0, 1, 2, 2], np.uint64), np.array([1, 2], np.uint32)
    if L.hnswgpu_device_count() > 0:                           # a box with a GPU answers (tests/test_gpu_graph_components.py checks the answers)
        assert h.knn_graph_components(3).labels[0] == 0
        assert native.csr_components(offs, cols).labels.tolist() == [0, 0, 0]
        return
    with pytest.raises(native.HnswError) as e:
        h.knn_graph_components(3)
    assert e.value.code == N.ERR_DEVICE
    with pytest.raises(native.HnswError) as e:
        native.csr_components(offs, cols)
    assert e.value.code == N.ERR_DEVICE
    o = _Outs(50)
    rc = L.hnswgpu_graph_components_device(h.handle, 3, 0, 0, None, _p(o.label), _p(o.sizes), _p(o.count), None)
    assert rc == N.ERR_DEVICE and N.last_error() and o.untouched()
    rc = L.hnswgpu_csr_components_device(0, 3, _p(offs), _p(cols), None, None, _p(o.label), _p(o.sizes), _p(o.count), None)
    assert rc == N.ERR_DEVICE and N.last_error() and o.untouched()
