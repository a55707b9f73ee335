"""The dendrogram entries (hnswgpu_forest_dendrogram / _device, hnswgpu_graph_dendrogram / _device, csrc/dendrogram.hip) as far as a
box without a GPU can see them: the ABI, every refusal that is answered before a device is needed, the calls that need none -- and
the contract restated in Python: `dendrogram`, the sequential union-find that keeps per root the last edge and the size.
tests/test_gpu_dendrogram.py imports it to build its expected answers, never from the code under test.  Here the model is checked
on a hand-made forest and against SpanningForestResult.labels_at.  CPU only."""
import ctypes as C

import numpy as np
import pytest

ENTRIES = ("hnswgpu_forest_dendrogram", "hnswgpu_forest_dendrogram_device", "hnswgpu_graph_dendrogram", "hnswgpu_graph_dendrogram_device")
LEFT, RIGHT, SIZE = 0xC3C3C3C3, 0x3C3C3C3C, 0x99999999
A, B, W, COUNT = 0xA5A5A5A5, 0x5A5A5A5A, 0x7FC01234, 0x7777


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ----------------------------------------------------------------------------------------------------- the model
def dendrogram(n, edges):
    """(left u32[m], right u32[m], size u32[m]) of the edges (a, b) over 0 .. n - 1 read in their order, or None when an edge joins
    two vertices that earlier edges join already: the sequential union-find, each root keeping the last edge of its tree (its cluster
    is n + that edge; none: the vertex itself) and the tree's size."""
    parent, last, size = list(range(n)), [None] * n, [1] * n

    def find(v):
        while parent[v] != v:
            parent[v] = parent[parent[v]]
            v = parent[v]
        return v
    left, right, sizes = [], [], []
    for e, (x, y) in enumerate(edges):
        x, y = int(x), int(y)
        rx, ry = find(x), find(y)
        if rx == ry:
            return None
        left.append(x if last[rx] is None else n + last[rx])
        right.append(y if last[ry] is None else n + last[ry])
        lo, hi = min(rx, ry), max(rx, ry)
        parent[hi] = lo
        size[lo] += size[hi]
        last[lo] = e
        sizes.append(size[lo])
    return np.array(left, np.uint32), np.array(right, np.uint32), np.array(sizes, np.uint32)


def leaves_under(n, left, right, cluster):
    """the vertices of a cluster id, by walking the table down"""
    out, stack = [], [int(cluster)]
    while stack:
        c = stack.pop()
        if c < n:
            out.append(c)
        else:
            stack += [int(left[c - n]), int(right[c - n])]
    return sorted(out)


def random_forest(n, rng, keep=0.85):
    """the edges of a random forest on 0 .. n - 1 under a random numbering, in random order, as an (m, 2) array"""
    v = rng.permutation(n)
    e = [(v[i], v[rng.integers(0, i)]) for i in range(1, n) if rng.random() < keep]
    e = np.array(e, np.int64).reshape(-1, 2)
    return e[rng.permutation(len(e))]


def test_model_on_a_hand_made_forest():
    """8 vertices: 0 - 1, 2 - 3, then 1 - 2 joins the two pairs, 5 - 6 apart, 4 to the four, 7 alone"""
    edges = [(0, 1), (3, 2), (1, 2), (6, 5), (4, 0)]
    left, right, size = dendrogram(8, edges)
    assert left.tolist() == [0, 3, 8, 6, 4]
    assert right.tolist() == [1, 2, 9, 5, 10]
    assert size.tolist() == [2, 2, 4, 2, 5]
    assert leaves_under(8, left, right, 12) == [0, 1, 2, 3, 4] and leaves_under(8, left, right, 11) == [5, 6] and leaves_under(8, left, right, 7) == [7]
    # a chain read from one end: every merge takes the cluster before it
    left, right, size = dendrogram(5, [(0, 1), (1, 2), (2, 3), (3, 4)])
    assert left.tolist() == [0, 5, 6, 7] and right.tolist() == [1, 2, 3, 4] and size.tolist() == [2, 3, 4, 5]
    # the same chain read from the middle outwards
    left, right, size = dendrogram(5, [(2, 1), (2, 3), (0, 1), (4, 3)])
    assert left.tolist() == [2, 5, 0, 4] and right.tolist() == [1, 3, 6, 7] and size.tolist() == [2, 3, 4, 5]
    assert [len(x) for x in dendrogram(3, [])] == [0, 0, 0]
    assert dendrogram(3, [(0, 1), (1, 2), (2, 0)]) is None and dendrogram(3, [(0, 1), (1, 0)]) is None


def test_model_agrees_with_labels_at(native):
    """for a random forest and a few prefixes e: the leaves under cluster n + e are exactly the component of a[e] under the first
    e + 1 edges, as SpanningForestResult.labels_at labels them"""
    rng = np.random.default_rng(11)
    n = 200
    e = random_forest(n, rng)
    m = len(e)
    a, b = e[:, 0].astype(np.uint32), e[:, 1].astype(np.uint32)
    left, right, size = dendrogram(n, e)
    w = np.arange(m, dtype=np.float32)                          # the height of merge e is e: a cut at e keeps the first e + 1 edges
    forest = native.SpanningForestResult(a, b, w, m, n)
    for edge in (0, 1, 2, m // 3, m // 2, m - 2, m - 1):
        labels = forest.labels_at(float(edge)).labels
        want = np.flatnonzero(labels == labels[a[edge]]).tolist()
        assert leaves_under(n, left, right, n + edge) == want, edge
        assert size[edge] == len(want)
    # and the result class: roots are the clusters that are nobody's child, one per component
    res = native.DendrogramResult(left, right, size, m, n, a, b, w)
    assert len(res.roots()) == forest.labels_at().n_components
    z = res.linkage()
    assert z.shape == (m, 4) and z.dtype == np.float64 and np.array_equal(z[:, 0], left) and np.array_equal(z[:, 3], size) and np.array_equal(z[:, 2], w)
    with pytest.raises(native.HnswError):
        native.DendrogramResult(left, right, size, m, n).linkage()


# ----------------------------------------------------------------------------------------------------- the ABI
def _small(native, n=50, d=8):
    X = np.random.default_rng(1).random((n, d), dtype=np.float32)
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
    assert protos[ENTRIES[0]][2] == ["device", "n", "m", "a", "b", "out_left", "out_right", "out_size"]
    assert protos[ENTRIES[1]][2] == ["device", "n", "m", "d_a", "d_b", "d_out_left", "d_out_right", "d_out_size", "stream"]
    assert protos[ENTRIES[2]][2] == ["idx", "k", "ef", "mode", "core_k", "out_a", "out_b", "out_w", "out_left", "out_right", "out_size", "out_n_edges"]
    assert protos[ENTRIES[3]][2] == ["idx", "k", "ef", "mode", "core_k", "d_out_a", "d_out_b", "d_out_w", "d_out_left", "d_out_right", "d_out_size",
                                     "out_n_edges", "stream"]
    assert protos[ENTRIES[0]][1][0] is C.c_int and protos[ENTRIES[0]][1][1] is C.c_uint64 and protos[ENTRIES[2]][1][3] is C.c_uint32
    text = open(N.HEADER_PATH).read()
    doc = text[text.index("dendrogram of a forest ---"):text.index("int hnswgpu_graph_dendrogram_device")]
    for word in ("merge order", "scipy", "n + i", "2^31 - 1", "n - 1", "cycle", "ceil(log2 m)", "ONE word", "16 (n + m) + 8 m", "Out of scope",
                 "condensed tree", "not a forest", "reordering", "byte for byte", "several host threads"):
        assert word in doc, word
    assert len(N.SYMBOLS) == 102
    assert hasattr(native.Hnsw, "knn_graph_dendrogram") and callable(native.forest_dendrogram) and hasattr(native.SpanningForestResult, "dendrogram")


class _Outs:
    """out arrays at their sentinels"""

    def __init__(self, slots):
        self.left, self.right, self.size = np.full(slots, LEFT, np.uint32), np.full(slots, RIGHT, np.uint32), np.full(slots, SIZE, np.uint32)
        self.a, self.b, self.w = np.full(slots, A, np.uint32), np.full(slots, B, np.uint32), np.full(slots, W, np.uint32).view(np.float32)
        self.count = np.full(1, COUNT, np.uint64)

    def untouched(self):
        return bool((self.left == LEFT).all() and (self.right == RIGHT).all() and (self.size == SIZE).all() and (self.a == A).all()
                    and (self.b == B).all() and (self.w.view(np.uint32) == W).all() and self.count[0] == COUNT)


def test_forest_entries_answer_every_refusal_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    ea, eb = np.array([0, 1, 2], np.uint32), np.array([1, 2, 3], np.uint32)
    o = _Outs(4)

    def host(n=4, m=3, a=ea, b=eb, left=o.left, right=o.right, size=o.size):
        return L.hnswgpu_forest_dendrogram(0, n, m, _p(a), _p(b), _p(left), _p(right), _p(size))

    def dev(n=4, m=3, a=ea, b=eb, left=o.left, right=o.right, size=o.size):
        return L.hnswgpu_forest_dendrogram_device(0, n, m, _p(a), _p(b), _p(left), _p(right), _p(size), None)

    def refused(call, word, **kw):
        rc = call(**kw)
        assert rc == N.ERR_ARG, (kw.keys(), rc, N.last_error())
        assert word in N.last_error(), (word, N.last_error())
        assert o.untouched(), kw.keys()
    for call in (host, dev):                                   # what either form sees without reading an array
        refused(call, "2^31", n=1 << 31, m=1)
        refused(call, "2^31", n=(1 << 63) + 5, m=0)
        refused(call, "at most n - 1", m=4)
        refused(call, "at most n - 1", n=3)
        refused(call, "at most n - 1", n=1, m=1)
        refused(call, "at most n - 1", n=0, m=1)
        refused(call, "at most n - 1", m=1 << 40)
        refused(call, "null a or b", a=None)
        refused(call, "null a or b", b=None)
        for name in ("left", "right", "size"):
            refused(call, "out_left, out_right or out_size", **{name: None})
        refused(call, "2^31", n=1 << 31, m=1 << 31, a=None)    # two faults at once: n first, then m, then the pointers
        refused(call, "at most n - 1", m=4, a=None)
    # the ends: the host form reads its arrays on the host (the device form's kernel needs a device: tests/test_gpu_dendrogram.py)
    refused(host, "not below n", a=np.array([0, 4, 2], np.uint32))
    refused(host, "not below n", b=np.array([1, 2, 0xFFFFFFFF], np.uint32))
    refused(host, "itself", a=np.array([0, 2, 2], np.uint32))
    refused(host, "edge 0", a=np.array([9, 2, 2], np.uint32))  # two faults at once: the first edge that has one
    # a cycle is the device's to find: without one the call says so, with one it is refused like the rest
    rc = host(a=np.array([0, 1, 0], np.uint32), b=np.array([1, 2, 2], np.uint32))
    assert rc == (N.ERR_ARG if L.hnswgpu_device_count() > 0 else N.ERR_DEVICE), (rc, N.last_error())
    assert o.untouched()
    for bad in (dict(n=3, a=[0, 1, 2], b=[1, 2, 0]), dict(n=3, a=[0], b=[3]), dict(n=3, a=[1], b=[1]), dict(n=3, a=[0, 1], b=[1])):
        with pytest.raises(native.HnswError) as err:           # the Python function hands the refusals on
            native.forest_dendrogram(**bad)
        assert err.value.code == N.ERR_ARG


def test_no_edge_needs_no_device(native):
    N = _N()
    L = native.lib()
    o = _Outs(4)
    for n in (0, 1, 2, 1000, (1 << 31) - 1):
        assert L.hnswgpu_forest_dendrogram(0, n, 0, None, None, None, None, None) == N.OK
        assert L.hnswgpu_forest_dendrogram_device(0, n, 0, None, None, None, None, None, None) == N.OK
        assert L.hnswgpu_forest_dendrogram(0, n, 0, _p(o.a), _p(o.b), _p(o.left), _p(o.right), _p(o.size)) == N.OK and o.untouched()
    for n in (0, 1, 5):
        got = native.forest_dendrogram(n, [], [])
        assert got.n_edges == 0 and len(got.left) == 0 and got.left.dtype == np.uint32 and got.roots().tolist() == list(range(n))
        assert got.a is None and got.weights is None
    got = native.SpanningForestResult(np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32), 0, 3).dendrogram()
    assert got.n_edges == 0 and got.linkage().shape == (0, 4) and got.roots().tolist() == [0, 1, 2]


def test_index_entries_answer_every_refusal_before_a_device_is_needed(native):
    """the forest call's refusals with the forest call's words, then the three new arrays"""
    N = _N()
    L = native.lib()
    X, h = _small(native)
    o = _Outs(49)

    def host(idx=h.handle, k=3, ef=0, mode=0, core_k=0, a=o.a, b=o.b, w=o.w, left=o.left, right=o.right, size=o.size, count=o.count):
        return L.hnswgpu_graph_dendrogram(idx, k, ef, mode, core_k, _p(a), _p(b), _p(w), _p(left), _p(right), _p(size), _p(count))

    def dev(idx=h.handle, k=3, ef=0, mode=0, core_k=0, a=o.a, b=o.b, w=o.w, left=o.left, right=o.right, size=o.size, count=o.count):
        return L.hnswgpu_graph_dendrogram_device(idx, k, ef, mode, core_k, _p(a), _p(b), _p(w), _p(left), _p(right), _p(size), _p(count), None)

    def forest(idx=h.handle, k=3, ef=0, mode=0, core_k=0, a=o.a, b=o.b, w=o.w, count=o.count, **_):
        return L.hnswgpu_graph_spanning_forest(idx, k, ef, mode, core_k, _p(a), _p(b), _p(w), _p(count))
    big = (1 << 30) // 50 + 1
    for call in (host, dev):
        for kw in (dict(idx=None), dict(count=None), dict(a=None), dict(b=None), dict(w=None), dict(k=0), dict(mode=2), dict(k=big), dict(k=1 << 40),
                   dict(core_k=4), dict(core_k=1 << 63), dict(k=4097), dict(k=0, ef=32), dict(mode=7, ef=32), dict(core_k=4, ef=32),
                   dict(k=0, left=None), dict(count=None, size=None)):
            assert forest(**kw) == N.ERR_ARG
            words = N.last_error()
            rc = call(**kw)
            assert rc == N.ERR_ARG and N.last_error() == words, (kw.keys(), rc, N.last_error(), words)
            assert o.untouched(), kw.keys()
        for name in ("left", "right", "size"):
            rc = call(**{name: None})
            assert rc == N.ERR_ARG and "out_left, out_right or out_size" in N.last_error(), (name, rc, N.last_error())
            assert o.untouched()
    for bad in (dict(knbn=0), dict(knbn=3, mode="both"), dict(knbn=3, ef=0), dict(knbn=3, core_k=4), dict(knbn=3, core_k=-1)):
        with pytest.raises(native.HnswError) as err:           # the Python method hands the refusals on
            h.knn_graph_dendrogram(**bad)
        assert err.value.code == N.ERR_ARG


def test_empty_and_one_point_indexes_have_no_merge_and_need_no_device(native):
    N = _N()
    L = native.lib()
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    for mode in ("union", "mutual"):
        for ef in (None, 16):
            res = e.knn_graph_dendrogram(5, ef, mode, 2)
            assert res.n_edges == 0 and len(res.left) == 0 and len(res.right) == 0 and len(res.sizes) == 0 and len(res.a) == 0
            assert res.left.dtype == np.uint32 and res.sizes.dtype == np.uint32 and res.weights.dtype == np.float32
            assert res.roots().tolist() == [] and res.linkage().shape == (0, 4)
    e.parallel_insert(np.zeros((0, 8), np.float32))            # (a handle exists from the first insertion on)
    one = native.Hnsw(8, 10, 16, 32, "DistL2")
    one.parallel_insert(np.ones((1, 8), np.float32))
    o = _Outs(1)
    for h in (e, one):
        for mode in (0, 1):
            o.count[0] = COUNT
            assert L.hnswgpu_graph_dendrogram(h.handle, 5, 0, mode, 0, None, None, None, None, None, None, _p(o.count)) == N.OK and o.count[0] == 0
            o.count[0] = COUNT
            rc = L.hnswgpu_graph_dendrogram_device(h.handle, 5, 32, mode, 5, _p(o.a), _p(o.b), _p(o.w), _p(o.left), _p(o.right), _p(o.size), _p(o.count), None)
            assert rc == N.OK and o.count[0] == 0
        o.count[0] = COUNT
        assert o.untouched()
        assert L.hnswgpu_graph_dendrogram(h.handle, 0, 0, 0, 0, None, None, None, None, None, None, _p(o.count)) == N.ERR_ARG     # still refused
        assert L.hnswgpu_graph_dendrogram(h.handle, 5, 0, 0, 6, None, None, None, None, None, None, _p(o.count)) == N.ERR_ARG
        assert o.untouched()
    got = one.knn_graph_dendrogram(5)
    assert got.n_edges == 0 and got.n_vertices == 1 and got.roots().tolist() == [0]


def test_without_a_device_a_well_formed_call_reports_no_device(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    ea, eb = np.array([0, 3, 1], np.uint32), np.array([1, 2, 2], np.uint32)
    if L.hnswgpu_device_count() > 0:                           # a box with a GPU answers (tests/test_gpu_dendrogram.py checks the answers)
        got = native.forest_dendrogram(4, ea, eb)
        assert got.left.tolist() == [0, 3, 4] and got.right.tolist() == [1, 2, 5] and got.sizes.tolist() == [2, 2, 4]
        got = h.knn_graph_dendrogram(3)
        assert 25 <= got.n_edges <= 49 and got.sizes.max() <= 50
        return
    with pytest.raises(native.HnswError) as e:
        native.forest_dendrogram(4, ea, eb)
    assert e.value.code == N.ERR_DEVICE
    with pytest.raises(native.HnswError) as e:
        h.knn_graph_dendrogram(3)
    assert e.value.code == N.ERR_DEVICE
    o = _Outs(49)
    rc = L.hnswgpu_forest_dendrogram_device(0, 4, 3, _p(ea), _p(eb), _p(o.left), _p(o.right), _p(o.size), None)
    assert rc == N.ERR_DEVICE and N.last_error() and o.untouched()
    rc = L.hnswgpu_graph_dendrogram_device(h.handle, 3, 0, 0, 0, _p(o.a), _p(o.b), _p(o.w), _p(o.left), _p(o.right), _p(o.size), _p(o.count), None)
    assert rc == N.ERR_DEVICE and N.last_error() and o.untouched()
