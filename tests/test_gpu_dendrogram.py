"""The dendrogram of a forest on the device (forest_dendrogram -> hnswgpu_forest_dendrogram / _device, Hnsw.knn_graph_dendrogram ->
hnswgpu_graph_dendrogram / _device, csrc/dendrogram.hip).

The expected answers never come from the code under test: `dendrogram` of tests/test_dendrogram_abi.py is the sequential union-find
over the same edges.  The answer is all integers and unique, so every comparison is exact: left, right, size, and the slots behind
the last edge that must stay as they were.  For the index entries the forest itself is knn_graph_spanning_forest's (checked against
its own model in tests/test_gpu_spanning_forest.py), byte for byte."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import uniform
from test_dendrogram_abi import A, B, COUNT, LEFT, RIGHT, SIZE, W, dendrogram, random_forest
from test_gpu_symmetric_graph import Index, _uniform_index, hub_data

pytestmark = pytest.mark.gpu
MODES = ("union", "mutual")
MODE_CODE = {"union": 0, "mutual": 1}
EFS = (None, 32)
PAD = 3                                                        # slots behind the last edge


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32).copy()).cuda()


def _host_of(t):
    return t.cpu().numpy().view(np.uint32)


# ----------------------------------------------------------------------------------------------------- the forest entries
def forest_host(native, n, a, b):
    """the host entry itself on out arrays at their sentinels: (rc, left, right, size)"""
    m = len(a)
    left, right, size = np.full(m + PAD, LEFT, np.uint32), np.full(m + PAD, RIGHT, np.uint32), np.full(m + PAD, SIZE, np.uint32)
    rc = native.lib().hnswgpu_forest_dendrogram(0, n, m, _p(a), _p(b), _p(left), _p(right), _p(size))
    return rc, left, right, size


def forest_device(native, n, a, b, stream=None):
    """the device entry on tensors at their sentinels: (rc, left, right, size)"""
    import torch
    m = len(a)
    d_a, d_b = _dev(a if m else np.zeros(1, np.uint32)), _dev(b if m else np.zeros(1, np.uint32))
    left, right, size = _dev(np.full(m + PAD, LEFT, np.uint32)), _dev(np.full(m + PAD, RIGHT, np.uint32)), _dev(np.full(m + PAD, SIZE, np.uint32))
    torch.cuda.synchronize()
    rc = native.lib().hnswgpu_forest_dendrogram_device(0, n, m, _ptr(d_a), _ptr(d_b), _ptr(left), _ptr(right), _ptr(size),
                                                       C.c_void_p(stream.cuda_stream) if stream is not None else None)
    assert np.array_equal(_host_of(d_a)[:m], a) and np.array_equal(_host_of(d_b)[:m], b), "the ends were written"
    return rc, _host_of(left), _host_of(right), _host_of(size)


def check_forest(native, n, edges, what=""):
    """host form (twice: the same bytes) and device form against the model; nothing written behind slot m - 1"""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    a, b = np.ascontiguousarray(edges[:, 0], np.uint32), np.ascontiguousarray(edges[:, 1], np.uint32)
    want = dendrogram(n, edges)
    assert want is not None, (what, "the model sees a cycle")
    m = len(a)
    first = None
    for form in ("host", "host again", "device"):
        rc, left, right, size = (forest_device if form == "device" else forest_host)(native, n, a, b)
        assert rc == 0, (what, form, native._native.last_error())
        for name, got, exp, sentinel in (("left", left, want[0], LEFT), ("right", right, want[1], RIGHT), ("size", size, want[2], SIZE)):
            bad = np.flatnonzero(got[:m] != exp)
            assert len(bad) == 0, (what, form, name, bad[:4], got[bad[:4]], exp[bad[:4]])
            assert (got[m:] == sentinel).all(), (what, form, name, "behind the last edge")
        if form == "host":
            first = left.tobytes() + right.tobytes() + size.tobytes()
        elif form == "host again":
            assert left.tobytes() + right.tobytes() + size.tobytes() == first, (what, "two calls differ")
    res = native.forest_dendrogram(n, a, b)
    assert res.n_edges == m and res.n_vertices == n and res.left.dtype == np.uint32 and res.sizes.dtype == np.uint32
    assert np.array_equal(res.left, want[0]) and np.array_equal(res.right, want[1]) and np.array_equal(res.sizes, want[2]), (what, "python")
    return want


def path(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], 1)


def test_tiny_forests(native):
    check_forest(native, 0, [], "nothing")
    check_forest(native, 5, [], "m = 0")
    left, right, size = check_forest(native, 2, [(1, 0)], "m = 1")
    assert (left.tolist(), right.tolist(), size.tolist()) == ([1], [0], [2])
    check_forest(native, 3, [(0, 1), (2, 1)], "m = 2, joined")
    check_forest(native, 4, [(0, 1), (2, 3)], "m = 2, apart")
    left, right, size = check_forest(native, 4, [(0, 1), (3, 2), (2, 1)], "m = 3")
    assert (left.tolist(), right.tolist(), size.tolist()) == ([0, 3, 5], [1, 2, 4], [2, 2, 4])
    check_forest(native, 9, [(8, 7), (7, 6), (6, 5)], "m = 3, a chain among isolated vertices")


@pytest.mark.parametrize("length", [63, 64, 65, 257])
def test_a_path_is_the_chain_dendrogram(native, length):
    """the edges in order: every merge takes the cluster before it, depth n - 1 -- what a pointer-jumping shortcut gets wrong.  Then
    reversed and permuted."""
    e = path(length)
    left, right, size = check_forest(native, length, e, f"path {length} in order")
    assert np.array_equal(size, np.arange(2, length + 1)) and np.array_equal(left[1:], length + np.arange(length - 2))
    check_forest(native, length, e[::-1], f"path {length} reversed")
    check_forest(native, length, e[::-1, ::-1], f"path {length} reversed, ends swapped")
    check_forest(native, length, e[np.random.default_rng(length).permutation(length - 1)], f"path {length} permuted")


@pytest.mark.parametrize("m", [1023, 1024, 1025])
def test_around_a_block_boundary(native, m):
    """2^10 edges less one, 2^10, one more: the last takes a level more.  A chain in order, and a random forest of exactly m edges"""
    check_forest(native, m + 1, path(m + 1), f"chain of {m}")
    rng = np.random.default_rng(m)
    e = random_forest(m + 40, rng, keep=1.0)[:m]
    check_forest(native, m + 40, e, f"random forest of {m}")


def _bit_reversed(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2)


def test_a_path_in_bit_reversed_order_is_the_balanced_tree(native):
    n = 4096
    e = path(n)
    order = np.argsort(np.array([_bit_reversed(i, 12) for i in range(n - 1)]), kind="stable")
    left, right, size = check_forest(native, n, e[order], "bit-reversed path")
    assert size[-1] == n
    check_forest(native, n, e, "path of 4096 in order")


def test_a_star_in_random_order(native):
    """70 000 leaves: every merge but the first takes the cluster before it, and every lower-half edge of a level meets at one root"""
    n = 70001
    rng = np.random.default_rng(7)
    for centre in (0, n - 1, 31337):
        leaves = np.setdiff1d(np.arange(n), [centre])[rng.permutation(n - 1)]
        e = np.stack([np.full(n - 1, centre), leaves], 1)
        e[::2] = e[::2, ::-1]                                   # the centre is a or b
        left, right, size = check_forest(native, n, e, f"star, centre {centre}")
        assert np.array_equal(size, np.arange(2, n + 1))


def test_several_components_and_isolated_vertices(native):
    rng = np.random.default_rng(21)
    x, y = path(2000), path(1500) + 2500                        # two paths apart, 500 vertices between them and 300 behind untouched
    e = np.concatenate([x, y[::-1]])
    left, right, size = check_forest(native, 4300, e[rng.permutation(len(e))], "two paths and isolated vertices")
    for n, keep in ((300, 0.3), (5000, 0.6), (5000, 0.97)):
        e = random_forest(n, rng, keep)
        assert 0 < len(e) < n - 1
        check_forest(native, n, e, f"random forest {n} keeping {keep}")
    t = np.arange(3000)                                         # 3000 paths of three, interleaved
    check_forest(native, 9000, np.concatenate([np.stack([t, t + 3000], 1), np.stack([t + 6000, t + 3000], 1)]), "paths of three")


def test_a_random_forest_in_random_order(native):
    n = 20000
    e = random_forest(n, np.random.default_rng(n), keep=1.0)
    assert len(e) == n - 1
    left, right, size = check_forest(native, n, e, "random tree of 20000")
    assert size[-1] == n
    res = native.forest_dendrogram(n, e[:, 0], e[:, 1])
    assert res.roots().tolist() == [2 * n - 2]
    spf = native.SpanningForestResult(e[:, 0].astype(np.uint32), e[:, 1].astype(np.uint32), np.arange(n - 1, dtype=np.float32), n - 1, n)
    via = spf.dendrogram()
    assert np.array_equal(via.left, left) and np.array_equal(via.right, right) and np.array_equal(via.sizes, size)
    assert np.array_equal(via.linkage()[:, 2], np.arange(n - 1))


def test_an_invalid_forest_is_an_argument_error_never_a_fault(native):
    NN = native._native
    # a cycle of 3000 that closes only with the last edge: the path 0 .. 2999 in random order, then 0 - 2999 (3001 vertices, so that
    # 3000 edges are not too many)
    ring_n = 3001
    ring = np.concatenate([path(3000)[np.random.default_rng(4).permutation(2999)], [[0, 2999]]])
    assert dendrogram(ring_n, ring) is None and dendrogram(ring_n, ring[:-1]) is not None
    bad = {"a triangle": (4, [(0, 1), (1, 2), (2, 0)], "cycle"),
           "a repeated pair": (4, [(0, 1), (2, 3), (1, 0)], "cycle"),
           "a repeated pair at once": (3, [(0, 1), (0, 1)], "cycle"),
           "a cycle that the last edge closes": (ring_n, ring, "cycle"),
           "a cycle in the middle": (ring_n, np.concatenate([ring[-500:], ring[:-500]]), "cycle"),
           "an end at n": (4, [(0, 1), (1, 4), (2, 3)], "not below n"),
           "an end far out": (4, [(0xFFFFFFFF, 1), (1, 2)], "not below n"),
           "a self-loop": (4, [(0, 1), (2, 2), (2, 3)], "itself")}
    for form in (forest_host, forest_device):
        for name, (n, e, word) in bad.items():
            e = np.asarray(e, np.int64)
            rc, left, right, size = form(native, n, e[:, 0].astype(np.uint32), e[:, 1].astype(np.uint32))
            assert rc == NN.ERR_ARG and word in NN.last_error(), (form.__name__, name, rc, NN.last_error())
            assert (left == LEFT).all() and (right == RIGHT).all() and (size == SIZE).all(), (form.__name__, name, "written")
        rc, left, right, size = form(native, 4, np.array([0, 3, 2], np.uint32), np.array([1, 2, 1], np.uint32))    # the well-formed one, after all that
        assert rc == NN.OK and left[:3].tolist() == [0, 3, 5] and right[:3].tolist() == [1, 2, 4] and size[:3].tolist() == [2, 2, 4]


def test_two_host_threads_call_at_once(native):
    jobs = {}
    for name, n in (("a", 20000), ("b", 3000)):
        e = random_forest(n, np.random.default_rng(n + 1), 0.9)
        jobs[name] = (n, e[:, 0].astype(np.uint32), e[:, 1].astype(np.uint32), dendrogram(n, e))
    out, errs = {}, []

    def run(name):
        try:
            out[name] = [native.forest_dendrogram(*jobs[name][:3]) for _ in range(3)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=(name,)) for name in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for name, (_, _, _, (left, right, size)) in jobs.items():
        for got in out[name]:
            assert np.array_equal(got.left, left) and np.array_equal(got.right, right) and np.array_equal(got.sizes, size), name


def test_forest_device_entry_on_a_stream(native):
    import torch
    n = 5000
    e = random_forest(n, np.random.default_rng(55), 0.9)
    a, b = e[:, 0].astype(np.uint32), e[:, 1].astype(np.uint32)
    want = dendrogram(n, e)
    m = len(a)
    rc, left, right, size = forest_device(native, n, a, b, torch.cuda.Stream())
    assert rc == 0, native._native.last_error()
    assert np.array_equal(left[:m], want[0]) and np.array_equal(right[:m], want[1]) and np.array_equal(size[:m], want[2])
    assert (left[m:] == LEFT).all() and (right[m:] == RIGHT).all() and (size[m:] == SIZE).all()


# ----------------------------------------------------------------------------------------------------- the index entries
def check_index(ix, k, ef, mode, core_k=0, what=""):
    """the forest is knn_graph_spanning_forest's, byte for byte; left, right and size are the model's on it"""
    what = f"{what} n {ix.n} k {k} ef {ef} {mode} core_k {core_k}"
    f = ix.h.knn_graph_spanning_forest(k, ef, mode, core_k)
    got = ix.h.knn_graph_dendrogram(k, ef, mode, core_k)
    assert got.n_edges == f.n_edges and got.n_vertices == ix.n, (what, got.n_edges, f.n_edges)
    assert got.a.tobytes() == f.a.tobytes() and got.b.tobytes() == f.b.tobytes() and got.weights.tobytes() == f.weights.tobytes(), (what, "the forest")
    want = dendrogram(ix.n, zip(f.a.tolist(), f.b.tolist()))
    assert want is not None, what
    assert got.left.dtype == np.uint32 and got.right.dtype == np.uint32 and got.sizes.dtype == np.uint32
    assert np.array_equal(got.left, want[0]) and np.array_equal(got.right, want[1]) and np.array_equal(got.sizes, want[2]), what
    return got


def check_all(ix, k, what="", efs=EFS, core_ks=(0,)):
    for ef in efs:
        for mode in MODES:
            for core_k in sorted({min(c, k) for c in core_ks}):
                check_index(ix, k, ef, mode, core_k, what)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_small_indexes(native, oracle, tmp_path, n):
    ix = Index(native, oracle, tmp_path, uniform(n, 8, 10 + n))
    for k in (1, 3):
        check_all(ix, k, "small", core_ks=(0, 3))
    got = ix.h.knn_graph_dendrogram(3)
    assert got.n_edges == n - 1 and (n == 1 or got.sizes[-1] == n)                # k >= n - 1: the complete graph, one tree
    # the host entry itself: the slots behind the count stay as they were
    s = n + 2
    a, b, w, c = np.full(s, A, np.uint32), np.full(s, B, np.uint32), np.full(s, W, np.uint32), np.full(1, COUNT, np.uint64)
    left, right, size = np.full(s, LEFT, np.uint32), np.full(s, RIGHT, np.uint32), np.full(s, SIZE, np.uint32)
    assert native.lib().hnswgpu_graph_dendrogram(ix.h.handle, 1, 0, 1, 0, _p(a), _p(b), _p(w), _p(left), _p(right), _p(size), _p(c)) == 0
    f = ix.h.knn_graph_spanning_forest(1, None, "mutual")
    m = int(c[0])
    assert m == f.n_edges and np.array_equal(a[:m], f.a) and np.array_equal(b[:m], f.b) and np.array_equal(w[:m], f.weights.view(np.uint32))
    want = dendrogram(n, zip(f.a.tolist(), f.b.tolist()))
    assert np.array_equal(left[:m], want[0]) and np.array_equal(right[:m], want[1]) and np.array_equal(size[:m], want[2])
    assert (a[m:] == A).all() and (b[m:] == B).all() and (w[m:] == W).all()
    assert (left[m:] == LEFT).all() and (right[m:] == RIGHT).all() and (size[m:] == SIZE).all()


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_wave_and_block_edges(native, oracle, tmp_path_factory, n):
    """k = 1 gives many components; one wavefront less one, one, one more; a block and a bit"""
    ix = _uniform_index(native, oracle, tmp_path_factory, n)
    for k in (1, 3):
        check_all(ix, k, "edges", core_ks=(0, 3))
    got = ix.h.knn_graph_dendrogram(1)
    assert got.n_edges < n - 1 and len(got.roots()) == n - got.n_edges


@pytest.mark.parametrize("k", [5, 16])
def test_many_blocks(native, oracle, tmp_path_factory, k):
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    check_all(ix, k, "3000", core_ks=(0, 3))
    got = ix.h.knn_graph_dendrogram(k)
    if got.n_edges == ix.n - 1:                                 # a connected forest: the last merge holds every point
        assert got.sizes[-1] == ix.n
    assert len(got.roots()) == ix.h.knn_graph_components(k).n_components


def test_a_connected_forest_ends_with_every_point(native, oracle, tmp_path_factory):
    ix = _uniform_index(native, oracle, tmp_path_factory, 257)
    got = ix.h.knn_graph_dendrogram(256)                        # the complete graph
    assert got.n_edges == 256 and got.sizes[-1] == 257 and got.roots().tolist() == [257 + 255]


def test_separated_clusters_give_forty_roots(native, oracle, tmp_path):
    """40 tight clusters of 50 points: as many roots as knn_graph_components counts components, each of 50 vertices"""
    ix = Index(native, oracle, tmp_path, hub_data()[:2000])
    got = check_index(ix, 5, None, "union", 0, "clusters")
    comps = ix.h.knn_graph_components(5)
    roots = got.roots()
    assert comps.n_components == 40 and len(roots) == comps.n_components
    assert (roots >= ix.n).all() and (got.sizes[roots - ix.n] == 50).all()
    for mode in MODES:
        for ef in EFS:
            d = check_index(ix, 5, ef, mode, 2, "clusters")
            assert len(d.roots()) == ix.h.knn_graph_components(5, ef, mode).n_components


def test_index_device_entry_on_a_stream(native, oracle, tmp_path_factory, tmp_path):
    import torch
    NN = native._native
    L = native.lib()
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    stream = torch.cuda.Stream()
    s = ix.n - 1
    for ef in EFS:
        for mode in MODES:
            f = ix.h.knn_graph_spanning_forest(5, ef, mode, 3)
            want = dendrogram(ix.n, zip(f.a.tolist(), f.b.tolist()))
            sent = (A, B, W, LEFT, RIGHT, SIZE)
            t = [_dev(np.full(s, x, np.uint32)) for x in sent]
            torch.cuda.synchronize()
            count = np.full(1, COUNT, np.uint64)
            rc = L.hnswgpu_graph_dendrogram_device(ix.h.handle, 5, 0 if ef is None else ef, MODE_CODE[mode], 3, *[_ptr(x) for x in t], _p(count),
                                                   C.c_void_p(stream.cuda_stream))
            assert rc == NN.OK, NN.last_error()
            c = int(count[0])
            got = [_host_of(x) for x in t]
            assert c == f.n_edges
            for g, exp, x in zip(got, (f.a, f.b, f.weights.view(np.uint32), *want), sent):
                assert np.array_equal(g[:c], exp) and (g[c:] == x).all(), (ef, mode)
    cold = Index(native, oracle, tmp_path, uniform(65, 8, 65), upload=False)               # never uploaded
    t = [torch.full((64,), -1, dtype=torch.int32, device="cuda") for _ in range(6)]
    count = np.full(1, COUNT, np.uint64)
    rc = L.hnswgpu_graph_dendrogram_device(cold.h.handle, 3, 0, 0, 0, *[_ptr(x) for x in t], _p(count), None)
    assert rc == NN.ERR_DEVICE and "upload" in NN.last_error()
    assert count[0] == COUNT and all(bool((x == -1).all()) for x in t)


def test_the_same_call_gives_the_same_bytes(native, oracle, tmp_path_factory, knob):
    """twice in a row; and with D arriving in many chunks (HNSWGPU_GRAPH_CHUNK = 97: 31 chunks, the last partial)"""
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)

    def all_of(ef, mode):
        got = ix.h.knn_graph_dendrogram(16, ef, mode, 3)
        return b"".join(x.tobytes() for x in (got.a, got.b, got.weights, got.left, got.right, got.sizes))
    for mode in MODES:
        first = {ef: all_of(ef, mode) for ef in EFS}
        for ef in EFS:
            assert all_of(ef, mode) == first[ef]
        knob("HNSWGPU_GRAPH_CHUNK", 97)
        try:
            for ef in EFS:
                assert all_of(ef, mode) == first[ef], (mode, ef, "chunks of 97")
        finally:
            knob("HNSWGPU_GRAPH_CHUNK", None)


def test_scipy_accepts_the_linkage_and_cuts_it_as_labels_at_does(native, oracle, tmp_path_factory):
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    ix = _uniform_index(native, oracle, tmp_path_factory, 257)
    got = ix.h.knn_graph_dendrogram(256)                        # connected: scipy's linkage has n - 1 rows
    z = got.linkage()
    assert hierarchy.is_valid_linkage(z)
    w = np.unique(got.weights)
    for i in (len(w) // 4, len(w) // 2, len(w) - 2):
        cut = (float(w[i]) + float(w[i + 1])) / 2                # strictly between two distinct weights
        assert float(w[i]) < cut < float(w[i + 1])
        mine = ix.h.knn_graph_spanning_forest(256).labels_at(cut).labels
        theirs = hierarchy.fcluster(z, cut, "distance")
        pairs = set(zip(mine.tolist(), theirs.tolist()))        # the same partition: a bijection between the two labellings
        assert len(pairs) == len(set(mine.tolist())) == len(set(theirs.tolist()))
