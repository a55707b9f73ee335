"""The minimum spanning forest on the device (Hnsw.knn_graph_spanning_forest -> hnswgpu_graph_spanning_forest / _device,
csr_spanning_forest -> hnswgpu_csr_spanning_forest / _device, csrc/spanning_forest.hip).

The expected answers never come from the code under test.  For the CSR entries the model is `spanning_forest`
(tests/test_spanning_forest_abi.py), Kruskal on the same entries.  For the index entries D is what the existing public calls return
for every point (exact_knn_graph_flat / knn_graph_flat), `pair_weights` applies the min / max / core rule and `spanning_forest` takes
the forest.  Under the strict total order (weight, lo, hi) the forest is unique, so every comparison is exact: the ends, the bits of
the weights, the count, and the slots behind the count that must stay as they were.  The cross-check ties the forest to the
components of tests/test_gpu_graph_components.py: at every cut the forest's components are knn_graph_components's."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import uniform
from test_gpu_graph_components import to_csr
from test_gpu_symmetric_graph import Index, _uniform_index, hub_data, positive
from test_spanning_forest_abi import pair_weights, spanning_forest

pytestmark = pytest.mark.gpu
MODES = ("union", "mutual")
MODE_CODE = {"union": 0, "mutual": 1}
EFS = (None, 32)
A, B, W, COUNT = 0xA5A5A5A5, 0x5A5A5A5A, 0x7FC01234, 0x7777


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _bits(w):
    return np.ascontiguousarray(w, np.float32).view(np.uint32)


# ----------------------------------------------------------------------------------------------------- the CSR entries
def csr_triples(offsets, cols, dists=None):
    """the (row, col, weight) entries of a CSR in entry order; no dists: every weight +0"""
    offsets = np.asarray(offsets, np.int64)
    rows = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))
    w = np.zeros(len(rows), np.float32) if dists is None else np.asarray(dists, np.float32)[:len(rows)]
    return list(zip(rows.tolist(), np.asarray(cols, np.int64)[:len(rows)].tolist(), w))


def csr_host(native, n, offsets, cols, dists=None):
    """the host entry itself on out arrays at their sentinels: (rc, a, b, w bits, count)"""
    m = max(n - 1, 1)
    a, b, w, c = np.full(m, A, np.uint32), np.full(m, B, np.uint32), np.full(m, W, np.uint32), np.full(1, COUNT, np.uint64)
    rc = native.lib().hnswgpu_csr_spanning_forest(0, n, _p(offsets), _p(cols), _p(dists), _p(a), _p(b), _p(w), _p(c))
    return rc, a, b, w, int(c[0])


def csr_device(native, n, offsets, cols, dists=None, stream=None):
    """the device entry on tensors at their sentinels: (rc, a, b, w bits, count)"""
    import torch
    m = max(n - 1, 1)
    d_offs = torch.from_numpy(offsets.view(np.int64).copy()).cuda()
    d_cols = torch.from_numpy(cols.view(np.int32).copy() if len(cols) else np.zeros(1, np.int32)).cuda()
    d_dists = torch.from_numpy(np.ascontiguousarray(dists, np.float32)).cuda() if dists is not None and len(dists) else None
    a = torch.from_numpy(np.full(m, A, np.uint32).view(np.int32)).cuda()
    b = torch.from_numpy(np.full(m, B, np.uint32).view(np.int32)).cuda()
    w = torch.from_numpy(np.full(m, W, np.uint32).view(np.int32)).cuda()
    torch.cuda.synchronize()
    c = np.full(1, COUNT, np.uint64)
    rc = native.lib().hnswgpu_csr_spanning_forest_device(0, n, _ptr(d_offs), _ptr(d_cols), _ptr(d_dists), _ptr(a), _ptr(b), _ptr(w), _p(c),
                                                         C.c_void_p(stream.cuda_stream) if stream is not None else None)
    return rc, a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32), w.cpu().numpy().view(np.uint32), int(c[0])


def check_csr(native, n, offsets, cols, dists=None, what=""):
    """host form (twice: the same bytes) and device form against the model; nothing written behind the count"""
    wa, wb, ww = spanning_forest(n, csr_triples(offsets, cols, dists))
    m = len(wa)
    first = None
    for form in ("host", "host again", "device"):
        rc, a, b, w, got_m = (csr_device if form == "device" else csr_host)(native, n, offsets, cols, dists)
        assert rc == 0, (what, form, native._native.last_error())
        assert got_m == m, (what, form, got_m, m)
        assert np.array_equal(a[:m], wa) and np.array_equal(b[:m], wb), (what, form, "ends", np.flatnonzero((a[:m] != wa) | (b[:m] != wb))[:4])
        assert np.array_equal(w[:m], _bits(ww)), (what, form, "weight bits", np.flatnonzero(w[:m] != _bits(ww))[:4])
        assert (a[m:] == A).all() and (b[m:] == B).all() and (w[m:] == W).all(), (what, form, "behind the count")
        if form == "host":
            first = a.tobytes() + b.tobytes() + w.tobytes()
        elif form == "host again":
            assert a.tobytes() + b.tobytes() + w.tobytes() == first, (what, "two calls differ")
    res = native.csr_spanning_forest(offsets, cols, dists)
    assert res.n_edges == m and np.array_equal(res.a, wa) and np.array_equal(res.b, wb) and np.array_equal(_bits(res.weights), _bits(ww)), (what, "python")
    assert res.a.dtype == np.uint32 and res.b.dtype == np.uint32 and res.weights.dtype == np.float32
    return wa, wb, ww


def test_tiny_graphs(native):
    none = np.zeros(0, np.uint32)
    check_csr(native, 1, np.array([0, 0], np.uint64), none, what="one vertex")
    check_csr(native, 1, np.array([0, 1], np.uint64), np.array([0], np.uint32), what="one vertex, a self-loop")
    a, b, w = check_csr(native, 2, np.array([0, 0, 0], np.uint64), none, what="two apart")
    assert len(a) == 0
    a, b, w = check_csr(native, 2, np.array([0, 1, 2], np.uint64), np.array([0, 1], np.uint32), what="two apart, self-loops")
    assert len(a) == 0
    for offs, col in (([0, 1, 1], 1), ([0, 0, 1], 0)):          # the one edge named from either end
        a, b, w = check_csr(native, 2, np.array(offs, np.uint64), np.array([col], np.uint32), np.array([2.5], np.float32), what="two joined")
        assert (a.tolist(), b.tolist(), w.tolist()) == ([0], [1], [2.5])


def _numberings(n, seed):
    return {"in order": np.arange(n), "reversed": np.arange(n)[::-1].copy(), "permuted": np.random.default_rng(seed).permutation(n)}


@pytest.mark.parametrize("length", [63, 64, 65, 257])
def test_a_path_named_from_one_end_only(native, length):
    """a deep chain under three numberings, random weights from a few values (ties by (lo, hi)); every edge is in the forest"""
    for name, v in _numberings(length, length).items():
        offsets, cols, order = to_csr(length, np.stack([v[:-1], v[1:]], 1))
        d = (np.random.default_rng(length + 1).integers(0, 5, length - 1).astype(np.float32) / 4)[order]
        a, b, w = check_csr(native, length, offsets, cols, d, what=f"path {length} {name}")
        assert len(a) == length - 1


def _bit_reversed(i, bits):
    return int(format(i, f"0{bits}b")[::-1], 2)


def test_a_path_that_halves_once_per_round(native):
    """4096 vertices in a path, edge i weighing the bit reversal of i: the pattern under which Boruvka's components only halve per
    round, so the rounds come as close to the bound ceil(log2 n) + 1 = 13 as a path lets them.  Then the same path with all weights
    equal: the ties are broken by (lo, hi), and the answer is the path in order."""
    n = 4096
    e = np.stack([np.arange(n - 1), np.arange(1, n)], 1)
    offsets, cols, order = to_csr(n, e)
    d = np.array([_bit_reversed(i, 12) for i in range(n - 1)], np.float32)[order]
    a, b, w = check_csr(native, n, offsets, cols, d, what="bit-reversed path")
    assert len(a) == n - 1 and np.array_equal(np.sort(w), np.sort(d))
    for dists in (np.full(n - 1, 0.5, np.float32), None):
        a, b, w = check_csr(native, n, offsets, cols, dists, what="equal path")
        assert np.array_equal(a, np.arange(n - 1)) and np.array_equal(b, np.arange(1, n))
    v = np.random.default_rng(4096).permutation(n)              # and under a random numbering, named from the larger end
    offsets, cols, order = to_csr(n, np.stack([v[1:], v[:-1]], 1))
    check_csr(native, n, offsets, cols, np.full(n - 1, 0.5, np.float32), what="equal path, permuted")


def test_a_grid_with_equal_weights_under_a_random_numbering(native):
    v = np.random.default_rng(64).permutation(64 * 64).reshape(64, 64)
    e = np.concatenate([np.stack([v[:, :-1].ravel(), v[:, 1:].ravel()], 1), np.stack([v[1:, :].ravel(), v[:-1, :].ravel()], 1)])
    offsets, cols, _ = to_csr(4096, e)
    a, b, w = check_csr(native, 4096, offsets, cols, np.ones(len(e), np.float32), what="grid")
    assert len(a) == 4095


def test_a_complete_graph_with_few_distinct_weights(native):
    n = 40
    rng = np.random.default_rng(40)
    e = np.array([(i, j) for i in range(n) for j in range(n) if i != j])
    offsets, cols, order = to_csr(n, e)
    d = (rng.integers(0, 8, len(e)).astype(np.float32) / 8)[order]          # the two directions of a pair differ: the min counts
    a, b, w = check_csr(native, n, offsets, cols, d, what="K40")
    assert len(a) == n - 1


def test_a_star_is_a_hub_row(native):
    """70 000 leaves: the centre's row holds them all, or the leaves name the centre -- one round hooks them all"""
    n = 70001
    d = (np.random.default_rng(7).integers(0, 3, n - 1).astype(np.float32))
    for centre in (0, n - 1):
        leaves = np.setdiff1d(np.arange(n), [centre])
        for name, e in (("hub row", np.stack([np.full(n - 1, centre), leaves], 1)), ("named by the leaves", np.stack([leaves, np.full(n - 1, centre)], 1))):
            offsets, cols, order = to_csr(n, e)
            a, b, w = check_csr(native, n, offsets, cols, d[order], what=f"star, centre {centre}, {name}")
            assert len(a) == n - 1


def test_disjoint_triangles_interleaved(native):
    t = np.arange(3000)
    e = np.concatenate([np.stack([t, t + 3000], 1), np.stack([t + 3000, t + 6000], 1), np.stack([t + 6000, t], 1)])
    offsets, cols, order = to_csr(9000, e)
    d = np.concatenate([np.full(3000, 1.0), np.full(3000, 3.0), np.full(3000, 2.0)]).astype(np.float32)[order]
    a, b, w = check_csr(native, 9000, offsets, cols, d, what="triangles")
    assert len(a) == 6000 and np.array_equal(w, np.repeat(np.array([1.0, 2.0], np.float32), 3000))         # the heaviest side of each is left out
    a, b, w = check_csr(native, 9000, offsets, cols, None, what="triangles, equal weights")
    assert len(a) == 6000


def test_two_paths_apart(native):
    x, y = np.arange(2000), np.arange(2000, 4000)
    e = np.concatenate([np.stack([x[:-1], x[1:]], 1), np.stack([y[1:], y[:-1]], 1)])
    offsets, cols, order = to_csr(4000, e)
    d = np.random.default_rng(8).random(len(e), dtype=np.float32)[order]
    a, b, w = check_csr(native, 4000, offsets, cols, d, what="two paths")
    assert len(a) == 3998


@pytest.mark.parametrize("n,out", [(20000, 1), (3000, 2)])
def test_random_graphs(native, n, out):
    rng = np.random.default_rng(n)
    e = np.stack([np.repeat(np.arange(n), out), rng.integers(0, n, n * out)], 1)
    offsets, cols, order = to_csr(n, e)
    d = (rng.integers(0, 50, len(e)).astype(np.float32) / 8)[order]
    a, b, w = check_csr(native, n, offsets, cols, d, what=f"random {n} x {out}")
    assert 0 < len(a) < n


def test_self_loops_repeats_and_empty_rows(native):
    """a repeated pair has the min of its weights, whichever row names it; self-loops and empty rows change nothing"""
    n = 300
    rng = np.random.default_rng(5)
    e = np.stack([rng.integers(0, n // 3, 200) * 3, rng.integers(0, n, 200)], 1)          # rows 1, 2 mod 3 are empty
    e = np.concatenate([e, e[:50], e[:50, ::-1][e[:50, 1] % 3 == 0], np.stack([np.arange(0, n, 3)] * 2, 1), [[n - 1, n - 1]] * 3])
    offsets, cols, order = to_csr(n, e)
    d = rng.integers(0, 9, len(e)).astype(np.float32)[order]
    assert (np.diff(offsets.astype(np.int64)) == 0).sum() >= n // 2
    a, b, w = check_csr(native, n, offsets, cols, d, what="loops, repeats, empty rows")
    lightest = {}
    for r, c, x in csr_triples(offsets, cols, d):
        if r != c:
            lightest[(min(r, c), max(r, c))] = min(lightest.get((min(r, c), max(r, c)), np.inf), float(x))
    assert all(lightest[(int(x), int(y))] == float(z) for x, y, z in zip(a, b, w))          # min wins
    assert len(lightest) < len([1 for r, c, _ in csr_triples(offsets, cols, d) if r != c])   # (there are repeats)


def test_weights_are_ordered_as_the_exact_key_orders_distances(native):
    """NaN (two payloads), -0, +0, +inf, negatives: ordered by value, -0 = +0, every NaN equal and last; the stored bits come back"""
    n = 2000
    rng = np.random.default_rng(9)
    e = np.stack([rng.integers(0, n, 3000), rng.integers(0, n, 3000)], 1)
    offsets, cols, order = to_csr(n, e)
    d = rng.random(3000, dtype=np.float32) - np.float32(0.25)
    d[::7], d[1::7], d[2::7], d[3::7] = np.nan, -0.0, np.inf, 0.0
    d.view(np.uint32)[::14] = 0xFFC00001                        # a negative NaN with a payload
    d = d[order]
    a, b, w = check_csr(native, n, offsets, cols, d, what="hostile weights")
    got = _bits(w)
    assert (got == 0x80000000).any() and (got == 0).any() and (got == 0xFFC00001).any() and (got == 0x7FC00000).any() and np.isinf(w).any()
    nan = np.isnan(w)
    assert nan[int(np.argmax(nan)):].all() and (np.diff(_order(w).astype(np.int64)) >= 0).all()
    check_csr(native, n, offsets, cols, None, what="no dists")


def test_an_invalid_graph_is_an_argument_error_never_a_fault(native):
    NN = native._native
    offs, cols = np.array([0, 2, 3, 3, 5], np.uint64), np.array([1, 2, 3, 0, 1], np.uint32)
    bad = {"offsets[0]": (np.array([1, 2, 3, 3, 5], np.uint64), cols),
           "descend": (np.array([0, 3, 2, 3, 5], np.uint64), cols),
           "descend ": (np.array([0, 2, 3, 6, 5], np.uint64), np.array([1, 2, 3, 0, 1, 1], np.uint32)),
           "not below n": (offs, np.array([1, 2, 4, 0, 1], np.uint32)),
           "not below n ": (offs, np.array([1, 2, 3, 0, 0xFFFFFFFF], np.uint32)),
           "2^32": (np.array([0, 0, 0, 0, 1 << 32], np.uint64), cols),
           "2^32 ": (np.array([0, 2, 3, 3, (1 << 64) - 1], np.uint64), cols)}
    for form in (csr_host, csr_device):
        for word, (o, c) in bad.items():
            rc, a, b, w, count = form(native, 4, o, c)
            assert rc == NN.ERR_ARG and word.strip() in NN.last_error(), (form.__name__, word, rc, NN.last_error())
            assert count == COUNT and (a == A).all() and (b == B).all() and (w == W).all(), (word, "written")
        rc, a, b, w, count = form(native, 4, offs, cols)          # the well-formed one, after all that
        assert rc == NN.OK and count == 3 and a[:3].tolist() == [0, 0, 0] and b[:3].tolist() == [1, 2, 3] and w[:3].tolist() == [0, 0, 0]


def test_two_host_threads_call_at_once(native):
    jobs = {}
    for name, (n, out) in {"a": (20000, 1), "b": (3000, 2)}.items():
        rng = np.random.default_rng(n + 1)
        offsets, cols, order = to_csr(n, np.stack([np.repeat(np.arange(n), out), rng.integers(0, n, n * out)], 1))
        d = (rng.integers(0, 50, len(cols)).astype(np.float32) / 8)[order]
        jobs[name] = (offsets, cols, d, spanning_forest(n, csr_triples(offsets, cols, d)))
    out, errs = {}, []

    def run(name):
        try:
            out[name] = [native.csr_spanning_forest(*jobs[name][:3]) for _ in range(3)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=(name,)) for name in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for name, (_, _, _, (a, b, w)) in jobs.items():
        for got in out[name]:
            assert np.array_equal(got.a, a) and np.array_equal(got.b, b) and np.array_equal(_bits(got.weights), _bits(w)), name


# ----------------------------------------------------------------------------------------------------- the index entries
_WANT = {}


def want_of(ix, k, ef, mode, core_k=0):
    """the model's (a, b, w), computed once per case and shared"""
    key = (id(ix), k, ef, mode, core_k)
    if key not in _WANT:
        res, pos = ix.D(k, ef)
        _WANT[key] = (ix, spanning_forest(ix.n, pair_weights(ix.n, res.counts, pos, res.dists, mode, core_k)))   # (ix is kept: an id is unique among LIVE objects only)
    return _WANT[key][1]


def check_index(ix, k, ef, mode, core_k=0, what=""):
    a, b, w = want_of(ix, k, ef, mode, core_k)
    got = ix.h.knn_graph_spanning_forest(k, ef, mode, core_k)
    what = f"{what} n {ix.n} k {k} ef {ef} {mode} core_k {core_k}"
    assert got.n_edges == len(a), (what, got.n_edges, len(a))
    assert got.a.dtype == np.uint32 and np.array_equal(got.a, a) and np.array_equal(got.b, b), (what, "ends", np.flatnonzero((got.a != a) | (got.b != b))[:4])
    assert got.weights.dtype == np.float32 and np.array_equal(_bits(got.weights), _bits(w)), (what, "weight bits")
    return got


def check_all(ix, k, what="", efs=EFS, core_ks=(0,)):
    for ef in efs:
        for mode in MODES:
            for core_k in sorted({min(c, k) for c in core_ks}):    # (core_k <= k)
                check_index(ix, k, ef, mode, core_k, what)


def _order(w):
    """the order bits of f32 weights, as the kernels compare them"""
    from test_exact_knn_abi import _order_bits
    return _order_bits(np.ascontiguousarray(w, np.float32))


def cross_check(ix, k, ef, cuts):
    """what ties the forest to the components: at every cut labels_at equals knn_graph_components, n_edges = n - c, the answer ascends
    by (weight, a, b) and a < b everywhere"""
    for mode in MODES:
        f = ix.h.knn_graph_spanning_forest(k, ef, mode)
        assert (f.a < f.b).all()
        key = list(zip(_order(f.weights).tolist(), f.a.tolist(), f.b.tolist()))
        assert key == sorted(key) and len(set(key)) == len(key), (mode, "not ascending")
        for cut in cuts:
            want = ix.h.knn_graph_components(k, ef, mode, cut)
            got = f.labels_at(cut)
            assert got.n_components == want.n_components, (mode, cut, got.n_components, want.n_components)
            assert np.array_equal(got.labels, want.labels) and np.array_equal(got.sizes, want.sizes), (mode, cut)
            if cut is None:
                assert f.n_edges == ix.n - want.n_components


@pytest.mark.parametrize("n", [1, 2, 3])
def test_small_indexes(native, oracle, tmp_path, n):
    ix = Index(native, oracle, tmp_path, uniform(n, 8, 10 + n))
    for k in (1, 3):
        check_all(ix, k, "small", core_ks=(0, 1, k))
    got = ix.h.knn_graph_spanning_forest(3)
    assert got.n_edges == n - 1                                  # k >= n - 1: the complete graph
    cross_check(ix, 3, None, (None, float("inf"), 0.0))
    # the host entry itself: the slots behind the count stay as they were
    a, b, w, c = np.full(n + 2, A, np.uint32), np.full(n + 2, B, np.uint32), np.full(n + 2, W, np.uint32), np.full(1, COUNT, np.uint64)
    assert native.lib().hnswgpu_graph_spanning_forest(ix.h.handle, 1, 0, 1, 0, _p(a), _p(b), _p(w), _p(c)) == 0
    want = want_of(ix, 1, None, "mutual")
    m = int(c[0])
    assert m == len(want[0]) and np.array_equal(a[:m], want[0]) and np.array_equal(b[:m], want[1]) and np.array_equal(w[:m], _bits(want[2]))
    assert (a[m:] == A).all() and (b[m:] == B).all() and (w[m:] == W).all()


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_wave_and_block_edges(native, oracle, tmp_path_factory, n):
    """k = 1 gives many components; one wavefront less one, one, one more; a block and a bit"""
    ix = _uniform_index(native, oracle, tmp_path_factory, n)
    for k in (1, 3):
        check_all(ix, k, "edges", core_ks=(0, 1, 3) if k == 3 else (0, 1))
    assert len(want_of(ix, 1, None, "union")[0]) < n - 1
    cross_check(ix, 3, 32, (None, float("inf"), 0.0))


@pytest.mark.parametrize("k", [5, 16])
def test_many_blocks(native, oracle, tmp_path_factory, k):
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    check_all(ix, k, "3000", core_ks=(0, 1, 3, k))


def test_the_forest_gives_the_components_at_every_cut(native, oracle, tmp_path_factory):
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    res, _ = ix.D(5, None)
    median = float(np.median(res.dists[np.arange(5)[None, :] < res.counts[:, None]]))
    for ef in EFS:
        cross_check(ix, 5, ef, (None, float("inf"), 0.0, median))
    f = ix.h.knn_graph_spanning_forest(5)
    assert 1 < f.labels_at(median).n_components < ix.n          # (the cut does cut)


def test_core_distances_only_raise_weights(native, oracle, tmp_path_factory):
    """mutual reachability on the model's side: the pairs are those of core_k = 0 and no weight falls; at core_k = k every weight is a
    k-th neighbour distance at least"""
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    res, pos = ix.D(5, None)
    plain = pair_weights(ix.n, res.counts, pos, res.dists, "union", 0)
    raised = pair_weights(ix.n, res.counts, pos, res.dists, "union", 5)
    assert [(x[0], x[1]) for x in plain] == [(x[0], x[1]) for x in raised]
    assert all(r[2] >= p[2] for p, r in zip(plain, raised)) and any(r[2] > p[2] for p, r in zip(plain, raised))
    got = check_index(ix, 5, None, "union", 5, "core")
    assert got.weights.min() >= res.dists[:, 4].min()


def test_separated_clusters_give_a_forest_of_forty_trees(native, oracle, tmp_path):
    """40 tight clusters of 50 points: the exact D never leaves a cluster (asserted on D) and joins each one -- exactly 39 edges of a
    spanning tree are missing"""
    ix = Index(native, oracle, tmp_path, hub_data()[:2000])
    cluster = np.arange(2000) // 50                             # (ids are 0 .. n - 1: position = id)
    res, pos = ix.D(5, None)
    assert bool((cluster[pos] == cluster[:, None])[np.arange(5)[None, :] < res.counts[:, None]].all())     # the precondition, on D
    got = check_index(ix, 5, None, "union", 0, "clusters")
    assert got.n_edges == ix.n - 1 - 39
    assert (cluster[got.a] == cluster[got.b]).all()
    for mode in MODES:
        for ef in EFS:
            check_index(ix, 5, ef, mode, 2, "clusters")


def test_exact_copies_tie_at_weight_zero(native, oracle, tmp_path):
    base = uniform(400, 8, 31)
    perm = np.random.default_rng(32).permutation(1200)
    X = np.ascontiguousarray(np.tile(base, (3, 1))[perm])
    ix = Index(native, oracle, tmp_path, X, np.ascontiguousarray((np.arange(1200, dtype=np.uint64) * 2 + 1)[perm]))
    for k in (1, 5):
        check_all(ix, k, "copies", core_ks=(0, 1, 2))
    got = check_index(ix, 2, None, "mutual", 0, "copies")
    assert (got.weights[:800] == 0).all() and got.labels_at(0.0).sizes.tolist() == [3] * 400              # two edges per triple, first
    cross_check(ix, 2, None, (None, 0.0))


def test_a_pair_whose_two_directions_differ(native, oracle, tmp_path):
    """DistJeffreys: d(i->j) and d(j->i) differ in their bits for some mutual pair of D; UNION weighs it by the smaller, MUTUAL by the
    larger -- and the cut between the two separates the modes, as it separates the components"""
    ix = Index(native, oracle, tmp_path, positive(300, 8, 0), metric="DistJeffreys")
    res, pos = ix.D(5, None)
    slot = {(i, int(pos[i, s])): res.dists[i, s] for i in range(ix.n) for s in range(int(res.counts[i]))}
    differing = sorted((i, j) for (i, j), d in slot.items() if i < j and (j, i) in slot and slot[(j, i)].view(np.uint32) != d.view(np.uint32))
    assert len(differing) >= 2, "the data must hold a pair whose two directions differ in their bits"     # on D
    lo, hi = differing[0]
    small, large = sorted((slot[(lo, hi)], slot[(hi, lo)]))
    union = {(x[0], x[1]): x[2] for x in pair_weights(ix.n, res.counts, pos, res.dists, "union")}
    mutual = {(x[0], x[1]): x[2] for x in pair_weights(ix.n, res.counts, pos, res.dists, "mutual")}
    assert union[(lo, hi)] == small and mutual[(lo, hi)] == large and small < large
    for mode in MODES:
        for core_k in (0, 3):
            check_index(ix, 5, None, mode, core_k, "Jeffreys")
    check_index(ix, 5, 32, "mutual", 0, "Jeffreys")
    cross_check(ix, 5, None, (None, float(small), float(large)))


def test_device_entry_on_a_stream(native, oracle, tmp_path_factory, tmp_path):
    import torch
    NN = native._native
    L = native.lib()
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    stream = torch.cuda.Stream()
    m = ix.n - 1
    for ef in EFS:
        for mode in MODES:
            for core_k in (0, 3):
                a, b, w = want_of(ix, 5, ef, mode, core_k)
                d_a = torch.from_numpy(np.full(m, A, np.uint32).view(np.int32)).cuda()
                d_b = torch.from_numpy(np.full(m, B, np.uint32).view(np.int32)).cuda()
                d_w = torch.from_numpy(np.full(m, W, np.uint32).view(np.int32)).cuda()
                torch.cuda.synchronize()
                count = np.full(1, COUNT, np.uint64)
                rc = L.hnswgpu_graph_spanning_forest_device(ix.h.handle, 5, 0 if ef is None else ef, MODE_CODE[mode], core_k, _ptr(d_a), _ptr(d_b),
                                                            _ptr(d_w), _p(count), C.c_void_p(stream.cuda_stream))
                assert rc == NN.OK, NN.last_error()
                c = int(count[0])
                got_a, got_b, got_w = (t.cpu().numpy().view(np.uint32) for t in (d_a, d_b, d_w))
                assert c == len(a) and np.array_equal(got_a[:c], a) and np.array_equal(got_b[:c], b) and np.array_equal(got_w[:c], _bits(w)), (ef, mode, core_k)
                assert (got_a[c:] == A).all() and (got_b[c:] == B).all() and (got_w[c:] == W).all()
    cold = Index(native, oracle, tmp_path, uniform(65, 8, 65), upload=False)               # never uploaded
    d_a = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    d_b = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    d_w = torch.full((64,), -1, dtype=torch.int32, device="cuda")
    count = np.full(1, COUNT, np.uint64)
    rc = L.hnswgpu_graph_spanning_forest_device(cold.h.handle, 3, 0, 0, 0, _ptr(d_a), _ptr(d_b), _ptr(d_w), _p(count), None)
    assert rc == NN.ERR_DEVICE and "upload" in NN.last_error()
    assert count[0] == COUNT and (d_a == -1).all() and (d_b == -1).all() and (d_w == -1).all()


def test_the_forest_of_the_symmetrised_graph_on_the_device(native, oracle, tmp_path_factory):
    """hnswgpu_symmetric_graph_device's outputs, as they stand on the device, into hnswgpu_csr_spanning_forest_device: DistL2 stores
    the same bits in both directions, so the CSR's forest is the index form's, UNION and MUTUAL"""
    import torch
    NN = native._native
    L = native.lib()
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    for mode in MODES:
        cap = 2 * ix.n * 5
        offs = torch.zeros(ix.n + 1, dtype=torch.int64, device="cuda")
        pos = torch.zeros(cap, dtype=torch.int32, device="cuda")
        dists = torch.zeros(cap, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc = L.hnswgpu_symmetric_graph_device(ix.h.handle, 5, 0, MODE_CODE[mode], cap, _ptr(offs), _ptr(pos), None, _ptr(dists), None, None, None)
        assert rc == NN.OK, NN.last_error()
        d_a = torch.zeros(ix.n - 1, dtype=torch.int32, device="cuda")
        d_b = torch.zeros(ix.n - 1, dtype=torch.int32, device="cuda")
        d_w = torch.zeros(ix.n - 1, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        count = np.zeros(1, np.uint64)
        rc = L.hnswgpu_csr_spanning_forest_device(0, ix.n, _ptr(offs), _ptr(pos), _ptr(dists), _ptr(d_a), _ptr(d_b), _ptr(d_w), _p(count), None)
        assert rc == NN.OK, NN.last_error()
        a, b, w = want_of(ix, 5, None, mode)
        c = int(count[0])
        assert c == len(a) and np.array_equal(d_a.cpu().numpy()[:c].view(np.uint32), a) and np.array_equal(d_b.cpu().numpy()[:c].view(np.uint32), b)
        assert np.array_equal(_bits(d_w.cpu().numpy()[:c]), _bits(w))


def test_the_same_call_gives_the_same_bytes(native, oracle, tmp_path_factory, knob):
    """twice in a row; and with D arriving in many chunks (HNSWGPU_GRAPH_CHUNK = 97: 31 chunks, the last partial)"""
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)

    def all_of(ef, mode):
        got = ix.h.knn_graph_spanning_forest(16, ef, mode, 3)
        return got.a.tobytes() + got.b.tobytes() + got.weights.tobytes()
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
        a, b, w = want_of(ix, 16, None, mode, 3)
        assert first[None] == a.tobytes() + b.tobytes() + w.tobytes()
