"""HDBSCAN on the device (forest_hdbscan -> hnswhdb_forest / _device, Hnsw.hdbscan -> hnswhdb_graph / _device,
csrc/condensed_tree.hip).

The expected answers never come from the code under test: `hdbscan_model` of tests/test_hdbscan_abi.py reads the header's definitions
over the same forest.  Exact, for host and device forms: the integer arrays and counts, all weight bits, selected, labels and the bits
of prob, with the sentinels behind the answers intact and two calls giving equal bytes.  Stabilities are compared EXACTLY where every
weight is a power of two (or 0, +inf, NaN) and the sizes are small: every term and every sum is then exact in f64 whatever the order,
and exact ties are legitimate -- the parent must win them.  On float weights they are compared within
|dev - fsum(terms)| <= rows(C) 2^-53 fsum(terms), the bound for any order of summation of rows(C) non-negative terms that are the same
bits in model and device; such a test first asserts on the model alone that every excess-of-mass decision has a margin
(tests/test_hdbscan_abi.py: has_margins), so that the exact comparison of the labels is sound."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from conftest import uniform
from test_gpu_dendrogram import _bit_reversed, path
from test_gpu_symmetric_graph import Index, _uniform_index
from test_hdbscan_abi import COUNT, METHOD_CODE, ORDER, Outs, balanced_pairs, has_margins, hdbscan_model, max_clusters

pytestmark = pytest.mark.gpu
PAD = 3                                                        # slots behind the last vertex and the last cluster
METHODS = ("eom", "leaf")
_TORCH_VIEW = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_TORCH_VIEW.get(a.dtype, a.dtype)).copy()).cuda()


def _host_like(t, like):
    return t.cpu().numpy().view(like.dtype)


# ----------------------------------------------------------------------------------------------------- the forest entries
def forest_host(native, n, a, b, w, mcs, method):
    """the host entry itself on out arrays at their sentinels: (rc, Outs)"""
    o = Outs(n + PAD, max_clusters(n, mcs) + PAD)
    m = len(a)
    rc = native.lib().hnswhdb_forest(0, n, m, _p(a) if m else None, _p(b) if m else None, _p(w) if m else None, mcs, METHOD_CODE[method],
                                             *[_p(o.arrays()[x]) for x in ORDER])
    return rc, o


def forest_device(native, n, a, b, w, mcs, method, stream=None):
    """the device entry on tensors at their sentinels: (rc, Outs)"""
    import torch
    o = Outs(n + PAD, max_clusters(n, mcs) + PAD)
    m = len(a)
    ins = [_dev(x if m else np.zeros(1, x.dtype)) for x in (a, b, w.view(np.uint32))]
    names = ORDER[:-2]
    t = {x: _dev(o.arrays()[x]) for x in names}
    torch.cuda.synchronize()
    rc = native.lib().hnswhdb_forest_device(0, n, m, *[_ptr(x) for x in ins], mcs, METHOD_CODE[method], *[_ptr(t[x]) for x in names], _p(o.k), _p(o.l),
                                                    C.c_void_p(stream.cuda_stream) if stream is not None else None)
    for x, src in zip(ins, (a, b, w.view(np.uint32))):
        assert np.array_equal(_host_like(x, src)[:m], src), "an input was written"
    for x in names:
        o.arrays()[x][:] = _host_like(t[x], o.arrays()[x])
    return rc, o


def compare(o, want, what, exact):
    """the out arrays of a call against the model; the slots behind n and K as they were"""
    n, K = want.n, want.K
    assert (int(o.k[0]), int(o.l[0])) == (K, want.L), (what, "counts", o.k[0], o.l[0], K, want.L)
    for name, got, exp in (("point_cluster", o.pc[:n], want.point_cluster), ("point_w", o.pw[:n], want.point_w),
                           ("cluster_parent", o.cparent[:K], want.cluster_parent), ("cluster_birth_w", o.cbirth[:K], want.cluster_birth_w),
                           ("cluster_size", o.csize[:K], want.cluster_size)):
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, (what, name, bad[:4], got[bad[:4]], exp[bad[:4]])
    stab = o.stab[:K].view(np.float64)
    for c in range(K):
        exp = float(want.stability[c])
        if exact or math.isinf(exp):
            assert stab[c] == exp, (what, "stability", c, stab[c], exp)
        else:
            assert abs(stab[c] - exp) <= len(want.terms[c]) * 2.0 ** -53 * exp, (what, "stability", c, stab[c], exp, len(want.terms[c]))
    for name, got, exp in (("selected", o.sel[:K], want.selected), ("labels", o.labels[:n], want.labels),
                           ("prob", o.prob[:n], want.prob.view(np.uint32))):
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, (what, name, bad[:4], got[bad[:4]], exp[bad[:4]])
    assert o.untouched(n, K), (what, "behind the answer")


def _bytes(o):
    return b"".join(o.arrays()[x].tobytes() for x in ORDER)


def check_forest(native, n, edges, w, mcs, what="", exact=True, methods=METHODS, forms=("host", "host again", "device")):
    """both methods: host form (twice: the same bytes) and device form against the model.  Returns the models by method."""
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    a, b = np.ascontiguousarray(edges[:, 0], np.uint32), np.ascontiguousarray(edges[:, 1], np.uint32)
    w = np.ascontiguousarray(w, np.float32)
    out = {}
    for method in methods:
        want = hdbscan_model(n, a, b, w, mcs, method)
        assert want is not None, (what, "the model refuses the forest")
        if not exact and method == "eom":
            assert has_margins(want), (what, mcs, "an excess-of-mass decision of the model is too close to a tie: choose another input")
        first = None
        for form in forms:
            rc, o = (forest_device if form == "device" else forest_host)(native, n, a, b, w, mcs, method)
            assert rc == 0, (what, mcs, method, form, native._native.last_error())
            compare(o, want, (what, mcs, method, form), exact)
            if form == "host":
                first = _bytes(o)
            elif form == "host again":
                assert _bytes(o) == first, (what, mcs, method, "two calls differ")
        out[method] = want
    return out


def by_level(count, per_level, low=-4):
    """count weights that ascend, powers of two, per_level of each"""
    return np.exp2(low + np.arange(count) // per_level).astype(np.float32)


def mcs_values(n):
    return sorted({x for x in (2, 3, 5, n, n + 1) if x >= 2})


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257])
def test_paths_of_the_vertex_counts(native, n):
    """a path in order has chain depth n - 1 and one cluster chain that the points leave one by one; reversed, and permuted, where
    true splits appear.  mcs = n: one cluster, the root; n + 1: not even a big node."""
    e = path(n)
    w = by_level(n - 1, 16)
    rng = np.random.default_rng(n)
    for mcs in mcs_values(n):
        got = check_forest(native, n, e, w, mcs, f"path {n} in order")
        assert got["eom"].K == 1 and (got["eom"].labels == -1).all()
        check_forest(native, n, e[::-1], w, mcs, f"path {n} reversed", forms=("host", "device"))
        check_forest(native, n, e[rng.permutation(n - 1)] if n > 1 else e, w, mcs, f"path {n} permuted", forms=("host", "device"))
    if n == 257:
        got = check_forest(native, n, e[rng.permutation(n - 1)], w, 5, "path 257 permuted again")
        assert got["eom"].K > 3
        # float weights: the bound, behind the margins
        wf = np.sort(np.random.default_rng(2570).random(n - 1, dtype=np.float32) + np.float32(0.05))
        check_forest(native, n, e[np.random.default_rng(2571).permutation(n - 1)], wf, 5, "path 257 permuted, float weights", exact=False)


def test_no_edge(native):
    for n in (1, 5, 300):
        got = check_forest(native, n, [], [], 2, f"m = 0, n = {n}")
        assert got["eom"].K == 1 and (got["eom"].labels == -1).all() and (got["eom"].point_w == 0x7F800000).all()
        res = native.forest_hdbscan(n, [], [], [], 2)
        assert res.n_clusters == 1 and res.n_labels == 0 and res.labels.tolist() == [-1] * n and res.probabilities.tolist() == [0.0] * n
        assert res.cluster_parent.tolist() == [0xFFFFFFFF] and res.cluster_size.tolist() == [n] and res.stability.tolist() == [0.0]


def test_the_bit_reversed_path_is_the_balanced_tree(native):
    """4 096 vertices; the weight of an edge is 2^(its level): mcs = 2 makes every merge above the pairs a true split, K at its bound"""
    n = 4096
    e = path(n)
    order = np.argsort(np.array([_bit_reversed(i, 12) for i in range(n - 1)]), kind="stable")
    level = np.array([len(format(i, "b")) - len(format(i, "b").rstrip("1")) for i in range(n - 1)])    # trailing ones of the edge's index
    w = np.exp2(level[order]).astype(np.float32)
    assert (np.diff(w) >= 0).all()
    for mcs in (2, 3, 64):
        got = check_forest(native, n, e[order], w, mcs, "bit-reversed path", forms=("host", "device") if mcs != 2 else ("host", "host again", "device"))
        if mcs == 2:
            assert got["eom"].K == max_clusters(n, 2) == 4095
        assert got["leaf"].L == n // (2 if mcs == 2 else 4 if mcs == 3 else 64)


def test_a_star_of_seventy_thousand_leaves(native):
    """every merge but the first takes the cluster before it: one chain that the points leave one by one, 70 001 rows in one cluster.
    A path of ten apart makes the star a cluster of its own (two big dendrogram roots)."""
    n_star = 70001
    rng = np.random.default_rng(7)
    leaves = 1 + rng.permutation(n_star - 1)
    star = np.stack([np.zeros(n_star - 1, np.int64), leaves], 1)
    star[::2] = star[::2, ::-1]
    tail = path(10) + n_star
    e = np.concatenate([tail, star])
    w = np.concatenate([np.full(9, 0.5, np.float32), by_level(n_star - 1, 20000, 0)])
    got = check_forest(native, n_star + 10, e, w, 5, "star and a path", forms=("host", "device"))
    assert got["eom"].K == 3 and got["eom"].L == 2 and got["eom"].cluster_size.tolist() == [n_star + 10, n_star, 10]
    got = check_forest(native, n_star, star, by_level(n_star - 1, 20000, 0), 5, "star alone", methods=("eom",), forms=("device",))
    assert got["eom"].K == 1


def comb(groups, mcs, per_level=8):
    """groups paths of mcs vertices closed at weight 1/2, group g + 1 joined to the groups before it: each split peels one group"""
    e, w = [], []
    for g in range(groups):
        for i in range(mcs - 1):
            e.append((g * mcs + i, g * mcs + i + 1))
            w.append(0.5)
    for g in range(1, groups):
        e.append((g * mcs, (g - 1) * mcs + mcs - 1))
        w.append(2.0 ** ((g - 1) // per_level))
    return groups * mcs, np.array(e, np.int64), np.array(w, np.float32)


def test_a_comb_has_a_cluster_tree_of_depth_two_hundred(native):
    """the arrival counters climb 199 steps in one launch, and the doubling needs all its rounds"""
    for mcs in (3, 5):
        n, e, w = comb(200, mcs)
        got = check_forest(native, n, e, w, mcs, "comb")["eom"]
        assert got.K == 2 * 200 - 1
        depth, c = 0, got.K - 1
        while c != 0:
            c, depth = int(got.cluster_parent[c]), depth + 1
        assert depth >= 199


def test_a_balanced_cluster_tree_of_256_leaves(native):
    n, a, b, w = balanced_pairs(256)
    got = check_forest(native, n, np.stack([a, b], 1), w, 2, "balanced pairs")
    assert got["eom"].K == 511 and got["leaf"].L == 256


def test_an_exact_tie_goes_to_the_parent(native):
    """two triples that close at 1/2 and join at 1, beside a third triple: the cluster of six is born at lambda 0 and splits at 1, its
    children lose their points at 2 -- (1 - 0) 6 against (2 - 1) 3 + (2 - 1) 3.  The parent wins: one label for the six."""
    e = [(0, 1), (1, 2), (3, 4), (4, 5), (6, 7), (7, 8), (2, 3)]
    w = [0.5] * 6 + [1.0]
    got = check_forest(native, 9, e, w, 3, "tie")
    eom = got["eom"]
    assert eom.K == 5 and eom.decisions == {1: (6.0, 6.0, 8)}
    assert eom.L == 2 and len(set(eom.labels[:6].tolist())) == 1 and eom.labels[6] != eom.labels[0]
    assert got["leaf"].L == 3
    res = native.forest_hdbscan(9, [x for x, _ in e], [y for _, y in e], w, 3)
    assert res.n_labels == 2 and res.labels.tolist() == eom.labels.tolist() and res.stability.tolist() == eom.stability.tolist()
    # the tie one level down as well: two such sixes under a common parent of twelve, every level a tie or a win of the parent
    e2 = e[:4] + [(2, 3)] + [(x + 9, y + 9) for x, y in e[:4]] + [(11, 12)] + [(5, 9)] + [(20, 21), (21, 22)]
    w2 = [0.5] * 4 + [1.0] + [0.5] * 4 + [1.0] + [2.0] + [4.0, 4.0]
    order = np.argsort(np.array(w2), kind="stable")
    check_forest(native, 23, np.array(e2)[order], np.array(w2)[order], 3, "ties on two levels")


def test_the_leaves_of_the_tie_under_the_shared_climb(native):
    """the first forest of test_an_exact_tie_goes_to_the_parent under HNSWGPU_SELECT_LEAF: the selection is the one that the second
    stage runs, and its climb runs for the leaf method too, where it carries the death lambdas and lets no cluster with children win.
    The model's two answers differ on this forest -- the tie's parent under excess of mass, its two children as leaves --, so a climb
    that decided the parent here would show.  Host and device form, byte for byte."""
    e = np.array([(0, 1), (1, 2), (3, 4), (4, 5), (6, 7), (7, 8), (2, 3)], np.uint32)
    a, b, w = np.ascontiguousarray(e[:, 0]), np.ascontiguousarray(e[:, 1]), np.array([0.5] * 6 + [1.0], np.float32)
    leaf, eom = hdbscan_model(9, a, b, w, 3, "leaf"), hdbscan_model(9, a, b, w, 3, "eom")
    assert (leaf.L, eom.L) == (3, 2) and leaf.selected.tolist() != eom.selected.tolist() and leaf.labels.tolist() != eom.labels.tolist()
    for form, call in (("host", forest_host), ("device", forest_device)):
        rc, o = call(native, 9, a, b, w, 3, "leaf")
        assert rc == 0, (form, native._native.last_error())
        compare(o, leaf, ("tie, leaf", form), True)


def test_equal_and_extreme_weights(native):
    rng = np.random.default_rng(3)
    n = 257
    e = path(n)[rng.permutation(n - 1)]
    check_forest(native, n, e, np.ones(n - 1, np.float32), 5, "all weights equal")
    zeros = np.zeros(n - 1, np.float32)
    zeros[1::2] = -0.0                                          # lambda = inf on every row: inf - inf terms are 0
    check_forest(native, n, e, zeros, 5, "weights 0 and -0")
    mixed = np.concatenate([np.zeros(100, np.float32), -np.zeros(28, np.float32), by_level(n - 1 - 128 - 3, 16),
                            np.array([0x7F800000, 0x7FC00001, 0xFFC12345], np.uint32).view(np.float32)])
    got = check_forest(native, n, e, mixed, 5, "zeros, then powers of two, +inf and two NaNs at the end")
    assert np.isinf(got["eom"].stability).any()
    check_forest(native, n, e, mixed, 2, "the same, mcs = 2")
    check_forest(native, n, e, np.concatenate([by_level(n - 4, 32), np.array([0x7F800000, 0x7F800000, 0x7FFFFFFF], np.uint32).view(np.float32)]), 3,
                 "+inf twice and a NaN at the end")


def test_the_number_of_big_dendrogram_roots(native):
    """isolated vertices and small components around none, one, two and five big ones (mcs = 4)"""
    def parts(sizes):
        e, start = [], 0
        for s in sizes:
            e += [(start + i, start + i + 1) for i in range(s - 1)]
            start += s + 1                                       # an isolated vertex between two parts
        return start, np.array(e, np.int64).reshape(-1, 2)
    for sizes, roots in (((2, 3, 1, 3), 0), ((3, 9, 2), 1), ((8, 2, 4, 3), 2), ((4, 5, 3, 6, 7, 2, 12), 5)):
        n, e = parts(sizes)
        e = e[np.random.default_rng(len(sizes)).permutation(len(e))]
        got = check_forest(native, n, e, by_level(len(e), 3), 4, f"{roots} big roots")["eom"]
        assert got.K >= (1 if roots < 2 else 1 + roots)
        if roots >= 2:                                           # the children of cluster 0 are the big dendrogram roots
            assert int((got.cluster_parent[1:] == 0).sum()) == roots
        if roots == 0:
            assert (got.point_w == 0x7F800000).all() and (got.labels == -1).all()


def test_an_invalid_forest_is_an_argument_error_never_a_fault(native):
    NN = native._native
    bad = {"weights that descend": (4, [(0, 1), (1, 2), (2, 3)], [1, 3, 2], "descend"),
           "a NaN before +inf": (4, [(0, 1), (1, 2), (2, 3)], [1, np.nan, np.inf], "descend"),
           "a triangle": (4, [(0, 1), (1, 2), (2, 0)], [1, 1, 1], "cycle"),
           "a repeated pair": (4, [(0, 1), (2, 3), (1, 0)], [1, 2, 3], "cycle"),
           "an end at n": (4, [(0, 1), (1, 4), (2, 3)], [1, 2, 3], "not below n"),
           "a self-loop": (4, [(0, 1), (2, 2), (2, 3)], [1, 2, 3], "itself")}
    for form in (forest_host, forest_device):
        for name, (n, e, w, word) in bad.items():
            e = np.asarray(e, np.int64)
            for method in METHODS:
                rc, o = form(native, n, e[:, 0].astype(np.uint32), e[:, 1].astype(np.uint32), np.array(w, np.float32), 2, method)
                assert rc == NN.ERR_ARG and word in NN.last_error(), (form.__name__, name, rc, NN.last_error())
                assert o.untouched(), (form.__name__, name, "written")
        check_forest(native, 4, [(0, 1), (3, 2), (2, 1)], [1, 1, 2], 2, "the well-formed one, after all that", forms=("host", "device"))


def test_two_host_threads_call_at_once(native):
    jobs = {}
    for name, n, mcs in (("a", 3000, 5), ("b", 700, 3)):
        rng = np.random.default_rng(n)
        e = path(n)[rng.permutation(n - 1)]
        w = by_level(n - 1, 128)
        jobs[name] = (n, e[:, 0].astype(np.uint32), e[:, 1].astype(np.uint32), w, mcs, hdbscan_model(n, e[:, 0], e[:, 1], w, mcs))
    out, errs = {}, []

    def run(name):
        try:
            out[name] = [native.forest_hdbscan(*jobs[name][:5]) for _ in range(3)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=(name,)) for name in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for name, job in jobs.items():
        want = job[5]
        for got in out[name]:
            assert got.n_clusters == want.K and np.array_equal(got.labels, want.labels) and np.array_equal(got.stability, want.stability), name
            assert got.probabilities.tobytes() == want.prob.tobytes() and np.array_equal(got.selected, want.selected.astype(bool))


def test_forest_device_entry_on_a_stream(native):
    import torch
    n = 3000
    e = path(n)[np.random.default_rng(55).permutation(n - 1)]
    a, b, w = e[:, 0].astype(np.uint32), e[:, 1].astype(np.uint32), by_level(n - 1, 128)
    for method in METHODS:
        rc, o = forest_device(native, n, a, b, w, 5, method, torch.cuda.Stream())
        assert rc == 0, native._native.last_error()
        compare(o, hdbscan_model(n, a, b, w, 5, method), ("stream", method), True)
    res = native.SpanningForestResult(a, b, w, n - 1, n).hdbscan(5)
    assert np.array_equal(res.labels, hdbscan_model(n, a, b, w, 5).labels)


# ----------------------------------------------------------------------------------------------------- the index entries
def check_index(ix, k, ef, mode, core_k, mcs, what="", methods=METHODS):
    """the forest and the dendrogram are knn_graph_dendrogram's, byte for byte; the rest is the model's on them"""
    what = f"{what} n {ix.n} k {k} ef {ef} {mode} core_k {core_k} mcs {mcs}"
    d = ix.h.knn_graph_dendrogram(k, ef, mode, core_k)
    out = {}
    for method in methods:
        got = ix.h.hdbscan(mcs, k, ef, mode, core_k, method)
        for name, x, y in (("a", got.forest.a, d.a), ("b", got.forest.b, d.b), ("w", got.forest.weights, d.weights), ("left", got.dendrogram.left, d.left),
                           ("right", got.dendrogram.right, d.right), ("size", got.dendrogram.sizes, d.sizes)):
            assert x.tobytes() == y.tobytes(), (what, name)
        assert got.forest.n_edges == d.n_edges
        want = hdbscan_model(ix.n, d.a, d.b, d.weights, mcs, method)
        assert want is not None, what
        if method == "eom":
            assert has_margins(want), (what, "an excess-of-mass decision of the model is too close to a tie: choose another input")
        assert (got.n_clusters, got.n_labels) == (want.K, want.L), (what, method)
        assert np.array_equal(got.point_cluster, want.point_cluster) and np.array_equal(got.point_w.view(np.uint32), want.point_w), (what, method)
        assert np.array_equal(got.cluster_parent, want.cluster_parent) and np.array_equal(got.cluster_birth_w.view(np.uint32), want.cluster_birth_w)
        assert np.array_equal(got.cluster_size, want.cluster_size), (what, method)
        for c in range(want.K):
            exp = float(want.stability[c])
            assert abs(got.stability[c] - exp) <= len(want.terms[c]) * 2.0 ** -53 * exp, (what, method, c, got.stability[c], exp)
        assert np.array_equal(got.selected, want.selected.astype(bool)) and np.array_equal(got.labels, want.labels), (what, method)
        assert got.probabilities.tobytes() == want.prob.tobytes(), (what, method)
        out[method] = (got, want)
    return out


@pytest.mark.parametrize("n", [1, 2, 3])
def test_small_indexes(native, oracle, tmp_path, n):
    ix = Index(native, oracle, tmp_path, uniform(n, 8, 10 + n))
    for k in (1, 3):
        for mode in ("union", "mutual"):
            for core_k in (0, min(3, k)):
                for mcs in (2, 3):
                    check_index(ix, k, None, mode, core_k, mcs, "small")
    got = ix.h.hdbscan(2, 3)
    assert got.n_clusters == 1 and got.labels.tolist() == [-1] * n and got.forest.n_edges == n - 1


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_wave_and_block_edges(native, oracle, tmp_path_factory, n):
    """k = 1 gives many components, most of them small: many dendrogram roots"""
    ix = _uniform_index(native, oracle, tmp_path_factory, n)
    for k in (1, 3):
        for ef in (None, 32):
            check_index(ix, k, ef, "union", 0, 5, "edges")
        check_index(ix, k, None, "mutual", 0, 3, "edges")


@pytest.mark.parametrize("k", [5, 16])
def test_many_blocks(native, oracle, tmp_path_factory, k):
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    for ef in (None, 32):
        for mode in ("union", "mutual"):
            for core_k in (0, 3):
                check_index(ix, k, ef, mode, core_k, 10 if core_k else 5, "3000", methods=METHODS if ef is None else ("eom",))


def blobs_and_noise(seed=0):
    """three tight Gaussian blobs of 60 points around far centres, and 20 points uniform on shells around them: 200 points of dimension 8"""
    rng = np.random.default_rng(seed)
    centres = np.zeros((3, 8), np.float32)
    centres[0, 0], centres[1, 1], centres[2, 2] = 20, 20, 20
    blobs = [c + rng.normal(0, 0.05, (60, 8)) for c in centres]
    dirs = rng.normal(0, 1, (20, 8))
    noise = centres[rng.integers(0, 3, 20)] + dirs / np.linalg.norm(dirs, axis=1)[:, None] * rng.uniform(1, 2, (20, 1))
    return np.ascontiguousarray(np.concatenate(blobs + [noise]), np.float32)


def test_three_blobs_and_noise(native, oracle, tmp_path):
    ix = Index(native, oracle, tmp_path, blobs_and_noise())
    got, want = check_index(ix, 10, None, "union", 9, 10, "blobs")["eom"]
    default = ix.h.hdbscan(10, 10)                              # core_k = min(mcs - 1, knbn) = 9
    assert np.array_equal(default.labels, got.labels) and default.probabilities.tobytes() == got.probabilities.tobytes()
    assert got.n_labels == 3
    seen = [set(got.labels[60 * i:60 * i + 60].tolist()) - {-1} for i in range(3)]
    assert all(len(s) == 1 for s in seen) and len(set.union(*seen)) == 3, seen
    assert (got.labels[:180] >= 0).sum() >= 150
    assert (got.probabilities >= 0).all() and (got.probabilities <= 1).all() and (got.probabilities[got.labels < 0] == 0).all()
    t = got.condensed_tree()
    assert len(t) == got.n_clusters - 1 + ix.n and (t["parent"] >= ix.n).all() and t["cluster_size"][:got.n_clusters - 1].tolist() == got.cluster_size[1:].tolist()


def test_index_device_entry_on_a_stream(native, oracle, tmp_path_factory, tmp_path):
    import torch
    from test_dendrogram_abi import A, B, LEFT, RIGHT, SIZE, W
    NN = native._native
    L = native.lib()
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    stream = torch.cuda.Stream()
    s, mcs = ix.n - 1, 5
    for ef, mode, with_six in ((None, "union", True), (32, "mutual", True), (None, "mutual", False)):
        d = ix.h.knn_graph_dendrogram(5, ef, mode, 3)
        want = hdbscan_model(ix.n, d.a, d.b, d.weights, mcs)
        sent = (A, B, W, LEFT, RIGHT, SIZE)
        six = [_dev(np.full(s, x, np.uint32)) for x in sent]
        o = Outs(ix.n + PAD, max_clusters(ix.n, mcs) + PAD)
        names = ORDER[:-2]
        t = {x: _dev(o.arrays()[x]) for x in names}
        count = np.full(1, COUNT, np.uint64)
        torch.cuda.synchronize()
        rc = L.hnswhdb_graph_device(ix.h.handle, 5, 0 if ef is None else ef, 0 if mode == "union" else 1, 3, mcs, 0,
                                            *[_ptr(x) if with_six else None for x in six], *[_ptr(t[x]) for x in names], _p(o.k), _p(o.l), _p(count),
                                            C.c_void_p(stream.cuda_stream))
        assert rc == NN.OK, NN.last_error()
        c = int(count[0])
        assert c == d.n_edges
        for g, exp, x in zip([_host_like(y, np.zeros(1, np.uint32)) for y in six],
                             (d.a, d.b, d.weights.view(np.uint32), d.left, d.right, d.sizes), sent):
            assert (np.array_equal(g[:c], exp) and (g[c:] == x).all()) if with_six else (g == x).all(), (ef, mode)
        for x in names:
            o.arrays()[x][:] = _host_like(t[x], o.arrays()[x])
        assert has_margins(want)
        compare(o, want, ("index on a stream", ef, mode), False)
    cold = Index(native, oracle, tmp_path, uniform(65, 8, 65), upload=False)               # never uploaded
    o = Outs(65, max_clusters(65, 5))
    t = {x: _dev(o.arrays()[x]) for x in ORDER[:-2]}
    count = np.full(1, COUNT, np.uint64)
    rc = L.hnswhdb_graph_device(cold.h.handle, 3, 0, 0, 0, 5, 0, *[None] * 6, *[_ptr(t[x]) for x in ORDER[:-2]], _p(o.k), _p(o.l), _p(count), None)
    assert rc == NN.ERR_DEVICE and "upload" in NN.last_error()
    for x in ORDER[:-2]:
        o.arrays()[x][:] = _host_like(t[x], o.arrays()[x])
    assert count[0] == COUNT and o.untouched()


def test_the_same_call_gives_the_same_bytes(native, oracle, tmp_path_factory, knob):
    """twice in a row; and with D arriving in many chunks (HNSWGPU_GRAPH_CHUNK = 97: 31 chunks, the last partial)"""
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)

    def all_of(ef, mode):
        got = ix.h.hdbscan(10, 16, ef, mode, 3)
        return b"".join(x.tobytes() for x in (got.forest.a, got.forest.weights, got.dendrogram.left, got.dendrogram.sizes, got.labels, got.probabilities,
                                              got.point_cluster, got.point_w, got.cluster_parent, got.cluster_birth_w, got.cluster_size, got.stability,
                                              got.selected))
    for mode in ("union", "mutual"):
        first = {ef: all_of(ef, mode) for ef in (None, 32)}
        for ef in (None, 32):
            assert all_of(ef, mode) == first[ef]
        knob("HNSWGPU_GRAPH_CHUNK", 97)
        try:
            for ef in (None, 32):
                assert all_of(ef, mode) == first[ef], (mode, ef, "chunks of 97")
        finally:
            knob("HNSWGPU_GRAPH_CHUNK", None)
