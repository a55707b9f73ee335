"""The selection stage of HDBSCAN on the device (HdbscanResult.select -> hnswhds_select / _device, csrc/cluster_select.hip).

The expected answers never come from the code under test: `select_model` of tests/test_hdbscan_select_abi.py reads the header's
rules over the condensed tree of `hdbscan_model` (tests/test_hdbscan_abi.py), and the model's own f64 stabilities are what the calls
are given.  Every comparison is exact: selected, labels, the count, the bits of prob, score and death, with the sentinels behind n
and K intact and two calls giving equal bytes.  Below cluster 0 a decision is one commutative f64 add in model and device alike: no
margin is needed.  Cluster 0's sum has the device's own shape: a test in which cluster 0 is a candidate either has stabilities whose
sum is exact in every order (small multiples of a power of two: `sums_exactly`), where exact ties are legitimate and cluster 0 must win
them, or first asserts on the model alone that the decision has a margin (root_has_margin)."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from test_gpu_dendrogram import _bit_reversed, path
from test_gpu_hdbscan import PAD, _dev, _host_like, _p, _ptr, by_level, comb
from test_gpu_symmetric_graph import Index, _uniform_index
from test_hdbscan_abi import METHOD_CODE, ORDER, Outs, balanced_pairs, hdbscan_model, max_clusters
from test_hdbscan_select_abi import IN_ORDER, OUT_ORDER, SelectOuts, model_of_arrays, root_has_margin, select_model, tree_arrays

pytestmark = pytest.mark.gpu
METHODS = ("eom", "leaf")
INF = math.inf


# ----------------------------------------------------------------------------------------------------- the two forms
def select_host(native, t, method="eom", allow=False, eps=0.0, max_size=0, null=()):
    """the host entry itself on out arrays at their sentinels: (rc, SelectOuts).  t: the six arrays; null: out arrays left out"""
    n, K = len(t["pc"]), len(t["parent"])
    o = SelectOuts(n + PAD, K + PAD)
    rc = native.lib().hnswhds_select(0, n, K, *[_p(t[x]) for x in IN_ORDER], METHOD_CODE[method], int(allow), eps, max_size,
                                     *[None if x in null else _p(o.arrays()[x]) for x in OUT_ORDER])
    return rc, o


def select_device(native, t, method="eom", allow=False, eps=0.0, max_size=0, null=(), stream=None):
    """the device entry on tensors at their sentinels: (rc, SelectOuts)"""
    import torch
    n, K = len(t["pc"]), len(t["parent"])
    o = SelectOuts(n + PAD, K + PAD)
    ins = [_dev(t[x].view(np.uint64) if t[x].dtype == np.float64 else t[x]) for x in IN_ORDER]
    names = OUT_ORDER[:-1]
    d = {x: _dev(o.arrays()[x]) for x in names}
    torch.cuda.synchronize()
    rc = native.lib().hnswhds_select_device(0, n, K, *[_ptr(x) for x in ins], METHOD_CODE[method], int(allow), eps, max_size,
                                            *[None if x in null else _ptr(d[x]) for x in names], _p(o.l),
                                            C.c_void_p(stream.cuda_stream) if stream is not None else None)
    for x, name in zip(ins, IN_ORDER):
        src = t[name].view(np.uint64) if t[name].dtype == np.float64 else t[name]
        assert np.array_equal(_host_like(x, src), src), ("an input was written", name)
    for x in names:
        o.arrays()[x][:] = _host_like(d[x], o.arrays()[x])
    return rc, o


def compare(o, want, what, null=()):
    """the out arrays of a call against the model, exactly; the slots behind n and K, and the arrays left out, as they were"""
    n, K = want.n, want.K
    assert int(o.l[0]) == want.L, (what, "n_labels", int(o.l[0]), want.L)
    for name, got, exp, upto in (("sel", o.sel, want.selected, K), ("labels", o.labels, want.labels, n), ("prob", o.prob, want.prob.view(np.uint32), n),
                                 ("score", o.score, want.score.view(np.uint32), n), ("death", o.death, want.death.view(np.uint64), K)):
        if name in null:
            assert (got == SelectOuts(1, 1).arrays()[name][0]).all(), (what, name, "left out, and written")
            continue
        bad = np.flatnonzero(got[:upto] != exp)
        assert len(bad) == 0, (what, name, bad[:4], got[bad[:4]], exp[bad[:4]])
    kept = SelectOuts(len(o.labels), len(o.sel))
    for name in null:
        o.arrays()[name][:] = kept.arrays()[name]
    assert o.untouched(n, K), (what, "behind the answer")


def _bytes(o):
    return b"".join(o.arrays()[x].tobytes() for x in OUT_ORDER)


def sums_exactly(values):
    """every value is a multiple of 2^-24 and all of them together stay below 2^28: their f64 sum is exact in every order"""
    return all(math.isfinite(v) and float(v) * 2.0 ** 24 == int(float(v) * 2.0 ** 24) for v in values) and sum(float(v) for v in values) < 2.0 ** 28


def check(native, base, what, method="eom", allow=False, eps=0.0, max_size=0, stability=None, forms=("host", "host again", "device")):
    """host form (twice: the same bytes) and device form against the model.  Returns the model."""
    want = select_model(base, method, allow, eps, max_size, stability)
    t = tree_arrays(base, stability)
    if allow and method == "eom":
        assert sums_exactly(t["stab"][1:]) or root_has_margin(want), (what, "cluster 0's decision is too close to a tie: choose another input")
    what = (what, method, allow, eps, max_size)
    first = None
    for form in forms:
        rc, o = (select_device if form == "device" else select_host)(native, t, method, allow, eps, max_size)
        assert rc == 0, (what, form, native._native.last_error())
        compare(o, want, (what, form))
        if form == "host":
            first = _bytes(o)
        elif form == "host again":
            assert _bytes(o) == first, (what, "two calls differ")
    return want


def forest(n, edges, w, mcs):
    edges = np.asarray(edges, np.int64).reshape(-1, 2)
    base = hdbscan_model(n, edges[:, 0], edges[:, 1], np.ascontiguousarray(w, np.float32), mcs)
    assert base is not None
    return base


# ----------------------------------------------------------------------------------------------------- the forests
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 257])
def test_paths_of_the_vertex_counts(native, n):
    """a path in order: K = 1, the root alone, with and without allow_single_cluster, the single-root threshold at eps = 0 (maxlambda(0))
    and at eps > 0 (1 / eps, between two weights, at one, above all of them); permuted, where true splits appear"""
    e, w = path(n), by_level(n - 1, 16)
    rng = np.random.default_rng(n)
    for mcs in sorted({x for x in (2, 3, n, n + 1) if x >= 2}):
        base = forest(n, e, w, mcs)
        assert base.K == 1
        for method in METHODS:
            got = check(native, base, f"path {n} in order, mcs {mcs}", method)
            assert got.L == 0 and (got.labels == -1).all()
            for eps in (0.0, 0.09375, 0.125, 1e6, INF):
                got = check(native, base, f"path {n} in order, mcs {mcs}", method, True, eps, forms=("host", "device"))
                assert got.L == 1 and got.selected.tolist() == [1]
                if eps == INF:
                    assert (got.labels == 0).all()
            got = check(native, base, f"path {n} in order, mcs {mcs}", method, True, 0.0, n - 1 if n > 1 else 5, forms=("host", "device"))
            assert got.L == (1 if method == "leaf" or n == 1 else 0)
        if n > 2:
            perm = forest(n, e[rng.permutation(n - 1)], w, mcs)
            for allow in (False, True):
                for eps in (0.0, 0.2, 3.0):
                    check(native, perm, f"path {n} permuted, mcs {mcs}", "eom", allow, eps, forms=("host", "device"))
                    check(native, perm, f"path {n} permuted, mcs {mcs}", "leaf", allow, eps, forms=("device",))


def test_a_comb_of_depth_two_hundred(native):
    """the climb over arrival counters goes 199 steps in one launch and the doublings need all their rounds.  The joins' weights are
    1, 2, 4, .. by eight: eps between two of them merges the lower levels, above all of them every level; eps EQUAL to a weight: a
    child born there stays (strict <), a parent born there is climbed past (strict >)"""
    n, e, w = comb(200, 3)
    base = forest(n, e, w, 3)
    assert base.K == 399
    depth, c = 0, base.K - 1
    while c != 0:
        c, depth = int(base.cluster_parent[c]), depth + 1
    assert depth >= 199
    seen = {}
    for method in METHODS:
        for eps in (0.0, 96.0, 64.0, 128.0, 2.0 ** 24, 2.0 ** 25, INF):
            for allow in (False, True):
                got = check(native, base, "comb", method, allow, eps, forms=("host", "host again", "device") if eps in (0.0, 64.0) else ("host", "device"))
                seen[method, eps, allow] = got
    leaf = {eps: seen["leaf", eps, False] for eps in (0.0, 96.0, 64.0, 128.0, 2.0 ** 25, INF)}
    # 200 leaves: nine born at weight 1, eight at each of 2 .. 2^23, seven at 2^24.  eps = 96: the 57 born at or below 64 end at the
    # cluster born at 128 that holds them.  eps = 64: the 49 born below 64 climb PAST the ancestors born at 64 to that same cluster;
    # the eight leaves born at 64 stay in F, under it, and the antichain drops them: the same 144.  eps = 128: one level further.
    assert [leaf[eps].L for eps in (0.0, 96.0, 64.0, 128.0)] == [200, 144, 144, 136]
    assert leaf[64.0].nested and not leaf[96.0].nested and np.array_equal(leaf[64.0].selected, leaf[96.0].selected)
    # above every weight the climbs end at the two children of 0, or at 0 itself
    assert leaf[2.0 ** 25].L == leaf[INF].L == 2 and seen["leaf", INF, True].selected.tolist() == [1] + [0] * 398
    assert seen["eom", INF, True].selected.tolist() == [1] + [0] * 398 and (seen["eom", INF, True].labels == 0).all()


def test_the_hand_made_forest(native):
    """tests/test_hdbscan_select_abi.py writes these answers out: eps = 1 is the birth of clusters 3 and 4 (strict <: nothing moves)"""
    from test_hdbscan_abi import HAND_A, HAND_B, HAND_W
    base = forest(12, np.stack([HAND_A, HAND_B], 1), HAND_W, 3)
    for kw, selected in ((dict(), [1, 3, 4]), (dict(eps=1.5), [1, 2]), (dict(eps=1.0), [1, 3, 4]), (dict(eps=np.nextafter(np.float32(1), np.float32(2))), [1, 2]),
                         (dict(max_size=3), [3, 4]), (dict(max_size=2), []), (dict(allow=True), [1, 3, 4]), (dict(allow=True, eps=INF), [0])):
        got = check(native, base, "hand-made", **kw)
        assert np.flatnonzero(got.selected).tolist() == selected, kw
    assert got.death.tolist() == [4.0, 0.5, 4.0, 2.0, 4.0] and got.score.tolist() == [0, 0, 0, 0, 0, 0, 0.875, 0, 0, 0, 0.5, 1.0]
    for mcs, w in ((3, [.5, .5, .5, .5, 1, 8, 8, 8, 8]), (7, HAND_W)):
        base = forest(12, np.stack([HAND_A, HAND_B], 1), w, mcs)
        for method in METHODS:
            for allow in (False, True):
                for eps in (0.0, 2.0, 4.0):
                    for max_size in (0, 3, 6, 11):
                        check(native, base, f"hand-made, mcs {mcs}", method, allow, eps, max_size, forms=("host", "device"))


@pytest.mark.parametrize("name", ["balanced pairs", "bit-reversed path"])
def test_max_cluster_size_at_a_size_and_one_below(native, name):
    """every cluster of a balanced tree has a power of two for its size: the limit at a size lets the clusters of that size win,
    one below it does not"""
    if name == "balanced pairs":
        n, a, b, w = balanced_pairs(256)
        base = forest(n, np.stack([a, b], 1), w, 2)
        assert base.K == 511
    else:
        n = 4096
        order = np.argsort(np.array([_bit_reversed(i, 12) for i in range(n - 1)]), kind="stable")
        level = np.array([len(format(i, "b")) - len(format(i, "b").rstrip("1")) for i in range(n - 1)])
        base = forest(n, path(n)[order], np.exp2(level[order]).astype(np.float32), 2)
        assert base.K == 4095
    # with a cluster's own stabilities the pairs win everywhere; size^2 lets every parent win (s^2 >= 2 (s / 2)^2, all exact), so the
    # limit alone decides: the highest clusters that fit
    stab = base.cluster_size.astype(np.float64) ** 2
    free = check(native, base, name, stability=stab)
    assert free.L == 2 and free.selected[0] == 0
    for size, allow, labels in ((64, False, n // 64), (63, False, n // 32), (64, True, n // 64), (2, False, n // 2), (1, False, 0), (n, True, 1),
                                (n - 1, True, 2), (n // 2, False, 2), (n // 2 - 1, False, 4)):
        got = check(native, base, name, "eom", allow, 0.0, size, stab, forms=("host", "device"))
        assert got.L == labels and (base.cluster_size[np.flatnonzero(got.selected)] <= size).all(), (size, allow, got.L)
        check(native, base, name, "leaf", allow, 0.0, size, stab, forms=("device",))
        check(native, base, name, "eom", allow, 0.0, size, forms=("device",))
    check(native, base, name, "eom", True, 8.0, 64, stab)
    check(native, base, name, "leaf", True, 3.0, 0, forms=("host", "device"))


def _three_cases_of_cluster_0(native, base, what):
    """allow_single_cluster on a forest with several dendrogram roots: stability[0] loses (its own 0), ties exactly with the sum
    (cluster 0 wins), wins outright -- the last two with a made-up stability[0]"""
    assert sums_exactly(base.stability)
    sub = select_model(base, "eom", True).root[1]
    assert sub > 0 and len(base.kids[0]) >= 2
    lost = check(native, base, what, "eom", True)
    assert lost.selected[0] == 0 and lost.L >= 2
    for own in (sub, 2 * sub + 1):
        stab = base.stability.copy()
        stab[0] = own
        for eps in (0.0, 0.75):
            won = check(native, base, what, "eom", True, eps, 0, stab)
            assert won.selected.tolist() == [1] + [0] * (base.K - 1) and won.L == 1
        assert check(native, base, what, "eom", False, 0.0, 0, stab, forms=("host", "device")).selected[0] == 0
        assert check(native, base, what, "eom", True, 0.0, base.n - 1, stab, forms=("host", "device")).selected[0] == 0    # cluster 0 holds n
    stab = base.stability.copy()
    stab[0] = np.nextafter(sub, 0.0)                            # one ulp below the sum: cluster 0 loses
    assert check(native, base, what, "eom", True, 0.0, 0, stab, forms=("host", "device")).selected[0] == 0
    check(native, base, what, "leaf", True, 0.0, 0, forms=("host", "device"))


def test_five_big_dendrogram_roots_among_isolated_vertices(native):
    """cluster 0's sum with few children (mcs = 4)"""
    e, start = [], 0
    for s in (4, 5, 3, 6, 7, 2, 12):
        e += [(start + i, start + i + 1) for i in range(s - 1)]
        start += s + 1                                           # an isolated vertex between two parts
    e = np.array(e, np.int64)
    e = e[np.random.default_rng(7).permutation(len(e))]
    base = forest(start, e, by_level(len(e), 3), 4)
    assert int((base.cluster_parent[1:] == 0).sum()) == 5
    _three_cases_of_cluster_0(native, base, "five big roots")


def test_three_hundred_pairs_under_cluster_0(native):
    """K = 301: cluster 0's children pass 256, every thread of the block adds, the first 45 twice"""
    n = 600
    w = np.exp2(np.arange(300) // 64).astype(np.float32)         # 1, 2, 4, 8, 16: five stabilities
    base = forest(n, np.stack([np.arange(0, n, 2), np.arange(1, n, 2)], 1), w, 2)
    assert base.K == 301 and len(base.kids[0]) == 300
    _three_cases_of_cluster_0(native, base, "300 pairs")
    rng = np.random.default_rng(300)                             # float stabilities: the margin, asserted on the model
    stab = np.concatenate([[0.0], rng.random(300) + 0.5])
    for own in (0.0, 100.0, 400.0):
        stab[0] = own
        got = check(native, base, "300 pairs, float stabilities", "eom", True, 0.0, 0, stab)
        assert got.selected[0] == (1 if own == 400.0 else 0)


# ----------------------------------------------------------------------------------------------------- edge values
def test_equal_and_extreme_weights(native):
    rng = np.random.default_rng(3)
    n = 257
    e = path(n)[rng.permutation(n - 1)]
    mixed = np.concatenate([np.zeros(100, np.float32), -np.zeros(28, np.float32), by_level(n - 1 - 128 - 3, 16),
                            np.array([0x7F800000, 0x7FC00001, 0xFFC12345], np.uint32).view(np.float32)])
    zeros = np.zeros(n - 1, np.float32)
    zeros[1::2] = -0.0
    for what, w, mcs in (("all weights equal", np.ones(n - 1, np.float32), 5), ("weights 0 and -0", zeros, 5),
                         ("zeros, powers of two, +inf and two NaNs", mixed, 5), ("the same, mcs = 2", mixed, 2)):
        base = forest(n, e, w, mcs)
        stab = np.where(np.isinf(base.stability), 2.0 ** 20, base.stability)    # (a stability of +inf is legal; the sums stay exact here)
        for method in METHODS:
            for allow in (False, True):
                for eps in (0.0, 1e-30, 0.0625, 1.0, INF):
                    check(native, base, what, method, allow, eps, 0, stab, forms=("host", "device"))
            check(native, base, what, method, True, 0.25, 40, stab, forms=("host", "device"))
        got = check(native, base, what + ", the tree's own stabilities", "eom", False, 0.5)
        assert ((got.score >= 0) & (got.score <= 1)).all()
    assert np.isinf(base.stability).any() and np.isinf(got.death).any() and (got.score == 1).any()


def test_births_of_zero_minus_zero_infinity_and_nan(native):
    """a tree written by hand, K = 7: clusters 3 and 4 under 1 are born at 0 and -0 (lambda +inf; below every eps > 0), 5 and 6 under 2
    at a NaN (counts as +inf: it never climbs) and at 1; cluster 2 itself is born at another NaN, which a climb from 6 stops at
    unless eps is +inf.  The points leave at 0, -0, 1/2, 2, +inf and a NaN."""
    nan1, nan2, minus0 = 0x7FC00001, 0xFFC12345, 0x80000000
    one, inf = int(np.array(1, np.float32).view(np.uint32)), 0x7F800000
    births = np.array([inf, inf, nan1, 0, minus0, nan2, one], np.uint32)
    pw = np.array([0.0, -0.0, 0.5, 2.0, np.inf, np.nan, 0.5, 0.5, 2.0, 2.0, 0.25, 0.25, 0.5, np.inf], np.float32).view(np.uint32)
    base = model_of_arrays([0xFFFFFFFF, 0, 0, 1, 1, 2, 2], births, [14, 4, 4, 2, 2, 2, 2], [0.0, 1.0, 1.0, 4.0, 4.0, 4.0, 4.0],
                           [3, 3, 4, 4, 5, 5, 6, 6, 1, 2, 1, 2, 0, 0], pw)
    seen = {}
    for method in METHODS:
        for allow in (False, True):
            for eps in (0.0, 1e-30, 0.5, 1.0, 2.0, INF):
                seen[method, allow, eps] = check(native, base, "hostile births", method, allow, eps, forms=("host", "device"))
            check(native, base, "hostile births", method, allow, 2.0, 3)
    assert np.flatnonzero(seen["eom", False, 0.0].selected).tolist() == [3, 4, 5, 6]
    assert np.flatnonzero(seen["eom", False, 1e-30].selected).tolist() == [1, 5, 6]      # 3 and 4 end at 1, a child of 0
    assert np.flatnonzero(seen["eom", False, 2.0].selected).tolist() == [1, 2]          # 6 ends at 2, born at a NaN > 2; 5 lies under it
    assert np.flatnonzero(seen["eom", False, 1.0].selected).tolist() == [1, 5, 6]        # 6 is born AT eps: it stays
    assert np.flatnonzero(seen["eom", False, INF].selected).tolist() == [1, 2] and seen["eom", False, INF].nested
    assert np.flatnonzero(seen["eom", True, INF].selected).tolist() == [0]
    assert seen["eom", False, 0.0].death.tolist() == [INF, INF, 4.0, INF, 2.0, 0.0, 2.0]


def test_every_optional_out_array_left_out(native):
    base = forest(*comb(20, 3), 3)
    want = select_model(base, "eom", True, 3.0, 30)
    t = tree_arrays(base)
    for form in (select_host, select_device):
        for null in (("sel",), ("prob",), ("score",), ("death",), ("sel", "prob", "score", "death")):
            rc, o = form(native, t, "eom", True, 3.0, 30, null)
            assert rc == 0, (form.__name__, null, native._native.last_error())
            compare(o, want, (form.__name__, null), null)


# ----------------------------------------------------------------------------------------------------- with the first stage
def _first_stage_device(native, n, a, b, w, mcs, method):
    """hnswhdb_forest_device on device tensors, which stay there: (tensors by name, Outs with the counts, K)"""
    import torch
    o = Outs(n, max_clusters(n, mcs))
    names = ORDER[:-2]
    d = {x: _dev(o.arrays()[x]) for x in names}
    ins = [_dev(x) for x in (a, b, w.view(np.uint32))]
    torch.cuda.synchronize()
    rc = native.lib().hnswhdb_forest_device(0, n, len(a), *[_ptr(x) for x in ins], mcs, METHOD_CODE[method], *[_ptr(d[x]) for x in names], _p(o.k), _p(o.l),
                                            None)
    assert rc == 0, native._native.last_error()
    return d, o, int(o.k[0])


@pytest.mark.parametrize("name", ["comb", "balanced pairs"])
def test_the_defaults_give_the_first_stages_own_bytes(native, name):
    """hnswhdb_forest_device, then hnswhds_select_device with the defaults on the arrays it wrote, in HBM throughout: selected, labels,
    the bits of prob and the count are that call's own, for both methods"""
    import torch
    if name == "comb":
        n, e, w = comb(200, 3)
        a, b, mcs = e[:, 0].astype(np.uint32), e[:, 1].astype(np.uint32), 3
    else:
        n, a, b, w = balanced_pairs(256)
        a, b, w, mcs = np.array(a, np.uint32), np.array(b, np.uint32), np.array(w, np.float32), 2
    for method in METHODS:
        d, first, K = _first_stage_device(native, n, a, b, w, mcs, method)
        o = SelectOuts(n + PAD, K + PAD)
        outs = {x: _dev(o.arrays()[x]) for x in OUT_ORDER[:-1]}
        torch.cuda.synchronize()
        rc = native.lib().hnswhds_select_device(0, n, K, *[_ptr(d[x]) for x in ("cparent", "cbirth", "csize", "stab", "pc", "pw")], METHOD_CODE[method], 0,
                                                0.0, 0, *[_ptr(outs[x]) for x in OUT_ORDER[:-1]], _p(o.l), C.c_void_p(torch.cuda.Stream().cuda_stream))
        assert rc == 0, native._native.last_error()
        got = {x: _host_like(outs[x], o.arrays()[x]) for x in outs}
        theirs = {x: _host_like(d[x], first.arrays()[x]) for x in ("sel", "labels", "prob")}
        assert int(o.l[0]) == int(first.l[0]) and K == hdbscan_model(n, a, b, w, mcs, method).K
        assert got["sel"][:K].tobytes() == theirs["sel"][:K].tobytes() and got["labels"][:n].tobytes() == theirs["labels"][:n].tobytes(), (name, method)
        assert got["prob"][:n].tobytes() == theirs["prob"][:n].tobytes(), (name, method)
        for x in got:
            o.arrays()[x][:] = got[x]
        assert o.untouched(n, K)


def test_composition_in_hbm_on_an_index_of_three_thousand(native, oracle, tmp_path_factory):
    """hnswhdb_graph_device, then hnswhds_select_device with all three options on the arrays it wrote; the model runs on those arrays
    (read back for the model alone), the device's own stabilities included: every decision below cluster 0 is one add"""
    import torch
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    n, mcs = ix.n, 10
    first = Outs(n, max_clusters(n, mcs))
    names = ORDER[:-2]
    d = {x: _dev(first.arrays()[x]) for x in names}
    edges = np.zeros(1, np.uint64)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc = native.lib().hnswhdb_graph_device(ix.h.handle, 16, 0, 0, 3, mcs, 0, *[None] * 6, *[_ptr(d[x]) for x in names], _p(first.k), _p(first.l), _p(edges),
                                           C.c_void_p(stream.cuda_stream))
    assert rc == 0, native._native.last_error()
    K = int(first.k[0])
    host = {x: _host_like(d[x], first.arrays()[x]) for x in names}
    base = model_of_arrays(host["cparent"][:K], host["cbirth"][:K], host["csize"][:K], host["stab"][:K].view(np.float64), host["pc"][:n], host["pw"][:n])
    births = np.sort(base.cluster_birth_w.view(np.float32)[np.isfinite(base.cluster_birth_w.view(np.float32))])
    assert K > 8 and len(births) > 4
    eps = float(np.float32((births[len(births) // 2 - 1] + births[len(births) // 2]) / 2) * np.float32(1.0001))
    assert not (births == np.float32(eps)).any()
    for method, allow, e, max_size in (("eom", True, eps, n // 4), ("eom", False, eps, 0), ("eom", True, 0.0, 0), ("leaf", True, eps, 50)):
        want = select_model(base, method, allow, e, max_size)
        if allow and method == "eom":
            assert root_has_margin(want)
        o = SelectOuts(n + PAD, K + PAD)
        outs = {x: _dev(o.arrays()[x]) for x in OUT_ORDER[:-1]}
        torch.cuda.synchronize()
        rc = native.lib().hnswhds_select_device(0, n, K, *[_ptr(d[x]) for x in ("cparent", "cbirth", "csize", "stab", "pc", "pw")], METHOD_CODE[method],
                                                int(allow), e, max_size, *[_ptr(outs[x]) for x in OUT_ORDER[:-1]], _p(o.l), C.c_void_p(stream.cuda_stream))
        assert rc == 0, native._native.last_error()
        for x in outs:
            o.arrays()[x][:] = _host_like(outs[x], o.arrays()[x])
        compare(o, want, ("composition", method, allow, e, max_size))
    for x in names:                                             # the first stage's arrays are as it wrote them
        assert np.array_equal(_host_like(d[x], first.arrays()[x]), host[x]), x


def test_an_epsilon_that_merges_two_of_three_blobs(native, oracle, tmp_path):
    """three tight blobs of 60 points, two of them near each other, and 20 points on shells around them; knbn = 64 reaches from blob
    to blob, so the forest is one tree.  Hnsw.hdbscan with an eps between the two splits gives two labels, the near blobs under one"""
    rng = np.random.default_rng(0)
    centres = np.zeros((3, 8), np.float32)
    centres[1, 0], centres[2, 1] = 8, 40
    blobs = [c + rng.normal(0, 0.05, (60, 8)) for c in centres]
    dirs = rng.normal(0, 1, (20, 8))
    noise = centres[rng.integers(0, 3, 20)] + dirs / np.linalg.norm(dirs, axis=1)[:, None] * rng.uniform(1, 2, (20, 1))
    ix = Index(native, oracle, tmp_path, np.ascontiguousarray(np.concatenate(blobs + [noise]), np.float32))
    plain = ix.h.hdbscan(10, 64, None, "union", 9)
    assert plain.n_labels == 3 and plain.outlier_scores is None
    chosen = np.flatnonzero(plain.selected)
    births = plain.cluster_birth_w[chosen]
    assert np.isfinite(births).all() and births.min() < births.max(), births    # one tree: the two near blobs split below the far one
    eps = float((births.min() + births.max()) / 2)
    got = ix.h.hdbscan(10, 64, None, "union", 9, cluster_selection_epsilon=eps, outlier_scores=True)
    base = model_of_arrays(plain.cluster_parent, plain.cluster_birth_w.view(np.uint32), plain.cluster_size, plain.stability, plain.point_cluster,
                           plain.point_w.view(np.uint32))
    want = select_model(base, "eom", False, eps)
    assert got.n_labels == want.L == 2 and np.array_equal(got.labels, want.labels) and np.array_equal(got.selected, want.selected.astype(bool))
    assert got.probabilities.tobytes() == want.prob.tobytes() and got.outlier_scores.tobytes() == want.score.tobytes()
    assert got.cluster_death_lambda.tobytes() == want.death.tobytes()
    seen = [set(got.labels[60 * i:60 * i + 60].tolist()) - {-1} for i in range(3)]
    assert all(len(s) == 1 for s in seen) and seen[0] == seen[1] != seen[2], seen
    assert got.forest is plain.forest or got.forest.n_edges == plain.forest.n_edges
    again = plain.select(cluster_selection_epsilon=eps)
    assert np.array_equal(again.labels, got.labels) and again.outlier_scores.tobytes() == got.outlier_scores.tobytes()
    assert np.array_equal(plain.select().labels, plain.labels) and plain.select().probabilities.tobytes() == plain.probabilities.tobytes()
    one = plain.select(allow_single_cluster=True, cluster_selection_epsilon=1e9)    # every climb ends at cluster 0
    assert one.n_labels == 1 and one.selected.tolist() == [True] + [False] * (plain.n_clusters - 1) and (one.labels == 0).all()


# ----------------------------------------------------------------------------------------------------- refusals, threads, a stream
def test_a_malformed_tree_is_an_argument_error_never_a_fault(native):
    """through the device form: the kernels check before anything walks the tree; nothing is written, and the next call works"""
    NN = native._native
    base = forest(*comb(40, 3), 3)
    good = tree_arrays(base)
    K = base.K

    def changed(name, at, value):
        x = good[name].copy()
        x[at] = value
        return {**good, name: x}
    leaf = int(np.flatnonzero([len(k) == 0 for k in base.kids])[-1])
    inner = int(base.cluster_parent[leaf])
    three = changed("parent", K - 1, int(base.cluster_parent[K - 3]))     # a third child there, and one child where it was
    cycle = good["parent"].copy()
    cycle[5], cycle[6] = 6, 5                                    # 5 -> 6 -> 5: refused for parent[5] >= 5, never walked
    bad = {"a parent at c": (changed("parent", 7, 7), "not below c"), "a parent above c": (changed("parent", 3, K - 1), "not below c"),
           "a parent of UINT32_MAX": (changed("parent", 9, 0xFFFFFFFF), "not below c"), "two clusters that name each other": ({**good, "parent": cycle}, "not below c"),
           "parent[0] = 0": (changed("parent", 0, 0), "cluster_parent[0]"), "a point_cluster at K": (changed("pc", 11, K), "point_cluster"),
           "a point_cluster of UINT32_MAX": (changed("pc", 0, 0xFFFFFFFF), "point_cluster"),
           "one child": (changed("parent", leaf, 0) if inner != 0 else three, "one child"), "three children": (three, "more than two"),
           "a NaN stability": (changed("stab", 5, math.nan), "stability"), "a negative stability": (changed("stab", K - 1, -1e-300), "stability"),
           "a stability of -inf at 0": (changed("stab", 0, -INF), "stability")}
    for name, (t, word) in bad.items():
        for method in METHODS:
            rc, o = select_device(native, t, method, True, 2.0, 7)
            assert rc == NN.ERR_ARG and word in NN.last_error(), (name, rc, NN.last_error())
            assert o.untouched(), (name, "written")
    rc, o = select_host(native, bad["three children"][0])
    assert rc == NN.ERR_ARG and o.untouched()
    check(native, base, "the well-formed one, after all that", "eom", True, 2.0, 7, forms=("host", "device"))


def test_two_host_threads_call_at_once(native):
    jobs = {}
    for name, n, mcs, kw in (("a", 3000, 5, dict(allow_single_cluster=True, cluster_selection_epsilon=0.3)), ("b", 700, 3, dict(max_cluster_size=40))):
        rng = np.random.default_rng(n)
        e = path(n)[rng.permutation(n - 1)]
        base = forest(n, e, by_level(n - 1, 128), mcs)
        res = native.HdbscanResult(base.labels, base.prob, base.point_cluster, base.point_w.view(np.float32), base.cluster_parent,
                                   base.cluster_birth_w.view(np.float32), base.cluster_size, base.stability, base.selected.astype(bool), base.K, base.L)
        want = select_model(base, "eom", kw.get("allow_single_cluster", False), kw.get("cluster_selection_epsilon", 0.0), kw.get("max_cluster_size", 0))
        assert sums_exactly(base.stability)
        jobs[name] = (res, kw, want)
    out, errs = {}, []

    def run(name):
        try:
            out[name] = [jobs[name][0].select(**jobs[name][1]) for _ in range(3)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=(name,)) for name in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for name, (_, _, want) in jobs.items():
        for got in out[name]:
            assert got.n_labels == want.L and np.array_equal(got.labels, want.labels) and np.array_equal(got.selected, want.selected.astype(bool)), name
            assert got.probabilities.tobytes() == want.prob.tobytes() and got.outlier_scores.tobytes() == want.score.tobytes()
            assert got.cluster_death_lambda.tobytes() == want.death.tobytes()


def test_device_entry_on_a_stream(native):
    import torch
    n = 3000
    e = path(n)[np.random.default_rng(55).permutation(n - 1)]
    base = forest(n, e, by_level(n - 1, 128), 5)
    t = tree_arrays(base)
    for method in METHODS:
        for allow, eps, max_size in ((False, 0.0, 0), (True, 0.3, 0), (False, 0.3, 100)):
            rc, o = select_device(native, t, method, allow, eps, max_size, stream=torch.cuda.Stream())
            assert rc == 0, native._native.last_error()
            compare(o, select_model(base, method, allow, eps, max_size), ("stream", method, allow, eps, max_size))
