"""The prediction stage of HDBSCAN on the device (hdbscan_assign -> hnswhdp_assign / _device, Hnsw.core_distances ->
hnswhdp_core_distances / _device, Hnsw.hdbscan_predict -> hnswhdp_predict / _device, csrc/cluster_predict.hip).

The expected answers never come from the code under test: `predict_model` of tests/test_hdbscan_predict_abi.py reads section 2 of the
header over a condensed tree of `hdbscan_model` and a selection of `select_model`, and the index form's rows come from the existing,
separately tested search entries with the positions resolved here.  Every comparison is exact: the integers and the bits of prob, score
and w, with the sentinels behind nq intact; the host form runs twice for equal bytes, the device form once."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

from conftest import uniform
from test_dendrogram_abi import random_forest
from test_gpu_dendrogram import path
from test_gpu_hdbscan import _dev, _host_like, _p, _ptr, by_level, comb
from test_gpu_symmetric_graph import Index, _uniform_index
from test_hdbscan_abi import ORDER, NONE, Model, Outs, balanced_pairs, bits_of, hdbscan_model, max_clusters
from test_hdbscan_predict_abi import (INF_BITS, TREE_ORDER, PredictOuts, assert_blob_property, blob_queries, blobs_and_shell, hand_case, hand_rows,
                                      HAND_CORE, predict_model, tree_args)
from test_hdbscan_select_abi import model_of_arrays, select_model

pytestmark = pytest.mark.gpu
PAD = 3
NAMES = PredictOuts.NAMES
INF = math.inf


# ----------------------------------------------------------------------------------------------------- the two forms
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assign_host(native, t, rows, k, core_k, null=(), n=None):
    """the host entry itself on out arrays at their sentinels: (rc, PredictOuts).  t: tree_args; null: out arrays left out"""
    pos, dist, counts = rows
    nq = len(counts)
    o = PredictOuts(nq + PAD)
    rc = native.lib().hnswhdp_assign(0, nq, k, _p(pos), _p(dist), _p(counts), core_k, len(t["pc"]) if n is None else n,
                                     *[_p(t[x]) if isinstance(t[x], np.ndarray) else t[x] for x in TREE_ORDER],
                                     *[None if x in null else _p(o.arrays()[x]) for x in NAMES])
    return rc, o


def assign_device(native, t, rows, k, core_k, null=(), stream=None):
    """the device entry on tensors at their sentinels: (rc, PredictOuts)"""
    import torch
    nq = len(rows[2])
    o = PredictOuts(nq + PAD)
    ins = {x: _dev(_bits(v)) for x, v in t.items() if isinstance(v, np.ndarray)}
    r = [_dev(x.reshape(-1)) for x in rows]
    d = {x: _dev(o.arrays()[x]) for x in NAMES}
    torch.cuda.synchronize()
    rc = native.lib().hnswhdp_assign_device(0, nq, k, *[_ptr(x) for x in r], core_k, len(t["pc"]),
                                            *[_ptr(ins[x]) if x in ins else t[x] for x in TREE_ORDER],
                                            *[None if x in null else _ptr(d[x]) for x in NAMES],
                                            C.c_void_p(stream.cuda_stream) if stream is not None else None)
    for x, v in ins.items():
        assert np.array_equal(_host_like(v, _bits(t[x])), _bits(t[x])), ("an input was written", x)
    for x, src in zip(r, rows):
        assert np.array_equal(_host_like(x, src), src.reshape(-1)), "a row was written"
    for x in NAMES:
        o.arrays()[x][:] = _host_like(d[x], o.arrays()[x])
    return rc, o


def compare(o, want, what, null=()):
    """the out arrays of a call against the model, exactly; the slots behind nq, and the arrays left out, as they were"""
    nq = len(want.labels)
    exp = {"labels": want.labels, "prob": want.prob.view(np.uint32), "score": None if want.score is None else want.score.view(np.uint32),
           "nearest": want.nearest, "w": want.w, "cluster": want.cluster}
    for name in NAMES:
        got = o.arrays()[name]
        if name in null:
            assert PredictOuts.untouched(o, 0, (name,)), (what, name, "left out, and written")
            continue
        bad = np.flatnonzero(got[:nq] != exp[name])
        assert len(bad) == 0, (what, name, bad[:4], got[bad[:4]], exp[name][bad[:4]])
    assert o.untouched(nq), (what, "behind the answer")


def _bytes(o):
    return b"".join(o.arrays()[x].tobytes() for x in NAMES)


def check(native, base, sel, core, rows, k, core_k, what, eps=0.0, death=True, forms=("host", "host again", "device")):
    """host form (twice: the same bytes) and device form against the model.  Returns the model's answer."""
    want = predict_model(base, sel.selected, eps, sel.death if death else None, core, *rows, core_k)
    t = tree_args(base, sel, core, eps, death)
    null = () if death else ("score",)
    first = None
    for form in forms:
        rc, o = (assign_device if form == "device" else assign_host)(native, t, rows, k, core_k, null)
        assert rc == 0, (what, form, native._native.last_error())
        compare(o, want, (what, form), null)
        if form == "host":
            first = _bytes(o)
        elif form == "host again":
            assert _bytes(o) == first, (what, "two calls differ")
    return want


_TREES = {}


def random_tree(n=300, mcs=3, seed=3):
    """a random forest's condensed tree, its default selection and core distances from the weights' own range: made once, shared"""
    if (n, mcs, seed) not in _TREES:
        rng = np.random.default_rng(seed)
        f = random_forest(n, rng)
        w = np.sort(rng.choice(np.array([0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0], np.float32), len(f)))
        base = hdbscan_model(n, f[:, 0].astype(np.uint32), f[:, 1].astype(np.uint32), w, mcs)
        assert base is not None and base.K > 8
        core = bits_of(rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 2.0], np.float32), n))
        _TREES[(n, mcs, seed)] = (base, select_model(base), core)
    return _TREES[(n, mcs, seed)]


def random_rows(rng, nq, k, n, counts="mixed", values=(0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0, 8.0)):
    """rows with ascending distances from a small set, so that ties between slots are the rule"""
    pos = rng.integers(0, n, (nq, k)).astype(np.uint32)
    dist = np.sort(rng.choice(np.array(values, np.float32), (nq, k)), axis=1)
    if counts == "mixed":
        c = rng.choice(np.array([0, 1, k, max(k // 2, 1)]), nq).astype(np.uint32)
        c[rng.integers(0, nq)] = k
    else:
        c = np.full(nq, counts, np.uint32)
    return pos, np.ascontiguousarray(dist).view(np.uint32), c


# ----------------------------------------------------------------------------------------------------- the assign form
def test_the_hand_made_case(native):
    pos, dist, counts = hand_rows()
    core = bits_of(HAND_CORE)
    for kw, eps in ((dict(), 0.0), (dict(eps=1.5), 1.5)):
        base, sel = hand_case(**kw)
        want = check(native, base, sel, core, (pos, dist, counts), 3, 2, ("hand", kw), eps)
        assert want.cluster.tolist() == [3, 3, 2, 4, 2, 0, 0, 1, 2, 3, 2, 1]
        check(native, base, sel, core, (pos, dist, counts), 3, 0, ("hand, core_k 0", kw), eps, forms=("host", "device"))
    base, sel = hand_case(7, allow_single_cluster=True)
    for eps in (0.0, 4.0):
        want = check(native, base, sel, core, (pos, dist, counts), 3, 2, ("hand, selected {0}", eps), eps)
        assert want.labels.tolist()[11] == (-1 if eps == 0 else 0)


@pytest.mark.parametrize("k", [1, 15, 16, 17, 64, 65])
def test_group_and_block_edges(native, k):
    """a group of 16 lanes less one, one, one more; four and five strides of a group; queries around a wavefront's four groups, a
    block's sixteen and many blocks; counts 0, 1, k and mixed in one batch"""
    base, sel, core = random_tree()
    rng = np.random.default_rng(k)
    for nq in (1, 15, 16, 17, 63, 64, 65, 257):
        forms = ("host", "host again", "device") if nq in (1, 65) else ("host", "device")
        for counts in ("mixed",) if nq not in (17, 64) else ("mixed", 0, 1, k):
            rows = random_rows(rng, nq, k, base.n, counts)
            for core_k in sorted({0, min(2, k), k}) if nq in (16, 65) else (min(2, k),):
                check(native, base, sel, core, rows, k, core_k, f"nq {nq} k {k} counts {counts} core_k {core_k}", forms=forms)


def test_a_climb_through_a_comb_of_depth_199(native):
    """the deepest leaf's points as nearest neighbours, with lambda_q below every birth (the walk ends at cluster 0 after 199 steps),
    between the levels' births, at one of them, and above all"""
    n, e, w = comb(200, 3)
    base = hdbscan_model(n, e[:, 0], e[:, 1], w, 3)
    sel = select_model(base)
    depth_of = [0] * base.K
    for c in range(1, base.K):
        depth_of[c] = depth_of[int(base.cluster_parent[c])] + 1
    deepest = int(np.argmax(depth_of))
    assert depth_of[deepest] >= 199
    members = np.flatnonzero(base.point_cluster == deepest)
    assert len(members)
    ws = [2.0 ** 30, INF, 2.0 ** 24, 3.0 * 2.0 ** 20, 2.0 ** 12, 3.0, 1.0, 0.75, 0.5, 0.25]
    nq, k = len(ws) * len(members), 4
    pos = np.zeros((nq, k), np.uint32)
    dist = np.zeros((nq, k), np.float32)
    for i, x in enumerate(ws):
        for j, v in enumerate(members):
            pos[i * len(members) + j, 0], dist[i * len(members) + j, 0] = v, x
    rows = (pos, dist.view(np.uint32), np.ones(nq, np.uint32))
    core = np.zeros(n, np.uint32)
    want = check(native, base, sel, core, rows, k, 1, "comb")
    assert (want.cluster[:len(members)] == 0).all() and (want.cluster[len(members):2 * len(members)] == 0).all()
    assert len(set(want.cluster.tolist())) >= 5
    for allow, eps in ((True, 0.0), (False, 40.0)):              # other selections over the same tree
        sel2 = select_model(base, "eom", allow, eps)
        check(native, base, sel2, core, rows, k, 0, ("comb", allow, eps), eps, forms=("host", "device"))


def test_a_balanced_cluster_tree_of_256_leaves(native):
    n, a, b, w = balanced_pairs(256)
    base = hdbscan_model(n, a, b, w, 2)
    assert base.K == 511
    rng = np.random.default_rng(256)
    core = bits_of(rng.choice(np.array([0.0, 1.0, 4.0], np.float32), n))
    rows = random_rows(rng, 300, 6, n, values=(0.5, 1.0, 2.0, 4.0, 16.0, 64.0, 256.0, 1024.0))
    for method in ("eom", "leaf"):
        sel = select_model(base, method)
        check(native, base, sel, core, rows, 6, 3, ("balanced pairs", method), forms=("host", "device"))
    sel = select_model(base, "eom", False, 3.0)
    check(native, base, sel, core, rows, 6, 6, "balanced pairs, eps 3", 3.0, forms=("host", "device"))


def test_hostile_values(native):
    """distances and core values 0, -0, +inf and two NaN payloads: the result by the stated order, the surviving bits as they were
    stored; every slot of a row at the same mr: slot 0; core_k = 0 and = k"""
    base, sel, _ = random_tree()
    rng = np.random.default_rng(99)
    hostile = np.array([0, 0x80000000, INF_BITS, 0x7FC00001, 0xFFC12345, 0x3F800000, 0x3E800000, 0xBF800000], np.uint32)
    core = rng.choice(hostile, base.n)
    nq, k = 130, 9
    pos = rng.integers(0, base.n, (nq, k)).astype(np.uint32)
    dist = rng.choice(hostile, (nq, k))
    counts = rng.integers(0, k + 1, nq).astype(np.uint32)
    dist[:20] = np.array(2.0, np.float32).view(np.uint32)       # every slot of these rows at the same mr, above every finite core
    counts[:20] = k
    flat = np.flatnonzero(np.array([order <= 2.0 for order in core.view(np.float32)]))    # (NaN and +inf: False)
    pos[:20] = rng.choice(flat, (20, k))
    for core_k in (0, 1, k):
        want = check(native, base, sel, core, (pos, dist, counts), k, core_k, f"hostile, core_k {core_k}")
        assert (want.nearest[:20] == pos[:20, 0]).all()
    for kw, eps in ((dict(allow_single_cluster=True), 0.0), (dict(eps=INF), INF)):
        sel2 = select_model(base, **kw)
        check(native, base, sel2, core, (pos, dist, counts), k, 1, ("hostile", kw), eps, forms=("host", "device"))


def test_selected_is_the_root_alone_as_the_selection_stage_wrote_it(native):
    """a path: K = 1; hnswhds_select with allow_single_cluster selects cluster 0; the threshold at eps = 0 (maxlambda(0)) and at
    eps > 0 (1 / eps, between two weights and at one)"""
    n = 40
    e, w = path(n), by_level(n - 1, 8)
    for eps in (0.0, 0.09375, 0.125):
        res = native.forest_hdbscan(n, e[:, 0], e[:, 1], w, 5, allow_single_cluster=True, cluster_selection_epsilon=eps)
        assert res.n_clusters == 1 and res.selected.tolist() == [True] and res.cluster_death_lambda is not None
        base = model_of_arrays(res.cluster_parent, res.cluster_birth_w.view(np.uint32), res.cluster_size, res.stability, res.point_cluster,
                               res.point_w.view(np.uint32))
        sel = Model()
        sel.selected, sel.death = res.selected.astype(np.uint8), res.cluster_death_lambda
        rng = np.random.default_rng(40)
        rows = random_rows(rng, 70, 5, n, values=sorted(set(w.tolist())) + [0.09375, 100.0])
        core = np.zeros(n, np.uint32)
        want = check(native, base, sel, core, rows, 5, 2, ("path, selected {0}", eps), eps)
        assert set(want.labels.tolist()) == {0, -1}
        got = native.hdbscan_assign(res, core.view(np.float32), rows[0], rows[1].view(np.float32), rows[2], 2, eps)
        assert np.array_equal(got.labels, want.labels) and got.probabilities.tobytes() == want.prob.tobytes()
        assert got.outlier_scores.tobytes() == want.score.tobytes() and np.array_equal(got.clusters, want.cluster)
        assert np.array_equal(got.nearest, want.nearest) and got.weights.tobytes() == want.w.tobytes()


def test_without_death_and_with_every_optional_output_left_out(native):
    base, sel, core = random_tree()
    rows = random_rows(np.random.default_rng(5), 65, 7, base.n)
    check(native, base, sel, core, rows, 7, 3, "no death", death=False)
    want = predict_model(base, sel.selected, 0.0, sel.death, core, *rows, 3)
    t = tree_args(base, sel, core)
    for null in (("prob",), ("score",), ("nearest",), ("w",), ("cluster",), NAMES[1:]):
        for call in (assign_host, assign_device):
            rc, o = call(native, t, rows, 7, 3, null)
            assert rc == 0, (null, native._native.last_error())
            compare(o, want, (call.__name__, null), null)


def test_a_malformed_input_is_an_argument_error_never_a_fault(native):
    """through the device form, whose kernel makes the checks: ERR_ARG, nothing written, and the next call right"""
    NN = native._native
    base, sel, core = random_tree()
    rows = random_rows(np.random.default_rng(6), 40, 5, base.n)
    good = tree_args(base, sel, core)
    want = predict_model(base, sel.selected, 0.0, sel.death, core, *rows, 2)

    def changed(x, at, value):
        x = x.copy()
        x.reshape(-1)[at] = value
        return x
    used = int(np.flatnonzero(rows[2] > 0)[0])
    two_cycle = good["parent"].copy()
    two_cycle[5], two_cycle[6] = 6, 5
    cases = [("not below c", {"parent": changed(good["parent"], 4, 4)}, rows),
             ("not below c", {"parent": two_cycle}, rows),
             ("cluster_parent[0]", {"parent": changed(good["parent"], 0, 0)}, rows),
             ("point_cluster", {"pc": changed(good["pc"], base.n - 1, base.K)}, rows),
             ("point_cluster", {"pc": changed(good["pc"], 0, NONE)}, rows),
             ("nbr_pos", {}, (changed(rows[0], used * 5, base.n), rows[1], rows[2])),
             ("nbr_pos", {}, (changed(rows[0], used * 5, NONE), rows[1], rows[2])),
             ("counts[q]", {}, (rows[0], rows[1], changed(rows[2], 7, 6))),
             ("counts[q]", {}, (rows[0], rows[1], changed(rows[2], 39, NONE)))]
    for word, kw, r in cases:
        rc, o = assign_device(native, {**good, **kw}, r, 5, 2)
        assert rc == NN.ERR_ARG and word in NN.last_error(), (word, rc, NN.last_error())
        assert o.untouched(), word
        rc, o = assign_device(native, good, rows, 5, 2)
        assert rc == 0
        compare(o, want, ("after", word))
    unused = int(np.flatnonzero(rows[2] < 5)[0])                # a slot behind counts[q] may hold anything
    rc, o = assign_device(native, good, (changed(rows[0], unused * 5 + 4, NONE), rows[1], rows[2]), 5, 2)
    assert rc == 0
    compare(o, want, "an unused slot")


def test_two_host_threads_call_at_once(native):
    base, sel, core = random_tree()
    t = tree_args(base, sel, core)
    jobs = []
    for i in range(2):
        rows = random_rows(np.random.default_rng(70 + i), 257, 16, base.n)
        jobs.append((rows, predict_model(base, sel.selected, 0.0, sel.death, core, *rows, 2)))
    errors = []

    def work(i):
        try:
            rows, want = jobs[i]
            for _ in range(5):
                rc, o = assign_host(native, t, rows, 16, 2)
                assert rc == 0
                compare(o, want, ("thread", i))
        except BaseException as e:                              # noqa: B902 (handed to the main thread)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors


def test_assign_device_entry_on_a_stream(native):
    import torch
    base, sel, core = random_tree()
    rows = random_rows(np.random.default_rng(8), 257, 17, base.n)
    want = predict_model(base, sel.selected, 0.0, sel.death, core, *rows, 4)
    rc, o = assign_device(native, tree_args(base, sel, core), rows, 17, 4, stream=torch.cuda.Stream())
    assert rc == 0
    compare(o, want, "on a stream")


# ----------------------------------------------------------------------------------------------------- core distances
def core_from_rows(res, core_k):
    """the slot of D's rows that the header names, from an existing graph call's answer"""
    c = np.minimum(res.counts.astype(np.int64), core_k)
    bits = np.ascontiguousarray(res.dists).view(np.uint32)
    return np.where(c > 0, bits[np.arange(len(c)), np.maximum(c - 1, 0)], 0).astype(np.uint32)


def core_device(native, ix, k, ef, core_k, stream=None):
    import torch
    out = _dev(np.full(ix.n + PAD, 0xABCD0003, np.uint32))
    torch.cuda.synchronize()
    rc = native.lib().hnswhdp_core_distances_device(ix.h.handle, k, 0 if ef is None else ef, core_k, _ptr(out),
                                                    C.c_void_p(stream.cuda_stream) if stream is not None else None)
    return rc, _host_like(out, np.zeros(1, np.uint32))


@pytest.mark.parametrize("k", [5, 16])
def test_core_distances_are_the_rows_slot(native, oracle, tmp_path_factory, k):
    import torch
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    for ef in (None, 32):
        res, _ = ix.D(k, ef)
        for core_k in (0, 1, k):
            want = core_from_rows(res, core_k)
            got = ix.h.core_distances(k, ef, core_k)
            assert got.dtype == np.float32 and got.view(np.uint32).tolist() == want.tolist(), (k, ef, core_k)
            rc, dev = core_device(native, ix, k, ef, core_k, torch.cuda.Stream() if core_k == 1 else None)
            assert rc == 0 and np.array_equal(dev[:ix.n], want) and (dev[ix.n:] == 0xABCD0003).all(), (k, ef, core_k)
        assert (core_from_rows(res, k) != 0).any()


@pytest.mark.parametrize("n", [1, 2])
def test_core_distances_of_small_indexes(native, oracle, tmp_path, n):
    ix = Index(native, oracle, tmp_path, uniform(n, 8, 10 + n))
    for k, core_k in ((1, 1), (3, 0), (3, 3)):
        for ef in (None, 16):
            res = ix.h.exact_knn_graph_flat(k) if ef is None else ix.h.knn_graph_flat(k, ef)
            want = core_from_rows(res, core_k)
            assert ix.h.core_distances(k, ef, core_k).view(np.uint32).tolist() == want.tolist(), (n, k, ef, core_k)
            rc, dev = core_device(native, ix, k, ef, core_k)
            assert rc == 0 and np.array_equal(dev[:n], want) and (dev[n:] == 0xABCD0003).all()


def test_core_distances_refusals_on_the_device(native, oracle, tmp_path):
    NN = native._native
    cold = Index(native, oracle, tmp_path, uniform(65, 8, 65), upload=False)               # never uploaded
    rc, dev = core_device(native, cold, 3, None, 1)
    assert rc == NN.ERR_DEVICE and "upload" in NN.last_error() and (dev == 0xABCD0003).all()
    for a, word in (((0, None, 0), "knbn must be > 0"), ((3, None, 4), "core_k = 4")):
        rc, dev = core_device(native, cold, *a)
        assert rc == NN.ERR_ARG and word in NN.last_error() and (dev == 0xABCD0003).all()
    assert len(cold.h.core_distances(3, None, 1)) == 65        # the host form uploads on first use


# ----------------------------------------------------------------------------------------------------- the index form
def rows_of_search(ix, Q, k, ef):
    """the rows of the EXISTING search entries, positions resolved with the index's table"""
    res = ix.h.exact_search_flat(Q, k) if ef is None else ix.h.parallel_search_flat(Q, k, ef)
    pos_of_flat, layer_offset = ix.table()[:2]
    pos = pos_of_flat[layer_offset[res.layers.astype(np.int64)] + res.ranks].astype(np.uint32)
    return pos, np.ascontiguousarray(res.dists).view(np.uint32), res.counts.astype(np.uint32)


def predict_host(native, ix, t, Q, k, ef, core_k, null=()):
    nq, d = Q.shape
    o = PredictOuts(nq + PAD)
    rc = native.lib().hnswhdp_predict(ix.h.handle, _p(Q), nq, d, k, 0 if ef is None else ef, core_k,
                                      *[_p(t[x]) if isinstance(t[x], np.ndarray) else t[x] for x in TREE_ORDER],
                                      *[None if x in null else _p(o.arrays()[x]) for x in NAMES])
    return rc, o


def predict_device(native, ix, t, Q, k, ef, core_k, null=(), stream=None, tensors=None):
    """tensors: the tree's arrays where they are in HBM already"""
    import torch
    nq, d = Q.shape
    o = PredictOuts(nq + PAD)
    ins = tensors or {x: _dev(_bits(v)) for x, v in t.items() if isinstance(v, np.ndarray)}
    q = _dev(Q)
    dv = {x: _dev(o.arrays()[x]) for x in NAMES}
    torch.cuda.synchronize()
    rc = native.lib().hnswhdp_predict_device(ix.h.handle, _ptr(q), nq, d, k, 0 if ef is None else ef, core_k,
                                             *[_ptr(ins[x]) if x in ins else t[x] for x in TREE_ORDER],
                                             *[None if x in null else _ptr(dv[x]) for x in NAMES],
                                             C.c_void_p(stream.cuda_stream) if stream is not None else None)
    for x in NAMES:
        o.arrays()[x][:] = _host_like(dv[x], o.arrays()[x])
    return rc, o


def clustering_of(ix, k, ef, core_k, mcs, eps=0.0):
    """the index's clustering through the existing calls, as a model and a selection with death"""
    res = ix.h.hdbscan(mcs, k, ef, "union", core_k, cluster_selection_epsilon=eps, outlier_scores=True)
    base = model_of_arrays(res.cluster_parent, res.cluster_birth_w.view(np.uint32), res.cluster_size, res.stability, res.point_cluster,
                           res.point_w.view(np.uint32))
    sel = Model()
    sel.selected, sel.death = res.selected.astype(np.uint8), res.cluster_death_lambda
    return res, base, sel


@pytest.mark.parametrize("ef", [None, 32])
def test_predict_is_the_search_then_the_assignment(native, oracle, tmp_path_factory, ef):
    import torch
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    k, core_k, mcs = 16, 3, 10
    res, base, sel = clustering_of(ix, k, ef, core_k, mcs)
    assert res.n_labels >= 2 and res.knn_params == (k, ef, core_k)
    core = core_from_rows(ix.D(k, ef)[0], core_k)
    rng = np.random.default_rng(257)
    Q = np.ascontiguousarray(np.concatenate([uniform(200, 8, 4242), ix.X[rng.integers(0, ix.n, 57)] + np.float32(1e-3)]), np.float32)
    for kq in (8, 16):
        rows = rows_of_search(ix, Q, kq, ef)
        want = predict_model(base, sel.selected, 0.0, sel.death, core, *rows, core_k)
        assert len(set(want.labels.tolist())) >= 3 and (want.labels >= 0).sum() >= 20
        t = tree_args(base, sel, core)
        first = None
        for form in ("host", "host again", "device"):
            rc, o = (predict_device(native, ix, t, Q, kq, ef, core_k, stream=torch.cuda.Stream()) if form == "device"
                     else predict_host(native, ix, t, Q, kq, ef, core_k))
            assert rc == 0, (form, native._native.last_error())
            compare(o, want, ("predict", ef, kq, form))
            if form == "host":
                first = o
            elif form == "host again":
                assert b"".join(x.tobytes() for x in first.arrays().values()) == b"".join(x.tobytes() for x in o.arrays().values())
    got = ix.h.hdbscan_predict(res, Q, knbn=16)                 # the Python method: ef and core_k as the clustering ran, core by itself
    assert np.array_equal(got.labels, want.labels) and got.probabilities.tobytes() == want.prob.tobytes()
    assert got.outlier_scores.tobytes() == want.score.tobytes() and got.weights.tobytes() == want.w.tobytes()
    assert np.array_equal(got.nearest, want.nearest) and np.array_equal(got.clusters, want.cluster)
    rc, o = predict_host(native, ix, tree_args(base, sel, core, death=False), Q, 16, ef, core_k, null=("score", "w"))
    assert rc == 0
    compare(o, predict_model(base, sel.selected, 0.0, None, core, *rows, core_k), "no death", null=("score", "w"))


def test_three_stages_compose_in_device_memory(native, oracle, tmp_path_factory):
    """hnswhdb_graph_device -> hnswhds_select_device -> hnswhdp_core_distances_device -> hnswhdp_predict_device on the arrays in HBM:
    the same bytes as the host path"""
    import torch
    NN = native._native
    L = native.lib()
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    k, ef, core_k, mcs, eps = 16, 32, 3, 10, 0.3
    res, base, sel = clustering_of(ix, k, ef, core_k, mcs, eps)
    core = core_from_rows(ix.D(k, ef)[0], core_k)
    Q = uniform(257, 8, 777)
    rc, host = predict_host(native, ix, tree_args(base, sel, core, eps), Q, 12, ef, core_k)
    assert rc == 0, NN.last_error()
    compare(host, predict_model(base, sel.selected, eps, sel.death, core, *rows_of_search(ix, Q, 12, ef), core_k), "host path")
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    n, slots = ix.n, max_clusters(ix.n, mcs)
    o = Outs(n, slots)
    names = ORDER[:-2]
    t = {x: _dev(o.arrays()[x]) for x in names}
    count = np.zeros(1, np.uint64)
    torch.cuda.synchronize()
    rc = L.hnswhdb_graph_device(ix.h.handle, k, ef, 0, core_k, mcs, 0, *[None] * 6, *[_ptr(t[x]) for x in names], _p(o.k), _p(o.l), _p(count), sp)
    assert rc == NN.OK, NN.last_error()
    K = int(o.k[0])
    assert K == base.K
    death, score = _dev(np.zeros(slots, np.uint64)), _dev(np.zeros(n, np.uint32))
    n_labels = np.zeros(1, np.uint64)
    rc = L.hnswhds_select_device(0, n, K, _ptr(t["cparent"]), _ptr(t["cbirth"]), _ptr(t["csize"]), _ptr(t["stab"]), _ptr(t["pc"]), _ptr(t["pw"]),
                                 0, 0, eps, 0, _ptr(t["sel"]), _ptr(t["labels"]), _ptr(t["prob"]), _ptr(score), _ptr(death), _p(n_labels), sp)
    assert rc == NN.OK, NN.last_error()
    d_core = _dev(np.zeros(n, np.uint32))
    assert L.hnswhdp_core_distances_device(ix.h.handle, k, ef, core_k, _ptr(d_core), sp) == NN.OK, NN.last_error()
    tensors = {"core": d_core, "parent": t["cparent"], "birth": t["cbirth"], "pc": t["pc"], "pw": t["pw"], "sel": t["sel"], "death": death}
    scalars = {"K": K, "eps": eps}
    rc, dev = predict_device(native, ix, scalars, Q, 12, ef, core_k, stream=stream, tensors=tensors)
    assert rc == NN.OK, NN.last_error()
    assert b"".join(x.tobytes() for x in dev.arrays().values()) == b"".join(x.tobytes() for x in host.arrays().values())


def test_blob_means_get_their_blobs_labels(native, oracle, tmp_path):
    X = blobs_and_shell()
    ix = Index(native, oracle, tmp_path, X)
    res = ix.h.hdbscan(10, 10, outlier_scores=True)             # core_k = 9, the exact graph
    assert res.n_labels == 3 and res.knn_params == (10, None, 9)
    got = ix.h.hdbscan_predict(res, blob_queries(X))            # knbn = 2 (core_k + 1) = 20
    assert_blob_property(got.labels, got.probabilities, got.outlier_scores, res.labels)
    base = model_of_arrays(res.cluster_parent, res.cluster_birth_w.view(np.uint32), res.cluster_size, res.stability, res.point_cluster,
                           res.point_w.view(np.uint32))
    core = core_from_rows(ix.D(10, None)[0], 9)
    want = predict_model(base, res.selected.astype(np.uint8), 0.0, res.cluster_death_lambda, core, *rows_of_search(ix, blob_queries(X), 20, None), 9)
    assert np.array_equal(got.labels, want.labels) and got.probabilities.tobytes() == want.prob.tobytes()
    assert got.outlier_scores.tobytes() == want.score.tobytes()


def test_an_index_never_uploaded_an_empty_one_and_f16_storage(native, oracle, tmp_path):
    NN = native._native
    cold = Index(native, oracle, tmp_path, native.round_to_f16(uniform(65, 8, 65)), upload=False)    # (rows that f16 storage accepts)
    tree = model_of_arrays([NONE], [INF_BITS], [65], [0.0], [0] * 65, bits_of([1.0] * 65))
    sel = Model()
    sel.selected, sel.death = np.ones(1, np.uint8), np.array([1.0])
    t = tree_args(tree, sel, np.zeros(65, np.uint32))
    Q = uniform(5, 8, 1)
    rc, o = predict_device(native, cold, t, Q, 3, 16, 1)
    assert rc == NN.ERR_DEVICE and "upload" in NN.last_error() and o.untouched()
    cold.h.set_storage("f16")
    for call in (predict_host, predict_device):
        rc, o = call(native, cold, t, Q, 3, 16, 1)
        assert rc == NN.ERR_ARG and "F16" in NN.last_error() and o.untouched()
    cold.h.set_storage("f32")
    rc, o = predict_host(native, cold, t, Q, 3, 16, 1)           # the host form uploads on first use
    assert rc == 0, NN.last_error()
    compare(o, predict_model(tree, sel.selected, 0.0, sel.death, t["core"], *rows_of_search(cold, Q, 3, 16), 1), "first use")
    # no point: every row is empty
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    res = e.hdbscan(5, 5, outlier_scores=True)
    for _ in range(2):                                          # without a handle, then with one that holds no point
        got = e.hdbscan_predict(res, Q)
        assert got.labels.tolist() == [-1] * 5 and got.probabilities.tolist() == [0.0] * 5 and got.outlier_scores.tolist() == [0.0] * 5
        assert got.nearest.tolist() == [NONE] * 5 and got.weights.tolist() == [INF] * 5 and got.clusters.tolist() == [0] * 5
        e.parallel_insert(np.zeros((0, 8), np.float32))
    core = np.full(2, 0x7FC00123, np.uint32)
    assert native.lib().hnswhdp_core_distances(e.handle, 3, 0, 1, _p(core)) == 0 and (core == 0x7FC00123).all()
    empty = Model()
    empty.h = e
    none = {x: None for x in TREE_ORDER}
    rc, o = predict_device(native, empty, {**none, "K": 0, "eps": 0.0}, Q, 3, 16, 1, null=("score",), tensors={})
    assert rc == 0, NN.last_error()
    assert o.labels[:5].tolist() == [-1] * 5 and o.nearest[:5].tolist() == [NONE] * 5 and o.w[:5].tolist() == [INF_BITS] * 5 and o.untouched(5, ("labels", "w"))
