"""The stream contract of hnswhdp_assign_device and hnswhdp_predict_device with work STILL PENDING on the caller's stream: the
harness, its delay and its two cases (read after write, write after read) are tests/test_gpu_stream_order.py's run_entry, imported,
not restated; the expected answers are predict_model's (tests/test_hdbscan_predict_abi.py), never a call of the entry under test.  The
decoy is the same tree under other point_w and core values: a valid input of the same sizes with another answer."""
import numpy as np
import pytest

from conftest import uniform
from test_gpu_hdbscan_predict import PAD, _bits, clustering_of, core_from_rows, random_rows, random_tree, rows_of_search
from test_gpu_stream_order import SENTINEL, Entry, _dev, run_entry
from test_gpu_symmetric_graph import _uniform_index
from test_hdbscan_predict_abi import TREE_ORDER, PredictOuts, predict_model, tree_args
from test_hdbscan_select_abi import model_of_arrays

pytestmark = pytest.mark.gpu
NAMES = PredictOuts.NAMES
MOVING = ("pw", "core")                                        # produced on the stream; the other arrays are final before the call


def _outs(nq):
    dtypes = dict(zip(NAMES, (np.int32, np.uint32, np.uint32, np.uint32, np.uint32, np.uint32)))
    return {x: ((nq + PAD,), dtypes[x]) for x in NAMES}


def _check(got, want, what):
    nq = len(want.labels)
    exp = {"labels": want.labels, "prob": want.prob.view(np.uint32), "score": want.score.view(np.uint32), "nearest": want.nearest, "w": want.w,
           "cluster": want.cluster}
    for name in NAMES:
        assert np.array_equal(got[name][:nq], exp[name]), (what, name)
        assert (got[name][nq:].view(np.uint8) == SENTINEL).all(), (what, name, "written behind the answer")


def _decoy(base, t):
    """other leaving weights and core distances; the model over them"""
    pw = (t["pw"].view(np.float32) * np.float32(4)).view(np.uint32)
    core = (t["core"].view(np.float32) + np.float32(3)).view(np.uint32)
    other = model_of_arrays(base.cluster_parent, base.cluster_birth_w, base.cluster_size, base.stability, base.point_cluster, pw)
    return pw, core, other


def _fixed(t, cache):
    import torch
    for x, v in t.items():
        if isinstance(v, np.ndarray) and x not in MOVING and x not in cache:
            cache[x] = _dev(_bits(v))
    torch.cuda.synchronize()
    return cache


def test_assign(native):
    L = native.lib()
    base, sel, core = random_tree()
    rows = random_rows(np.random.default_rng(12), 1500, 12, base.n)
    t = tree_args(base, sel, core)
    pw, decoy_core, other = _decoy(base, t)
    want = predict_model(base, sel.selected, 0.0, sel.death, core, *rows, 3)
    wrong = predict_model(other, sel.selected, 0.0, sel.death, decoy_core, *rows, 3)
    assert not np.array_equal(want.cluster, wrong.cluster) and not np.array_equal(want.w, wrong.w)
    cache, r = {}, {}

    def call(p, sp):
        _fixed(t, cache)
        if not r:
            r.update(pos=_dev(rows[0].reshape(-1)), dist=_dev(rows[1].reshape(-1)), counts=_dev(rows[2]))
            import torch
            torch.cuda.synchronize()
        ptr = {**{x: v.data_ptr() for x, v in cache.items()}, **p}
        return L.hnswhdp_assign_device(0, len(rows[2]), 12, r["pos"].data_ptr(), r["dist"].data_ptr(), r["counts"].data_ptr(), 3, base.n,
                                       *[ptr[x] if x in ptr else t[x] for x in TREE_ORDER], *[p[x] for x in NAMES], sp[0])
    ins = {"pw": (t["pw"], pw), "core": (t["core"], decoy_core)}
    run_entry(native, Entry("hdbscan_assign_device", ins, _outs(1500), call, lambda got: _check(got, want, "hdbscan assign")))


@pytest.mark.parametrize("ef", [None, 32])
def test_predict(native, oracle, tmp_path_factory, ef):
    L = native.lib()
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    k, core_k = 16, 3
    _, base, sel = clustering_of(ix, k, ef, core_k, 10)
    core = core_from_rows(ix.D(k, ef)[0], core_k)
    Q = uniform(600, 8, 99)
    rows = rows_of_search(ix, Q, 10, ef)
    t = tree_args(base, sel, core)
    pw, decoy_core, other = _decoy(base, t)
    want = predict_model(base, sel.selected, 0.0, sel.death, core, *rows, core_k)
    wrong = predict_model(other, sel.selected, 0.0, sel.death, decoy_core, *rows, core_k)
    assert not np.array_equal(want.cluster, wrong.cluster) and not np.array_equal(want.w, wrong.w)
    cache, q = {}, {}

    def call(p, sp):
        _fixed(t, cache)
        if not q:
            q.update(q=_dev(Q))
            import torch
            torch.cuda.synchronize()
        ptr = {**{x: v.data_ptr() for x, v in cache.items()}, **p}
        return L.hnswhdp_predict_device(ix.h.handle, q["q"].data_ptr(), 600, 8, 10, 0 if ef is None else ef, core_k,
                                        *[ptr[x] if x in ptr else t[x] for x in TREE_ORDER], *[p[x] for x in NAMES], sp[0])
    ins = {"pw": (t["pw"], pw), "core": (t["core"], decoy_core)}
    run_entry(native, Entry(f"hdbscan_predict_device ef {ef}", ins, _outs(600), call, lambda got: _check(got, want, "hdbscan predict")))
