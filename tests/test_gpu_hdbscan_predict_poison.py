"""hnswhdp_assign, hnswhdp_predict, hnswhdp_core_distances and their _device forms read no scratch that their own call has not
written: under HNSWGPU_POISON_SCRATCH = 0xFF, 0x5A and 0x01 with the helpers of tests/test_gpu_scratch_poison.py, imported.  Each case
runs the comparison of tests/test_gpu_hdbscan_predict.py against predict_model with the knob unset and then at the byte, and the
answers' bytes are equal."""
import numpy as np
import pytest

import test_gpu_hdbscan_predict as HP
from test_gpu_hdbscan import comb
from test_gpu_scratch_poison import BYTES, _once, _poisoned
from test_gpu_symmetric_graph import _uniform_index
from test_hdbscan_abi import hdbscan_model
from test_hdbscan_predict_abi import predict_model, tree_args
from test_hdbscan_select_abi import select_model

pytestmark = pytest.mark.gpu


def _assign_case(name):
    if name == "comb":                                          # every round of the doubling; selected {0} besides
        n, e, w = comb(200, 3)
        base = hdbscan_model(n, e[:, 0], e[:, 1], w, 3)
        core = np.zeros(n, np.uint32)
        sels = [(select_model(base), 0.0), (select_model(base, "eom", True, 1e9), 1e9)]
    else:
        base, sel, core = HP.random_tree()
        sels = [(sel, 0.0), (select_model(base, "leaf"), 0.0)]
    rows = HP.random_rows(np.random.default_rng(31), 257, 17, base.n)
    return base, core, rows, [(s, eps, predict_model(base, s.selected, eps, s.death, core, *rows, 3)) for s, eps in sels]


def _assign_rows(native, base, core, rows, sels, what):
    out = []
    for sel, eps, want in sels:
        t = tree_args(base, sel, core, eps)
        for call in (HP.assign_host, HP.assign_device):
            rc, got = call(native, t, rows, 17, 3)
            assert rc == 0, (what, native._native.last_error())
            HP.compare(got, want, (what, eps, call.__name__))
            out.append(HP._bytes(got))
    return out


@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("name", ["comb", "random tree"])
def test_assign_under_poisoned_scratch(native, knob, capfd, name, byte):
    base, core, rows, sels = _once(("hdbscan predict", name), lambda: _assign_case(name))
    _poisoned(knob, capfd, byte, ("hdbscan predict", name), lambda _: _assign_rows(native, base, core, rows, sels, name))


def _index_case(native, ix, ef):
    k, core_k = 16, 3
    _, base, sel = HP.clustering_of(ix, k, ef, core_k, 10)
    core = HP.core_from_rows(ix.D(k, ef)[0], core_k)
    Q = HP.uniform(257, 8, 5)
    want = predict_model(base, sel.selected, 0.0, sel.death, core, *HP.rows_of_search(ix, Q, 10, ef), core_k)
    return base, sel, core, Q, want


def _index_rows(native, ix, ef, case):
    base, sel, core, Q, want = case
    out = []
    got = ix.h.core_distances(16, ef, 3)
    assert np.array_equal(got.view(np.uint32), core)
    out.append(got.tobytes())
    rc, dev = HP.core_device(native, ix, 16, ef, 3)
    assert rc == 0 and np.array_equal(dev[:ix.n], core)
    out.append(dev.tobytes())
    t = tree_args(base, sel, core)
    for call in (HP.predict_host, HP.predict_device):
        rc, o = call(native, ix, t, Q, 10, ef, 3)
        assert rc == 0, native._native.last_error()
        HP.compare(o, want, ("predict", ef, call.__name__))
        out.append(HP._bytes(o))
    return out


@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("ef", [None, 32])
def test_index_forms_under_poisoned_scratch(native, oracle, tmp_path_factory, knob, capfd, ef, byte):
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    case = _once(("hdbscan predict index", ef), lambda: _index_case(native, ix, ef))
    _poisoned(knob, capfd, byte, ("hdbscan predict index", ef), lambda _: _index_rows(native, ix, ef, case))
