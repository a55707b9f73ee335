"""The stream contract of hnswhds_select_device with work STILL PENDING on the caller's stream: the harness, its delay and its two
cases (read after write, write after read) are tests/test_gpu_stream_order.py's run_entry, imported, not restated, as
tests/test_gpu_hdbscan_stream_order.py does for the first stage; the expected answers are select_model's
(tests/test_hdbscan_select_abi.py) over a condensed tree that hdbscan_model gives, never a call of the entry under test."""
import numpy as np
import pytest

from test_dendrogram_abi import random_forest
from test_gpu_stream_order import N_CSR, SENTINEL, Entry, run_entry
from test_hdbscan_abi import hdbscan_model
from test_hdbscan_select_abi import IN_ORDER, select_model, tree_arrays

pytestmark = pytest.mark.gpu
MCS = 5
PAD = 3
ORDER = ("sel", "labels", "prob", "score", "death")


def _outs(n, K):
    return {"sel": ((K + PAD,), np.uint8), "labels": ((n + PAD,), np.int32), "prob": ((n + PAD,), np.uint32), "score": ((n + PAD,), np.uint32),
            "death": ((K + PAD,), np.uint64)}


def _check(got, want, count, what):
    n, K = want.n, want.K
    assert int(count[0]) == want.L, (what, count, want.L)
    for name, exp, upto in (("sel", want.selected, K), ("labels", want.labels, n), ("prob", want.prob.view(np.uint32), n),
                            ("score", want.score.view(np.uint32), n), ("death", want.death.view(np.uint64), K)):
        assert np.array_equal(got[name][:upto], exp), (what, name)
        assert (got[name][upto:].view(np.uint8) == SENTINEL).all(), (what, name, "written behind the answer")


@pytest.mark.parametrize("method,allow,eps,max_size", [(0, 0, 0.0, 0), (0, 1, 0.3, 200), (1, 1, 0.3, 0)])
def test_select(native, method, allow, eps, max_size):
    """a random forest over 5000 vertices under ascending powers of two (the stabilities are exact).  The decoy is the same tree under
    other stabilities, births and leaving weights: a valid input of the same sizes with another answer.  Those three arrays are
    produced on the stream; the parents, the sizes and the points' clusters are the same in both and final before the call."""
    L = native.lib()
    f = random_forest(N_CSR, np.random.default_rng(11))
    a, b = np.ascontiguousarray(f[:, 0].astype(np.uint32)), np.ascontiguousarray(f[:, 1].astype(np.uint32))
    w = np.exp2(np.arange(len(f)) // 256 - 4).astype(np.float32)
    base = hdbscan_model(N_CSR, a, b, w, MCS)
    assert base is not None and base.K > 10
    true = tree_arrays(base)
    decoy_stab = base.cluster_size.astype(np.float64) ** 2      # every parent wins: the highest clusters are chosen
    decoy_pw = (true["pw"].view(np.float32) * np.float32(4)).view(np.uint32)
    decoy_birth = (true["birth"].view(np.float32) * np.float32(0.5)).view(np.uint32)
    decoy_birth[np.isinf(true["birth"].view(np.float32))] = np.array(1e30, np.float32).view(np.uint32)
    name = "eom" if method == 0 else "leaf"
    want = select_model(base, name, bool(allow), eps, max_size)
    other = select_model(base, name, bool(allow), eps, max_size, decoy_stab)
    assert method == 1 or not np.array_equal(want.labels, other.labels)    # (leaf reads no stability: its decoy shows in prob and score)
    count = np.zeros(1, np.uint64)
    fixed = {}

    def call(p, sp):
        import torch
        from test_gpu_stream_order import _dev
        for x in ("parent", "size", "pc"):                      # (the same in input and decoy: they live outside the harness)
            if x not in fixed:
                fixed[x] = _dev(true[x])
                torch.cuda.synchronize()
        count[:] = 0x7777
        ptr = {**{x: fixed[x].data_ptr() for x in fixed}, **p}
        return L.hnswhds_select_device(0, N_CSR, base.K, *[ptr[x] for x in IN_ORDER], method, allow, eps, max_size, *[p[x] for x in ORDER],
                                       count.ctypes.data, sp[0])
    ins = {"stab": (true["stab"], decoy_stab), "pw": (true["pw"], decoy_pw), "birth": (true["birth"], decoy_birth)}
    run_entry(native, Entry(f"hdbscan_select_device {name} {allow} {eps} {max_size}", ins, _outs(N_CSR, base.K), call,
                            lambda got: _check(got, want, count, "hdbscan select")))
