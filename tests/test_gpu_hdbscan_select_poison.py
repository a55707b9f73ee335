"""hnswhds_select and hnswhds_select_device read no scratch that their own call has not written: both forms under
HNSWGPU_POISON_SCRATCH = 0xFF, 0x5A and 0x01 with the helpers of tests/test_gpu_scratch_poison.py, imported.  Each case runs the
comparison of tests/test_gpu_hdbscan_select.py against select_model with the knob unset and then at the byte, and the answers' bytes
are equal."""
import numpy as np
import pytest

import test_gpu_hdbscan_select as HS
from test_gpu_hdbscan import comb
from test_gpu_scratch_poison import BYTES, _once, _poisoned
from test_hdbscan_abi import balanced_pairs
from test_hdbscan_select_abi import select_model, tree_arrays

pytestmark = pytest.mark.gpu
# every path of the host side: the defaults; the epsilon climb, F and the second doubling; cluster 0 selected; the size test; leaf
OPTIONS = (("eom", False, 0.0, 0), ("eom", True, 96.0, 0), ("eom", False, 3.0, 40), ("leaf", True, 1e9, 0), ("leaf", False, 0.0, 0))


def _case(name):
    if name == "comb":
        base = HS.forest(*comb(200, 3), 3)
    elif name == "balanced pairs":
        n, a, b, w = balanced_pairs(256)
        base = HS.forest(n, np.stack([a, b], 1), w, 2)
    else:                                                       # 300 pairs under cluster 0, which wins: its made-up stability
        base = HS.forest(600, np.stack([np.arange(0, 600, 2), np.arange(1, 600, 2)], 1), np.exp2(np.arange(300) // 64).astype(np.float32), 2)
        base.stability = base.stability.copy()
        base.stability[0] = 1e6
    return base, tree_arrays(base), {o: select_model(base, *o) for o in OPTIONS}


def _rows(native, t, wants, what):
    out = []
    for o in OPTIONS:
        for call in (HS.select_host, HS.select_device):
            rc, got = call(native, t, *o)
            assert rc == 0, (what, o, native._native.last_error())
            HS.compare(got, wants[o], (what, o, call.__name__))
            out.append(HS._bytes(got))
    return out


@pytest.mark.parametrize("byte", BYTES)
@pytest.mark.parametrize("name", ["comb", "balanced pairs", "300 pairs"])
def test_select_under_poisoned_scratch(native, knob, capfd, name, byte):
    base, t, wants = _once(("hdbscan select", name), lambda: _case(name))
    _poisoned(knob, capfd, byte, ("hdbscan select", name), lambda _: _rows(native, t, wants, name))
