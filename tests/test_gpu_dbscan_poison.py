"""hnswdbs_exact, hnswdbs_csr and their _device forms read no scratch that their own call has not written: under
HNSWGPU_POISON_SCRATCH = 0xFF, 0x5A and 0x01 with the helpers of tests/test_gpu_scratch_poison.py, imported.  Each case runs the
comparison of tests/test_gpu_dbscan.py against dbscan_model with the knob unset and then at the byte, and the answers' bytes are
equal."""
import numpy as np
import pytest

import test_gpu_dbscan as DB
from conftest import uniform
from test_dbscan_abi import dbscan_model, sets_of_csr
from test_gpu_scratch_poison import BYTES, _once, _poisoned, _tmp

pytestmark = pytest.mark.gpu


def _case(native, oracle, tmp_path_factory):
    n = 1000                                                    # no multiple of 64, four slabs, a part-filled last tile
    ix = DB.Dump(native, oracle, _tmp(tmp_path_factory, "dbscan"), uniform(n, 5, 51), np.random.default_rng(51).permutation(n).astype(np.uint64) + 2, "DistL2")
    eps = np.sort(ix.Dp[0])[5]
    want = ix.want(eps, 4)
    assert want.n_clusters >= 2 and min(DB._kinds(want)) >= 1
    csr = DB.csr_of_matrix(ix.Dp, np.sort(ix.Dp[0])[9], 4)
    return ix, eps, want, csr, dbscan_model(sets_of_csr(*csr, eps), 4, 1)


def _rows(native, case):
    ix, eps, want, csr, want_csr = case
    out = []
    for call in (DB.exact_host, DB.exact_device):
        rc, got, c = call(native, ix.h, ix.n, eps, 4)
        DB.compare(rc, got, c, want, call.__name__)
        out.append(DB._bytes(got))
    for call in (DB.csr_host, DB.csr_device):
        rc, got, c = call(native, *csr, eps, 4, 1)
        DB.compare(rc, got, c, want_csr, call.__name__)
        out.append(DB._bytes(got))
    return out


@pytest.mark.parametrize("byte", BYTES)
def test_dbscan_under_poisoned_scratch(native, oracle, tmp_path_factory, knob, capfd, byte):
    case = _once(("dbscan",), lambda: _case(native, oracle, tmp_path_factory))
    _poisoned(knob, capfd, byte, ("dbscan",), lambda _: _rows(native, case))
