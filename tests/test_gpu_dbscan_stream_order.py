"""The stream contract of hnswdbs_exact_device and hnswdbs_csr_device with work STILL PENDING on the caller's stream: the harness,
its delay and its two cases (read after write, write after read) are tests/test_gpu_stream_order.py's run_entry, imported, not
restated; the expected answers are dbscan_model's (tests/test_dbscan_abi.py), never a call of the entry under test.  The exact form
has no device input besides the index: its case is write after read.  The CSR form's decoy is the same graph under other distances:
a valid input of the same sizes with another answer."""
import numpy as np
import pytest

from conftest import uniform
from test_dbscan_abi import dbscan_model, sets_of_csr
from test_gpu_dbscan import DTYPES, NAMES, PAD, Dump, csr_of_matrix
from test_gpu_stream_order import SENTINEL, Entry, run_entry

pytestmark = pytest.mark.gpu


def _outs(n):
    return {x: ((n + PAD,), DTYPES[x]) for x in NAMES}


def _check(got, want, what):
    n = len(want.labels)
    exp = {"label": want.labels, "core": want.core, "count": want.counts, "anchor": want.anchors}
    for x in NAMES:
        assert np.array_equal(got[x][:n], exp[x]), (what, x)
        assert (got[x][n:].view(np.uint8) == SENTINEL).all(), (what, x, "written behind the answer")


@pytest.fixture(scope="module")
def index(native, oracle, tmp_path_factory):
    n = 3000
    ix = Dump(native, oracle, tmp_path_factory.mktemp("order"), uniform(n, 8, 41), np.random.default_rng(41).permutation(n).astype(np.uint64) * 3 + 5, "DistL2")
    return ix, np.sort(ix.Dp[0])[5]


def test_exact(native, index):
    L = native.lib()
    ix, eps = index
    want = ix.want(eps, 5)
    assert want.n_clusters >= 2
    c = np.zeros(1, np.uint64)

    def call(p, sp):
        return L.hnswdbs_exact_device(ix.h.handle, float(eps), 5, *[p[x] for x in NAMES], c.ctypes.data, sp[0])

    def check(got):
        _check(got, want, "dbscan exact")
        assert int(c[0]) == want.n_clusters
    run_entry(native, Entry("dbscan_exact_device", {}, _outs(ix.n), call, check))


def test_csr(native, index):
    L = native.lib()
    ix, eps = index
    offs, cols, dists = csr_of_matrix(ix.Dp, np.sort(ix.Dp[0])[12], 3)
    decoy = (dists * np.float32(0.5)).astype(np.float32)
    want = dbscan_model(sets_of_csr(offs, cols, dists, eps), 5)
    wrong = dbscan_model(sets_of_csr(offs, cols, decoy, eps), 5)
    assert not np.array_equal(want.labels, wrong.labels) and not np.array_equal(want.counts, wrong.counts)
    n = ix.n
    c = np.zeros(1, np.uint64)

    def call(p, sp):
        return L.hnswdbs_csr_device(0, n, p["offsets"], p["cols"], p["dists"], float(eps), 5, 0, *[p[x] for x in NAMES], c.ctypes.data, sp[0])

    def check(got):
        _check(got, want, "dbscan csr")
        assert int(c[0]) == want.n_clusters
    ins = {"dists": (dists, decoy), "cols": (cols, np.roll(cols, 1)), "offsets": (offs, np.minimum(offs, offs[-1] // 2))}
    run_entry(native, Entry("dbscan_csr_device", ins, _outs(n), call, check))
