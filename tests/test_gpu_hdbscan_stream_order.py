"""The stream contract of hnswhdb_forest_device and hnswhdb_graph_device with work STILL PENDING on the caller's
stream: the harness, its delay and its two cases (read after write, write after read) are tests/test_gpu_stream_order.py's run_entry,
imported, not restated; the expected answers are hdbscan_model's (tests/test_hdbscan_abi.py) over forests that the suite's models
give, never a call of the entry under test."""
import numpy as np
import pytest

from test_dendrogram_abi import dendrogram, random_forest
from test_gpu_stream_order import (GRAPH_K, GRAPH_MODES, MODE_CODE, N_CSR, SENTINEL, Entry, _check_dendrogram, _check_forest, _index_forest_want,
                                   ix, run_entry)  # noqa: F401  (ix: the module's index fixture)
from test_hdbscan_abi import has_margins, hdbscan_model, max_clusters

pytestmark = pytest.mark.gpu
MCS = 5
PAD = 3


def _outs(n, slots):
    return {"labels": ((n + PAD,), np.int32), "prob": ((n + PAD,), np.uint32), "pc": ((n + PAD,), np.uint32), "pw": ((n + PAD,), np.uint32),
            "cparent": ((slots + PAD,), np.uint32), "cbirth": ((slots + PAD,), np.uint32), "csize": ((slots + PAD,), np.uint32),
            "stab": ((slots + PAD,), np.float64), "sel": ((slots + PAD,), np.uint8)}


ORDER = ("labels", "prob", "pc", "pw", "cparent", "cbirth", "csize", "stab", "sel")


def _check(got, want, counts, exact, what):
    n, K = want.n, want.K
    assert (int(counts[0]), int(counts[1])) == (K, want.L), (what, counts, K, want.L)
    for name, exp, upto in (("labels", want.labels, n), ("prob", want.prob.view(np.uint32), n), ("pc", want.point_cluster, n), ("pw", want.point_w, n),
                            ("cparent", want.cluster_parent, K), ("cbirth", want.cluster_birth_w, K), ("csize", want.cluster_size, K),
                            ("sel", want.selected, K)):
        assert np.array_equal(got[name][:upto], exp), (what, name)
        assert (got[name][upto:].view(np.uint8) == SENTINEL).all(), (what, name, "written behind the answer")
    for c in range(K):
        exp = float(want.stability[c])
        bound = 0.0 if exact else len(want.terms[c]) * 2.0 ** -53 * exp
        assert abs(got["stab"][c] - exp) <= bound, (what, "stability", c, got["stab"][c], exp)
    assert (got["stab"][K:].view(np.uint8) == SENTINEL).all(), (what, "stab", "written behind the answer")


def test_forest_hdbscan(native):
    """two random forests over the same 5000 vertices, cut to the same number of edges, under two sets of ascending weights (powers
    of two: the stabilities are exact)"""
    L = native.lib()
    f1, f2 = random_forest(N_CSR, np.random.default_rng(11)), random_forest(N_CSR, np.random.default_rng(12))
    m = min(len(f1), len(f2))
    f1, f2 = f1[:m], f2[:m]
    a1, b1, a2, b2 = (np.ascontiguousarray(x.astype(np.uint32)) for x in (f1[:, 0], f1[:, 1], f2[:, 0], f2[:, 1]))
    w1, w2 = np.exp2(np.arange(m) // 256 - 4).astype(np.float32), np.exp2(np.arange(m) // 128 - 6).astype(np.float32)
    want, other = hdbscan_model(N_CSR, a1, b1, w1, MCS), hdbscan_model(N_CSR, a2, b2, w2, MCS)
    assert want is not None and other is not None and want.K > 10 and not np.array_equal(want.labels, other.labels)
    counts = np.zeros(2, np.uint64)

    def call(p, sp):
        counts[:] = 0x7777
        return L.hnswhdb_forest_device(0, N_CSR, m, p["a"], p["b"], p["w"], MCS, 0, *[p[x] for x in ORDER], counts[0:1].ctypes.data,
                                               counts[1:2].ctypes.data, sp[0])
    run_entry(native, Entry("forest_hdbscan_device", {"a": (a1, a2), "b": (b1, b2), "w": (w1, w2)}, _outs(N_CSR, max_clusters(N_CSR, MCS)), call,
                            lambda got: _check(got, want, counts, True, "forest hdbscan")))


@pytest.mark.parametrize("ef,mode", GRAPH_MODES)
def test_graph_hdbscan(native, oracle, ix, ef, mode):  # noqa: F811
    L = native.lib()
    want_forest = _index_forest_want(ix, oracle, ef, mode)
    want_dendrogram = dendrogram(ix.n, zip(want_forest[0].tolist(), want_forest[1].tolist()))
    want = hdbscan_model(ix.n, *want_forest, MCS)
    assert want is not None and has_margins(want), "an excess-of-mass decision of the model is too close to a tie: choose another input"
    counts = np.zeros(3, np.uint64)

    def call(p, sp):
        counts[:] = 0x7777
        return L.hnswhdb_graph_device(ix.h.handle, GRAPH_K, ef, MODE_CODE[mode], 0, MCS, 0, p["a"], p["b"], p["w"], p["left"], p["right"], p["size"],
                                              *[p[x] for x in ORDER], counts[0:1].ctypes.data, counts[1:2].ctypes.data, counts[2:3].ctypes.data, sp[0])

    def check(got):
        _check_forest(got, want_forest, int(counts[2]), "index hdbscan, forest")
        _check_dendrogram(got, want_dendrogram, int(counts[2]), "index hdbscan, dendrogram")
        _check(got, want, counts, False, "index hdbscan")
    outs = {"a": ((ix.n - 1,), np.uint32), "b": ((ix.n - 1,), np.uint32), "w": ((ix.n - 1,), np.float32), "left": ((ix.n - 1,), np.uint32),
            "right": ((ix.n - 1,), np.uint32), "size": ((ix.n - 1,), np.uint32)}
    outs.update(_outs(ix.n, max_clusters(ix.n, MCS)))
    run_entry(native, Entry(f"graph_hdbscan_device, ef {ef} {mode}", {}, outs, call, check))
