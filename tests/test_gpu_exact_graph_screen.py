"""The exact k-NN graph of the stored points behind the matrix-core screen (hnswxg_*; the SELF variants of csrc/exact_screen.hip and
csrc/exact_screen_long.hip).  References: the CPU oracle's matrix ordered over the OTHER points (test_gpu_knn_graph._exact_expected)
and the existing exact_knn_graph_flat, byte for byte.  Inputs, shims and assertions are those of tests/test_gpu_exact_screen_shapes.py
and its siblings, imported; the certification condition is checked on the oracle's matrix without a device."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_exact_screen_shapes as SH
from dump_writer import dump_order
from test_gpu_exact_knn_hostile import N as NH, _case
from test_gpu_exact_long import lowest_possible_long
from test_gpu_exact_screen import MARGIN, METRICS, _benign
from test_gpu_knn_graph import _assert_rows, _exact_expected, _outside_the_cosine_domain
from test_gpu_scratch_poison import _once, _poisoned, _tmp
from test_gpu_stream_order import Entry, _knn_outs, _res, run_entry

gpu = pytest.mark.gpu
FIELDS = ("ids", "dists", "layers", "ranks", "counts")
# d: 30 puts a DistCosine norm into the row's last chunk, 256 | 257 are the two sides of the routing, 1121 has the long coefficient;
# n: 700 is one slab and six tiles, the last of 60 points; 2500 three slabs, the last of 452 rows, and a last tile of 68
CERTIFIED = [(m, d, n) for m in METRICS for d in (3, 30, 128, 256, 257, 1121) for n in (700, 2500)]


def _same(a, b):
    return all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in FIELDS)


def _graph_case(oracle, metric, d, n):
    """SH.Flat's index (ids = rows: row i of a NULL point_ids answer is point i) and the oracle's n x n matrix, kept on the case"""
    case = SH._flat_case(metric, d, n, 1)
    if getattr(case, "D", None) is None:
        case.D = oracle.dist_matrix(metric, case.X, case.X)
    return case


@pytest.mark.parametrize("metric,d,n", CERTIFIED)
def test_stored_points_can_be_certified(oracle, metric, d, n):
    """no device: fewer than 54 OTHER points have a lowest possible bound at or below a point's k-th distance"""
    case = _graph_case(oracle, metric, d, n)
    other = ~np.eye(n, dtype=bool)
    lb = lowest_possible_long(metric, case.X, case.X)
    by_distance = np.sort(np.where(other, case.D, np.inf), axis=1)
    for k in (k for k in SH._ks(n) if k < n):
        assert int((((lb <= by_distance[:, k - 1:k]) & other).sum(1) - k).max()) < MARGIN, (metric, d, n, k)


@gpu
@pytest.mark.parametrize("metric,d,n", CERTIFIED)
def test_bit_exact_and_certified(native, oracle, tmp_path, metric, d, n):
    case = _graph_case(oracle, metric, d, n)
    h = case.load(native, tmp_path)
    pos = np.empty(n, np.int64)
    pos[np.asarray(dump_order(case.levels)[0])] = np.arange(n)
    want = _exact_expected(case.D, case.ids, pos, case.pids, np.arange(n), max(SH._ks(n)))   # a smaller k: its prefix
    for k in SH._ks(n):
        res, stats = h.exact_knn_graph_screened_flat(k)
        what = f"{metric} d {d} n {n} k {k} stats {stats.tolist()}"
        assert _same(res, h.exact_knn_graph_flat(k)) and stats.tolist() == [n, 0, 0], what
        _assert_rows(res, [w[:, :k] for w in want[:4]] + [np.minimum(want[4], k)], what)
        assert not res.ids[:, n - 1:].any() and not res.dists[:, n - 1:].view(np.uint32).any(), what


def _crowd_case(metric, n=680, d=30):
    """80 exact copies of one row under ids of their own, three points per DataId elsewhere; a filter that holds every copy and every
    second other id; the points named: every copy, 60 other ids on both sides of the filter, ten of them twice, shuffled.  A copy
    sees 79 others at bound +0 against lists of 64 keys: its row must fall back"""
    rng = np.random.default_rng(21)
    X = _benign(metric, n, d, 22)
    copies = rng.choice(n, 80, replace=False)
    X[copies] = X[copies[0]]
    case = SH.Plain(metric, X, X[:1], seed=23)
    case.ids = np.empty(n, np.uint64)
    case.ids[copies] = 1000 + np.arange(80, dtype=np.uint64)
    case.ids[np.setdiff1d(np.arange(n), copies)] = rng.permutation(n - 80).astype(np.uint64) // 3
    case.allowed = np.unique(np.concatenate([case.ids[copies], np.arange(0, 200, 2, dtype=np.uint64)]))
    named = np.concatenate([case.ids[copies], np.arange(70, 130, dtype=np.uint64)])
    case.named = rng.permutation(np.concatenate([named, named[75:85]]))
    return case


def _crowd(native, factory, metric):
    def make():
        case = _crowd_case(metric)
        h = case.load(native, _tmp(factory, "graph_screen" + metric))
        return case, h, h.exact_knn_graph_flat(10, case.named, case.allowed)
    return _once(("graph_screen", metric), make)


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_identity_and_fallback_through_both_entries(native, tmp_path_factory, metric):
    """the existing call's bytes -- copies and same-id points are answers, the point itself never, allowed or not --, every copy's row
    through the fallback into its own slot of the shuffled batch; the device entry behind a delayed producer on a caller's stream
    (tests/test_gpu_exact_screen_stream_order.py's style)"""
    import torch
    case, h, old = _crowd(native, tmp_path_factory, metric)
    m, stats = len(case.named), np.zeros(3, np.uint64)
    res, host_stats = h.exact_knn_graph_screened_flat(10, case.named, case.allowed)
    assert _same(res, old) and host_stats[1] >= 80 and host_stats[2] == 0 and int(host_stats.sum()) == m, (metric, host_stats)
    allowed = torch.from_numpy(case.allowed.view(np.int64)).cuda()

    def call(p, sp):
        stats[:] = 99
        return native.lib().hnswxg_exact_graph_batch_device(h.handle, p["pts"], m, 10, C.c_void_p(allowed.data_ptr()), len(case.allowed), p["ids"], p["dists"],
                                                            p["layers"], p["ranks"], p["counts"], stats.ctypes.data_as(C.c_void_p), sp[0])

    def check(got):
        assert _same(_res(got, m, 10), old) and stats.tolist() == host_stats.tolist(), stats
    run_entry(native, Entry("hnswxg_exact_graph_batch_device", {"pts": (case.named, np.ascontiguousarray(case.named[::-1]))}, _knn_outs(m, 10), call, check))


@gpu
def test_under_poisoned_scratch(native, tmp_path_factory, knob, capfd):
    """certified and fallen-back points of the host entry, and the matrix, with every scratch block filled with 0xFF first"""
    case, h, old = _crowd(native, tmp_path_factory, "DistL2")

    def run(_):
        res, stats = h.exact_knn_graph_screened_flat(10, case.named, case.allowed)
        assert _same(res, old) and stats[1] >= 80 and stats[0] >= 1, stats
        return [getattr(res, f) for f in FIELDS] + [stats, h.exact_graph_screen_matrix(case.named)]
    _poisoned(knob, capfd, 0xFF, ("graph_screen", "crowd"), run)


@gpu
@pytest.mark.parametrize("d", (25, 545))
@pytest.mark.parametrize("metric", METRICS)
def test_hostile_values(native, tmp_path, metric, d):
    """zero rows, overflowing norms, NaN / +-inf as points of the graph: the existing call's bytes whatever falls back"""
    h = _case(metric, d).load(native, tmp_path)
    for k in (1, 10, NH - 1, NH + 5):
        res, stats = h.exact_knn_graph_screened_flat(k)
        assert _same(res, h.exact_knn_graph_flat(k)) and int(stats.sum()) == NH and stats[2] == 0, (metric, d, k, stats)


class _SelfMatrix:
    """a case whose handle answers exact_screen_matrix from hnswxg_screen_matrix for 150 named rows (two tiles, shuffled, `first`
    among them, `never` not): what SH._assert_bound then reads, the named rows being its queries"""

    def __init__(self, case, first=(), never=()):
        rest = np.random.default_rng(31).permutation(np.setdiff1d(np.arange(case.X.shape[0]), np.concatenate([first, never]).astype(np.int64)))
        self.rows = np.random.default_rng(32).permutation(np.concatenate([np.asarray(first, np.int64), rest[:150 - len(first)]]))
        self.case, self.metric, self.X, self.levels, self.Q = case, case.metric, case.X, case.levels, case.X[self.rows]

    def load(self, native, tmp_path):
        h = self.case.load(native, tmp_path)
        h.exact_screen_matrix = lambda Q: h.exact_graph_screen_matrix(self.case.ids[self.rows])
        return h


@gpu
@pytest.mark.parametrize("d", (1, 130, 256, 257, 1121, 4096))
@pytest.mark.parametrize("metric", METRICS)
def test_the_bound_with_rows_as_queries(native, oracle, tmp_path, metric, d):
    """hnswxg_screen_matrix: never above the oracle's f32 distance, the own pair included; +0 outside the norm range; on in-range
    inputs not below the truth moved by 2 E (the long coefficient beyond d = 1120)"""
    hostile = _case(metric, d)
    # (DistCosine: the reference defines no distance where a hostile row cancels against itself or another -- such rows are no queries)
    undefined = hostile.hostile[_outside_the_cosine_domain(hostile.X[hostile.hostile])] if metric == "DistCosine" else np.zeros(0, np.int64)
    named = _SelfMatrix(hostile, np.setdiff1d(hostile.hostile, undefined), undefined)
    _, _, inside = SH._assert_bound(native, oracle, tmp_path, named, f"graph {metric} d {d} hostile", False)
    assert (~inside).any() and inside.any()
    for kind, (X, _) in SH._bound_inputs(metric, d).items():
        case = _SelfMatrix(SH.Plain(metric, X, X[:1]))
        lb, _, inside = SH._assert_bound(native, oracle, tmp_path, case, f"graph {metric} d {d} {kind}", d <= 1120)
        floor = lowest_possible_long(metric, case.Q, case.X)
        assert inside.all() and (lb.astype(np.float64) >= floor * (1 - 2.0 ** -22) - 2.0 ** -140).all(), (metric, d, kind, float((floor - lb).max()))
        assert metric != "DistL2" or not lb[np.arange(150), case.rows].view(np.uint32).any(), (metric, d, kind, "a point's own pair must carry +0")


@gpu
@pytest.mark.parametrize("metric,d,n,k", [("DistL2", 30, 255, 10), ("DistL1", 30, 700, 10), ("DistL2", 30, 700, 4043), ("DistL2", 4097, 700, 10),
                                          ("DistL2", 30, 1, 10)])
def test_not_screened(native, tmp_path, metric, d, n, k):
    """fewer than 256 points (one: no answer), a distance without a screen, lists above 4096 keys, rows above 4096 elements"""
    h = SH.Flat(metric, d, n, 1).load(native, tmp_path)
    res, stats = h.exact_knn_graph_screened_flat(k)
    assert stats.tolist() == [0, 0, n] and _same(res, h.exact_knn_graph_flat(k)) and res.counts.tolist() == [min(k, n - 1)] * n


@gpu
def test_no_point_named_and_an_unknown_id(native, tmp_path):
    h = SH.Flat("DistL2", 30, 700, 1).load(native, tmp_path)
    res, stats = h.exact_knn_graph_screened_flat(10, np.zeros(0, np.uint64))
    assert res.counts.shape == (0,) and stats.tolist() == [0, 0, 0]
    pts = np.array([3, 700, 5, 9999], np.uint64)
    outs = [np.full((4, 10), 7, t) for t in (np.uint64, np.float32, np.uint8, np.int32)] + [np.full(4, 7, np.uint32), np.full(3, 7, np.uint64)]
    rc = native.lib().hnswxg_exact_graph_batch(h.handle, pts.ctypes.data_as(C.c_void_p), 4, 10, None, 0, *(o.ctypes.data_as(C.c_void_p) for o in outs))
    assert rc == native._native.ERR_ARG and "2 of the 4 point_ids name no point" in native._native.last_error()
    assert all((o == 7).all() for o in outs)
    with pytest.raises(native.HnswError, match="2 of the 4 point_ids"):
        h.exact_graph_screen_matrix(pts)
