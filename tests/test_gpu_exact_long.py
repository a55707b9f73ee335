"""The exact k-NN screen for long rows (csrc/exact_screen_long.hip; hnswxl_exact_search_batch(_device), hnswxl_screen_matrix): queries
and rows both streamed through LDS, d up to 4096.  The cases, their inputs and their assertions are those of
tests/test_gpu_exact_screen_shapes.py, imported; the reference is the CPU oracle's matrix and lexsort, never a device path.

Beyond d = 1120 the bound's error term has the coefficient of DESIGN.md 15.16, restated in `coeff`; `lowest_possible_long` is the
truth moved by twice that term, and the certification condition (fewer than 54 rows outside the answer whose lowest possible bound
reaches the k-th distance) is checked with it on the oracle's matrix, without a device, for every certified case."""
import ctypes as C
import types

import numpy as np
import pytest

import test_gpu_exact_screen_shapes as SH
from test_gpu_exact_knn import _assert_answers
from test_gpu_exact_knn_hostile import N as NH, _assert_hostile, _case
from test_gpu_exact_screen import MARGIN, METRICS, bound_terms, lowest_possible
from test_gpu_scratch_poison import _once, _poisoned, _tmp
from test_gpu_stream_order import Entry, _knn_outs, _res, run_entry

gpu = pytest.mark.gpu
# both sides of the routing at 256, of hnswxs's wave counts (544 | 545) and of its last screened row (1120 | 1121); 1158 = 32 * 36 + 6
DIMS = (257, 545, 784, 1121, 1158, 4096)
CERTIFIED = [(m, d, n, nq) for m in METRICS for d in DIMS for n, nq in SH.SHAPES if n == 700 or d <= 1121]


def coeffs(metric, d):
    """(screen_coeff, screen_coeff_long beyond d = 1120) in units of 2^-24"""
    return {"DistL2": (4 * d + 32, 4 * d + 96), "DistDot": (d + 32, d + 64), "DistCosine": (2 * d + 32, 2 * d + 96)}[metric]


def lowest_possible_long(metric, Q, X):
    d = Q.shape[1]
    if d <= 1120:
        return lowest_possible(metric, Q, X)
    pre, E, finish = bound_terms(metric, Q, X)          # E: with screen_coeff
    short, wide = coeffs(metric, d)
    E = E * (wide / short)
    return finish(pre - 2 * E if metric == "DistL2" else pre + 2 * E)


@pytest.mark.parametrize("metric,d,n,nq", CERTIFIED)
def test_long_rows_can_be_certified(oracle, metric, d, n, nq):
    """no device: the inputs' condition, with the long path's coefficient"""
    case = SH._flat_case(metric, d, n, nq)
    D = SH._known(oracle, case).D
    lb = lowest_possible_long(metric, case.Q, case.X)
    for k in (k for k in SH._ks(n) if k < n):
        kth = np.sort(D, axis=1)[:, k - 1].astype(np.float64)
        worst = int(((lb <= kth[:, None]).sum(1) - k).max())
        assert worst < MARGIN, (metric, d, n, k, worst)


@gpu
@pytest.mark.parametrize("metric,d,n,nq", CERTIFIED)
def test_bit_exact_and_certified(native, oracle, tmp_path, metric, d, n, nq):
    """the oracle's answers byte for byte, p_ids included, every query certified: one slab with a part-filled tile, and five slabs"""
    case = SH._flat_case(metric, d, n, nq)
    h = case.load(native, tmp_path)
    for k in SH._ks(n):
        res, stats = h.exact_search_long_flat(case.Q, k)
        what = f"{metric} d {d} n {n} k {k} stats {stats.tolist()}"
        SH._assert_certified(oracle, case, res, stats, k, what)
        assert stats[1] == 0, what


class _LongMatrix:
    """a case whose handle answers exact_screen_matrix from hnswxl_screen_matrix: what SH._assert_bound then reads"""

    def __init__(self, case):
        self.case, self.metric, self.Q, self.X, self.levels = case, case.metric, case.Q, case.X, case.levels

    def load(self, native, tmp_path):
        h = self.case.load(native, tmp_path)
        h.exact_screen_matrix = h.exact_long_matrix
        return h


@gpu
@pytest.mark.parametrize("d", (1, 130, 784, 1121, 4096))
@pytest.mark.parametrize("metric", METRICS)
def test_the_bound_at_every_length(native, oracle, tmp_path, metric, d):
    """hnswxl_screen_matrix: lb is a number, never -0, never above the oracle's f32 distance, +0 outside the norm range, and on
    in-range inputs not below the truth moved by 2 E -- E with the long coefficient beyond d = 1120"""
    _, _, inside = SH._assert_bound(native, oracle, tmp_path, _LongMatrix(_case(metric, d)), f"long {metric} d {d} hostile", False)
    assert (~inside).any() and inside.any()
    for kind, (X, Q) in SH._bound_inputs(metric, d).items():
        case = SH.Plain(metric, X, Q)
        lb, D, inside = SH._assert_bound(native, oracle, tmp_path, _LongMatrix(case), f"long {metric} d {d} {kind}", d <= 1120)
        floor = lowest_possible_long(metric, case.Q, case.X)
        assert inside.all() and (lb.astype(np.float64) >= floor * (1 - 2.0 ** -22) - 2.0 ** -140).all(), (metric, d, kind, float((floor - lb).max()))


@gpu
@pytest.mark.parametrize("d", (545, 1121))
@pytest.mark.parametrize("metric", METRICS)
def test_hostile_values(native, oracle, tmp_path, metric, d):
    case = _case(metric, d)
    h = case.load(native, tmp_path)
    known = SH._known(oracle, case)
    for k in (1, 10, 300, NH - 1, NH + 5):
        res, stats = h.exact_search_long_flat(case.Q, k)
        assert int(stats.sum()) == len(case.Q) and stats[2] == 0
        _assert_hostile(known, case, res, k, what=f"long {metric} d {d} k {k} stats {stats.tolist()}")


def device_call(native, h, Q, k, allowed=None):
    """hnswxl_exact_search_batch_device on device tensors, null stream: (answers, stats) -- SH.device_call's pattern"""
    import torch
    nq, d = Q.shape
    dq = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
    da = None if allowed is None else torch.from_numpy(np.ascontiguousarray(allowed).view(np.int64)).cuda()
    outs = [torch.full(shape, fill, dtype=t, device="cuda") for shape, fill, t in (((nq, k), -1, torch.int64), ((nq, k), -1.0, torch.float32),
            ((nq, k), 9, torch.uint8), ((nq, k), -1, torch.int32), ((nq,), -1, torch.int32))]
    stats = np.full(3, 99, np.uint64)
    torch.cuda.synchronize()
    rc = native.lib().hnswxl_exact_search_batch_device(h.handle, C.c_void_p(dq.data_ptr()), nq, d, k, None if da is None else C.c_void_p(da.data_ptr()),
                                                       0 if da is None else len(allowed), *(C.c_void_p(o.data_ptr()) for o in outs),
                                                       stats.ctypes.data_as(C.c_void_p), None)
    assert rc == 0, native._native.last_error()
    o = [t.cpu().numpy() for t in outs]
    return types.SimpleNamespace(ids=o[0].view(np.uint64), dists=o[1], layers=o[2], ranks=o[3], counts=o[4].view(np.uint32)), stats


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_routing_and_edges(native, oracle, tmp_path, metric):
    """d = 256: the resident screen's bytes and stats.  d = 4097: not screened, the oracle's answers, the matrix refuses.  d = 545,
    nq = 256: two whole tiles"""
    case = SH._flat_case(metric, 256, 700, 37)
    h = case.load(native, tmp_path)
    for k in (10, 705):
        (a, sa), (b, sb) = h.exact_search_long_flat(case.Q, k), h.exact_search_screened_flat(case.Q, k)
        assert sa.tolist() == sb.tolist() == [37, 0, 0]
        assert all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in ("ids", "dists", "layers", "ranks", "counts"))
    case = SH.Flat(metric, 4097, 700, 37)
    h = case.load(native, tmp_path)
    res, stats = h.exact_search_long_flat(case.Q, 10)
    assert stats.tolist() == [0, 0, 37], stats
    _assert_answers(SH._known(oracle, case), metric, res, case.Q, case.X, case.ids, 10, what=f"{metric} d 4097")
    with pytest.raises(native.HnswError, match="rows too long") as err:
        h.exact_long_matrix(case.Q)
    assert err.value.code == native._native.ERR_ARG
    case = SH.Flat(metric, 545, 700, 256)
    h = case.load(native, tmp_path)
    for k in (1, 100):
        res, stats = h.exact_search_long_flat(case.Q, k)
        SH._assert_certified(oracle, case, res, stats, k, f"{metric} two whole tiles k {k} stats {stats.tolist()}")
        assert stats[1] == 0


def _filtered_crowd(metric, n=700):
    case = SH.copies_case(metric, n=n, d=545)
    rows = np.sort(np.concatenate([case.copies, np.random.default_rng(12).choice(np.setdiff1d(np.arange(n), case.copies), 100, replace=False)]))
    return case, rows


def _both_calls(native, case, h, rows, known):
    """host and _device entry under the filter: the oracle's answers, the queries next to the copies fall back"""
    out, allowed = [], np.sort(case.ids[rows])
    for call in ("host", "device"):
        res, stats = h.exact_search_long_flat(case.Q, 10, allowed) if call == "host" else device_call(native, h, case.Q, 10, allowed)
        what = f"long {case.metric} {call} filter of {len(rows)}, stats {stats.tolist()}"
        _assert_answers(known, case.metric, res, case.Q, case.X, case.ids, 10, rows, what=what)
        assert stats[1] >= 1 and stats[0] >= 1 and stats[2] == 0 and int(stats.sum()) == len(case.Q), what
        out += [res.ids, res.dists, res.layers, res.ranks, res.counts, stats]
    return out


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_a_fallback_under_a_filter(native, oracle, tmp_path, metric):
    case, rows = _filtered_crowd(metric)
    _both_calls(native, case, case.load(native, tmp_path), rows, SH._known(oracle, case))


@gpu
def test_under_poisoned_scratch(native, oracle, tmp_path_factory, knob, capfd):
    """the style of tests/test_gpu_exact_screen_poison.py at d = 545, n = 2500 (three slabs), scratch filled with 0xFF: certified and
    fallen-back queries of both entries, and the matrix"""
    def make():
        case, rows = _filtered_crowd("DistL2", n=2500)
        return case, case.load(native, _tmp(tmp_path_factory, "long"), "long"), rows, SH._known(oracle, case)

    def run(_):
        case, h, rows, known = made
        lb = h.exact_long_matrix(case.Q)
        assert (lb <= known.D[:, np.asarray(SH.dump_order(case.levels)[0])]).all() and (lb > 0).any()
        return _both_calls(native, case, h, rows, known) + [lb]
    made = _once(("long", "made"), make)
    _poisoned(knob, capfd, 0xFF, ("long", "d545"), run)


@gpu
def test_the_device_entry_behind_a_delayed_producer(native, oracle, tmp_path):
    """the style of tests/test_gpu_exact_screen_stream_order.py: run_entry's two cases on a caller's stream, with fallbacks"""
    case = SH.copies_case("DistL2", n=3000, d=545)
    h = case.load(native, tmp_path, "order")
    known, L, (nq, d), stats = SH._known(oracle, case), native.lib(), case.Q.shape, np.zeros(3, np.uint64)

    def call(p, sp):
        stats[:] = 99
        return L.hnswxl_exact_search_batch_device(h.handle, p["q"], nq, d, 10, None, 0, p["ids"], p["dists"], p["layers"], p["ranks"], p["counts"],
                                                  stats.ctypes.data_as(C.c_void_p), sp[0])

    def check(got):
        _assert_answers(known, case.metric, _res(got, nq, 10), case.Q, case.X, case.ids, 10, what=f"long, stream order, stats {stats.tolist()}")
        assert int(stats.sum()) == nq and stats[2] == 0 and stats[1] >= 1, stats
    run_entry(native, Entry("hnswxl_exact_search_batch_device", {"q": (case.Q, np.ascontiguousarray(case.Q[::-1]))}, _knn_outs(nq, 10), call, check))
