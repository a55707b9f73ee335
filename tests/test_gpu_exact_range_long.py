"""Exact range search behind the streamed screen for long rows (csrc/exact_range_screen_long.hip,
include/hnsw_mi355x_exact_range_long.h): the answers are the CPU oracle's distance matrix cut at the radius and lexsorted
(_expected / _assert_range of test_gpu_exact_range), byte for byte, never a device path's; stats say which path answered.  Inputs,
radii and assertions are those of test_gpu_exact_range_screen and test_gpu_exact_long."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_exact_screen_shapes as SH
from test_gpu_exact_knn_hostile import _case
from test_gpu_exact_range import INF, _assert_range, _expected, _median_radii, _p
from test_gpu_exact_range_screen import CAND_CAP, _load, _radii, _same
from test_gpu_exact_screen import METRICS, _benign
from test_gpu_scratch_poison import _poisoned
from test_gpu_stream_order import Entry, _csr_outs, _untouched_behind, run_entry

pytestmark = pytest.mark.gpu
ENTRY = "hnswxrl_exact_range_search_batch"


def _device(native, h, Q, radii, cap, allowed=None):
    """hnswxrl_exact_range_search_batch_device on device tensors, null stream"""
    import torch
    nq, d = Q.shape
    dev = [torch.from_numpy(a).cuda() for a in (Q, radii)] + [torch.from_numpy(allowed.astype(np.int64)).cuda() if allowed is not None else None]
    outs = [torch.full((n,), -1, dtype=t, device="cuda") for n, t in ((nq + 1, torch.int64), (cap + 1, torch.int64), (cap + 1, torch.float32),
                                                                       (cap + 1, torch.uint8), (cap + 1, torch.int32))]
    ptr = [C.c_void_p(t.data_ptr()) if t is not None else None for t in dev + outs]
    stats = np.full(3, 99, np.uint64)
    torch.cuda.synchronize()
    rc = getattr(native.lib(), ENTRY + "_device")(h.handle, ptr[0], nq, d, ptr[1], ptr[2], 0 if allowed is None else len(allowed), cap, *ptr[3:], _p(stats), None)
    off, ids, dd, ll, rr = [t.cpu().numpy() for t in outs]
    total = min(int(off[-1]), cap)
    return rc, native.RangeResult(off.astype(np.uint64), ids[:total].astype(np.uint64), dd[:total], ll[:total], rr[:total]), stats


def _both_forms(native, h, Q, radii, D, ids, pids, want_stats, what, rows=None):
    """the host form twice and the device form: the oracle's answer, equal bytes, the stats"""
    assert Q.shape[0] * D.shape[1] < CAND_CAP        # the condition of stats == (nq, 0, 0): not even every pair outgrows a buffer
    allowed = None if rows is None else np.sort(ids[rows])
    res, stats = h.exact_range_search_long_flat(Q, radii, allowed)
    offsets, _ = _assert_range(res, D, ids, radii, rows, pids=pids, what=what + f" stats {stats.tolist()}")
    assert stats.tolist() == list(want_stats), (what, stats)
    again, _ = h.exact_range_search_long_flat(Q, radii, allowed)
    rc, dev, dstats = _device(native, h, Q, radii, int(offsets[-1]), allowed)
    assert rc == 0 and dstats.tolist() == list(want_stats), (what, rc, dstats)
    assert _same(again, res) and _same(dev, res), what
    return res


def _planted(metric, d, n, nq):
    X, Q = _benign(metric, n, d, 300 + d), _benign(metric, nq, d, 400 + d)
    X[n - 100:] = X[:100]                         # planted exact copies
    Q[:3] = X[5:8]
    return X, Q


# d: both sides of the routing (257) and of the coefficient switch (1121), d % 32 != 0 and d % 8 != 0, the last length; the larger shape
# (several slabs, whole and part-filled tiles) up to d = 1121, the cut of test_gpu_exact_long for the oracle's time
@pytest.mark.parametrize("d,n,nq", [(d, n, nq) for d in (257, 545, 784, 1121, 1158, 4096) for n, nq in ((700, 37), (5000, 150)) if n == 700 or d <= 1121])
@pytest.mark.parametrize("metric", METRICS)
def test_bit_exact(native, oracle, tmp_path, metric, d, n, nq):
    X, Q = _planted(metric, d, n, nq)
    h, ids, pids = _load(native, tmp_path, metric, X)
    D = oracle.dist_matrix(metric, Q, X)
    radii = _radii(D)
    with np.errstate(invalid="ignore"):
        assert any((D[q] == radii[q]).sum() >= 2 for q in range(0, nq, 7)), "no radius on a tie"
    _both_forms(native, h, Q, radii, D, ids, pids, (nq, 0, 0), f"{metric} d {d} n {n}")


@pytest.mark.parametrize("d", (784, 4096))
@pytest.mark.parametrize("metric", METRICS)
def test_complete_where_rounding_is_worst(native, oracle, tmp_path, metric, d):
    """every query's radius is exactly its oracle distance to one row: a bound or a coefficient that is not sound loses that row"""
    for kind, (X, Q) in SH._bound_inputs(metric, d).items():
        h, ids, pids = _load(native, tmp_path, metric, X, name="b" + str(len(kind)))
        D = oracle.dist_matrix(metric, Q, X)
        radii = D[np.arange(len(Q)), (np.arange(len(Q)) * 19 + 3) % len(X)].copy()
        _both_forms(native, h, Q, radii, D, ids, pids, (len(Q), 0, 0), f"{metric} d {d} {kind}")


@pytest.mark.parametrize("metric", METRICS)
def test_routing_and_edges(native, oracle, tmp_path, metric):
    """d = 256: the resident screen's bytes and stats.  d = 4097: not screened.  d = 545: two whole tiles; one filter"""
    X, Q = _planted(metric, 256, 700, 37)
    h, ids, pids = _load(native, tmp_path, metric, X, name="r256")
    D = oracle.dist_matrix(metric, Q, X)
    res = _both_forms(native, h, Q, _radii(D), D, ids, pids, (37, 0, 0), f"{metric} d 256")
    old, old_stats = h.exact_range_search_screened_flat(Q, _radii(D))
    assert _same(res, old) and old_stats.tolist() == [37, 0, 0]
    X, Q = _planted(metric, 4097, 300, 37)
    h, ids, pids = _load(native, tmp_path, metric, X, name="r4097")
    D = oracle.dist_matrix(metric, Q, X)
    _both_forms(native, h, Q, _radii(D), D, ids, pids, (0, 0, 37), f"{metric} d 4097")
    X, Q = _planted(metric, 545, 700, 256)
    h, ids, pids = _load(native, tmp_path, metric, X, name="r545")
    D = oracle.dist_matrix(metric, Q, X)
    _both_forms(native, h, Q, _radii(D), D, ids, pids, (256, 0, 0), f"{metric} two whole tiles")
    rows = np.sort(np.random.default_rng(13).choice(700, 250, replace=False))
    _both_forms(native, h, Q[:37], _radii(D[:37]), D[:37], ids, pids, (37, 0, 0), f"{metric} filter", rows)


@pytest.mark.parametrize("metric", METRICS)
def test_hostile_rows(native, oracle, tmp_path, metric):
    """NaN, +-inf, +-0, +-FLT_MAX, norms outside [2^-40, 2^40]: the pairs outside the proved range are candidates for every radius
    >= -0 and the exact chain decides them"""
    case = _case(metric, 545)
    h = case.load(native, tmp_path)
    D = oracle.dist_matrix(metric, case.Q, case.X)
    nq = len(case.Q)
    for name, radii in (("+inf", np.full(nq, INF, np.float32)), ("median", _median_radii(D)), ("0", np.zeros(nq, np.float32))):
        res = _both_forms(native, h, case.Q, radii, D, case.ids, case.pids, (nq, 0, 0), f"{metric} radius {name}")
        assert not np.isnan(res.dists).any() and not (res.dists.view(np.uint32) == 0x80000000).any(), name


@pytest.fixture(scope="module")
def d300(native, oracle, tmp_path_factory):
    """DistL2, d = 300, n = 700, 300 queries: three tiles of 128"""
    X, Q = _planted("DistL2", 300, 700, 300)
    h, ids, pids = _load(native, tmp_path_factory.mktemp("d300"), "DistL2", X)
    D = oracle.dist_matrix("DistL2", Q, X)
    return h, Q, ids, pids, D, _radii(D)


def test_fallback_and_chunks(native, d300, knob):
    h, Q, ids, pids, D, radii = d300
    base = _both_forms(native, h, Q, radii, D, ids, pids, (300, 0, 0), "unhooked")
    knob("HNSWGPU_RANGE_SCREEN_CAP", 700 // 50)            # below one query's candidates (a radius of +inf has 700)
    res, stats = h.exact_range_search_long_flat(Q, radii)
    knob("HNSWGPU_RANGE_SCREEN_CAP", None)
    assert _same(res, base) and stats.tolist() == [0, 300, 0], stats
    knob("HNSWGPU_RANGE_SCREEN_TILES", 1)
    _both_forms(native, h, Q, radii, D, ids, pids, (300, 0, 0), "three chunks")     # (the offsets carry from chunk to chunk)
    knob("HNSWGPU_RANGE_SCREEN_TILES", None)


def test_capacity_rule(native, d300):
    h, Q, ids, _, D, radii = d300
    N, L = native._native, native.lib()
    offsets, _ = _expected(D, ids, radii)
    total = int(offsets[-1])

    def raw(name, cap, with_out, *tail):
        offs = np.full(len(Q) + 1, 0x5A5A5A5A, np.uint64)
        outs = [np.full(max(cap, 1) * w, 0xA5, np.uint8) for w in (8, 4, 1, 4)]
        rc = getattr(L, name)(h.handle, _p(Q), len(Q), 300, _p(radii), None, 0, cap, _p(offs), *[_p(o) if with_out else None for o in outs], *tail)
        return rc, N.last_error(), offs, outs
    for cap, with_out in ((total - 1, True), (0, False)):          # one slot short; count only
        rc, msg, offs, outs = raw(ENTRY, cap, with_out, None)
        assert rc == N.ERR_CAPACITY and msg == raw("hnswgpu_exact_range_search_batch", cap, with_out)[1] and str(total) in msg, (rc, msg)
        assert np.array_equal(offs, offsets) and all((o == 0xA5).all() for o in outs)      # complete offsets, no out slot touched


def test_poisoned_scratch(native, d300, knob, capfd):
    h, Q, ids, pids, D, radii = d300
    rows = np.sort(np.random.default_rng(5).choice(700, 300, replace=False))

    def run(_):
        res = _both_forms(native, h, Q, radii, D, ids, pids, (300, 0, 0), "poison", rows)
        return [res.offsets, res.ids, res.dists, res.layers, res.ranks]
    _poisoned(knob, capfd, 0xFF, ("range screen long", "filter"), run)


def test_stream_contract(native, oracle, tmp_path):
    """queries and radii arrive late on the caller's stream (run_entry of test_gpu_stream_order); cap = every pair, so that no mix of
    true and decoy inputs can ask for more"""
    X, Q = _planted("DistL2", 545, 700, 37)
    h, ids, pids = _load(native, tmp_path, "DistL2", X)
    D = oracle.dist_matrix("DistL2", Q, X)
    radii, cap, stats = _radii(D), 37 * 700, np.zeros(3, np.uint64)

    def call(p, sp):
        return getattr(native.lib(), ENTRY + "_device")(h.handle, p["q"], 37, 545, p["radii"], None, 0, cap, p["offsets"], p["ids"], p["dists"], p["layers"],
                                                        p["ranks"], _p(stats), sp[0])

    def check(got):
        total = int(got["offsets"][-1])
        res = native.RangeResult(got["offsets"], got["ids"][:total], got["dists"][:total], got["layers"][:total], got["ranks"][:total])
        _assert_range(res, D, ids, radii, pids=pids, what="streamed range screen")
        _untouched_behind(got, total)
        assert stats.tolist() == [37, 0, 0]
    ins = {"q": (Q, np.ascontiguousarray(Q[::-1])), "radii": (radii, np.full(37, INF, np.float32))}
    run_entry(native, Entry(ENTRY + "_device", ins, _csr_outs(37, cap, False), call, check))
