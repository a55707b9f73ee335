"""Exact range search behind the matrix-core screen (csrc/exact_range_screen.hip, include/hnsw_mi355x_exact_range_screen.h): the
answers are the CPU oracle's distance matrix cut at the radius and lexsorted (_expected / _assert_range of test_gpu_exact_range),
byte for byte, never the existing device path's; stats say which path answered.  Hand-written dumps, but for the built index of
test_gpu_exact_range."""
import ctypes as C

import numpy as np
import pytest

from conftest import uniform
from dump_writer import write_dump
from test_gpu_exact_knn_hostile import _case
from test_gpu_exact_range import INF, _assert_range, _built_case, _cycled_radii, _expected, _median_radii, _p
from test_gpu_exact_screen import DIMS, METRICS, SHAPES, _benign
from test_gpu_scratch_poison import BYTES, _poisoned
from test_gpu_stream_order import Entry, _csr_outs, _untouched_behind, ix, run_entry  # noqa: F401 (ix: a fixture)

pytestmark = pytest.mark.gpu
CAND_CAP = 2 << 20   # RS_CAND_CAP of exact_range_screen.hip, the smaller default capacity


def _load(native, tmp_path, metric, X, ids=None, name="rs"):
    ids = np.arange(len(X), dtype=np.uint64) if ids is None else ids
    levels = np.zeros(len(X), np.int64)
    levels[::17], levels[::190] = 1, 2
    _, pids = write_dump(tmp_path, name, X, ids, levels, metric)
    h = native.HnswIo(tmp_path, name).load_hnsw(metric)
    h.upload(0)
    return h, ids, pids


def _radii(D):
    """per query in turn: the distance to row q % 100 (which has an exact copy: a tie on the boundary), the next f32 below it, 0, -0,
    -1, +inf, NaN"""
    r = np.zeros(len(D), np.float32)
    for q in range(len(D)):
        at = D[q, q % 100]
        r[q] = (at, np.nextafter(at, -INF), 0.0, -0.0, -1.0, INF, np.nan)[q % 7]
    return r


def _device(native, h, Q, radii, cap, allowed=None, count_only=False):
    import torch
    nq, d = Q.shape
    dev = [torch.from_numpy(a).cuda() for a in (Q, radii)] + [torch.from_numpy(allowed.astype(np.int64)).cuda() if allowed is not None else None]
    outs = [torch.full((n,), -1, dtype=t, device="cuda") for n, t in ((nq + 1, torch.int64), (cap + 1, torch.int64), (cap + 1, torch.float32),
                                                                       (cap + 1, torch.uint8), (cap + 1, torch.int32))]
    ptr = [C.c_void_p(t.data_ptr()) if t is not None else None for t in dev + outs]
    stats = np.full(3, 99, np.uint64)
    torch.cuda.synchronize()
    rc = native.lib().hnswxr_exact_range_search_batch_device(h.handle, ptr[0], nq, d, ptr[1], ptr[2], 0 if allowed is None else len(allowed), cap, ptr[3],
                                                              *([None] * 4 if count_only else ptr[4:]), _p(stats), None)
    off, ids, dd, ll, rr = [t.cpu().numpy() for t in outs]
    total = min(int(off[-1]), cap)
    return rc, native.RangeResult(off.astype(np.uint64), ids[:total].astype(np.uint64), dd[:total], ll[:total], rr[:total]), stats


def _same(a, b):
    return (np.array_equal(a.offsets, b.offsets) and np.array_equal(a.ids, b.ids) and np.array_equal(a.dists.view(np.uint32), b.dists.view(np.uint32))
            and np.array_equal(a.layers, b.layers) and np.array_equal(a.ranks, b.ranks))


def _both_forms(native, h, Q, radii, D, ids, pids, want_stats, what, rows=None):
    """the host form twice and the device form: the oracle's answer, equal bytes, the stats"""
    allowed = None if rows is None else np.sort(ids[rows])
    res, stats = h.exact_range_search_screened_flat(Q, radii, allowed)
    offsets, _ = _assert_range(res, D, ids, radii, rows, pids=pids, what=what + f" stats {stats.tolist()}")
    assert stats.tolist() == list(want_stats), (what, stats)
    again, _ = h.exact_range_search_screened_flat(Q, radii, allowed)
    rc, dev, dstats = _device(native, h, Q, radii, int(offsets[-1]), allowed)
    assert rc == 0 and dstats.tolist() == list(want_stats), (what, rc, dstats)
    assert _same(again, res) and _same(dev, res), what
    return res


@pytest.mark.parametrize("n,nq", SHAPES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_bit_exact(native, oracle, tmp_path, metric, d, n, nq):
    assert nq * n < CAND_CAP                      # the condition of stats == (nq, 0, 0): not even every pair outgrows a buffer
    X, Q = _benign(metric, n, d, 300 + d), _benign(metric, nq, d, 400 + d)
    X[n - 100:] = X[:100]                         # planted exact copies
    Q[:3] = X[5:8]
    h, ids, pids = _load(native, tmp_path, metric, X)
    D = oracle.dist_matrix(metric, Q, X)
    radii = _radii(D)
    with np.errstate(invalid="ignore"):
        assert any((D[q] == radii[q]).sum() >= 2 for q in range(0, nq, 7)), "no radius on a tie"
    _both_forms(native, h, Q, radii, D, ids, pids, (nq, 0, 0), f"{metric} d {d} n {n}")


@pytest.mark.parametrize("d", (250, 260, 540, 550, 1100, 1125))   # dpad 256 / 288, 544 / 576, 1120 / 1152: four, two, one wavefront, none
@pytest.mark.parametrize("metric", METRICS)
def test_lds_boundaries(native, oracle, tmp_path, metric, d):
    n, nq = 300, 70
    X, Q = _benign(metric, n, d, 500 + d), _benign(metric, nq, d, 600 + d)
    X[n - 100:] = X[:100]
    h, ids, pids = _load(native, tmp_path, metric, X)
    D = oracle.dist_matrix(metric, Q, X)
    _both_forms(native, h, Q, _radii(D), D, ids, pids, (0, 0, nq) if d > 1120 else (nq, 0, 0), f"{metric} d {d}")


@pytest.mark.parametrize("d", (33, 128))
@pytest.mark.parametrize("metric", METRICS)
def test_hostile_rows(native, oracle, tmp_path, metric, d):
    """NaN, +-inf, +-0, +-FLT_MAX, norms outside [2^-40, 2^40]: the pairs outside the proved range are candidates for every radius
    >= -0 and the exact chain decides them"""
    case = _case(metric, d)
    h = case.load(native, tmp_path)
    D = oracle.dist_matrix(metric, case.Q, case.X)
    nq = len(case.Q)
    for name, radii in (("+inf", np.full(nq, INF, np.float32)), ("median", _median_radii(D)), ("0", np.zeros(nq, np.float32))):
        res = _both_forms(native, h, case.Q, radii, D, case.ids, case.pids, (nq, 0, 0), f"{metric} d {d} radius {name}")
        assert not np.isnan(res.dists).any() and not (res.dists.view(np.uint32) == 0x80000000).any(), name


@pytest.fixture(scope="module")
def built(native, oracle):
    """test_gpu_exact_range's built index (DistL2, d = 33, n = 2500, 37 queries, every kind of radius) and 300 more queries: three
    tiles of 128"""
    h, X, Q, ids, D, radii, _ = _built_case(native, oracle, "DistL2", 33)
    Q3 = uniform(300, 33, 77)
    D3 = oracle.dist_matrix("DistL2", Q3, X)
    return h, X, Q, ids, D, radii, Q3, D3, _cycled_radii(D3)[0]


def test_filter(native, built):
    h, X, Q, ids, D, radii = built[:6]
    rows = np.sort(np.random.default_rng(13).choice(len(X), 900, replace=False))
    _both_forms(native, h, Q, radii, D, ids, None, (len(Q), 0, 0), "filter", rows)


def _raw(native, h, Q, radii, cap, screened, with_out=True):
    nq, d = Q.shape
    offs = np.full(nq + 1, 0x5A5A5A5A, np.uint64)
    outs = [np.full(max(cap, 1) * w, 0xA5, np.uint8) for w in (8, 4, 1, 4)]
    ptrs = [_p(o) if with_out else None for o in outs]
    L = native.lib()
    if screened:
        rc = L.hnswxr_exact_range_search_batch(h.handle, _p(Q), nq, d, _p(radii), None, 0, cap, _p(offs), *ptrs, None)
    else:
        rc = L.hnswgpu_exact_range_search_batch(h.handle, _p(Q), nq, d, _p(radii), None, 0, cap, _p(offs), *ptrs)
    return rc, native._native.last_error(), offs, outs


def test_capacity_rule(native, built):
    h, X, Q, ids, D, radii = built[:6]
    N = native._native
    offsets, want = _expected(D, ids, radii)
    total = int(offsets[-1])
    rc, msg, offs, outs = _raw(native, h, Q, radii, total - 1, True)
    assert rc == N.ERR_CAPACITY and msg == _raw(native, h, Q, radii, total - 1, False)[1] and str(total) in msg, (rc, msg)
    assert np.array_equal(offs, offsets) and all((o == 0xA5).all() for o in outs)      # complete offsets, no out slot touched
    rc, msg, offs, outs = _raw(native, h, Q, radii, 0, True, with_out=False)           # count only
    assert rc == N.ERR_CAPACITY and np.array_equal(offs, offsets) and msg == _raw(native, h, Q, radii, 0, False, with_out=False)[1]
    rc, _, offs, _ = _raw(native, h, Q, np.full(len(Q), -1.0, np.float32), 0, True, with_out=False)
    assert rc == N.OK and not offs.any()
    rc, _, offs, outs = _raw(native, h, Q, radii, total, True)
    assert rc == N.OK and np.array_equal(offs, offsets) and np.array_equal(outs[0].view(np.uint64), np.concatenate([ids[w] for w in want]))


def test_capacity_hook_falls_back(native, built, knob):
    h, X, Q, ids, D, radii = built[:6]
    base, stats = h.exact_range_search_screened_flat(Q, radii)
    offsets, _ = _assert_range(base, D, ids, radii, what="unhooked")
    assert stats.tolist() == [len(Q), 0, 0] and int(np.diff(offsets).max()) == len(X)
    for cap in (len(X) // 50, int(offsets[-1]) // 3):        # below one query's candidates; about a third of the answers
        knob("HNSWGPU_RANGE_SCREEN_CAP", cap)
        res, stats = h.exact_range_search_screened_flat(Q, radii)
        assert _same(res, base) and stats.tolist() == [0, len(Q), 0], (cap, stats)
    knob("HNSWGPU_RANGE_SCREEN_CAP", None)


def test_key_buffer_outgrown(native, built, knob):
    """one tile per chunk and a capacity between a chunk's candidates and the call's answers: no chunk outgrows the candidate
    buffer, the answers outgrow the key buffer (the scatter drops what does not fit, the total tells).  The condition: a chunk's
    candidates are its pairs with bound <= radius, at most those with oracle distance <= radius (1 + 2^-10) (the bound of
    DESIGN.md 15.13 is closer than that at d = 33)"""
    h, X, _, ids, _, _, Q3, D3, r3 = built
    base, stats = h.exact_range_search_screened_flat(Q3, r3)
    _assert_range(base, D3, ids, r3, what="unhooked")
    with np.errstate(invalid="ignore"):
        near = (D3 <= (r3 * np.float32(1 + 2.0 ** -10))[:, None]).sum(1)
    cap = (int(max(near[a:a + 128].sum() for a in (0, 128, 256))) + len(base.ids)) // 2
    assert stats.tolist() == [300, 0, 0] and max(near[a:a + 128].sum() for a in (0, 128, 256)) < cap < len(base.ids)
    knob("HNSWGPU_RANGE_SCREEN_TILES", 1)
    knob("HNSWGPU_RANGE_SCREEN_CAP", cap)
    res, stats = h.exact_range_search_screened_flat(Q3, r3)
    assert _same(res, base) and stats.tolist() == [0, 300, 0], stats
    knob("HNSWGPU_RANGE_SCREEN_CAP", None)
    knob("HNSWGPU_RANGE_SCREEN_TILES", None)


def test_one_tile_per_chunk(native, built, knob):
    h, X, _, ids, _, _, Q3, D3, r3 = built
    knob("HNSWGPU_RANGE_SCREEN_TILES", 1)
    _both_forms(native, h, Q3, r3, D3, ids, None, (len(Q3), 0, 0), "three chunks")     # (the offsets carry from chunk to chunk)
    knob("HNSWGPU_RANGE_SCREEN_TILES", None)


@pytest.mark.parametrize("metric,n", (("DistL1", 700), ("DistL2", 255)))
def test_not_screened(native, oracle, tmp_path, metric, n):
    X, Q = uniform(n, 30, 21), uniform(37, 30, 22)
    X[n - 100:] = X[:100]
    h, ids, pids = _load(native, tmp_path, metric, X)
    D = oracle.dist_matrix(metric, Q, X)
    _both_forms(native, h, Q, _radii(D), D, ids, pids, (0, 0, 37), f"{metric} n {n}")


@pytest.mark.parametrize("byte", BYTES)
def test_poisoned_scratch(native, built, knob, capfd, byte):
    h, X, _, ids, _, _, Q3, D3, r3 = built
    rows = np.sort(np.random.default_rng(5).choice(len(X), 1200, replace=False))

    def run(_):
        res = _both_forms(native, h, Q3, r3, D3, ids, None, (len(Q3), 0, 0), "poison", rows)
        return [res.offsets, res.ids, res.dists, res.layers, res.ranks]
    _poisoned(knob, capfd, byte, ("range screen", "filter"), run)


def test_stream_contract(native, oracle, ix):
    """queries, radii and the filter arrive late on the caller's stream (run_entry of test_gpu_stream_order and its fixture)"""
    L = native.lib()
    D = oracle.dist_matrix(ix.metric, ix.Q, ix.X)
    cap = ix.nq * len(ix.allowed)
    stats = np.zeros(3, np.uint64)

    def call(p, sp):
        return L.hnswxr_exact_range_search_batch_device(ix.h.handle, p["q"], ix.nq, ix.d, p["radii"], p["allowed"], len(ix.allowed), cap, p["offsets"], p["ids"],
                                                        p["dists"], p["layers"], p["ranks"], _p(stats), sp[0])

    def check(got):
        total = int(got["offsets"][-1])
        res = native.RangeResult(got["offsets"], got["ids"][:total], got["dists"][:total], got["layers"][:total], got["ranks"][:total])
        _assert_range(res, D, ix.ids, ix.radii, rows=ix.allowed.astype(np.int64), pids=ix.pids, what="screened exact range")
        _untouched_behind(got, total)
        assert stats.tolist() == [ix.nq, 0, 0]
    ins = {"q": (ix.Q, np.ascontiguousarray(ix.Q[::-1])), "radii": (ix.radii, ix.radii_decoy), "allowed": (ix.allowed, ix.allowed_decoy)}
    run_entry(native, Entry("hnswxr_exact_range_search_batch_device", ins, _csr_outs(ix.nq, cap, False), call, check))
