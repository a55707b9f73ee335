"""Exact DBSCAN behind the two-sided matrix-core screen (hnswxd_exact / _device, hnswxd_bounds_matrix, csrc/dbscan_screen.hip).

References, never the code under test: the CPU oracle's f32 distance matrix of the rows against themselves fed to `dbscan_model` of
tests/test_dbscan_abi.py (through `Dump` of tests/test_gpu_dbscan.py: indexes written by hand, positions known), and beside it the
bytes of hnswdbs_exact on the same index.  Every comparison is exact.  What an input must contain for a case to mean anything is
asserted on the MODEL."""
import ctypes as C

import numpy as np
import pytest

from conftest import uniform
from dump_writer import dump_order
from test_gpu_dbscan import (CLUSTERS, DTYPES, FLT_MAX, INF, NAMES, PAD, Dump, _bytes, _fresh, _kinds, _p, blob_data, compare,
                             exact_device, exact_host, hostile_rows)
from test_gpu_stream_order import _dev, _host, _sentinel

pytestmark = pytest.mark.gpu
SCREENED = ("DistL2", "DistCosine", "DistDot")


def screened_host(native, h, n, eps, ms):
    o, c, st = _fresh(n), np.full(1, CLUSTERS, np.uint64), np.full(4, 7, np.uint64)
    rc = native.lib().hnswxd_exact(h.handle, float(eps), ms, *[_p(o[x]) for x in NAMES], _p(c), _p(st))
    return rc, o, int(c[0]), st.tolist()


def screened_device(native, h, n, eps, ms, stream=None):
    import torch
    o, c, st = {x: _dev(_sentinel((n + PAD,), DTYPES[x])) for x in NAMES}, np.full(1, CLUSTERS, np.uint64), np.full(4, 7, np.uint64)
    torch.cuda.synchronize()
    rc = native.lib().hnswxd_exact_device(h.handle, float(eps), ms, *[C.c_void_p(o[x].data_ptr()) for x in NAMES], _p(c), _p(st),
                                          C.c_void_p(stream.cuda_stream) if stream is not None else None)
    torch.cuda.synchronize()
    return rc, {x: _host(o[x], DTYPES[x]) for x in NAMES}, int(c[0]), st.tolist()


def rows_of(metric, d, n):
    """n rows of tests/test_gpu_dbscan.py's blob_data(metric, d): equal parts of four to ten blobs, close pairs of centres among them
    (blobs b and b + 6), more than 40 rows each at every n; an eighth uniform rows; 10 exact copies under their original's DataId; 10
    rows that share a DataId with a blob row without being its copy."""
    X, ids = blob_data(metric, d)
    rows, nb = n - n // 8 - 20, max(4, -(-(n - n // 8 - 20) // 200))
    blob = np.concatenate([200 * b + np.arange(-(-rows // nb)) for b in (0, 6, 1, 7, 2, 8, 3, 9, 4, 10)[:nb]])[:rows]
    take = np.concatenate([blob, 2400 + np.arange(n // 8 + 10)])
    X, ids = np.concatenate([X[take], X[take[:10]]]), np.concatenate([ids[take], ids[take[:10]]])
    ids[n - 20:n - 10] = ids[20:30]
    assert len(X) == n
    return X, ids


def eps_at(ix, ms):
    """a value OF D: the max(ms, 3)-th smallest distance of data row 0, a blob row -- pairs at exactly eps sit in the screen's band"""
    return np.sort(ix.Dp[int(np.flatnonzero(ix.perm == 0)[0])])[max(ms, 3) - 1]


def both(native, ix, eps, ms, what, stats=None):
    """the screened host form against the model and against hnswdbs_exact's bytes; returns (bytes, stats)"""
    rc, old, c_old = exact_host(native, ix.h, ix.n, eps, ms)
    compare(rc, old, c_old, ix.want(eps, ms), (what, "existing"))
    rc, got, c, st = screened_host(native, ix.h, ix.n, eps, ms)
    compare(rc, got, c, ix.want(eps, ms), (what, "screened"))
    assert _bytes(got) == _bytes(old) and c == c_old and (stats is None or st[:3] == stats), (what, st)
    return _bytes(got), st


# ------------------------------------------------------------------------------------------------------------ 1. the bounds
@pytest.mark.parametrize("metric", SCREENED)
def test_bounds_hold_the_oracles_distance(native, oracle, tmp_path_factory, metric):
    """300 rows against themselves: lb <= the oracle's f32 distance <= ub; a pair with a row outside the proved range -- NaN, +-inf,
    +-FLT_MAX, all zeros, a squared norm below 2^-40 -- has lb = +0 and ub = +inf.  (DistCosine: the reference asserts on +-inf and
    +-FLT_MAX rows, so the oracle cannot take them; NaN rows stand in.)  Fails without the entry."""
    levels = np.zeros(300, np.int64)                          # Dump's levels at seed 0, restated: column f of the matrices is row at[f]
    rng = np.random.default_rng(0)
    levels[rng.random(300) < 0.1] = 1
    levels[rng.random(300) < 0.02] = 2
    at = np.asarray(dump_order(levels)[0])
    bad = np.zeros(300, bool)
    bad[[3, 40, 41, 100, 101, 200, 201, 299]] = True
    for d in (1, 31, 32, 33, 128):
        X = uniform(300, d, 7 * d) + np.float32(0.01)
        X[3], X[40], X[41], X[100], X[101], X[200], X[201], X[299] = np.nan, INF, -INF, FLT_MAX, -FLT_MAX, 0.0, -0.0, 1e-9
        if metric == "DistCosine":
            X[[40, 41, 100, 101], 0] = np.nan
        ix = Dump(native, oracle, tmp_path_factory.mktemp(f"b{d}"), X, np.arange(300, dtype=np.uint64), metric)
        by_flat = ix.h.dbscan_bounds_matrix(X)
        lb, ub = np.empty_like(by_flat[0]), np.empty_like(by_flat[1])
        lb[:, at], ub[:, at] = by_flat
        D = oracle.dist_matrix(metric, X, X)
        out = bad[:, None] | bad[None, :]
        assert not lb[out].view(np.uint32).any() and np.isposinf(ub[out]).all(), (metric, d)
        assert (lb[~out] <= D[~out]).all() and (D[~out] <= ub[~out]).all() and np.isfinite(ub[~out]).all(), (metric, d)


# ------------------------------------------------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("metric,d", [(m, d) for m in SCREENED for d in (1, 33, 128)] + [("DistL2", 257), ("DistL2", 545)])
def test_shapes_against_the_model_and_the_existing_call(native, oracle, tmp_path_factory, metric, d):
    """n on both sides of a tile of 32 W queries, of a block of rows and of a slab; d = 257 and 545: the first dpad of W = 2 and of
    W = 1.  eps a value of D and the next f32 below it.  Stats: every point through the screen, p pairs through the chain with
    1 <= p < n * n / 4 (the band is exercised; the screen decides most pairs).  At d = 1 DistDot and DistCosine know one distance,
    +0, between unit rows: the model has one cluster, every pair sits in the band and the larger n outgrow the buffer -- there only
    the answers and the sum of the stats are held."""
    import torch
    flat = d == 1 and metric != "DistL2"
    for n in (256, 257, 319, 320, 2113):
        X, ids = rows_of(metric, d, n)
        ix = Dump(native, oracle, tmp_path_factory.mktemp(f"s{n}"), X, ids, metric, seed=n)
        for ms in (1, 2, 5, 40):
            at = eps_at(ix, ms)
            for eps in (at, np.nextafter(at, -INF)):
                want = ix.want(eps, ms)
                assert flat or (want.n_clusters >= 2 and (ms < 5 or _kinds(want)[0] >= 1)), (metric, d, n, ms, eps, want.n_clusters)
                a, st = both(native, ix, eps, ms, (metric, d, n, ms, eps))
                assert sum(st[:3]) == n and (flat or (st[:3] == [n, 0, 0] and 1 <= st[3] < n * n // 4)), (metric, d, n, ms, st)
                b, st2 = both(native, ix, eps, ms, "again")
                assert a == b and st2 == st, ("two calls, two answers", metric, d, n, ms)
        rc, got, c, st3 = screened_device(native, ix.h, n, eps, 40, stream=torch.cuda.Stream())
        compare(rc, got, c, ix.want(eps, 40), (metric, d, n, "device form, a caller's stream"))
        assert _bytes(got) == a and st3 == st


# ------------------------------------------------------------------------------------------------------------ 3. to 7.
@pytest.mark.parametrize("metric", SCREENED)
def test_hostile_rows(native, oracle, tmp_path, metric):
    """NaN, +-inf, +-0 and +-FLT_MAX rows among 320 (hostile_rows places them up to row 304): the bytes of hnswdbs_exact.
    (DistCosine: NaN rows in place of the +-inf and +-FLT_MAX rows, on which the reference asserts.)"""
    n = 320
    X = hostile_rows(n)
    if metric == "DistCosine":
        X[[6, 71, 301, 8, 73, 304], 0] = np.nan
    ix = Dump(native, oracle, tmp_path, X, np.random.default_rng(3).permutation(n).astype(np.uint64) * 3 + 1, metric)
    for eps in (np.float32(0.0), np.float32(-0.0), INF, np.float32(-1.0), FLT_MAX):
        for ms in (1, 2, 4):
            rc, old, c_old = exact_host(native, ix.h, n, eps, ms)
            for call in (screened_host, screened_device):
                rc, got, c, st = call(native, ix.h, n, eps, ms)
                assert rc == 0 and _bytes(got) == _bytes(old) and c == c_old and st[:3] == [n, 0, 0], (metric, eps, ms, call.__name__, st)


@pytest.fixture(scope="module")
def blobs(native, oracle, tmp_path_factory):
    """one of case 2's inputs: 2113 x 33 DistL2, min_samples 5, eps a value of D"""
    ix = Dump(native, oracle, tmp_path_factory.mktemp("blobs"), *rows_of("DistL2", 33, 2113), "DistL2", seed=2113)
    eps = eps_at(ix, 5)
    assert ix.want(eps, 5).n_clusters >= 2 and _kinds(ix.want(eps, 5))[0] >= 1
    return ix, eps, both(native, ix, eps, 5, "blobs", [2113, 0, 0])


def test_an_outgrown_buffer_is_the_existing_calls_answer(native, blobs, knob):
    ix, eps, (base, st) = blobs
    assert st[3] > 64
    knob("HNSWGPU_DBSCAN_SCREEN_CAP", 64)
    assert both(native, ix, eps, 5, "cap 64", [0, ix.n, 0])[0] == base
    knob("HNSWGPU_DBSCAN_SCREEN_CAP", None)
    assert both(native, ix, eps, 5, "unhooked") == (base, st)


@pytest.mark.parametrize("byte", (0xFF, 0x5A))
def test_poisoned_scratch(native, blobs, knob, byte):
    ix, eps, base = blobs
    knob("HNSWGPU_POISON_SCRATCH", byte)
    assert both(native, ix, eps, 5, ("poison", byte)) == base
    rc, got, c, st = screened_device(native, ix.h, ix.n, eps, 5)
    assert rc == 0 and _bytes(got) == base[0] and st == base[1]


def test_what_is_not_screened(native, oracle, tmp_path_factory):
    """a distance without a screen, and fewer than 256 points: the existing path, whole"""
    for metric, n in (("DistL1", 300), ("DistL2", 255)):
        ix = Dump(native, oracle, tmp_path_factory.mktemp(metric), uniform(n, 8, n), np.arange(n, dtype=np.uint64), metric)
        eps = np.sort(ix.Dp[0])[4]
        assert both(native, ix, eps, 4, (metric, n))[1] == [0, 0, n, 0]
        res, stats = ix.h.dbscan_screened(eps, 4)                # the Python method
        assert np.array_equal(res.labels, ix.want(eps, 4).labels) and stats.tolist() == [0, 0, n, 0]


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_a_border_point_at_exactly_eps_from_two_clusters(native, oracle, tmp_path, order):
    """the construction of tests/test_gpu_dbscan.py in DistL2 among 300 far rows, so that the screen runs: x = 2 is at exactly eps
    from a core point of either cluster and goes to the one of the smaller position"""
    x = np.concatenate([np.array([-1.5, -1, 0, 2, 4, 5, 5.5], np.float32), 100 + 10 * np.arange(300, dtype=np.float32)])
    ids = np.arange(307, dtype=np.uint64) + 3
    ids[:7] = ids[:7] if order == "ascending" else ids[:7][::-1].copy()
    ix = Dump(native, oracle, tmp_path, x[:, None].copy(), ids, "DistL2")
    want = ix.want(2.0, 4)
    assert want.labels[:7].tolist() == [0, 0, 0, 0, 1, 1, 1] and x[ix.perm[want.anchors[3]]] == (0 if order == "ascending" else 4)
    st = both(native, ix, 2.0, 4, ("tie", order), [307, 0, 0])[1]
    assert st[3] >= 1
