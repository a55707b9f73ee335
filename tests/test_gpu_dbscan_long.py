"""Exact DBSCAN behind the streamed two-sided screen (hnswxdl_exact / _device, hnswxdl_bounds_matrix, csrc/dbscan_screen_long.hip), rows
of up to 4096 elements.

References, never the code under test: the CPU oracle's f32 distance matrix fed to `dbscan_model` (through `Dump` of
tests/test_gpu_dbscan.py) and the bytes of hnswdbs_exact on the same index.  Every comparison is exact.  Beyond d = 1120 both bounds'
error term has the coefficient of DESIGN.md 15.16 / 15.19, restated by `coeffs` of tests/test_gpu_exact_long.py; `possible_band` is
the truth moved by twice that term to either side, and every shape case counts, on the oracle's matrix and before the device is
asked, the pairs that may be undecided with it."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_exact_screen_shapes as SH
from conftest import uniform
from dump_writer import dump_order
from test_gpu_dbscan import CLUSTERS, DTYPES, FLT_MAX, INF, NAMES, PAD, Dump, _bytes, _fresh, _kinds, _p, compare, exact_host, hostile_rows
from test_gpu_dbscan_screen import SCREENED, eps_at, screened_host
from test_gpu_exact_long import coeffs
from test_gpu_exact_screen import bound_terms
from test_gpu_stream_order import _dev, _host, _sentinel

pytestmark = pytest.mark.gpu
CAND_CAP = 2 << 20          # DS_CAND_CAP: candidates of one chunk and pass


def long_host(native, h, n, eps, ms):
    o, c, st = _fresh(n), np.full(1, CLUSTERS, np.uint64), np.full(4, 7, np.uint64)
    rc = native.lib().hnswxdl_exact(h.handle, float(eps), ms, *[_p(o[x]) for x in NAMES], _p(c), _p(st))
    return rc, o, int(c[0]), st.tolist()


def long_device(native, h, n, eps, ms, stream=None):
    import torch
    o, c, st = {x: _dev(_sentinel((n + PAD,), DTYPES[x])) for x in NAMES}, np.full(1, CLUSTERS, np.uint64), np.full(4, 7, np.uint64)
    torch.cuda.synchronize()
    rc = native.lib().hnswxdl_exact_device(h.handle, float(eps), ms, *[C.c_void_p(o[x].data_ptr()) for x in NAMES], _p(c), _p(st),
                                           C.c_void_p(stream.cuda_stream) if stream is not None else None)
    torch.cuda.synchronize()
    return rc, {x: _host(o[x], DTYPES[x]) for x in NAMES}, int(c[0]), st.tolist()


def both(native, ix, eps, ms, what, stats=None):
    """the new host form against the model and against hnswdbs_exact's bytes; returns (bytes, stats)"""
    rc, old, c_old = exact_host(native, ix.h, ix.n, eps, ms)
    compare(rc, old, c_old, ix.want(eps, ms), (what, "existing"))
    rc, got, c, st = long_host(native, ix.h, ix.n, eps, ms)
    compare(rc, got, c, ix.want(eps, ms), (what, "long"))
    assert _bytes(got) == _bytes(old) and c == c_old and (stats is None or st[:3] == stats), (what, st)
    return _bytes(got), st


def possible_band(metric, X):
    """(lowest possible lb, highest possible ub) of every pair of rows in f64: the truth moved by 2 E, E with the coefficient the
    call uses at this d -- the same on both sides"""
    pre, E, finish = bound_terms(metric, X, X)                 # E: with screen_coeff
    short, wide = coeffs(metric, X.shape[1])
    E = E * (wide / short if X.shape[1] > 1120 else 1.0)
    s = -1.0 if metric == "DistL2" else 1.0
    return finish(pre + 2 * s * E), finish(pre - 2 * s * E)


def flat_blobs(metric, d, n):
    """n rows of intrinsic dimension 3 around the origin, signed coordinates, through test_gpu_exact_screen_shapes' fixed 3 x d matrix
    (DistDot: normalised): equal parts of four or more wide blobs whose centres are about as far from the origin as the blobs are
    wide -- the error term is a multiple of |q|^2 + |x|^2, which is then of the order of the squared distances --, more than 40 rows
    each, two of them close; an eighth uniform rows; 10 exact copies under their original's DataId; 10 rows that share a DataId with
    a blob row without being its copy."""
    rng = np.random.default_rng(1000 + d + n)
    rows = n - n // 8 - 20
    nb = max(4, -(-rows // 200))
    centres = np.array([(0.5, 0, 0), (0.5, 0.3, 0), (-0.5, 0, 0.1), (0, -0.5, 0), (0, 0, 0.5), (0, 0.5, -0.2), (-0.3, -0.3, -0.3), (0.3, -0.3, 0.4),
                        (-0.4, 0.4, 0.2), (0.2, 0.2, -0.5), (-0.1, -0.5, 0.4)])[:nb]
    z = np.concatenate([centres[np.arange(rows) % nb] + 0.06 * rng.standard_normal((rows, 3)), rng.random((n // 8 + 10, 3)) - 0.5])
    A = np.random.default_rng(7000 + d).standard_normal((3, d))
    X = np.ascontiguousarray((z @ A).astype(np.float32))
    if metric == "DistDot":
        X = SH._unit(X)
    ids = np.arange(len(X), dtype=np.uint64) * 2 + 5
    X, ids = np.concatenate([X, X[:10]]), np.concatenate([ids, ids[:10]])
    ids[n - 20:n - 10] = ids[20:30]
    assert len(X) == n
    return X, ids


# ------------------------------------------------------------------------------------------------------------ 1. the bounds
@pytest.mark.parametrize("d", (1, 130, 784, 1121, 4096))
@pytest.mark.parametrize("metric", SCREENED)
def test_bounds_hold_the_oracles_distance(native, oracle, tmp_path_factory, metric, d):
    """300 rows of DESIGN.md 15.13's worst inputs (same sign, cancellation, exact copies) against 37 queries through the streamed
    kernel: lb <= the oracle's f32 distance <= ub, ub finite; d = 1121 and 4096 are the test of 15.19's derivation.  With a NaN row,
    a zero row and a row of squared norm below 2^-40 on either side: lb = +0 and ub = +inf.  Fails without the entry."""
    def bounds(X, Q, name):
        case = SH.Plain(metric, X, Q)
        by_flat = case.load(native, tmp_path_factory.mktemp("b")).dbscan_long_bounds_matrix(case.Q)
        lb, ub = np.empty_like(by_flat[0]), np.empty_like(by_flat[1])
        lb[:, np.asarray(dump_order(case.levels)[0])], ub[:, np.asarray(dump_order(case.levels)[0])] = by_flat
        return lb, ub, oracle.dist_matrix(metric, case.Q, case.X)

    for kind, (X, Q) in SH._bound_inputs(metric, d).items():
        lb, ub, D = bounds(X[:300], Q, kind)
        assert (lb <= D).all() and (D <= ub).all() and np.isfinite(ub).all(), (metric, d, kind, float((lb - D).max()), float((D - ub).max()))
    X, Q = (a.copy() for a in SH._bound_inputs(metric, d)["same sign"])
    X, bad = X[:300], np.zeros(300, bool)
    X[3], X[200], X[299], bad[[3, 200, 299]] = np.nan, 0.0, 1e-9, True
    Q[:3] = X[[3, 200, 299]]
    lb, ub, D = bounds(X, Q, "outside")
    out = (np.arange(37) < 3)[:, None] | bad[None, :]
    assert not lb[out].view(np.uint32).any() and np.isposinf(ub[out]).all(), (metric, d)
    assert (lb[~out] <= D[~out]).all() and (D[~out] <= ub[~out]).all() and np.isfinite(ub[~out]).all(), (metric, d)


# ------------------------------------------------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("d", (257, 545, 784, 1121, 1158, 4096))
@pytest.mark.parametrize("metric", SCREENED)
def test_shapes_against_the_model_and_the_existing_call(native, oracle, tmp_path_factory, metric, d):
    """both sides of the routing (257) and of the coefficient switch (1120 | 1121), d % 32 != 0, d % 8 != 0, the last length; n: whole
    tiles, one slot into a third tile with a row block of one row, a tile whose last two wavefronts have no query, and (d <= 545)
    several slabs.  eps a value of D and the next f32 below it."""
    import torch
    for n in (256, 257, 320) + ((2113,) if d <= 545 else ()):
        X, ids = flat_blobs(metric, d, n)
        ix = Dump(native, oracle, tmp_path_factory.mktemp(f"s{n}"), X, ids, metric, seed=n)
        low, high = possible_band(metric, X)
        for ms in (1, 5, 40):
            at = eps_at(ix, ms)
            for eps in (at, np.nextafter(at, -INF)):
                want = ix.want(eps, ms)
                assert want.n_clusters >= 2 and (ms < 5 or _kinds(want)[0] >= 1), (metric, d, n, ms, eps, want.n_clusters)
                may = int(((low <= float(eps)) & (float(eps) < high)).sum())      # the input, before the device is asked
                assert may < min(n * n // 4, CAND_CAP), (metric, d, n, ms, may)
                a, st = both(native, ix, eps, ms, (metric, d, n, ms, eps))
                assert st[:3] == [n, 0, 0] and 1 <= st[3] < n * n // 4, (metric, d, n, ms, st, may)
                b, st2 = both(native, ix, eps, ms, "again")
                assert a == b and st2 == st, ("two calls, two answers", metric, d, n, ms)
        rc, got, c, st3 = long_device(native, ix.h, n, eps, 40, stream=torch.cuda.Stream())
        compare(rc, got, c, ix.want(eps, 40), (metric, d, n, "device form, a caller's stream"))
        assert _bytes(got) == a and st3 == st


# ------------------------------------------------------------------------------------------------------------ 3. to 6.
@pytest.mark.parametrize("d", (545, 1121))
@pytest.mark.parametrize("metric", SCREENED)
def test_hostile_rows(native, oracle, tmp_path, metric, d):
    """tests/test_gpu_dbscan_screen.py's hostile case at long rows -- hostile_rows' three columns repeated to d, so that a NaN, +-inf,
    zero or +-FLT_MAX row stays one --: the bytes of hnswdbs_exact from both forms"""
    n = 320
    X = np.ascontiguousarray(np.tile(hostile_rows(n), (1, -(-d // 3)))[:, :d])
    if metric == "DistCosine":
        X[[6, 71, 301, 8, 73, 304], 0] = np.nan
    ix = Dump(native, oracle, tmp_path, X, np.random.default_rng(3).permutation(n).astype(np.uint64) * 3 + 1, metric)
    for eps in (np.float32(0.0), np.float32(-0.0), INF, np.float32(-1.0), FLT_MAX):
        for ms in (1, 2, 4):
            rc, old, c_old = exact_host(native, ix.h, n, eps, ms)
            for call in (long_host, long_device):
                rc, got, c, st = call(native, ix.h, n, eps, ms)
                assert rc == 0 and _bytes(got) == _bytes(old) and c == c_old and st[:3] == [n, 0, 0], (metric, d, eps, ms, call.__name__, st)


def test_routing(native, oracle, tmp_path_factory):
    """d = 128: hnswxd_exact's bytes and stats.  d = 4097, a distance without a screen, fewer than 256 points: not screened"""
    ix = Dump(native, oracle, tmp_path_factory.mktemp("r128"), *flat_blobs("DistL2", 128, 320), "DistL2")
    eps = eps_at(ix, 5)
    a, st = both(native, ix, eps, 5, "d 128", [320, 0, 0])
    rc, got, c, st_old = screened_host(native, ix.h, ix.n, eps, 5)
    assert rc == 0 and _bytes(got) == a and st == st_old
    for metric, d, n in (("DistL2", 4097, 256), ("DistL1", 300, 300), ("DistL2", 300, 255)):
        ix = Dump(native, oracle, tmp_path_factory.mktemp(f"r{d}{n}"), uniform(n, d, n), np.arange(n, dtype=np.uint64), metric)
        eps = np.sort(ix.Dp[0])[4]
        assert both(native, ix, eps, 4, (metric, d, n))[1] == [0, 0, n, 0]
        res, stats = ix.h.dbscan_screened_long(eps, 4)                # the Python method
        assert np.array_equal(res.labels, ix.want(eps, 4).labels) and stats.tolist() == [0, 0, n, 0]
    with pytest.raises(native.HnswError, match="rows too long"):
        Dump(native, oracle, tmp_path_factory.mktemp("m"), uniform(256, 4097, 1), np.arange(256, dtype=np.uint64), "DistL2").h.dbscan_long_bounds_matrix(
            uniform(2, 4097, 2))


@pytest.fixture(scope="module")
def blobs(native, oracle, tmp_path_factory):
    """one of case 2's inputs: 320 x 784 DistL2, min_samples 5, eps a value of D"""
    ix = Dump(native, oracle, tmp_path_factory.mktemp("blobs"), *flat_blobs("DistL2", 784, 320), "DistL2", seed=320)
    eps = eps_at(ix, 5)
    return ix, eps, both(native, ix, eps, 5, "blobs", [320, 0, 0])


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
    rc, got, c, st = long_device(native, ix.h, ix.n, eps, 5)
    assert rc == 0 and _bytes(got) == base[0] and st == base[1]
