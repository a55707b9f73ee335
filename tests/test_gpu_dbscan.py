"""DBSCAN on the device (hnswdbs_exact / _device, hnswdbs_csr / _device, csrc/dbscan.hip) against `dbscan_model` of
tests/test_dbscan_abi.py, section 1 of include/hnsw_mi355x_dbscan.h restated sequentially.

The expected answers never come from the code under test.  Exact form: the sets come from the CPU oracle's distance matrix of the
stored rows against themselves (oracle_lib.dist_matrix, as tests/test_gpu_exact_range.py takes it), `D[i] <= eps` on f32, rows and
columns brought into POSITION order.  Every index is a dump written by hand (tests/dump_writer.py: the entry never reads the graph),
so the dump order that orders equal DataIds is known.  CSR form: the sets are read off the CSR itself.  Every comparison is exact,
integers only; three sentinel slots behind n stay untouched, and so do the optional arrays that were left out.  What the inputs must
contain for a test to mean anything is asserted on the MODEL, never on device output."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import uniform
from dump_writer import write_dump
from test_dbscan_abi import dbscan_model, sets_of_csr, sets_of_matrix
from test_gpu_stream_order import _dev, _host, _sentinel, SENTINEL

pytestmark = pytest.mark.gpu
PAD = 3
NAMES = ("label", "core", "count", "anchor")
DTYPES = {"label": np.int32, "core": np.uint8, "count": np.uint32, "anchor": np.uint32}
METRICS = ("DistL2", "DistCosine", "DistDot", "DistL1", "DistHellinger", "DistJeffreys", "DistJensenShannon")
PROBABILITY = ("DistHellinger", "DistJeffreys", "DistJensenShannon")
INF = np.float32(np.inf)
FLT_MAX = np.float32(np.finfo(np.float32).max)
CLUSTERS = 0x7777


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ----------------------------------------------------------------------------------------------------- calls and comparison
def _fresh(n):
    return {x: _sentinel((n + PAD,), DTYPES[x]) for x in NAMES}


def exact_host(native, h, n, eps, ms, given=NAMES):
    """(rc, the out arrays with their sentinel tails, c) of hnswdbs_exact; the arrays not in `given` are handed in as NULL"""
    o, c = _fresh(n), np.full(1, CLUSTERS, np.uint64)
    rc = native.lib().hnswdbs_exact(h.handle, float(eps), ms, *[_p(o[x]) if x in given else None for x in NAMES], _p(c))
    return rc, o, int(c[0])


def exact_device(native, h, n, eps, ms, given=NAMES, stream=None):
    import torch
    o, c = {x: _dev(_sentinel((n + PAD,), DTYPES[x])) for x in NAMES}, np.full(1, CLUSTERS, np.uint64)
    torch.cuda.synchronize()
    rc = native.lib().hnswdbs_exact_device(h.handle, float(eps), ms, *[C.c_void_p(o[x].data_ptr()) if x in given else None for x in NAMES], _p(c),
                                           C.c_void_p(stream.cuda_stream) if stream is not None else None)
    torch.cuda.synchronize()
    return rc, {x: _host(o[x], DTYPES[x]) for x in NAMES}, int(c[0])


def csr_host(native, offs, cols, dists, eps, ms, add_self, given=NAMES):
    n = len(offs) - 1
    o, c = _fresh(n), np.full(1, CLUSTERS, np.uint64)
    rc = native.lib().hnswdbs_csr(0, n, _p(offs), _p(cols) if len(cols) else None, _p(dists), float(eps), ms, add_self,
                                  *[_p(o[x]) if x in given else None for x in NAMES], _p(c))
    return rc, o, int(c[0])


def csr_device(native, offs, cols, dists, eps, ms, add_self, given=NAMES, stream=None):
    import torch
    n = len(offs) - 1
    o, c = {x: _dev(_sentinel((n + PAD,), DTYPES[x])) for x in NAMES}, np.full(1, CLUSTERS, np.uint64)
    ins = [_dev(offs), _dev(cols) if len(cols) else None, _dev(dists) if dists is not None and len(dists) else None]
    before = [None if t is None else t.clone() for t in ins]
    torch.cuda.synchronize()
    rc = native.lib().hnswdbs_csr_device(0, n, *[C.c_void_p(t.data_ptr()) if t is not None else None for t in ins], float(eps), ms, add_self,
                                         *[C.c_void_p(o[x].data_ptr()) if x in given else None for x in NAMES], _p(c),
                                         C.c_void_p(stream.cuda_stream) if stream is not None else None)
    torch.cuda.synchronize()
    assert all(t is None or torch.equal(t.view(torch.uint8), b.view(torch.uint8)) for t, b in zip(ins, before)), "an input changed"
    return rc, {x: _host(o[x], DTYPES[x]) for x in NAMES}, int(c[0])


def compare(rc, got, c, want, what, given=NAMES):
    """exact, every slot; the tails and the arrays left out at their sentinels"""
    assert rc == 0, (what, rc)
    n = len(want.labels)
    exp = {"label": want.labels, "core": want.core, "count": want.counts, "anchor": want.anchors}
    assert c == want.n_clusters, (what, c, want.n_clusters)
    for x in NAMES:
        if x in given:
            bad = np.flatnonzero(got[x][:n] != exp[x])
            assert len(bad) == 0, (what, x, len(bad), bad[:5], got[x][:n][bad[:5]], exp[x][bad[:5]])
            assert (got[x][n:].view(np.uint8) == SENTINEL).all(), (what, x, "written behind the answer")
        else:
            assert (got[x].view(np.uint8) == SENTINEL).all(), (what, x, "an array that was left out was written")


def _bytes(got):
    return b"".join(got[x].tobytes() for x in NAMES)


# ----------------------------------------------------------------------------------------------------- indexes written by hand
class Dump:
    """rows X under ids on a few layers, written by hand and loaded: position p is row perm[p], the ascending (DataId, dump order)
    order; Dp the oracle's matrix of the rows against themselves in position order, computed once and never modified"""

    def __init__(self, native, oracle, tmp, X, ids, metric, upload=True, seed=0):
        self.X, self.n, self.metric = np.ascontiguousarray(X, np.float32), len(X), metric
        self.ids = np.asarray(ids, np.uint64)
        levels = np.zeros(self.n, np.int64)
        rng = np.random.default_rng(seed)
        levels[rng.random(self.n) < 0.1] = 1
        levels[rng.random(self.n) < 0.02] = 2
        order, _ = write_dump(tmp, "dbs", self.X, self.ids, levels, metric)
        flat_of_row = np.empty(self.n, np.int64)
        flat_of_row[np.asarray(order)] = np.arange(self.n)
        self.perm = np.lexsort((flat_of_row, self.ids))
        self.h = native.HnswIo(str(tmp), "dbs").load_hnsw(metric)
        assert self.h.get_nb_point() == self.n
        if upload:
            self.h.upload(0)
        D = oracle.dist_matrix(metric, self.X, self.X)
        self.Dp = np.ascontiguousarray(D[np.ix_(self.perm, self.perm)])
        self._want = {}

    def want(self, eps, ms):
        key = (np.float32(eps).tobytes(), ms)
        if key not in self._want:
            self._want[key] = dbscan_model(sets_of_matrix(self.Dp, eps), ms)
        return self._want[key]


def _kinds(want):
    core = want.core.astype(bool)
    return int((~core & (want.labels >= 0)).sum()), int((want.labels < 0).sum())     # border points, noise points


# ----------------------------------------------------------------------------------------------------- 1. exact form, general
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257])
def test_small_indexes_and_dimensions(native, oracle, tmp_path_factory, n):
    """a part-filled last tile, lanes past the slab, an odd number of float4 chunks; the host form twice for equal bytes, the device
    form once"""
    for d in (1, 3, 4, 5, 25):
        X = uniform(n, d, 100 * n + d)
        ids = np.random.default_rng(n + d).permutation(n).astype(np.uint64) * 3 + 1
        ix = Dump(native, oracle, tmp_path_factory.mktemp(f"s{n}_{d}"), X, ids, "DistL2", seed=n)
        s = np.sort(ix.Dp, axis=1)
        for ms, eps in ((1, 0.0), (2, s[0, min(1, n - 1)]), (3, s[n // 2, min(3, n - 1)]), (4, np.median(s[:, min(4, n - 1)])), (1, INF)):
            want = ix.want(eps, ms)
            rc, a, c = exact_host(native, ix.h, n, eps, ms)
            compare(rc, a, c, want, ("host", n, d, ms, eps))
            rc, b, c = exact_host(native, ix.h, n, eps, ms)
            assert rc == 0 and _bytes(a) == _bytes(b), ("two calls, two answers", n, d, ms)
            rc, g, c = exact_device(native, ix.h, n, eps, ms)
            compare(rc, g, c, want, ("device", n, d, ms, eps))
            assert _bytes(g) == _bytes(a)
        assert ix.want(INF, 1).n_clusters == 1 and ix.want(0.0, 1).n_clusters == n


# ----------------------------------------------------------------------------------------------------- 2. seven metrics
N_BLOBS, PER_BLOB, N_NOISE, N_COPIES, N_SHARED = 12, 200, 450, 100, 50


def blob_data(metric, d=4, seed=5):
    """3000 rows of dimension 4: 12 blobs of 200 around centres that come in close pairs, 450 uniform rows, 100 exact copies of blob rows that carry
    their original's DataId, and 50 further rows that share a DataId with a blob row without being its copy (dump order decides
    their positions).  Positive and summing to 1 for the probability metrics, unit length for DistDot and DistCosine."""
    rng = np.random.default_rng(seed)
    base = rng.random((N_BLOBS // 2, d)) * 0.6 + 0.2
    centres = np.concatenate([base, base + rng.normal(0, 0.05, base.shape)])
    blobs = np.repeat(centres, PER_BLOB, axis=0) + rng.normal(0, 0.02, (N_BLOBS * PER_BLOB, d))
    X = np.abs(np.concatenate([blobs, rng.random((N_NOISE + N_SHARED, d))])) + 1e-3
    src = rng.choice(N_BLOBS * PER_BLOB, N_COPIES, replace=False)
    X = np.concatenate([X, X[src]])
    n = len(X)
    if metric in PROBABILITY:
        X = X / X.sum(1)[:, None]
    X = np.ascontiguousarray(X.astype(np.float32))
    if metric in ("DistDot", "DistCosine"):
        import oracle_lib
        for i in range(n):                                      # the crate's l2_normalize, f32
            oracle_lib.lib().orc_l2_normalize(X[i].ctypes.data, d)
    X[n - N_COPIES:] = X[src]                                   # exact copies, bit for bit
    ids = rng.permutation(n).astype(np.uint64) * 3 + 1
    ids[n - N_COPIES:] = ids[src]
    ids[N_BLOBS * PER_BLOB + N_NOISE:n - N_COPIES] = ids[rng.choice(N_BLOBS * PER_BLOB, N_SHARED, replace=False)]
    assert n == 3000 and len(np.unique(ids)) == n - N_COPIES - N_SHARED
    return X, ids


def eps_from(Dp, ms, one_way=False):
    """a value OF D: the max(ms, 3)-th smallest distance of a row, so that pairs sit exactly on the boundary -- the first row for
    which (one_way) some pair is within it in one direction only"""
    k = max(ms, 3)
    first = np.sort(Dp[0])[k - 1]
    for i in range(len(Dp)):
        eps = np.sort(Dp[i])[k - 1]
        if not one_way:
            return eps
        if eps > first * np.float32(1.5):                       # (a row out in the noise: its scale is not the blobs')
            continue
        with np.errstate(invalid="ignore"):
            hit = Dp <= eps
        if (hit != hit.T).any():
            return eps
    raise AssertionError("no eps among D's values with a pair that is within it one way only: change the data")


@pytest.mark.parametrize("metric", METRICS)
def test_seven_metrics_on_blobs_and_noise(native, oracle, tmp_path, metric):
    """3000 points: 188 tiles, 12 slabs of 256 rows.  min_samples 1, 2, 5 and 40, eps a value of D and the next f32 below it.
    Every point is in its own set (its distance to itself is within every eps used here), so min_samples 1 has neither border nor
    noise and min_samples 2 has no border (a point that is not core has only itself): those are asserted for 5 and 40."""
    X, ids = blob_data(metric)
    ix = Dump(native, oracle, tmp_path, X, ids, metric)
    n = ix.n
    asym = metric in ("DistJeffreys", "DistJensenShannon")
    two_sided = 0
    for ms in (1, 2, 5, 40):
        at = eps_from(ix.Dp, ms, one_way=asym and ms == 5)
        for eps in (at, np.nextafter(at, -INF)):
            want = ix.want(eps, ms)
            border, noise = _kinds(want)
            assert want.n_clusters >= 2, (metric, ms, eps, want.n_clusters)
            assert (ms < 2 or noise >= 1) and (ms < 5 or border >= 1), (metric, ms, eps, border, noise)
            sets = sets_of_matrix(ix.Dp, eps)
            if ms == 5:
                core = want.core.astype(bool)
                two_sided += sum(1 for i in np.flatnonzero(~core & (want.labels >= 0)) if len({int(want.labels[j]) for j, _ in sets[i] if core[j]}) >= 2)
                if asym and eps == at:
                    with np.errstate(invalid="ignore"):
                        hit = ix.Dp <= eps
                    assert (hit != hit.T).any(), "a pair within eps in one direction only"
            assert (ix.Dp == eps).any() == (eps == at)
            rc, got, c = exact_host(native, ix.h, n, eps, ms)
            compare(rc, got, c, want, (metric, ms, eps))
    assert two_sided >= 1, "a border point with candidates in two clusters"
    # equal DataIds that are no copies: the dump order has decided (their rows differ, so a swap would show)
    eps = eps_from(ix.Dp, 5)
    rc, got, c = exact_device(native, ix.h, n, eps, 5)
    compare(rc, got, c, ix.want(eps, 5), (metric, "device"))


# ----------------------------------------------------------------------------------------------------- 3. extremes
@pytest.mark.parametrize("order", ["ascending", "permuted"])
def test_a_chain_is_one_cluster_across_every_tile_and_slab(native, oracle, tmp_path, order):
    n = 2000
    X = np.arange(n, dtype=np.float32)[:, None].copy()
    ids = np.arange(n, dtype=np.uint64) if order == "ascending" else np.random.default_rng(4).permutation(n).astype(np.uint64)
    ix = Dump(native, oracle, tmp_path, X, ids, "DistL1")
    want = ix.want(1.0, 3)
    ends = np.flatnonzero(np.isin(ix.perm, (0, n - 1)))
    assert want.n_clusters == 1 and (want.labels == 0).all() and np.flatnonzero(want.core == 0).tolist() == ends.tolist()
    for call in (exact_host, exact_device):
        rc, got, c = call(native, ix.h, n, 1.0, 3)
        compare(rc, got, c, want, ("chain", order, call.__name__))
    below = np.nextafter(np.float32(1), np.float32(0))
    rc, got, c = exact_host(native, ix.h, n, below, 2)
    compare(rc, got, c, ix.want(below, 2), ("chain", order, "below"))
    assert c == 0


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_a_border_point_at_exactly_eps_from_two_clusters(native, oracle, tmp_path, order):
    """the second hand-made case of tests/test_dbscan_abi.py on the device: the tie goes to the smaller position"""
    x = np.array([-1.5, -1, 0, 2, 4, 5, 5.5], np.float32)
    ids = np.arange(7, dtype=np.uint64) + 3 if order == "ascending" else np.arange(7, dtype=np.uint64)[::-1] + 3
    ix = Dump(native, oracle, tmp_path, x[:, None].copy(), ids, "DistL1")
    want = ix.want(2.0, 4)
    assert want.labels.tolist() == [0, 0, 0, 0, 1, 1, 1] and want.anchors.tolist() == [2, 2, 2, 2, 4, 4, 4]
    assert x[ix.perm[want.anchors[3]]] == (0 if order == "ascending" else 4)
    for call in (exact_host, exact_device):
        rc, got, c = call(native, ix.h, 7, 2.0, 4)
        compare(rc, got, c, want, ("tie", order, call.__name__))


def hostile_rows(n=500, d=3):
    """uniform rows among which: rows with a NaN element, +inf and -inf rows, rows of +0 and of -0, rows of FLT_MAX and -FLT_MAX"""
    X = uniform(n, d, 77) * np.float32(0.25)
    X[5], X[70], X[300] = np.nan, (0.5, np.nan, 0.5), (np.nan, 0, 0)
    X[6], X[71], X[301] = INF, -INF, (INF, 0, 0)
    X[7], X[72], X[302], X[303] = 0.0, -0.0, (0.0, -0.0, 0.0), 0.0
    X[8], X[73], X[304] = FLT_MAX, -FLT_MAX, FLT_MAX
    return X


@pytest.mark.parametrize("metric", ["DistL2", "DistL1"])
def test_hostile_values(native, oracle, tmp_path, metric):
    n = 500
    X = hostile_rows(n)
    ids = np.random.default_rng(3).permutation(n).astype(np.uint64) * 3 + 1
    ix = Dump(native, oracle, tmp_path, X, ids, metric)
    nan_rows = np.flatnonzero(np.isin(ix.perm, (5, 70, 300)))
    assert np.isnan(ix.Dp[nan_rows]).all() and np.isnan(ix.Dp[:, nan_rows]).all()           # nobody's neighbour, their own included
    assert np.isinf(ix.Dp).any() and (ix.Dp == 0).sum() > n - 6
    for eps in (np.float32(0.0), np.float32(-0.0), INF, np.float32(-1.0), FLT_MAX):
        for ms in (1, 2, 4):
            want = ix.want(eps, ms)
            assert (want.counts[nan_rows] == 0).all() and (want.labels[nan_rows] == -1).all()
            if eps == INF:                                      # one cluster of everything that is not NaN
                assert want.n_clusters == 1 and np.flatnonzero(want.labels < 0).tolist() == nan_rows.tolist()
            if eps < 0:
                assert want.n_clusters == 0 and (want.counts == 0).all()
            for call in (exact_host, exact_device):
                rc, got, c = call(native, ix.h, n, eps, ms)
                compare(rc, got, c, want, (metric, eps, ms, call.__name__))
    assert _bytes_of(ix.want(0.0, 2)) == _bytes_of(ix.want(-0.0, 2)) and ix.want(0.0, 2).n_clusters >= 1     # -0 equals +0: the zero rows


def _bytes_of(want):
    return want.labels.tobytes() + want.core.tobytes() + want.counts.tobytes() + want.anchors.tobytes()


@pytest.fixture(scope="module")
def plain(native, oracle, tmp_path_factory):
    """700 uniform rows of dimension 8, DistL2, and an eps with clusters, border points and noise at min_samples 4"""
    n = 700
    ix = Dump(native, oracle, tmp_path_factory.mktemp("plain"), uniform(n, 8, 9), np.random.default_rng(9).permutation(n).astype(np.uint64) + 11, "DistL2")
    eps = np.sort(ix.Dp[0])[4]
    want = ix.want(eps, 4)
    assert want.n_clusters >= 2 and min(_kinds(want)) >= 1
    return ix, eps, want


def test_refusals_on_a_device(native, oracle, tmp_path, plain):
    N = native._native
    ix, eps, want = plain
    ix.h.set_arithmetic("simd8")
    try:
        for call in (exact_host, exact_device):
            rc, got, c = call(native, ix.h, ix.n, eps, 4)
            assert rc == N.ERR_ARG and "SIMD8" in N.last_error() and c == CLUSTERS and (_bytes(got) == bytes([SENTINEL]) * len(_bytes(got)))
    finally:
        ix.h.set_arithmetic("scalar")
    X = native.round_to_f16(uniform(100, 8, 2))
    half = Dump(native, oracle, tmp_path, X, np.arange(100, dtype=np.uint64), "DistL2", upload=False)
    half.h.set_storage("f16")
    half.h.upload(0)
    for call in (exact_host, exact_device):
        rc, got, c = call(native, half.h, 100, 0.5, 4)
        assert rc == N.ERR_ARG and "HNSWGPU_STORAGE_F16" in N.last_error() and c == CLUSTERS
    rc, got, c = exact_host(native, ix.h, ix.n, eps, 4)          # the next call is right
    compare(rc, got, c, want, "after the refusals")


def test_device_form_wants_a_resident_replica(native, oracle, tmp_path):
    N = native._native
    ix = Dump(native, oracle, tmp_path, uniform(100, 8, 3), np.arange(100, dtype=np.uint64), "DistL2", upload=False)
    rc, got, c = exact_device(native, ix.h, 100, 0.5, 3)
    assert rc == N.ERR_DEVICE and "upload" in N.last_error() and c == CLUSTERS and _bytes(got) == bytes([SENTINEL]) * len(_bytes(got))
    rc, got, c = exact_host(native, ix.h, 100, 0.5, 3)           # the host form uploads on first use
    compare(rc, got, c, ix.want(0.5, 3), "first use")
    rc, got, c = exact_device(native, ix.h, 100, 0.5, 3)
    compare(rc, got, c, ix.want(0.5, 3), "resident now")


def test_an_index_without_a_point(native):
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    e.parallel_insert(np.zeros((0, 8), np.float32))
    for call in (exact_host, exact_device):
        rc, got, c = call(native, e, 0, 0.5, 3)
        assert rc == 0 and c == 0 and _bytes(got) == bytes([SENTINEL]) * len(_bytes(got))
    assert e.dbscan(0.5, 3).n_clusters == 0


def test_two_threads_on_one_handle(native, plain):
    ix, eps, want = plain
    other = ix.want(np.sort(ix.Dp[1])[7], 6)
    out, errs = {}, []

    def run(name, e, ms):
        try:
            out[name] = [exact_host(native, ix.h, ix.n, e, ms) for _ in range(4)]
        except Exception as err:  # noqa: BLE001
            errs.append(err)
    ts = [threading.Thread(target=run, args=("a", eps, 4)), threading.Thread(target=run, args=("b", np.sort(ix.Dp[1])[7], 6))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for name, w in (("a", want), ("b", other)):
        for rc, got, c in out[name]:
            compare(rc, got, c, w, ("thread", name))


def test_a_callers_stream_and_the_optional_outputs(native, plain):
    import torch
    ix, eps, want = plain
    stream = torch.cuda.Stream()
    rc, got, c = exact_device(native, ix.h, ix.n, eps, 4, stream=stream)
    compare(rc, got, c, want, "a caller's stream")
    for given in (("label",), ("label", "core"), ("label", "count"), ("label", "anchor")):
        for call in (exact_host, exact_device):
            rc, got, c = call(native, ix.h, ix.n, eps, 4, given=given)
            compare(rc, got, c, want, (call.__name__, given), given=given)
    res = ix.h.dbscan(eps, 4)                                   # the Python method
    assert res.n_clusters == want.n_clusters and np.array_equal(res.labels, want.labels) and np.array_equal(res.core, want.core.astype(bool))
    assert np.array_equal(res.counts, want.counts) and np.array_equal(res.anchors, want.anchors)


# ----------------------------------------------------------------------------------------------------- 4. CSR form
def csr_of_matrix(Dp, eps, seed):
    """the CSR of the sets D[i] <= eps with every row's entries in shuffled order"""
    rng = np.random.default_rng(seed)
    with np.errstate(invalid="ignore"):
        hit = Dp <= np.float32(eps)
    rows = [rng.permutation(np.flatnonzero(hit[i])) for i in range(len(Dp))]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    cols = np.concatenate(rows).astype(np.uint32) if offs[-1] else np.zeros(0, np.uint32)
    dists = np.concatenate([Dp[i, r] for i, r in enumerate(rows)]).astype(np.float32) if offs[-1] else np.zeros(0, np.float32)
    return offs, cols, dists


def _csr_both(native, offs, cols, dists, eps, ms, add_self, what):
    want = dbscan_model(sets_of_csr(offs, cols, dists, eps), ms, add_self)
    out = []
    for call in (csr_host, csr_device):
        rc, got, c = call(native, offs, cols, dists, eps, ms, add_self)
        assert rc == 0, (what, native._native.last_error())
        compare(rc, got, c, want, (what, call.__name__))
        out.append(got)
    assert _bytes(out[0]) == _bytes(out[1])
    return want, out[0]


def test_csr_built_from_d_gives_the_exact_forms_bytes(native, plain):
    ix, eps, want = plain
    rc, exact, c = exact_host(native, ix.h, ix.n, eps, 4)
    compare(rc, exact, c, want, "exact")
    offs, cols, dists = csr_of_matrix(ix.Dp, eps, 1)
    _, got = _csr_both(native, offs, cols, dists, eps, 4, 0, "the sets themselves")
    assert _bytes(got) == _bytes(exact)
    offs, cols, dists = csr_of_matrix(ix.Dp, np.sort(ix.Dp[0])[30], 2)          # a wider CSR, cut by eps
    _, got = _csr_both(native, offs, cols, dists, eps, 4, 0, "a wider CSR under eps")
    assert _bytes(got) == _bytes(exact)


def test_csr_of_the_symmetric_graph(native, plain):
    """the outputs of symmetric_knn_graph_flat (k = 8, union) as they stand, add_self 1, eps at a stored distance"""
    ix, _, _ = plain
    g = ix.h.symmetric_knn_graph_flat(8, None, "union")
    offs, cols, dists = g.offsets, g.pos.astype(np.uint32), g.dists
    eps = np.sort(dists)[len(dists) // 3]
    for ms, e in ((4, eps), (4, np.nextafter(eps, -INF)), (9, INF), (3, eps)):
        want, _ = _csr_both(native, offs, cols, dists, e, ms, 1, ("symmetric graph", ms, e))
        assert want.n_clusters >= 1 and (ms != 4 or min(_kinds(want)) >= 1)
    want, _ = _csr_both(native, offs, cols, None, -1.0, 9, 1, "without dists")
    assert (want.counts == np.diff(offs.astype(np.int64)) + 1).all()
    res = native.csr_dbscan(offs, cols, dists, eps, 4, add_self=True)
    w = dbscan_model(sets_of_csr(offs, cols, dists, eps), 4, 1)
    assert res.n_clusters == w.n_clusters and np.array_equal(res.labels, w.labels) and np.array_equal(res.anchors, w.anchors)


def test_csr_self_loops_duplicates_a_hub_and_empty_rows(native):
    n = 1500
    rng = np.random.default_rng(8)
    rows = [[] for _ in range(n)]
    rows[0] = [j for j in range(1, n)]                          # a hub row of n - 1 entries
    for i in range(1, n):
        if i % 7 == 0:
            continue                                            # empty rows
        rows[i] = rng.integers(0, n, int(rng.integers(1, 6))).tolist()
        if i % 5 == 0:
            rows[i] += [i, i]                                   # self loops, twice
        if i % 3 == 0:
            rows[i] += rows[i][:2]                              # duplicated entries
    offs = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    cols = np.concatenate([np.asarray(r, np.uint32) for r in rows if r])
    dists = rng.integers(0, 4, len(cols)).astype(np.float32) * np.float32(0.25)        # few values: ties for the anchor by position
    dists[rng.random(len(cols)) < 0.02] = np.nan
    dists[rng.random(len(cols)) < 0.02] = -0.0
    for ms, eps, add in ((4, 0.5, 0), (4, 0.5, 1), (2, 0.25, 0), (6, INF, 1), (1, 0.0, 0)):
        want, _ = _csr_both(native, offs, cols, dists, eps, ms, add, ("hub", ms, eps, add))
        assert want.core[0] == 1
    want, _ = _csr_both(native, offs, cols, dists, 0.5, 4, 0, "again")
    assert want.n_clusters >= 1 and min(_kinds(want)) >= 1
    empty = np.zeros(n + 1, np.uint64)
    want, _ = _csr_both(native, empty, np.zeros(0, np.uint32), None, 1.0, 1, 1, "no entry at all")
    assert want.n_clusters == n
    want, _ = _csr_both(native, empty, np.zeros(0, np.uint32), None, 1.0, 1, 0, "no entry, no self")
    assert want.n_clusters == 0


def test_csr_device_form_refuses_malformed_graphs(native):
    """descending offsets, a col >= n, offsets[0] != 0 through the device form: ERR_ARG in hnswgpu_csr_components' words, nothing
    written, and the next call right"""
    N = native._native
    offs, cols = np.array([0, 2, 3, 3, 5], np.uint64), np.array([1, 2, 0, 0, 3], np.uint32)
    dists = np.array([.5, .25, .5, 1, 0], np.float32)
    for bad_offs, bad_cols, word in ((np.array([0, 3, 2, 3, 5], np.uint64), cols, "the offsets descend"),
                                     (offs, np.array([1, 2, 0, 4, 3], np.uint32), "a col is not below n"),
                                     (offs, np.array([1, 2, 0, 0xFFFFFFFF, 3], np.uint32), "a col is not below n"),
                                     (np.array([1, 2, 3, 3, 5], np.uint64), cols, "offsets[0] is not 0")):
        rc, got, c = csr_device(native, bad_offs, bad_cols, dists, 1.0, 2, 0)
        assert rc == N.ERR_ARG and N.last_error() == "csr dbscan: " + word, (rc, N.last_error())
        assert c == CLUSTERS and _bytes(got) == bytes([SENTINEL]) * len(_bytes(got))
        _csr_both(native, offs, cols, dists, 1.0, 2, 0, "the next call")
