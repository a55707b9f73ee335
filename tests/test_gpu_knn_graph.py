"""Queries by stored point on the device (Hnsw.knn_graph_flat / exact_knn_graph_flat -> hnswgpu_graph_search_batch /
hnswgpu_exact_graph_batch and their _device forms, csrc/knn_graph.hip): the k-NN graph of the indexed points, the point itself
excluded by IDENTITY (its p_id) and not by id or distance.

The expected answers never come from the code under test.  Exact graph: per point the lexsort of the CPU oracle's distance matrix
over the OTHER points (by distance, DataId, dump position), and the device's own exact_search_flat(X[p], k + 1) with the point's own
(layer, rank) removed.  Approximate graph: the oracle's `search` of the stored vectors with knbn = k + 1 and the drop rule applied
in Python (tests/test_knn_graph_abi.py), and parallel_search_flat(X[pts], k + 1, ef) with the same rule.  Every comparison is exact:
ids, f32 bits, (layer, rank), counts, zeroed tails.  What the inputs must contain (rows without an own entry, copies at distance
0) is asserted on the oracle's side, never on device output."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import f64_reference as F
from conftest import uniform
from dump_writer import dump_order, write_dump
from test_gpu_exact_knn_hostile import Case, N
from test_knn_graph_abi import apply_drop_self, resolve

pytestmark = pytest.mark.gpu
KS = (1, 10, N - 1, N + 5)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _assert_rows(res, want, what="", only=None):
    """res against (ids, dists, layers, ranks, counts): everything, the zeros behind the answers included.  A NaN is compared as a
    NaN (the exact search returns the canonical one, whatever the oracle's payload is).  only: the rows to compare (all)."""
    only = slice(None) if only is None else only
    ids, dists, layers, ranks, counts = [w[only] for w in want[:5]]
    assert np.array_equal(res.counts[only], counts), (what, "counts", res.counts[only][:8], counts[:8])
    assert np.array_equal(res.ids[only], ids), (what, "ids", np.argwhere(res.ids[only] != ids)[:4])
    nan = np.isnan(dists)
    assert np.array_equal(np.isnan(res.dists[only]), nan), (what, "NaN")
    assert np.array_equal(res.dists[only].view(np.uint32)[~nan], dists.view(np.uint32)[~nan]), (what, "f32 bits")
    assert np.array_equal(res.layers[only], layers) and np.array_equal(res.ranks[only], ranks), (what, "p_ids")


def _exact_expected(D, ids, pos, pids, rows_queried, k, allowed_rows=None):
    """from the oracle's n x n matrix D (row i: the distances of point i's vector to every point): per queried row p the candidates
    (allowed_rows or all) other than p, ordered by (distance, DataId, dump position), cut at k"""
    n = len(ids)
    cand = np.arange(n) if allowed_rows is None else np.asarray(allowed_rows, np.int64)
    out = (np.zeros((len(rows_queried), k), np.uint64), np.zeros((len(rows_queried), k), np.float32), np.zeros((len(rows_queried), k), np.uint8),
           np.zeros((len(rows_queried), k), np.int32), np.zeros(len(rows_queried), np.uint32))
    for i, p in enumerate(rows_queried):
        c = cand[cand != p]
        o = c[np.lexsort((pos[c], ids[c], D[p, c]))][:k]
        m = len(o)
        out[0][i, :m], out[1][i, :m] = ids[o], D[p, o] + np.float32(0.0)          # (a -0 distance comes back as +0)
        out[2][i, :m], out[3][i, :m] = [pids[r][0] for r in o], [pids[r][1] for r in o]
        out[4][i] = m
    return out


class _Wide:
    def __init__(self, res):
        self.ids, self.dists, self.layers, self.ranks, self.counts = res.ids, res.dists, res.layers, res.ranks, res.counts


# ----------------------------------------------------------------------------------------------------- 1. exact graph, hand-written dumps
# the issue's dimensions, and DistCosine at d = 30 as well: of 3, 25, 32, 33, 128 none puts the norm into the row's LAST data chunk
# (3, 25, 33: in the padding behind it; 32, 128: in the side array)
SWEEP = [(m, d) for m in F.METRICS for d in (3, 25, 32, 33, 128)] + [("DistCosine", 30)]


@functools.lru_cache(maxsize=2)
def _case(metric, d):
    return Case(metric, d)


def _outside_the_cosine_domain(X):
    """The rows that have a partner row (themselves included) on which the reference's DistCosine panics: it asserts
    dist_unchecked >= -2e-5 (the oracle throws there), and two of the sweep's rows cancel that badly against themselves and each
    other.  The reference defines no distance for such a pair, so the oracle has no expected value for the rows of these points;
    they stay in the index as candidates of every other point -- those pairs are inside the domain -- and their own rows are
    checked against the device's exact search alone.  The oracle's arithmetic (f32 products widened, three f64 sums left to
    right), with half the reference's margin so that no pair near the bound reaches the oracle."""
    with np.errstate(all="ignore"):
        s0 = np.zeros((len(X), len(X)))
        s = np.zeros(len(X))
        for i in range(X.shape[1]):
            s0 = s0 + (X[:, None, i] * X[None, :, i]).astype(np.float64)
            s = s + (X[:, i] * X[:, i]).astype(np.float64)
        du = 1. - s0 / np.sqrt(s[:, None] * s[None, :])
        bad = (s[:, None] > 0) & (s[None, :] > 0) & ~(du >= -0.00001)
    return np.flatnonzero(bad.any(1) | bad.any(0))


@pytest.mark.parametrize("metric,d", SWEEP)
def test_exact_graph_hostile_sweep_bit_exact(native, oracle, tmp_path, metric, d):
    """n = 700: three slabs and 44 tiles, the last of 12 queries; every point is queried (point_ids NULL), so the own row of most
    points lies in another slab than most of its neighbours"""
    case = _case(metric, d)
    h = case.load(native, tmp_path)
    order = dump_order(case.levels)[0]
    pos = np.empty(N, np.int64)
    pos[order] = np.arange(N)
    outside = _outside_the_cosine_domain(case.X) if metric == "DistCosine" else np.zeros(0, np.int64)
    assert len(outside) <= 2 and set(outside.tolist()) <= set(case.hostile.tolist())
    inside = np.setdiff1d(np.arange(N), outside)
    D = np.zeros((N, N), np.float32)
    D[inside] = oracle.dist_matrix(metric, case.X[inside], case.X)
    rows = resolve(case.ids, None)[0]                         # (ids are unique: row i of the answer is the point of the i-th smallest id)
    assert np.array_equal(case.ids[rows], np.sort(case.ids))
    with_oracle = np.flatnonzero(np.isin(rows, inside))
    own = [case.pids[r] for r in rows]
    for k in KS:
        res = h.exact_knn_graph_flat(k)
        _assert_rows(res, _exact_expected(D, case.ids, pos, case.pids, rows, k), f"{metric} d {d} k {k}", with_oracle)
        assert res.counts.tolist() == [min(k, N - 1)] * N
        wide = h.exact_search_flat(case.X[rows], k + 1)       # the device's own exact search of the same vectors, own p_id removed
        _assert_rows(res, apply_drop_self(_Wide(wide), own, k), f"{metric} d {d} k {k} against exact_search_flat")


# ----------------------------------------------------------------------------------------------------- 2. repeated ids, filters, entries
@pytest.fixture(scope="module")
def rep(native, oracle, tmp_path_factory):
    """600 rows, every DataId carried by three of them; of 75 ids the three rows hold ONE vector (test_gpu_exact_knn_hostile's
    construction), permuted, on three layers"""
    n, d, metric = 600, 12, "DistL2"
    rng = np.random.default_rng(41)
    X = uniform(n, d, 42)
    for g in range(75):
        X[3 * g + 1] = X[3 * g + 2] = X[3 * g]
    ids = np.arange(n, dtype=np.uint64) // 3
    perm = rng.permutation(n)
    X, ids = np.ascontiguousarray(X[perm]), ids[perm]
    levels = np.zeros(n, np.int64)
    p = rng.permutation(n)
    levels[p[:150]] = 1
    levels[p[150:200]] = 2
    tmp = tmp_path_factory.mktemp("rep")
    order, pids = write_dump(tmp, "rep", X, ids, levels, metric)
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)
    h = native.HnswIo(tmp, "rep").load_hnsw(metric)
    h.upload(0)
    D = oracle.dist_matrix(metric, X, X)
    return dict(h=h, X=X, ids=ids, pos=pos, pids=pids, D=D, n=n)


def _rows_named(r, pts):
    """the rows that the DataIds pts name: of the three points of an id, the first in dump order"""
    in_dump_order = np.argsort(r["pos"])
    by_pos, unknown = resolve(r["ids"][in_dump_order], pts)
    assert unknown == 0
    return in_dump_order[by_pos]


def test_repeated_ids_and_exact_copies(native, rep):
    """NULL ids: 600 rows in (id, dump order) order, each of the three points of an id with a row of its own.  A point with two
    exact copies gets both back at distance 0, in dump order, and never itself."""
    r = rep
    h, ids, pos, pids, D, n = r["h"], r["ids"], r["pos"], r["pids"], r["D"], r["n"]
    rows = np.lexsort((pos, ids))
    assert np.array_equal(rows, _rows_named(r, None))
    for k in (1, 2, 10, n + 5):
        res = h.exact_knn_graph_flat(k)
        _assert_rows(res, _exact_expected(D, ids, pos, pids, rows, k), f"repeated ids k {k}")
    res = h.exact_knn_graph_flat(2)
    copies = 0
    for i, p in enumerate(rows):
        own = pids[p]
        assert own not in list(zip(res.layers[i].tolist(), res.ranks[i].tolist())), (i, "the point itself")
        if ids[p] < 75:                                       # (by construction: the three rows of these ids hold one vector)
            others = [q for q in np.flatnonzero(ids == ids[p]) if q != p]
            others.sort(key=lambda q: pos[q])
            assert (res.ids[i] == ids[p]).all() and not res.dists[i].any()
            assert list(zip(res.layers[i].tolist(), res.ranks[i].tolist())) == [pids[q] for q in others], (i, "copies in dump order")
            copies += 1
    assert copies == 225
    # an id names the first of its points in dump order; a repeated query gets a row each time
    pts = np.array([3, 74, 75, 199, 3, 3, 150], np.uint64)
    named = _rows_named(r, pts)
    assert all(pos[named[j]] == pos[ids == pts[j]].min() for j in range(len(pts)))
    res = h.exact_knn_graph_flat(7, pts)
    _assert_rows(res, _exact_expected(D, ids, pos, pids, named, 7), "named ids")
    assert np.array_equal(res.ids[0], res.ids[4]) and np.array_equal(res.ranks[0], res.ranks[5])


def test_filter_and_shuffled_subset(native, rep):
    """a filter that allows some queried points and excludes others; point_ids a shuffled subset with duplicates; ids in the
    filter that name no point; the empty filter"""
    r = rep
    h, ids, pos, pids, D, n = r["h"], r["ids"], r["pos"], r["pids"], r["D"], r["n"]
    rng = np.random.default_rng(5)
    allowed_ids = np.sort(rng.choice(200, 90, replace=False).astype(np.uint64))
    allowed_rows = np.flatnonzero(np.isin(ids, allowed_ids))
    pts = rng.choice(200, 70, replace=True).astype(np.uint64)
    assert len(np.unique(pts)) < len(pts) and np.isin(pts, allowed_ids).any() and (~np.isin(pts, allowed_ids)).any()
    named = _rows_named(r, pts)
    with_strangers = np.sort(np.concatenate([allowed_ids, np.array([1000, 10 ** 15], np.uint64)]))
    for k in (1, 5, 269, 300):                                 # 270 rows are allowed: 269 or 270 candidates
        want = _exact_expected(D, ids, pos, pids, named, k, allowed_rows)
        _assert_rows(h.exact_knn_graph_flat(k, pts, with_strangers), want, f"filter k {k}")
        assert set(want[4].tolist()) == ({k} if k < 269 else {269, min(k, 270)})
    res = h.exact_knn_graph_flat(3, pts, np.zeros(0, np.uint64))
    assert not res.counts.any() and not res.ids.any() and not res.dists.any()
    with pytest.raises(native.HnswError) as e:
        h.exact_knn_graph_flat(3, pts, np.array([9, 4], np.uint64))
    assert e.value.code == 1


def test_unknown_id_leaves_the_outputs_untouched(native, rep):
    h = rep["h"]
    NN = native._native
    L = native.lib()
    pts = np.array([3, 200, 5, 10 ** 12, 7], np.uint64)       # ids are 0 .. 199
    for exact in (True, False):
        oi, od = np.full((5, 4), 0xA5A5, np.uint64), np.full((5, 4), -3.0, np.float32)
        ol, orr, oc = np.full((5, 4), 9, np.uint8), np.full((5, 4), -1, np.int32), np.full(5, 77, np.uint32)
        if exact:
            rc = L.hnswgpu_exact_graph_batch(h.handle, _p(pts), 5, 4, None, 0, _p(oi), _p(od), _p(ol), _p(orr), _p(oc))
        else:
            rc = L.hnswgpu_graph_search_batch(h.handle, _p(pts), 5, 4, 16, _p(oi), _p(od), _p(ol), _p(orr), _p(oc))
        assert rc == NN.ERR_ARG and NN.last_error().startswith("2 of the 5"), (rc, NN.last_error())
        assert (oi == 0xA5A5).all() and (od == -3.0).all() and (ol == 9).all() and (orr == -1).all() and (oc == 77).all()


def test_one_point_gives_count_zero(native, tmp_path):
    X = uniform(1, 5, 3)
    write_dump(tmp_path, "one", X, np.array([42], np.uint64), np.zeros(1, np.int64), "DistL2")
    h = native.HnswIo(tmp_path, "one").load_hnsw("DistL2")
    h.upload(0)
    for res in (h.exact_knn_graph_flat(3), h.exact_knn_graph_flat(3, [42, 42])):
        assert not res.counts.any() and not res.ids.any() and not res.dists.any() and not res.ranks.any()


def test_device_entries_on_a_stream(native, rep):
    """the exact _device entry with torch buffers on a stream of the caller's, ids and filter resident: the host entry's answers;
    NULL layer / rank arrays; an unknown id leaves the device arrays untouched"""
    _device_entries(native, rep["h"], rep["n"], np.arange(200, dtype=np.uint64), True)


def test_approximate_device_entry_on_a_stream(native, built):
    """the same for the approximate entry, on a built index"""
    _device_entries(native, built["h"], built["n"], built["ids"], False)


def _device_entries(native, h, n, pool, exact):
    import torch
    NN = native._native
    L = native.lib()
    pts = np.random.default_rng(8).choice(pool, 50).astype(np.uint64)
    allowed = np.sort(np.random.default_rng(9).choice(pool, 60, replace=False).astype(np.uint64))
    stream = torch.cuda.Stream()
    k = 6

    def bufs(np_):
        b = (torch.full((np_, k), -1, dtype=torch.int64, device="cuda"), torch.full((np_, k), -1.0, dtype=torch.float32, device="cuda"),
             torch.full((np_, k), 9, dtype=torch.uint8, device="cuda"), torch.full((np_, k), -1, dtype=torch.int32, device="cuda"),
             torch.full((np_,), -1, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        return b

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def same(b, want, pids=True):
        assert np.array_equal(b[0].cpu().numpy().astype(np.uint64), want.ids) and np.array_equal(b[4].cpu().numpy().astype(np.uint32), want.counts)
        assert np.array_equal(b[1].cpu().numpy().view(np.uint32), want.dists.view(np.uint32))
        if pids:
            assert np.array_equal(b[2].cpu().numpy(), want.layers) and np.array_equal(b[3].cpu().numpy(), want.ranks)
        else:
            assert (b[2] == 9).all() and (b[3] == -1).all()
    dpts = torch.from_numpy(pts.astype(np.int64)).cuda()
    dal = torch.from_numpy(allowed.astype(np.int64)).cuda()
    for p_np, p_dev, np_ in ((pts, dpts, len(pts)), (None, None, n)):
        for al_np, al_dev in ((None, None), (allowed, dal)) if exact else ():
            for with_pids in (True, False):
                b = bufs(np_)
                rc = L.hnswgpu_exact_graph_batch_device(h.handle, ptr(p_dev), np_, k, ptr(al_dev), 0 if al_np is None else len(al_np), ptr(b[0]), ptr(b[1]),
                                                        ptr(b[2]) if with_pids else None, ptr(b[3]) if with_pids else None, ptr(b[4]),
                                                        C.c_void_p(stream.cuda_stream))
                assert rc == NN.OK, NN.last_error()
                same(b, h.exact_knn_graph_flat(k, p_np, al_np), with_pids)
        for with_pids in () if exact else (True, False):
            b = bufs(np_)
            rc = L.hnswgpu_graph_search_batch_device(h.handle, ptr(p_dev), np_, k, 32, ptr(b[0]), ptr(b[1]), ptr(b[2]) if with_pids else None,
                                                     ptr(b[3]) if with_pids else None, ptr(b[4]), C.c_void_p(stream.cuda_stream))
            assert rc == NN.OK, NN.last_error()
            same(b, h.knn_graph_flat(k, 32, p_np), with_pids)
    bad = torch.from_numpy(np.array([int(pool[0]), int(pool[1]), int(pool.max()) + 1], np.int64)).cuda()
    b = bufs(3)
    if exact:
        rc = L.hnswgpu_exact_graph_batch_device(h.handle, ptr(bad), 3, k, None, 0, *[ptr(t) for t in b], C.c_void_p(stream.cuda_stream))
    else:
        rc = L.hnswgpu_graph_search_batch_device(h.handle, ptr(bad), 3, k, 32, *[ptr(t) for t in b], C.c_void_p(stream.cuda_stream))
    assert rc == NN.ERR_ARG and NN.last_error().startswith("1 of the 3")
    assert (b[0] == -1).all() and (b[1] == -1.0).all() and (b[2] == 9).all() and (b[3] == -1).all() and (b[4] == -1).all()


def test_two_threads_on_one_handle(native, built):
    h = built["h"]
    pts = {"a": built["ids"][::7].copy(), "b": None}
    want = {name: (h.exact_knn_graph_flat(9, p), h.knn_graph_flat(9, 32, p)) for name, p in pts.items()}
    out, errs = {}, []

    def run(name):
        try:
            out[name] = [(h.exact_knn_graph_flat(9, pts[name]), h.knn_graph_flat(9, 32, pts[name])) for _ in range(4)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=(name,)) for name in pts]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for name in pts:
        for got in out[name]:
            for g, w in zip(got, want[name]):
                _assert_rows(g, (w.ids, w.dists, w.layers, w.ranks, w.counts), name)


# ----------------------------------------------------------------------------------------------------- 3. approximate graph, built indexes
def _planted(n, d, seed):
    """40 groups of 14 exact copies among n rows: with k = 10 a point of a group finds 11 others of its group at distance 0, so
    its own entry can be missing from a (k + 1)-wide answer"""
    X = uniform(n, d, seed)
    rows = np.random.default_rng(seed).permutation(n)[:40 * 14].reshape(40, 14)
    for g in rows:
        X[g] = X[g[0]]
    return X


SHAPES = {"l2": ("DistL2", 2000, 25, 8, None), "cosine": ("DistCosine", 3000, 8, 12, None), "copies": ("DistL2", 1500, 8, 12, _planted)}


@pytest.fixture(scope="module", params=list(SHAPES))
def built(request, native, oracle, tmp_path_factory):
    """an index built by the oracle, dumped and loaded by the product (both sides walk the same graph); the oracle's (k + 1)-wide
    answers for every stored vector, computed once; every point's own p_id from the exact search under a filter of its own id"""
    metric, n, d, m, gen = SHAPES[request.param]
    X = gen(n, d, 77) if gen else uniform(n, d, 77)
    ids = np.random.default_rng(n).permutation(n).astype(np.uint64) * 2 + 10
    o = oracle.OracleHnsw(m, n, 16, 48, metric)
    o.insert_batch(X, ids)
    tmp = tmp_path_factory.mktemp("built")
    o.file_dump(str(tmp), "g")
    h = native.HnswIo(str(tmp), "g").load_hnsw(metric)
    h.upload(0)
    me = h.exact_search_filters_flat(X, 1, [np.array([v], np.uint64) for v in ids])
    assert me.counts.tolist() == [1] * n and np.array_equal(me.ids[:, 0], ids)
    own = list(zip(me.layers[:, 0].tolist(), me.ranks[:, 0].tolist()))
    assert len(set(own)) == n
    k, ef = 10, 40
    ref = o.parallel_search(X, k + 1, ef)
    return dict(name=request.param, h=h, o=o, X=X, ids=ids, own=own, k=k, ef=ef, ref=ref, n=n)


def _subset(b, rows):
    class R:
        pass
    r = R()
    ref = b["ref"]
    r.ids, r.dists, r.layers, r.ranks, r.counts = ref.ids[rows], ref.dists[rows], ref.layers[rows], ref.ranks[rows], ref.counts[rows]
    return r


def test_approximate_graph_is_the_search_without_the_point(native, built, knob):
    """every point (NULL ids) and an explicit permutation of all ids, in one chunk and in three (HNSWGPU_GRAPH_CHUNK = ceil(n / 3)
    + 33: the last one partial), strict ties on: the oracle's search with the rule, and the device's own search with the rule"""
    b = built
    h, X, ids, own, k, ef, n = b["h"], b["X"], b["ids"], b["own"], b["k"], b["ef"], b["n"]
    rows_all = np.argsort(ids)                                # (ids are unique: NULL ids give the points by ascending id)
    perm = np.random.default_rng(4).permutation(n)
    want_all = apply_drop_self(_subset(b, rows_all), [own[r] for r in rows_all], k)
    absent = want_all[5]
    if b["name"] == "copies":
        assert len(absent) >= 40, len(absent)                 # the precondition, on the ORACLE's answers: rows without an own entry ...
        assert any(b["ref"].counts[rows_all[i]] == k + 1 for i in absent)
    assert len(absent) < n                                    # ... and rows with one
    want_perm = apply_drop_self(_subset(b, perm), [own[r] for r in perm], k)
    chunk = (n + 2) // 3 + 33
    assert 2 * chunk < n < 3 * chunk
    for c in (None, chunk):
        knob("HNSWGPU_GRAPH_CHUNK", c)
        _assert_rows(h.knn_graph_flat(k, ef), want_all, f"{b['name']} NULL ids chunk {c}")
        _assert_rows(h.knn_graph_flat(k, ef, ids[perm]), want_perm, f"{b['name']} permutation chunk {c}")
    knob("HNSWGPU_GRAPH_CHUNK", None)
    wide = h.parallel_search_flat(X[perm], k + 1, ef)
    _assert_rows(h.knn_graph_flat(k, ef, ids[perm]), apply_drop_self(_Wide(wide), [own[r] for r in perm], k), f"{b['name']} device search")


def test_approximate_graph_with_strict_ties_off(native, built, knob):
    """the index's tie setting is the search's: with strict ties off the graph is the lean search's answer with the rule, whole
    and in three chunks"""
    b = built
    h, X, ids, own, k, ef, n = b["h"], b["X"], b["ids"], b["own"], b["k"], b["ef"], b["n"]
    pts = np.random.default_rng(6).permutation(n)[:n // 2]
    h.set_strict_ties(False)
    try:
        wide = h.parallel_search_flat(X[pts], k + 1, ef)
        want = apply_drop_self(_Wide(wide), [own[r] for r in pts], k)
        for c in (None, (len(pts) + 2) // 3 + 7):
            knob("HNSWGPU_GRAPH_CHUNK", c)
            _assert_rows(h.knn_graph_flat(k, ef, ids[pts]), want, f"{b['name']} lean chunk {c}")
    finally:
        h.set_strict_ties(True)
        knob("HNSWGPU_GRAPH_CHUNK", None)


def test_recall_is_the_recall_of_the_two_flat_results(native, built):
    b = built
    h, ids, k, ef, n = b["h"], b["ids"], b["k"], b["ef"], b["n"]
    from hnsw_rs_amd.api import _recall
    pts = ids[np.random.default_rng(2).permutation(n)[:300]]
    for p in (pts, None):
        got, exact = h.knn_graph_flat(k, ef, p), h.exact_knn_graph_flat(k, p)
        want = _recall(got, exact)[1]
        by_hand = sum(len(np.intersect1d(got.ids[i, :got.counts[i]], exact.ids[i, :exact.counts[i]])) for i in range(len(exact.counts))) / exact.counts.sum()
        assert h.knn_graph_recall(k, ef, p) == want == by_hand and 0.5 < want <= 1.0
