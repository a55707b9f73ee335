"""Exact range search on the device (Hnsw.exact_range_search_flat -> hnswgpu_exact_range_search_batch, csrc/exact_range.hip): every
eligible point with dist(q, p) <= radii[q], ascending by (distance, origin id), in CSR form.
The expected answer never comes from the code under test: D = oracle_lib.dist_matrix(metric, Q, X) (the CPU oracle's
Distance::eval), the eligible rows with D[q] <= radii[q] as f32 values, ordered by np.lexsort((ids, D[q])); every comparison is
exact (offsets, ids, f32 bit patterns, p_ids).  What the inputs must contain for a test to mean anything is asserted on the
ORACLE's matrix, never on device output."""
import ctypes as C
import threading

import numpy as np
import pytest

import f64_reference as F
from conftest import uniform
from test_gpu_exact_knn import CASES, _build, _gen
from test_gpu_exact_knn_hostile import N as HN, Case, _f64_violations

pytestmark = pytest.mark.gpu
FLT_MAX = np.float32(np.finfo(np.float32).max)
INF = np.float32(np.inf)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _expected(D, ids, radii, rows=None):
    """(offsets, per query the rows of its answer in order) from the oracle's matrix"""
    ids = np.asarray(ids, np.uint64)
    rows = np.arange(D.shape[1]) if rows is None else np.asarray(rows, np.int64)
    want = []
    with np.errstate(invalid="ignore"):
        for q in range(D.shape[0]):
            hit = rows[D[q, rows] <= radii[q]]                      # (IEEE: a NaN on either side is no hit)
            want.append(hit[np.lexsort((ids[hit], D[q, hit]))])     # (-0 == +0 for the sort: the id decides)
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in want])]).astype(np.uint64)
    return offsets, want


def _assert_range(res, D, ids, radii, rows=None, pids=None, what=""):
    ids = np.asarray(ids, np.uint64)
    offsets, want = _expected(D, ids, radii, rows)
    assert res.offsets.dtype == np.uint64 and np.array_equal(res.offsets, offsets), (what, res.offsets[:8], offsets[:8])
    assert len(res.ids) == len(res.dists) == len(res.layers) == len(res.ranks) == int(offsets[-1]), what
    for q in range(D.shape[0]):
        g_ids, g_d, g_l, g_r = res.of(q)
        assert np.array_equal(g_ids, ids[want[q]]), (what, q, g_ids[:8], ids[want[q]][:8])
        w = D[q, want[q]] + np.float32(0.0)                         # a -0 distance comes back as +0
        assert np.array_equal(g_d.view(np.uint32), w.view(np.uint32)), (what, q)
        if pids is not None:
            assert list(zip(g_l.tolist(), g_r.tolist())) == [pids[r] for r in want[q]], (what, q, "p_ids")
    return offsets, want


def _kth(D, q, j):
    """the query's exact j-th smallest oracle distance (NaN sorts last)"""
    return np.sort(D[q])[min(j, D.shape[1]) - 1]


def _cycled_radii(D, start=0):
    """per query, in turn (from kind `start` on): its j-th smallest distance for j in 1, 10, 64, 65, 1000 (the boundary is included), nextafter below
    each (excluded), a value below its minimum, a value above every finite distance, +inf"""
    kinds = [("at", j) for j in (1, 10, 64, 65, 1000)] + [("below", j) for j in (1, 10, 64, 65, 1000)] + [("none", 0), ("all", 0), ("inf", 0)]
    finite_max = np.float32(D[np.isfinite(D)].max())
    radii, kind_of = np.zeros(D.shape[0], np.float32), []
    for q in range(D.shape[0]):
        kind, j = kinds[(q + start) % len(kinds)]
        if kind == "at":
            r = _kth(D, q, j)
        elif kind == "below":
            r = np.nextafter(_kth(D, q, j), -INF)
        elif kind == "none":
            r = np.nextafter(np.nanmin(D[q]), -INF)
        elif kind == "all":
            r = np.nextafter(finite_max, INF)
        else:
            r = INF
        radii[q] = r
        kind_of.append(kind)
    return radii, kind_of


# ----------------------------------------------------------------------------------------------------- 1. built indexes
RANGE_CASES = [("DistL2", 128), ("DistCosine", 30), ("DistCosine", 25), ("DistDot", 100), ("DistL1", 130), ("DistHellinger", 33),
               ("DistJeffreys", 31), ("DistJensenShannon", 32)]
assert all(c in CASES for c in RANGE_CASES) and {m for m, _ in RANGE_CASES} == set(F.METRICS)
assert {25, 30, 31, 32, 33, 128, 130} <= {d for _, d in RANGE_CASES}


def _built_case(native, oracle, metric, d):
    """n = 2500 (no multiple of 64 or of a slab), 37 queries (two tiles and a part); rows 1500 .. 2499 are exact copies of rows
    0 .. 999, so a radius equal to one of their distances is a tie on the boundary"""
    n, nq = 2500, 37
    X, Q = _gen(metric)(n, d, 21), _gen(metric)(nq, d, 22)
    X[1500:] = X[:1000]
    Q[:3] = X[5:8]
    ids = np.random.default_rng(d).permutation(n).astype(np.uint64) * 3 + 1
    h = _build(native, X, metric, ids)
    D = oracle.dist_matrix(metric, Q, X)
    radii, kinds = _cycled_radii(D)
    return h, X, Q, ids, D, radii, kinds


@pytest.mark.parametrize("metric,d", RANGE_CASES)
def test_all_metrics_bit_exact(native, oracle, metric, d):
    h, X, Q, ids, D, radii, kinds = _built_case(native, oracle, metric, d)
    n = len(X)
    with np.errstate(invalid="ignore"):
        counts = (D <= radii[:, None]).sum(1)
        assert (counts == 0).any() and (counts == n).any(), counts
        ties = [q for q in range(len(Q)) if kinds[q] == "at" and (D[q] == radii[q]).sum() >= 2]
    assert ties, "no radius equal to a distance that two rows share"
    res = h.exact_range_search_flat(Q, radii)
    _assert_range(res, D, ids, radii, what=f"{metric} d {d}")
    nb = h.exact_range_search(Q[:2], radii[:2])
    assert [len(x) for x in nb] == counts[:2].tolist() and all(isinstance(x, native.Neighbour) for x in nb[0])
    s = np.sort(D, axis=1)
    checked = 0
    for k in (1, 10, 100):                        # a prefix of the range answer is the exact k-NN answer restricted to the ball
        knn = h.exact_search_flat(Q, k)
        for q in range(len(Q)):
            g_ids, g_d, g_l, g_r = res.of(q)
            m = min(k, len(g_ids))
            if s[q, k - 1] <= radii[q]:
                assert m == k
                checked += 1
            assert np.array_equal(g_ids[:m], knn.ids[q, :m]) and np.array_equal(g_d[:m].view(np.uint32), knn.dists[q, :m].view(np.uint32)), (k, q)
            assert np.array_equal(g_l[:m], knn.layers[q, :m]) and np.array_equal(g_r[:m], knn.ranks[q, :m]), (k, q)
    assert checked > 30


# ----------------------------------------------------------------------------------------------------- 2. small n
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_small_indexes_and_query_counts(native, oracle, n):
    X = uniform(n, 8, n)
    ids = np.arange(n, dtype=np.uint64)[::-1].copy() + 7
    h = _build(native, X, "DistL2", ids)
    for nq in (1, 16, 17):
        Q = uniform(nq, 8, 100 + nq)
        Q[0] = X[n // 2]
        D = oracle.dist_matrix("DistL2", Q, X)
        for start in (range(13) if nq == 1 else (0, 7)):     # every kind of radius, whatever nq is
            r, _ = _cycled_radii(D, start)
            _assert_range(h.exact_range_search_flat(Q, r), D, ids, r, what=f"n {n} nq {nq} start {start}")
        _assert_range(h.exact_range_search_flat(Q, float("inf")), D, ids, np.full(nq, INF), what=f"n {n} nq {nq} scalar inf")


# ----------------------------------------------------------------------------------------------------- 3. hostile values
def _median_radii(D):
    return np.array([np.sort(D[q])[D.shape[1] // 2] for q in range(D.shape[0])], np.float32)


@pytest.mark.parametrize("d", (1, 31, 32, 128, 784))
@pytest.mark.parametrize("metric", F.METRICS)
def test_hostile_values(native, oracle, tmp_path, metric, d):
    """700 rows and 37 queries of the hostile sweep, loaded from a hand-written dump: NaN-distance rows never appear, +inf rows
    only under a +inf radius, a -0 distance comes back as +0, p_ids are the writer's, and under radius +inf the returned distances
    lie within the float64 bound"""
    case = Case(metric, d)
    h = case.load(native, tmp_path)
    D = oracle.dist_matrix(metric, case.Q, case.X)
    nq = len(case.Q)
    for name, r in (("+inf", INF), ("NaN", np.float32(np.nan)), ("-0", np.float32(-0.0)), ("0", np.float32(0.0)), ("-1", np.float32(-1.0)),
                    ("FLT_MAX", FLT_MAX), ("median", None)):
        radii = _median_radii(D) if r is None else np.full(nq, r, np.float32)
        res = h.exact_range_search_flat(case.Q, radii if r is None else float(r))
        _assert_range(res, D, case.ids, radii, pids=case.pids, what=f"{metric} d {d} radius {name}")
        assert not np.isnan(res.dists).any(), name
        assert not (res.dists.view(np.uint32) == 0x80000000).any(), (name, "a -0 distance")
        for q in range(nq):
            if not radii[q] == INF:
                assert not np.isinf(res.of(q)[1]).any(), (name, q, "a +inf distance under a finite radius")
        if name in ("NaN", "-1"):
            assert len(res.ids) == 0, name
        if name == "+inf":
            row_of = np.array([case.row_of_id[int(v)] for v in res.ids], np.int64)
            got = np.full(D.shape, np.nan, np.float32)               # the rows left out: a NaN distance, by the oracle
            for q in range(nq):
                a, b = int(res.offsets[q]), int(res.offsets[q + 1])
                got[q, row_of[a:b]] = res.dists[a:b]
            assert np.array_equal(np.isnan(got), np.isnan(D))
            bad, _ = _f64_violations(case, got)
            assert not bad, (metric, d, bad[:4])


# ----------------------------------------------------------------------------------------------------- 4. filters
@pytest.mark.parametrize("metric,d", [("DistL2", 32), ("DistCosine", 31), ("DistJensenShannon", 128)])
def test_filters_over_hostile_rows(native, oracle, tmp_path, metric, d):
    case = Case(metric, d)
    h = case.load(native, tmp_path)
    D = oracle.dist_matrix(metric, case.Q, case.X)
    nq = len(case.Q)
    med = _median_radii(D)
    radii = np.array([(INF, med[q], FLT_MAX)[q % 3] for q in range(nq)], np.float32)
    rng = np.random.default_rng(19)
    no_point = np.array([2, 3, 10 ** 15], np.uint64)                 # (ids are 3 i + 1)
    for name, rows in (("dense", np.sort(rng.choice(HN, 630, replace=False))), ("1 %", np.sort(rng.choice(case.hostile, 7, replace=False))),
                       ("empty", np.zeros(0, np.int64))):
        for extra in (np.zeros(0, np.uint64), no_point):
            allowed = np.sort(np.concatenate([case.ids[rows], extra]))
            res = h.exact_range_search_flat(case.Q, radii, allowed)
            offsets, _ = _assert_range(res, D, case.ids, radii, rows, pids=case.pids, what=f"{metric} filter {name}")
            assert (offsets[-1] == 0) == (name == "empty")
    with pytest.raises(native.HnswError) as e:
        h.exact_range_search_flat(case.Q, radii, np.array([9, 4], np.uint64))     # unsorted
    assert e.value.code == 1


# ----------------------------------------------------------------------------------------------------- 5. - 8. one built index
@pytest.fixture(scope="module")
def built(native, oracle):
    return _built_case(native, oracle, "DistL2", 33)


def _raw_call(native, h, Q, radii, cap, with_out=True, sentinel=0xA5):
    """the host entry itself: (rc, offsets, ids, dists, layers, ranks), the out arrays pre-filled with a sentinel byte"""
    nq, d = Q.shape
    offs = np.full(nq + 1, 0x5A5A5A5A, np.uint64)
    outs = [np.frombuffer(bytes([sentinel]) * (max(cap, 1) * w), dtype=t).copy() for w, t in ((8, np.uint64), (4, np.float32), (1, np.uint8), (4, np.int32))]
    ptrs = [_p(o) if with_out else None for o in outs]
    rc = native.lib().hnswgpu_exact_range_search_batch(h.handle, _p(Q), nq, d, _p(radii), None, 0, cap, _p(offs), *ptrs)
    return rc, offs, outs


def test_capacity(native, built):
    h, X, Q, ids, D, radii, _ = built
    N = native._native
    offsets, want = _expected(D, ids, radii)
    total = int(offsets[-1])
    rc, offs, outs = _raw_call(native, h, Q, radii, total - 1)
    assert rc == N.ERR_CAPACITY and str(total) in N.last_error(), (rc, N.last_error())
    assert np.array_equal(offs, offsets)                               # complete, whatever the capacity
    for o in outs:
        assert (o.view(np.uint8) == 0xA5).all()                        # no out slot was touched
    rc, offs, outs = _raw_call(native, h, Q, radii, total)
    assert rc == N.OK, N.last_error()
    assert np.array_equal(offs, offsets) and np.array_equal(outs[0], np.concatenate([ids[w] for w in want]))
    rc, offs, outs = _raw_call(native, h, Q, radii, 0, with_out=False)   # count only
    assert rc == N.ERR_CAPACITY and np.array_equal(offs, offsets)
    none = np.full(len(Q), -1.0, np.float32)
    rc, offs, outs = _raw_call(native, h, Q, none, 0, with_out=False)    # ... of a batch without answers: nothing is missing
    assert rc == N.OK and not offs.any()
    res = h.exact_range_search_flat(Q, radii)                            # the Python method: a guess, then the exact total
    assert total > max(1024, 32 * len(Q)) and np.array_equal(res.offsets, offsets) and len(res.ids) == total


def test_fill_pass_in_chunks(native, built, knob):
    """HNSWGPU_RANGE_HITS_PER_PASS below one query's answer and at about a third of the total: the plan takes several turns, a
    query larger than the budget gets a pass of its own, the answers do not change"""
    h, X, Q, ids, D, radii, _ = built
    base = h.exact_range_search_flat(Q, radii)
    offsets, _ = _assert_range(base, D, ids, radii, what="unhooked")
    total, largest = int(offsets[-1]), int(np.diff(offsets).max())
    assert largest == len(X)
    for budget in (largest // 50, 1, total // 3):
        knob("HNSWGPU_RANGE_HITS_PER_PASS", budget)
        res = h.exact_range_search_flat(Q, radii)
        assert np.array_equal(res.offsets, base.offsets) and np.array_equal(res.ids, base.ids), budget
        assert np.array_equal(res.dists.view(np.uint32), base.dists.view(np.uint32)), budget
        assert np.array_equal(res.layers, base.layers) and np.array_equal(res.ranks, base.ranks), budget
    knob("HNSWGPU_RANGE_HITS_PER_PASS", None)


def test_long_batches_are_cut_into_chunks(native, oracle, knob):
    """130 000 queries of d = 128 on 64 points: 66 MB of queries are more than the host entry stages at once (128 070 queries), and
    a block's 8 005 tiles are more than one chunk of the count pass holds (7 883) -- both loops take a second turn; checked with
    the default budget and with one that cuts the fill pass as well"""
    n, d, nq = 64, 128, 130_000
    X, Q = uniform(n, d, 211), uniform(nq, d, 212)
    ids = np.random.default_rng(9).permutation(n).astype(np.uint64) + 11
    h = _build(native, X, "DistL2", ids)
    D = oracle.dist_matrix("DistL2", Q, X)
    assert (D > 0).all()
    s = np.sort(D, axis=1)
    radii = np.where(np.arange(nq) % 4 == 0, s[:, 0], np.where(np.arange(nq) % 4 == 1, s[:, 2], np.where(np.arange(nq) % 4 == 2, 0.0, s[:, 63])))
    radii = radii.astype(np.float32)
    radii[1000:3000] = 0.0                                               # a run of empty answers
    hit = D <= radii[:, None]
    offsets = np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.uint64)
    key = (D.view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[None, :]      # (distances > 0: the bit patterns order them)
    key[~hit] = np.uint64(0xFFFFFFFFFFFFFFFF)
    order = np.argsort(key, axis=1, kind="stable")
    keep = np.take_along_axis(hit, order, 1)
    want_ids = ids[order][keep]
    want_d = np.take_along_axis(D, order, 1)[keep]
    assert int(offsets[-1]) == len(want_ids) and (np.diff(offsets) == 0).any() and (np.diff(offsets) == n).any()
    for budget in (None, 100_000):
        knob("HNSWGPU_RANGE_HITS_PER_PASS", budget)
        res = h.exact_range_search_flat(Q, radii)
        assert np.array_equal(res.offsets, offsets), budget
        assert np.array_equal(res.ids, want_ids) and np.array_equal(res.dists.view(np.uint32), want_d.view(np.uint32)), budget
    knob("HNSWGPU_RANGE_HITS_PER_PASS", None)


def test_device_entry_on_a_stream(native, built):
    """hnswgpu_exact_range_search_batch_device with torch buffers on a stream of the caller's, radii and filter resident on the
    device: HNSWGPU_ERR_CAPACITY leaves complete offsets and untouched out arrays, the exact capacity gives the oracle's answer"""
    import torch
    h, X, Q, ids, D, radii, _ = built
    N = native._native
    L = native.lib()
    nq, d = Q.shape
    rows = np.sort(np.random.default_rng(13).choice(len(X), 900, replace=False))
    allowed = np.sort(ids[rows])
    dq, dr = torch.from_numpy(Q).cuda(), torch.from_numpy(radii).cuda()
    dal = torch.from_numpy(allowed.astype(np.int64)).cuda()
    stream = torch.cuda.Stream()
    for al, al_rows in ((None, None), (dal, rows)):
        offsets, want = _expected(D, ids, radii, al_rows)
        total = int(offsets[-1])
        for cap, with_pids in ((total - 1, True), (total, True), (total + 5, False), (0, False)):
            o_off = torch.full((nq + 1,), -1, dtype=torch.int64, device="cuda")
            o_ids = torch.full((cap + 1,), -1, dtype=torch.int64, device="cuda")
            o_d = torch.full((cap + 1,), -1.0, dtype=torch.float32, device="cuda")
            o_l = torch.full((cap + 1,), 9, dtype=torch.uint8, device="cuda")
            o_r = torch.full((cap + 1,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            count_only = cap == 0
            rc = L.hnswgpu_exact_range_search_batch_device(
                h.handle, C.c_void_p(dq.data_ptr()), nq, d, C.c_void_p(dr.data_ptr()), C.c_void_p(al.data_ptr()) if al is not None else None,
                0 if al is None else len(allowed), cap, C.c_void_p(o_off.data_ptr()), None if count_only else C.c_void_p(o_ids.data_ptr()),
                None if count_only else C.c_void_p(o_d.data_ptr()), C.c_void_p(o_l.data_ptr()) if with_pids else None,
                C.c_void_p(o_r.data_ptr()) if with_pids else None, C.c_void_p(stream.cuda_stream))
            assert np.array_equal(o_off.cpu().numpy().astype(np.uint64), offsets), cap
            if cap < total:
                assert rc == N.ERR_CAPACITY and str(total) in N.last_error()
                assert (o_ids == -1).all() and (o_d == -1.0).all() and (o_l == 9).all() and (o_r == -1).all()
                continue
            assert rc == N.OK, N.last_error()
            w = np.concatenate(want)
            assert np.array_equal(o_ids.cpu().numpy()[:total].astype(np.uint64), ids[w])
            assert np.array_equal(o_d.cpu().numpy()[:total].view(np.uint32), np.concatenate([D[q, want[q]] for q in range(nq)]).view(np.uint32))
            assert (o_ids[total:] == -1).all() and (o_d[total:] == -1.0).all()          # nothing behind the answers
            host = h.exact_range_search_flat(Q, radii, None if al is None else allowed)
            if with_pids:
                assert np.array_equal(o_l.cpu().numpy()[:total], host.layers) and np.array_equal(o_r.cpu().numpy()[:total], host.ranks)
            else:
                assert (o_l == 9).all() and (o_r == -1).all()


def test_two_threads_on_one_handle(native, built):
    h, X, Q, ids, D, radii, _ = built
    other = np.roll(radii, 5)
    want = {"a": h.exact_range_search_flat(Q, radii), "b": h.exact_range_search_flat(Q, other)}
    _assert_range(want["a"], D, ids, radii, what="single-threaded a")
    _assert_range(want["b"], D, ids, other, what="single-threaded b")
    out, errs = {}, []

    def run(name, r):
        try:
            out[name] = [h.exact_range_search_flat(Q, r) for _ in range(4)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=("a", radii)), threading.Thread(target=run, args=("b", other))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for name in ("a", "b"):
        for r in out[name]:
            assert np.array_equal(r.offsets, want[name].offsets) and np.array_equal(r.ids, want[name].ids)
            assert np.array_equal(r.dists.view(np.uint32), want[name].dists.view(np.uint32))
            assert np.array_equal(r.layers, want[name].layers) and np.array_equal(r.ranks, want[name].ranks)
