"""Exhaustive exact k-NN on the device (Hnsw.exact_search_flat -> hnswgpu_exact_search_batch, csrc/exact_knn.hip).
The expected answer never comes from the code under test: D = oracle_lib.dist_matrix(metric, Q, X) (the CPU oracle's
Distance::eval), order = np.lexsort((origin_ids, D[q]))[:k]; every comparison is exact (ids, f32 bit patterns, counts, p_ids)
unless it says otherwise.  The f64 reference (tests/f64_reference.py) checks the same answers sharing nothing with the oracle.
Every input here is benign (uniform, normalised, probability vectors) and every index is built.  Hostile values -- subnormals,
magnitudes mixed over 2^-60 .. 2^60, overflowing sums, +inf tie groups, NaN distances -- and repeated origin ids live in
tests/test_gpu_exact_knn_hostile.py, on indexes loaded from hand-written dumps (tests/dump_writer.py): the builder refuses such rows."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import f64_reference as F
from conftest import normalized, probability, uniform

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gen(metric):
    return {"DistDot": normalized}.get(metric, probability if metric in F.PROBABILITY_METRICS else uniform)


def _build(native, X, metric, ids=None, nthreads=1, m=8, efc=24):
    h = native.Hnsw(m, len(X), 16, efc, metric)
    h.set_build_options(nthreads=nthreads)
    h.parallel_insert(X, ids)
    h.upload(0)
    return h


def _assert_answers(oracle, metric, res, Q, X, ids, k, rows=None, what=""):
    """res against the lexsort of the oracle's distances by (distance, origin id), restricted to `rows` (the allowed rows)"""
    ids = np.asarray(ids, np.uint64)
    rows = np.arange(len(X)) if rows is None else np.asarray(rows, np.int64)
    D = oracle.dist_matrix(metric, Q, X)
    want_c = min(k, len(rows))
    assert res.counts.tolist() == [want_c] * len(Q), (what, res.counts[:8])
    for q in range(len(Q)):
        order = rows[np.lexsort((ids[rows], D[q, rows]))][:k]
        assert np.array_equal(res.ids[q, :want_c], ids[order]), (what, q, res.ids[q, :8], ids[order][:8])
        got, want = res.dists[q, :want_c], D[q, order]
        nan = np.isnan(want)          # (a NaN comes back as a NaN: its sign and payload are the machine's, not the contract's)
        assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), (what, q)
        assert np.isnan(got[nan]).all(), (what, q, "NaN")
        assert not res.ids[q, want_c:].any() and not res.dists[q, want_c:].view(np.uint32).any(), (what, q, "slots behind the answers")
        assert not res.layers[q, want_c:].any() and not res.ranks[q, want_c:].any(), (what, q)


def _assert_pids(h, res):
    origin = F.GraphWalk(h).origin
    seen = 0
    for q in range(len(res.counts)):
        for j in range(int(res.counts[q])):
            pid = (int(res.layers[q, j]), int(res.ranks[q, j]))
            if pid in origin:
                assert origin[pid] == int(res.ids[q, j]), (q, j, pid)
                seen += 1
    assert seen > 0


CASES = [("DistL2", 128), ("DistL2", 1), ("DistL2", 784), ("DistL2", 33), ("DistCosine", 25), ("DistCosine", 30), ("DistCosine", 31),
         ("DistCosine", 32), ("DistCosine", 126), ("DistCosine", 130), ("DistDot", 100), ("DistDot", 3), ("DistL1", 130), ("DistL1", 25),
         ("DistHellinger", 33), ("DistHellinger", 100), ("DistJeffreys", 31), ("DistJeffreys", 128), ("DistJensenShannon", 32),
         ("DistJensenShannon", 3)]


@pytest.mark.parametrize("metric,d", CASES)
def test_all_metrics_bit_exact(native, oracle, metric, d):
    """n = 2500 (no multiple of the 64-row step or of a slab), 37 queries (two tiles of 16 and a part), k from 1 to n + 5; d over
    the residues of the row stride, DistCosine with the norm in the row's padding (25, 130), in the row's LAST chunk (30, 126)
    and in the side array (31, 32)"""
    n, nq = 2500, 37
    X, Q = _gen(metric)(n, d, 21), _gen(metric)(nq, d, 22)
    Q[:3] = X[5:8]
    ids = np.random.default_rng(d).permutation(n).astype(np.uint64) * 3 + 1
    h = _build(native, X, metric, ids)
    for k in (1, 10, 100, 1024, n + 5):
        res = h.exact_search_flat(Q, k)
        _assert_answers(oracle, metric, res, Q, X, ids, k, what=f"{metric} d {d} k {k}")
        if k == 10 and d in (128, 25, 3):
            _assert_pids(h, res)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_small_indexes_and_query_counts(native, oracle, n):
    X = uniform(n, 8, n)
    ids = np.arange(n, dtype=np.uint64)[::-1].copy() + 7
    h = _build(native, X, "DistL2", ids)
    for nq in (1, 16, 48, 50):
        Q = uniform(nq, 8, 100 + nq)
        for k in (1, 10, n + 5):
            _assert_answers(oracle, "DistL2", h.exact_search_flat(Q, k), Q, X, ids, k, what=f"n {n} nq {nq} k {k}")


def _golden(native, name):
    h = native.HnswIo(GOLD, name).load_hnsw()
    dm = native.DataMap.from_hnswdump(GOLD, name)
    ids = np.asarray(dm.get_dataid_iter(), np.uint64)
    X = np.stack([np.array(dm.get_data(i)) for i in ids]).astype(np.float32)
    return h, X, ids, np.load(os.path.join(GOLD, name + ".npz"))


@pytest.mark.parametrize("name,metric", [("l1_grid_d4", "DistL1"), ("l2_dup_d16", "DistL2")])
def test_ties_are_cut_by_data_id(native, oracle, name, metric):
    """the small-integer grid and duplicated vectors: for every k of a range the answer is the (distance, DataId) order, and for
    some (query, k) the cut goes through a group of equal distances"""
    h, X, ids, z = _golden(native, name)
    h.upload(0)
    Q = np.concatenate([z["queries"], X[:24]]).astype(np.float32)
    D = oracle.dist_matrix(metric, Q, X)
    cuts = 0
    for k in list(range(1, 24)) + [len(X) - 1]:
        _assert_answers(oracle, metric, h.exact_search_flat(Q, k), Q, X, ids, k, what=f"{name} k {k}")
        s = np.sort(D, axis=1)
        if k < len(X):
            cuts += int((s[:, k - 1] == s[:, k]).sum())
    assert cuts > 20, cuts


def test_answer_is_independent_of_the_graph(native, oracle):
    """the same (vectors, ids) -- ids shuffled and sparse, vectors with duplicates -- in an index inserted serially and in one
    inserted in another order by four threads: identical answers"""
    n, d = 1500, 24
    rng = np.random.default_rng(5)
    X = uniform(n, d, 31)
    X[rng.choice(n, 200, replace=False)] = X[rng.choice(n, 200, replace=False)]
    ids = rng.choice(10 ** 12, n, replace=False).astype(np.uint64)
    perm = rng.permutation(n)
    a = _build(native, X, "DistL2", ids)
    b = _build(native, X[perm], "DistL2", ids[perm], nthreads=4)
    Q = np.concatenate([uniform(40, d, 32), X[:20]])
    for k in (7, 300):
        ra, rb = a.exact_search_flat(Q, k), b.exact_search_flat(Q, k)
        _assert_answers(oracle, "DistL2", ra, Q, X, ids, k, what="serial")
        assert np.array_equal(ra.ids, rb.ids) and np.array_equal(ra.dists.view(np.uint32), rb.dists.view(np.uint32))
        assert np.array_equal(ra.counts, rb.counts)


@pytest.mark.parametrize("metric,d", [("DistL2", 20), ("DistCosine", 25), ("DistJeffreys", 12)])
def test_filter(native, oracle, metric, d):
    n = 2100
    X, Q = _gen(metric)(n, d, 41), _gen(metric)(35, d, 42)
    ids = np.random.default_rng(6).permutation(n).astype(np.uint64) * 5
    h = _build(native, X, metric, ids)
    rng = np.random.default_rng(7)
    for frac in (0.01, 0.3, 1.0):
        rows = np.sort(rng.choice(n, max(1, int(frac * n)), replace=False))
        allowed = np.sort(np.concatenate([ids[rows], np.array([2, 3, 10 ** 15], np.uint64)]))   # + ids that name no point
        for k in (1, 10, 500):
            _assert_answers(oracle, metric, h.exact_search_flat(Q, k, allowed), Q, X, ids, k, rows, what=f"{metric} allowed {frac} k {k}")
    res = h.exact_search_flat(Q, 10, np.zeros(0, np.uint64))
    assert not res.counts.any() and not res.ids.any()
    res = h.exact_search_flat(Q, 10, np.array([2, 3], np.uint64))   # only ids that name no point
    assert not res.counts.any()
    with pytest.raises(native.HnswError):
        h.exact_search_flat(Q, 10, np.array([9, 4], np.uint64))     # unsorted


@pytest.mark.parametrize("metric,d", [("DistL2", 12), ("DistL1", 12), ("DistDot", 12), ("DistCosine", 25), ("DistCosine", 32),
                                      ("DistHellinger", 12), ("DistJeffreys", 12), ("DistJensenShannon", 12)])
def test_against_the_f64_reference(native, metric, d):
    n = 400
    X, Q = _gen(metric)(n, d, 51), _gen(metric)(40, d, 52)
    Q[:5] = X[:5]
    h = _build(native, X, metric)
    for k in (10, n + 5):
        res = h.exact_search_flat(Q, k)
        fails = F.check_exact_knn(metric, X, Q, res.ids, res.dists, res.counts, k, range(n))
        assert not fails, fails[:4]
    members = sorted(np.random.default_rng(8).choice(n, 120, replace=False).tolist())
    res = h.exact_search_flat(Q, 10, np.asarray(members, np.uint64))
    fails = F.check_exact_knn(metric, X, Q, res.ids, res.dists, res.counts, 10, members)
    assert not fails, fails[:4]


def _reach_index(native, oracle, tmp_path):
    from test_f64_reference import _index
    X, o, h, reach, gen = _index(native, oracle, tmp_path, "DistL2", 300, 12, 16, 17, "agree")
    h.upload(0)
    return X, h, np.asarray(sorted(reach), np.uint64), gen(80, 12, 61)


def test_agrees_with_the_search_itself(native, oracle, tmp_path):
    """an exhaustive-ef search reaches exactly the common reachable set: the exact search filtered to that set returns the same
    distance bits and counts, and the same ids wherever a query's distances are pairwise distinct"""
    X, h, reach, Q = _reach_index(native, oracle, tmp_path)
    ex = h.exact_search_flat(Q, 10, reach)
    got = h.parallel_search_flat(Q, 10, 512)
    assert np.array_equal(ex.counts, got.counts)
    assert np.array_equal(ex.dists.view(np.uint32), got.dists.view(np.uint32))
    distinct = 0
    for q in range(len(Q)):
        c = int(ex.counts[q])
        if len(np.unique(ex.dists[q, :c])) == c:
            distinct += 1
            assert np.array_equal(ex.ids[q], got.ids[q]), q
            assert np.array_equal(ex.layers[q], got.layers[q]) and np.array_equal(ex.ranks[q], got.ranks[q]), q
    assert distinct > len(Q) // 2


def test_recall_flat(native, oracle, tmp_path):
    X, h, reach, Q = _reach_index(native, oracle, tmp_path)
    by_dist, by_id = h.recall_flat(Q, 10, 512, reach)       # exhaustive ef on tie-free data
    assert by_dist == 1.0 and by_id == 1.0
    by_dist, by_id = h.recall_flat(Q, 10, 10)                # a real search against all points
    assert 0.0 <= by_id <= by_dist <= 1.0
    Xb = uniform(20000, 16, 71)
    hb = _build(native, Xb, "DistL2", m=6, efc=16)
    lo = hb.recall_flat(uniform(200, 16, 72), 10, 10)
    hi = hb.recall_flat(uniform(200, 16, 72), 10, 200)
    assert 0.0 <= lo[1] <= lo[0] <= 1.0 and 0.0 <= hi[1] <= hi[0] <= 1.0 and hi[1] >= lo[1]
    nb = hb.exact_search(uniform(2, 16, 73), 3)
    assert len(nb) == 2 and len(nb[0]) == 3 and nb[0][0].distance <= nb[0][1].distance and isinstance(nb[0][0], native.Neighbour)


def test_simd8_arithmetic_is_refused_not_answered_in_the_other_arithmetic(native):
    X = uniform(300, 37, 81)
    h = _build(native, X, "DistL2")
    h.set_arithmetic("simd8")
    try:
        with pytest.raises(native.HnswError) as e:
            h.exact_search_flat(X[:4], 5)
        assert e.value.code == 1 and "SIMD8" in str(e.value)
    finally:
        h.set_arithmetic("scalar")
    assert h.exact_search_flat(X[:4], 5).counts.tolist() == [5] * 4


def test_concurrent_exact_and_ordinary_search_on_one_handle(native, oracle):
    n, d = 20000, 32
    X, Q = uniform(n, d, 91), uniform(300, d, 92)
    h = _build(native, X, "DistL2", m=8, efc=24, nthreads=0)
    ex0, se0 = h.exact_search_flat(Q, 10), h.parallel_search_flat(Q, 10, 64)
    _assert_answers(oracle, "DistL2", ex0, Q, X, np.arange(n), 10, what="serial")
    out, errs = {}, []

    def run(name, fn):
        try:
            out[name] = [fn() for _ in range(4)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=("exact", lambda: h.exact_search_flat(Q, 10))),
          threading.Thread(target=run, args=("search", lambda: h.parallel_search_flat(Q, 10, 64)))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for r in out["exact"]:
        assert np.array_equal(r.ids, ex0.ids) and np.array_equal(r.dists.view(np.uint32), ex0.dists.view(np.uint32)) and np.array_equal(r.counts, ex0.counts)
    for r in out["search"]:
        assert np.array_equal(r.ids, se0.ids) and np.array_equal(r.dists.view(np.uint32), se0.dists.view(np.uint32)) and np.array_equal(r.counts, se0.counts)


@pytest.mark.parametrize("n,d,m,efc,metric", [(1_000_000, 128, 16, 200, "DistL2"), (1_200_000, 25, 24, 400, "DistCosine")])
def test_full_size(native, oracle, n, d, m, efc, metric):
    """BASELINE configs 2 and 3 at their real size (GPU-assisted build, as the full-size parity tests build theirs), 2 000 queries,
    k = 10: every returned pair's distance bits are the oracle's dist_eval, rows are ordered by (distance, id), and the f64
    reference finds no nearer point left out for a sample of 32 queries (evaluated in row chunks)."""
    from test_gpu_round2 import _clustered
    X = _clustered(n, d, 0x5EED0001)
    X[np.random.default_rng(3).choice(n, 2000, replace=False)] = X[np.random.default_rng(4).choice(n, 2000, replace=False)]
    h = native.Hnsw(m, n, 16, efc, metric)
    h.set_build_options(nthreads=0, gpu_device=0, gpu_window=0)
    h.parallel_insert(X)
    h.upload(0)
    nq, k = 2000, 10
    Q = _clustered(nq, d, 0x5EED0002)
    Q[:100] = X[np.random.default_rng(5).choice(n, 100, replace=False)]
    res = h.exact_search_flat(Q, k)
    assert res.counts.tolist() == [k] * nq
    assert int(res.ids.max()) < n
    for q in range(nq):
        for j in range(k):
            want = np.float32(oracle.dist_eval(metric, Q[q], X[int(res.ids[q, j])]))
            assert want.view(np.uint32) == res.dists[q, j].view(np.uint32), (q, j, want, res.dists[q, j])
    key = (res.dists.view(np.uint32).astype(np.uint64) << np.uint64(32)) | res.ids
    assert np.all(key[:, 1:] > key[:, :-1])
    sample = np.concatenate([np.arange(8), np.random.default_rng(6).choice(np.arange(8, nq), 24, replace=False)])
    fails = F.check_exact_knn(metric, X, Q[sample], res.ids[sample], res.dists[sample], res.counts[sample], k, range(n))
    assert not fails, fails[:4]


def test_long_batches_are_cut_into_chunks(native, oracle):
    """4000 queries with k = 1024 on 3000 points: 250 tiles of 12 slabs of 16 lists of 1024 keys are 393 MB, more than the scratch
    budget of one call, and 4000 rows of answers are more than the host entry stages at once -- both loops take a second turn"""
    n, d, nq, k = 3000, 8, 4000, 1024
    X, Q = uniform(n, d, 111), uniform(nq, d, 112)
    ids = np.random.default_rng(9).permutation(n).astype(np.uint64) + 11
    h = _build(native, X, "DistL2", ids)
    _assert_answers(oracle, "DistL2", h.exact_search_flat(Q, k), Q, X, ids, k, what="chunks")


def test_largest_knbn_at_size(native, oracle):
    """knbn = 4096, the largest the entry accepts, on 200 000 points (every slab shorter than knbn: every row is inserted), with
    and without a filter; 4097 is refused"""
    n, d, k = 200_000, 16, 4096
    X, Q = uniform(n, d, 121), uniform(20, d, 122)
    ids = np.random.default_rng(10).permutation(n).astype(np.uint64)
    h = _build(native, X, "DistL2", ids, nthreads=0, m=6, efc=12)
    _assert_answers(oracle, "DistL2", h.exact_search_flat(Q, k), Q, X, ids, k, what="k 4096")
    rows = np.sort(np.random.default_rng(11).choice(n, n // 3, replace=False))
    _assert_answers(oracle, "DistL2", h.exact_search_flat(Q, k, np.sort(ids[rows])), Q, X, ids, k, rows, what="k 4096 filtered")
    with pytest.raises(native.HnswError) as e:
        h.exact_search_flat(Q, k + 1)
    assert e.value.code == 1


def test_device_entry_on_a_stream(native):
    """hnswgpu_exact_search_batch_device with torch buffers on a stream of the caller's, a device-resident filter, with and
    without layer / rank outputs: the same answers as the host entry"""
    import torch
    n, d, nq, k = 5000, 24, 70, 12
    X, Q = uniform(n, d, 131), uniform(nq, d, 132)
    ids = np.random.default_rng(12).permutation(n).astype(np.uint64) * 2
    h = _build(native, X, "DistL2", ids)
    L = native.lib()
    allowed = np.sort(ids[np.random.default_rng(13).choice(n, 900, replace=False)])
    dq = torch.from_numpy(Q).cuda()
    dal = torch.from_numpy(allowed.astype(np.int64)).cuda()
    stream = torch.cuda.Stream()
    for al in (None, dal):
        want = h.exact_search_flat(Q, k, None if al is None else allowed)
        for with_pids in (True, False):
            o_ids = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
            o_d = torch.full((nq, k), -1.0, dtype=torch.float32, device="cuda")
            o_l = torch.full((nq, k), 9, dtype=torch.uint8, device="cuda")
            o_r = torch.full((nq, k), -1, dtype=torch.int32, device="cuda")
            o_c = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            rc = L.hnswgpu_exact_search_batch_device(h.handle, C.c_void_p(dq.data_ptr()), nq, d, k,
                                                     C.c_void_p(al.data_ptr()) if al is not None else None, 0 if al is None else len(allowed),
                                                     C.c_void_p(o_ids.data_ptr()), C.c_void_p(o_d.data_ptr()),
                                                     C.c_void_p(o_l.data_ptr()) if with_pids else None,
                                                     C.c_void_p(o_r.data_ptr()) if with_pids else None, C.c_void_p(o_c.data_ptr()),
                                                     C.c_void_p(stream.cuda_stream))
            assert rc == 0
            assert np.array_equal(o_ids.cpu().numpy().astype(np.uint64), want.ids)
            assert np.array_equal(o_d.cpu().numpy().view(np.uint32), want.dists.view(np.uint32))
            assert np.array_equal(o_c.cpu().numpy().astype(np.uint32), want.counts)
            if with_pids:
                assert np.array_equal(o_l.cpu().numpy(), want.layers) and np.array_equal(o_r.cpu().numpy(), want.ranks)
            else:
                assert (o_l == 9).all() and (o_r == -1).all()

