"""Exact k-NN for a set of filters, each query naming its own (Hnsw.exact_search_filters_flat ->
hnswgpu_exact_search_batch_filter_set / _device, csrc/exact_knn.hip): row q must be what the one-filter call returns for query q
alone under filters[filter_of[q]].
The expected answer never comes from the code under test: D = oracle_lib.dist_matrix(metric, Q, X) (the CPU oracle's
Distance::eval), and per query order = rows[np.lexsort((ids[rows], D[q, rows]))][:k] over the rows ITS filter allows; ids, f32 bit
patterns, p_ids, counts and the zeros behind the answers are compared exactly.  The one-filter exact_search_flat is a second
opinion only.  What an input must contain (ties at the cut, an empty eligible set, k above the eligible) is asserted on the
oracle's matrix.  Most indexes are hand-written dumps (tests/dump_writer.py): the exhaustive search never reads the graph, and a
hand-written dump fixes the flat order of the rows -- which 64-row step and which bitmap word a point falls into -- and every p_id."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import f64_reference as F
from conftest import normalized, probability, uniform
from dump_writer import write_dump

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NOISE = np.array([2, 5, 10 ** 15], np.uint64)   # ids that name no point (the indexes below use ids 3 i + 1)


def _gen(metric):
    return {"DistDot": normalized}.get(metric, probability if metric in F.PROBABILITY_METRICS else uniform)


class _Index:
    """n rows in a hand-written dump: ids 3 perm(i) + 1, levels geometric; flat[i] = the row at flat position i"""

    def __init__(self, native, path, metric, n, d, seed):
        rng = np.random.default_rng(seed)
        self.metric, self.n, self.d = metric, n, d
        self.X = _gen(metric)(n, d, seed)
        self.ids = rng.permutation(n).astype(np.uint64) * 3 + 1
        levels = np.minimum(rng.geometric(0.6, n) - 1, 5)
        order, pids = write_dump(path, "fs", self.X, self.ids, levels, metric)
        self.flat = np.asarray(order, np.int64)
        self.layer = np.array([p[0] for p in pids], np.uint8)
        self.rank = np.array([p[1] for p in pids], np.int32)
        self.h = native.HnswIo(path, "fs").load_hnsw(metric)
        self.h.upload(0)

    def filter(self, rows, noise=False):
        f = np.sort(self.ids[np.asarray(rows, np.int64)])
        return np.sort(np.concatenate([f, NOISE])) if noise else f


def _assert_set(oracle, ix, res, Q, rows_of, filter_of, k, what="", D=None):
    """every row of res against the oracle's distances ordered by (distance, origin id) over the rows of the query's own filter"""
    D = oracle.dist_matrix(ix.metric, Q, ix.X) if D is None else D
    assert len(res.counts) == len(Q)
    for q in range(len(Q)):
        rows = np.asarray(rows_of[int(filter_of[q])], np.int64)
        order = rows[np.lexsort((ix.ids[rows], D[q, rows]))][:k]
        c = len(order)
        assert int(res.counts[q]) == c == min(k, len(rows)), (what, q, int(res.counts[q]), c)
        assert np.array_equal(res.ids[q, :c], ix.ids[order]), (what, q, res.ids[q, :8], ix.ids[order][:8])
        assert np.array_equal(res.dists[q, :c].view(np.uint32), D[q, order].view(np.uint32)), (what, q, "distance bits")
        assert np.array_equal(res.layers[q, :c], ix.layer[order]) and np.array_equal(res.ranks[q, :c], ix.rank[order]), (what, q, "p_ids")
        assert not res.ids[q, c:].any() and not res.dists[q, c:].view(np.uint32).any(), (what, q, "slots behind the answers")
        assert not res.layers[q, c:].any() and not res.ranks[q, c:].any(), (what, q, "slots behind the answers")
    return D


def _same(a, b, what=""):
    assert np.array_equal(a.counts, b.counts), what
    assert np.array_equal(a.ids, b.ids) and np.array_equal(a.dists.view(np.uint32), b.dists.view(np.uint32)), what
    assert np.array_equal(a.layers, b.layers) and np.array_equal(a.ranks, b.ranks), what


def _seven(ix, seed):
    """rows of the seven filters: empty, one id, ~1 %, ~50 %, every id, ~30 % (its id vector gets ids that name no point mixed in),
    and one whose rows all lie inside a single 64-row step (flat positions 640 .. 703, every third)"""
    rng = np.random.default_rng(seed)
    n = ix.n
    rows = [np.zeros(0, np.int64), np.array([n // 3]), np.sort(rng.choice(n, n // 100, replace=False)),
            np.flatnonzero(rng.random(n) < 0.5), np.arange(n), np.flatnonzero(rng.random(n) < 0.3), ix.flat[640:704:3]]
    filters = [ix.filter(r, noise=(i == 5)) for i, r in enumerate(rows)]
    pos = np.empty(n, np.int64)
    pos[ix.flat] = np.arange(n)
    assert len(set((pos[rows[6]] // 64).tolist())) == 1 and len(rows[6]) == 22
    return rows, filters


CASES = [("DistL2", 33), ("DistCosine", 25), ("DistCosine", 30), ("DistCosine", 32), ("DistDot", 12), ("DistL1", 25),
         ("DistHellinger", 33), ("DistJeffreys", 31), ("DistJensenShannon", 32)]


@pytest.mark.parametrize("metric,d", CASES)
def test_mixed_tiles_all_metrics(native, oracle, tmp_path, metric, d):
    """n = 2 530 (W = 80 words, n % 32 != 0, no multiple of 64, several slabs), 37 queries (two tiles and a part), seven filters and
    every tile mixing at least four of them; DistCosine with the norm in the padding (25), in the row's last chunk (30) and in
    the side array (32).  Then the union-skip trap: tiles that pair the one-step filter with the filter of every id and the empty
    one -- each query its own answer, the empty one count 0."""
    ix = _Index(native, tmp_path, metric, 2530, d, 1000 + d)
    assert (ix.n + 31) // 32 == 80 and ix.n % 32 and ix.n % 64
    rows, filters = _seven(ix, 7)
    Q = _gen(metric)(37, d, 2000 + d)
    Q[:3] = ix.X[5:8]
    mixed = ((np.arange(37) * 3 + 1) % 7).astype(np.uint32)
    trap = np.array([6, 4, 0] * 12 + [6], np.uint32)
    for t0 in (0, 16, 32):
        assert len(set(mixed[t0:t0 + 16].tolist())) >= 4
    assert set(trap[:16].tolist()) == set(trap[16:32].tolist()) == {6, 4, 0}
    D = None
    for k in (1, 10, 300):
        for name, fo in (("mixed", mixed), ("trap", trap)):
            res = ix.h.exact_search_filters_flat(Q, k, filters, fo)
            D = _assert_set(oracle, ix, res, Q, rows, fo, k, f"{metric} d {d} k {k} {name}", D)
            assert not res.counts[fo == 0].any()
            assert res.counts[fo == 6].tolist() == [min(k, 22)] * int((fo == 6).sum())
    # the one-filter call as a second opinion, for one query of every filter
    res = ix.h.exact_search_filters_flat(Q, 10, filters, mixed)
    for q in range(7):
        one = ix.h.exact_search_flat(Q[q:q + 1], 10, filters[int(mixed[q])])
        assert np.array_equal(one.ids[0], res.ids[q]) and np.array_equal(one.dists.view(np.uint32)[0], res.dists.view(np.uint32)[q])
        assert one.counts[0] == res.counts[q]


@pytest.fixture(scope="module")
def base(native, tmp_path_factory):
    """DistL2, 2 530 x 33 with its seven filters"""
    ix = _Index(native, tmp_path_factory.mktemp("efs_base"), "DistL2", 2530, 33, 77)
    ix.rows, ix.filters = _seven(ix, 8)
    return ix


def test_odd_w_a_slots_last_word_abuts_the_next_slots_first(native, oracle, tmp_path):
    """n = 2 450: W = 77 words.  Filters 0 and 1 differ only in ids whose bits fall into the LAST word of a slot (flat positions
    2 432 .. 2 449), filter 2 is filter 0 again; the queries are those very rows, so a bit read from the neighbouring slot's word
    changes the nearest answer"""
    ix = _Index(native, tmp_path, "DistL2", 2450, 8, 5)
    assert (ix.n + 31) // 32 == 77
    common = ix.flat[np.flatnonzero(np.random.default_rng(6).random(2432) < 0.3)]
    last = ix.flat[2432:]
    rows = [np.concatenate([common, last[0::2]]), np.concatenate([common, last[1::2]]), np.concatenate([common, last[0::2]])]
    filters = [ix.filter(r) for r in rows]
    Q = np.concatenate([ix.X[last], uniform(15, 8, 9)]).astype(np.float32)
    fo = (np.arange(len(Q)) % 3).astype(np.uint32)
    D = oracle.dist_matrix("DistL2", Q, ix.X)
    differ = 0
    for q in range(len(last)):   # the query is a last-word row: under the filter that holds it, it is its own nearest; under the other it is absent
        a, b = rows[0][np.argmin(D[q, rows[0]])], rows[1][np.argmin(D[q, rows[1]])]
        differ += int(a != b)
    assert differ == len(last)
    for k in (1, 5):
        _assert_set(oracle, ix, ix.h.exact_search_filters_flat(Q, k, filters, fo), Q, rows, fo, k, f"W 77 k {k}", D)


def test_one_filter_per_query_and_one_filter_for_all(base, oracle):
    """filter_of=None: 33 queries, 33 different filters.  Every query naming the same filter: bit-identical to the one-filter call"""
    ix = base
    Q = uniform(33, ix.d, 31)
    rng = np.random.default_rng(32)
    rows = [np.sort(rng.choice(ix.n, int(s), replace=False)) for s in rng.integers(0, 600, 33)]
    rows[4], rows[20] = np.zeros(0, np.int64), np.arange(ix.n)
    filters = [ix.filter(r) for r in rows]
    assert len({f.tobytes() for f in filters}) == 33
    for k in (1, 10):
        _assert_set(oracle, ix, ix.h.exact_search_filters_flat(Q, k, filters), Q, rows, np.arange(33), k, f"one filter per query k {k}")
    for f in (3, 5, 0):
        same = np.zeros(33, np.uint32)
        got = ix.h.exact_search_filters_flat(Q, 10, [ix.filters[f]], same)
        _assert_set(oracle, ix, got, Q, [ix.rows[f]], same, 10, f"every query names filter {f}")
        _same(got, ix.h.exact_search_flat(Q, 10, ix.filters[f]), f"against exact_search_flat, filter {f}")
        _same(ix.h.exact_search_filters_flat(Q, 10, ix.filters, np.full(33, f, np.uint32)), got, f"filter {f} as one of seven")


def test_k_above_the_eligible(base, oracle):
    """k = 300 against filters of 0, 1, 25 and 22 ids: the count is the size of the query's OWN eligible set, zeros follow"""
    ix = base
    Q = uniform(21, ix.d, 41)
    fo = np.array([0, 1, 2, 6, 4, 3, 5] * 3, np.uint32)
    sizes = [len(r) for r in ix.rows]
    assert sizes[0] == 0 and sizes[1] == 1 and sizes[2] < 300 and sizes[6] < 300 and sizes[4] > 300
    res = ix.h.exact_search_filters_flat(Q, 300, ix.filters, fo)
    _assert_set(oracle, ix, res, Q, ix.rows, fo, 300, "k above eligible")
    assert res.counts.tolist() == [min(300, sizes[f]) for f in fo]
    nb = ix.h.exact_search_filters(Q[:3], 300, ix.filters, fo[:3])
    assert [len(x) for x in nb] == [0, 1, sizes[2]] and nb[1][0].d_id == int(ix.ids[ix.rows[1][0]])


@pytest.mark.parametrize("name,metric", [("l1_grid_d4", "DistL1"), ("l2_dup_d16", "DistL2")])
def test_ties_under_a_filter_are_cut_by_data_id(native, oracle, name, metric):
    """the small-integer grid and the duplicated vectors under three filters: for some (query, k) the cut at position k goes
    through a group of equal distances among the rows the query's filter allows (asserted on the oracle's matrix)"""
    h = native.HnswIo(GOLD, name).load_hnsw()
    dm = native.DataMap.from_hnswdump(GOLD, name)
    ids = np.asarray(dm.get_dataid_iter(), np.uint64)
    X = np.stack([np.array(dm.get_data(i)) for i in ids]).astype(np.float32)
    z = np.load(os.path.join(GOLD, name + ".npz"))
    h.upload(0)
    n = len(X)
    Q = np.concatenate([z["queries"], X[:24]]).astype(np.float32)
    rng = np.random.default_rng(3)
    rows = [np.flatnonzero(rng.random(n) < 0.7), np.flatnonzero(rng.random(n) < 0.4), np.arange(n)]
    filters = [np.sort(ids[r]) for r in rows]
    fo = (np.arange(len(Q)) % 3).astype(np.uint32)
    D = oracle.dist_matrix(metric, Q, X)
    cuts = 0
    for k in list(range(1, 24)):
        res = h.exact_search_filters_flat(Q, k, filters, fo)
        for q in range(len(Q)):
            r = rows[fo[q]]
            order = r[np.lexsort((ids[r], D[q, r]))]
            c = min(k, len(r))
            assert int(res.counts[q]) == c
            assert np.array_equal(res.ids[q, :c], ids[order[:c]]), (name, k, q)
            assert np.array_equal(res.dists[q, :c].view(np.uint32), D[q, order[:c]].view(np.uint32)), (name, k, q)
            assert not res.ids[q, c:].any() and not res.dists[q, c:].view(np.uint32).any()
            if k < len(r) and D[q, order[k - 1]] == D[q, order[k]]:
                cuts += 1
                assert ids[order[k - 1]] < ids[order[k]]
    assert cuts > 20, cuts


def test_a_set_beyond_the_budget_is_served_in_groups(native, base, oracle, knob):
    """a bitmap of this index is 80 words = 320 bytes; 0.00065 MiB = 681 bytes hold two: seven filters are four groups, and with
    these queries the group of filters 2 and 3 has no query at all"""
    ix = base
    Q = uniform(70, ix.d, 51)
    fo = np.array([0, 1, 4, 5, 6, 4, 6, 5, 1], np.uint32)[np.arange(70) % 9]
    assert not np.isin([2, 3], fo).any()
    whole = ix.h.exact_search_filters_flat(Q, 10, ix.filters, fo)
    D = _assert_set(oracle, ix, whole, Q, ix.rows, fo, 10, "default budget")
    knob("HNSWGPU_FILTER_SET_MB", "0.00065")
    grouped = ix.h.exact_search_filters_flat(Q, 10, ix.filters, fo)
    _assert_set(oracle, ix, grouped, Q, ix.rows, fo, 10, "four groups", D)
    _same(grouped, whole, "four groups against one")
    every = ((np.arange(70) * 3 + 1) % 7).astype(np.uint32)    # every group has queries, every tile of a group is dense
    _assert_set(oracle, ix, ix.h.exact_search_filters_flat(Q, 300, ix.filters, every), Q, ix.rows, every, 300, "four groups, k 300", D)
    knob("HNSWGPU_FILTER_SET_MB", "0.0004")                    # 419 bytes: one bitmap, seven groups
    _assert_set(oracle, ix, ix.h.exact_search_filters_flat(Q, 10, ix.filters, fo), Q, ix.rows, fo, 10, "seven groups", D)
    knob("HNSWGPU_FILTER_SET_MB", "0.0002")                    # 209 bytes: not even one bitmap
    with pytest.raises(native.HnswError) as e:
        ix.h.exact_search_filters_flat(Q, 10, ix.filters, fo)
    assert e.value.code == native._native.ERR_ARG and "HNSWGPU_FILTER_SET_MB" in str(e.value)
    knob("HNSWGPU_FILTER_SET_MB", None)
    _same(ix.h.exact_search_filters_flat(Q, 10, ix.filters, fo), whole, "knob restored")


def test_long_batches_are_cut_into_chunks_with_a_list(native, oracle, tmp_path, knob):
    """the shape of test_gpu_exact_knn.test_long_batches_are_cut_into_chunks (3 000 points, 4 000 queries, k = 1 024) under three
    filters, one bitmap per group: the host entry stages 3 847 queries at a time, and of those the 3 650 that name filter 1 are
    more than the 213 tiles the scratch budget holds -- both loops take a second turn while the queries go through the list"""
    n, d, nq, k = 3000, 8, 4000, 1024
    ix = _Index(native, tmp_path, "DistL2", n, d, 111)
    Q = uniform(nq, d, 112)
    rng = np.random.default_rng(113)
    rows = [np.flatnonzero(rng.random(n) < 0.2), np.flatnonzero(rng.random(n) < 0.6), np.arange(n)]
    filters = [ix.filter(r) for r in rows]
    fo = np.ones(nq, np.uint32)
    fo[0::40], fo[20::40] = 0, 2
    assert int((fo[:3847] == 1).sum()) > 213 * 16 and len(rows[0]) < k < len(rows[1])
    knob("HNSWGPU_FILTER_SET_MB", "0.0004")                    # 419 bytes hold one bitmap of 94 words
    _assert_set(oracle, ix, ix.h.exact_search_filters_flat(Q, k, filters, fo), Q, rows, fo, k, "chunks with a list")


def _torch_call(native, h, Q, k, filters, filter_of, stream, with_pids=True):
    """hnswgpu_exact_search_batch_filter_set_device on torch buffers pre-filled with sentinels, on the caller's stream"""
    import torch
    dev = torch.device("cuda", 0)
    nq, d = Q.shape
    flat = np.concatenate(filters) if sum(len(f) for f in filters) else np.zeros(1, np.uint64)
    offsets = np.zeros(len(filters) + 1, np.uint64)
    np.cumsum([len(f) for f in filters], out=offsets[1:])
    with torch.cuda.stream(stream):
        q = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
        t_ids = torch.from_numpy(flat.view(np.int64)).to(dev)
        t_off = torch.from_numpy(offsets.view(np.int64)).to(dev)
        t_of = torch.from_numpy(np.ascontiguousarray(filter_of, dtype=np.uint32).view(np.int32)).to(dev)
        ids = torch.full((nq, k), -1, dtype=torch.int64, device=dev)
        dists = torch.full((nq, k), -1.0, dtype=torch.float32, device=dev)
        layers = torch.full((nq, k), 9, dtype=torch.uint8, device=dev)
        ranks = torch.full((nq, k), -1, dtype=torch.int32, device=dev)
        counts = torch.full((nq,), -1, dtype=torch.int32, device=dev)
    stream.synchronize()
    rc = native.lib().hnswgpu_exact_search_batch_filter_set_device(
        h.handle, C.c_void_p(q.data_ptr()), nq, d, k, C.c_void_p(t_ids.data_ptr()), C.c_void_p(t_off.data_ptr()), len(filters),
        C.c_void_p(t_of.data_ptr()), C.c_void_p(ids.data_ptr()), C.c_void_p(dists.data_ptr()),
        C.c_void_p(layers.data_ptr()) if with_pids else None, C.c_void_p(ranks.data_ptr()) if with_pids else None,
        C.c_void_p(counts.data_ptr()), C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return rc, (ids.cpu().numpy(), dists.cpu().numpy(), layers.cpu().numpy(), ranks.cpu().numpy(), counts.cpu().numpy())


def test_device_entry_on_a_stream(native, base, oracle):
    """torch buffers on a stream of the caller's, with and without out_layer / out_rank: the host entry's answers.  One entry of
    d_filter_of that names no filter: HNSWGPU_ERR_ARG, the outputs keep their sentinels, and the next valid call answers."""
    import torch
    ix = base
    Q = uniform(70, ix.d, 61)
    fo = ((np.arange(70) * 5 + 2) % 7).astype(np.uint32)
    k = 12
    want = ix.h.exact_search_filters_flat(Q, k, ix.filters, fo)
    _assert_set(oracle, ix, want, Q, ix.rows, fo, k, "host entry")
    stream = torch.cuda.Stream(torch.device("cuda", 0))

    def check(with_pids):
        rc, (ids, dists, layers, ranks, counts) = _torch_call(native, ix.h, Q, k, ix.filters, fo, stream, with_pids)
        assert rc == 0, native._native.last_error()
        assert np.array_equal(ids.view(np.uint64), want.ids) and np.array_equal(dists.view(np.uint32), want.dists.view(np.uint32))
        assert np.array_equal(counts.view(np.uint32), want.counts)
        if with_pids:
            assert np.array_equal(layers, want.layers) and np.array_equal(ranks, want.ranks)
        else:
            assert (layers == 9).all() and (ranks == -1).all()
    check(True)
    check(False)
    bad = fo.copy()
    bad[37] = len(ix.filters)
    rc, (ids, dists, layers, ranks, counts) = _torch_call(native, ix.h, Q, k, ix.filters, bad, stream)
    assert rc == native._native.ERR_ARG and "filter_of" in native._native.last_error()
    assert (ids == -1).all() and (dists == -1.0).all() and (layers == 9).all() and (ranks == -1).all() and (counts == -1).all()
    check(True)


def _oracle_filtered(o, Q, k, ef, filters, filter_of):
    """orc_search_filter once per query under that query's filter: [(ids, dists)], nothing for a query on which the reference panics"""
    out = []
    for q in range(len(Q)):
        try:
            ids, dd, _, _ = o.search_filter(Q[q], k, ef, filters[int(filter_of[q])])
        except RuntimeError as e:
            assert "panics" in str(e)
            ids, dd = np.zeros(0, np.uint64), np.zeros(0, np.float32)
        out.append((np.asarray(ids, np.uint64), np.asarray(dd, np.float32)))
    return out


def test_recall_filters_flat(native, oracle, tmp_path):
    """on a built index of 5 000 points at ef = 400: the recall computed here from the oracle's filtered search answers and the
    oracle's exact answers (recall_flat's definition); one filter named by every query: recall_flat(..., allowed_ids)"""
    n, d, k, ef = 5000, 16, 10, 400
    X = uniform(n, d, 71)
    origin = (np.arange(n, dtype=np.uint64) * 2 + 5)
    o = oracle.OracleHnsw(8, n, 16, 40, "DistL2")
    o.insert_batch(X, origin)
    o.file_dump(tmp_path, "rc")
    h = native.HnswIo(tmp_path, "rc").load_hnsw("DistL2")
    h.upload(0)
    Q = uniform(60, d, 72)
    rng = np.random.default_rng(73)
    rows = [np.flatnonzero(rng.random(n) < f) for f in (0.5, 0.05, 0.002, 1.0)] + [np.zeros(0, np.int64)]
    filters = [np.sort(origin[r]) for r in rows]
    fo = ((np.arange(60) * 2 + 1) % 5).astype(np.uint32)
    got = _oracle_filtered(o, Q, k, ef, filters, fo)
    D = oracle.dist_matrix("DistL2", Q, X)
    total = by_dist = by_id = 0
    for q in range(60):
        r = rows[fo[q]]
        order = r[np.lexsort((origin[r], D[q, r]))][:k]
        if len(order) == 0:
            continue
        total += len(order)
        by_dist += int(np.count_nonzero(got[q][1] <= D[q, order[-1]]))
        by_id += len(np.intersect1d(got[q][0], origin[order]))
    assert total > 0
    assert h.recall_filters_flat(Q, k, ef, filters, fo) == (by_dist / total, by_id / total)
    for f in (0, 2):
        assert h.recall_filters_flat(Q, k, ef, [filters[f]], np.zeros(60, np.uint32)) == h.recall_flat(Q, k, ef, filters[f])
    lo = h.recall_filters_flat(Q, k, 10, filters, fo)
    assert 0.0 <= lo[1] <= lo[0] <= 1.0


def test_concurrent_filter_set_exact_and_ordinary_search_on_one_handle(native, oracle, tmp_path):
    """one handle, two threads: the filter-set exact call and an ordinary search (shared lock, pooled scratch); the exact answers
    are the oracle's matrix ordered per query, the search's are the oracle's search of the same graph"""
    n, d = 8000, 32
    X, Q = uniform(n, d, 91), uniform(300, d, 92)
    ids = np.arange(n, dtype=np.uint64)
    o = oracle.OracleHnsw(8, n, 16, 24, "DistL2")
    o.insert_batch(X, ids)
    o.file_dump(tmp_path, "cc")
    h = native.HnswIo(tmp_path, "cc").load_hnsw("DistL2")
    h.upload(0)
    rng = np.random.default_rng(93)
    rows = [np.flatnonzero(rng.random(n) < f) for f in (0.5, 0.01, 1.0, 0.1)]
    filters = [ids[r] for r in rows]
    fo = (np.arange(300) % 4).astype(np.uint32)
    D = oracle.dist_matrix("DistL2", Q, X)
    want_ids, want_d = np.zeros((300, 10), np.uint64), np.zeros((300, 10), np.float32)
    for q in range(300):
        r = rows[fo[q]]
        order = r[np.lexsort((ids[r], D[q, r]))][:10]
        want_ids[q], want_d[q] = ids[order], D[q, order]
    se = o.parallel_search(Q, 10, 64)
    out, errs = {}, []

    def run(name, fn):
        try:
            out[name] = [fn() for _ in range(4)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=("exact", lambda: h.exact_search_filters_flat(Q, 10, filters, fo))),
          threading.Thread(target=run, args=("search", lambda: h.parallel_search_flat(Q, 10, 64)))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for r in out["exact"]:
        assert r.counts.tolist() == [10] * 300
        assert np.array_equal(r.ids, want_ids) and np.array_equal(r.dists.view(np.uint32), want_d.view(np.uint32))
    for r in out["search"]:
        assert np.array_equal(r.ids, se.ids) and np.array_equal(r.dists.view(np.uint32), se.dists.view(np.uint32)) and np.array_equal(r.counts, se.counts)
