"""A set of filters for one batch, each query naming its own (hnswgpu_search_batch_filter_set / _device,
Hnsw.parallel_search_filters_flat): query q must be answered exactly as Hnsw::search_filter(data_q, knbn, ef,
Some(&filters[filter_of[q]])).  The reference everywhere is the oracle's orc_search_filter, called once per query with that
query's own vector; ids, f32 distance bits, layers, ranks, counts and status are compared for EVERY query of every batch."""
import ctypes as C

import numpy as np
import pytest

from conftest import uniform

pytestmark = pytest.mark.gpu

N_MIXED, D_MIXED = 2003, 16   # n is no multiple of 32: the last bitmap word of slot s abuts the first of slot s + 1


class _Ans:
    def __init__(self, ids, dists, layers, ranks, counts, status):
        self.ids, self.dists, self.layers, self.ranks, self.counts, self.status = ids, dists, layers, ranks, counts, status


def _oracle_answers(o, Q, k, ef, filters, filter_of):
    """orc_search_filter once per query, under that query's filter; a query on which the reference panics: status 1, count 0"""
    nq = Q.shape[0]
    a = _Ans(np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros((nq, k), np.uint8), np.zeros((nq, k), np.int32),
             np.zeros(nq, np.uint32), np.zeros(nq, np.uint8))
    for q in range(nq):
        try:
            ids, dd, ll, rr = o.search_filter(Q[q], k, ef, filters[int(filter_of[q])])
        except RuntimeError as e:
            assert "panics" in str(e)
            a.status[q] = 1
            continue
        c = len(ids)
        a.counts[q] = c
        a.ids[q, :c], a.dists[q, :c], a.layers[q, :c], a.ranks[q, :c] = ids, dd, ll, rr
    return a


def _assert_equal(got, ref, what=""):
    """every query: status, count, and the count's worth of ids, distance bits, layers and ranks"""
    nq = len(ref.counts)
    assert len(got.counts) == nq
    assert np.array_equal(np.asarray(got.status, np.uint8), ref.status), (what, np.flatnonzero(np.asarray(got.status) != ref.status)[:8].tolist())
    assert np.array_equal(got.counts, ref.counts), (what, np.flatnonzero(got.counts != ref.counts)[:8].tolist())
    for q in range(nq):
        c = int(ref.counts[q])
        assert np.array_equal(got.ids[q, :c], ref.ids[q, :c]), f"{what}: ids of query {q}"
        assert np.array_equal(got.dists[q, :c].view(np.uint32), ref.dists[q, :c].view(np.uint32)), f"{what}: distance bits of query {q}"
        assert np.array_equal(got.layers[q, :c], ref.layers[q, :c]), f"{what}: layers of query {q}"
        assert np.array_equal(got.ranks[q, :c], ref.ranks[q, :c]), f"{what}: ranks of query {q}"


def _pair(native, oracle, path, X, m, efc, dist, ids=None):
    o = oracle.OracleHnsw(m, len(X), 16, efc, dist)
    o.insert_batch(X, ids)
    o.file_dump(path, "fs")
    h = native.HnswIo(path, "fs").load_hnsw(dist)
    h.upload(0)
    return o, h


def _subset(origin, frac, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(origin, int(round(len(origin) * frac)), replace=False)).astype(np.uint64)


@pytest.fixture(scope="module")
def mixed(native, oracle, tmp_path_factory):
    """2 003 points x 16, M = 8, origin ids 7 i + 3 (a flat id taken for an origin id shows), in DistL2 and DistCosine; five filters:
    every id, ~50 %, ~10 %, ~1 %, none; 96 queries naming them interleaved"""
    X = uniform(N_MIXED, D_MIXED, 301)
    origin = (7 * np.arange(N_MIXED) + 3).astype(np.uint64)
    out = {"X": X, "origin": origin, "Q": uniform(96, D_MIXED, 302)}
    for dist in ("DistL2", "DistCosine"):
        out[dist] = _pair(native, oracle, tmp_path_factory.mktemp("fs_" + dist), X, 8, 40, dist, origin)
    out["filters"] = [origin.copy(), _subset(origin, 0.5, 1), _subset(origin, 0.1, 2), _subset(origin, 0.01, 3), np.zeros(0, np.uint64)]
    out["filter_of"] = ((np.arange(96) * 3 + 1) % 5).astype(np.uint32)   # 1 4 2 0 3 1 4 ...: interleaved, every filter used
    return out


@pytest.mark.parametrize("ef", [16, 100, 200])   # one per instantiation of the literal kernel: return_points in 1 / 2 VGPR slots / memory
def test_mixed_set_matches_the_oracle_query_by_query(mixed, ef):
    o, h = mixed["DistL2"]
    ref = _oracle_answers(o, mixed["Q"], 10, ef, mixed["filters"], mixed["filter_of"])
    got = h.parallel_search_filters_flat(mixed["Q"], 10, ef, mixed["filters"], mixed["filter_of"])
    _assert_equal(got, ref, f"DistL2 ef {ef}")
    fo = mixed["filter_of"]
    assert np.all(got.counts[fo == 4] == 0) and np.all(got.counts[fo == 0] == 10)       # the empty filter, the filter of every id
    for f in (1, 2, 3):                                                                # every answer is allowed by ITS filter
        for q in np.flatnonzero(fo == f):
            assert np.isin(got.ids[q, :got.counts[q]], mixed["filters"][f]).all()


def test_mixed_set_second_metric(mixed):
    o, h = mixed["DistCosine"]
    ref = _oracle_answers(o, mixed["Q"], 10, 48, mixed["filters"], mixed["filter_of"])
    _assert_equal(h.parallel_search_filters_flat(mixed["Q"], 10, 48, mixed["filters"], mixed["filter_of"]), ref, "DistCosine ef 48")


def test_filter_of_none_is_one_filter_per_query(mixed):
    o, h = mixed["DistL2"]
    Q = mixed["Q"][:12]
    filters = [_subset(mixed["origin"], 0.2, 50 + q) for q in range(12)]
    ref = _oracle_answers(o, Q, 5, 24, filters, np.arange(12))
    _assert_equal(h.parallel_search_filters_flat(Q, 5, 24, filters), ref, "one filter per query")


def test_tie_saturated_index_keeps_the_reference_heap_order(native, oracle, tmp_path):
    """integer-valued coordinates (few distinct distances: the answer depends on the order inside Rust's BinaryHeap), 3 filters"""
    rng = np.random.default_rng(77)
    n, d = 1200, 6
    X = np.ascontiguousarray(rng.integers(0, 4, (n, d)).astype(np.float32))
    o, h = _pair(native, oracle, tmp_path, X, 8, 40, "DistL2")
    Q = np.ascontiguousarray(np.random.default_rng(78).integers(0, 4, (60, d)).astype(np.float32))
    origin = np.arange(n, dtype=np.uint64)
    filters = [origin, _subset(origin, 0.5, 4), _subset(origin, 0.1, 5)]
    filter_of = (np.arange(60) % 3).astype(np.uint32)
    for ef in (32, 200):
        ref = _oracle_answers(o, Q, 10, ef, filters, filter_of)
        assert sum(len(np.unique(ref.dists[q, :ref.counts[q]])) < ref.counts[q] for q in range(60)) > 20   # the answers really tie
        _assert_equal(h.parallel_search_filters_flat(Q, 10, ef, filters, filter_of), ref, f"ties ef {ef}")


def test_a_set_beyond_the_budget_is_served_in_groups(native, mixed, knob):
    """a bitmap of this index is 63 words = 252 bytes; 0.0006 MiB = 629 bytes hold two: 7 filters are four groups"""
    o, h = mixed["DistL2"]
    Q = uniform(70, D_MIXED, 303)
    origin = mixed["origin"]
    filters = [_subset(origin, f, 20 + i) for i, f in enumerate((0.5, 0.02, 1.0, 0.1, 0.0, 0.3, 0.05))]
    filter_of = ((np.arange(70) * 5 + 2) % 7).astype(np.uint32)
    ref = _oracle_answers(o, Q, 10, 40, filters, filter_of)
    whole = h.parallel_search_filters_flat(Q, 10, 40, filters, filter_of)
    _assert_equal(whole, ref, "default budget")
    knob("HNSWGPU_FILTER_SET_MB", "0.0006")
    grouped = h.parallel_search_filters_flat(Q, 10, 40, filters, filter_of)
    _assert_equal(grouped, ref, "four groups")
    _assert_equal(grouped, whole, "four groups against one")
    # some groups have no query at all, and a group may be a single filter
    few = np.where(np.arange(70) % 2 == 0, 6, 0).astype(np.uint32)
    _assert_equal(h.parallel_search_filters_flat(Q, 10, 40, filters, few), _oracle_answers(o, Q, 10, 40, filters, few), "empty groups")
    knob("HNSWGPU_FILTER_SET_MB", "0.0002")   # 209 bytes: not even one bitmap
    with pytest.raises(native.HnswError) as e:
        h.parallel_search_filters_flat(Q, 10, 40, filters, filter_of)
    assert e.value.code == native._native.ERR_ARG and "HNSWGPU_FILTER_SET_MB" in str(e.value)
    knob("HNSWGPU_FILTER_SET_MB", None)
    _assert_equal(h.parallel_search_filters_flat(Q, 10, 40, filters, filter_of), ref, "knob restored")


# ------------------------------------------------------------------------------------------------- the device entries
def _torch_call(native, h, Q, k, ef, filters, filter_of, stream, one_filter=False, fill=0):
    """hnswgpu_search_batch_filter_set_device (one_filter: hnswgpu_search_batch_filtered_device with filters[0]) on torch buffers,
    launched on the caller's stream: (status code, answers with the d_stats words, n_panics)"""
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
        ids = torch.full((nq, k), fill, dtype=torch.int64, device=dev)
        dists = torch.full((nq, k), float(fill), dtype=torch.float32, device=dev)
        layers = torch.full((nq, k), fill, dtype=torch.uint8, device=dev)
        ranks = torch.full((nq, k), fill, dtype=torch.int32, device=dev)
        counts = torch.full((nq,), fill, dtype=torch.int32, device=dev)
        stats = torch.full((nq, 8), fill, dtype=torch.int32, device=dev)
    stream.synchronize()
    panics = C.c_uint32(12345)
    L = native.lib()
    if one_filter:
        rc = L.hnswgpu_search_batch_filtered_device(h.handle, q.data_ptr(), nq, d, k, ef, t_ids.data_ptr(), len(filters[0]), ids.data_ptr(),
                                                    dists.data_ptr(), layers.data_ptr(), ranks.data_ptr(), counts.data_ptr(), stats.data_ptr(),
                                                    stream.cuda_stream, C.byref(panics))
    else:
        rc = L.hnswgpu_search_batch_filter_set_device(h.handle, q.data_ptr(), nq, d, k, ef, t_ids.data_ptr(), t_off.data_ptr(), len(filters),
                                                      t_of.data_ptr(), ids.data_ptr(), dists.data_ptr(), layers.data_ptr(), ranks.data_ptr(),
                                                      counts.data_ptr(), stats.data_ptr(), stream.cuda_stream, C.byref(panics))
    stream.synchronize()
    st = stats.cpu().numpy().view(np.uint32)
    a = _Ans(ids.cpu().numpy().view(np.uint64), dists.cpu().numpy(), layers.cpu().numpy(), ranks.cpu().numpy(), counts.cpu().numpy().view(np.uint32),
             (st[:, 3] == 6).astype(np.uint8))
    a.stats = st
    return rc, a, panics.value


def test_one_filter_named_by_every_query_is_the_one_filter_call(native, mixed):
    """ids, distances, counts, status and the work counters (d_stats words 0-2) of hnswgpu_search_batch_filtered, host and device"""
    import torch
    o, h = mixed["DistL2"]
    Q = mixed["Q"]
    allowed = mixed["filters"][2]
    zeros = np.zeros(len(Q), np.uint32)
    ref = _oracle_answers(o, Q, 10, 40, [allowed], zeros)
    host_set = h.parallel_search_filters_flat(Q, 10, 40, [allowed], zeros)
    host_one = h.parallel_search_filter_flat(Q, 10, 40, allowed)
    _assert_equal(host_set, ref, "host entry")
    _assert_equal(host_set, host_one, "host entry against hnswgpu_search_batch_filtered")
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    rc, dev_set, p_set = _torch_call(native, h, Q, 10, 40, [allowed], zeros, stream)
    assert rc == 0, native._native.last_error()
    rc, dev_one, p_one = _torch_call(native, h, Q, 10, 40, [allowed], zeros, stream, one_filter=True)
    assert rc == 0, native._native.last_error()
    _assert_equal(dev_set, ref, "device entry")
    _assert_equal(dev_set, dev_one, "device entry against hnswgpu_search_batch_filtered_device")
    assert np.array_equal(dev_set.stats[:, :3], dev_one.stats[:, :3])     # n_dist, n_expand, n_ids_read
    assert np.array_equal(dev_set.stats[:, 3], dev_one.stats[:, 3])
    assert p_set == p_one == 0


def test_device_entry_refuses_a_filter_of_beyond_the_set_before_it_searches(native, mixed):
    """no fault is provoked: the checking kernel counts the entry that names no filter and the call returns before the search
    kernel is launched -- nothing is written, and the handle goes on answering"""
    import torch
    o, h = mixed["DistL2"]
    Q, filters = mixed["Q"], mixed["filters"]
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    bad = mixed["filter_of"].copy()
    bad[37] = len(filters)
    rc, a, panics = _torch_call(native, h, Q, 10, 100, filters, bad, stream, fill=121)
    assert rc == native._native.ERR_ARG and "filter_of" in native._native.last_error()
    fill = 121
    assert np.all(a.ids == fill) and np.all(a.dists == float(fill)) and np.all(a.layers == fill) and np.all(a.ranks == fill)
    assert np.all(a.counts == fill) and np.all(a.stats == fill) and panics == 0
    rc, a, panics = _torch_call(native, h, Q, 10, 100, filters, mixed["filter_of"], stream)
    assert rc == 0, native._native.last_error()
    _assert_equal(a, _oracle_answers(o, Q, 10, 100, filters, mixed["filter_of"]), "after the refused call")
    assert panics == 0


# ------------------------------------------------------------------------------------------------- panics
def test_status_follows_the_oracle_where_the_reference_can_panic(native, oracle, tmp_path):
    """k = ef = 1 -- the only place where the kernel's panic branch (`peek().unwrap()` on a return_points the filter emptied,
    src/hnsw.rs:973) could be taken -- on the index, the queries and the filter densities of the existing k = ef = 1 filtered test
    (test_gpu_round2.test_filtered_search_matches_oracle), sparse, empty and every-id filters interleaved.  Status must be 1
    exactly where the oracle reports the panic, the other answers valid, and without a status array the call must return
    HNSWGPU_ERR_REF_PANIC exactly when the oracle reports one.
    Measured when this test was written: the oracle reports NO panic on this construction (0 of 50), nor on that of
    tests/test_second_opinion.py, nor on 72 000 filtered queries over 150 random small graphs at (k, ef) in {(1, 1), (2, 2), (1, 2)}:
    with ef = 1 a candidate is only accepted when nearer than return_points' single entry, so no popped candidate is ever farther
    than a refused entry point standing alone, and `retain` never empties the heap.  So the HNSWGPU_ERR_REF_PANIC return of the new
    entry is reached by no test here, as it is by no test of hnswgpu_search_batch_filtered; what is asserted is agreement with the
    oracle, whichever it reports."""
    from test_gpu_parity import build_pair
    N = native._native
    X, o, h = build_pair(native, oracle, tmp_path, 3000, 8, 6, 60, "DistL2", seed=14)
    Q = uniform(50, 8, 9)
    origin = np.arange(3000, dtype=np.uint64)
    filters = [_subset(origin, 0.01, 8), origin, np.zeros(0, np.uint64), _subset(origin, 0.3, 9)]
    filter_of = (np.arange(50) % 4).astype(np.uint32)
    ref = _oracle_answers(o, Q, 1, 1, filters, filter_of)
    n_panics = int(ref.status.sum())
    print(f"oracle: {n_panics} of 50 queries panic; counts {ref.counts.tolist()}")
    assert ref.status[filter_of == 1].sum() == 0 and np.all(ref.counts[filter_of == 1] == 1)    # never under the filter of every id
    got = h.parallel_search_filters_flat(Q, 1, 1, filters, filter_of)
    _assert_equal(got, ref, "k = ef = 1")
    # without a status array the panics, if any, are reported as a status code; the other answers are valid
    ids = np.zeros((50, 1), np.uint64); dd = np.zeros((50, 1), np.float32); ll = np.zeros((50, 1), np.uint8); rr = np.zeros((50, 1), np.int32)
    cnt = np.zeros(50, np.uint32)
    flat = np.concatenate(filters)
    offsets = np.zeros(len(filters) + 1, np.uint64)
    np.cumsum([len(f) for f in filters], out=offsets[1:])
    rc = native.lib().hnswgpu_search_batch_filter_set(h.handle, Q.ctypes.data, 50, 8, 1, 1, flat.ctypes.data, offsets.ctypes.data, len(filters),
                                                      filter_of.ctypes.data, ids.ctypes.data, dd.ctypes.data, ll.ctypes.data, rr.ctypes.data,
                                                      cnt.ctypes.data, None)
    assert rc == (N.ERR_REF_PANIC if n_panics else N.OK), N.last_error()
    if n_panics:
        assert "panics" in N.last_error()
    _assert_equal(_Ans(ids, dd, ll, rr, cnt, ref.status), ref, "without out_status")
    import torch
    rc, a, panics = _torch_call(native, h, Q, 1, 1, filters, filter_of, torch.cuda.Stream(torch.device("cuda", 0)))
    assert rc == 0 and panics == n_panics
    _assert_equal(a, ref, "device entry")
