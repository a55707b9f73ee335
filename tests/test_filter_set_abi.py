"""The filter-set entries (hnswgpu_search_batch_filter_set / _device, Hnsw.parallel_search_filters_flat) as far as a box without a
GPU can see them: the prototypes generated from the header, every HNSWGPU_ERR_ARG case of the host entry with its message, the
empty index, and the Python method's own checks.  CPU only; tests/test_gpu_filter_set.py checks the answers."""
import ctypes as C

import numpy as np
import pytest

ENTRIES = ("hnswgpu_search_batch_filter_set", "hnswgpu_search_batch_filter_set_device")


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _small(native, n=50, d=8):
    X = np.random.default_rng(1).random((n, d), dtype=np.float32)
    h = native.Hnsw(8, n, 16, 32, "DistL2")
    h.set_build_options(nthreads=1)
    h.parallel_insert(X)
    return X, h


def test_both_prototypes_are_in_the_header_and_exported(native):
    N = _N()
    protos = N.HEADER.prototypes
    for name in ENTRIES:
        assert name in protos and name in N.SYMBOLS, name
        res, args, names, _ = protos[name]
        assert res is C.c_int
        assert getattr(native.lib(), name) is not None
    host, dev = protos[ENTRIES[0]][2], protos[ENTRIES[1]][2]
    assert host == ["idx", "queries", "nq", "d", "k", "ef", "filter_ids", "filter_offsets", "n_filters", "filter_of", "out_ids", "out_dists",
                    "out_layer", "out_rank", "out_counts", "out_status"]
    assert dev == ["idx", "d_queries", "nq", "d", "k", "ef", "d_filter_ids", "d_filter_offsets", "n_filters", "d_filter_of", "d_out_ids",
                   "d_out_dists", "d_out_layer", "d_out_rank", "d_out_counts", "d_stats", "stream", "n_panics"]
    # beside the existing filtered pair: same outputs, same trailing arguments
    assert host[-6:] == protos["hnswgpu_search_batch_filtered"][2][-6:]
    assert [n.replace("d_", "", 1) for n in dev[-8:]] == [n.replace("d_", "", 1) for n in protos["hnswgpu_search_batch_filtered_device"][2][-8:]]
    assert "HNSWGPU_FILTER_SET_MB" in open(N.HEADER_PATH).read() or "_FILTER_SET_MB" in open(N.HEADER_PATH).read()


def test_every_argument_error_of_the_host_entry_names_what_is_wrong(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    Q = X[:4].copy()
    k = 3
    ids, dists, counts, status = np.zeros((4, k), np.uint64), np.zeros((4, k), np.float32), np.full(4, 99, np.uint32), np.zeros(4, np.uint8)
    f_ids = np.array([1, 5, 9, 2, 3], np.uint64)          # filter 0 = {1, 5, 9}, filter 1 = {2, 3}
    f_off = np.array([0, 3, 5], np.uint64)
    f_of = np.array([0, 1, 1, 0], np.uint32)

    def call(idx=h.handle, q=Q, nq=4, fi=f_ids, fo=f_off, nf=2, of=f_of, oi=ids, od=dists, oc=counts):
        return L.hnswgpu_search_batch_filter_set(idx, _p(q), nq, 8, k, 16, _p(fi), _p(fo), nf, _p(of), _p(oi), _p(od), None, None, _p(oc),
                                                 _p(status))

    def refused(word, **kw):
        rc = call(**kw)
        assert rc == N.ERR_ARG, (kw.keys(), rc, N.last_error())
        assert word in N.last_error(), (word, N.last_error())
        assert np.all(counts == 99)                      # nothing was searched, nothing written

    refused("null", idx=None)
    refused("null buffer", q=None)
    refused("null buffer", oi=None)
    refused("null buffer", od=None)
    refused("null buffer", oc=None)
    refused("filter_of", of=None)
    refused("filter_offsets", fo=None)
    refused("filter_ids", fi=None)
    refused("n_filters", nf=0)                                                       # no filter, but queries
    refused("start at 0", fo=np.array([1, 3, 5], np.uint64))
    refused("ascend", fo=np.array([0, 4, 3], np.uint64))
    refused("filter 1 ", fi=np.array([1, 5, 9, 3, 2], np.uint64))                    # the unsorted vector is named
    refused("filter 0 ", fi=np.array([5, 1, 9, 2, 3], np.uint64))
    refused("filter_of[2] = 2", of=np.array([0, 1, 2, 0], np.uint32))                # == n_filters
    refused("filter_of[3]", of=np.array([0, 1, 1, 0xFFFFFFFF], np.uint32))
    # descending ACROSS a boundary is two sorted vectors, not an error: {1, 5, 9} then {2, 3} is the valid set above;
    # equal neighbours inside a vector are sorted; an empty vector (two equal offsets) is a filter that allows nothing
    for kw in ({}, {"fi": np.array([1, 5, 5, 2, 3], np.uint64)}, {"fo": np.array([0, 0, 5], np.uint64), "fi": np.array([1, 2, 3, 5, 9], np.uint64)}):
        rc = call(**kw)
        assert rc in (N.OK, N.ERR_DEVICE), N.last_error()   # well formed: answered, or "no device" on a box without one
        if rc == N.ERR_DEVICE:
            assert "device" in N.last_error().lower()
    # the device entry checks what it can see from the host
    dev = lambda **kw: L.hnswgpu_search_batch_filter_set_device(kw.get("idx", h.handle), _p(Q), 4, 8, k, 16, _p(f_ids), _p(kw.get("fo", f_off)),
                                                                kw.get("nf", 2), _p(kw.get("of", f_of)), _p(ids), _p(dists), None, None, _p(counts),
                                                                None, None, None)
    assert dev(idx=None) == N.ERR_ARG
    assert dev(nf=0) == N.ERR_ARG and "n_filters" in N.last_error()
    assert dev(of=None) == N.ERR_ARG and "filter_of" in N.last_error()
    assert dev(fo=None) == N.ERR_ARG and "filter_offsets" in N.last_error()


def test_zero_queries_and_the_empty_index(native):
    N = _N()
    X, h = _small(native)
    # no query: nothing to do, whatever the set (even none)
    rc = native.lib().hnswgpu_search_batch_filter_set(h.handle, None, 0, 8, 3, 16, None, None, 0, None, None, None, None, None, None, None)
    assert rc == N.OK, N.last_error()
    # an index without a point answers every query with nothing (src/hnsw.rs:1498-1503)
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    Q = X[:5].copy()
    res = e.parallel_search_filters_flat(Q, 4, 16, [np.array([1, 2], np.uint64), np.zeros(0, np.uint64)], [0, 1, 1, 0, 0])
    assert res.counts.tolist() == [0] * 5 and res.status.tolist() == [0] * 5
    assert res.ids.shape == (5, 4) and res.dists.shape == (5, 4) and res.to_neighbours() == [[]] * 5


def test_python_method_checks_its_own_arguments(native):
    N = _N()
    X, h = _small(native)
    Q = X[:4].copy()
    f = [np.array([1, 5, 9], np.uint64), np.array([2, 3], np.uint64)]
    for bad in (lambda: h.parallel_search_filters_flat(Q, 3, 16, f),                       # filter_of=None: 2 filters for 4 queries
                lambda: h.parallel_search_filters_flat(Q, 3, 16, f + f + f),               # ... 6 filters for 4 queries
                lambda: h.parallel_search_filters_flat(Q, 3, 16, f, [0, 1, 0]),            # one index per query
                lambda: h.parallel_search_filters_flat(Q, 3, 16, f, [0, 1, -1, 0]),
                lambda: h.parallel_search_filters_flat(Q, 3, 16, f, [0, 1, 2, 0]),         # refused by the library: names no filter
                lambda: h.parallel_search_filters_flat(Q, 3, 16, [[9, 1]], [0, 0, 0, 0]),  # ... : not sorted
                lambda: h.parallel_search_filters_flat(Q, 3, 16, [], [0, 0, 0, 0]),
                lambda: h.parallel_search_filters_flat(Q[0], 3, 16, f, [0])):
        with pytest.raises(native.HnswError) as e:
            bad()
        assert e.value.code == N.ERR_ARG, str(e.value)
    # well formed: answered on a box with a GPU (tests/test_gpu_filter_set.py checks the answers), "no device" without one
    try:
        res = h.parallel_search_filters_flat(Q, 3, 16, f + f)
        assert all(c <= m for c, m in zip(res.counts.tolist(), [3, 2, 3, 2])) and res.status.tolist() == [0] * 4
        assert all(np.isin(res.ids[q, :res.counts[q]], (f + f)[q]).all() for q in range(4))
    except native.HnswError as e:
        assert native.lib().hnswgpu_device_count() == 0 and e.code == N.ERR_DEVICE
