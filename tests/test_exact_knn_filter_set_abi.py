"""The exact k-NN entries for a set of filters (hnswgpu_exact_search_batch_filter_set / _device, Hnsw.exact_search_filters_flat,
Hnsw.recall_filters_flat) as far as a box without a GPU can see them: the prototypes generated from the header, every
HNSWGPU_ERR_ARG case of the host entry with its message, the "no device" answer, the empty index, the Python methods' own checks,
and a numpy emulation of a MIXED tile -- 16 queries with a mask each, the union skip of a 64-row step, the threshold lists, the
merge -- against np.lexsort restricted per query.  CPU only; tests/test_gpu_exact_knn_filter_set.py checks the answers."""
import ctypes as C

import numpy as np
import pytest

from test_exact_knn_abi import KEY_NONE, SlabList, _order_bits

ENTRIES = ("hnswgpu_exact_search_batch_filter_set", "hnswgpu_exact_search_batch_filter_set_device")


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
    assert host == ["idx", "queries", "nq", "d", "k", "filter_ids", "filter_offsets", "n_filters", "filter_of", "out_ids", "out_dists",
                    "out_layer", "out_rank", "out_counts"]
    assert dev == ["idx", "d_queries", "nq", "d", "k", "d_filter_ids", "d_filter_offsets", "n_filters", "d_filter_of", "d_out_ids",
                   "d_out_dists", "d_out_layer", "d_out_rank", "d_out_counts", "stream"]
    # the filter arguments of the search's filter-set pair, the outputs of the exact pair
    assert host[5:9] == protos["hnswgpu_search_batch_filter_set"][2][6:10]
    assert dev[5:9] == protos["hnswgpu_search_batch_filter_set_device"][2][6:10]
    assert host[-5:] == protos["hnswgpu_exact_search_batch"][2][-5:]
    assert dev[-6:] == protos["hnswgpu_exact_search_batch_device"][2][-6:]
    assert [a for a in protos[ENTRIES[0]][1][5:9]] == [a for a in protos["hnswgpu_search_batch_filter_set"][1][6:10]]
    # the package's copy of the header is the tree's
    import os
    tree = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnsw_mi355x.h")
    assert open(N.HEADER_PATH, "rb").read() == open(tree, "rb").read()
    pkg = os.path.join(os.path.dirname(N.__file__), "hnsw_mi355x.h")
    assert open(pkg, "rb").read() == open(tree, "rb").read()
    text = open(tree).read()
    assert "does NOT depend on how the queries are grouped into tiles, groups or chunks" in text


def test_every_argument_error_of_the_host_entry_names_what_is_wrong(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    Q = X[:4].copy()
    k = 3
    ids, dists, counts = np.zeros((4, k), np.uint64), np.zeros((4, k), np.float32), np.full(4, 99, np.uint32)
    f_ids = np.array([1, 5, 9, 2, 3], np.uint64)          # filter 0 = {1, 5, 9}, filter 1 = {2, 3}
    f_off = np.array([0, 3, 5], np.uint64)
    f_of = np.array([0, 1, 1, 0], np.uint32)

    def call(idx=h.handle, q=Q, nq=4, d=8, k=k, fi=f_ids, fo=f_off, nf=2, of=f_of, oi=ids, od=dists, oc=counts):
        return L.hnswgpu_exact_search_batch_filter_set(idx, _p(q), nq, d, k, _p(fi), _p(fo), nf, _p(of), _p(oi), _p(od), None, None, _p(oc))

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
    refused("knbn", k=0)
    refused("4096", k=4097)
    refused("dimension", d=7)
    # the checks of the set come first: a bad set with a bad k is reported as the bad set
    refused("start at 0", fo=np.array([1, 3, 5], np.uint64), k=0)
    refused("filter_of[2] = 2", of=np.array([0, 1, 2, 0], np.uint32), d=7)
    h.set_arithmetic("simd8")
    try:
        refused("SIMD8")
        refused("ascend", fo=np.array([0, 4, 3], np.uint64))
        rc = L.hnswgpu_exact_search_batch_filter_set_device(h.handle, _p(Q), 4, 8, k, _p(f_ids), _p(f_off), 2, _p(f_of), _p(ids), _p(dists), None,
                                                            None, _p(counts), None)
        assert rc == N.ERR_ARG and "SIMD8" in N.last_error()
    finally:
        h.set_arithmetic("scalar")
    # well formed (descending ACROSS a boundary is two sorted vectors; equal neighbours are sorted; an empty vector is a filter):
    # answered, or "no device" on a box without one -- never a crash
    for kw in ({}, {"fi": np.array([1, 5, 5, 2, 3], np.uint64)}, {"fo": np.array([0, 0, 5], np.uint64), "fi": np.array([1, 2, 3, 5, 9], np.uint64)}):
        counts[:] = 99
        rc = call(**kw)
        if L.hnswgpu_device_count() == 0:
            assert rc == N.ERR_DEVICE and "device" in N.last_error().lower(), (rc, N.last_error())
        else:
            assert rc == N.OK, N.last_error()
        counts[:] = 99
    # the device entry checks what it can see from the host
    dev = lambda **kw: L.hnswgpu_exact_search_batch_filter_set_device(
        kw.get("idx", h.handle), _p(kw.get("q", Q)), 4, kw.get("d", 8), kw.get("k", k), _p(f_ids), _p(kw.get("fo", f_off)), kw.get("nf", 2),
        _p(kw.get("of", f_of)), _p(kw.get("oi", ids)), _p(dists), None, None, _p(counts), None)
    assert dev(idx=None) == N.ERR_ARG
    assert dev(q=None) == N.ERR_ARG and "null buffer" in N.last_error()
    assert dev(oi=None) == N.ERR_ARG and "null buffer" in N.last_error()
    assert dev(nf=0) == N.ERR_ARG and "n_filters" in N.last_error()
    assert dev(of=None) == N.ERR_ARG and "filter_of" in N.last_error()
    assert dev(fo=None) == N.ERR_ARG and "filter_offsets" in N.last_error()
    assert dev(k=0) == N.ERR_ARG and "knbn" in N.last_error()
    assert dev(k=4097) == N.ERR_ARG and "4096" in N.last_error()
    assert dev(d=7) == N.ERR_ARG and "dimension" in N.last_error()
    if L.hnswgpu_device_count() == 0:
        assert dev() == N.ERR_DEVICE and N.last_error()


def test_zero_queries_and_the_empty_index(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    rc = L.hnswgpu_exact_search_batch_filter_set(h.handle, None, 0, 8, 3, None, None, 0, None, None, None, None, None, None)
    assert rc == N.OK, N.last_error()
    rc = L.hnswgpu_exact_search_batch_filter_set_device(h.handle, None, 0, 8, 3, None, None, 0, None, None, None, None, None, None, None)
    assert rc == N.OK, N.last_error()
    # an index without a point: counts and outputs zeroed, by the Python method and by the entry itself
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    Q = X[:5].copy()
    res = e.exact_search_filters_flat(Q, 4, [np.array([1, 2], np.uint64), np.zeros(0, np.uint64)], [0, 1, 1, 0, 0])
    assert res.counts.tolist() == [0] * 5 and res.ids.shape == (5, 4) and res.to_neighbours() == [[]] * 5
    assert e.exact_search_filters(Q, 4, [[1, 2]], [0] * 5) == [[]] * 5
    assert e.recall_filters_flat(Q, 4, 16, [[1, 2]], [0] * 5) == (1.0, 1.0)
    e.parallel_insert(np.zeros((0, 8), np.float32))   # now there is a handle, still without a point: the entry itself answers
    assert e.handle is not None and e.get_nb_point() == 0
    ids, dists = np.full((5, 4), 7, np.uint64), np.full((5, 4), 7, np.float32)
    layers, ranks, counts = np.full((5, 4), 7, np.uint8), np.full((5, 4), 7, np.int32), np.full(5, 7, np.uint32)
    f_ids, f_off, f_of = np.array([1, 2], np.uint64), np.array([0, 2], np.uint64), np.zeros(5, np.uint32)
    rc = L.hnswgpu_exact_search_batch_filter_set(e.handle, _p(Q), 5, 8, 4, _p(f_ids), _p(f_off), 1, _p(f_of), _p(ids), _p(dists), _p(layers),
                                                 _p(ranks), _p(counts))
    assert rc == N.OK, N.last_error()
    assert not counts.any() and not ids.any() and not dists.any() and not layers.any() and not ranks.any()


def test_python_methods_check_their_own_arguments(native):
    N = _N()
    X, h = _small(native)
    Q = X[:4].copy()
    f = [np.array([1, 5, 9], np.uint64), np.array([2, 3], np.uint64)]
    for m in (lambda *a: h.exact_search_filters_flat(a[0], 3, *a[1:]), lambda *a: h.exact_search_filters(a[0], 3, *a[1:]),
              lambda *a: h.recall_filters_flat(a[0], 3, 16, *a[1:])):
        for bad in (lambda: m(Q, f),                       # filter_of=None: 2 filters for 4 queries
                    lambda: m(Q, f + f + f),               # ... 6 filters for 4 queries
                    lambda: m(Q, f, [0, 1, 0]),            # one index per query
                    lambda: m(Q, f, [[0, 1], [0, 1]]),     # a wrong shape
                    lambda: m(Q, f, [0, 1, -1, 0]),
                    lambda: m(Q, f, [0, 1, 2 ** 32, 0]),
                    lambda: m(Q, f, [0, 1, 2, 0]),         # refused by the library: names no filter
                    lambda: m(Q, [[9, 1]], [0, 0, 0, 0]),  # ... : not sorted
                    lambda: m(Q, [], [0, 0, 0, 0]),
                    lambda: m(Q[0], f, [0])):
            with pytest.raises(native.HnswError) as e:
                bad()
            assert e.value.code == N.ERR_ARG, str(e.value)
    with pytest.raises(native.HnswError) as e:
        h.exact_search_filters_flat(Q, 0, f + f)
    assert e.value.code == N.ERR_ARG
    # well formed: answered on a box with a GPU, "no device" without one
    try:
        res = h.exact_search_filters_flat(Q, 3, f + f)
        assert res.counts.tolist() == [3, 2, 3, 2] and res.status is None
        assert all(np.isin(res.ids[q, :res.counts[q]], (f + f)[q]).all() for q in range(4))
    except native.HnswError as e:
        assert native.lib().hnswgpu_device_count() == 0 and e.code == N.ERR_DEVICE


# ------------------------------------------------------------------------------------------- emulation of a mixed tile
def _emulate_tile(D, rank, k, slab_rows, tword, allow, words, nvalid):
    """exact_knn_slab_kernel<METRIC, true> for one tile and exact_knn_merge_kernel for its queries.  D[t]: the distances of the
    tile's query t; allow: the group's bitmaps, `words` u32 per slot, behind one another; tword[t]: first word of the bitmap of
    query t's filter (0 for the slots behind the last query).  Returns per query the merged keys and how many 64-row steps ran."""
    n = D.shape[1]
    cap = min(k, n)
    keys = [(_order_bits(D[t]).astype(np.uint64) << np.uint64(32)) | rank.astype(np.uint64) for t in range(16)]
    valid_bits = (1 << nvalid) - 1
    one_filter = all(t >= nvalid or tword[t] == tword[0] for t in range(16))
    lists, steps = [], 0
    for lo in range(0, n, slab_rows):
        hi = min(n, lo + slab_rows)
        sl = [SlabList(cap) for _ in range(16)]
        for r0 in range(lo, hi, 64):
            rows = np.arange(r0, min(hi, r0 + 64))
            if one_filter:
                bit = (allow[tword[0] + (rows >> 5)] >> (rows & 31).astype(np.uint32)) & 1
                elig = np.where(bit != 0, valid_bits, 0)
            else:
                elig = np.zeros(len(rows), np.int64)
                for t in range(16):   # one word per query and lane; the padding slots read slot 0 and are masked off
                    elig |= ((allow[tword[t] + (rows >> 5)] >> (rows & 31).astype(np.uint32)) & 1).astype(np.int64) << t
                elig &= valid_bits
            if not elig.any():        # the wave-uniform skip: no row of the step is eligible for ANY query
                continue
            steps += 1
            for t in range(nvalid):
                sl[t].offer_wave([keys[t][r] for r in rows], ((elig >> t) & 1).astype(bool))
        lists.append(sl)
    out = []
    for t in range(16):
        per_slab = [s[t].keys for s in lists]
        assert all(x == sorted(x) for x in per_slab)
        if t >= nvalid:
            assert not any(per_slab), "a slot behind the last query inserted"
            continue
        heads, got = [0] * len(per_slab), []
        for _ in range(min(k, sum(len(x) for x in per_slab))):
            cur = [lst[h] if h < len(lst) else KEY_NONE for lst, h in zip(per_slab, heads)]
            s = int(np.argmin(np.array(cur, np.uint64)))
            got.append(cur[s])
            heads[s] += 1
        out.append(np.array(got, np.uint64))
    return out, steps


def _bitmaps(masks, words):
    """allow_bitmap_set_kernel's layout: slot s in words [s words, (s + 1) words), bit f % 32 of word f / 32; bits past n are zero"""
    allow = np.zeros(len(masks) * words, np.uint32)
    for s, m in enumerate(masks):
        for f in np.flatnonzero(m):
            allow[s * words + (f >> 5)] |= np.uint32(1) << np.uint32(f & 31)
    return allow


@pytest.mark.parametrize("n,k,slab_rows,nvalid,levels", [(1000, 10, 256, 16, 7), (777, 64, 320, 5, 3), (2450, 100, 640, 16, 4000),
                                                        (65, 65, 64, 1, 1), (300, 7, 64, 11, 2)])
def test_mixed_tile_emulation_against_lexsort_per_query(n, k, slab_rows, nvalid, levels):
    """16 queries naming seven filters -- empty, one id, ~1 %, ~50 %, every id, one whose rows lie inside a single 64-row step, and
    the ~50 % one less the last row -- so that the union skip sees steps that are eligible for some queries only; distances with
    heavy duplication: every query's answer is the lexsort by (distance, DataId rank) of ITS OWN allowed rows.  W = ceil(n / 32)
    is odd for some n: a slot's last word abuts the next slot's first."""
    rng = np.random.default_rng(n * 7 + k)
    words = (n + 31) // 32
    half = rng.random(n) < 0.5
    half[n - 1] = True
    step = np.zeros(n, bool)
    step[(n // 128) * 64:(n // 128) * 64 + 64][::3] = True
    less = half.copy()
    less[n - 1] = False
    one = np.zeros(n, bool)
    one[n // 3] = True
    masks = [np.zeros(n, bool), one, rng.random(n) < 0.01, half, np.ones(n, bool), step, less]
    allow = _bitmaps(masks, words)
    rank = rng.permutation(n).astype(np.uint32)
    D = (rng.integers(0, levels, (16, n)) / np.float32(levels)).astype(np.float32)
    if n > 100:
        D[:, rng.choice(n, 5, replace=False)] = np.nan
    for trial, slot_of in enumerate(((np.arange(16) * 3 + 1) % 7, np.array([5, 4, 0] * 5 + [5]), np.full(16, 3), np.array([0, 5] * 8))):
        tword = [int(slot_of[t]) * words if t < nvalid else 0 for t in range(16)]
        got, steps = _emulate_tile(D, rank, k, slab_rows, tword, allow, words, nvalid)
        assert len(got) == nvalid
        for t in range(nvalid):
            rows = np.flatnonzero(masks[slot_of[t]])
            want_rows = rows[np.lexsort((rank[rows], D[t, rows]))][:k]
            want = (_order_bits(D[t, want_rows]).astype(np.uint64) << np.uint64(32)) | rank[want_rows].astype(np.uint64)
            assert np.array_equal(got[t], want), (trial, t, int(slot_of[t]))
        used = set(int(s) for s in slot_of[:nvalid])
        if used <= {0, 5}:   # only the empty filter and the one-step filter: every other 64-row step is skipped
            assert steps <= 2 * ((n + slab_rows - 1) // slab_rows) and (steps >= 1) == (5 in used)
        if used == {0}:
            assert steps == 0
