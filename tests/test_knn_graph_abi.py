"""The queries by stored point (hnswgpu_graph_search_batch / hnswgpu_exact_graph_batch and their _device forms, csrc/knn_graph.hip)
as far as a box without a GPU can see them: the ABI, every argument check, the "no device" answer behind the checks, and a numpy
emulation of the two rules the device applies -- the resolution of DataIds by binary search over the (id, dump order) table, and
the removal of a point's own entry from a (k + 1)-wide answer -- against brute force.  CPU only; tests/test_gpu_knn_graph.py
checks the answers, with the two emulations below as its expected values."""
import ctypes as C

import numpy as np
import pytest

ENTRIES = ("hnswgpu_graph_search_batch", "hnswgpu_graph_search_batch_device", "hnswgpu_exact_graph_batch", "hnswgpu_exact_graph_batch_device")


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


# ----------------------------------------------------------------------------------------------------- the two rules, emulated
def resolve(ids_in_dump_order, point_ids):
    """graph_resolve_kernel: (the dump position of every named point, the number of ids that name no point).  The table is the
    dump positions in ascending (id, dump position) order; per id a lower bound over the table's ids, so a repeated id names the
    first of its points in dump order.  point_ids None: every point, in the table's order."""
    ids = np.asarray(ids_in_dump_order, np.uint64)
    n = len(ids)
    order = np.argsort(ids, kind="stable")
    if point_ids is None:
        return order.copy(), 0
    flat, unknown = np.zeros(len(point_ids), np.int64), 0
    for i, v in enumerate(np.asarray(point_ids, np.uint64)):
        lo, hi = 0, n
        while lo < hi:
            mid = lo + (hi - lo) // 2
            if ids[order[mid]] < v:
                lo = mid + 1
            else:
                hi = mid
        if lo < n and ids[order[lo]] == v:
            flat[i] = order[lo]
        else:
            unknown += 1
    return flat, unknown


def drop_self(pids, own, k):
    """graph_compact_kernel on one row: pids = the (layer, rank) of the entries of a (k + 1)-wide answer, in order; own = the queried
    point's.  Returns the positions that stay, in order: without the point's own entry, or -- when there is none and the answer
    is full -- without the last one."""
    assert len(pids) <= k + 1
    keep = [j for j, p in enumerate(pids) if tuple(p) != tuple(own)]
    if len(keep) == len(pids) and len(pids) == k + 1:
        keep = keep[:k]
    return keep


def apply_drop_self(wide, own_pids, k):
    """drop_self over a whole (k + 1)-wide result (anything with ids, dists, layers, ranks, counts): the k-wide arrays the graph call
    must return -- (ids, dists, layers, ranks, counts, rows without an own entry), zeros behind the answers"""
    np_ = len(wide.counts)
    ids, dists = np.zeros((np_, k), np.uint64), np.zeros((np_, k), np.float32)
    layers, ranks, counts = np.zeros((np_, k), np.uint8), np.zeros((np_, k), np.int32), np.zeros(np_, np.uint32)
    absent = []
    for i in range(np_):
        c = int(wide.counts[i])
        pids = list(zip(wide.layers[i, :c].tolist(), wide.ranks[i, :c].tolist()))
        keep = drop_self(pids, own_pids[i], k)
        if tuple(own_pids[i]) not in pids:
            absent.append(i)
        m = len(keep)
        ids[i, :m], dists[i, :m], layers[i, :m], ranks[i, :m], counts[i] = wide.ids[i, keep], wide.dists[i, keep], wide.layers[i, keep], wide.ranks[i, keep], m
    return ids, dists, layers, ranks, counts, absent


@pytest.mark.parametrize("seed", range(6))
def test_resolution_against_brute_force(seed):
    """random id tables with repeated ids (three points per id for a part), queried with known ids, repeated queries and ids that
    name no point -- below, between and above the table's"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 200))
    ids = rng.integers(5, 5 + max(2, n // 2), n).astype(np.uint64) * 3          # repeats; every id a multiple of 3
    pts = np.concatenate([rng.choice(ids, 40), np.array([0, 4, 10 ** 15], np.uint64), rng.choice(ids, 5)]).astype(np.uint64)
    rng.shuffle(pts)
    flat, unknown = resolve(ids, pts)
    known = np.isin(pts, ids)
    assert unknown == int((~known).sum()) == 3
    for i in np.flatnonzero(known):
        assert flat[i] == np.flatnonzero(ids == pts[i])[0], (i, pts[i])           # the first point in dump order that carries the id
    allp, unknown = resolve(ids, None)
    assert unknown == 0 and sorted(allp.tolist()) == list(range(n))
    assert np.array_equal(allp, np.lexsort((np.arange(n), ids)))                 # ascending (id, dump order)
    if len(np.unique(ids)) == n:
        assert np.array_equal(ids[allp], np.sort(ids))


def test_resolution_with_ids_zero_to_n_gives_row_i_for_id_i():
    perm = np.random.default_rng(3).permutation(100).astype(np.uint64)
    allp, _ = resolve(perm, None)
    assert np.array_equal(perm[allp], np.arange(100, dtype=np.uint64))


@pytest.mark.parametrize("k", [1, 3, 10])
def test_drop_self_against_brute_force(k):
    """the three cases: own entry present (anywhere, in a full and in a short answer), absent from a full answer, absent from a
    short one"""
    rng = np.random.default_rng(k)
    seen = set()
    for _ in range(400):
        c = int(rng.integers(0, k + 2))
        pool = [(int(l), int(r)) for l in range(3) for r in range(8)]
        pids = [pool[j] for j in rng.choice(len(pool), c, replace=False)]
        present = c > 0 and rng.random() < 0.5
        own = pids[int(rng.integers(0, c))] if present else (7, 7)
        keep = drop_self(pids, own, k)
        want = [p for p in pids if p != own]
        if not present and c == k + 1:
            want = want[:-1]
        assert [pids[j] for j in keep] == want and len(keep) <= k
        assert len(keep) == (c - 1 if present else min(c, k))
        seen.add((present, c == k + 1))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}


# ----------------------------------------------------------------------------------------------------- the ABI
def test_header_parses_and_binds_the_four_entries(native):
    N = _N()
    protos = N.HEADER.prototypes
    for name in ENTRIES:
        assert name in protos and name in N.SYMBOLS, name
        assert protos[name][0] is C.c_int
        assert getattr(native.lib(), name) is not None
    outs = ["out_ids", "out_dists", "out_layer", "out_rank", "out_counts"]
    assert protos[ENTRIES[0]][2] == ["idx", "point_ids", "np", "k", "ef"] + outs
    assert protos[ENTRIES[1]][2] == ["idx", "d_point_ids", "np", "k", "ef"] + ["d_" + o for o in outs] + ["stream"]
    assert protos[ENTRIES[2]][2] == ["idx", "point_ids", "np", "k", "allowed_ids", "n_allowed"] + outs
    assert protos[ENTRIES[3]][2] == ["idx", "d_point_ids", "np", "k", "d_allowed_ids", "n_allowed"] + ["d_" + o for o in outs] + ["stream"]
    assert "HNSWGPU_GRAPH_CHUNK" in open(N.HEADER_PATH).read()
    for m in ("knn_graph_flat", "exact_knn_graph_flat", "knn_graph_recall"):
        assert hasattr(native.Hnsw, m), m


def _calls(native, h, n):
    """the four entries as functions of what a check looks at; the outputs are poisoned and must stay so"""
    L = native.lib()
    pts = np.arange(3, dtype=np.uint64)
    out = dict(oi=np.full(30, 5, np.uint64), od=np.full(30, 5, np.float32), oc=np.full(3, 5, np.uint32))

    def approx(dev):
        def call(idx=h.handle, p=pts, np_=3, k=10, al=None, na=0, oi=out["oi"], od=out["od"], oc=out["oc"]):
            if dev:
                return L.hnswgpu_graph_search_batch_device(idx, _p(p), np_, k, 32, _p(oi), _p(od), None, None, _p(oc), None)
            return L.hnswgpu_graph_search_batch(idx, _p(p), np_, k, 32, _p(oi), _p(od), None, None, _p(oc))
        return call

    def exact(dev):
        def call(idx=h.handle, p=pts, np_=3, k=10, al=None, na=0, oi=out["oi"], od=out["od"], oc=out["oc"]):
            if dev:
                return L.hnswgpu_exact_graph_batch_device(idx, _p(p), np_, k, _p(al), na, _p(oi), _p(od), None, None, _p(oc), None)
            return L.hnswgpu_exact_graph_batch(idx, _p(p), np_, k, _p(al), na, _p(oi), _p(od), None, None, _p(oc))
        return call
    return [("approx host", approx(False), False), ("approx device", approx(True), False), ("exact host", exact(False), True),
            ("exact device", exact(True), True)], out


def test_every_argument_error_names_the_offender(native):
    N = _N()
    n = 50
    X, h = _small(native, n)
    calls, out = _calls(native, h, n)
    for name, call, is_exact in calls:
        def refused(word, **kw):
            rc = call(**kw)
            assert rc == N.ERR_ARG, (name, kw.keys(), rc, N.last_error())
            assert word in N.last_error(), (name, word, N.last_error())
        refused("null", idx=None)
        refused("null buffer", oi=None)
        refused("null buffer", od=None)
        refused("null buffer", oc=None)
        refused("nb_point", p=None, np_=3)                 # NULL ids mean every point: np must be nb_point
        refused("nb_point", p=None, np_=n + 1)
        refused("knbn", k=0)
        if is_exact:
            refused("4096", k=4097)
            refused("filter", na=4)                        # ids announced, none given
            h.set_arithmetic("simd8")
            try:
                refused("SIMD8")
            finally:
                h.set_arithmetic("scalar")
        if name == "exact host":
            refused("sorted", al=np.array([5, 3, 9], np.uint64), na=3)
    for o in out.values():
        assert (o == 5).all()                              # nothing was written by a refused call


def test_then_comes_no_device(native):
    """a well-formed call on a box without a GPU: HNSWGPU_ERR_DEVICE from all four entries, k = 4096 and SIMD-order arithmetic of
    the APPROXIMATE call included (they are the exact call's limits only)"""
    N = _N()
    n = 50
    X, h = _small(native, n)
    if native.lib().hnswgpu_device_count() > 0:            # a box with a GPU answers (tests/test_gpu_knn_graph.py checks the answers)
        assert h.exact_knn_graph_flat(3).counts.tolist() == [3] * n and h.knn_graph_flat(3, 32).counts.tolist() == [3] * n
        return
    calls, out = _calls(native, h, n)
    big = dict(oi=np.zeros(3 * 4097, np.uint64), od=np.zeros(3 * 4097, np.float32))
    for name, call, is_exact in calls:
        assert call() == N.ERR_DEVICE and N.last_error(), name
        assert call(k=4096 if is_exact else 4097, **big) == N.ERR_DEVICE, name
        allp = dict(oi=np.zeros(n * 10, np.uint64), od=np.zeros(n * 10, np.float32), oc=np.zeros(n, np.uint32))
        assert call(p=None, np_=n, **allp) == N.ERR_DEVICE, name
    for m in (lambda: h.knn_graph_flat(5, 32), lambda: h.exact_knn_graph_flat(5, [1, 2]), lambda: h.knn_graph_recall(5, 32, [0])):
        with pytest.raises(native.HnswError) as e:
            m()
        assert e.value.code == N.ERR_DEVICE


def test_no_points_and_the_empty_index(native):
    N = _N()
    X, h = _small(native)
    for res in (h.knn_graph_flat(4, 32, []), h.exact_knn_graph_flat(4, [])):      # no point named: nothing to do, no device needed
        assert res.ids.shape == (0, 4) and res.counts.shape == (0,)
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    for res in (e.knn_graph_flat(4, 32), e.exact_knn_graph_flat(4)):              # every point of an empty index
        assert res.ids.shape == (0, 4)
    for m in (lambda: e.knn_graph_flat(4, 32, [3]), lambda: e.exact_knn_graph_flat(4, [3, 4])):
        with pytest.raises(native.HnswError) as err:
            m()
        assert err.value.code == N.ERR_ARG and "name no point" in str(err.value)
