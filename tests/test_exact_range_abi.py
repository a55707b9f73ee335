"""The exact range search entries (hnswgpu_exact_range_search_batch / _device, csrc/exact_range.hip) as far as a box without a GPU can
see them: the ABI, every argument check with its message, the empty index, the "no device" answer, and a numpy emulation of the
device's plan -- counters per (query, slab), the scan in query-major and slab-minor order, the write bases, the fill pass's chunks
and the ballot-prefix compaction -- against brute force.  CPU only; tests/test_gpu_exact_range.py checks the answers."""
import ctypes as C

import numpy as np
import pytest

ENTRIES = ("hnswgpu_exact_range_search_batch", "hnswgpu_exact_range_search_batch_device")


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


def test_header_parses_and_binds_both_entries_and_the_status(native):
    N = _N()
    protos = N.HEADER.prototypes
    for name in ENTRIES:
        assert name in protos and name in N.SYMBOLS, name
        assert protos[name][0] is C.c_int
        assert getattr(native.lib(), name) is not None
    host, dev = protos[ENTRIES[0]][2], protos[ENTRIES[1]][2]
    assert host == ["idx", "queries", "nq", "d", "radii", "allowed_ids", "n_allowed", "cap", "out_offsets", "out_ids", "out_dists", "out_layer",
                    "out_rank"]
    assert dev == ["idx", "d_queries", "nq", "d", "d_radii", "d_allowed_ids", "n_allowed", "cap", "d_out_offsets", "d_out_ids", "d_out_dists",
                   "d_out_layer", "d_out_rank", "stream"]
    assert N.HEADER.constants["HNSWGPU_ERR_CAPACITY"] == 9 and N.ERR_CAPACITY == 9
    assert native.HnswError(N.ERR_CAPACITY, "x").code == 9
    assert "HNSWGPU_RANGE_HITS_PER_PASS" in open(N.HEADER_PATH).read()
    assert hasattr(native, "RangeResult") and hasattr(native.Hnsw, "exact_range_search_flat") and hasattr(native.Hnsw, "exact_range_search")


def test_every_argument_error_names_the_offender(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    Q = X[:3].copy()
    rad = np.full(3, 0.5, np.float32)
    offs = np.full(4, 77, np.uint64)
    ids, dists = np.full(16, 5, np.uint64), np.full(16, 5, np.float32)

    def host(idx=h.handle, q=Q, d=8, r=rad, al=None, na=0, cap=16, of=offs, oi=ids, od=dists):
        return L.hnswgpu_exact_range_search_batch(idx, _p(q), 3, d, _p(r), _p(al), na, cap, _p(of), _p(oi), _p(od), None, None)

    def dev(idx=h.handle, q=Q, d=8, r=rad, al=None, na=0, cap=16, of=offs, oi=ids, od=dists):
        return L.hnswgpu_exact_range_search_batch_device(idx, _p(q), 3, d, _p(r), _p(al), na, cap, _p(of), _p(oi), _p(od), None, None, None)

    for call in (host, dev):
        def refused(word, **kw):
            rc = call(**kw)
            assert rc == N.ERR_ARG, (kw.keys(), rc, N.last_error())
            assert word in N.last_error(), (word, N.last_error())
        refused("null", idx=None)
        refused("queries", q=None)
        refused("radii", r=None)
        refused("out_offsets", of=None)
        refused("dimension", d=7)
        refused("out_ids", oi=None)                       # cap > 0 with NULL out arrays
        refused("out_dists", od=None)
        refused("filter", na=4)                           # ids announced, none given
        h.set_arithmetic("simd8")
        try:
            refused("SIMD8")
        finally:
            h.set_arithmetic("scalar")
    rc = host(al=np.array([5, 3, 9], np.uint64), na=3)
    assert rc == N.ERR_ARG and "sorted" in N.last_error()
    assert (offs == 77).all() and (ids == 5).all()         # nothing was written by a refused call


def test_empty_index_and_zero_queries_answer_without_a_device(native):
    N = _N()
    L = native.lib()
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    Q = np.random.default_rng(2).random((5, 8), dtype=np.float32)
    res = e.exact_range_search_flat(Q, 1.0)
    assert res.offsets.tolist() == [0] * 6 and res.counts.tolist() == [0] * 5 and len(res.ids) == 0
    assert res.to_neighbours() == [[]] * 5 and e.exact_range_search(Q, np.full(5, 2.0, np.float32)) == [[]] * 5
    X, h = _small(native)
    offs = np.full(1, 9, np.uint64)
    rc = L.hnswgpu_exact_range_search_batch(h.handle, None, 0, 8, None, None, 0, 0, _p(offs), None, None, None, None)
    assert rc == N.OK and offs[0] == 0
    with pytest.raises(native.HnswError) as err:           # the Python method's own check
        h.exact_range_search_flat(Q, np.zeros(4, np.float32))
    assert err.value.code == N.ERR_ARG


def test_without_a_device_a_well_formed_call_reports_no_device(native):
    N = _N()
    X, h = _small(native)
    Q = X[:3].copy()
    if native.lib().hnswgpu_device_count() > 0:            # a box with a GPU answers (tests/test_gpu_exact_range.py checks the answer)
        assert h.exact_range_search_flat(Q, 0.0).counts.tolist() == [1, 1, 1]
        return
    with pytest.raises(native.HnswError) as e:
        h.exact_range_search_flat(Q, 0.5)
    assert e.value.code == N.ERR_DEVICE
    offs = np.zeros(4, np.uint64)
    rc = native.lib().hnswgpu_exact_range_search_batch_device(h.handle, _p(Q), 3, 8, _p(np.zeros(3, np.float32)), None, 0, 0, _p(offs), None, None,
                                                              None, None, None)
    assert rc == N.ERR_DEVICE and N.last_error()


def test_range_result_views(native):
    offs = np.array([0, 2, 2, 5], np.uint64)
    r = native.RangeResult(offs, np.arange(5, dtype=np.uint64), np.arange(5, dtype=np.float32), np.zeros(5, np.uint8), np.arange(5, dtype=np.int32))
    assert r.counts.tolist() == [2, 0, 3]
    ids, dists, layers, ranks = r.of(2)
    assert ids.tolist() == [2, 3, 4] and ids.base is not None and len(r.of(1)[0]) == 0
    nb = r.to_neighbours()
    assert [len(x) for x in nb] == [2, 0, 3] and nb[2][1] == native.Neighbour(3, 3.0, (0, 3))


# ----------------------------------------------------------------------------------------------------- the plan, emulated
def _chunk_end(offs, qa, q_end, budget, max_q):
    """range_chunk_end of exact_range.hip: consecutive queries whose answers fit the budget, at most max_q, one at least"""
    qb = qa + 1
    while qb < q_end and qb - qa < max_q and offs[qb + 1] - offs[qa] <= budget:
        qb += 1
    return qb


def _emulate(hit, key, slab_rows, budget, max_q):
    """hit[q, r], key[q, r] -> the offsets and every query's sorted keys as the device produces them: the count pass's counters
    [q][slab], the scan (query major, slab minor) into offsets and (query, slab) bases, then per chunk of the plan the fill pass --
    per (tile, slab) wavefront, 64 rows at a time, the hitting lanes write at base + ballot prefix -- a sort per segment"""
    nq, n = hit.shape
    n_slabs = (n + slab_rows - 1) // slab_rows
    cnt = np.array([[int(hit[q, s * slab_rows:(s + 1) * slab_rows].sum()) for s in range(n_slabs)] for q in range(nq)], np.int64).reshape(nq, n_slabs)
    flat = cnt.reshape(-1)
    excl = np.concatenate([[0], np.cumsum(flat)])[:-1].reshape(nq, n_slabs)       # the scan: query major, slab minor
    offs = np.concatenate([excl[:, 0], [flat.sum()]]).astype(np.int64)
    pref = excl - excl[:, :1]                                                      # what the counters hold after the scan
    answers, chunks = [None] * nq, []
    qa = 0
    while qa < nq:
        qb = _chunk_end(offs, qa, nq, budget, max_q)
        chunks.append((qa, qb))
        hits = int(offs[qb] - offs[qa])
        slots = np.full(hits, -1, np.int64)
        written = np.zeros(hits, np.int64)
        for tile0 in range(qa, qb, 16):                                           # tiles are formed from the chunk's first query
            for s in range(n_slabs):
                lo, hi = s * slab_rows, min(n, (s + 1) * slab_rows)
                for q in range(tile0, min(qb, tile0 + 16)):
                    pos = int(offs[q] - offs[qa] + pref[q, s])
                    for r0 in range(lo, hi, 64):
                        lanes = np.flatnonzero(hit[q, r0:min(hi, r0 + 64)])
                        for j, lane in enumerate(lanes):                          # the ballot's prefix: hitting lanes below this one
                            slots[pos + j] = key[q, r0 + lane]
                            written[pos + j] += 1
                        pos += len(lanes)
        assert (written == 1).all()                                              # every slot exactly once: the bases are disjoint
        for q in range(qa, qb):
            answers[q] = np.sort(slots[offs[q] - offs[qa]:offs[q + 1] - offs[qa]])
        qa = qb
    return offs, answers, chunks


@pytest.mark.parametrize("n,nq,slab_rows,budget,max_q", [(1000, 37, 256, 300, 1 << 20), (777, 50, 320, 40, 1 << 20), (300, 33, 64, 10 ** 9, 1 << 20),
                                                         (65, 20, 64, 1, 1 << 20), (1, 5, 64, 3, 1 << 20), (500, 70, 512, 2000, 16)])
def test_plan_and_write_bases_against_brute_force(n, nq, slab_rows, budget, max_q):
    """random hit matrices with runs of empty queries and one query that hits every row (more than the budget): the offsets are
    the brute-force counts, every chunk but a single-query one fits the budget, chunks tile the batch in order, and every query's
    sorted slots are its brute-force keys"""
    rng = np.random.default_rng(n * 7 + nq)
    hit = rng.random((nq, n)) < rng.choice([0.0, 0.01, 0.2, 0.9], nq)[:, None]
    hit[nq // 2] = True                                      # one query larger than the budget (where the budget is small)
    hit[3:9] = False                                         # a run of empty queries, and the batch's last ones
    hit[nq - 2:] = False
    key = rng.permutation(nq * n).reshape(nq, n).astype(np.int64)
    offs, answers, chunks = _emulate(hit, key, slab_rows, budget, max_q)
    assert offs[0] == 0 and np.array_equal(np.diff(offs), hit.sum(1))
    assert chunks[0][0] == 0 and chunks[-1][1] == nq and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    for qa, qb in chunks:
        assert qb > qa and qb - qa <= max_q
        assert qb - qa == 1 or offs[qb] - offs[qa] <= budget
        if qb < nq and qb - qa < max_q:                      # greedy: the next query would not have fitted
            assert offs[qb + 1] - offs[qa] > budget
    if n * 1 > budget:
        assert (nq // 2, nq // 2 + 1) in chunks
    for q in range(nq):
        assert np.array_equal(answers[q], np.sort(key[q, hit[q]])), q
