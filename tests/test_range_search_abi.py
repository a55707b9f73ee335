"""The approximate range search entries (hnswgpu_range_search_batch / _device, csrc/range_search.hip) as far as a box without a GPU
can see them: the ABI, every argument check (answered before any device is needed), the empty index, the "no device" answer -- and
`range_rule`, the rounds of the contract restated in Python over ANY `search(Q, k, ef)`.  tests/test_gpu_range_search.py imports
range_rule and the fixture to build its expected answers from the oracle's search, never from the code under test.  Here the rule
is checked against a numpy model of the cut on hostile radii, and run on the oracle over the fixture, asserting what those inputs
must contain (several settling efs, saturated, empty and unsaturated-at-ef_max queries).  CPU only."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import uniform

ENTRIES = ("hnswgpu_range_search_batch", "hnswgpu_range_search_batch_device")
QUANTILES = (0, .0005, .003, .01, .03, .06, .2, .5)
PAIRS = ((8, 256), (64, 1024), (512, 2048), (1, 1), (3, 100))


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ----------------------------------------------------------------------------------------------------- the rule
def ef_sequence(ef_first, ef_max):
    """e_0 = ef_first, e_{j+1} = min(2 e_j, ef_max), up to and including ef_max"""
    seq = [ef_first]
    while seq[-1] < ef_max:
        seq.append(min(2 * seq[-1], ef_max))
    return seq


class RangeAnswer:
    """what range_rule returns: CSR offsets, the entries, per query the settling ef and the flags"""

    def __init__(self, offsets, ids, dists, layers, ranks, ef, flags):
        self.offsets, self.ids, self.dists, self.layers, self.ranks, self.ef, self.flags = offsets, ids, dists, layers, ranks, ef, flags

    @property
    def counts(self):
        return np.diff(self.offsets)


def range_rule(search, Q, radii, ef_first, ef_max):
    """The contract of hnswgpu_range_search_batch, round by round, over search(Q, k, ef) -> an object with ids, dists, layers, ranks
    (rows of width k) and counts.  Pending queries are searched again from scratch with knbn = ef = e; m is the longest prefix with
    dist <= radius (f32 values; a NaN or negative radius gives 0); a query settles when m < c, c < e or e == ef_max."""
    Q = np.ascontiguousarray(Q, np.float32)
    radii = np.asarray(radii, np.float32)
    nq = len(Q)
    rows = [None] * nq
    ef = np.zeros(nq, np.uint32)
    flags = np.zeros(nq, np.uint8)
    pending = np.arange(nq)
    for e in ef_sequence(ef_first, ef_max):
        if len(pending) == 0:
            break
        res = search(Q[pending], e, e)
        still = []
        for i, q in enumerate(pending):
            c = min(int(res.counts[i]), e)
            r = radii[q]
            m = 0
            if r >= np.float32(0):                            # (false for NaN and negative radii, true for -0.0)
                while m < c and res.dists[i, m] <= r:
                    m += 1
            if m < c or c < e or e == ef_max:
                rows[q] = (res.ids[i, :m].copy(), res.dists[i, :m].copy(), res.layers[i, :m].copy(), res.ranks[i, :m].copy())
                ef[q] = e
                flags[q] = 1 if m == c == e else 0
            else:
                still.append(q)
        pending = np.array(still, np.int64)
    assert len(pending) == 0
    offsets = np.zeros(nq + 1, np.uint64)
    if nq:
        np.cumsum([len(r[0]) for r in rows], out=offsets[1:])

    def cat(j, dtype):
        return np.concatenate([r[j] for r in rows]).astype(dtype) if nq else np.zeros(0, dtype)
    return RangeAnswer(offsets, cat(0, np.uint64), cat(1, np.float32), cat(2, np.uint8), cat(3, np.int32), ef, flags)


def radii_from_quantiles(D):
    """query i's radius: the QUANTILES[i % 8] quantile of its distance row D[i] (f32); the first of every eight is the radius 0.0"""
    r = np.array([np.quantile(D[i].astype(np.float64), QUANTILES[i % 8]) for i in range(len(D))]).astype(np.float32)
    r[0::8] = 0.0
    return r


@functools.lru_cache(maxsize=1)
def fixture():
    """The fixture of the GPU tests: 3000 uniform points of dimension 8 in an index built by the oracle (DistL2, M = 8, ef_c = 64), 300
    queries, radii from the quantiles of every query's oracle distance row.  Returns (oracle index, X, Q, radii)."""
    import oracle_lib
    X, Q = uniform(3000, 8, 1), uniform(300, 8, 2)
    o = oracle_lib.OracleHnsw(8, 3000, 16, 64, "DistL2")
    o.insert_batch(X)
    return o, X, Q, radii_from_quantiles(oracle_lib.dist_matrix("DistL2", Q, X))


@functools.lru_cache(maxsize=None)
def fixture_expected(ef_first, ef_max):
    """range_rule over the oracle's search on the fixture, computed once per (ef_first, ef_max) and shared; never modified"""
    o, X, Q, radii = fixture()
    return range_rule(o.parallel_search, Q, radii, ef_first, ef_max)


# ----------------------------------------------------------------------------------------------------- the ABI
def _small(native, n=50, d=8):
    X = np.random.default_rng(1).random((n, d), dtype=np.float32)
    h = native.Hnsw(8, n, 16, 32, "DistL2")
    h.set_build_options(nthreads=1)
    h.parallel_insert(X)
    return X, h


def test_header_parses_and_binds_both_entries_and_names_the_hook(native):
    N = _N()
    protos = N.HEADER.prototypes
    for name in ENTRIES:
        assert name in protos and name in N.SYMBOLS, name
        assert protos[name][0] is C.c_int
        assert getattr(native.lib(), name) is not None
    host, dev = protos[ENTRIES[0]][2], protos[ENTRIES[1]][2]
    assert host == ["idx", "queries", "nq", "d", "radii", "ef_first", "ef_max", "allowed_ids", "n_allowed", "cap", "out_offsets", "out_ids",
                    "out_dists", "out_layer", "out_rank", "out_ef", "out_flags"]
    assert dev == ["idx", "d_queries", "nq", "d", "d_radii", "ef_first", "ef_max", "d_allowed_ids", "n_allowed", "cap", "d_out_offsets",
                   "d_out_ids", "d_out_dists", "d_out_layer", "d_out_rank", "d_out_ef", "d_out_flags", "stream"]
    text = open(N.HEADER_PATH).read()
    assert "HNSWGPU_RANGE_CHUNK" in text
    reload_comment = text[text.index("The HNSWGPU_* tuning and test hooks"):text.index("int hnswgpu_reload_env")]
    assert "HNSWGPU_RANGE_CHUNK" in reload_comment
    for method in ("range_search_flat", "range_search", "range_recall_flat"):
        assert hasattr(native.Hnsw, method), method
    r = native.RangeResult(np.zeros(1, np.uint64), *[np.zeros(0)] * 4)
    assert r.ef is None and r.flags is None


def test_every_argument_error_is_answered_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    Q = X[:3].copy()
    rad = np.full(3, 0.5, np.float32)
    offs = np.full(4, 77, np.uint64)
    ids, dists = np.full(16, 5, np.uint64), np.full(16, 5, np.float32)
    some = np.array([1, 4, 9], np.uint64)

    def host(idx=h.handle, q=Q, d=8, r=rad, e0=4, e1=16, al=None, na=0, cap=16, of=offs, oi=ids, od=dists):
        return L.hnswgpu_range_search_batch(idx, _p(q), 3, d, _p(r), e0, e1, _p(al), na, cap, _p(of), _p(oi), _p(od), None, None, None, None)

    def dev(idx=h.handle, q=Q, d=8, r=rad, e0=4, e1=16, al=None, na=0, cap=16, of=offs, oi=ids, od=dists):
        return L.hnswgpu_range_search_batch_device(idx, _p(q), 3, d, _p(r), e0, e1, _p(al), na, cap, _p(of), _p(oi), _p(od), None, None, None, None,
                                                   None)

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
        refused("ef_first", e0=0)                         # 1 <= ef_first
        refused("ef_max", e0=17, e1=16)                   # ef_first <= ef_max
        refused("4096", e0=4, e1=4097)                    # ef_max <= 4096
        refused("4096", e0=4097, e1=4097)
        refused("filter", e0=1, e1=16, al=some, na=3)     # with a filter ef_first >= 2 ...
        refused("filter", e0=1, e1=16, al=some, na=0)     # ... also with the filter that allows nothing
        refused("filter", na=4)                           # ids announced, none given
        refused("out_ids", oi=None)                       # cap > 0 with NULL out arrays
        refused("out_dists", od=None)
    rc = host(al=np.array([5, 3, 9], np.uint64), na=3)
    assert rc == N.ERR_ARG and "sorted" in N.last_error()
    assert (offs == 77).all() and (ids == 5).all()         # nothing was written by a refused call
    for bad in ((0, 4), (5, 4), (4, 4097)):                # the Python method hands the library's answer on
        with pytest.raises(native.HnswError) as err:
            h.range_search_flat(Q, 0.5, *bad)
        assert err.value.code == N.ERR_ARG
    with pytest.raises(native.HnswError) as err:
        h.range_search_flat(Q, np.zeros(4, np.float32), 4, 16)
    assert err.value.code == N.ERR_ARG


def test_empty_index_and_zero_queries_answer_without_a_device(native):
    N = _N()
    L = native.lib()
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    Q = np.random.default_rng(2).random((5, 8), dtype=np.float32)
    res = e.range_search_flat(Q, 1.0, 4, 16)
    assert res.offsets.tolist() == [0] * 6 and res.counts.tolist() == [0] * 5 and len(res.ids) == 0
    assert res.ef.tolist() == [0] * 5 and res.flags.tolist() == [0] * 5
    assert e.range_search(Q, np.full(5, 2.0, np.float32), 4, 16) == [[]] * 5
    X, h = _small(native)
    offs = np.full(1, 9, np.uint64)
    rc = L.hnswgpu_range_search_batch(h.handle, None, 0, 8, None, 4, 16, None, 0, 0, _p(offs), None, None, None, None, None, None)
    assert rc == N.OK and offs[0] == 0


def test_without_a_device_a_well_formed_call_reports_no_device(native):
    N = _N()
    X, h = _small(native)
    Q = X[:3].copy()
    if native.lib().hnswgpu_device_count() > 0:            # a box with a GPU answers (tests/test_gpu_range_search.py checks the answer)
        res = h.range_search_flat(Q, 0.0, 4, 16)
        assert res.counts.tolist() == [1, 1, 1] and res.ef.tolist() == [4, 4, 4]
        return
    with pytest.raises(native.HnswError) as e:
        h.range_search_flat(Q, 0.5, 4, 16)
    assert e.value.code == N.ERR_DEVICE
    offs = np.zeros(4, np.uint64)
    rc = native.lib().hnswgpu_range_search_batch_device(h.handle, _p(Q), 3, 8, _p(np.zeros(3, np.float32)), 4, 16, None, 0, 0, _p(offs), None, None,
                                                        None, None, None, None, None)
    assert rc == N.ERR_DEVICE and N.last_error()


# ----------------------------------------------------------------------------------------------------- the rule against a model
def _cut_model(dists, r):
    """the cut as one numpy expression: the index of the first entry that is not <= r, 0 for a NaN or negative radius"""
    if not r >= np.float32(0):
        return 0
    fail = ~(dists <= r)
    return int(np.argmax(fail)) if fail.any() else len(dists)


class _Table:
    """a search over a table: query i (its first element is i) reaches reach[i] points, whose ascending distances are rows[i]"""

    def __init__(self, rows):
        self.rows = rows
        self.calls = []

    def __call__(self, Q, k, ef):
        assert k == ef
        which = Q[:, 0].astype(np.int64)
        self.calls.append((k, which.tolist()))

        class R:
            pass
        r = R()
        r.ids = np.zeros((len(Q), k), np.uint64)
        r.dists = np.zeros((len(Q), k), np.float32)
        r.layers = np.zeros((len(Q), k), np.uint8)
        r.ranks = np.zeros((len(Q), k), np.int32)
        r.counts = np.zeros(len(Q), np.uint32)
        for i, q in enumerate(which):
            c = min(k, len(self.rows[q]))
            r.counts[i] = c
            r.dists[i, :c] = self.rows[q][:c]
            r.ids[i, :c] = 1000 * q + np.arange(c)
            r.ranks[i, :c] = np.arange(c) + 7
            r.dists[i, c:] = -5.0                              # (what lies behind the count must never be read)
        return r


@pytest.mark.parametrize("ef_first,ef_max", [(1, 1), (2, 64), (3, 100), (8, 256), (64, 64)])
def test_range_rule_against_the_cut_model_on_hostile_radii(ef_first, ef_max):
    rng = np.random.default_rng(ef_first * 1000 + ef_max)
    rows = []
    for q in range(60):
        reach = int(rng.choice([0, 1, 5, 63, 64, 65, 100, 300]))
        dd = np.sort(rng.random(reach, dtype=np.float32))
        dd[rng.random(reach) < 0.3] = dd[reach // 2] if reach else 0      # runs of equal distances
        dd = np.sort(dd)
        if q % 5 == 0 and reach:
            dd[0] = 0.0 if q % 10 else -0.0                               # a stored vector: distance +-0
        if q % 7 == 3 and reach > 2:
            dd[-1] = np.inf
        if q % 11 == 4 and reach > 3:
            dd[-1] = np.nan                                               # (a NaN distance sorts last and never matches)
        rows.append(dd)
    hostile = [np.nan, -1.0, -0.0, 0.0, np.inf, -np.inf, 1e-30]
    radii = np.zeros(60, np.float32)
    for q in range(60):
        radii[q] = hostile[q % len(hostile)] if q % 2 == 0 or len(rows[q]) == 0 else rows[q][int(rng.integers(len(rows[q])))]   # ... or an entry's own distance
    Q = np.zeros((60, 2), np.float32)
    Q[:, 0] = np.arange(60)
    table = _Table(rows)
    got = range_rule(table, Q, radii, ef_first, ef_max)
    seq = ef_sequence(ef_first, ef_max)
    assert seq[0] == ef_first and seq[-1] == ef_max and all(b == min(2 * a, ef_max) for a, b in zip(seq, seq[1:]))
    searched = {q: [k for k, which in table.calls if q in which] for q in range(60)}
    for q in range(60):
        for e in seq:                                                      # the model: the first e that settles
            c = min(e, len(rows[q]))
            m = _cut_model(rows[q][:c], radii[q])
            if m < c or c < e or e == ef_max:
                break
        a, b = int(got.offsets[q]), int(got.offsets[q + 1])
        assert (b - a, int(got.ef[q]), int(got.flags[q])) == (m, e, int(m == c == e)), (q, radii[q])
        assert np.array_equal(got.dists[a:b].view(np.uint32), rows[q][:m].view(np.uint32)) and np.array_equal(got.ids[a:b], 1000 * q + np.arange(m))
        assert np.array_equal(got.ranks[a:b], np.arange(m) + 7)
        assert searched[q] == seq[:seq.index(e) + 1]                       # searched once per round up to its settling round, never again
        if np.isnan(radii[q]) or radii[q] < 0:
            assert m == 0
        if radii[q] == np.inf and not np.isnan(rows[q][:c]).any():
            assert m == c
    assert got.offsets[0] == 0 and got.offsets[-1] == len(got.ids)


def test_the_fixture_contains_what_the_gpu_tests_need(oracle):
    """on the ORACLE's side: several settling efs, saturated queries, empty answers, queries that reach ef_max unsaturated; the
    sequence 3, 6, ..., 96, 100 ends in a clamped step; (512, 2048) sends queries through ef above 1024"""
    o, X, Q, radii = fixture()
    assert radii[0] == 0 and (radii[0::8] == 0).all() and (radii[1::8] > 0).all() and np.isfinite(radii).all()
    want = fixture_expected(8, 256)
    assert len(set(want.ef.tolist())) >= 4, sorted(set(want.ef.tolist()))
    assert np.count_nonzero(want.flags & 1) >= 1
    assert np.count_nonzero(want.counts == 0) >= 1
    assert np.count_nonzero((want.ef == 256) & (want.flags == 0)) >= 1
    assert set(want.ef.tolist()) <= set(ef_sequence(8, 256))
    assert ((want.flags & 1) == 0)[want.ef < 256].all()                   # saturation is possible under rule (c) only
    assert (want.counts[(want.flags & 1) == 1] == 256).all()
    w = fixture_expected(3, 100)
    assert ef_sequence(3, 100)[-2:] == [96, 100] and np.count_nonzero(w.ef == 100) >= 1
    w = fixture_expected(512, 2048)
    assert np.count_nonzero(w.ef == 2048) >= 1
    w = fixture_expected(1, 1)
    assert (w.ef == 1).all() and (w.counts <= 1).all() and np.count_nonzero(w.flags & 1) >= 1
    # every answer is a prefix of ONE oracle search at the settling ef
    for q in (1, 5, 6, 7, 15):
        e = int(want.ef[q])
        ids, dists, layers, ranks = o.search(Q[q], e, e)
        m = int(want.counts[q])
        a = int(want.offsets[q])
        assert np.array_equal(want.ids[a:a + m], ids[:m]) and np.array_equal(want.dists[a:a + m].view(np.uint32), dists[:m].view(np.uint32))
        assert (dists[:m] <= radii[q]).all() and (m == len(ids) or dists[m] > radii[q])
