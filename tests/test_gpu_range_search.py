"""Approximate range search on the device (Hnsw.range_search_flat -> hnswgpu_range_search_batch / _device, csrc/range_search.hip):
the graph's answers cut at a radius, ef doubled until the result set reaches past the ball.

The expected answers never come from the code under test: they are `range_rule` (tests/test_range_search_abi.py: the contract's
rounds restated in Python) over the CPU oracle's parallel_search / parallel_search_filter -- the reference's `search`.  Every
comparison is exact: offsets, ids, f32 bits, (layer, rank), ef, flags.  As a second opinion the same rule runs over the device's
own parallel_search_flat.  The indexes are built by the oracle, dumped and loaded by the product, so both sides walk one graph.
What the inputs must contain is asserted on the oracle's side."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import probability, uniform
from test_range_search_abi import PAIRS, ef_sequence, fixture, fixture_expected, radii_from_quantiles, range_rule

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _same(got, want, what=""):
    """a RangeResult against a RangeAnswer: everything, bit for bit"""
    assert np.array_equal(got.offsets, want.offsets), (what, "offsets", np.flatnonzero(got.offsets != want.offsets)[:4])
    assert np.array_equal(got.ef, want.ef), (what, "ef", np.flatnonzero(got.ef != want.ef)[:4])
    assert np.array_equal(got.flags, want.flags), (what, "flags", np.flatnonzero(got.flags != want.flags)[:4])
    assert np.array_equal(got.ids, want.ids), (what, "ids", np.flatnonzero(got.ids != want.ids)[:4])
    assert np.array_equal(got.dists.view(np.uint32), want.dists.view(np.uint32)), (what, "f32 bits")
    assert np.array_equal(got.layers, want.layers) and np.array_equal(got.ranks, want.ranks), (what, "p_ids")


def _load(native, o, tmp, metric):
    o.file_dump(str(tmp), "r")
    h = native.HnswIo(str(tmp), "r").load_hnsw(metric)
    h.upload(0)
    return h


@pytest.fixture(scope="module")
def fx(native, oracle, tmp_path_factory):
    """the fixture of tests/test_range_search_abi.py, loaded by the product"""
    o, X, Q, radii = fixture()
    return dict(h=_load(native, o, tmp_path_factory.mktemp("fx"), "DistL2"), o=o, X=X, Q=Q, radii=radii)


def _raw(native, h, Q, radii, ef_first, ef_max, cap, with_out=True, allowed=None, with_ids=True):
    """the host entry itself: (rc, offsets, [ids, dists, layers, ranks], ef, flags), the out arrays pre-filled with a sentinel"""
    nq, d = Q.shape
    offs = np.full(nq + 1, 0x5A5A5A5A, np.uint64)
    outs = [np.frombuffer(b"\xA5" * (max(cap, 1) * w), dtype=t).copy() for w, t in ((8, np.uint64), (4, np.float32), (1, np.uint8), (4, np.int32))]
    ptrs = [_p(o) if with_out else None for o in outs]
    if not with_ids:
        ptrs[0] = None
    ef, flags = np.full(nq, 0xEEEE, np.uint32), np.full(nq, 0xEE, np.uint8)
    rc = native.lib().hnswgpu_range_search_batch(h.handle, _p(Q), nq, d, _p(radii), ef_first, ef_max, _p(allowed), 0 if allowed is None else len(allowed),
                                                 cap, _p(offs), *ptrs, _p(ef), _p(flags))
    return rc, offs, outs, ef, flags


# ----------------------------------------------------------------------------------------------------- 1, 2. the pairs, whole and in groups
def test_the_fixture_is_the_one_the_oracle_was_asked_about(fx):
    """the preconditions, on the oracle's side (tests/test_range_search_abi.py asserts the rest)"""
    want = fixture_expected(8, 256)
    assert len(set(want.ef.tolist())) >= 4 and (want.flags & 1).any() and (want.counts == 0).any() and ((want.ef == 256) & (want.flags == 0)).any()
    assert (fixture_expected(512, 2048).ef == 2048).any()                 # a round through the literal-heap kernel


@pytest.mark.parametrize("ef_first,ef_max", PAIRS)
def test_pairs_against_the_oracle_and_the_device_search(native, fx, ef_first, ef_max):
    h, Q, radii = fx["h"], fx["Q"], fx["radii"]
    got = h.range_search_flat(Q, radii, ef_first, ef_max)
    _same(got, fixture_expected(ef_first, ef_max), f"({ef_first}, {ef_max}) oracle")
    _same(got, range_rule(h.parallel_search_flat, Q, radii, ef_first, ef_max), f"({ef_first}, {ef_max}) device search")
    assert set(got.ef.tolist()) <= set(ef_sequence(ef_first, ef_max))


@pytest.mark.parametrize("chunk", [7, 1])
@pytest.mark.parametrize("ef_first,ef_max", PAIRS)
def test_pairs_in_groups(native, fx, knob, ef_first, ef_max, chunk):
    """HNSWGPU_RANGE_CHUNK = 7: 43 groups, the last of 6 queries; = 1: a group per query.  The answers are identical."""
    h, Q, radii = fx["h"], fx["Q"], fx["radii"]
    assert len(Q) == 42 * 7 + 6
    knob("HNSWGPU_RANGE_CHUNK", chunk)
    _same(h.range_search_flat(Q, radii, ef_first, ef_max), fixture_expected(ef_first, ef_max), f"({ef_first}, {ef_max}) chunk {chunk}")


# ----------------------------------------------------------------------------------------------------- 3. capacity
def test_capacity(native, fx, knob):
    h, Q, radii = fx["h"], fx["Q"], fx["radii"]
    N = native._native
    want = fixture_expected(8, 256)
    total = int(want.offsets[-1])
    assert total > 0 and int(want.offsets[-7]) < total                    # the last group of 6 holds answers: the overflow falls there
    for chunk in (None, 7):
        knob("HNSWGPU_RANGE_CHUNK", chunk)
        rc, offs, outs, ef, flags = _raw(native, h, Q, radii, 8, 256, total)
        assert rc == N.OK, N.last_error()
        assert np.array_equal(offs, want.offsets) and np.array_equal(outs[0], want.ids) and np.array_equal(outs[3], want.ranks)
        assert np.array_equal(outs[1].view(np.uint32), want.dists.view(np.uint32)) and np.array_equal(outs[2], want.layers)
        assert np.array_equal(ef, want.ef) and np.array_equal(flags, want.flags)
        rc, offs, outs, ef, flags = _raw(native, h, Q, radii, 8, 256, total - 1)
        assert rc == N.ERR_CAPACITY and str(total) in N.last_error()
        assert np.array_equal(offs, want.offsets)                         # complete, whatever the capacity
        assert np.array_equal(ef, want.ef) and np.array_equal(flags, want.flags)
        rc, offs, outs, ef, flags = _raw(native, h, Q, radii, 8, 256, 0, with_out=False)   # count only
        assert rc == N.ERR_CAPACITY and str(total) in N.last_error() and np.array_equal(offs, want.offsets)
        none = np.full(len(Q), -1.0, np.float32)
        rc, offs, outs, ef, flags = _raw(native, h, Q, none, 8, 256, 0, with_out=False)    # ... of a batch without answers: nothing is missing
        assert rc == N.OK and not offs.any() and (ef == 8).all() and not flags.any()
    knob("HNSWGPU_RANGE_CHUNK", None)
    rc, offs, outs, ef, flags = _raw(native, h, Q, radii, 8, 256, total, with_ids=False)   # cap > 0 with NULL out_ids
    assert rc == N.ERR_ARG and "out_ids" in N.last_error() and (offs == 0x5A5A5A5A).all()
    res = h.range_search_flat(Q, radii, 64, 1024)                         # the Python method: a guess, then the exact total
    assert int(fixture_expected(64, 1024).offsets[-1]) > max(1024, 32 * len(Q))
    _same(res, fixture_expected(64, 1024), "retry with the exact total")


# ----------------------------------------------------------------------------------------------------- 4. radii
def test_hostile_radii(native, fx):
    h, o, X = fx["h"], fx["o"], fx["X"]
    Q = np.ascontiguousarray(X[[5, 5, 5, 5, 900, 900]])                   # stored vectors: the nearest entry is at distance 0
    radii = np.array([np.nan, -1.0, -0.0, 0.0, -0.0, np.inf], np.float32)
    want = range_rule(o.parallel_search, Q, radii, 8, 256)
    assert want.counts.tolist() == [0, 0, 1, 1, 1, 256]                   # on the oracle: distance 0 matches +-0; +inf saturates
    assert want.dists[0] == 0 and want.flags.tolist() == [0, 0, 0, 0, 0, 1] and want.ef.tolist() == [8, 8, 8, 8, 8, 256]
    _same(h.range_search_flat(Q, radii, 8, 256), want, "hostile radii")
    allq = fx["Q"][:40]
    inf = np.full(40, np.inf, np.float32)
    want = range_rule(o.parallel_search, allq, inf, 8, 256)
    assert (want.counts == 256).all() and (want.flags == 1).all()         # +inf on 3000 points: saturated at ef_max
    _same(h.range_search_flat(allq, inf, 8, 256), want, "+inf")


def test_inf_radius_on_a_small_index_settles_by_what_the_search_reaches(native, oracle, tmp_path):
    X, Q = uniform(100, 8, 11), uniform(20, 8, 12)
    o = oracle.OracleHnsw(8, 100, 16, 64, "DistL2")
    o.insert_batch(X)
    h = _load(native, o, tmp_path, "DistL2")
    inf = np.full(20, np.inf, np.float32)
    want = range_rule(o.parallel_search, Q, inf, 8, 256)
    assert (want.ef == 128).all() and (want.counts < 128).all() and not want.flags.any()   # rule (b): c < 128, flag 0
    _same(h.range_search_flat(Q, inf, 8, 256), want, "100 points")


# ----------------------------------------------------------------------------------------------------- 5. filter
def test_filter(native, fx):
    h, o, Q, radii = fx["h"], fx["o"], fx["Q"], fx["radii"]
    N = native._native
    allowed = np.sort(np.random.default_rng(3).choice(3000, 300, replace=False).astype(np.uint64))
    wide = np.minimum(radii * np.float32(2.0), np.float32(10.0))          # (a tenth of the points are allowed: wider balls hold some)
    want = range_rule(lambda q, k, ef: o.parallel_search_filter(q, k, ef, allowed), Q, wide, 2, 256)
    assert len(set(want.ef.tolist())) >= 3 and (want.counts > 0).any() and (want.counts == 0).any()
    assert np.isin(want.ids, allowed).all()
    got = h.range_search_flat(Q, wide, 2, 256, allowed)
    _same(got, want, "filter, oracle")
    _same(got, range_rule(lambda q, k, ef: h.parallel_search_filter_flat(q, k, ef, allowed), Q, wide, 2, 256), "filter, device search")
    res = h.range_search_flat(Q, wide, 2, 256, np.zeros(0, np.uint64))    # the filter that allows nothing: empty in round 0
    assert not res.offsets.any() and (res.ef == 2).all() and not res.flags.any() and len(res.ids) == 0
    for bad in (dict(ef_first=1, allowed_ids=allowed), dict(ef_first=2, allowed_ids=allowed[::-1].copy())):
        with pytest.raises(native.HnswError) as e:
            h.range_search_flat(Q, wide, bad["ef_first"], 256, bad["allowed_ids"])
        assert e.value.code == N.ERR_ARG


# ----------------------------------------------------------------------------------------------------- 6. the cut kernel's step boundary
@pytest.mark.parametrize("width", [1, 63, 64, 65])
def test_row_widths_around_the_step(native, fx, width):
    h, o, Q, radii = fx["h"], fx["o"], fx["Q"], fx["radii"]
    want = range_rule(o.parallel_search, Q, radii, width, width)
    assert (want.ef == width).all() and (want.counts == width).any() and (want.counts == 0).any()
    if width > 2:
        assert ((want.counts > 0) & (want.counts < width)).any()
    _same(h.range_search_flat(Q, radii, width, width), want, f"width {width}")


# ----------------------------------------------------------------------------------------------------- 7. ties
def test_tie_groups_on_the_boundary(native, oracle, tmp_path):
    """every vector occurs three times, so every distance does: the radius of a query is the distance it shares with a group of
    three, which lies exactly on the boundary and is kept whole.  Strict against the oracle; strict ties off against the device's
    own search under the same setting."""
    base = uniform(400, 8, 21)
    X = np.ascontiguousarray(np.repeat(base, 3, axis=0)[np.random.default_rng(22).permutation(1200)])
    Q = uniform(60, 8, 23)
    o = oracle.OracleHnsw(8, 1200, 16, 64, "DistL2")
    o.insert_batch(X)
    h = _load(native, o, tmp_path, "DistL2")
    D = np.sort(oracle.dist_matrix("DistL2", Q, X), axis=1)
    radii = np.array([D[i, 3 * (i % 20) + 1] for i in range(60)], np.float32)   # the (i % 20)-th nearest vector's distance, shared by its three copies
    want = range_rule(o.parallel_search, Q, radii, 4, 128)
    a = want.offsets
    whole = [q for q in range(60) if a[q + 1] - a[q] >= 3 and (want.dists[int(a[q + 1]) - 3:int(a[q + 1])] == radii[q]).all()]
    assert len(whole) >= 30 and len(set(want.ef.tolist())) >= 3           # the tie group on the boundary came back whole
    _same(h.range_search_flat(Q, radii, 4, 128), want, "ties, strict")
    h.set_strict_ties(False)
    try:
        _same(h.range_search_flat(Q, radii, 4, 128), range_rule(h.parallel_search_flat, Q, radii, 4, 128), "ties, strict off")
    finally:
        h.set_strict_ties(True)


# ----------------------------------------------------------------------------------------------------- 8. other distances, the other arithmetic
@pytest.mark.parametrize("metric,d,m,gen", [("DistCosine", 25, 24, uniform), ("DistJeffreys", 12, 12, probability)])
def test_other_distances(native, oracle, tmp_path, metric, d, m, gen):
    X, Q = gen(1500, d, 31), gen(96, d, 32)
    o = oracle.OracleHnsw(m, 1500, 16, 64, metric)
    o.insert_batch(X)
    h = _load(native, o, tmp_path, metric)
    radii = radii_from_quantiles(oracle.dist_matrix(metric, Q, X))
    want = range_rule(o.parallel_search, Q, radii, 8, 256)
    assert len(set(want.ef.tolist())) >= 3 and (want.flags & 1).any() and (want.counts == 0).any()
    _same(h.range_search_flat(Q, radii, 8, 256), want, metric)


def test_simd_order_arithmetic(native, oracle, tmp_path):
    """DistL2 at d = 25 (three blocks of 8 and a tail: the two summation orders differ in the last bits), the index set to
    HNSWGPU_ARITH_SIMD8 against the oracle's set_simd_order(True); switching back restores the scalar answers"""
    X, Q = uniform(1500, 25, 41), uniform(96, 25, 42)
    o = oracle.OracleHnsw(12, 1500, 16, 64, "DistL2")
    o.insert_batch(X)
    h = _load(native, o, tmp_path, "DistL2")
    radii = radii_from_quantiles(oracle.dist_matrix("DistL2", Q, X))
    scalar = range_rule(o.parallel_search, Q, radii, 8, 256)
    h.set_arithmetic("simd8")
    o.set_simd_order(True)
    try:
        want = range_rule(o.parallel_search, Q, radii, 8, 256)
        assert len(want.dists) != len(scalar.dists) or (want.dists.view(np.uint32) != scalar.dists.view(np.uint32)).any()   # (the orders differ here)
        _same(h.range_search_flat(Q, radii, 8, 256), want, "simd8")
    finally:
        h.set_arithmetic("scalar")
        o.set_simd_order(False)
    _same(h.range_search_flat(Q, radii, 8, 256), scalar, "back to scalar")


# ----------------------------------------------------------------------------------------------------- 9. the device entry, threads, nothing to do
def test_device_entry_on_a_stream(native, fx, knob):
    """every buffer in HBM (torch), on a stream of the caller's: the host entry's answers; NULL layer / rank / ef / flags; the filter;
    too small a capacity; nq == 0"""
    import torch
    h, Q, radii = fx["h"], fx["Q"], fx["radii"]
    N = native._native
    L = native.lib()
    stream = torch.cuda.Stream()
    allowed = np.sort(np.random.default_rng(3).choice(3000, 300, replace=False).astype(np.uint64))
    dq, dr = torch.from_numpy(Q).cuda(), torch.from_numpy(radii).cuda()
    dal = torch.from_numpy(allowed.astype(np.int64)).cuda()
    nq, d = Q.shape

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def call(ef_first, ef_max, cap, al=None, with_pids=True, with_ef=True, n=nq):
        o_off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
        o_ids = torch.full((cap + 1,), -1, dtype=torch.int64, device="cuda")
        o_d = torch.full((cap + 1,), -1.0, dtype=torch.float32, device="cuda")
        o_l = torch.full((cap + 1,), 9, dtype=torch.uint8, device="cuda")
        o_r = torch.full((cap + 1,), -1, dtype=torch.int32, device="cuda")
        o_ef = torch.full((max(n, 1),), -1, dtype=torch.int32, device="cuda")
        o_fl = torch.full((max(n, 1),), 9, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = L.hnswgpu_range_search_batch_device(h.handle, ptr(dq), n, d, ptr(dr), ef_first, ef_max, ptr(al), 0 if al is None else len(allowed), cap,
                                                 ptr(o_off), ptr(o_ids), ptr(o_d), ptr(o_l) if with_pids else None, ptr(o_r) if with_pids else None,
                                                 ptr(o_ef) if with_ef else None, ptr(o_fl) if with_ef else None, C.c_void_p(stream.cuda_stream))
        return rc, [t.cpu().numpy() for t in (o_off, o_ids, o_d, o_l, o_r, o_ef, o_fl)]

    for chunk in (None, 7):
        knob("HNSWGPU_RANGE_CHUNK", chunk)
        cases = (((8, 256), None, None), ((512, 2048), None, None), ((2, 256), allowed, dal)) if chunk is None else (((8, 256), None, None),)
        for (ef_first, ef_max), al_np, al_dev in cases:
            want = h.range_search_flat(Q, radii, ef_first, ef_max, al_np)  # (the host entry, checked against the oracle above)
            total = int(want.offsets[-1])
            for with_pids, with_ef in ((True, True), (False, False)):
                rc, (off, ids, dd, ll, rr, ef, fl) = call(ef_first, ef_max, total, al_dev, with_pids, with_ef)
                assert rc == N.OK, N.last_error()
                assert np.array_equal(off.astype(np.uint64), want.offsets) and np.array_equal(ids[:total].astype(np.uint64), want.ids)
                assert np.array_equal(dd[:total].view(np.uint32), want.dists.view(np.uint32))
                assert ids[total] == -1 and dd[total] == -1.0              # nothing behind the total
                if with_pids:
                    assert np.array_equal(ll[:total], want.layers) and np.array_equal(rr[:total], want.ranks)
                else:
                    assert (ll == 9).all() and (rr == -1).all()
                if with_ef:
                    assert np.array_equal(ef.astype(np.uint32), want.ef) and np.array_equal(fl, want.flags)
                else:
                    assert (ef == -1).all() and (fl == 9).all()
            rc, (off, ids, dd, ll, rr, ef, fl) = call(ef_first, ef_max, total - 1, al_dev)
            assert rc == N.ERR_CAPACITY and str(total) in N.last_error() and np.array_equal(off.astype(np.uint64), want.offsets)
            assert ids[total - 1] == -1                                     # (unspecified contents, but never a slot behind cap)
    knob("HNSWGPU_RANGE_CHUNK", None)
    rc, (off, ids, dd, ll, rr, ef, fl) = call(8, 256, 4, n=0)
    assert rc == N.OK and off.tolist() == [0] and (ids == -1).all()


def test_two_threads_on_one_handle(native, fx):
    h, Q, radii = fx["h"], fx["Q"], fx["radii"]
    pairs = {"a": (8, 256), "b": (3, 100)}
    out, errs = {}, []

    def run(name):
        try:
            out[name] = [h.range_search_flat(Q, radii, *pairs[name]) for _ in range(4)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=(name,)) for name in pairs]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for name in pairs:
        for got in out[name]:
            _same(got, fixture_expected(*pairs[name]), name)


def test_no_query_and_no_point(native, fx):
    h = fx["h"]
    N = native._native
    res = h.range_search_flat(np.zeros((0, 8), np.float32), 1.0, 8, 256)
    assert res.offsets.tolist() == [0] and len(res.ids) == 0 and len(res.ef) == 0
    offs = np.full(1, 9, np.uint64)
    rc = native.lib().hnswgpu_range_search_batch(h.handle, None, 0, 8, None, 8, 256, None, 0, 0, _p(offs), None, None, None, None, None, None)
    assert rc == N.OK and offs[0] == 0
    e = native.Hnsw(8, 10, 16, 32, "DistL2")                              # an empty index
    res = e.range_search_flat(fx["Q"][:5], 1.0, 8, 256)
    assert res.offsets.tolist() == [0] * 6 and len(res.ids) == 0


def test_recall_against_the_exact_range_search(native, fx):
    """range_recall_flat is the recall by id of the two flat results, and the share of saturated queries"""
    h, Q, radii = fx["h"], fx["Q"], fx["radii"]
    got, exact = h.range_search_flat(Q, radii, 64, 1024), h.exact_range_search_flat(Q, radii)
    found = sum(len(np.intersect1d(got.of(q)[0], exact.of(q)[0])) for q in range(len(Q)))
    recall, saturated = h.range_recall_flat(Q, radii, 64, 1024)
    assert recall == found / int(exact.offsets[-1]) and 0.0 < recall <= 1.0
    assert saturated == np.count_nonzero(fixture_expected(64, 1024).flags & 1) / len(Q)
    for q in np.flatnonzero((got.flags & 1) == 0)[:50]:                   # an unsaturated answer holds no point outside the ball
        assert np.isin(got.of(q)[0], exact.of(q)[0]).all()
