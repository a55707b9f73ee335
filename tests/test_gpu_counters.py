"""The device's per-query work counters (d_stats words 0, 1, 2 and word 7's descent share) against the oracle's, query by query
(include/hnsw_mi355x.h, d_stats): they define the algorithmic bytes of every roofline number bench.py reports, and they catch a
kernel that skips or repeats work where the answers do not show it (a false "already visited", one expansion too many or too few
at the stop rule, src/hnsw.rs:981).  Every case also asserts that the path it is about really ran, and runs lean
(set_strict_ties(False)) as well: there every query the device does not flag (status 2) must be the reference's, counters included.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import normalized, probability, uniform
from test_gpu_parity import _tie_heavy, assert_same

pytestmark = pytest.mark.gpu


class _Res:
    """what _device_search returns: the answers like a BatchResult, and st = the stats words, uint32 (nq, 8)"""

    def __init__(self, ids, dists, layers, ranks, counts, st):
        self.ids, self.dists, self.layers, self.ranks, self.counts, self.st = ids, dists, layers, ranks, counts, st


def _device_search(native, h, Q, k, ef, allowed=None):
    """hnswgpu_search_batch_device (or _filtered_device with the sorted id vector `allowed`) on buffers of the HIP runtime:
    answers and the per-query stats words."""
    lib = native.lib()
    hip = C.CDLL("libamdhip64.so")
    Q = np.ascontiguousarray(Q, dtype=np.float32)
    nq, d = Q.shape
    bufs = []

    def dmalloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 4))) == 0
        bufs.append(p)
        return p

    def put(a):
        p = dmalloc(a.nbytes)
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
        return p

    def fetch(p, shape, dtype):
        a = np.zeros(shape, dtype)
        assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), p, C.c_size_t(a.nbytes), 2) == 0
        return a

    try:
        q = put(Q)
        ids, dd, lay, rk, cnt, st = (dmalloc(nq * k * 8), dmalloc(nq * k * 4), dmalloc(nq * k), dmalloc(nq * k * 4), dmalloc(nq * 4),
                                     dmalloc(nq * 32))
        if allowed is None:
            rc = lib.hnswgpu_search_batch_device(h.handle, q, nq, d, k, ef, ids, dd, lay, rk, cnt, st, None)
        else:
            al = np.ascontiguousarray(allowed, dtype=np.uint64)
            rc = lib.hnswgpu_search_batch_filtered_device(h.handle, q, nq, d, k, ef, put(al), len(al), ids, dd, lay, rk, cnt, st,
                                                          None, None)
        assert rc == 0, native._native.last_error()
        return _Res(fetch(ids, (nq, k), np.uint64), fetch(dd, (nq, k), np.float32), fetch(lay, (nq, k), np.uint8),
                    fetch(rk, (nq, k), np.int32), fetch(cnt, (nq,), np.uint32), fetch(st, (nq, 8), np.uint32))
    finally:
        for p in bufs:
            hip.hipFree(p)


def _device_rows(st):
    st = st.astype(np.int64)
    return np.stack([st[:, 0], st[:, 1], st[:, 2], st[:, 7] >> 16, (st[:, 7] >> 8) & 0xFF], 1)


def assert_same_counters(st, ref, what=""):
    """words 0, 1, 2 and word 7's descent fields (n_dist << 16, lists << 8) == the oracle's per-query counters"""
    got, want = _device_rows(st), ref.per_query.astype(np.int64)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (f"{what}: counters of {bad.size} of {len(st)} queries differ from the oracle's, first {bad[:4].tolist()}: "
                           f"device {got[bad[:4]].tolist()} oracle {want[bad[:4]].tolist()} "
                           f"(n_dist, n_expand, n_ids_read, descent n_dist, descent lists), status {st[bad[:4], 3].tolist()}")


def _differs(res, ref):
    """per query: answers (count, ids, distance bits, p_ids) or counters other than the oracle's"""
    nq, k = res.ids.shape
    j = np.arange(k)[None, :]
    live = j < ref.counts.astype(np.int64)[:, None]
    ans = ((res.ids != ref.ids.astype(np.uint64)) | (res.dists.view(np.uint32) != ref.dists.view(np.uint32))
           | (res.layers != ref.layers) | (res.ranks != ref.ranks)) & live
    return (res.counts != ref.counts) | ans.any(1) | (_device_rows(res.st) != ref.per_query.astype(np.int64)).any(1)


def assert_lean_sound(res, ref, tie_heavy=False, what=""):
    """lean mode's contract (include/hnsw_mi355x.h, ties): (i) a query with status 0 and no equal distances met is the reference's
    answer, counters included; (ii) every query that differs from the oracle in anything carries status 2; (iii) on tie-heavy data
    such queries exist"""
    status, ties_met = res.st[:, 3], (res.st[:, 7] & 1) != 0
    diff = _differs(res, ref)
    clean = (status == 0) & ~ties_met
    assert not (diff & clean).any(), f"{what}: {int((diff & clean).sum())} unflagged tie-free queries differ, first {np.nonzero(diff & clean)[0][:4]}"
    bad = np.nonzero(diff & (status != 2))[0]
    assert bad.size == 0, f"{what}: {bad.size} queries differ from the oracle without status 2, first {bad[:4].tolist()} (status {status[bad[:4]].tolist()})"
    assert set(np.unique(status).tolist()) <= {0, 2, 3}, f"{what}: lean statuses {np.unique(status).tolist()}"   # (3: literal kernel)
    if tie_heavy:
        assert (status == 2).any(), f"{what}: no query flagged on tie-heavy data"


def check(native, h, o, Q, k, ef, what="", lean=True, tie_heavy=False, res=None):
    """strict (and lean) device call == the oracle in answers and per-query counters; returns the strict result"""
    ref = o.parallel_search(Q, k, ef, want_counters="per_query")
    if res is None:
        res = _device_search(native, h, Q, k, ef)
    assert_same(res, ref)
    assert_same_counters(res.st, ref, what)
    if lean:
        h.set_strict_ties(False)
        try:
            lres = _device_search(native, h, Q, k, ef)
        finally:
            h.set_strict_ties(True)
        assert_lean_sound(lres, ref, tie_heavy, what + " (lean)")
    return res, ref


def _pair(native, oracle, tmp_path, X, m, efc, dist, tag):
    o = oracle.OracleHnsw(m, len(X), 16, efc, dist)
    o.insert_batch(X)
    o.file_dump(tmp_path, tag)
    h = native.HnswIo(tmp_path, tag).load_hnsw(dist)
    h.upload(0)
    return o, h


def _launch_lines(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[hnswgpu launch]")]


# ------------------------------------------------------------------------------------------------------------------ metrics
METRICS = [  # dist, d, data, M
    ("DistL2", 16, "uniform", 12),
    ("DistCosine", 25, "uniform", 16),      # the norm rides in the row's padding
    ("DistCosine", 32, "uniform", 12),      # no room in the row: the separate norm array
    ("DistDot", 30, "normalized", 16),
    ("DistL1", 10, "uniform", 12),
    ("DistHellinger", 12, "probability", 12),
    ("DistJeffreys", 12, "probability", 12),
    ("DistJensenShannon", 12, "probability", 12),
]
_GEN = {"uniform": uniform, "normalized": normalized, "probability": probability}


@pytest.mark.parametrize("dist,d,data,m", METRICS)
def test_counters_match_the_oracle_per_metric(native, oracle, tmp_path, knob, capfd, dist, d, data, m):
    X = _GEN[data](2500, d, 40 + d)
    o, h = _pair(native, oracle, tmp_path, X, m, 60, dist, "m")
    Q = _GEN[data](300, d, 41 + d)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res, _ = check(native, h, o, Q, 10, 48, dist)
    knob("HNSWGPU_TRACE_LAUNCH", None)
    assert any("strict 1" in ln and "slots 1" in ln for ln in _launch_lines(capfd))   # the strict one-query kernel, S = 1
    assert np.all(res.st[:, 3] != 1)


@pytest.mark.parametrize("dist,normalize", [("DistL2", False), ("DistCosine", False), ("DistDot", True), ("DistL1", False)])
def test_counters_in_simd8_arithmetic(native, oracle, tmp_path, dist, normalize):
    """set_arithmetic("simd8") against the oracle in the same summation order (set_simd_order): other distances, another walk --
    the same work as the reference in that order"""
    gen = normalized if normalize else uniform
    d = 37
    o, h = _pair(native, oracle, tmp_path, gen(2500, d, 61), 12, 60, dist, "s8")
    Q = gen(300, d, 62)
    h.set_arithmetic("simd8")
    o.set_simd_order(True)
    try:
        res, ref = check(native, h, o, Q, 10, 64, dist + " simd8")
        o.set_simd_order(False)
        scalar = o.parallel_search(Q, 10, 64, want_counters="per_query")
        # the path ran: the scalar order gives other distance bits somewhere
        assert not np.array_equal(scalar.dists.view(np.uint32), res.dists.view(np.uint32))
    finally:
        h.set_arithmetic("scalar")
        o.set_simd_order(False)


# ------------------------------------------------------------------------------------------------------- result-set shapes
@pytest.fixture(scope="module")
def shapes_pair(native, oracle, tmp_path_factory):
    X = uniform(3000, 8, 71)
    return _pair(native, oracle, tmp_path_factory.mktemp("shapes"), X, 12, 60, "DistL2", "sh")


RESULT_SET_SHAPES = [(10, 10, 1), (10, 64, 1), (10, 65, 2), (10, 128, 2), (10, 129, 4), (10, 256, 4),   # k, ef, slots per lane
                     (10, 257, 16), (100, 1000, 16), (40, 20, 1)]                                        # (40, 20): k > ef, ef = max(ef, k)


@pytest.mark.parametrize("k,ef,slots", RESULT_SET_SHAPES)
def test_counters_at_every_result_set_shape(native, shapes_pair, knob, capfd, k, ef, slots):
    o, h = shapes_pair
    Q = uniform(200, 8, 72)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, k, ef)
    knob("HNSWGPU_TRACE_LAUNCH", None)
    lines = _launch_lines(capfd)
    assert any(f"slots {slots}," in ln for ln in lines), lines
    check(native, h, o, Q, k, ef, f"k {k} ef {ef}", res=res)


def test_counters_of_the_literal_kernel_above_ef_1024(native, shapes_pair, knob, capfd):
    """ef = 1100: no register-resident result set; the literal-heap kernel answers every query"""
    o, h = shapes_pair
    Q = uniform(40, 8, 73)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, 10, 1100)
    knob("HNSWGPU_TRACE_LAUNCH", None)
    lines = _launch_lines(capfd)
    assert lines and all("literal kernel" in ln for ln in lines), lines
    assert np.all(res.st[:, 3] == 3)
    check(native, h, o, Q, 10, 1100, "ef 1100", res=res)


# ------------------------------------------------------------------------------------------------------------- visited set
def test_counters_with_16_bit_cells_and_migration_to_the_hbm_bitmap(native, oracle, tmp_path, knob, capfd):
    X = uniform(20000, 16, 81)
    o, h = _pair(native, oracle, tmp_path, X, 16, 60, "DistL2", "vis")
    Q = uniform(600, 16, 82)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, 10, 128)
    assert any("visited set cell16" in ln for ln in _launch_lines(capfd))
    assert not res.st[:, 6].any()          # default sizing: nobody left the LDS table
    check(native, h, o, Q, 10, 128, "cell16", res=res)
    knob("HNSWGPU_HASH_BITS", "8")         # 256 cells: most queries move to their HBM bitmap slice inside the launch
    capfd.readouterr()
    res = _device_search(native, h, Q, 10, 128)
    assert any("table 2^8 cells" in ln and "visited set cell16" in ln for ln in _launch_lines(capfd))
    assert res.st[:, 6].sum() > len(Q) // 4
    check(native, h, o, Q, 10, 128, "cell16 -> HBM bitmap", res=res)
    knob("HNSWGPU_HASH_BITS", None)
    knob("HNSWGPU_TRACE_LAUNCH", None)


# --------------------------------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("kind,dist,ef", [("grid", "DistL2", 32), ("duplicates", "DistL2", 64), ("grid", "DistL1", 100)])
def test_counters_under_ties(native, oracle, tmp_path, knob, capfd, kind, dist, ef):
    """equal distances: the in-kernel replay from the heap-operation log (status 3), the flagged queries rerun by run_exact
    (HNSWGPU_NO_INKERNEL), the replay taken from the first tie on (HNSWGPU_EXACT_FIRST=1), lean flags (status 2)"""
    n, d = 1200, 6
    o, h = _pair(native, oracle, tmp_path, _tie_heavy(kind, n, d, 77), 8, 40, dist, "ties")
    Q = _tie_heavy(kind, 200, d, 78)
    res, _ = check(native, h, o, Q, 10, ef, f"{kind} {dist}", tie_heavy=True)
    assert (res.st[:, 3] == 3).sum() > 10                       # replays ran
    knob("HNSWGPU_NO_INKERNEL", "1")
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, 10, ef)
    lines = _launch_lines(capfd)
    assert any("strict 0" in ln for ln in lines) and any("literal kernel" in ln for ln in lines), lines
    assert (res.st[:, 3] == 3).sum() > 10
    check(native, h, o, Q, 10, ef, "run_exact", lean=False, res=res)
    knob("HNSWGPU_NO_INKERNEL", None)
    knob("HNSWGPU_TRACE_LAUNCH", None)
    knob("HNSWGPU_EXACT_FIRST", "1")
    res = _device_search(native, h, Q, 10, ef)
    assert (res.st[:, 3] == 3).sum() > 10
    check(native, h, o, Q, 10, ef, "exact first", lean=False, res=res)
    knob("HNSWGPU_EXACT_FIRST", None)


# ----------------------------------------------------------------------------------------------------------------- pair pass
@pytest.mark.parametrize("n,d,m,dist,normalize,k,ef,nq", [
    (6000, 32, 12, "DistCosine", False, 10, 100, 600),
    (6000, 10, 8, "DistL1", False, 5, 20, 513),
    (5000, 40, 32, "DistL2", False, 10, 10, 640),
    (5000, 16, 4, "DistL2", False, 1, 1, 600),
])
def test_counters_of_the_pair_pass(native, oracle, tmp_path, knob, capfd, n, d, m, dist, normalize, k, ef, nq):
    gen = normalized if normalize else uniform
    o, h = _pair(native, oracle, tmp_path, gen(n, d, n + d + m), m, 100, dist, "pp")
    Q = gen(nq, d, 11)
    knob("HNSWGPU_PAIR_SEARCH", "1")
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, k, ef)
    assert any("pair pass" in ln for ln in _launch_lines(capfd))
    knob("HNSWGPU_TRACE_LAUNCH", None)
    assert np.mean(res.st[:, 3] == 0) > 0.5                 # most queries answered by the pass itself
    check(native, h, o, Q, k, ef, "pair pass", res=res)
    knob("HNSWGPU_PAIR_SEARCH", None)


# ------------------------------------------------------------------------------------------------------------------- descent
@pytest.mark.parametrize("n,d,m,k,ef,slots", [
    (3000, 24, 8, 10, 48, 1),       # short upper lists: the two-queries-per-wavefront descent
    (2500, 16, 40, 10, 50, 16),     # 2M = 80 ids per row: S = 16 forced, upper lists of 40
    (2500, 16, 100, 10, 30, 16),    # 2M = 200
    (40, 8, 6, 10, 64, 1),          # fewer points than ef
])
def test_counters_of_both_descent_kernels(native, oracle, tmp_path, knob, capfd, n, d, m, k, ef, slots):
    o, h = _pair(native, oracle, tmp_path, uniform(n, d, n + m), m, 100, "DistL2", "dsc")
    assert o.get_max_level_observed() >= 1
    Q = uniform(300, d, 5)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, k, ef)
    assert any(f"slots {slots}," in ln for ln in _launch_lines(capfd))
    knob("HNSWGPU_TRACE_LAUNCH", None)
    assert ((res.st[:, 7] >> 8) & 0xFF).min() >= 1            # the descent read at least one upper list
    check(native, h, o, Q, k, ef, "pair descent", res=res)
    knob("HNSWGPU_NO_PAIR_DESCENT", "1")
    check(native, h, o, Q, k, ef, "single descent")
    knob("HNSWGPU_NO_PAIR_DESCENT", None)


def test_counters_on_a_single_point_index(native, oracle, tmp_path):
    for seed in (400, 401, 402):
        o, h = _pair(native, oracle, tmp_path, uniform(1, 5, seed), 8, 20, "DistL2", f"one{seed}")
        L = o.get_max_level_observed()
        Q = uniform(6, 5, 410)
        res, ref = check(native, h, o, Q, 3, 10, f"single point at level {L}")
        assert ref.per_query.tolist() == [[2, L + 1, 0, 1, L]] * 6


# ------------------------------------------------------------------------------------------------------------------ filtered
@pytest.fixture(scope="module")
def filter_pair(native, oracle, tmp_path_factory):
    X = uniform(6000, 12, 91)
    X[3000:3300] = X[:300]
    return _pair(native, oracle, tmp_path_factory.mktemp("flt"), X, 12, 60, "DistL2", "flt")


@pytest.mark.parametrize("pct", [1, 30, 100])
def test_filtered_counters(native, filter_pair, pct):
    """hnsw_search_exact_kernel with a filter (its loop never stops early): counters of every query, those on which the
    reference panics (status 6 here, 1 in the oracle) included -- the work up to the panic.  Strict and lean calls share that
    kernel, so there is no lean variant."""
    o, h = filter_pair
    n = 6000
    allowed = np.sort(np.random.default_rng(pct).choice(n, n * pct // 100, replace=False)).astype(np.uint64)
    Q = np.concatenate([uniform(200, 12, 92), uniform(6000, 12, 91)[:50]])
    for k, ef in ((10, 20), (1, 1)):
        ref = o.parallel_search_filter(Q, k, ef, allowed, want_counters="per_query")
        res = _device_search(native, h, Q, k, ef, allowed)
        assert np.array_equal(res.st[:, 3] == 6, ref.status == 1)
        assert np.all((res.st[:, 3] == 3) | (res.st[:, 3] == 6))   # the exact kernel answered every query
        assert_same(res, ref)
        assert_same_counters(res.st, ref, f"filtered {pct} %, k {k} ef {ef}")
