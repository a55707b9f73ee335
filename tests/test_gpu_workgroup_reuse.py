"""A workgroup's SECOND query, on every path of the search kernels.  Every search kernel is a persistent grid: a workgroup (one
wavefront) answers a query, takes the next work item from the counter and starts again on the same LDS tile, visited table or bitmap
slice, log and heap scratch and registers.  The grid is min(resident workgroups, queries), and a test batch is smaller than the 4 096
to 5 120 resident workgroups of an MI355X, so without help every workgroup of a test answers one query and leaves.  HNSWGPU_MAX_WG
(test hook) caps the workgroups of every persistent launch of a search call; here every path runs on ONE workgroup (the whole work
list serially, in a fixed order) and on THREE (a race for the counter; 3 divides none of the query counts).

The bar is the suite's: ids, f32 distance bits, p_ids, counts, status and the per-query work counters identical to the oracle -- the
counters are where state that leaks from one query into the next shows first.  Every case asserts
  * from the HNSWGPU_TRACE_LAUNCH lines, that every launch of its calls ran on at most the cap's workgroups and had more work items
    than workgroups (_assert_capped), and
  * with G the cap, that at least 8 G of its queries take the rare path the case is about and at least 8 G do not (_assert_split):
    on G workgroups some rare-path query is then followed by another query on its workgroup, and the other way round.  Where the path
    is the whole case (a result-set shape, a metric, the literal kernel) there are 16 G queries at least.  The tie case says where
    its data or its hook leaves no query off the path, and asserts exactly that there.
Data, indexes and helpers are the surrounding suite's.
"""
import re
import sys
import threading

import numpy as np
import pytest

from conftest import uniform
from test_gpu_counters import (METRICS, RESULT_SET_SHAPES, _GEN, _device_search, _pair, assert_lean_sound, assert_same_counters, check, filter_pair,  # noqa: F401
                               shapes_pair)
from test_gpu_filter_set import D_MIXED, _assert_equal, _oracle_answers, _torch_call, mixed  # noqa: F401
from test_gpu_parity import assert_same, build_pair
from test_gpu_relaunch import _forced_call, _n, _passes, _split_bits, _spread, literal_pair, shapes  # noqa: F401
from test_gpu_replay_lds import tie_index  # noqa: F401
from test_gpu_round2 import _assert_filtered

pytestmark = pytest.mark.gpu

CAPS = [1, 3]
_WG = re.compile(r"(\d+) workgroups(?! per CU)")


class _Trace:
    """capfd for the helpers that read it (they keep the "[hnswgpu launch]" lines of what they read), and a record of every line read
    through it: take() = the library's trace lines since the last take()"""

    def __init__(self, capfd):
        self.capfd, self.err = capfd, []

    def readouterr(self):
        r = self.capfd.readouterr()
        self.err.extend(r.err.splitlines())
        sys.stdout.write(r.out)     # (what the test printed stays in its report)
        return r

    def take(self):
        self.readouterr()
        lines, self.err = [ln for ln in self.err if ln.startswith("[hnswgpu ")], []
        return lines


@pytest.fixture
def trace(capfd):
    return _Trace(capfd)


def _cap(knob, trace, g):
    knob("HNSWGPU_MAX_WG", g)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    trace.take()


def _assert_capped(lines, g, what, kinds=("descent", "launch"), beside_the_case=None):
    """every launch of the trace: its line names its workgroups, at most g, fewer than its work items (a query; a pair of queries in
    the pair pass and in the two-per-wavefront descent).  beside_the_case: what marks the lines of a launch that is capped like
    every other but may have as few queries as it likes.  Returns [(line, queries, workgroups)]."""
    out = []
    for ln in lines:
        if "filter set:" in ln:     # (names a group of a filter set, not a launch)
            continue
        m = _WG.search(ln)
        assert m, f"{what}: a launch without its workgroup count: {ln}"
        wg, n = int(m.group(1)), _n(ln)
        per = 2 if ("pair pass" in ln or "two per wavefront 1" in ln) else 1
        assert 1 <= wg <= g, f"{what}: {wg} workgroups under a cap of {g}: {ln}"
        if beside_the_case is None or beside_the_case not in ln:
            assert (n + per - 1) // per > wg, f"{what}: {n} queries on {wg} workgroups reuse none: {ln}"
        out.append((ln, n, wg))
    for kind in kinds:
        assert any(ln.startswith(f"[hnswgpu {kind}]") for ln, _, _ in out), (what, kind, lines)
    return out


def _assert_split(rare, g, what):
    rare = np.asarray(rare, bool)
    n_rare, n_rest = int(rare.sum()), int((~rare).sum())
    print(f"{what}: cap {g}: {n_rare} queries on the rare path, {n_rest} not")
    assert n_rare >= 8 * g and n_rest >= 8 * g, f"{what}: {n_rare} queries on the rare path, {n_rest} not; {8 * g} of each are needed"


def _run(native, knob, trace, g, h, o, Q, k, ef, what, lean=True, tie_heavy=False):
    """strict (and lean) call under the cap == the oracle in answers and per-query counters; every launch capped"""
    _cap(knob, trace, g)
    res, ref = check(native, h, o, Q, k, ef, f"{what}, cap {g}", lean=lean, tie_heavy=tie_heavy)
    lines = trace.take()
    _assert_capped(lines, g, what)
    return res, ref, lines


# ------------------------------------------------------------------------------------------------------ a. result-set shapes
@pytest.mark.parametrize("g", CAPS)
@pytest.mark.parametrize("k,ef,slots", RESULT_SET_SHAPES)
def test_every_result_set_shape_query_after_query(native, shapes_pair, knob, trace, k, ef, slots, g):
    """strict and lean kernels at 1, 2, 4 and 16 result slots per lane (rows of more than 64 ids: the descent case below, M = 40);
    no rare path inside the case: 200 queries >= 16 g"""
    o, h = shapes_pair
    Q = uniform(200, 8, 72)
    assert len(Q) >= 16 * g
    _, _, lines = _run(native, knob, trace, g, h, o, Q, k, ef, f"k {k} ef {ef}")
    one = [ln for ln in lines if "visited set" in ln]
    assert len(one) == 2 and all(f"slots {slots}," in ln for ln in one), lines
    assert "strict 1" in one[0] and "strict 0" in one[1], lines


# ------------------------------------------------------------------------------------- b. visited-set migration inside a launch
@pytest.mark.parametrize("g", CAPS)
def test_back_to_the_lds_table_after_a_query_that_ended_on_the_bitmap(native, shapes, knob, trace, g):
    """16-bit cells, a table that some queries outgrow: they end on the workgroup's HBM bitmap slice (stats word 6), the next query
    of the workgroup starts on the LDS table again"""
    _, o, h, Q = shapes
    ref = o.parallel_search(Q, 10, 128, want_counters="per_query")
    b, moved, stayed = _split_bits(ref, 8 * max(CAPS))
    knob("HNSWGPU_HASH_BITS", b)
    res, _, lines = _run(native, knob, trace, g, h, o, Q, 10, 128, f"cell16, 2^{b} cells")
    one = [ln for ln in lines if "visited set" in ln]
    assert len(one) == 2 and all(f"table 2^{b} cells" in ln and "visited set cell16" in ln for ln in one), lines
    on_bitmap = res.st[:, 6] != 0
    assert on_bitmap[moved].all() and not on_bitmap[stayed].any(), (int(on_bitmap[moved].sum()), int(moved.sum()), int(on_bitmap[stayed].sum()))
    _assert_split(on_bitmap, g, "migration")


def test_back_to_the_32_bit_table_after_a_query_that_ended_on_the_bitmap(native, oracle, tmp_path, knob, trace):
    """the 32-bit-cell kernel: cells are 32-bit while the id bits left of the bucket do not fit a 16-bit cell, idbits - (b - 3) > 13.
    At the 66 000 points of test_gpu_relaunch (17 id bits) that is a table of 2^6 cells, which the first batch of 64 ids outgrows:
    every query moves to the bitmap and none stays.  With more than 2^18 points (19 id bits) a table of 2^8 cells is 32-bit: 192
    visited points fill it, and at ef 32 some queries stay below and some do not (the oracle's counters: asserted on the CPU)."""
    o, h = _pair(native, oracle, tmp_path, _spread(263000, 8, 51), 6, 16, "DistL2", "c32")
    Q = _spread(600, 8, 52)
    ref = o.parallel_search(Q, 10, 32, want_counters="per_query")
    b, moved, stayed = _split_bits(ref, 8 * max(CAPS), 8, 8)
    knob("HNSWGPU_HASH_BITS", b)
    for g in CAPS:
        res, _, lines = _run(native, knob, trace, g, h, o, Q, 10, 32, "cell32")
        one = [ln for ln in lines if "visited set" in ln]
        assert len(one) == 2 and all("table 2^8 cells" in ln and "visited set cell32" in ln for ln in one), lines
        on_bitmap = res.st[:, 6] != 0
        assert on_bitmap[moved].all() and not on_bitmap[stayed].any(), (int(on_bitmap[moved].sum()), int(moved.sum()), int(on_bitmap[stayed].sum()))
        _assert_split(on_bitmap, g, "migration from 32-bit cells")


# ---------------------------------------------------------------------------------------------------------- c. three launches
def test_three_launches_on_three_workgroups(native, shapes, knob, trace):
    """one slice: workgroup 0 owns it, workgroups 1 and 2 hand every query that outgrows its table back -- and take the next one;
    tables 2^b, 2^(b + 2), then the global-bitmap kernel on min(3, 1 slice) = 1 workgroup.  The split is the second launch's: the
    queries it hands on to the third, and those it answers.  (One of the 600 queries meets equal distances in the bitmap launch, whose
    kernels only flag: the literal kernel searches that one query again, behind the case and on one workgroup -- the one launch here
    that cannot have more queries than workgroups.)"""
    g = 3
    _, o, h, Q = shapes
    _cap(knob, trace, g)
    res, _, b = _forced_call(native, knob, trace, h, o, Q, 10, 128, "three launches, cap 3")
    launches = _assert_capped(trace.take(), g, "three launches", beside_the_case="literal kernel")
    bitmap = [wg for ln, _, wg in launches if "visited set bitmap" in ln]
    assert bitmap == [1, 1], launches                        # strict, lean
    assert all(wg == g for ln, _, wg in launches if "visited set" in ln and "visited set bitmap" not in ln), launches
    n1, n2, n3 = res.n
    print(f"three launches under cap 3: {n1} > {n2} > {n3} queries")
    _assert_split(np.arange(n2) < n3, g, "second launch: handed back")


# -------------------------------------------------------------------------------------------------------------------- d. ties
@pytest.mark.parametrize("g", CAPS)
@pytest.mark.parametrize("ef", [10, 100])
@pytest.mark.parametrize("dist", ["DistL2", "DistDot"])
def test_a_query_after_one_that_replayed_its_log(native, tie_index, knob, trace, dist, ef, g):
    """status 3 (the log replayed on the literal heaps) and the others on one workgroup: by default; the replay taken from the first
    tie on with 512 and with 64 heap entries in LDS (LDS-only and general heap operations within one replay); the tie rerun through
    the literal kernel with a work list (HNSWGPU_NO_INKERNEL); lean (status 2).
    Where the split exists it is asserted: ef 10, by default, without the in-kernel replay and lean.  Where it cannot exist, that
    every query is on the path is asserted instead (a replay after a replay, 255 times on one workgroup):
    * HNSWGPU_EXACT_FIRST takes every pop of every query from the literal heap, whatever the query meets: status 3 by construction;
    * at ef 100 a search visits hundreds of points of an index in which three points in ten have copies: every one of the 256 queries
      meets equal distances, and more queries of any kind would too -- no batch on this index has a query off the path."""
    o, h, Q = tie_index(dist)
    what = f"{dist} ef {ef}"

    def on_the_path(status, value, which):
        rare = status == value
        if ef == 10:
            _assert_split(rare, g, f"{what} {which}: status {value}")
        else:
            assert rare.all(), f"{what} {which}: {int((~rare).sum())} queries without status {value}: assert the split here"

    res, ref, _ = _run(native, knob, trace, g, h, o, Q, 10, ef, what + " default", lean=False)
    on_the_path(res.st[:, 3], 3, "default")
    knob("HNSWGPU_EXACT_FIRST", "1")
    for cand_lds in (512, 64):
        knob("HNSWGPU_CAND_LDS", cand_lds)
        res, _, _ = _run(native, knob, trace, g, h, o, Q, 10, ef, f"{what} exact first, cand_lds {cand_lds}", lean=False)
        assert np.all(res.st[:, 3] == 3)
    knob("HNSWGPU_CAND_LDS", None)
    knob("HNSWGPU_EXACT_FIRST", None)
    knob("HNSWGPU_NO_INKERNEL", "1")
    res, _, lines = _run(native, knob, trace, g, h, o, Q, 10, ef, what + " no in-kernel", lean=False)
    rerun = [_n(ln) for ln in lines if "literal kernel, pass 0" in ln]
    assert rerun == [int((res.st[:, 3] == 3).sum())] and any("strict 0" in ln for ln in lines), lines
    on_the_path(res.st[:, 3], 3, "no in-kernel")
    knob("HNSWGPU_NO_INKERNEL", None)
    _cap(knob, trace, g)
    h.set_strict_ties(False)
    try:
        lres = _device_search(native, h, Q, 10, ef)
    finally:
        h.set_strict_ties(True)
    _assert_capped(trace.take(), g, what + " lean")
    assert_lean_sound(lres, ref, True, what + " (lean)")
    on_the_path(lres.st[:, 3], 2, "lean")


# ---------------------------------------------------------------------------------------------------------- e. literal kernel
@pytest.mark.parametrize("g", CAPS)
def test_literal_kernel_above_ef_1024_query_after_query(native, shapes_pair, knob, trace, g):
    o, h = shapes_pair
    Q = uniform(50, 8, 73)
    assert len(Q) >= 16 * g
    res, _, lines = _run(native, knob, trace, g, h, o, Q, 10, 1100, "ef 1100")
    assert all("literal kernel" in ln for ln in lines if ln.startswith("[hnswgpu launch]")), lines
    assert np.all(res.st[:, 3] == 3)


@pytest.mark.parametrize("g", CAPS)
@pytest.mark.parametrize("pct", [1, 30])
def test_literal_kernel_under_one_filter_query_after_query(native, filter_pair, knob, trace, pct, g):
    """host and device entry.  The oracle reports no panic on this or any construction the suite knows, so a query with status 6 (the
    reference panics, count 0) followed by another query on its workgroup is exercised by NO test, here or elsewhere; what is asserted
    is agreement with the oracle, panics included should it ever report one.  At k = ef = 1 the split is between the queries that
    find no allowed point (count 0) and those that find one"""
    o, h = filter_pair
    allowed = np.sort(np.random.default_rng(pct).choice(6000, 6000 * pct // 100, replace=False)).astype(np.uint64)
    Q = np.concatenate([uniform(200, 12, 92), uniform(6000, 12, 91)[:50]])
    assert len(Q) >= 16 * g
    _cap(knob, trace, g)
    for k, ef in ((10, 20), (1, 1)):
        what = f"filtered {pct} %, k {k} ef {ef}"
        ref = o.parallel_search_filter(Q, k, ef, allowed, want_counters="per_query")
        _assert_filtered(h, o, Q, k, ef, allowed)
        res = _device_search(native, h, Q, k, ef, allowed)
        assert np.array_equal(res.st[:, 3] == 6, ref.status == 1) and np.all((res.st[:, 3] == 3) | (res.st[:, 3] == 6))
        assert np.all(res.counts[res.st[:, 3] == 6] == 0)
        assert_same(res, ref)
        assert_same_counters(res.st, ref, what)
        lines = trace.take()
        _assert_capped(lines, g, what)
        assert sum("literal kernel, pass 0" in ln for ln in lines) == 2, lines
        if ef == 1:
            _assert_split(ref.counts == 0, g, what + ": nothing found")
        if ref.status.any():
            last = np.flatnonzero(ref.status == 1)[-1]
            assert (ref.status[last:] == 0).any()


@pytest.mark.parametrize("g", CAPS)
def test_literal_kernel_under_another_filter_than_the_query_before(native, mixed, knob, trace, g):
    """151 queries naming five filters interleaved (1 4 2 0 3 1 ...): on one workgroup every query runs under another slot than the one
    before it, a query under the empty filter (nothing allowed, count 0) is followed by one under a filter that allows points.  Host
    entry, host entry with the set served in groups (work lists and slot lists), device entry with the counters of every query.
    (No query of the set panics by the oracle: a status 6 followed by a query under another filter is not exercised.)"""
    import torch
    o, h = mixed["DistL2"]
    filters = mixed["filters"]
    Q = uniform(151, D_MIXED, 304)
    filter_of = ((np.arange(len(Q)) * 3 + 1) % 5).astype(np.uint32)
    assert np.all(filter_of[1:] != filter_of[:-1])
    ref = _oracle_answers(o, Q, 10, 100, filters, filter_of)
    _assert_split(filter_of == 4, g, "filter set: under the empty filter")
    if ref.status.any():    # every panicking query has a successor under another filter
        assert np.flatnonzero(ref.status == 1)[-1] < len(Q) - 1
    _cap(knob, trace, g)
    _assert_equal(h.parallel_search_filters_flat(Q, 10, 100, filters, filter_of), ref, "host entry")
    lines = trace.take()
    _assert_capped(lines, g, "filter set, host entry")
    assert [_n(ln) for ln in lines if "literal kernel, pass 0" in ln] == [len(Q)], lines
    knob("HNSWGPU_FILTER_SET_MB", "0.0006")      # two bitmaps of this index: three groups
    _assert_equal(h.parallel_search_filters_flat(Q, 10, 100, filters, filter_of), ref, "host entry, groups")
    lines = trace.take()
    _assert_capped(lines, g, "filter set, groups")
    assert sorted(_n(ln) for ln in lines if "literal kernel, pass 0" in ln) == sorted(int((filter_of // 2 == i).sum()) for i in range(3)), lines
    knob("HNSWGPU_FILTER_SET_MB", None)
    rc, got, panics = _torch_call(native, h, Q, 10, 100, filters, filter_of, torch.cuda.Stream(torch.device("cuda", 0)))
    assert rc == 0, native._native.last_error()
    _assert_capped(trace.take(), g, "filter set, device entry")
    _assert_equal(got, ref, "device entry")
    assert panics == int(ref.status.sum())
    for f, allowed in enumerate(filters):
        mine = np.flatnonzero(filter_of == f)
        one = o.parallel_search_filter(Q[mine], 10, 100, allowed, want_counters="per_query")
        assert np.array_equal(got.stats[mine, 3], np.where(one.status == 1, 6, 3)), (f, got.stats[mine, 3].tolist())
        assert_same_counters(got.stats[mine], one, f"filter set, filter {f}")


@pytest.mark.parametrize("g", CAPS)
def test_second_pass_of_the_literal_kernel_query_after_query(native, literal_pair, knob, trace, g):
    """HNSWGPU_LITERAL_CAND_CAP=64: pass 0 lists the queries whose candidate heap outgrows 64 entries and goes on with the next;
    pass 1 answers that list on the same few workgroups"""
    o, h = literal_pair
    allowed = np.sort(np.random.default_rng(30).choice(6000, 1800, replace=False)).astype(np.uint64)
    Q = np.concatenate([_spread(200, 12, 93), _spread(6000, 12, 91)[:50]])
    knob("HNSWGPU_LITERAL_CAND_CAP", 64)
    _cap(knob, trace, g)
    ref = o.parallel_search_filter(Q, 10, 20, allowed, want_counters="per_query")
    res = _device_search(native, h, Q, 10, 20, allowed)
    lines = trace.take()
    _assert_capped(lines, g, "two passes")
    (p0, p1), = _passes([ln for ln in lines if ln.startswith("[hnswgpu launch]")])
    assert p0 == len(Q)
    _assert_split(np.arange(p0) < p1, g, "literal kernel: to the second pass")
    assert np.array_equal(res.st[:, 3] == 6, ref.status == 1) and np.all((res.st[:, 3] == 3) | (res.st[:, 3] == 6))
    assert_same(res, ref)
    assert_same_counters(res.st, ref, "filtered, two passes")


# ------------------------------------------------------------------------------------------------------------- f. pair pass
def _pair_call(native, knob, trace, g, h, o, Q, k, ef, what):
    knob("HNSWGPU_PAIR_SEARCH", "1")
    _cap(knob, trace, g)
    res = _device_search(native, h, Q, k, ef)
    lines = trace.take()
    _assert_capped(lines, g, what)
    launch = [ln for ln in lines if ln.startswith("[hnswgpu launch]")]
    assert "pair pass" in launch[0] and _n(launch[0]) == len(Q), lines
    check(native, h, o, Q, k, ef, what, res=res)
    _assert_capped(trace.take(), g, what + " (lean)")
    return res, launch


@pytest.mark.parametrize("g", CAPS)
def test_pairs_after_pairs_that_handed_queries_back(native, oracle, tmp_path, knob, trace, g):
    """601 queries: 300 full pairs and a half-filled last one.  Integer grid data (equal distances everywhere): a strict pair pass
    hands a query that meets a tie back and its half takes the next pair's; every second query is off the grid and meets none"""
    rng = np.random.default_rng(3)
    n, d = 6000, 8
    o, h = _pair(native, oracle, tmp_path, rng.integers(0, 4, size=(n, d)).astype(np.float32), 12, 100, "DistL2", "grid")
    Q = rng.integers(0, 4, size=(601, d)).astype(np.float32)
    off = np.random.default_rng(4).permutation(601)[:300]
    Q[off] = uniform(300, d, 12) * np.float32(3)
    res, launch = _pair_call(native, knob, trace, g, h, o, Q, 10, 48, "pair pass, grid")
    assert len(launch) >= 2 and "visited set" in launch[1], launch
    back = _n(launch[1])
    print(f"pair pass on the grid: {back} of 601 queries handed back, status 3: {int((res.st[:, 3] == 3).sum())}")
    _assert_split(np.arange(601) < back, g, "pair pass: handed back")


@pytest.mark.parametrize("g", CAPS)
@pytest.mark.parametrize("d", [25, 32])      # DistCosine: the norm in the row's padding / beside the row
def test_pairs_after_pairs_that_outgrew_their_tables(native, oracle, tmp_path, knob, trace, d, g):
    """the table shrunk (HNSWGPU_HASH_BITS from the oracle's counters) so that some halves move to their bitmap slice and some do
    not; the query tile carries the query's norm behind the row"""
    o, h = _pair(native, oracle, tmp_path, _spread(4000, d, 31 + d), 16, 100, "DistCosine", "pc")
    Q = _spread(601, d, 32 + d)
    ref = o.parallel_search(Q, 10, 100, want_counters="per_query")
    b, moved, stayed = _split_bits(ref, 8 * max(CAPS))
    knob("HNSWGPU_HASH_BITS", b)
    res, launch = _pair_call(native, knob, trace, g, h, o, Q, 10, 100, f"pair pass, DistCosine d {d}")
    assert f"tables 2^{b} cells" in launch[0], launch
    on_bitmap = res.st[:, 6] != 0
    print(f"pair pass d {d}, 2^{b} cells: {int(on_bitmap.sum())} on the bitmap; the oracle: {int(moved.sum())} outgrow, {int(stayed.sum())} stay")
    _assert_split(on_bitmap, g, f"pair pass d {d}: on the bitmap")


# ------------------------------------------------------------------------------------------------- g. every metric, one workgroup
@pytest.mark.parametrize("dist,d,data,m", METRICS)
def test_every_metric_on_one_workgroup(native, oracle, tmp_path, knob, trace, dist, d, data, m):
    """the query tile's layout differs per metric (DistCosine keeps the query's norm behind the row): 300 queries through one tile"""
    o, h = _pair(native, oracle, tmp_path, _GEN[data](2500, d, 40 + d), m, 60, dist, "m")
    res, _, lines = _run(native, knob, trace, 1, h, o, _GEN[data](300, d, 41 + d), 10, 48, dist)
    assert any("strict 1" in ln and "slots 1" in ln for ln in lines) and np.all(res.st[:, 3] != 1)


@pytest.mark.parametrize("dist", ["DistL2", "DistCosine"])
def test_simd8_arithmetic_on_one_workgroup(native, oracle, tmp_path, knob, trace, dist):
    d = 37
    o, h = _pair(native, oracle, tmp_path, uniform(2500, d, 61), 12, 60, dist, "s8")
    Q = uniform(300, d, 62)
    h.set_arithmetic("simd8")
    o.set_simd_order(True)
    try:
        res, _, _ = _run(native, knob, trace, 1, h, o, Q, 10, 64, dist + " simd8")
        o.set_simd_order(False)                # the path ran: the scalar order gives other distance bits somewhere
        assert not np.array_equal(o.parallel_search(Q, 10, 64).dists.view(np.uint32), res.dists.view(np.uint32))
    finally:
        h.set_arithmetic("scalar")
        o.set_simd_order(False)


# ------------------------------------------------------------------------------------------------- h. both descent kernels
@pytest.mark.parametrize("n,d,m,k,ef,slots,pair", [
    (3000, 24, 8, 10, 48, 1, 1),        # short upper lists: two queries per wavefront
    (2500, 16, 40, 10, 50, 16, 0),      # upper lists of 40 ids: one query per wavefront; rows of 80 ids, the 16-slot kernels
])
def test_both_descent_kernels_query_after_query(native, oracle, tmp_path, knob, trace, n, d, m, k, ef, slots, pair):
    """q += gridDim.x: 301 queries (151 pairs) through one and through three wavefronts' tiles"""
    o, h = _pair(native, oracle, tmp_path, uniform(n, d, n + m), m, 100, "DistL2", "dsc")
    assert o.get_max_level_observed() >= 1
    Q = uniform(301, d, 5)
    for g in CAPS:
        res, _, lines = _run(native, knob, trace, g, h, o, Q, k, ef, "descent")
        assert all(f"two per wavefront {pair}," in ln for ln in lines if ln.startswith("[hnswgpu descent]")), lines
        assert any(f"slots {slots}," in ln for ln in lines), lines
        assert ((res.st[:, 7] >> 8) & 0xFF).min() >= 1            # the descent read at least one upper list
        knob("HNSWGPU_NO_PAIR_DESCENT", "1")
        _, _, lines = _run(native, knob, trace, g, h, o, Q, k, ef, "single descent")
        assert all("two per wavefront 0," in ln for ln in lines if ln.startswith("[hnswgpu descent]")), lines
        knob("HNSWGPU_NO_PAIR_DESCENT", None)


# ------------------------------------------------------------------------------------------------------------ i. the hook itself
def _workgroups(native, trace, h, Q, k=10, ef=64):
    """[workgroups of every launch] of one plain call"""
    trace.take()
    res = _device_search(native, h, Q, k, ef)
    lines = trace.take()
    return res, lines, [int(_WG.search(ln).group(1)) for ln in lines]


def test_the_hook_parses_and_reloads(native, shapes_pair, knob, trace, monkeypatch):
    """below 1 or not a number: unset; read on hnswgpu_reload_env, not on the launch path"""
    o, h = shapes_pair
    Q = uniform(200, 8, 72)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    _, _, free = _workgroups(native, trace, h, Q)
    assert len(free) == 2 and min(free) > 3, free            # descent (100 pairs), search (200 queries)
    for v in ("0", "-3", "x", ""):
        knob("HNSWGPU_MAX_WG", v)
        assert _workgroups(native, trace, h, Q)[2] == free, v
    knob("HNSWGPU_MAX_WG", "3")
    assert _workgroups(native, trace, h, Q)[2] == [3, 3]
    monkeypatch.setenv("HNSWGPU_MAX_WG", "2")                # not told: the library keeps what it read
    assert _workgroups(native, trace, h, Q)[2] == [3, 3]
    native.reload_env()
    assert _workgroups(native, trace, h, Q)[2] == [2, 2]
    monkeypatch.delenv("HNSWGPU_MAX_WG")
    assert _workgroups(native, trace, h, Q)[2] == [2, 2]
    native.reload_env()
    assert _workgroups(native, trace, h, Q)[2] == free


def test_a_capped_call_changes_no_answer_and_leaves_no_trace(native, shapes, knob, trace):
    """one plain batch: the same bytes under the cap as without it; after it the uncapped call is what it was, launch lines included
    (the adaptive table size has settled before)"""
    _, o, h, Q = shapes
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    seen = [_workgroups(native, trace, h, Q, 10, 128)[1] for _ in range(2)]
    while seen[-1] != seen[-2] and len(seen) < 8:
        seen.append(_workgroups(native, trace, h, Q, 10, 128)[1])
    assert seen[-1] == seen[-2], seen
    before, lines_before, _ = _workgroups(native, trace, h, Q, 10, 128)
    assert lines_before == seen[-1]

    def same(a, b, what):
        for name in ("ids", "dists", "layers", "ranks", "counts"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (what, name)
        assert np.array_equal(a.st[:, [0, 1, 2, 3, 6, 7]], b.st[:, [0, 1, 2, 3, 6, 7]]), what

    for g in CAPS:
        knob("HNSWGPU_MAX_WG", g)
        capped, lines, wgs = _workgroups(native, trace, h, Q, 10, 128)
        assert wgs == [g] * len(wgs) and len(lines) == len(lines_before), lines
        same(capped, before, f"cap {g}")
    knob("HNSWGPU_MAX_WG", None)
    after, lines_after, _ = _workgroups(native, trace, h, Q, 10, 128)
    assert lines_after == lines_before, (lines_after, lines_before)
    same(after, before, "after")


def test_concurrent_callers_under_the_cap(native, oracle, tmp_path, knob, trace):
    """two host threads on one handle, three workgroups each: every call has its own workspace, sized from its own capped grid"""
    X, o, h = build_pair(native, oracle, tmp_path, 5000, 24, 12, 80, "DistL2", seed=61)
    batches = [uniform(300 + 37 * t, 24, 70 + t) for t in range(2)]
    refs = [o.parallel_search(b, 8, 48) for b in batches]
    _cap(knob, trace, 3)
    assert _workgroups(native, trace, h, batches[0], 8, 48)[2] == [3, 3]      # the cap is in force: descent, search
    knob("HNSWGPU_TRACE_LAUNCH", None)
    out, errs = [None] * 2, []

    def work(t):
        try:
            for _ in range(3):
                out[t] = h.parallel_search_flat(batches[t], 8, 48)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    for t in range(2):
        assert_same(out[t], refs[t])
