"""The fixed-shape search kernels (csrc/search_kernels.inc: hnsw_search_kernel<METRIC, S, TABLE, SHAPE, STRICT>).  SHAPE_R128_EF knows
at compile time that a row is 128 elements and that ef == 64 S; the host launches it exactly where the replica and the call have that
shape (DeviceIndex::SearchCall::shape_launch: DistL2 on f32 rows in the scalar arithmetic, ef 64 or 128, 16-bit-cell tables), and
SHAPE_ANY -- the kernel that takes both values at run time -- everywhere else.  HNSWGPU_NO_SHAPE=1 sends every launch to SHAPE_ANY.

Every case runs its call twice, by default and under HNSWGPU_NO_SHAPE=1, and asserts
  * from the "[hnswgpu shape]" trace lines (HNSWGPU_TRACE_LAUNCH=2: level 1 stays one line per launch) which kernel every launch
    of either call ran,
  * that the two calls agree bit for bit in ids, distances, counts, layers, ranks and the stats words, and
  * that the answers and the per-query work counters are the oracle's (strict), or sound by the lean contract (lean).
Of the eight stats words, 4 and 5 are the query's start and end on the device clock and differ between any two calls; they are left
out.  Word 6 (the query ended on its workgroup's HBM bitmap slice) follows the size of the visited table, which the driver adapts
from one call to the next with the same ef (table_feedback: two calls on the SAME kernel differ in it); it is compared where the test
fixes the table size (HNSWGPU_HASH_BITS).

d stays a run-time value in SHAPE_R128_EF (the scalar distance routines never read it), so rows of 97 .. 128 elements, padded to
128, take it too.  Graphs are built by the product builder on the host with one thread and read back by the oracle from the dump.
"""
import re

import numpy as np
import pytest

from conftest import uniform
from test_gpu_counters import _device_search, assert_lean_sound, assert_same_counters
from test_gpu_parity import assert_same
from test_gpu_relaunch import _assert_three_launches, _visited

pytestmark = pytest.mark.gpu

R128, ANY = "SHAPE_R128_EF", "SHAPE_ANY"
N, NQ, K = 4000, 300, 10


def _grid(n, d, seed):
    """small-integer grid (coordinates 0 .. 15: squared distances are integers): equal distances are frequent, without being the rule"""
    return np.ascontiguousarray(np.random.default_rng(seed).integers(0, 16, (n, d)).astype(np.float32))


def _index(native, oracle, tmp_path, X, m, dist="DistL2", efc=100, tag="shape"):
    hb = native.Hnsw(m, len(X), 16, efc, dist)
    hb.set_build_options(nthreads=1)
    hb.parallel_insert(X)
    hb.file_dump(tmp_path, tag)
    del hb
    h = native.HnswIo(tmp_path, tag).load_hnsw(dist)
    h.upload(0)
    return oracle.OracleHnsw.load(tmp_path, tag, dist), h


def _traced(native, capfd, h, Q, k, ef):
    """the call, its "[hnswgpu shape]" lines (one per launch of the one-query kernels) and its "[hnswgpu launch]" lines"""
    capfd.readouterr()
    res = _device_search(native, h, Q, k, ef)
    err = capfd.readouterr().err.splitlines()
    res.shapes = [re.search(r"queries on (SHAPE_\w+):", ln).group(1) for ln in err if ln.startswith("[hnswgpu shape]")]
    res.lines = [ln for ln in err if ln.startswith("[hnswgpu launch]")]
    res.launches = h.last_kernel_ms()[1]
    return res


def _assert_bit_equal(a, b, what, words=(0, 1, 2, 3, 7)):
    assert np.array_equal(a.counts, b.counts), what
    assert np.array_equal(a.ids, b.ids), what
    assert np.array_equal(a.dists.view(np.uint32), b.dists.view(np.uint32)), what
    assert np.array_equal(a.layers, b.layers) and np.array_equal(a.ranks, b.ranks), what
    for w in words:
        bad = np.flatnonzero(a.st[:, w] != b.st[:, w])
        assert bad.size == 0, f"{what}: stats word {w} differs for {bad.size} queries, first {bad[:4].tolist()}: {a.st[bad[:4], w].tolist()} / {b.st[bad[:4], w].tolist()}"


def _both(native, knob, capfd, h, o, Q, k, ef, want, what, strict=True, tie_heavy=False, words=(0, 1, 2, 3, 7)):
    """the call by default (every launch on the shape `want` names: a name, or a list with one name per launch) and under
    HNSWGPU_NO_SHAPE=1 (SHAPE_ANY throughout): the same bits, and the oracle's answers.  Returns (default result, oracle's)."""
    ref = o.parallel_search(Q, k, ef, want_counters="per_query")
    knob("HNSWGPU_TRACE_LAUNCH", "2")
    h.set_strict_ties(strict)
    try:
        res = _traced(native, capfd, h, Q, k, ef)
        knob("HNSWGPU_NO_SHAPE", "1")
        off = _traced(native, capfd, h, Q, k, ef)
        knob("HNSWGPU_NO_SHAPE", None)
    finally:
        h.set_strict_ties(True)
    assert len(res.shapes) >= 1 and len(res.shapes) == sum("visited set" in ln for ln in res.lines), (what, res.shapes, res.lines)
    assert res.shapes == ([want] * len(res.shapes) if isinstance(want, str) else want), (what, res.shapes)
    assert off.shapes == [ANY] * len(res.shapes), (what, off.shapes)
    assert all(f"strict {int(strict)}" in ln for ln in res.lines + off.lines if "visited set" in ln and "bitmap" not in ln), (what, res.lines)
    _assert_bit_equal(res, off, what, words)
    if strict:
        assert_same(res, ref)
        assert_same_counters(res.st, ref, what)
        assert np.all(np.isin(res.st[:, 3], (0, 3))), (what, np.unique(res.st[:, 3]))
    else:
        assert_lean_sound(res, ref, tie_heavy, what)
    return res, ref


# --------------------------------------------------------------------------------------------------------------- main path
@pytest.fixture(scope="module")
def main_pair(native, oracle, tmp_path_factory):
    return _index(native, oracle, tmp_path_factory.mktemp("shape_main"), uniform(N, 128, 128), 16)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("ef,slots", [(64, 1), (128, 2)])
def test_main_path(native, main_pair, knob, capfd, ef, slots, strict):
    o, h = main_pair
    res, _ = _both(native, knob, capfd, h, o, uniform(NQ, 128, 7), K, ef, R128, f"d 128 ef {ef} strict {strict}", strict=strict)
    assert all(f"slots {slots}," in ln and "cell16" in ln for ln in res.lines if "visited set" in ln), res.lines


@pytest.mark.parametrize("d", [100, 97])
def test_padded_rows(native, oracle, tmp_path, knob, capfd, d):
    """rows of d < 128 elements behind a stride of 128: the shape keeps d a run-time value, so they take it"""
    o, h = _index(native, oracle, tmp_path, uniform(N, d, d), 16)
    for ef in (64, 128):
        _both(native, knob, capfd, h, o, uniform(NQ, d, 8), K, ef, R128, f"d {d} ef {ef}")
    _both(native, knob, capfd, h, o, uniform(NQ, d, 8), K, 64, R128, f"d {d} lean", strict=False)


# ------------------------------------------------------------------------------------------------- ties and literal replay
TIE_SEED = 41


def test_ties_and_literal_replay(native, oracle, tmp_path, knob, capfd):
    """data from a small integer grid.  On the CPU first, from the oracle: at least 8 queries whose first k + 1 answers hold two equal
    neighbouring distances within the first k.  The device's final result array holds the oracle's distances, so for exactly those
    queries final_order_ambiguous fires on the device (its condition reads nothing else) and the first k come from
    literal_return_points: every one of them must carry status 3 and the oracle's ids.  Queries that replayed their log through
    literal_candidate_pop (stats word 7 bit 1) must occur as well."""
    o, h = _index(native, oracle, tmp_path, _grid(N, 128, TIE_SEED), 16)
    Q = _grid(NQ, 128, TIE_SEED + 1)
    for ef in (64, 128):
        wide = o.parallel_search(Q, K + 1, ef)
        full = wide.counts == K + 1
        amb = full & (wide.dists[:, :K] == wide.dists[:, 1:K + 1]).any(1)
        print(f"ef {ef}: {int(amb.sum())} of {NQ} queries with equal distances among the oracle's first {K}")
        assert amb.sum() >= 8
        res, _ = _both(native, knob, capfd, h, o, Q, K, ef, R128, f"ties ef {ef}")
        st3, popped = res.st[:, 3] == 3, (res.st[:, 7] & 2) != 0
        print(f"ef {ef}: status 3: {int(st3.sum())} queries, {int((st3 & popped).sum())} behind a literal pop, {int((st3 & ~popped).sum())} by the final order alone")
        assert st3.sum() >= 8 and np.all(st3[amb]), (int(st3.sum()), np.flatnonzero(amb & ~st3)[:8])
        assert (st3 & popped).any(), "no query replayed its log"
        assert h.last_tie_count() == int(st3.sum())
    _both(native, knob, capfd, h, o, Q, K, 64, R128, "ties lean", strict=False, tie_heavy=True)


# ---------------------------------------------------------------------------------------------------- overflow and relaunch
def test_overflow_and_relaunch(native, main_pair, knob, capfd):
    """first tables of 2^6 cells, one bitmap slice: every query outgrows the first table and the second (asserted from the oracle's
    counters), so what the first two launches answer they answer after a migration to workgroup 0's slice inside the launch -- one
    query each: a launch has a workgroup per query, and workgroup 0 starts with the first of the list.  The second launch has tables of
    2^8 cells; the third runs the bitmap kernels, which exist as SHAPE_ANY only."""
    o, h = main_pair
    Q = uniform(NQ, 128, 9)
    knob("HNSWGPU_HASH_BITS", 6)
    knob("HNSWGPU_BITMAP_SLICES", 1)
    res, ref = _both(native, knob, capfd, h, o, Q, K, 64, [R128, R128, ANY], "relaunch", words=(0, 1, 2, 3, 6, 7))
    assert np.all(_visited(ref) > 0.75 * 2 ** 8)
    n1, n2, n3 = _assert_three_launches(res.lines, 6, len(Q), res.launches, "relaunch")
    print(f"relaunch: {n1} / {n2} / {n3} queries")
    assert n1 > n2 > n3


# ------------------------------------------------------------------------------------------------- a workgroup's second query
@pytest.mark.parametrize("strict", [True, False])
def test_second_query_of_a_workgroup(native, main_pair, knob, capfd, strict):
    o, h = main_pair
    knob("HNSWGPU_MAX_WG", 3)
    res, _ = _both(native, knob, capfd, h, o, uniform(40, 128, 10), K, 64, R128, f"3 workgroups, strict {strict}", strict=strict)
    assert all(" 3 workgroups" in ln for ln in res.lines if "visited set" in ln), res.lines


# ---------------------------------------------------------------------------------- calls that must not take the new kernel
@pytest.mark.parametrize("ef", [50, 65])
def test_other_ef_runs_shape_any(native, main_pair, knob, capfd, ef):
    o, h = main_pair
    _both(native, knob, capfd, h, o, uniform(NQ, 128, 11), K, ef, ANY, f"ef {ef}")


@pytest.mark.parametrize("d,m,dist", [(128, 40, "DistL2"), (64, 16, "DistL2"), (128, 16, "DistCosine")])
def test_other_indexes_run_shape_any(native, oracle, tmp_path, knob, capfd, d, m, dist):
    """lists of more than 64 ids (the 16-slot kernels), rows of another stride, another metric"""
    o, h = _index(native, oracle, tmp_path, uniform(2000, d, d + m), m, dist)
    res, _ = _both(native, knob, capfd, h, o, uniform(200, d, 12), K, 64, ANY, f"{dist} d {d} M {m}")
    if m == 40:
        assert all("slots 16," in ln for ln in res.lines if "visited set" in ln), res.lines
