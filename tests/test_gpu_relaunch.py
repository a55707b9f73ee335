"""The search driver's relaunch paths (SearchCall::relaunch_loop behind its first launch, pass 1 of run_exact), which need several
million points -- or a candidate heap of more than 2^17 entries -- before a call takes them by itself.  Two test hooks bring them to
test sizes: HNSWGPU_BITMAP_SLICES caps the HBM visited-bitmap slices of a search launch (1: only workgroup 0 owns one, every other
workgroup hands a query whose LDS table fills up back to the host), HNSWGPU_LITERAL_CAND_CAP the candidate heap of the literal
kernel's first pass.  With one slice and a forced first table (HNSWGPU_HASH_BITS = b) a call is three launches of the one-query
kernels: tables of 2^b cells, tables of 2^(b + 2), then the TABLE_GLOBAL_BITMAP kernels on one persistent workgroup.

The bar is the suite's: ids, f32 distance bits, p_ids, counts and the per-query work counters identical to the oracle -- a query that
was abandoned and searched again reports the work of ONE search.  Every test asserts from the HNSWGPU_TRACE_LAUNCH lines that the
path it is about ran.  b comes from the oracle's per-query counters, on the CPU: at least 5 % of the queries visit more points at
layer 0 than a table of 2^(b + 2) cells takes (0.75 x 2^(b + 2): the third launch is not empty) and at least 5 % fit it with the 64
ids of one more list (the second launch answers some).  Uniform data visits within a factor 1.4 of its median, which no power of
two separates; rows confined to subspaces of 3, 6, 10 and d dimensions (_spread) visit within a factor 4 to 7.
"""
import re

import numpy as np
import pytest

import f64_reference as F
import oracle_lib
from conftest import probability, uniform
from test_gpu_counters import _device_search, _launch_lines, _pair, assert_lean_sound, assert_same_counters, check
from test_gpu_f64_reference import _exhaustive_index
from test_gpu_filter_set import _assert_equal, _oracle_answers
from test_gpu_parity import _tie_heavy, assert_same

pytestmark = pytest.mark.gpu


def _spread(n, d, seed, kind="uniform"):
    """rows of `kind` of which a quarter each live in the first 3, 6, 10 and all d coordinates (zeros behind): searches among them
    visit few to many points"""
    x = probability(n, d, seed) if kind == "probability" else uniform(n, d, seed)
    r = np.random.default_rng(seed + 1000).integers(0, 4, n)
    for part, keep in ((0, 3), (1, 6), (2, 10)):   # (probability vectors: nearly nothing there -- a zero against a non-zero is a NaN)
        x[r == part, keep:] *= np.float32(1e-3 if kind == "probability" else 0)
    if kind == "probability":
        x = (x / x.sum(1, dtype=np.float32)[:, None]).astype(np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if kind == "normalized":
        for i in range(n):
            oracle_lib.lib().orc_l2_normalize(x[i].ctypes.data, d)
    return x


def _visited(ref):
    """points a query visits at layer 0 by the oracle (the kernels' n_visited): its distance evaluations without the descent's"""
    return ref.per_query[:, 0].astype(np.int64) - ref.per_query[:, 3].astype(np.int64)


def _forced_bits(ref, lo=6, hi=12):
    """the b of the module's docstring, from the oracle's counters; asserts both 5 % conditions"""
    vis = _visited(ref)
    share = {b: (np.mean(vis > 0.75 * 2 ** (b + 2)), np.mean(vis + 64 <= 0.75 * 2 ** (b + 2))) for b in range(lo, hi + 1)}
    b = max(share, key=lambda t: min(share[t]))
    over, fit = share[b]
    assert over >= 0.05, f"b {b}: only {over:.3f} of the queries outgrow 2^{b + 2} cells (visited: {np.percentile(vis, [0, 5, 50, 95, 100])})"
    assert fit >= 0.05, f"b {b}: only {fit:.3f} of the queries fit 2^{b + 2} cells (visited: {np.percentile(vis, [0, 5, 50, 95, 100])})"
    return b


def _split_bits(ref, need, lo=6, hi=12):
    """a first table of 2^b cells that some queries outgrow INSIDE a launch and some do not (_forced_bits sizes the table after the
    next, 2^(b + 2)), from the oracle's counters: a query that visits more than 0.75 x 2^b points at layer 0 moves to its bitmap
    slice, one that stays 64 ids (a batch) below that never does (gather_batch's first check).  Asserts `need` queries of each kind;
    returns b and the two sets."""
    vis = _visited(ref)
    sets = {b: (vis > 0.75 * 2 ** b, vis + 64 <= 0.75 * 2 ** b) for b in range(lo, hi + 1)}
    b = max(sets, key=lambda t: min(sets[t][0].sum(), sets[t][1].sum()))
    moved, stayed = sets[b]
    assert moved.sum() >= need and stayed.sum() >= need, (b, int(moved.sum()), int(stayed.sum()), np.percentile(vis, [0, 5, 50, 95, 100]))
    return b, moved, stayed


_QUERIES = re.compile(r"\] (?:pair pass: |literal kernel, pass \d: )?(\d+) queries")


def _n(line):
    return int(_QUERIES.search(line).group(1))


def _assert_three_launches(lines, b, first, launches, what=""):
    """tables of 2^b cells, tables of 2^(b + 2), the bitmap kernels, on `first` > n2 > n3 >= 1 queries; and last_kernel_ms's count"""
    one = [ln for ln in lines if "visited set" in ln]
    assert len(one) == 3, (what, lines)
    assert f"table 2^{b} cells" in one[0] and "visited set bitmap" not in one[0], (what, one)
    assert f"table 2^{b + 2} cells" in one[1] and "visited set bitmap" not in one[1], (what, one)
    assert "visited set bitmap" in one[2], (what, one)
    n1, n2, n3 = (_n(ln) for ln in one)
    assert n1 == first and n1 > n2 > n3 >= 1, (what, n1, n2, n3)
    pair = sum("pair pass" in ln for ln in lines)
    literal = 1 if any("literal kernel" in ln for ln in lines) else 0   # (rerun_ties counts its passes as one launch)
    assert launches == 3 + pair + literal, (what, launches, lines)
    return n1, n2, n3


def _forced_call(native, knob, capfd, h, o, Q, k, ef, what, slices=1, lean=True, tie_heavy=False, bits=None):
    """the call under HNSWGPU_BITMAP_SLICES and the b of the oracle: three launches, answers and counters; strict, then lean"""
    ref = o.parallel_search(Q, k, ef, want_counters="per_query")
    b = _forced_bits(ref) if bits is None else bits
    knob("HNSWGPU_HASH_BITS", b)
    knob("HNSWGPU_BITMAP_SLICES", slices)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, k, ef)
    lines = _launch_lines(capfd)
    _, launches = h.last_kernel_ms()
    res.ties = h.last_tie_count()
    res.lines = lines
    res.n = _assert_three_launches(lines, b, len(Q), launches, what)
    assert_same(res, ref)
    assert_same_counters(res.st, ref, what)
    assert np.all(res.st[:, 3] != 1), f"{what}: queries left abandoned {np.flatnonzero(res.st[:, 3] == 1)[:8]}"
    if lean:
        h.set_strict_ties(False)
        try:
            lres = _device_search(native, h, Q, k, ef)
            _, launches = h.last_kernel_ms()
        finally:
            h.set_strict_ties(True)
        lines = _launch_lines(capfd)
        assert all("strict 0" in ln for ln in lines if "visited set" in ln) and not any("literal kernel" in ln for ln in lines), lines
        _assert_three_launches(lines, b, len(Q), launches, what + " (lean)")
        assert_lean_sound(lres, ref, tie_heavy, what + " (lean)")
    knob("HNSWGPU_TRACE_LAUNCH", None)
    return res, ref, b


# ------------------------------------------------------------------------------------------- a. every result-set shape
@pytest.fixture(scope="module")
def shapes(native, oracle, tmp_path_factory):
    X = _spread(4000, 16, 21)
    o, h = _pair(native, oracle, tmp_path_factory.mktemp("relaunch"), X, 16, 100, "DistL2", "rl")
    return X, o, h, _spread(600, 16, 22)


@pytest.mark.parametrize("ef,slots", [(64, 1), (128, 2), (256, 4), (512, 16)])
def test_three_launches_at_every_result_set_shape(native, shapes, knob, capfd, ef, slots):
    X, o, h, Q = shapes
    res, _, _ = _forced_call(native, knob, capfd, h, o, Q, 10, ef, f"ef {ef}")
    assert all(f"slots {slots}," in ln for ln in res.lines if "visited set" in ln), res.lines
    # ... and against something that shares nothing with the oracle: every returned distance within the f64 bound of its id's
    fails = F.check_per_answer("DistL2", X, Q, res.ids, res.dists, res.counts)
    assert not fails, fails[:4]


def test_three_launches_on_rows_of_more_than_64_ids(native, oracle, tmp_path, knob, capfd):
    """M = 40: lists of 80 ids, the 16-slot kernels at any ef, the loop over a list's batches inside gather_batch -- a query gives up
    in front of the first or the second batch of a list"""
    o, h = _pair(native, oracle, tmp_path, _spread(4000, 16, 23), 40, 100, "DistL2", "m40")
    res, _, _ = _forced_call(native, knob, capfd, h, o, _spread(600, 16, 24), 10, 100, "M 40")
    assert all("slots 16," in ln for ln in res.lines if "visited set" in ln), res.lines


@pytest.mark.parametrize("n,d,m,ef,slots", [(250, 16, 24, 256, 4), (500, 16, 32, 512, 16), (250, 16, 40, 256, 16)])
def test_exhaustive_search_through_three_launches(native, oracle, tmp_path, knob, capfd, n, d, m, ef, slots):
    """ef >= n: the answers of the global-bitmap kernels are the exact f64 k-NN of the reachable set.  Every query visits every
    reachable point, so only workgroup 0 -- the one with a slice -- answers in the first two launches (n1 > n2 > n3 all the same,
    the 5 % conditions cannot hold); and only with 4 and 16 slots: a third launch needs more than 0.75 x 2^8 = 192 points behind
    the smallest first table (2^6 cells), ef >= n with 1 or 2 slots at most 128."""
    X, h, reach = _exhaustive_index(native, oracle, tmp_path, "DistL2", n, d, m, 3)
    assert len(reach) > 192
    Q = uniform(200, d, 4)
    Q[:10] = X[:10]
    knob("HNSWGPU_HASH_BITS", 6)
    knob("HNSWGPU_BITMAP_SLICES", 1)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = h.parallel_search_flat(Q, 10, ef)
    lines = _launch_lines(capfd)
    _assert_three_launches(lines, 6, len(Q), h.last_kernel_ms()[1], f"exhaustive, slots {slots}")
    assert all(f"slots {slots}," in ln for ln in lines if "visited set" in ln), lines
    fails = F.check_exact_knn("DistL2", X, Q, res.ids, res.dists, res.counts, 10, reach)
    assert not fails, fails[:4]


# ---------------------------------------------------------------------------------------------------------- b. metrics
@pytest.mark.parametrize("dist,d,kind,simd8", [
    ("DistCosine", 25, "uniform", False),        # the norm rides in the row's padding
    ("DistCosine", 32, "uniform", False),        # the separate norm array
    ("DistDot", 30, "normalized", False),
    ("DistL1", 12, "uniform", False),
    ("DistJensenShannon", 12, "probability", False),
    ("DistL2", 37, "uniform", True),             # SIMD-order arithmetic: KM_L2_SIMD8's kernels, the oracle in the same order
])
def test_three_launches_per_metric(native, oracle, tmp_path, knob, capfd, dist, d, kind, simd8):
    o, h = _pair(native, oracle, tmp_path, _spread(4000, d, 31 + d, kind), 16, 100, dist, "met")
    Q = _spread(600, d, 32 + d, kind)
    if simd8:
        h.set_arithmetic("simd8")
        o.set_simd_order(True)
    try:
        res, _, _ = _forced_call(native, knob, capfd, h, o, Q, 10, 100, dist + (" simd8" if simd8 else ""))
        if simd8:
            o.set_simd_order(False)                # the path ran: the scalar order gives other distance bits somewhere
            assert not np.array_equal(o.parallel_search(Q, 10, 100).dists.view(np.uint32), res.dists.view(np.uint32))
    finally:
        h.set_arithmetic("scalar")
        o.set_simd_order(False)


# ----------------------------------------------------------------------------------------------- c. 32-bit cells first
def test_three_launches_from_32_bit_cells(native, oracle, tmp_path, knob, capfd):
    """66 000 points, 17 id bits: a first table of 2^6 cells cannot keep 14 bits of an id in a 16-bit cell, so the first launch runs
    the 32-bit-cell kernels, the grown table (2^8) is 16-bit cells, the last launch the bitmap.  Every query leaves the first launch at
    gather_batch's first check (n_visited + 64 > 0.75 x cells).  Its exit behind a failed 32-bit probe is reached by no input, here or
    at any n: visit_cell32 fails only on a table without an empty cell, and the first check keeps every table below 75 % load
    (after a batch n_visited <= 0.75 x cells) -- that exit is defensive."""
    o, h = _pair(native, oracle, tmp_path, _spread(66000, 8, 51), 6, 16, "DistL2", "c32")
    Q = _spread(600, 8, 52)
    res, _, _ = _forced_call(native, knob, capfd, h, o, Q, 10, 32, "cell32 first", bits=6)
    one = [ln for ln in res.lines if "visited set" in ln]
    assert "visited set cell32" in one[0] and "visited set cell16" in one[1], one
    _forced_bits(o.parallel_search(Q, 10, 32, want_counters="per_query"), 6, 6)     # both 5 % conditions at b = 6


# --------------------------------------------------------------------------------------------------------------- d. ties
TIES = [("grid", 4000, 6, 100), ("duplicates", 4000, 6, 122)]


@pytest.mark.parametrize("kind,n,d,ef", TIES)
def test_ties_across_relaunches(native, oracle, tmp_path, knob, capfd, kind, n, d, ef):
    """hnswgpu_last_tie_count (include/hnsw_mi355x.h: queries that met a place where values do not decide, resolved or flagged) ==
    the queries with stats status 3 in a strict call -- every one of them ends with the literal heaps, inside a launch or in
    rerun_ties behind the last.  First without any cap, then through three launches: the in-kernel literal answers are counted
    in a control word the driver does not zero between launches, the flagged list spans them, and rerun_ties runs behind the
    bitmap launch (its kernels only flag)."""
    o, h = _pair(native, oracle, tmp_path, _tie_heavy(kind, n, d, 77), 8, 40, "DistL2", "ties")
    Q = _tie_heavy(kind, 600, d, 78)
    res = _device_search(native, h, Q, 10, ef)
    plain_ties, plain_status3 = h.last_tie_count(), int((res.st[:, 3] == 3).sum())
    print(f"{kind}: one launch: last_tie_count {plain_ties}, status 3 {plain_status3}")
    assert plain_status3 > 20 and plain_ties == plain_status3
    res, _, b = _forced_call(native, knob, capfd, h, o, Q, 10, ef, kind, tie_heavy=True)
    status3 = int((res.st[:, 3] == 3).sum())
    print(f"{kind}: three launches {res.n}: last_tie_count {res.ties}, status 3 {status3}")
    assert any("literal kernel" in ln for ln in res.lines), res.lines       # rerun_ties behind the bitmap launch
    assert status3 == plain_status3 and res.ties == status3, (res.ties, status3, plain_status3)
    knob("HNSWGPU_NO_INKERNEL", "1")       # nothing resolved in a launch: the flagged list grows over three launches
    res, _, _ = _forced_call(native, knob, capfd, h, o, Q, 10, ef, kind + " no in-kernel", lean=False, bits=b)
    assert all("strict 0" in ln for ln in res.lines if "visited set" in ln), res.lines
    flagged = [_n(ln) for ln in res.lines if "literal kernel, pass 0" in ln]
    print(f"{kind}: no in-kernel: last_tie_count {res.ties}, literal kernel on {flagged}")
    assert flagged == [res.ties] and res.ties == int((res.st[:, 3] == 3).sum()) and res.ties >= status3
    knob("HNSWGPU_NO_INKERNEL", None)
    knob("HNSWGPU_EXACT_FIRST", "1")
    _forced_call(native, knob, capfd, h, o, Q, 10, ef, kind + " exact first", lean=False, bits=b)
    knob("HNSWGPU_EXACT_FIRST", None)


# ------------------------------------------------------------------------------------------ e. the pair pass without slices
@pytest.mark.parametrize("nq", [1024, 1025])       # odd: the last wave's second half idles
def test_pair_pass_hands_back_what_has_no_slice(native, oracle, tmp_path, knob, capfd, nq):
    """two slices: workgroup 0 of the pair pass owns both of its halves', every other half whose table fills up goes to retry_out
    (`have_bm == false`); the one-query kernels take those over with tables of the same size (two workgroups with a slice), grow
    them, then go to the bitmap.  Strict: queries that met equal distances come back too."""
    o, h = _pair(native, oracle, tmp_path, _spread(4000, 25, 61), 16, 100, "DistCosine", "pp")
    Q = _spread(nq, 25, 62)
    knob("HNSWGPU_PAIR_SEARCH", "1")

    ref = o.parallel_search(Q, 10, 100, want_counters="per_query")
    b = _forced_bits(ref)
    knob("HNSWGPU_HASH_BITS", b)
    knob("HNSWGPU_BITMAP_SLICES", 2)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, 10, 100)
    lines = _launch_lines(capfd)
    assert "pair pass" in lines[0] and f"tables 2^{b} cells" in lines[0], lines
    assert _n(lines[0]) == nq
    handed_back = _n(lines[1])     # what the first one-query launch takes over
    assert 0 < handed_back < nq, lines
    _assert_three_launches(lines, b, handed_back, h.last_kernel_ms()[1], "pair pass")
    assert_same(res, ref)
    assert_same_counters(res.st, ref, "pair pass")
    assert np.all(res.st[:, 3] != 1)
    h.set_strict_ties(False)
    try:
        lres = _device_search(native, h, Q, 10, 100)
        launches = h.last_kernel_ms()[1]
    finally:
        h.set_strict_ties(True)
    lines = _launch_lines(capfd)
    assert "pair pass" in lines[0], lines
    _assert_three_launches(lines, b, _n([ln for ln in lines if "visited set" in ln][0]), launches, "pair pass (lean)")
    assert_lean_sound(lres, ref, False, "pair pass (lean)")


# ------------------------------------------------------------------------------------ f. the literal kernel's second pass
def _passes(lines):
    """[(queries of pass 0, queries of pass 1)] of every run_exact of the call; pass 1 must take some of pass 0's queries, not all"""
    p0 = [_n(ln) for ln in lines if "literal kernel, pass 0" in ln]
    p1 = [_n(ln) for ln in lines if "literal kernel, pass 1" in ln]
    assert p0 and len(p1) == len(p0), lines
    assert all(0 < b < a for a, b in zip(p0, p1)), (p0, p1)
    return list(zip(p0, p1))


@pytest.fixture(scope="module")
def literal_pair(native, oracle, tmp_path_factory):
    X = _spread(6000, 12, 91)
    X[3000:3300] = X[:300]
    return _pair(native, oracle, tmp_path_factory.mktemp("lit"), X, 12, 60, "DistL2", "lit")


# (the oracle does not expose its heaps' sizes: chosen so that pass 1 takes a sizeable share of pass 0's queries, which _passes asserts.
# To choose them again for other data: stats word 6 of a query the literal kernel answered is lenC, its candidate heap's size at the end
# of the search -- a lower bound of the capacity it needed; a value near the median of word 6 splits the queries)
CAP_PLAIN, CAP_FILTER, CAP_SET, CAP_TIES = 768, {20: 128, 200: 512}, 256, 96


def test_second_pass_of_the_literal_kernel_above_ef_1024(native, literal_pair, knob, capfd):
    o, h = literal_pair
    Q = _spread(120, 12, 92)
    knob("HNSWGPU_LITERAL_CAND_CAP", CAP_PLAIN)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, 10, 1100)
    print(_passes(_launch_lines(capfd)))
    assert np.all(res.st[:, 3] == 3)
    check(native, h, o, Q, 10, 1100, "ef 1100, two passes", lean=False, res=res)


def test_second_pass_of_the_literal_kernel_under_a_filter(native, literal_pair, knob, capfd):
    o, h = literal_pair
    allowed = np.sort(np.random.default_rng(30).choice(6000, 1800, replace=False)).astype(np.uint64)
    Q = np.concatenate([_spread(200, 12, 93), _spread(6000, 12, 91)[:50]])
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    for k, ef in ((10, 20), (10, 200)):
        knob("HNSWGPU_LITERAL_CAND_CAP", CAP_FILTER[ef])
        ref = o.parallel_search_filter(Q, k, ef, allowed, want_counters="per_query")
        capfd.readouterr()
        res = _device_search(native, h, Q, k, ef, allowed)
        print(_passes(_launch_lines(capfd)))
        assert np.array_equal(res.st[:, 3] == 6, ref.status == 1)           # the reference panics: status 6, count 0
        assert np.all((res.st[:, 3] == 3) | (res.st[:, 3] == 6)) and np.all(res.counts[res.st[:, 3] == 6] == 0)
        assert_same(res, ref)
        assert_same_counters(res.st, ref, f"filtered, two passes, ef {ef}")


def test_second_pass_of_the_literal_kernel_under_a_filter_set(native, literal_pair, knob, capfd):
    """the device entry (hnswgpu_search_batch_filter_set_device), which hands the d_stats words out: every query's answer and
    status against the oracle under its own filter, and its counters and status word against the oracle's one-filter search of
    that filter's queries -- a query that outgrew pass 0's heap (status 4 there) reports one search, ended by the literal kernel"""
    import torch
    from test_gpu_filter_set import _torch_call
    o, h = literal_pair
    rng = np.random.default_rng(31)
    origin = np.arange(6000, dtype=np.uint64)
    filters = [origin, np.sort(rng.choice(origin, 3000, replace=False)), np.sort(rng.choice(origin, 600, replace=False)),
               np.sort(rng.choice(origin, 60, replace=False)), np.zeros(0, np.uint64)]
    Q = _spread(95, 12, 94)
    filter_of = ((np.arange(95) * 3 + 1) % 5).astype(np.uint32)
    ref = _oracle_answers(o, Q, 10, 100, filters, filter_of)
    knob("HNSWGPU_LITERAL_CAND_CAP", CAP_SET)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    rc, got, panics = _torch_call(native, h, Q, 10, 100, filters, filter_of, torch.cuda.Stream(torch.device("cuda", 0)))
    passes = _passes(_launch_lines(capfd))
    assert rc == 0, native._native.last_error()
    # (_assert_equal: status 1 and count 0 exactly where the reference panics; the oracle reports no panic on this set -- nor on any
    # construction the suite knows, tests/test_gpu_filter_set.py -- so there is nothing to require here beyond that)
    _assert_equal(got, ref, "filter set, two passes")
    assert panics == int(ref.status.sum())
    assert np.all(got.counts[np.asarray(got.status) == 1] == 0) and np.all(got.counts[filter_of == 4] == 0)
    for f, allowed in enumerate(filters):
        mine = np.flatnonzero(filter_of == f)
        one = o.parallel_search_filter(Q[mine], 10, 100, allowed, want_counters="per_query")
        assert np.array_equal(got.stats[mine, 3], np.where(one.status == 1, 6, 3)), (f, got.stats[mine, 3].tolist())
        assert_same_counters(got.stats[mine], one, f"filter set, two passes, filter {f}")
    print(passes)


def test_second_pass_of_the_literal_kernel_in_the_tie_rerun(native, oracle, tmp_path, knob, capfd):
    o, h = _pair(native, oracle, tmp_path, _tie_heavy("grid", 4000, 6, 77), 8, 40, "DistL2", "tl")
    Q = _tie_heavy("grid", 300, 6, 78)
    knob("HNSWGPU_NO_INKERNEL", "1")
    knob("HNSWGPU_LITERAL_CAND_CAP", CAP_TIES)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, 10, 100)
    lines = _launch_lines(capfd)
    assert "strict 0" in lines[0], lines
    (flagged, _), = _passes(lines)
    assert flagged == h.last_tie_count() == int((res.st[:, 3] == 3).sum())
    check(native, h, o, Q, 10, 100, "tie rerun, two passes", lean=False, res=res)


# ----------------------------------------------------------------------------------------------- g. back to normal, the hooks
def test_forced_calls_leave_no_trace(native, shapes, knob, capfd):
    """without the hooks the call is one launch again, the same bytes, and on the table size the adaptive sizing had settled on:
    calls under HNSWGPU_HASH_BITS give it no feedback"""
    X, o, h, Q = shapes
    knob("HNSWGPU_TRACE_LAUNCH", "1")

    def plain():
        capfd.readouterr()
        res = _device_search(native, h, Q, 10, 128)
        lines = _launch_lines(capfd)
        assert len(lines) == 1 and h.last_kernel_ms()[1] == 1, lines
        return res, re.search(r"table 2\^(\d+) cells", lines[0]).group(1)

    sizes = [plain()[1] for _ in range(2)]
    while sizes[-1] != sizes[-2] and len(sizes) < 8:
        sizes.append(plain()[1])
    assert sizes[-1] == sizes[-2], sizes
    before, settled = plain()
    assert settled == sizes[-1]
    _forced_call(native, knob, capfd, h, o, Q, 10, 128, "between")
    knob("HNSWGPU_HASH_BITS", None)
    knob("HNSWGPU_BITMAP_SLICES", None)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    after, size = plain()
    assert size == settled, (size, settled)
    for name in ("ids", "dists", "layers", "ranks", "counts"):
        assert getattr(after, name).tobytes() == getattr(before, name).tobytes(), name
    assert np.array_equal(after.st[:, [0, 1, 2, 3, 6, 7]], before.st[:, [0, 1, 2, 3, 6, 7]])


def test_the_two_hooks_parse_clamp_and_reload(native, shapes, knob, capfd):
    """HNSWGPU_BITMAP_SLICES below 1 or not a number: unset; HNSWGPU_LITERAL_CAND_CAP below 1: unset, else at least 64 (the
    launch line names the capacity); both follow hnswgpu_reload_env"""
    X, o, h, Q = shapes
    Q = Q[:64]
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    knob("HNSWGPU_HASH_BITS", 8)

    def launches():
        capfd.readouterr()
        h.parallel_search_flat(Q, 10, 64)
        return len(_launch_lines(capfd))

    for v in ("0", "-3", "x"):
        knob("HNSWGPU_BITMAP_SLICES", v)
        assert launches() == 1, v
    knob("HNSWGPU_BITMAP_SLICES", "1")
    assert launches() > 1
    knob("HNSWGPU_BITMAP_SLICES", None)
    assert launches() == 1

    def capacity():
        capfd.readouterr()
        h.parallel_search_flat(Q, 10, 1100)
        return int(re.search(r"(\d+) in all", _launch_lines(capfd)[0]).group(1))

    assert capacity() == 4000
    for v, want in (("0", 4000), ("-5", 4000), ("1", 64), ("3000", 3000), ("100000", 4000)):
        knob("HNSWGPU_LITERAL_CAND_CAP", v)
        assert capacity() == want, v
    knob("HNSWGPU_LITERAL_CAND_CAP", None)
    assert capacity() == 4000
