"""Rows of 801 to 8000 elements on every kernel that reads them.  No other test, sweep or benchmark configuration has a dimension
above 800; a long row brings no new rounding rule (DESIGN.md section 5 holds at any d, f64_reference's bound up to d = 8000) but a
regime of sizes: tens of rounds of loads in front of a row loop's exits and tails, a query tile of 4 to 32 KB in a workgroup's LDS
beside the visited table, the literal-heap kernel at the floor of its LDS budget, gather tasks of 2 to 4 rows, 2000 chunks per row
in the exact k-NN tiles.  Every comparison is exact (ids, f32 distance bits, p_ids, counts, per-query work counters against the
oracle) unless a test says otherwise; the f64 reference is the second opinion.

The rounds of row_dist (search_kernels.inc) at these strides.  A row of stride rs is U = rs / 32 units of 128 bytes (8 chunks of four
elements), rs / 4 chunks: rs / 16 per lane at four lanes per row (G = 4: batches of <= 16 rows), rs / 8 at two (G = 2).  A round is 8
loads per lane (16 in DEEP's loop), so the per-lane chunk count modulo the round length is 2 (U mod 4) at G = 4 and 4 (U mod 2) at
G = 2, and the tails behind the last full round are the ones test_gpu_distance_variants lists:

  plain G = 4   U div 4 rounds of 8, then for U mod 4 = 0, 1, 2, 3 the tails -, 2, 4, 4+2      (group_dist_simd8: the same rounds)
  plain G = 2   U div 2 rounds of 8, then for U mod 2 = 0, 1 the tails -, 4
  DEEP  G = 2   U div 4 rounds of 16, then for U mod 4 = 0, 1, 2, 3: -, 4, 8, 8+4
  PIPE  G       a = U div 4 (G = 4) or U div 2 (G = 2) rounds of 8 on two register sets that take turns; a odd leaves through the
                first `break`, a even through the second; then the plain tails

  stride (d of the sweep)            U    plain G=4    plain G=2   DEEP G=2        PIPE G=4           PIPE G=2          chunks per lane
    832 (801, 832)                   26    6 x 8, 4     13 x 8, -   6 x 16, 8      a  6 second, 4     a  13 first,  -     52 / 104
   1024 (1022, 1023, 1024)           32    8 x 8, -     16 x 8, -   8 x 16, -      a  8 second, -     a  16 second, -     64 / 128
   1056 (1025, 1054, 1055, 1056)     33    8 x 8, 2     16 x 8, 4   8 x 16, 4      a  8 second, 2     a  16 second, 4     66 / 132
   1216 (1200)                       38    9 x 8, 4     19 x 8, -   9 x 16, 8      a  9 first,  4     a  19 first,  -     76 / 152
   1248 (1246, 1247, 1248)           39    9 x 8, 4+2   19 x 8, 4   9 x 16, 8+4    a  9 first,  4+2   a  19 first,  4     78 / 156
   1536 (1536)                       48   12 x 8, -     24 x 8, -  12 x 16, -      a 12 second, -     a  24 second, -     96 / 192
   2048 (2047, 2048)                 64   16 x 8, -     32 x 8, -  16 x 16, -      a 16 second, -     a  32 second, -    128 / 256
   3072 (3072)                       96   24 x 8, -     48 x 8, -  24 x 16, -      a 24 second, -     a  48 second, -    192 / 384
   4096 (4094, 4095, 4096)          128   32 x 8, -     64 x 8, -  32 x 16, -      a 32 second, -     a  64 second, -    256 / 512
   4128 (4097)                      129   32 x 8, 2     64 x 8, 4  32 x 16, 4      a 32 second, 2     a  64 second, 4    258 / 516
   6144 (6144)                      192   48 x 8, -     96 x 8, -  48 x 16, -      a 48 second, -     a  96 second, -    384 / 768
   8000 (7999, 8000)                250   62 x 8, 4    125 x 8, -  62 x 16, 8      a 62 second, 4     a 125 first,  -    500 / 1000
What ends the row: the last entry of each cell -- a round of 16 (DEEP, U mod 4 = 0), of 8 (`-` elsewhere), or the tail of 4 or 2.

LONG_D has U mod 4 = 0, 1 and 2 only, and at G = 4 only even a: no stride of it runs the tails 4+2 (DEEP: 8+4) behind a long loop, and
none leaves the PIPE loop through its first `break` at four lanes per row.  EXTRA_D adds U = 39 (stride 1248: U mod 4 = 3, a = 9 at
G = 4 and 19 at G = 2, both odd) with the three DistCosine neighbours 1246 / 1247 / 1248, and d = 1200 (U = 38: the first `break` at
G = 4 in front of a tail of 4), which is also the stride of the DistJeffreys index of section b.

DistCosine keeps a row's f64 norm in the row's last two floats where rs - d >= 2 (norm_fits_row), else in an array beside the rows; the
round that ends with the row's last chunk lifts it out (norm_tail).  In LONG_D the norm is inside the row at 801, 1025, 1054 and 4097
-- always in a TAIL: 1054 puts it into the last two floats of a stride of 1056 (the tail of 2 at G = 4, of 4 at G = 2 and in DEEP,
behind 8 or 16 rounds), 1055 and 1056 put it beside the row, as 1023, 1024, 2047, 2048, 4095, 4096, 7999 and 8000 do.  EXTRA_D adds
1022 and 4094: the norm inside strides of 1024 and 4096, lifted out of the last FULL round (of 8; of 16 in DEEP; in PIPE the round
behind the second `break`); 1200 (stride 1216) has it in PIPE's round behind the first `break` at G = 2, 1246 in the tail of 4+2.
"""
import re

import numpy as np
import pytest

import f64_reference as F
from conftest import normalized, probability, uniform
from test_gpu_counters import _device_search, _launch_lines, _pair, assert_same_counters, check
from test_gpu_f16_storage import _same_bits, _sweep_inputs, _to
from test_gpu_parity import assert_same
from test_gpu_build_windows import _case as _build_case, oracle_build  # noqa: F401 (oracle_build: the module's fixture, used below)
from test_gpu_exact_knn import _assert_answers
from test_gpu_exact_range import _assert_range, _cycled_radii
from test_gpu_graph_components import check_all as _components_all
from test_gpu_knn_graph import _Wide, _assert_rows, _exact_expected
from test_gpu_range_search import _same as _same_range
from test_gpu_relaunch import _forced_call, _n
from test_gpu_round6 import _device_call_with_stats
from test_gpu_spanning_forest import check_all as _forest_all
from test_gpu_symmetric_graph import Index, _check_all as _symmetric_all
from test_knn_graph_abi import apply_drop_self
from test_range_search_abi import radii_from_quantiles, range_rule

pytestmark = pytest.mark.gpu

EXTRA_D = (1022, 1200, 1246, 1247, 1248, 4094)
ALL_D = tuple(sorted(set(F.LONG_D) | set(EXTRA_D)))
ALL_BATCHES = (1, 16, 17, 32, 33, 64)
ALL_BATCHES_D = (1024, 1054, 1248, 4096, 8000)               # (the issue's four, and the stride with every tail)
FOUR = ("DistL2", "DistCosine", "DistDot", "DistL1")
VARIANT_BATCHES = {"plain": ALL_BATCHES, "deep": (17, 32, 33, 64), "pipe": ALL_BATCHES}   # DEEP exists at two lanes per row only


def _batches(d, variant="plain"):
    return tuple(b for b in (ALL_BATCHES if d in ALL_BATCHES_D else (17, 64)) if b in VARIANT_BATCHES[variant])


def _bits_differ(got, want):
    """where two f32 matrices differ in their bits; two NaNs are the same answer whatever their payloads"""
    return (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))


def _mismatches(what, got, want):
    return [f"{what}: query {q} row {r}: {got.view(np.uint32)[q, r]:#x} != {want.view(np.uint32)[q, r]:#x}"
            for q, r in np.argwhere(_bits_differ(got, want))[:3]]


# ------------------------------------------------------------------------------------------------------------ a. the routine
def _reference_may_panic(metric, Q, R):
    """DistHellinger asserts 1 - sum >= -1e-6 on its f32 sum (the crate panics, the oracle throws).  The f64 sum of p == q is 1 and
    the f32 sum is off by up to gamma(d + 4) of it -- 5e-5 at d = 801, 5e-4 at d = 8000 --, so on long rows the reference has no
    answer for a pair whose sum may come out above 1 + 1e-6: pairs[q, r] is True where the error bound of the sum (f64_reference's,
    for DistHellinger) cannot rule that out.  Those pairs are held to the f64 bound alone."""
    if metric != "DistHellinger":
        return np.zeros((len(Q), len(R)), bool)
    d = Q.shape[1]
    s = np.sum(np.sqrt(Q.astype(np.float64))[:, None, :] * np.sqrt(R.astype(np.float64))[None, :, :], -1)
    return s * (1 + F.gamma(d + 4)) + d * F.TINY >= 1 + 0.9e-6


def _hostile(oracle, metric, d, simd8=False):
    """the hostile sweep of (metric, d), its f64 analysis, the oracle's distances and where the oracle has one"""
    Q, R = F.hostile_sweep(metric, d, 7, simd8)
    skip = _reference_may_panic(metric, Q, R)
    want = np.zeros((len(Q), len(R)), np.float32)
    for q in range(len(Q)):
        rows = np.flatnonzero(~skip[q])
        want[q, rows] = oracle.dist_matrix(metric, Q[q:q + 1], R[rows], simd8=simd8)[0]
    return Q, R, F.analyse(metric, Q[:, None, :], R[None, :, :], simd8), want, ~skip


def _routine(native, oracle, metric, variants, simd8=False):
    arith = "simd8" if simd8 else "scalar"
    fails, checked, overflows, compared = [], 0, 0, 0
    for d in ALL_D:
        Q, R, an, want, has = _hostile(oracle, metric, d, simd8)
        compared += int(has.sum())
        for nf in _batches(d):
            plain = native.eval_distance_matrix(metric, Q, R, nf, arithmetic=arith)
            what = f"{metric} {arith} d {d} batch {nf}"
            fails += _mismatches(what + " / oracle", np.where(has, plain, 0), want)
            fails += [what + ": " + m for m in F.describe(metric, an, plain, F.violations(an, plain))]
            for variant in variants:
                if nf in VARIANT_BATCHES[variant]:
                    got = native.eval_distance_matrix(metric, Q, R, nf, variant=variant)
                    fails += _mismatches(f"{what} {variant} / plain", got, plain)
        checked += int(np.isfinite(an.err).sum())
        overflows += int(an.must_inf.sum())
        assert len(fails) < 8, fails
    assert not fails, fails
    # against a vacuous pass (a property of the reference side alone; DistJensenShannon has no bound for a pair with a coordinate
    # whose mean rounds to 0, which among 801 to 8000 coordinates is every pair of the two subnormal rows)
    assert checked > (0.75 if metric == "DistJensenShannon" else 0.9) * len(ALL_D) * 4 * 70 and compared > 0.9 * len(ALL_D) * 4 * 70
    if metric == "DistL2":
        assert overflows > 100


@pytest.mark.parametrize("metric", F.METRICS)
def test_routine_on_long_rows(native, oracle, metric):
    """eval_distance_matrix on hostile_sweep(metric, d, 7) for every d of LONG_D and EXTRA_D: the plain routine == the oracle's
    scalar left-to-right sums, 0 ulp, and within the f64 bound; DEEP and PIPE == the plain routine, bit for bit.  Batches of
    1, 16, 17, 32, 33 and 64 at d 1024, 1054, 1248, 4096 and 8000; 17 and 64 elsewhere."""
    _routine(native, oracle, metric, ("deep", "pipe"))


@pytest.mark.parametrize("metric", FOUR)
def test_routine_on_long_rows_simd8(native, oracle, metric):
    """group_dist_simd8 on the hostile sweep in the ranges of the SIMD-order bound (hostile_sweep(simd8=True)): == the oracle's
    dist_simd8, 0 ulp, and within the f64 bound of that arithmetic"""
    _routine(native, oracle, metric, (), simd8=True)


@pytest.mark.parametrize("metric", FOUR)
def test_routine_on_long_rows_half_rows(native, oracle, metric):
    """storage="f16" on representable rows with the planted values of the F16 routine sweep (the specials of binary16 at moving places
    and in the row's last element, a copy of a query, zero rows): == the oracle on the same f32 values, == storage="f32" at the same
    batch and variant, bit for bit, through the plain, DEEP and PIPE loops; and within the f64 bound"""
    fails = []
    for d in ALL_D:
        Q, R = _sweep_inputs(native, metric, d)
        want = oracle.dist_matrix(metric, Q, R)
        an = F.analyse(metric, Q[:, None, :], R[None, :, :])
        for nf in _batches(d):
            for variant in ("plain", "deep", "pipe"):
                if nf not in VARIANT_BATCHES[variant]:
                    continue
                what = f"{metric} d {d} batch {nf} {variant}"
                f16 = native.eval_distance_matrix(metric, Q, R, nf, storage="f16", variant=variant)
                f32 = native.eval_distance_matrix(metric, Q, R, nf, storage="f32", variant=variant)
                fails += _mismatches(what + " f16 / oracle", f16, want)
                fails += _mismatches(what + " f16 / f32", f16, f32)
            fails += [f"{metric} d {d} batch {nf} f16: " + m for m in F.describe(metric, an, f16, F.violations(an, f16))]
        assert len(fails) < 8, fails
    assert not fails, fails


# --------------------------------------------------------------------------- b. search parity at every result-set shape
K = 10
EFS = ((24, 1), (100, 2), (200, 4), (600, 16), (1100, None))   # ef, result slots per lane (None: the literal-heap kernel)
INDEXES = {  # name: dist, d, M, n, data
    "l2_1024": ("DistL2", 1024, 16, 1500, "half"),          # (representable rows: section f stores them as binary16 too)
    "cos_1054": ("DistCosine", 1054, 24, 1200, "half"),     # the norm in the last two floats of a stride of 1056
    "cos_1055": ("DistCosine", 1055, 24, 1200, "uniform"),  # ... and beside the rows
    "dot_1536": ("DistDot", 1536, 16, 1200, "unit"),
    "l1_2048": ("DistL1", 2048, 12, 1000, "uniform"),
    "l2_4096": ("DistL2", 4096, 32, 1000, "uniform"),       # lists of 64 ids: two lanes per row, DEEP at ef <= 128
    "l2_4097": ("DistL2", 4097, 40, 800, "uniform"),        # deg_stride > 64: 16 slots at any ef, the loop over a list's batches
    "jeff_1200": ("DistJeffreys", 1200, 12, 800, "probability"),
    "l2_8000": ("DistL2", 8000, 16, 600, "uniform"),        # a tile of 32 000 bytes: 53 248 bytes of LDS at ef 200, of the 160 KiB
}                                                           # the device reports (section j); two tiles of the descent: 64 256
EFC = 100


def _rows(native, kind, n, d, seed):
    if kind == "half":
        return native.round_to_f16(uniform(n, d, seed))
    return {"uniform": uniform, "unit": normalized, "probability": probability}[kind](n, d, seed)


_built = {}


@pytest.fixture
def index(native, oracle, tmp_path_factory):
    """index(name) -> (X, the oracle's index, the product's handle on the oracle's dump (strict, f32 rows, uploaded), Q): built once
    per module.  Q is 300 queries of the data's kind (f32, any values) and 40 stored points."""
    def get(name):
        if name not in _built:
            dist, d, m, n, kind = INDEXES[name]
            seed = 7000 + d
            X = _rows(native, kind, n, d, seed)
            o, h = _pair(native, oracle, tmp_path_factory.mktemp("long_" + name), X, m, EFC, dist, name)
            Q = np.ascontiguousarray(np.concatenate([_rows(native, "uniform" if kind == "half" else kind, 300, d, seed + 1), X[5:45]]))
            _built[name] = (X, o, h, Q)
        X, o, h, Q = _built[name]
        h.set_strict_ties(True)
        return X, o, h, Q
    return get


def _traced(native, knob, capfd, h, Q, k, ef):
    """the device call under HNSWGPU_TRACE_LAUNCH: (result with the stats words, the launch lines)"""
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    try:
        res = _device_search(native, h, Q, k, ef)
    finally:
        lines = _launch_lines(capfd)
        knob("HNSWGPU_TRACE_LAUNCH", None)
    return res, lines


def _assert_kernel(lines, name, ef, slots, what):
    """from the launch lines: the one-query strict kernel with the intended result slots on 16-bit cells (n <= 1500: 11 id bits), or
    the literal-heap kernel"""
    if slots is None:
        assert lines and all("literal kernel" in ln for ln in lines), (what, lines)
        return
    if INDEXES[name][2] > 32:
        slots = 16
    one = [ln for ln in lines if "visited set" in ln]
    assert one and all(f"slots {slots}," in ln and "strict 1," in ln and "visited set cell16" in ln for ln in one), (what, lines)


@pytest.mark.parametrize("ef,slots", EFS)
@pytest.mark.parametrize("name", list(INDEXES))
def test_search_parity(native, index, knob, capfd, name, ef, slots):
    """strict: ids, distance bits, p_ids, counts and the per-query work counters are the oracle's, at 1, 2, 4 and 16 result slots per
    lane and in the literal-heap kernel (asserted from the launch line); lean: every unflagged query is the oracle's too"""
    X, o, h, Q = index(name)
    what = f"{name} ef {ef}"
    res, lines = _traced(native, knob, capfd, h, Q, K, ef)
    for ln in lines:
        print(what + ": " + ln)
    _assert_kernel(lines, name, ef, slots, what)
    check(native, h, o, Q, K, ef, what, res=res)
    fails = F.check_per_answer(INDEXES[name][0], X, Q, res.ids, res.dists, res.counts)   # ... and what shares nothing with the oracle
    assert not fails, (what, fails[:4])


# ------------------------------------------------------------------------------------------------- c. ties on long rows
def _grid_tripled(n, d, seed):
    """integer grid rows (values 0 to 3), each of them three times: every distance to a stored point comes three times"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 4, (n // 3, d)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([base, base, base])[rng.permutation(3 * (n // 3))])


@pytest.fixture(scope="module", params=[1024, 2048])
def grid(request, native, oracle, tmp_path_factory):
    d = request.param
    X = _grid_tripled(1200, d, 77 + d)
    o, h = _pair(native, oracle, tmp_path_factory.mktemp(f"grid{d}"), X, 8, 40, "DistL2", "grid")
    Q = np.ascontiguousarray(np.concatenate([np.random.default_rng(78 + d).integers(0, 4, (150, d)).astype(np.float32), X[:50]]))
    return d, o, h, Q


def _literal_passes(lines):
    return ([_n(ln) for ln in lines if "literal kernel, pass 0" in ln], [_n(ln) for ln in lines if "literal kernel, pass 1" in ln])


def test_ties(native, grid, knob, capfd):
    """Equal distances in every answer: the strict answer is the oracle's (ids, not only distances), with the literal heaps inside the
    launch, with the literal-heap kernel behind it (HNSWGPU_NO_INKERNEL), and with that kernel's second pass (a first-pass candidate
    heap of HNSWGPU_LITERAL_CAND_CAP entries).  The literal-heap kernel's LDS (run_exact) is max(10 KiB, tile + ids + 4096) bytes:
    at d = 1024 (tile 4096) the 10 KiB still hold, 5888 bytes of heaps -- r_lds_cap = ef + 2 = 102 entries of return_points and
    cand_lds = min(cap, 634) of candidate_points; at d = 2048 (tile 8192; any tile above 5888 bytes, d > 1472) it is the floor of
    4096 bytes: r_lds_cap = 102 and cand_lds = min(cap, 410) at ef = 100, and r_lds_cap = cand_lds = 256 at ef = 1100 (section b),
    where return_points no longer fits LDS."""
    d, o, h, Q = grid
    ef = 100
    res, lines = _traced(native, knob, capfd, h, Q, K, ef)
    assert all("strict 1," in ln for ln in lines if "visited set" in ln), lines
    assert h.last_tie_count() > 20 and h.last_tie_count() == int((res.st[:, 3] == 3).sum())
    res, ref = check(native, h, o, Q, K, ef, f"grid d {d}", tie_heavy=True, res=res)
    assert sum(len(np.unique(ref.dists[i, :ref.counts[i]])) < ref.counts[i] for i in range(len(Q))) > 20   # (the data really ties)
    knob("HNSWGPU_NO_INKERNEL", "1")
    res, lines = _traced(native, knob, capfd, h, Q, K, ef)
    p0, p1 = _literal_passes(lines)
    assert all("strict 0," in ln for ln in lines if "visited set" in ln) and p0 == [h.last_tie_count()] and p0[0] > 20 and not p1, lines
    check(native, h, o, Q, K, ef, f"grid d {d}, literal kernel", lean=False, res=res)
    knob("HNSWGPU_LITERAL_CAND_CAP", 128)      # (the median size of a candidate heap at the end of these searches: word 6)
    res, lines = _traced(native, knob, capfd, h, Q, K, ef)
    p0, p1 = _literal_passes(lines)
    print(f"grid d {d}: literal kernel on {p0}, second pass on {p1}; candidate heap sizes at the end {np.percentile(res.st[res.st[:, 3] == 3, 6], [0, 50, 100])}")
    assert len(p0) == 1 and len(p1) == 1 and 0 < p1[0] <= p0[0], lines
    check(native, h, o, Q, K, ef, f"grid d {d}, literal kernel in two passes", lean=False, res=res)


# ------------------------------------------------------------------------------- d. visited-set paths with a long tile
def test_visited_set_paths_with_a_16_kb_tile(native, index, knob, capfd):
    """DistL2 d = 4096 at ef = 200 (a query visits 983 to 995 of the 1000 points, by the oracle's counters).  A first table of 2^8
    cells (HNSWGPU_HASH_BITS): every query moves to its bitmap slice inside the launch.  With one slice (HNSWGPU_BITMAP_SLICES = 1)
    the call is three launches -- 2^8 cells, the grown table of 2^10 (768 points at most: too small again), the bitmap kernels --
    in which only workgroup 0, the one with a slice, answers during the first two.  Answers and counters are the oracle's."""
    X, o, h, Q = index("l2_4096")
    knob("HNSWGPU_HASH_BITS", 8)
    res, lines = _traced(native, knob, capfd, h, Q, K, 200)
    one = [ln for ln in lines if "visited set" in ln]
    assert len(one) == 1 and "table 2^8 cells" in one[0] and "visited set cell16" in one[0], lines
    plain = res.st[:, 3] == 0                                                       # (word 6 of such a query: bitmap_used)
    assert plain.sum() >= 0.75 * len(Q) and np.all(res.st[plain, 6] == 1), "queries that did not move to the bitmap"
    check(native, h, o, Q, K, 200, "l2_4096, 2^8 cells", res=res)
    _forced_call(native, knob, capfd, h, o, Q, K, 200, "l2_4096, one slice", bits=8)


# ------------------------------------------------------------------------------------ e. two queries per wavefront
def _assert_is_oracle(got, ref, what):
    ids, dbits, cnt, st = got
    assert np.array_equal(cnt, ref.counts.astype(np.uint32)), what
    live = np.arange(ids.shape[1])[None, :] < cnt.astype(np.int64)[:, None]
    assert np.array_equal(ids[live], ref.ids.astype(np.uint64)[live]), what
    assert np.array_equal(dbits[live], ref.dists.view(np.uint32)[live]), what
    assert_same_counters(st, ref, what)


@pytest.mark.parametrize("name", ["l2_1024", "l1_2048", "jeff_1200", "l2_8000"])
def test_descent_two_queries_per_wavefront(native, index, knob, capfd, name):
    """M <= 16: no list above the search layer holds more than 16 ids, the descent stages two query tiles per wavefront
    (hnsw_descend_pair_kernel).  Same answers and counters -- word 7 is the descent's own share -- as hnsw_descend_kernel
    (HNSWGPU_NO_PAIR_DESCENT) and the oracle; 341 queries: the last wavefront holds one."""
    X, o, h, Q = index(name)
    Q = np.ascontiguousarray(np.concatenate([Q, Q[:1]]))
    ref = o.parallel_search(Q, K, 48, want_counters="per_query")
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    two = _device_call_with_stats(native, h, Q, K, 48)
    assert "two per wavefront 1" in capfd.readouterr().err
    knob("HNSWGPU_NO_PAIR_DESCENT", "1")
    one = _device_call_with_stats(native, h, Q, K, 48)
    assert "two per wavefront 0" in capfd.readouterr().err
    _assert_is_oracle(two, ref, name + ", two per wavefront")
    _assert_is_oracle(one, ref, name + ", one per wavefront")
    assert (two[3][:, 7] >> 16).min() >= 1


@pytest.mark.parametrize("name", ["cos_1054", "l2_1024"])
def test_pair_search(native, index, knob, capfd, name):
    """HNSWGPU_PAIR_SEARCH=1, 601 queries at ef = 100: two tiles, two tables and two mirrors in a workgroup's LDS (pair_lds_bytes:
    27 392 and 18 912 bytes at these strides, so pair_occupancy gives at least 1 and the pass runs -- asserted from the trace).  Answers and
    counters equal those of the one-query kernels and the oracle."""
    X, o, h, Q = index(name)
    Q = np.ascontiguousarray(np.concatenate([Q, Q[39:300]]))
    assert len(Q) == 601
    ref = o.parallel_search(Q, K, 100, want_counters="per_query")
    knob("HNSWGPU_PAIR_SEARCH", "0")
    one = _device_call_with_stats(native, h, Q, K, 100)
    knob("HNSWGPU_PAIR_SEARCH", "1")
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    two = _device_call_with_stats(native, h, Q, K, 100)
    lines = _launch_lines(capfd)
    assert lines and "pair pass" in lines[0] and _n(lines[0]) == 601, lines
    print(name + ": " + lines[0])
    _assert_is_oracle(one, ref, name + ", one-query kernels")
    _assert_is_oracle(two, ref, name + ", pair pass")
    assert np.mean(two[3][:, 3] == 0) > 0.5, "the pass answered fewer than half of the queries"


# --------------------------------------------------------------------------------------- f. F16 and SIMD8 searches
@pytest.mark.parametrize("ef", [100, 200, 1100])
@pytest.mark.parametrize("name", ["l2_1024", "cos_1054"])
def test_half_storage_search(native, index, ef, name):
    """the same handle at F32, at F16 (round_load on binary16 chunks; DistCosine's norms move beside the rows), at F32 again: the
    oracle's answers and counters each time, and the same bits"""
    X, o, h, Q = index(name)
    assert native.f16_representable(X) == (0, None)
    ref = o.parallel_search(Q, K, ef, want_counters="per_query")
    got = []
    try:
        for storage in ("f32", "f16", "f32"):
            _to(h, storage)
            res = _device_search(native, h, Q, K, ef)
            what = f"{name} ef {ef} {storage}"
            assert_same(res, ref)
            assert_same_counters(res.st, ref, what)
            got.append(res)
    finally:
        _to(h, "f32")
    _same_bits(got[1], got[0], f"{name} ef {ef} f16 / f32")
    _same_bits(got[2], got[0], f"{name} ef {ef} f32 again")


def test_simd8_search(native, index):
    """HNSWGPU_ARITH_SIMD8 on DistL2 d = 4096 (group_dist_simd8: 32 rounds of 8 block pairs per lane) against the oracle searching in
    its SIMD-order arithmetic; the scalar order gives other distance bits, and comes back"""
    X, o, h, Q = index("l2_4096")
    scalar = o.parallel_search(Q, K, 100, want_counters="per_query")
    h.set_arithmetic("simd8")
    o.set_simd_order(True)
    try:
        ref = o.parallel_search(Q, K, 100, want_counters="per_query")
        res = _device_search(native, h, Q, K, 100)
        assert_same(res, ref)
        assert_same_counters(res.st, ref, "l2_4096 simd8")
        assert not np.array_equal(ref.dists.view(np.uint32), scalar.dists.view(np.uint32))
    finally:
        h.set_arithmetic("scalar")
        o.set_simd_order(False)
    res = _device_search(native, h, Q, K, 100)
    assert_same(res, scalar)
    assert_same_counters(res.st, scalar, "l2_4096 scalar again")


# -------------------------------------------------------------------------------------------- g. host-buffer entry
def test_host_buffer_entry(native, index, knob):
    """hnswgpu_search_batch on numpy memory, 2049 queries of d = 4096 (16 KB each: 4 rows per gather task -- tasks have had 20 rows
    or more --, 1025 rows per chunk): the default (2 chunks, up to 8 threads), HNSWGPU_HOST_CHUNKS = 1 and 3 (2049 queries make at
    most 2 chunks; 3073 make the three), HNSWGPU_HOST_THREADS = 1 -- the same bytes as the device-buffer call each time"""
    X, o, h, Q = index("l2_4096")
    big = np.ascontiguousarray(np.concatenate([uniform(3073 - len(X[:200]), 4096, 4242), X[:200]]))

    def host(Qh):
        r = h.parallel_search_flat(Qh, K, 48)
        return r.ids, r.dists.view(np.uint32), r.counts

    for nq in (2049, 3073):
        Qh = big[3073 - nq:]
        want = _device_call_with_stats(native, h, Qh, K, 48)[:3]
        for chunks, threads in ((None, None), (1, None), (3, None), (None, 1), (3, 1)):
            knob("HNSWGPU_HOST_CHUNKS", chunks)
            knob("HNSWGPU_HOST_THREADS", threads)
            got = host(Qh)
            for a, b, what in zip(got, want, ("ids", "distance bits", "counts")):
                assert a.tobytes() == b.tobytes(), (nq, chunks, threads, what)
    ref = o.parallel_search(big[:300], K, 48)
    knob("HNSWGPU_HOST_CHUNKS", None)
    knob("HNSWGPU_HOST_THREADS", None)
    assert_same(h.parallel_search_flat(big[:300], K, 48), ref)


# ------------------------------------------------------------------------- h. what reads rows outside the search path
FLAT_D = (1024, 4097, 8000)
_flat = {}


@pytest.fixture
def flat(native, oracle, tmp_path_factory):
    """flat(d): 700 points of dimension d (50 of them exact copies of others: ties that the DataId cuts) under shuffled sparse ids,
    built by the oracle (M = 8) and loaded by the product and -- from the same dump -- by the oracle again; 70 queries, five of them
    stored points; every point's own p_id; the oracle's 70 x 700 distances.  Built once per d and left unchanged."""
    def get(d):
        if d not in _flat:
            n = 700
            X = uniform(n, d, 300 + d)
            X[600:650] = X[:50]
            ids = np.random.default_rng(d).permutation(n).astype(np.uint64) * 3 + 5
            tmp = tmp_path_factory.mktemp(f"flat{d}")
            ix = Index(native, oracle, tmp, X, ids)
            o = oracle.OracleHnsw.load(str(tmp), "g", "DistL2")
            Q = uniform(70, d, 301 + d)
            Q[:5] = X[5:10]
            me = ix.h.exact_search_filters_flat(X, 1, [np.array([v], np.uint64) for v in ids])
            assert me.counts.tolist() == [1] * n and np.array_equal(me.ids[:, 0], ids)
            pids = list(zip(me.layers[:, 0].tolist(), me.ranks[:, 0].tolist()))
            _flat[d] = dict(d=d, n=n, X=X, ids=ids, ix=ix, h=ix.h, o=o, Q=Q, pids=pids, D=oracle.dist_matrix("DistL2", Q, X))
        return _flat[d]
    return get


@pytest.mark.parametrize("d", FLAT_D)
def test_exact_knn_on_long_rows(native, oracle, flat, d):
    """exact_knn_prep_kernel and the tiles of nchunk x TQ chunks at nchunk = 256, 1025 and 2000 (196 until now): the (distance, id)
    order of the oracle's distances, bit for bit, and the exact k-NN in f64; under a filter too"""
    f = flat(d)
    h, X, Q, ids, k = f["h"], f["X"], f["Q"], f["ids"], 10
    res = h.exact_search_flat(Q, k)
    _assert_answers(oracle, "DistL2", res, Q, X, ids, k, what=f"d {f['d']}")
    by_row = {int(v): i for i, v in enumerate(ids)}
    rows_of = np.vectorize(by_row.get)

    def f64(res, members):
        fails = F.check_exact_knn("DistL2", X, Q, rows_of(res.ids), res.dists, res.counts, k, members)
        assert not fails, (f["d"], fails[:4])

    f64(res, range(f["n"]))
    rows = np.sort(np.random.default_rng(9).choice(f["n"], 200, replace=False))
    res = h.exact_search_flat(Q, k, np.sort(ids[rows]))
    _assert_answers(oracle, "DistL2", res, Q, X, ids, k, rows, what=f"d {f['d']} filtered")
    f64(res, rows.tolist())


@pytest.mark.parametrize("d", FLAT_D)
def test_exact_range_on_long_rows(native, flat, d):
    """every point within a query's radius, the radii cycled through the kinds of the exact range tests (at and just below a j-th
    distance, none, all, +inf): the oracle's distances decide, bit for bit"""
    f = flat(d)
    radii, kinds = _cycled_radii(f["D"])
    assert {"at", "below", "none", "all", "inf"} <= set(kinds)
    _assert_range(f["h"].exact_range_search_flat(f["Q"], radii), f["D"], f["ids"], radii, pids=f["pids"], what=f"d {f['d']}")


@pytest.mark.parametrize("d", FLAT_D)
def test_knn_graphs_on_long_rows(native, oracle, flat, d):
    """the exact graph (its prep kernel reads the stored rows) of 70 named points against the oracle's distances, and of every
    point against the device's own exact search without the point; the approximate graph (its gather kernel: e / ix.d) against the
    oracle's search of the same vectors on the same dump, without the point"""
    f = flat(d)
    h, o, X, ids, pids, n, k = f["h"], f["o"], f["X"], f["ids"], f["pids"], f["n"], 10
    pts = np.random.default_rng(4).permutation(n)[:70]
    Dn = np.zeros((n, n), np.float32)
    Dn[pts] = oracle.dist_matrix("DistL2", X[pts], X)
    _assert_rows(h.exact_knn_graph_flat(k, ids[pts]), _exact_expected(Dn, ids, np.arange(n), pids, pts, k), f"d {f['d']} exact, 70 points")
    rows_all = np.argsort(ids)                                   # (ids are unique: NULL ids give the points by ascending id)
    wide = h.exact_search_flat(X[rows_all], k + 1)
    _assert_rows(h.exact_knn_graph_flat(k), apply_drop_self(_Wide(wide), [pids[r] for r in rows_all], k), f"d {f['d']} exact, every point")
    ref = o.parallel_search(X[pts], k + 1, 40)
    _assert_rows(h.knn_graph_flat(k, 40, ids[pts]), apply_drop_self(ref, [pids[r] for r in pts], k), f"d {f['d']} approximate")


def test_graph_pipeline_on_long_rows(native, flat):
    """d = 1024: the symmetrised graph, its components and its minimum spanning forest from the exact and from the approximate graph,
    both modes, against their Python models -- the gather and the whole pipeline on long rows"""
    ix = flat(1024)["ix"]
    _symmetric_all(native, ix, 5, "d 1024")
    _components_all(ix, 5, "d 1024")
    _forest_all(ix, 5, "d 1024")


def test_range_search_through_the_graph(native, oracle, index):
    """DistL2 d = 1024: rounds of searches at growing ef until a query's answers reach past its radius -- the rule applied to the
    oracle's searches, bit for bit, efs and flags included"""
    X, o, h, Q = index("l2_1024")
    Q = Q[:96]
    radii = radii_from_quantiles(oracle.dist_matrix("DistL2", Q, X))
    want = range_rule(o.parallel_search, Q, radii, 8, 256)
    assert len(set(want.ef.tolist())) >= 3 and (want.flags & 1).any() and (want.counts == 0).any()
    _same_range(h.range_search_flat(Q, radii, 8, 256), want, "l2_1024")


# ------------------------------------------------------------------------------------- i. GPU-assisted construction
def test_gpu_assisted_build(native, oracle, oracle_build):
    """DistL2 d = 1024, n = 2000, windows of 256 points (hnsw_build_search_kernel and hnsw_build_select_kernel stage a 4 KB tile):
    the dump equals the windowed oracle's byte for byte, and every list of the result holds f64-correct distances"""
    cfg = dict(dist="DistL2", d=1024, m=12, efc=60, n=2000)
    stats, sizes = _build_case(native, oracle_build, oracle, cfg)
    assert sizes == [256, 256, 256, 208] and stats["selections_pruned"] > 500 and stats["max_candidates"] == 60, (stats, sizes)
    directory, _, _, _, X = oracle_build(cfg)
    h = native.HnswIo(directory, "gpu").load_hnsw("DistL2")
    check = {}
    fails = F.check_graph(h, X, "DistL2", cfg["m"], oracle.levels(cfg["m"], len(X), 1.0), check)
    assert not fails, fails[:4]
    assert check["edges"] > 2000 * 12


# ------------------------------------------------------------------------ j. the LDS limit: the clamp and the refusal
def _lds_limit(native):
    """the device's limit as the library reads it (hipDeviceAttributeMaxSharedMemoryPerBlock), from the refusal of rows that fit no
    device: the message names it"""
    with pytest.raises(native.HnswError) as e:
        native.eval_distance_matrix("DistL2", np.zeros((1, 400000), np.float32), np.zeros((1, 400000), np.float32), 1)
    assert e.value.code == native._native.ERR_ARG and "d = 400000" in str(e.value), e.value
    return int(re.search(r"limit is (\d+) bytes", str(e.value)).group(1))


def _search_lds(rs, tb, slots=4, heap=256):
    """a strict one-query launch on DistL2 rows of stride rs with 2^tb 16-bit cells (search_lds_bytes)"""
    return 4 * rs + 256 + (2 << tb) + ((64 * slots + 64 if slots <= 4 else 0) + heap) * 8


def test_the_table_is_clamped_where_it_does_not_fit(native, oracle, tmp_path, knob, capfd):
    """300 points (9 id bits: tables of at most 2^12 cells) at the smallest stride at which a strict launch with four result slots no
    longer fits 2^12 cells and 256 heap entries beside the tile, by the limit the device reports: the launch line names 2^11 cells and
    no more bytes than the limit; two tiles do not fit either, so the descent runs one query per wavefront (M = 8: it would take two);
    the answers and counters are the oracle's.  (Above d = 8000 the f64 bound is not stated: the oracle alone.)"""
    limit = _lds_limit(native)
    print(f"LDS limit of a workgroup: {limit} bytes")
    rs = next(r for r in range(32, 1 << 20, 32) if _search_lds(r, 12) > limit)
    assert _search_lds(rs, 11, heap=512) <= limit and 2 * 4 * rs + 256 > limit, (rs, limit)
    X = uniform(300, rs, 31)
    o, h = _pair(native, oracle, tmp_path, X, 8, 40, "DistL2", "clamp")
    Q = np.ascontiguousarray(np.concatenate([uniform(50, rs, 32), X[:10]]))
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, K, 200)
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if ln.startswith("[hnswgpu launch]")]
    print(f"stride {rs}: " + lines[0])
    assert len(lines) == 1 and "table 2^11 cells" in lines[0] and "slots 4," in lines[0] and "strict 1," in lines[0], lines
    lds = int(re.search(r"(\d+) bytes of LDS", lines[0]).group(1))
    assert lds in (_search_lds(rs, 11), _search_lds(rs, 11, heap=512)) and lds <= limit, (lds, limit)
    assert "two per wavefront 0" in err and "two per wavefront 1" not in err, err
    knob("HNSWGPU_TRACE_LAUNCH", None)
    check(native, h, o, Q, K, 200, f"stride {rs}, clamped table", res=res)
    # one stride below, the table asked for fits: nothing is clamped
    assert _search_lds(rs - 32, 12) <= limit


def test_rows_that_fit_no_launch_are_refused(native):
    """64 points at the smallest d whose tile leaves no room for the smallest search state (min_workgroup_lds_bytes: 4 rs + 4896 bytes
    above the limit): the search is refused with HNSWGPU_ERR_ARG before its first launch, the message names d, the bytes and the
    limit, and no output array is touched; one stride below, the same call answers"""
    from hnsw_rs_amd.api import BatchResult
    limit = _lds_limit(native)
    rs = next(r for r in range(32, 1 << 20, 32) if 4 * r + 4896 > limit)
    for d, refused in ((rs - 31, True), (rs - 32, False)):
        X = uniform(64, d, 33)
        h = native.Hnsw(8, 64, 16, 24, "DistL2")
        h.set_build_options(nthreads=1)
        h.parallel_insert(X)
        h.upload(0)
        out = BatchResult(np.full((5, 3), 0xA5A5, np.uint64), np.full((5, 3), -3.0, np.float32), np.full((5, 3), 9, np.uint8),
                          np.full((5, 3), -7, np.int32), np.full(5, 77, np.uint32))
        if not refused:
            res = h.parallel_search_flat(X[:5], 3, 16, out=out)
            assert res.counts.tolist() == [3] * 5 and res.ids[:, 0].tolist() == [0, 1, 2, 3, 4] and (res.dists[:, 0] == 0).all()
            continue
        with pytest.raises(native.HnswError) as e:
            h.parallel_search_flat(X[:5], 3, 16, out=out)
        msg = str(e.value)
        assert e.value.code == native._native.ERR_ARG, e.value
        assert f"d = {d} " in msg and f"{4 * rs + 4896} bytes" in msg and f"{limit} bytes" in msg, msg
        assert (out.ids == 0xA5A5).all() and (out.dists == -3.0).all() and (out.layers == 9).all() and (out.ranks == -7).all() and (out.counts == 77).all()
