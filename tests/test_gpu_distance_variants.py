"""The row loops of the distance routine that only the search kernel's expansion loop compiles.

The arithmetic sweeps of the suite (test_gpu_round2, test_gpu_f64_reference, test_gpu_f16_storage) go through eval_matrix_kernel with
batch_dist's defaults.  The expansion loop of hnsw_search_kernel calls batch_dist<METRIC, DEEP, PIPE, RS> instead (search_kernels.inc):
    DEEP   a strict search with 1 or 2 result slots per lane (ef <= 128)
    PIPE   a strict search with 4 result slots per lane (ef 129 .. 256)
    RS=128 a search with ef 64 or 128 on DistL2 / f32 rows of stride 128 (lean; strict: together with DEEP)
-- three more texts of the same left-to-right sum, each with loop bounds, exits and a DistCosine norm_tail condition of its own.
eval_distance_matrix(variant=...) runs them through the same test kernel, on the layout the search uploads (the norm of a DistCosine
row inside its padding where it fits, else beside it; half rows narrowed on the host).  Sections a - d hold them to the standing
contract (0 ulp against the oracle, and against the plain routine) and to the f64 bound on the hostile sweep; section e runs searches
at the row lengths no other search test has, which covers the inlined copies themselves.

The rounds of row_dist.  A row of stride rs is U = rs / 32 units of 128 bytes (8 chunks of four elements); a round of NU loads per
lane at G lanes per row covers NU * G chunks.  Batches of <= 16 rows run G = 4, larger ones G = 2 (a batch of 33: G = 2, then G = 4).

  plain G = 4   U div 4 rounds of 8, then for U mod 4 = 0, 1, 2, 3 the tails -, 2, 4, 4+2
  plain G = 2   U div 2 rounds of 8, then for U mod 2 = 0, 1 the tails -, 4
  DEEP  G = 2   U div 4 rounds of 16, then for U mod 4 = 0, 1, 2, 3: -, 4, 8, 8+4  (differs from plain from U = 4 on: d >= 97);
                DEEP's G = 4 groups are the plain ones (batches 1, 16 and the second group of 33)
  PIPE  G       a = U div (4 at G = 4, 2 at G = 2) rounds of 8 on two register sets that take turns (entered if a >= 1: d >= 33 at
                G = 2, d >= 97 at G = 4); a odd leaves through the first `break`, a even through the second; then the plain tails

  stride (d of the sweep)          DEEP G=2           PIPE G=4                 PIPE G=2
   32 (1, 25, 32: controls)        4                  a 0: tail 2              a 0: tail 4        (no variant round: fall through)
   64 (33 .. 64)                   8                  a 0: tail 4              a 1 first,  -
   96 (65 .. 96)                   8+4                a 0: tails 4+2           a 1 first,  4
  128 (97 .. 128)                  1 x 16, -          a 1 first,  -            a 2 second, -
  160 (129, 130, 158, 159, 160)    1 x 16, 4          a 1 first,  2            a 2 second, 4
  192 (161, 191, 192)              1 x 16, 8          a 1 first,  4            a 3 first,  -
  224 (193, 200, 224)              1 x 16, 8+4        a 1 first,  4+2          a 3 first,  4
  256 (225, 254, 255, 256)         2 x 16, -          a 2 second, -            a 4 second, -
  288 (257)                        2 x 16, 4          a 2 second, 2            a 4 second, 4
  320 (300)                        2 x 16, 8          a 2 second, 4            a 5 first,  -
  352 (350, 351)                   2 x 16, 8+4        a 2 second, 4+2          a 5 first,  4
  384 (383, 384), 416 (385)        3 x 16, - / 4      a 3 first,  - / 2        a 6 second, - / 4
  512 (511, 512), 544 (513)        4 x 16, - / 4      a 4 second, - / 2        a 8 second, - / 4
  640 (640), 768 (767, 768)        5, 6 x 16, -       a 5 first, 6 second, -   a 10, 12 second, -
  800 (769 .. 800)                 6 x 16, 4          a 6 second, 2            a 12 second, 4
So both exits of the PIPE loop are taken at either G with every tail behind them ({-, 2, 4, 4+2} at G = 4: strides 128 .. 224 behind
the first, 256 .. 352 behind the second; {-, 4} at G = 2: 64 / 96 and 192 / 224 behind the first, 128 / 160 and 256 / 288 behind the
second), and every DEEP continuation {-, 4, 8, 8+4} behind one round of 16 (128 .. 224) and behind two (256 .. 352).

DistCosine keeps a row's f64 norm in the last two floats of the row where the padding has room (norm_fits_row: rs - d >= 2) and in an
array beside the rows where not (d = 31 or 0 mod 32); the round that ends with the row's last chunk lifts it out (norm_tail).  The
neighbours 158 / 159 (stride 160) and 254 / 255 (stride 256) straddle the two layouts: at 160 the last chunk sits in DEEP's tail of
4, in PIPE's tail of 2 (G = 4) and tail of 4 behind the second break (G = 2); at 256 in DEEP's second round of 16 and in PIPE's last
round, reached through the second break at both G.  A PIPE last round that holds an in-row norm and leaves through the first break:
strides 128 (G = 4), 64 and 192 (G = 2; d = 161).  224 / 225 are a norm beside a stride of 224 next to a norm inside a stride of 256.  SWEEP_D has no d in 194 .. 224,
none in 321 .. 352 and neither 158 nor 254: EXTRA_D adds them here."""
import numpy as np
import pytest

import f64_reference as F
from conftest import probability, uniform
from test_gpu_counters import _device_search, _launch_lines, _pair, assert_same_counters
from test_gpu_f16_storage import _same_bits, _sweep_inputs
from test_gpu_parity import assert_same, build_pair

pytestmark = pytest.mark.gpu

EXTRA_D = (158, 200, 224, 225, 254, 350, 351)
ALL_D = tuple(sorted(set(F.SWEEP_D) | set(EXTRA_D)))
CONTROLS = (1, 25, 32)                                       # no round of either variant: the plain tails
SWEEP = {  # variant: (the d at which its loop differs from the plain one + the controls, the batch sizes)
    "deep": (tuple(d for d in ALL_D if d >= 97 or d in CONTROLS), (17, 32, 33, 64)),          # DEEP exists at two lanes per row only
    "pipe": (tuple(d for d in ALL_D if d >= 33 or d in CONTROLS), (1, 16, 17, 32, 33, 64)),
}
ALL_BATCHES = (1, 16, 17, 32, 33, 64)
R128_D = tuple(range(97, 129))
STRIDES = {(d + 31) // 32 * 32 for d in SWEEP["deep"][0]}
assert {160, 192, 224, 256, 288, 320, 352} <= STRIDES and STRIDES <= {(d + 31) // 32 * 32 for d in SWEEP["pipe"][0]}


def _inputs(metric, d):
    """3 queries x 70 rows as test_search_distance_routine_sweep draws them (probability vectors for the three probability
    metrics), with an exact copy of a query and a row whose first half is zero"""
    if metric in F.PROBABILITY_METRICS:
        rows = probability(70, d, 100 + d) if d > 1 else np.ones((70, 1), np.float32)
        q = probability(3, d, 200 + d) if d > 1 else np.ones((3, 1), np.float32)
    else:
        rng = np.random.default_rng([11, d, F.METRICS.index(metric)])
        scale = 0.05 if metric == "DistDot" else 3.0
        q = ((rng.random((3, d), dtype=np.float32) - 0.3) * scale).astype(np.float32)
        rows = ((rng.random((70, d), dtype=np.float32) - 0.3) * scale).astype(np.float32)
    rows[5] = q[0]
    if d > 2:
        rows[6, : d // 2] = 0.0
    return np.ascontiguousarray(q), np.ascontiguousarray(rows)


def _mismatches(what, got, want):
    return [f"{what}: query {q} row {r}: {got[q, r]:#x} != {want[q, r]:#x}" for q, r in np.argwhere(got != want)[:3]]


# --------------------------------------------------------------------------------- a. bit parity: the oracle, the plain routine
@pytest.mark.parametrize("variant", ["deep", "pipe"])
@pytest.mark.parametrize("metric", F.METRICS)
def test_variant_sweep(native, oracle, metric, variant):
    """eval_distance_matrix(variant) == the oracle's scalar left-to-right sums == the plain routine of the same call, bit for bit,
    at every d and batch size of the variant's sweep.  Tolerance: 0 ulp."""
    ds, batches = SWEEP[variant]
    fails = []
    for d in ds:
        q, rows = _inputs(metric, d)
        want = oracle.dist_matrix(metric, q, rows).view(np.uint32)
        for nf in batches:
            got = native.eval_distance_matrix(metric, q, rows, nf, variant=variant).view(np.uint32)
            plain = native.eval_distance_matrix(metric, q, rows, nf, variant="plain").view(np.uint32)
            fails += _mismatches(f"d {d} batch {nf} {variant} / oracle", got, want)
            fails += _mismatches(f"d {d} batch {nf} {variant} / plain", got, plain)
        assert len(fails) < 8, fails
    assert not fails, fails
    if metric in ("DistL2", "DistL1"):
        assert native.eval_distance_matrix(metric, q, rows, 32, variant=variant)[0, 5] == 0.0


# ------------------------------------------------------------------------------------------- b. the f64 bound, hostile values
def _hostile(native, metric, variant, ds, batches):
    fails, checked, overflows = [], 0, 0
    for d in ds:
        Q, R = F.hostile_sweep(metric, d, 7)
        an = F.analyse(metric, Q[:, None, :], R[None, :, :])
        for nf in batches:
            got = native.eval_distance_matrix(metric, Q, R, nf, variant=variant)
            fails += [f"d {d} batch {nf} {variant}: " + m for m in F.describe(metric, an, got, F.violations(an, got))]
        checked += int(np.isfinite(an.err).sum())
        overflows += int(an.must_inf.sum())
        assert len(fails) < 8, fails
    assert not fails, fails
    # against a vacuous pass (a property of the reference side alone: F.analyse gives the same counts without a device)
    assert checked > 0.9 * len(ds) * 4 * 70
    if metric == "DistL2":
        assert overflows > 100


@pytest.mark.parametrize("variant", ["deep", "pipe"])
@pytest.mark.parametrize("metric", F.METRICS)
def test_variant_within_the_f64_bound(native, metric, variant):
    """test_distance_routine_within_the_f64_bound for the variants: the hostile sweep (overflowing sums, subnormals, exact zeros,
    cancellation) over the d and batch sizes of (a), every result within the bound of the f64 truth, +inf where an L2 sum must
    overflow"""
    _hostile(native, metric, variant, *SWEEP[variant])


# ------------------------------------------------------------------------------------------------------------- c. half rows
@pytest.mark.parametrize("variant", ["deep", "pipe"])
@pytest.mark.parametrize("metric", ["DistL2", "DistCosine", "DistDot", "DistL1"])
def test_variant_sweep_half_rows(native, oracle, metric, variant):
    """storage="f16" through the variants (the KM_*_F16 kernels; DistCosine's norms always beside the rows): the oracle's distances on
    the same f32 values, and storage="f32" through the same variant, bit for bit"""
    ds, batches = SWEEP[variant]
    fails = []
    for d in ds:
        Q, R = _sweep_inputs(native, metric, d)
        want = oracle.dist_matrix(metric, Q, R).view(np.uint32)
        for nf in batches:
            got = native.eval_distance_matrix(metric, Q, R, nf, storage="f16", variant=variant).view(np.uint32)
            f32 = native.eval_distance_matrix(metric, Q, R, nf, storage="f32", variant=variant).view(np.uint32)
            fails += _mismatches(f"d {d} batch {nf} {variant} f16 / oracle", got, want)
            fails += _mismatches(f"d {d} batch {nf} {variant} f16 / f32", got, f32)
        assert len(fails) < 8, fails
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------ d. fixed stride
@pytest.mark.parametrize("variant", ["r128", "deep+r128"])
def test_fixed_stride_sweep(native, oracle, variant):
    """RS = 128 (the rounds folded at compile time), DistL2 on every d that pads to 128: the oracle and the plain routine, 0 ulp"""
    fails = []
    for d in R128_D:
        q, rows = _inputs("DistL2", d)
        want = oracle.dist_matrix("DistL2", q, rows).view(np.uint32)
        for nf in ALL_BATCHES:
            got = native.eval_distance_matrix("DistL2", q, rows, nf, variant=variant).view(np.uint32)
            plain = native.eval_distance_matrix("DistL2", q, rows, nf, variant="plain").view(np.uint32)
            fails += _mismatches(f"d {d} batch {nf} {variant} / oracle", got, want)
            fails += _mismatches(f"d {d} batch {nf} {variant} / plain", got, plain)
        assert len(fails) < 8, fails
    assert not fails, fails


@pytest.mark.parametrize("variant", ["r128", "deep+r128"])
def test_fixed_stride_within_the_f64_bound(native, variant):
    _hostile(native, "DistL2", variant, R128_D, ALL_BATCHES)


# ------------------------------------------------------------------------- e. searches at the row lengths no search test has
N, M, EFC, NQ, K = 2000, 24, 100, 200, 10                    # layer-0 lists of up to 48 ids: a first expansion brings more than 32 fresh ones
EFS = ((64, 1), (100, 2), (200, 4))                          # ef, result slots per lane: DEEP, DEEP, PIPE


def _strict_search(native, knob, capfd, h, Q, ef, slots, what):
    """the strict device call; asserts from the launch lines that the one-query strict kernel with `slots` slots per lane ran"""
    h.set_strict_ties(True)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    try:
        res = _device_search(native, h, Q, K, ef)
    finally:
        lines = [ln for ln in _launch_lines(capfd) if "visited set" in ln]
        knob("HNSWGPU_TRACE_LAUNCH", None)
    assert lines and "strict 1," in lines[0] and f"slots {slots}," in lines[0], (what, lines)
    assert all("strict 1," in ln and f"slots {slots}," in ln for ln in lines if "bitmap" not in ln), (what, lines)
    return res


@pytest.mark.parametrize("d", [130, 161, 200, 250, 300])
@pytest.mark.parametrize("dist", ["DistL2", "DistCosine"])
def test_search_at_uncovered_row_lengths(native, oracle, tmp_path, knob, capfd, dist, d):
    """strides 160, 192, 224, 256 and 320 (DistCosine: the norm inside the row at all five): ids, distance bits, counts, layers,
    ranks and the per-query work counters of a strict search are the oracle's, at 1, 2 (DEEP) and 4 (PIPE) slots per lane"""
    X, o, h = build_pair(native, oracle, tmp_path, N, d, M, EFC, dist, seed=900 + d)
    Q = uniform(NQ, d, 17)
    for ef, slots in EFS:
        what = f"{dist} d {d} ef {ef}"
        ref = o.parallel_search(Q, K, ef, want_counters="per_query")
        res = _strict_search(native, knob, capfd, h, Q, ef, slots, what)
        assert_same(res, ref)
        assert_same_counters(res.st, ref, what)


@pytest.mark.parametrize("d", [161, 250])
@pytest.mark.parametrize("dist", ["DistL2", "DistCosine"])
def test_search_at_uncovered_row_lengths_half_rows(native, oracle, tmp_path, knob, capfd, dist, d):
    """the same calls on data rounded to binary16, at F32 and at F16: both the oracle's, and F16 == F32 bit for bit"""
    X = native.round_to_f16(uniform(N, d, 950 + d))
    o, h = _pair(native, oracle, tmp_path, X, M, EFC, dist, "h")
    Q = uniform(NQ, d, 18)
    for ef, slots in EFS:
        ref = o.parallel_search(Q, K, ef, want_counters="per_query")
        got = {}
        for storage in ("f32", "f16"):
            h.set_storage(storage)
            h.upload(0)
            what = f"{dist} d {d} ef {ef} {storage}"
            got[storage] = _strict_search(native, knob, capfd, h, Q, ef, slots, what)
            assert_same(got[storage], ref)
            assert_same_counters(got[storage].st, ref, what)
        _same_bits(got["f16"], got["f32"], f"{dist} d {d} ef {ef}")
