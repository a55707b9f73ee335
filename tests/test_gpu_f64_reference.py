"""The device against the float64 reference (tests/f64_reference.py), which shares no code and no recollection with oracle/:
the distance routine on the hostile sweep, exhaustive searches (ef >= n) against the exact k-NN in f64 on every path of the
search, and the GPU-assisted builder's neighbour lists.  The bit-exact oracle comparisons elsewhere stay as they are; these
checks catch what the kernels and the oracle could get wrong together (a formula, a convention) above the last bit."""
import numpy as np
import pytest

import f64_reference as F
from conftest import normalized, probability, uniform
from test_gpu_counters import _launch_lines
from test_gpu_parity import _tie_heavy

pytestmark = pytest.mark.gpu

ALL_BATCHES_D = (1, 3, 8, 25, 31, 32, 33, 64, 100, 128, 200, 784, 800)


# ------------------------------------------------------------------------------------------------------- distance routine
@pytest.mark.parametrize("metric,arith", [(m, "scalar") for m in F.METRICS] + [(m, "simd8") for m in ("DistL2", "DistL1", "DistDot", "DistCosine")])
def test_distance_routine_within_the_f64_bound(native, metric, arith):
    """eval_distance_matrix (the search kernel's own routine) on the hostile sweep, rows in batches of 1, 16, 17, 32, 33 and 64
    (the lane-group branches), and eval_distances on the matched pairs: every result within the bound of the f64 truth, +inf
    where an L2 sum must overflow.  DistCosine runs d = 25 (norm in the row's padding) and d = 32 (separate norm array) too."""
    simd8 = arith == "simd8"
    fails, checked, overflows = [], 0, 0
    for d in F.SWEEP_D:
        Q, R = F.hostile_sweep(metric, d, 7, simd8)
        an = F.analyse(metric, Q[:, None, :], R[None, :, :], simd8)
        for nf in ((1, 16, 17, 32, 33, 64) if d in ALL_BATCHES_D else (17, 64)):
            got = native.eval_distance_matrix(metric, Q, R, nf, arithmetic=arith)
            bad = F.violations(an, got)
            fails += [f"d {d} batch {nf}: " + m for m in F.describe(metric, an, got, bad)]
        checked += int(np.isfinite(an.err).sum())
        overflows += int(an.must_inf.sum())
        if not simd8:
            pa, pb = np.repeat(Q, 17, 0)[:64], R[:64]
            pan = F.analyse(metric, pa, pb)
            got = native.eval_distances(metric, pa, pb)
            fails += [f"d {d} eval_distances: " + m for m in F.describe(metric, pan, got, F.violations(pan, got))]
        assert len(fails) < 8, fails
    assert not fails, fails
    assert checked > 0.9 * len(F.SWEEP_D) * 4 * 70
    if metric == "DistL2":
        assert overflows > 100


# ------------------------------------------------------------------------------------------------------- exhaustive search
def _gen(metric):
    return {"DistDot": normalized}.get(metric, probability if metric in F.PROBABILITY_METRICS else uniform)


def _exhaustive_index(native, oracle, tmp_path, metric, n, d, m, seed, efc=100, product=False, data=None):
    """an index (oracle-built and reloaded, or product-built) on which every layer-0 entry reaches one set: the first of a fixed
    run of seeds.  Returns (X, h uploaded to device 0, the reachable set)."""
    for s in range(seed, seed + 20):
        X = data(n, d, s) if data is not None else _gen(metric)(n, d, s)
        if product:
            h = native.Hnsw(m, n, 16, efc, metric)
            h.set_build_options(nthreads=1)
            h.parallel_insert(X)
        else:
            o = oracle.OracleHnsw(m, n, 16, efc, metric)
            o.insert_batch(X)
            o.file_dump(tmp_path, f"x{s}")
            h = native.HnswIo(tmp_path, f"x{s}").load_hnsw(metric)
        reach = F.common_reachable_set(h)
        if reach is not None:
            h.upload(0)
            return X, h, reach
    raise AssertionError(f"{metric} n {n} M {m}: no seed in {seed}..{seed + 19} whose layer-0 entries reach one set")


def _search_traced(native, knob, capfd, h, Q, k, ef, allowed=None):
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    try:
        res = h.parallel_search_flat(Q, k, ef) if allowed is None else h.parallel_search_filter_flat(Q, k, ef, allowed)
    finally:
        knob("HNSWGPU_TRACE_LAUNCH", None)
    return res, _launch_lines(capfd)


def _assert_exact(metric, X, Q, res, k, members, what, simd8=False):
    fails = F.check_exact_knn(metric, X, Q, res.ids, res.dists, res.counts, k, members, simd8)
    assert not fails, (what, fails[:4])


@pytest.mark.parametrize("n,d,m,ef,slots", [(60, 8, 16, 64, 1), (120, 8, 16, 128, 2), (250, 16, 24, 256, 4), (500, 16, 32, 512, 16)])
@pytest.mark.parametrize("product", [False, True], ids=["oracle_built", "product_built"])
def test_exhaustive_search_at_every_result_set_shape(native, oracle, tmp_path, knob, capfd, n, d, m, ef, slots, product):
    """ef >= n: the device's answers are the exact f64 k-NN of the reachable layer-0 set, with 1, 2, 4 and 16 result slots per lane
    (k <= n < ef), and with k > ef (ef = max(ef, k) >= n)"""
    X, h, reach = _exhaustive_index(native, oracle, tmp_path, "DistL2", n, d, m, 3, product=product)
    Q = uniform(200, d, 4)
    Q[:10] = X[:10]
    res, lines = _search_traced(native, knob, capfd, h, Q, 10, ef)
    assert any(f"slots {slots}," in ln for ln in lines), lines
    _assert_exact("DistL2", X, Q, res, 10, reach, f"slots {slots}")
    res = h.parallel_search_flat(Q, n + 5, 8)                  # k > ef, k > n
    _assert_exact("DistL2", X, Q, res, n + 5, reach, "k > ef")


def test_exhaustive_search_in_the_literal_heap_kernel(native, oracle, tmp_path, knob, capfd):
    X, h, reach = _exhaustive_index(native, oracle, tmp_path, "DistL2", 500, 16, 32, 3)
    Q = uniform(60, 16, 5)
    res, lines = _search_traced(native, knob, capfd, h, Q, 10, 1100)
    assert lines and all("literal kernel" in ln for ln in lines), lines
    _assert_exact("DistL2", X, Q, res, 10, reach, "ef 1100")


@pytest.mark.parametrize("metric,d", [("DistL2", 12), ("DistL1", 12), ("DistDot", 12), ("DistCosine", 25), ("DistCosine", 32),
                                      ("DistHellinger", 12), ("DistJeffreys", 12), ("DistJensenShannon", 12)])
def test_exhaustive_search_for_every_metric(native, oracle, tmp_path, knob, capfd, metric, d):
    """every metric, strict and lean (set_strict_ties(False): lean answers may differ from the reference only where distances tie,
    so they too are the exact k-NN modulo ties); k <= n < ef and k > ef"""
    X, h, reach = _exhaustive_index(native, oracle, tmp_path, metric, 150, d, 16, 3)
    Q = _gen(metric)(100, d, 6)
    Q[:10] = X[20:30]
    res, lines = _search_traced(native, knob, capfd, h, Q, 10, 160)
    assert any("strict 1" in ln for ln in lines), lines
    _assert_exact(metric, X, Q, res, 10, reach, metric)
    _assert_exact(metric, X, Q, h.parallel_search_flat(Q, 170, 10), 170, reach, metric + " k > ef")
    h.set_strict_ties(False)
    try:
        res, lines = _search_traced(native, knob, capfd, h, Q, 10, 160)
    finally:
        h.set_strict_ties(True)
    assert any("strict 0" in ln for ln in lines), lines
    _assert_exact(metric, X, Q, res, 10, reach, metric + " lean")


@pytest.mark.parametrize("kind", ["grid", "duplicates"])
def test_exhaustive_search_under_ties_strict_and_lean(native, oracle, tmp_path, kind):
    """equal distances everywhere: strict (the literal replay) and lean answers both equal the f64 k-NN modulo ties"""
    m = 16 if kind == "grid" else 32                           # (duplicates cut small graphs apart: M = 32 keeps one reachable set)
    X, h, reach = _exhaustive_index(native, oracle, tmp_path, "DistL2", 120, 6, m, 3, data=lambda n, d, s: _tie_heavy(kind, n, d, s))
    Q = _tie_heavy(kind, 100, 6, 8)
    _assert_exact("DistL2", X, Q, h.parallel_search_flat(Q, 10, 128), 10, reach, kind)
    h.set_strict_ties(False)
    try:
        _assert_exact("DistL2", X, Q, h.parallel_search_flat(Q, 10, 128), 10, reach, kind + " lean")
    finally:
        h.set_strict_ties(True)


@pytest.mark.parametrize("metric,d", [("DistL2", 16), ("DistCosine", 25), ("DistJensenShannon", 12)])
def test_exhaustive_filtered_search(native, oracle, tmp_path, knob, capfd, metric, d):
    """search_filter with ef >= n: the answer is the f64 k-NN of reachable & allowed, for several allowed fractions (queries on
    which the reference panics, status 1, aside)"""
    X, h, reach = _exhaustive_index(native, oracle, tmp_path, metric, 250, d, 24, 3)
    n = len(X)
    Q = _gen(metric)(120, d, 9)
    rng = np.random.default_rng(10)
    answered = 0
    for frac in (0.02, 0.1, 0.5, 0.9):
        allowed = np.sort(rng.choice(n, max(1, int(frac * n)), replace=False)).astype(np.uint64)
        res, lines = _search_traced(native, knob, capfd, h, Q, 10, 256, allowed)
        assert lines, "no launch traced"
        ok = res.status == 0
        answered += int(ok.sum())
        sub = type(res)(res.ids[ok], res.dists[ok], res.layers[ok], res.ranks[ok], res.counts[ok])
        _assert_exact(metric, X, Q[ok], sub, 10, reach & set(allowed.tolist()), f"{metric} allowed {frac}")
    assert answered > 2 * len(Q)


@pytest.mark.parametrize("metric,d", [("DistL2", 8), ("DistCosine", 32)])
def test_exhaustive_search_through_the_pair_pass(native, oracle, tmp_path, knob, capfd, metric, d):
    """HNSWGPU_PAIR_SEARCH=1, 600 queries (the pass needs >= 512): two queries per wavefront.  On 120 points the id bits are too
    few for the default table size (search_device.hip: idbits - (tb - 3) >= 1), so the table is shrunk by
    HNSWGPU_PAIR_TBITS_DELTA."""
    X, h, reach = _exhaustive_index(native, oracle, tmp_path, metric, 120, d, 16, 3)
    Q = _gen(metric)(600, d, 11)
    knob("HNSWGPU_PAIR_SEARCH", "1")
    knob("HNSWGPU_PAIR_TBITS_DELTA", "-20")
    try:
        res, lines = _search_traced(native, knob, capfd, h, Q, 10, 128)
    finally:
        knob("HNSWGPU_PAIR_SEARCH", None)
        knob("HNSWGPU_PAIR_TBITS_DELTA", None)
    assert any("pair pass" in ln for ln in lines), lines
    _assert_exact(metric, X, Q, res, 10, reach, "pair pass")


@pytest.mark.parametrize("m", [40, 100])
def test_exhaustive_search_on_rows_of_more_than_64_ids(native, oracle, tmp_path, knob, capfd, m):
    X, h, reach = _exhaustive_index(native, oracle, tmp_path, "DistL2", 250, 16, m, 1)
    Q = uniform(150, 16, 12)
    res, lines = _search_traced(native, knob, capfd, h, Q, 10, 256)
    assert any("slots 16," in ln for ln in lines), lines      # 2M > 64 ids per row: 16 slots forced
    _assert_exact("DistL2", X, Q, res, 10, reach, f"M {m}")


def test_exhaustive_search_with_both_descent_kernels(native, oracle, tmp_path, knob):
    X, h, reach = _exhaustive_index(native, oracle, tmp_path, "DistL2", 250, 16, 24, 3)
    assert h.get_max_level_observed() >= 1
    Q = uniform(301, 16, 13)                                   # odd: the last wavefront of the pair descent holds one query
    _assert_exact("DistL2", X, Q, h.parallel_search_flat(Q, 10, 256), 10, reach, "pair descent")
    knob("HNSWGPU_NO_PAIR_DESCENT", "1")
    try:
        _assert_exact("DistL2", X, Q, h.parallel_search_flat(Q, 10, 256), 10, reach, "single descent")
    finally:
        knob("HNSWGPU_NO_PAIR_DESCENT", None)


@pytest.mark.parametrize("metric,d", [("DistL2", 37), ("DistL1", 37), ("DistDot", 37), ("DistCosine", 37)])
def test_exhaustive_search_in_simd8_arithmetic(native, oracle, tmp_path, metric, d):
    X, h, reach = _exhaustive_index(native, oracle, tmp_path, metric, 150, d, 16, 3)
    Q = _gen(metric)(100, d, 14)
    h.set_arithmetic("simd8")
    try:
        res = h.parallel_search_flat(Q, 10, 160)
    finally:
        h.set_arithmetic("scalar")
    _assert_exact(metric, X, Q, res, 10, reach, metric + " simd8", simd8=True)
    scalar = h.parallel_search_flat(Q, 10, 160)
    if metric != "DistL1":                                     # the path ran: other distance bits somewhere
        assert not np.array_equal(scalar.dists.view(np.uint32), res.dists.view(np.uint32))


# ------------------------------------------------------------------------------------------------------- the builder's graph
@pytest.mark.parametrize("name,n,opts", [
    ("gpu windows", 20_000, dict(nthreads=8, gpu_device=0, gpu_window=4096)),
    ("gpu window 1", 1500, dict(nthreads=1, gpu_device=0, gpu_window=1)),
    ("host", 20_000, dict(nthreads=8)),
])
def test_builder_graph_against_f64(native, oracle, name, n, opts):
    """Every list of every layer of a built graph (GPU-assisted with windows of many points and several host threads, as in
    test_gpu_round2's window test at a smaller n; one point per window and the host builder as controls): stored distances within
    the bound of the f64 distance between owner and neighbour, no owner in its own list and no duplicate p_id
    (src/hnsw.rs:1258-1266), at most M ids (2M at layer 0), every neighbour of a layer-l list on layer >= l, distances
    non-decreasing (src/hnsw.rs:1280)."""
    from test_gpu_round2 import _clustered
    m, d = 16, 32
    X = _clustered(n, d, 7)
    h = native.Hnsw(m, n, 16, 200, "DistL2")
    h.set_build_options(fast_arithmetic=False, **opts)
    h.parallel_insert(X)
    assert h.get_nb_point() == n
    stats = {}
    fails = F.check_graph(h, X, "DistL2", m, oracle.levels(m, n), stats=stats)
    assert not fails, (name, fails[:6])
    assert stats["edges"] > n * m // 2 and stats["owners_named"] == n, stats


@pytest.mark.parametrize("metric,d,data", [("DistCosine", 25, "uniform"), ("DistCosine", 32, "uniform"), ("DistDot", 16, "normalized"),
                                           ("DistJensenShannon", 12, "probability")])
def test_builder_graph_against_f64_other_metrics(native, oracle, metric, d, data):
    """The same check of the multi-threaded, large-window GPU-assisted build beyond DistL2: DistCosine with the norm in the row's
    padding (d = 25) and in an array beside the row (d = 32), DistDot on normalized rows, DistJensenShannon on probability vectors.
    That path cannot be compared bit for bit (the host threads link a window's points in no fixed order); one thread and real
    windows are compared byte for byte in tests/test_gpu_build_windows.py."""
    n, m = 5000, 16
    X = {"uniform": uniform, "normalized": normalized, "probability": probability}[data](n, d, 7)
    h = native.Hnsw(m, n, 16, 200, metric)
    h.set_build_options(fast_arithmetic=False, nthreads=8, gpu_device=0, gpu_window=4096)
    h.parallel_insert(X)
    assert h.get_nb_point() == n
    stats = {}
    fails = F.check_graph(h, X, metric, m, oracle.levels(m, n), stats=stats)
    assert not fails, (metric, d, fails[:6])
    assert stats["edges"] > n * m // 2 and stats["owners_named"] == n, stats
