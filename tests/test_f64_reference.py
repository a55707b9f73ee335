"""The float64 reference (tests/f64_reference.py) on the CPU: its bound is sound -- the oracle's scalar and SIMD-order f32
evaluations lie within it on a hostile sweep -- and it has teeth -- plausible wrong formulas are rejected on the same sweep.
Then the exhaustive-search helper against the oracle: with ef >= n the reference's search_layer never evicts and never stops
early (src/hnsw.rs:981, :1028-1052), so its answer is the exact k-NN of the layer-0 set its entry reaches.  These checks
share no code with oracle/ or the kernels; they must hold before a GPU is asked the same questions
(tests/test_gpu_f64_reference.py)."""
import numpy as np
import pytest

import f64_reference as F
from conftest import normalized, probability, uniform

METRICS = F.METRICS


def _oracle_safe(metric, Q, R, simd8):
    """where the oracle's dist_matrix may be called: the crate's asserts (DistCosine 1 - cos >= -2e-5, DistHellinger
    1 - sum >= -1e-6) throw, and a throw cannot cross the C ABI.  Decided from the f64 bound, so no call can trip them."""
    an = F.analyse(metric, Q[:, None, :], R[None, :, :], simd8)
    safe = np.isfinite(an.err)
    if metric == "DistCosine" and not simd8:
        a, b = np.broadcast_arrays(Q[:, None, :].astype(np.float64), R[None, :, :].astype(np.float64))
        s1, s2 = (a * a).sum(-1), (b * b).sum(-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            c = (a * b).sum(-1) / np.sqrt(s1 * s2)
        safe &= (s1 == 0) | (s2 == 0) | (1 - c - an.err >= -1.5e-5)
    if metric == "DistHellinger":
        s = (np.sqrt(Q[:, None, :].astype(np.float64)) * np.sqrt(R[None, :, :].astype(np.float64))).sum(-1)
        safe &= s * (1 + F.gamma(Q.shape[1] + 6)) + Q.shape[1] * F.TINY <= 1 + 0.9e-6
    return an, safe


def _oracle_matrix(oracle, metric, Q, R, safe, simd8):
    got = np.full((len(Q), len(R)), np.nan, np.float32)
    for i in range(len(Q)):
        cols = np.nonzero(safe[i])[0]
        if cols.size:
            got[i, cols] = oracle.dist_matrix(metric, Q[i:i + 1], R[cols], simd8=simd8)[0]
    return got


def _sweep(oracle, metric, simd8, dims=F.SWEEP_D):
    for d in dims:
        Q, R = F.hostile_sweep(metric, d, 7, simd8)
        an, safe = _oracle_safe(metric, Q, R, simd8)
        yield d, Q, R, an, safe, _oracle_matrix(oracle, metric, Q, R, safe, simd8)


@pytest.mark.parametrize("metric,simd8", [(m, False) for m in METRICS] + [(m, True) for m in ("DistL2", "DistL1", "DistDot", "DistCosine")])
def test_oracle_lies_within_the_bound_on_the_hostile_sweep(oracle, metric, simd8):
    """Soundness: both of the oracle's summation orders (the probability distances have one) within the bound everywhere the
    bound is finite; +inf where an L2 sum must overflow; and the bound is finite almost everywhere."""
    pairs = bounded = overflows = 0
    fails = []
    for d, Q, R, an, safe, got in _sweep(oracle, metric, simd8):
        bad = F.violations(an, got) & safe
        fails += [f"d {d}: " + m for m in F.describe(metric, an, got, bad)]
        pairs += an.err.size
        bounded += int(safe.sum())
        overflows += int((an.must_inf & safe).sum())
    assert not fails, fails[:8]
    assert bounded > 0.9 * pairs, f"{metric}: only {bounded} of {pairs} pairs checked"
    if metric == "DistL2":
        assert overflows > 100, f"{metric}: the sweep holds only {overflows} sums that must overflow"


def test_bound_is_tight_enough_to_matter(oracle):
    """the bound is a few ulps of the sum's magnitude, not a blanket tolerance: L2 of d = 128 uniform vectors within ~1e-5"""
    X = uniform(64, 128, 3)
    an = F.analyse("DistL2", X[:8, None, :], X[None, :, :])
    rel = an.err / np.maximum(an.truth, 1e-30)
    assert np.median(rel[an.truth > 0]) < 2e-5
    assert F.bound("DistL2", X[0], X[1]) == pytest.approx(float(an.err[0, 1]))


# ------------------------------------------------------------------------------------------------------------ teeth
def _mutants(metric, Q, R):
    """plausible wrong formulas, computed in numpy (f64, then rounded to f32): name -> matrix over (Q, R)"""
    a, b = np.broadcast_arrays(Q[:, None, :].astype(np.float64), R[None, :, :].astype(np.float64))
    out = {}
    with np.errstate(all="ignore"):
        if metric == "DistL2":
            out["L2 without sqrt"] = ((a - b) ** 2).sum(-1)
            out["L2 dropping the last coordinate"] = np.sqrt(((a - b)[..., :-1] ** 2).sum(-1))
        if metric == "DistL1":
            out["L1 dropping the first coordinate"] = np.abs(a - b)[..., 1:].sum(-1)
        if metric == "DistDot":
            s = (a * b).sum(-1)
            out["Dot without the clamp"] = 1 - s
            out["Dot without 1 -"] = np.maximum(s, 0)
        if metric == "DistCosine":
            s0, s1 = (a * b).sum(-1), (a * a).sum(-1)
            s2w = np.roll((R.astype(np.float64) ** 2).sum(-1), 1)[None, :]     # the norm of the neighbouring row
            out["Cosine with the norm of the wrong row"] = np.where((s1 > 0) & (s2w > 0), np.maximum(1 - s0 / np.sqrt(s1 * s2w), 0), 0)
        if metric == "DistHellinger":
            out["Hellinger without sqrt"] = np.maximum(1 - (np.sqrt(a) * np.sqrt(b)).sum(-1), 0)
        if metric == "DistJensenShannon":
            m = 0.5 * (a + b)
            t = np.where(a > 0, a * np.log(a / m), 0) + np.where(b > 0, b * np.log(b / m), 0)
            out["JS without 1/2"] = np.sqrt(np.maximum(t.sum(-1), 0))
            out["JS without sqrt"] = 0.5 * t.sum(-1)
        if metric == "DistJeffreys":
            am, bm = np.maximum(a, F.M_MIN), np.maximum(b, F.M_MIN)
            out["Jeffreys with log2"] = ((a - b) * np.log2(am / bm)).sum(-1)
    out[f"{metric} with the coordinates shifted by one"] = F.analyse(metric, Q[:, None, :], np.roll(R, 1, axis=1)[None, :, :]).truth
    with np.errstate(over="ignore"):
        return {k: v.astype(np.float32) for k, v in out.items()}


@pytest.mark.parametrize("metric", METRICS)
def test_wrong_formulas_are_rejected_on_the_sweep(metric):
    """Teeth: every mutation is rejected somewhere on the sweep (while the true formula, rounded to f32, never is)."""
    rejected = {}
    for d in F.SWEEP_D:
        Q, R = F.hostile_sweep(metric, d, 7)
        an = F.analyse(metric, Q[:, None, :], R[None, :, :])
        assert not (F.violations(an, an.truth.astype(np.float32)) & ~an.must_inf).any(), (metric, d)
        for name, got in _mutants(metric, Q, R).items():
            rejected[name] = rejected.get(name, 0) + int(F.violations(an, got).sum())
    print({k: v for k, v in rejected.items()})
    assert rejected and all(v > 0 for v in rejected.values()), rejected


# ------------------------------------------------------------------------------------------------------ exhaustive search
def _index(native, oracle, tmp_path, metric, n, d, m, seed, tag):
    """an oracle-built index on which every layer-0 entry reaches the same set: the first of a fixed run of seeds (the oracle's
    construction is deterministic, so this picks the same seed every time)"""
    gen = {"DistDot": normalized}.get(metric, probability if metric in F.PROBABILITY_METRICS else uniform)
    for s in range(seed, seed + 20):
        X = gen(n, d, s)
        o = oracle.OracleHnsw(m, n, 16, 60, metric)
        o.insert_batch(X)
        o.file_dump(tmp_path, tag)
        h = native.HnswIo(tmp_path, tag).load_hnsw(metric)
        reach = F.common_reachable_set(h)
        if reach is not None:
            return X, o, h, reach, gen
    raise AssertionError(f"{metric} n {n} M {m}: no seed in {seed}..{seed + 19} whose layer-0 entries reach one set")


@pytest.mark.parametrize("metric", METRICS)
def test_oracle_exhaustive_search_is_the_exact_knn(native, oracle, tmp_path, metric):
    """ef >= n: the oracle's parallel_search equals the f64 k-NN of the reachable layer-0 set (tie-tolerant), for k <= n < ef
    and for k > ef; and search_filter equals the k-NN of reachable & allowed, panicking queries aside."""
    n, d = 150, 12
    X, o, h, reach, gen = _index(native, oracle, tmp_path, metric, n, d, 16, 17, "ex")
    assert len(reach) > 0.9 * n
    Q = gen(40, d, 18)
    Q[:5] = X[:5]                                              # queries that ARE points
    for k, ef in ((10, 160), (150, 150), (200, 10)):          # ef = max(ef, k) >= n throughout
        r = o.parallel_search(Q, k, ef)
        fails = F.check_exact_knn(metric, X, Q, r.ids, r.dists, r.counts, k, reach)
        assert not fails, (k, ef, fails[:4])
    rng = np.random.default_rng(19)
    panics = 0
    for frac in (0.05, 0.3, 0.8):
        allowed = np.sort(rng.choice(n, max(1, int(frac * n)), replace=False)).astype(np.uint64)
        r = o.parallel_search_filter(Q, 10, 160, allowed)
        ok = r.status == 0
        panics += int((~ok).sum())
        members = reach & set(allowed.tolist())
        fails = F.check_exact_knn(metric, X, Q[ok], r.ids[ok], r.dists[ok], r.counts[ok], 10, members)
        assert not fails, (frac, fails[:4])
    assert panics < len(Q)


def test_the_check_catches_a_wrong_answer(native, oracle, tmp_path):
    """the exhaustive comparison rejects a dropped neighbour, a wrong distance and an answer out of order"""
    n, d = 150, 12
    X, o, h, reach, gen = _index(native, oracle, tmp_path, "DistL2", n, d, 16, 17, "bad")
    Q = gen(10, d, 18)
    r = o.parallel_search(Q, 10, 160)
    assert not F.check_exact_knn("DistL2", X, Q, r.ids, r.dists, r.counts, 10, reach)
    ids, dists = r.ids.copy(), r.dists.copy()
    ids[0, 3] = F.exact_knn("DistL2", X, Q[0], 40, reach)[0][30]     # the 31st neighbour instead of the 4th
    assert F.check_exact_knn("DistL2", X, Q, ids, dists, r.counts, 10, reach)
    dists = r.dists.copy()
    dists[1, 2] = np.nextafter(np.nextafter(dists[1, 2], np.float32(9), dtype=np.float32), np.float32(9), dtype=np.float32) * np.float32(1.001)
    assert F.check_exact_knn("DistL2", X, Q, r.ids, dists, r.counts, 10, reach)
    ids, dists = r.ids.copy(), r.dists.copy()
    ids[2, [0, 9]], dists[2, [0, 9]] = ids[2, [9, 0]], dists[2, [9, 0]]
    assert F.check_exact_knn("DistL2", X, Q, ids, dists, r.counts, 10, reach)


def test_reachability_sees_a_cut_graph(native, oracle, tmp_path):
    """two clusters far apart with M = 2: the layer-0 entries need not reach one set; the helper reports each entry's own set"""
    rng = np.random.default_rng(5)
    X = np.concatenate([rng.random((60, 4)), rng.random((60, 4)) + 1000]).astype(np.float32)
    o = oracle.OracleHnsw(2, 120, 16, 10, "DistL2")
    o.insert_batch(X)
    o.file_dump(tmp_path, "cut")
    h = native.HnswIo(tmp_path, "cut").load_hnsw("DistL2")
    reach = F.GraphWalk(h).layer0_reachability()
    assert all(len(s) >= 1 for s in reach.values())
    assert max(len(s) for s in reach.values()) <= 120


def test_graph_check_on_oracle_and_host_builds(native, oracle, tmp_path):
    """the graph check passes on the oracle's serial graph and on the host builder's parallel one, and rejects stored distances
    that do not belong to the vectors"""
    n, m = 2000, 12
    X = uniform(n, 16, 31)
    o = oracle.OracleHnsw(m, n, 16, 100, "DistL2")
    o.insert_batch(X)
    o.file_dump(tmp_path, "g")
    for h in (native.HnswIo(tmp_path, "g").load_hnsw("DistL2"), native.Hnsw(m, n, 16, 100, "DistL2")):
        if h.get_nb_point() == 0:
            h.set_build_options(nthreads=4)
            h.parallel_insert(X)
        stats = {}
        assert not F.check_graph(h, X, "DistL2", m, oracle.levels(m, n), stats=stats)
        assert stats["owners_named"] == n and len(stats["former_entry_points"]) <= h.get_max_level_observed()
    Xb = X.copy()
    Xb[7] *= np.float32(1.0001)
    assert F.check_graph(h, Xb, "DistL2", m, oracle.levels(m, n))
