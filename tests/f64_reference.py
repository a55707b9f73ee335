"""A plain float64 reference of the seven distances, a rigorous bound on how far an f32 evaluation may lie from it, exact k-NN
in float64, and layer-0 reachability of a dumped graph.

TEST INFRASTRUCTURE ONLY.  This module shares no code and no recollection with `oracle/` or the kernels: every distance is
computed from its mathematical definition on the f32 inputs widened to f64.  The few rules that come from the crate and not
from the mathematics are listed in CONVENTIONS; they are the only part this check takes on trust.

The bound (`analyse`, `bound`) holds for ANY summation order -- the scalar left-to-right order and the 8-lane SIMD order alike
-- so it checks the quantity, not the last bit: a kernel and an oracle that share one wrong formula both fail it.
"""
import collections

import numpy as np

# ----------------------------------------------------------------------------------------------------- conventions
# Rules of the crate (anndists 0.1, as restated in oracle/PIN.md) that the mathematics alone does not fix.  Each one is
# applied below, by name, and nowhere else may the reference bend towards the product.
CONVENTIONS = (
    ("cosine_zero_vector", "DistCosine of a zero vector is 0 (the crate returns 0 unless both norms are > 0; oracle/PIN.md)."),
    ("jeffreys_m_min", "DistJeffreys takes max(x, M_MIN) with M_MIN = 1e-30 (as f32) for both coordinates before the ratio; "
                       "a zero coordinate is thereby finite (oracle/PIN.md)."),
    ("jensenshannon_zero_terms", "DistJensenShannon skips the term a*ln(a/m) where a == 0 (and likewise for b): the limit "
                                 "0*ln 0 = 0 of the mathematics, written as a skip in the crate (oracle/PIN.md)."),
    ("dot_and_hellinger_clamp", "DistDot is max(1 - sum a*b, 0) and DistHellinger sqrt(max(1 - sum sqrt(a)sqrt(b), 0)): the "
                                "clamp at 0 is the crate's; it is 1-Lipschitz and adds nothing to the bound (oracle/PIN.md)."),
)
M_MIN = float(np.float32(1.0e-30))          # the crate's constant is an f32

METRICS = ("DistL2", "DistL1", "DistDot", "DistCosine", "DistHellinger", "DistJeffreys", "DistJensenShannon")
PROBABILITY_METRICS = ("DistHellinger", "DistJeffreys", "DistJensenShannon")

# ----------------------------------------------------------------------------------------------------- error model
U = 2.0 ** -24                  # unit roundoff of f32 (round to nearest)
U_EFF = U + 2.0 ** -40          # the same, with room for the f64 evaluation of the truth itself (d <= 8000)
TINY = 2.0 ** -149              # an underflowing f32 operation is off by at most TINY / 2 (absolute)
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN_NORMAL = 2.0 ** -126


def gamma(n):
    """gamma_n = n u / (1 - n u): the relative error of n rounded operations in a row (Higham, Accuracy and Stability, 3.1)"""
    return n * U_EFF / (1.0 - n * U_EFF)


def _sqrt_err(y, e):
    """|fl(sqrt(y_hat)) - sqrt(y)| for y >= 0 and |y_hat - y| <= e: |sqrt(x) - sqrt(y)| = |x - y| / (sqrt(x) + sqrt(y)), which
    is <= sqrt(|x - y|) and <= |x - y| / sqrt(y); plus the rounding of the sqrt.  The sqrt(e) branch keeps values near 0 honest."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lin = np.where(y > 0, e / np.sqrt(np.where(y > 0, y, 1.0)), np.inf)
    return np.minimum(np.sqrt(e), lin) + U_EFF * np.sqrt(y + e)


Analysis = collections.namedtuple("Analysis", "truth err must_inf may_inf may_nan")
"""Per pair: truth = the distance in f64; err = the bound on |f32 result - truth| (np.inf: no bound can be given, the pair is
not checked); must_inf = the f32 result must be +inf; may_inf = +inf is admissible; may_nan = NaN is admissible (the sqrt of a
sum that may round below 0)."""


def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, "the reference takes the f32 inputs the product sees"
    return a.astype(np.float64)


def analyse(metric, a, b, simd8=False):
    """The f64 truth and the bound of every pair (a[..., :], b[..., :]) (broadcast; the last axis is the dimension).

    simd8 matters for DistCosine only: the crate's SIMD build sums the three products in f32 and finishes in f32, the scalar
    build sums f32 products in f64.  Every other bound holds for any summation order."""
    a, b = np.broadcast_arrays(_f64(a), _f64(b))
    d = a.shape[-1]
    shape = a.shape[:-1]
    false = np.zeros(shape, bool)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if metric in ("DistL2", "DistL1"):
            t = a - b
            if metric == "DistL2":
                # fl(fl(a - b)^2): 2 roundings per term, then d - 1 additions in any order, all terms >= 0
                S = np.sum(t * t, -1)
                E = gamma(d + 3) * S + d * TINY
                truth, err = np.sqrt(S), _sqrt_err(S, E)
            else:
                S = np.sum(np.abs(t), -1)
                E = gamma(d + 1) * S + d * TINY
                truth, err = S, E
            # non-negative terms: no partial sum exceeds S + E; if even S - E is beyond FLT_MAX some operation overflowed
            return Analysis(truth, err, S - E > FLT_MAX, S + E >= FLT_MAX, false)
        if metric == "DistDot":
            p = a * b
            s, A = np.sum(p, -1), np.sum(np.abs(p), -1)
            E = gamma(d + 1) * A + d * TINY           # signed terms: gamma_d times the sum of their magnitudes
            truth = np.maximum(1.0 - s, 0.0)          # CONVENTIONS dot_and_hellinger_clamp
            err = E + U_EFF * (np.abs(1.0 - s) + E)   # the rounding of 1 - s
            err = np.where(A * (1 + gamma(d + 1)) < FLT_MAX, err, np.inf)  # a partial sum may overflow: no bound
            return Analysis(truth, err, false, false, false)
        if metric == "DistCosine":
            return _cosine(a, b, d, simd8)
        assert (a >= 0).all() and (b >= 0).all(), f"{metric} is defined on non-negative vectors"
        if metric == "DistHellinger":
            r = np.sqrt(a) * np.sqrt(b)
            s = np.sum(r, -1)
            E = gamma(d + 4) * s + d * TINY           # sqrt, sqrt, product, d - 1 additions; non-negative terms
            y = np.maximum(1.0 - s, 0.0)              # CONVENTIONS dot_and_hellinger_clamp
            Ey = E + U_EFF * (np.abs(1.0 - s) + E)
            return Analysis(np.sqrt(y), _sqrt_err(y, Ey), false, false, false)
        if metric == "DistJeffreys":
            am, bm = np.maximum(a, M_MIN), np.maximum(b, M_MIN)    # CONVENTIONS jeffreys_m_min
            r = am / bm
            L = np.log(r)
            t = (a - b) * L                            # >= 0 term by term, also after rounding (the signs are exact)
            S = np.sum(t, -1)
            u1 = U_EFF / (1 - U_EFF)
            eps = u1 + 2 * U_EFF * (np.abs(L) + u1)    # the ratio's rounding through ln, then logf (< 1 ulp <= 2u|ln|)
            e = np.abs(a - b) * ((np.abs(L) + eps) * (1 + U_EFF) ** 2 - np.abs(L)) + TINY
            Esum = np.sum(e, -1)
            E = Esum + gamma(d + 1) * (S + Esum) + d * TINY
            ratio_ok = np.all((r < FLT_MAX / 2) & (r > 2.0 ** -125), -1)
            err = np.where(ratio_ok, E, np.inf)
            return Analysis(S, err, ratio_ok & (S - E > FLT_MAX), S + E >= FLT_MAX, false)
        if metric == "DistJensenShannon":
            m = 0.5 * (a + b)
            La = np.where(a > 0, np.log(np.where(a > 0, a, 1.0) / np.where(m > 0, m, 1.0)), 0.0)
            Lb = np.where(b > 0, np.log(np.where(b > 0, b, 1.0) / np.where(m > 0, m, 1.0)), 0.0)
            ta, tb = a * La, b * Lb                    # CONVENTIONS jensenshannon_zero_terms (a == 0: no term)
            s = np.sum(ta + tb, -1)
            A = np.sum(np.abs(ta) + np.abs(tb), -1)
            u1 = U_EFF / (1 - U_EFF)
            # the sum a + b and the ratio x / m: 2 roundings through ln (0.5 * is exact above the subnormal range), logf,
            # the product x * ln
            eps_a = 2.01 * u1 + 2 * U_EFF * (np.abs(La) + 2.01 * u1)
            eps_b = 2.01 * u1 + 2 * U_EFF * (np.abs(Lb) + 2.01 * u1)
            e = (np.where(a > 0, a * ((np.abs(La) + eps_a) * (1 + U_EFF) - np.abs(La)) + TINY, 0.0)
                 + np.where(b > 0, b * ((np.abs(Lb) + eps_b) * (1 + U_EFF) - np.abs(Lb)) + TINY, 0.0))
            # a mean in the subnormal range: 0.5 * (a + b) = 0.5 * k 2^-149 rounds to within a factor 3/2 for k >= 2, so ln is
            # off by < ln 1.5 (absolute, on terms below 2^-125); k = 1 rounds the mean to 0 and the term to inf: no bound
            sub = (a + b > 0) & (a + b < 2.0 ** -125)
            e = np.where(sub, (a + b) * (0.5 + 3 * U_EFF * (np.abs(La) + np.abs(Lb) + 1)) + 2 * TINY, e)
            Esum = np.sum(e, -1)
            E = Esum + gamma(2 * d) * (A + Esum) + 2 * d * TINY   # up to 2d signed terms
            y = 0.5 * s
            Ey = 0.5 * E + TINY
            ok = ~np.any(a + b == TINY, -1)
            err = np.where(ok, _sqrt_err(np.maximum(y, 0.0), Ey), np.inf)
            return Analysis(np.sqrt(np.maximum(y, 0.0)), err, false, false, y - Ey < 0)
    raise ValueError(metric)


def _cosine(a, b, d, simd8):
    p0, p1, p2 = a * b, a * a, b * b                   # exact in f64 (24 + 24 bits)
    s0, s1, s2 = np.sum(p0, -1), np.sum(p1, -1), np.sum(p2, -1)
    A0 = np.sum(np.abs(p0), -1)
    zero = (s1 == 0) | (s2 == 0)                       # CONVENTIONS cosine_zero_vector: every product is exactly 0 too
    big = np.maximum(np.max(p1, -1), np.max(p2, -1)) >= FLT_MAX   # an f32 product overflows
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        N = np.sqrt(s1 * s2)
        c = np.where(zero, 0.0, s0 / np.where(zero, 1.0, N))
        if not simd8:
            # f32 products (one rounding each) summed in f64 (d roundings of 2^-53 each), finished in f64, cast to f32
            e64 = (d + 8) * 2.0 ** -52
            e = U + e64
            E0 = e * A0 * (1 + U) + d * TINY
            s1lo, s1hi = s1 * (1 - e) - d * TINY, s1 * (1 + e) + d * TINY
            s2lo, s2hi = s2 * (1 - e) - d * TINY, s2 * (1 + e) + d * TINY
            Nlo, Nhi = np.sqrt(s1lo * s2lo), np.sqrt(s1hi * s2hi)
            Ec = E0 / Nlo + np.abs(s0) * np.maximum(1 / Nlo - 1 / N, 1 / N - 1 / Nhi) + e64 * (np.abs(c) + 1)
            err = Ec + U * (np.abs(1 - c) + Ec) + TINY + e64
            ok = (s1lo > 0) & (s2lo > 0)
        else:
            # the crate's SIMD build: three f32 sums, then s1 * s2, sqrt, the division and 1 - x, each rounded in f32
            g = gamma(d + 1)
            E0 = g * A0 + d * TINY
            s1lo, s1hi = s1 * (1 - g) - d * TINY, s1 * (1 + g) + d * TINY
            s2lo, s2hi = s2 * (1 - g) - d * TINY, s2 * (1 + g) + d * TINY
            Nlo = np.sqrt(s1lo * s2lo * (1 - U)) * (1 - U)
            Nhi = np.sqrt(s1hi * s2hi * (1 + U)) * (1 + U)
            Eq = E0 / Nlo + np.abs(s0) * np.maximum(1 / Nlo - 1 / N, 1 / N - 1 / Nhi)
            Eq = Eq + U * (np.abs(c) + Eq) + TINY
            err = Eq + U * (np.abs(1 - c) + Eq) + TINY
            ok = ((s1lo > 0) & (s2lo > 0) & (s1lo * s2lo >= FLT_MIN_NORMAL) & (s1hi * s2hi < FLT_MAX * (1 - U))
                  & (np.maximum(np.maximum(s1hi, s2hi), A0 * (1 + g)) < FLT_MAX))
    truth = np.where(zero, 0.0, np.maximum(1.0 - c, 0.0))
    err = np.where(zero, 0.0, np.where(ok & ~big, err, np.inf))
    false = np.zeros(truth.shape, bool)
    return Analysis(truth, err, false, false, false)


def truth(metric, a, b):
    """the distance in f64 from its definition"""
    return analyse(metric, a, b).truth


def bound(metric, a, b, simd8=False):
    """the bound on |f32 result - f64 truth| of one pair (np.inf where none can be given)"""
    return float(analyse(metric, np.asarray(a, np.float32), np.asarray(b, np.float32), simd8).err)


def violations(an, got):
    """Boolean mask: where the f32 results `got` contradict the analysis `an` (see Analysis)."""
    g = np.asarray(got, dtype=np.float32).astype(np.float64)
    bounded = np.isfinite(an.err)
    fin = np.isfinite(g)
    ok_val = fin & (np.abs(g - an.truth) <= an.err) & ~an.must_inf
    ok_inf = (g == np.inf) & (an.must_inf | an.may_inf)
    ok_nan = np.isnan(g) & an.may_nan
    return bounded & ~(ok_val | ok_inf | ok_nan)


def check_matrix(metric, Q, R, got, simd8=False):
    """violations of got[q, r] = d(Q[q], R[r]); returns (mask, analysis)"""
    an = analyse(metric, Q[:, None, :], R[None, :, :], simd8)
    return violations(an, got), an


def describe(metric, an, got, mask, limit=4):
    idx = np.argwhere(mask)[:limit]
    return [f"{metric} at {tuple(int(v) for v in i)}: got {float(np.asarray(got)[tuple(i)])!r} truth {an.truth[tuple(i)]!r} "
            f"bound {an.err[tuple(i)]!r}" for i in idx]


# ----------------------------------------------------------------------------------------------------- k-NN in float64
def _analyse_rows(metric, X, q, ids, simd8=False, chunk=4096):
    outs = [analyse(metric, q[None, :], X[ids[i:i + chunk]], simd8) for i in range(0, len(ids), chunk)]
    return Analysis(*[np.concatenate([getattr(o, f) for o in outs]) for f in Analysis._fields])


def check_per_answer(metric, X, Q, ids, dists, counts, simd8=False, chunk=512):
    """Every returned (id, dist): dist within the bound of the f64 d(q, X[id]); the ids of a row unique; the distances of a row
    non-decreasing.  Returns a list of failure strings (empty: all good).  It is nq * k f64 distances."""
    fails = []
    nq, k = ids.shape
    counts = np.asarray(counts).astype(np.int64)
    live = np.arange(k)[None, :] < counts[:, None]
    if ids[live].size and int(ids[live].max()) >= len(X):
        fails.append(f"an id beyond the {len(X)} points: {int(ids[live].max())}")
        return fails
    for s in range(0, nq, chunk):
        e = min(nq, s + chunk)
        I = np.where(live[s:e], ids[s:e], 0).astype(np.int64)
        an = analyse(metric, Q[s:e, None, :], X[I], simd8)
        bad = violations(an, dists[s:e]) & live[s:e]
        if bad.any():
            fails += [f"query {s + i[0]} slot {i[1]} id {int(I[tuple(i)])}: " + m.split(": ", 1)[1]
                      for i, m in zip(np.argwhere(bad)[:4], describe(metric, an, dists[s:e], bad))]
        lv = live[s:e]
        srt = np.sort(np.where(lv, ids[s:e].astype(np.int64), -1 - np.arange(k)[None, :]), 1)   # dead slots: distinct negatives
        for i in np.nonzero((srt[:, 1:] == srt[:, :-1]).any(1))[0][:4]:
            fails.append(f"query {s + i}: duplicate ids {ids[s + i, :counts[s + i]].tolist()}")
        dr = dists[s:e].astype(np.float64)
        down = (dr[:, 1:] < dr[:, :-1]) & lv[:, 1:]
        for i in np.nonzero(down.any(1))[0][:4]:
            fails.append(f"query {s + i}: distances not non-decreasing {dr[i, :counts[s + i]].tolist()}")
        if len(fails) > 8:
            break
    return fails


def check_exact_knn(metric, X, Q, ids, dists, counts, k, members, simd8=False):
    """The answers of an exhaustive search against the exact k-NN in f64 of the candidate set `members` (origin ids = rows of X),
    tie-tolerant: the count is min(k, |members|); ids are unique members; each distance lies within its bound of the f64 truth;
    distances are non-decreasing; and no member left out is certainly nearer than the last one returned (its f64 distance plus
    its bound below the returned k-th distance).  So two answers may swap only where their f64 distances lie within the sum of
    their bounds.  Returns a list of failure strings."""
    members = np.asarray(sorted(int(m) for m in members), dtype=np.int64)
    fails = check_per_answer(metric, X, Q, ids, dists, counts, simd8)
    want = min(k, len(members))
    mset = set(members.tolist())
    for i in range(len(Q)):
        c = int(counts[i])
        if c != want:
            fails.append(f"query {i}: {c} answers, the exact k-NN has {want}")
            continue
        row = [int(v) for v in ids[i, :c]]
        if not set(row) <= mset:
            fails.append(f"query {i}: ids outside the candidate set: {sorted(set(row) - mset)[:4]}")
            continue
        if c == len(members) or c == 0:
            continue
        rest = np.setdiff1d(members, np.asarray(row, np.int64), assume_unique=True)
        an = _analyse_rows(metric, X, Q[i], rest, simd8)
        kth = float(dists[i, c - 1])
        nearer = an.truth + an.err < kth
        if nearer.any():
            j = int(np.argmax(nearer))
            fails.append(f"query {i}: id {int(rest[j])} left out at f64 distance {an.truth[j]!r} (bound {an.err[j]!r}) "
                         f"though the answer's last distance is {kth!r}")
        if len(fails) > 8:
            break
    return fails


def exact_knn(metric, X, q, k, members=None, simd8=False):
    """(ids, f64 distances, bounds) of the k nearest rows of X to q (or of `members`), ascending in f64, ids ascending on ties"""
    ids = np.arange(len(X)) if members is None else np.asarray(sorted(members), np.int64)
    an = _analyse_rows(metric, X, q, ids, simd8)
    order = np.lexsort((ids, an.truth))[:k]
    return ids[order], an.truth[order], an.err[order]


# ----------------------------------------------------------------------------------------------------- graph walks
class GraphWalk:
    """The neighbour lists of an index (product Hnsw, built or reloaded from a dump), read from the host side with get_neighbours.
    Points are named by PointId (layer, rank); `origin` maps them to origin ids as far as the lists and the entry point name them."""

    def __init__(self, h):
        self.h = h
        self.max_level = h.get_max_level_observed()
        self.count = [h.get_layer_nb_point(L) for L in range(self.max_level + 1)]
        o, pid = h.get_entry_point()
        self.entry = (int(pid[0]), int(pid[1]))
        self.origin = {self.entry: int(o)}
        self.lists = {}          # (pid, l) -> (origins, pids, dists)
        # every point's list of EVERY layer: a former entry point keeps lists above its own level (it took the reverse edges of
        # the higher points inserted while it was the entry point, src/hnsw.rs:1158-1165), and the descent reads them
        for L in range(self.max_level + 1):
            for r in range(self.count[L]):
                for l in range(self.max_level + 1):
                    ids, layers, ranks, dists = h.get_neighbours(L, r, l)
                    pids = [(int(a), int(b)) for a, b in zip(layers, ranks)]
                    for p, oid in zip(pids, ids):
                        self.origin[p] = int(oid)
                    self.lists[((L, r), l)] = (ids.astype(np.int64), pids, dists)

    def points(self):
        return [(L, r) for L in range(self.max_level + 1) for r in range(self.count[L])]

    def layer0_entries(self):
        """every point the greedy descent can hand to layer 0: the entry point and every point a list of layer >= 1 names (the
        descent moves only along those lists, src/hnsw.rs:1511-1529).  That is mostly points of level >= 1, but a former entry
        point of a lower level can sit in such a list too (see check_graph)."""
        upper = {p for (owner, l), (_, pids, _) in self.lists.items() if l >= 1 for p in pids}
        return [self.entry] + sorted(p for p in upper if p != self.entry)

    def layer0_reachability(self):
        """{entry PointId: frozenset of origin ids reachable in layer 0 from it} for every possible layer-0 entry"""
        adj = {p: self.lists[(p, 0)][1] for p in self.points()}
        radj = collections.defaultdict(list)
        for p, nb in adj.items():
            for q in nb:
                radj[q].append(p)

        def bfs(start, graph):
            seen, todo = {start}, [start]
            while todo:
                p = todo.pop()
                for q in graph.get(p, ()):
                    if q not in seen:
                        seen.add(q)
                        todo.append(q)
            return seen

        r0 = bfs(self.entry, adj)
        back = bfs(self.entry, radj)           # points from which the entry point is reachable
        full = frozenset(self.origin[p] for p in r0)
        out = {}
        for e in self.layer0_entries():
            if e in r0 and e in back:          # reach(e) is inside r0 and contains the entry point: it IS r0
                out[e] = full
            else:
                out[e] = frozenset(self.origin[p] for p in bfs(e, adj))
        return out


def common_reachable_set(h):
    """the layer-0 set every possible entry reaches, or None if the entries reach different sets"""
    sets = set(GraphWalk(h).layer0_reachability().values())
    return next(iter(sets)) if len(sets) == 1 else None


# ----------------------------------------------------------------------------------------------------- the hostile sweep
# every dimension 1..130 (every residue mod 8, 32 and 64 of the lane groups) and the larger residues the device sweeps use
SWEEP_D = tuple(sorted(set(list(range(1, 131)) + [159, 160, 161, 191, 192, 193, 255, 256, 257, 300, 383, 384, 385, 511, 512, 513,
                                                  640, 767, 768, 769, 783, 784, 785, 799, 800])))
# rows as long as the ones people index (1024 .. 4096 wide) and up to where U_EFF is stated: the powers of two with their neighbours,
# 1054 / 1055 / 1056 for DistCosine (the norm in the last two floats of a stride of 1056, then beside the row).  A tuple of its own:
# the tests parametrised on SWEEP_D stay as quick as they are
LONG_D = (801, 832, 1023, 1024, 1025, 1054, 1055, 1056, 1536, 2047, 2048, 3072, 4095, 4096, 4097, 6144, 7999, 8000)


def _mixed(rng, shape, lo, hi, signed=True):
    """magnitudes 2^lo .. 2^hi mixed within one vector"""
    v = np.exp2(rng.uniform(lo, hi, shape))
    if signed:
        v *= rng.choice([-1.0, 1.0], shape)
    return v.astype(np.float32)


def _prob(v):
    v = np.asarray(v, np.float64)
    s = v.sum(-1, keepdims=True)
    return np.where(s > 0, v / np.where(s > 0, s, 1.0), 0.0).astype(np.float32)


def hostile_sweep(metric, d, seed, simd8=False):
    """(Q, R): 4 queries and 70 rows of dimension d whose pairs cover the places where f32 distances go wrong.
    Real-valued metrics: uniform, magnitudes 2^-60 .. 2^60 mixed within one vector, near-identical vectors (cancellation),
    exact copies, exact zeros and subnormals, a zero vector, scaled copies, and (L2, L1) sums that overflow f32.
    Probability metrics: probability vectors with zeros, near-one-hot vectors, p == q, near-identical p and q, subnormal
    coordinates, magnitudes mixed over 2^-60 .. 1."""
    rng = np.random.default_rng([seed, d, METRICS.index(metric), int(simd8)])
    Q = np.zeros((4, d), np.float32)
    R = np.zeros((70, d), np.float32)
    if metric not in PROBABILITY_METRICS:
        hi = {"DistDot": 50, "DistCosine": 30 if simd8 else 60}.get(metric, 60)
        lo = -30 if (metric == "DistCosine" and simd8) else -60
        Q[0] = rng.uniform(-1, 1, d)
        Q[1] = _mixed(rng, d, lo, hi)
        Q[2] = rng.uniform(-1, 1, d)
        Q[2, rng.random(d) < 0.4] = 0.0
        sub = rng.random(d) < 0.3
        Q[2, sub] = _mixed(rng, int(sub.sum()), -149, -127)
        if metric in ("DistL2", "DistL1"):
            Q[3] = _mixed(rng, d, 60, 64)                      # sums that overflow f32 (L2 from about 2^64 / sqrt(d))
        elif metric == "DistDot":
            Q[3] = rng.uniform(-1, 1, d)
            Q[3] /= np.linalg.norm(Q[3]) or 1.0                 # its domain: unit vectors
        else:
            Q[3] = _mixed(rng, d, lo, lo + 10)                  # a tiny vector
        R[0:16] = rng.uniform(-1, 1, (16, d))
        R[16:28] = _mixed(rng, (12, d), lo, hi)
        for j in range(28, 36):                                  # near-identical (cancellation) and exact copies
            q = Q[j % 4].astype(np.float64)
            R[j] = q if j >= 32 else q * (1 + 2.0 ** -20 * rng.standard_normal(d))
        R[36:44] = rng.uniform(-1, 1, (8, d))
        R[36:44][rng.random((8, d)) < 0.4] = 0.0
        sub = rng.random((8, d)) < 0.3
        R[36:44][sub] = _mixed(rng, int(sub.sum()), -149, -127)
        if metric in ("DistL2", "DistL1"):
            R[44:52] = -_mixed(rng, (8, d), 60, 64) * np.sign(Q[3]).astype(np.float32)
        elif metric == "DistDot":
            v = rng.uniform(-1, 1, (8, d))
            R[44:52] = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-30)
        else:
            R[44:52] = _mixed(rng, (8, d), lo, lo + 10)
        R[52] = 0.0                                              # the zero vector
        for j in range(53, 64):                                  # scaled copies: cos = 1, L2 = |1 - s| |q|
            R[j] = Q[j % 4] * np.float32(2.0 ** rng.integers(-8, 9))
        R[64:70] = rng.uniform(0, 1e-3, (6, d))
        if metric == "DistDot":                                  # keep |a . b| summable in f32 (else no bound)
            R[53:64] = np.clip(R[53:64], -2.0 ** 40, 2.0 ** 40)
    else:
        def prob_with_zeros(n):
            v = rng.random((n, d)) + 1e-3
            v[rng.random((n, d)) < 0.2] = 0.0
            return _prob(v)

        def one_hot(n):
            v = np.where(rng.random((n, d)) < 0.5, 0.0, 1e-8 * rng.random((n, d)))
            v[np.arange(n), rng.integers(0, d, n)] = 1.0
            return _prob(v)

        def with_subnormals(n):
            v = rng.random((n, d)) + 1e-3
            sub = rng.random((n, d)) < 0.3
            v[sub] = 2.0 ** rng.uniform(-149, -127, int(sub.sum()))
            p = _prob(v)
            p[sub] = np.exp2(rng.uniform(-149, -127, int(sub.sum()))).astype(np.float32)
            return p

        Q[0] = prob_with_zeros(1)[0]
        Q[1] = one_hot(1)[0]
        Q[2] = with_subnormals(1)[0]
        Q[3] = _prob(np.exp2(rng.uniform(-60, 0, d)))
        R[0:16] = prob_with_zeros(16)
        R[16:24] = one_hot(8)
        R[24:28] = Q                                             # p == q
        for j in range(28, 36):                                  # near-identical p and q
            R[j] = _prob(Q[j % 4].astype(np.float64) * (1 + 1e-6 * rng.standard_normal(d)))
        R[36:44] = with_subnormals(8)
        R[44:52] = _prob(np.exp2(rng.uniform(-60, 0, (8, d))))
        R[52] = _prob(rng.random(d))
        for j in range(53, 64):                                  # one-hot at the query's own largest coordinate
            v = np.where(rng.random(d) < 0.5, 0.0, 1e-8 * rng.random(d))
            v[int(np.argmax(Q[j % 4]))] = 1.0
            R[j] = _prob(v)
        R[64:70] = _prob(rng.random((6, d)) ** 8)
        if d == 1:
            Q[:] = 1.0
            R[:] = 1.0
    return np.ascontiguousarray(Q), np.ascontiguousarray(R)


def check_graph(h, X, metric, m, levels=None, stats=None, chunk=20000):
    """Every list of every layer of a built index against the f64 reference: each stored distance within the bound of the f64
    distance between owner and neighbour (owner first, as the builder evaluates it); no list holds its owner or a p_id twice
    (src/hnsw.rs:1258-1266); at most M ids, 2M at layer 0; every neighbour of a layer-l list lives on layer >= l, former entry
    points aside (see below); stored distances non-decreasing (src/hnsw.rs:1280).  Owners are named by the lists and the entry point; `levels` (the level of every input
    row, drawn in input order) names the rest -- ranks inside a layer follow the input order -- and is checked against every
    owner the lists name.  Returns a list of failure strings; `stats` receives counts."""
    w = GraphWalk(h)
    fails = []
    owner = dict(w.origin)
    if levels is not None:
        members = [np.nonzero(np.asarray(levels) == L)[0] for L in range(w.max_level + 1)]
        for L in range(w.max_level + 1):
            if len(members[L]) != w.count[L]:
                fails.append(f"layer {L} holds {w.count[L]} points, the levels say {len(members[L])}")
                members = None
                break
        if members is not None:
            wrong = [(p, o) for p, o in w.origin.items() if int(members[p[0]][p[1]]) != o]
            if wrong:
                fails.append(f"{len(wrong)} points are not where the input order puts them, e.g. {wrong[:3]}")
            else:
                owner = {p: int(members[p[0]][p[1]]) for p in w.points()}
    own_a, nb_a, dist_a = [], [], []
    below = {}          # level -> the points of that level met in lists of a higher layer
    for (p, l), (ids, pids, dists) in w.lists.items():
        cap = 2 * m if l == 0 else m
        if len(pids) > cap:
            fails.append(f"{p} layer {l}: {len(pids)} ids > {cap}")
        if len(set(pids)) != len(pids):
            fails.append(f"{p} layer {l}: a p_id twice {pids}")
        if p in pids:
            fails.append(f"{p} layer {l}: the owner in its own list")
        for q in pids:
            if q[0] < l:
                below.setdefault(q[0], set()).add(q)
        if len(dists) > 1 and not np.all(dists[1:] >= dists[:-1]):
            fails.append(f"{p} layer {l}: stored distances not non-decreasing {dists.tolist()}")
        if p in owner and len(ids):
            own_a.append(np.full(len(ids), owner[p], np.int64))
            nb_a.append(ids)
            dist_a.append(dists)
    # A neighbour below the list's layer is the reference's own doing in one case only: a point whose level exceeds the entry
    # point's searches its top layers from the (lower) entry point, and search_layer returns that entry point whatever its level
    # (src/hnsw.rs:1158-1165, :951-967).  The entry points of a build have strictly increasing levels, so at most ONE point of each
    # level may appear so; anything more is a wrong edge.
    for lv, pts in below.items():
        if len(pts) > 1:
            fails.append(f"{len(pts)} points of level {lv} in lists of higher layers, e.g. {sorted(pts)[:4]}: only a former entry "
                         f"point may be there")
    if own_a:
        own, nb, dist = np.concatenate(own_a), np.concatenate(nb_a), np.concatenate(dist_a)
        if int(nb.max()) >= len(X):
            fails.append(f"a neighbour id beyond the {len(X)} points")
        else:
            for s in range(0, len(own), chunk):
                an = analyse(metric, X[own[s:s + chunk]], X[nb[s:s + chunk]])
                bad = violations(an, dist[s:s + chunk])
                for i in np.nonzero(bad)[0][:4]:
                    fails.append(f"edge {int(own[s + i])} -> {int(nb[s + i])}: stored {float(dist[s + i])!r}, f64 {an.truth[i]!r} "
                                 f"bound {an.err[i]!r}")
    if stats is not None:
        stats.update(edges=int(sum(len(a) for a in nb_a)), lists=len(w.lists), owners_named=len(owner),
                     former_entry_points=sorted(p for pts in below.values() for p in pts))
    return fails
