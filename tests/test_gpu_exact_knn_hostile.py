"""Exhaustive exact k-NN on the device on HOSTILE values: the sweep of tests/f64_reference.py (magnitudes 2^-60 .. 2^60 in one
vector, subnormals, cancellation, exact copies, sums that overflow f32, near-identical probability vectors) as rows AND queries
of csrc/exact_knn.hip and csrc/exact_tile.hpp -- its own chain (chain4, scalar-operand query elements), its own DistCosine finish (norm_in_tail) and its
own total order on f32 distances (dist_order_bits / make_key / dist_of_key: +inf tie groups, NaN last and canonical, ties cut
by origin id, then dump order).

The builder cannot take such rows (the reference refuses a NaN distance during insertion and asserts the domain of DistCosine /
DistHellinger on row-to-row pairs), and the exact search never reads the graph: every index here is a dump written by hand
(tests/dump_writer.py) and loaded with HnswIo.load_hnsw.

As in tests/test_gpu_exact_knn.py the expected answer is the lexsort of the CPU oracle's distances and every comparison is
exact; the float64 reference checks every pair's distance sharing nothing with the oracle.  What the inputs must contain for
these tests to mean anything (+inf tie groups cut at k, NaN distances, ties at the cuts, pairs with a finite f64 bound) is
asserted on the ORACLE's matrix, never on device output; test_input_conditions needs no device."""
import ctypes as C
import functools

import numpy as np
import pytest

import f64_reference as F
from conftest import normalized, uniform
from dump_writer import write_dump
from test_gpu_exact_knn import _assert_answers

gpu = pytest.mark.gpu
SWEEP_SEED = 7            # one seed for queries and rows: cross-seed pairs leave the domain the reference asserts for DistHellinger
DIMS = (1, 3, 8, 25, 30, 31, 32, 33, 64, 100, 126, 128, 130, 784)
N, N_BENIGN_Q = 700, 33
KS = (1, 10, 64, 65, 300, N - 1, N, N + 5)
CUT_KS = (1, 10, 64, 65, 300, N - 1)
CANONICAL_NAN = 0x7FC00000


def _benign(metric, n, d, seed):
    if metric in F.PROBABILITY_METRICS:      # (conftest.probability zeroes every fifth coordinate: 0 / 0 at d = 1)
        return F._prob(np.random.default_rng(seed).random((n, d)) + 1e-3)
    return normalized(n, d, seed) if metric == "DistDot" else uniform(n, d, seed)


class Case:
    """One (metric, d): 37 queries (the sweep's 4, then 33 benign: two tiles of 16 and a part), 700 rows (benign, the sweep's 70 at
    flat positions round(linspace(0, 699, 70)): in every slab and next to the 64-row steps), three layers each holding hostile
    rows (the dump order is not the row order), origin ids a sparse permutation"""

    def __init__(self, metric, d):
        self.metric, self.d = metric, d
        Qh, Rh = F.hostile_sweep(metric, d, SWEEP_SEED)
        self.Q = np.ascontiguousarray(np.concatenate([Qh, _benign(metric, N_BENIGN_Q, d, 1000 + d)]))
        self.hostile = np.round(np.linspace(0, N - 1, len(Rh))).astype(np.int64)
        assert len(np.unique(self.hostile)) == len(Rh)
        self.X = _benign(metric, N, d, 2000 + d)
        self.X[self.hostile] = Rh
        self.benign = np.setdiff1d(np.arange(N), self.hostile)
        rng = np.random.default_rng(3000 + d)
        self.levels = np.zeros(N, np.int64)
        hp, bp = rng.permutation(self.hostile), rng.permutation(self.benign)
        self.levels[hp[:2]] = 2
        self.levels[bp[:3]] = 2
        self.levels[hp[2:10]] = 1
        self.levels[bp[3:35]] = 1
        self.ids = rng.permutation(N).astype(np.uint64) * 3 + 1
        self.row_of_id = {int(v): i for i, v in enumerate(self.ids)}

    def load(self, native, tmp_path):
        """the index, loaded from the hand-written dump and uploaded; self.pids[row] = (layer, rank) by the writer"""
        order, self.pids = write_dump(tmp_path, "hostile", self.X, self.ids, self.levels, self.metric)
        assert order != sorted(order)
        h = native.HnswIo(tmp_path, "hostile").load_hnsw(self.metric)
        assert h.get_nb_point() == N
        h.upload(0)
        return h


@functools.lru_cache(maxsize=4)
def _case(metric, d):
    return Case(metric, d)


def _rows_of(case, res, q, c):
    return np.array([case.row_of_id[int(v)] for v in res.ids[q, :c]], np.int64)


def _assert_hostile(oracle, case, res, k, rows=None, what=""):
    """_assert_answers (ids, f32 bits, counts against the oracle's lexsort) and what it leaves open: a NaN comes back as THE
    canonical quiet NaN, behind every number, and (out_layer, out_rank) of EVERY returned slot is the writer's (layer, rank)"""
    _assert_answers(oracle, case.metric, res, case.Q, case.X, case.ids, k, rows, what)
    for q in range(len(case.Q)):
        c = int(res.counts[q])
        got = res.dists[q, :c]
        nan = np.isnan(got)
        assert (got.view(np.uint32)[nan] == CANONICAL_NAN).all(), (what, q, "a NaN that is not the canonical one")
        assert not nan.any() or nan[int(np.argmax(nan)):].all(), (what, q, "a number behind a NaN")
        want_pids = [case.pids[r] for r in _rows_of(case, res, q, c)]
        assert list(zip(res.layers[q, :c].tolist(), res.ranks[q, :c].tolist())) == want_pids, (what, q, "p_ids")


def _oracle_matrix(oracle, case):
    return oracle.dist_matrix(case.metric, case.Q, case.X)


def _f64_violations(case, got):
    """F.violations of a 37 x 700 matrix against the f64 analysis, a few queries at a time (d = 784 is 20 M pairs of elements)"""
    bad, finite = [], 0
    for s in range(0, len(case.Q), 8):
        an = F.analyse(case.metric, case.Q[s:s + 8, None, :], case.X[None, :, :])
        mask = F.violations(an, got[s:s + 8])
        finite += int(np.isfinite(an.err).sum())
        bad += [f"query {s + i[0]} row {i[1]}: " + m for i, m in zip(np.argwhere(mask)[:4], F.describe(case.metric, an, got[s:s + 8], mask))]
    return bad, finite / got.size


def _cuts_through_ties(D, ks):
    s = np.sort(D, axis=1)                      # (NaN sorts last; NaN == NaN is false: a cut inside the NaN group is test (b)'s)
    return sum(int((s[:, k - 1] == s[:, k]).sum()) for k in ks)


# ----------------------------------------------------------------------------------------------------- the inputs (no device)
@pytest.mark.parametrize("metric", F.METRICS)
def test_input_conditions(oracle, metric):
    """What the construction must deliver, on the oracle's matrix: DistL2 at least 78 +inf distances per d and a +inf tie group
    cut at k = n - 1 for every query and at k = 300 for some query of every d >= 8; DistJensenShannon at least one NaN and one +inf over the 14 d; per metric at least
    0.99 of the pairs with a finite f64 bound, at least 100 cuts through a tie, and the oracle itself inside the f64 bound"""
    n_nan = n_inf = cuts = 0
    share = []
    for d in DIMS:
        case = _case(metric, d)
        D = _oracle_matrix(oracle, case)
        bad, fin = _f64_violations(case, D)
        assert not bad, (metric, d, bad[:4])
        share.append(fin)
        n_nan += int(np.isnan(D).sum())
        n_inf += int(np.isposinf(D).sum())
        cuts += _cuts_through_ties(D, CUT_KS)
        if metric == "DistL2":
            assert int(np.isposinf(D).sum()) >= 78, (d, int(np.isposinf(D).sum()))
            s = np.sort(D, axis=1)
            # every query meets rows of 2^60 .. 2^64: k = n - 1 cuts its +inf group; from d = 8 on the query of that size
            # overflows against (nearly) every row and k = 300 cuts inside its group (d = 1, 3: too few squares to reach 2^128)
            assert (np.isposinf(s[:, N - 2]) & np.isposinf(s[:, N - 1])).all(), (d, "no +inf tie group at k = n - 1")
            assert d < 8 or (np.isposinf(s[:, 299]) & np.isposinf(s[:, 300])).any(), (d, "no +inf tie group at k = 300")
    assert min(share) >= 0.99, (metric, min(share))
    assert cuts >= 100, (metric, cuts)
    if metric == "DistJensenShannon":
        assert n_nan >= 1 and n_inf >= 1, (n_nan, n_inf)


# ----------------------------------------------------------------------------------------------------- (a) every metric x d
@gpu
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", F.METRICS)
def test_hostile_sweep_bit_exact(native, oracle, tmp_path, metric, d):
    """k from 1 through the +inf and NaN groups to n + 5: ids, f32 bits, counts and every p_id against the oracle's lexsort;
    with k = n + 5 every pair comes back: the 37 x 700 matrix rebuilt from (ids, dists) lies within the f64 bound"""
    case = _case(metric, d)
    h = case.load(native, tmp_path)
    for k in KS:
        res = h.exact_search_flat(case.Q, k)
        _assert_hostile(oracle, case, res, k, what=f"{metric} d {d} k {k}")
    got = np.full((len(case.Q), N), -1.0, np.float32)
    for q in range(len(case.Q)):
        got[q, _rows_of(case, res, q, N)] = res.dists[q, :N]
    bad, _ = _f64_violations(case, got)
    assert not bad, (metric, d, bad[:4])


# ----------------------------------------------------------------------------------------------------- (b) a cut inside the NaNs
NAN_CUT_DIMS = (8, 30, 100)         # the sweep delivers a query with 2 NaN distances here (queries 0, 1 and 3); asserted below


def _nan_cut(oracle, d):
    case = _case("DistJensenShannon", d)
    D = _oracle_matrix(oracle, case)
    q = int(np.isnan(D).sum(1).argmax())
    nan_rows = np.flatnonzero(np.isnan(D[q]))
    assert len(nan_rows) >= 2, (d, q, len(nan_rows))
    return case, q, nan_rows


@pytest.mark.parametrize("d", NAN_CUT_DIMS)
def test_nan_cut_input(oracle, d):
    _nan_cut(oracle, d)


@gpu
@pytest.mark.parametrize("d", NAN_CUT_DIMS)
def test_cut_inside_the_nan_group(native, oracle, tmp_path, d):
    """k = n - 1 on a query with at least 2 NaN distances (by the oracle): the last answer is a NaN and the NaN left out bears the
    largest origin id of the group"""
    case, q, nan_rows = _nan_cut(oracle, d)
    h = case.load(native, tmp_path)
    for k in (N - len(nan_rows), N - len(nan_rows) + 1, N - 1, N):
        res = h.exact_search_flat(case.Q, k)
        _assert_hostile(oracle, case, res, k, what=f"NaN cut k {k}")
    res = h.exact_search_flat(case.Q, N - 1)
    assert res.dists[q, N - 2].view(np.uint32) == CANONICAL_NAN
    left_out = set(case.ids.tolist()) - set(res.ids[q].tolist())
    assert left_out == {int(case.ids[nan_rows].max())}


# ----------------------------------------------------------------------------------------------------- (c) under a filter
@gpu
@pytest.mark.parametrize("metric,d", [("DistL2", 33), ("DistCosine", 30), ("DistJensenShannon", 30)])
def test_hostile_rows_under_a_filter(native, oracle, tmp_path, metric, d):
    case = _case(metric, d)
    h = case.load(native, tmp_path)
    rng = np.random.default_rng(17)
    filters = {"half of the hostile rows and 100 benign": np.concatenate([rng.choice(case.hostile, 35, replace=False),
                                                                           rng.choice(case.benign, 100, replace=False)]),
               "the hostile rows": case.hostile, "the benign rows": case.benign}
    for name, rows in filters.items():
        rows = np.sort(rows)
        allowed = np.sort(case.ids[rows])
        for k in (1, 10, 300):
            res = h.exact_search_flat(case.Q, k, allowed)
            _assert_hostile(oracle, case, res, k, rows, what=f"{metric} d {d} {name} k {k}")


# ----------------------------------------------------------------------------------------------------- (d) repeated origin ids
@gpu
def test_repeated_origin_ids_are_cut_by_dump_order(native, oracle, tmp_path):
    """600 rows, every origin id borne by three of them (ids i // 3, permuted), the three on different layers for many ids; of
    75 ids the three rows hold one vector, so (distance, id) ties and only the dump order -- visible in (out_layer, out_rank) --
    decides.  For k = 1 .. 24 and k = n the answer is lexsort((dump position, id, distance)); a filter naming one id admits
    the three points that bear it."""
    n, d, metric = 600, 12, "DistL2"
    rng = np.random.default_rng(41)
    X = uniform(n, d, 42)
    for g in range(75):                                   # 150 rows duplicated: rows 3g + 1, 3g + 2 = row 3g (same id)
        X[3 * g + 1] = X[3 * g + 2] = X[3 * g]
    ids = np.arange(n, dtype=np.uint64) // 3
    perm = rng.permutation(n)
    X, ids = np.ascontiguousarray(X[perm]), ids[perm]
    levels = np.zeros(n, np.int64)
    p = rng.permutation(n)
    levels[p[:150]] = 1
    levels[p[150:200]] = 2
    order, pids = write_dump(tmp_path, "rep", X, ids, levels, metric)
    pos = np.empty(n, np.int64)
    pos[order] = np.arange(n)                             # the dump position of every row
    h = native.HnswIo(tmp_path, "rep").load_hnsw(metric)  # (the loader accepts repeated ids)
    h.upload(0)
    dup_rows = np.flatnonzero(ids < 75)
    Q = np.ascontiguousarray(np.concatenate([uniform(13, d, 43), X[dup_rows[::9]]]))   # 13 + 25 queries
    D = oracle.dist_matrix(metric, Q, X)
    full = [np.lexsort((pos, ids, D[q])) for q in range(len(Q))]
    cuts = 0
    for k in list(range(1, 25)) + [n]:
        res = h.exact_search_flat(Q, k)
        assert res.counts.tolist() == [k] * len(Q)
        for q in range(len(Q)):
            want = full[q][:k]
            assert np.array_equal(res.ids[q], ids[want]), (k, q)
            assert np.array_equal(res.dists[q].view(np.uint32), D[q, want].view(np.uint32)), (k, q)
            assert list(zip(res.layers[q].tolist(), res.ranks[q].tolist())) == [pids[r] for r in want], (k, q, "dump order")
            if k < n:
                a, b = full[q][k - 1], full[q][k]
                cuts += int(D[q, a] == D[q, b] and ids[a] == ids[b])
    assert cuts >= 20, cuts
    for one in (3, 74, 75, 199):                          # ids with one vector three times, and with three vectors
        rows = np.flatnonzero(ids == one)
        assert len(rows) == 3
        res = h.exact_search_flat(Q, 5, np.array([one], np.uint64))
        assert res.counts.tolist() == [3] * len(Q)
        for q in range(len(Q)):
            want = rows[np.lexsort((pos[rows], D[q, rows]))]
            assert list(zip(res.layers[q, :3].tolist(), res.ranks[q, :3].tolist())) == [pids[r] for r in want], (one, q)
            assert np.array_equal(res.dists[q, :3].view(np.uint32), D[q, want].view(np.uint32)) and (res.ids[q, :3] == one).all()


# ----------------------------------------------------------------------------------------------------- (e) the device entry
@gpu
def test_device_entry_on_hostile_values(native, tmp_path):
    """hnswgpu_exact_search_batch_device on a stream of the caller's: the host entry's answers, NaN and +inf included"""
    import torch
    case = _case("DistL2", 33)
    h = case.load(native, tmp_path)
    L = native.lib()
    nq = len(case.Q)
    dq = torch.from_numpy(case.Q).cuda()
    stream = torch.cuda.Stream()
    for k in (300, N + 5):
        want = h.exact_search_flat(case.Q, k)
        o_ids = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
        o_d = torch.full((nq, k), -1.0, dtype=torch.float32, device="cuda")
        o_l = torch.full((nq, k), 9, dtype=torch.uint8, device="cuda")
        o_r = torch.full((nq, k), -1, dtype=torch.int32, device="cuda")
        o_c = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = L.hnswgpu_exact_search_batch_device(h.handle, C.c_void_p(dq.data_ptr()), nq, case.d, k, None, 0, C.c_void_p(o_ids.data_ptr()),
                                                 C.c_void_p(o_d.data_ptr()), C.c_void_p(o_l.data_ptr()), C.c_void_p(o_r.data_ptr()),
                                                 C.c_void_p(o_c.data_ptr()), C.c_void_p(stream.cuda_stream))
        assert rc == 0
        assert np.array_equal(o_ids.cpu().numpy().astype(np.uint64), want.ids)
        assert np.array_equal(o_d.cpu().numpy().view(np.uint32), want.dists.view(np.uint32))
        assert np.array_equal(o_c.cpu().numpy().astype(np.uint32), want.counts)
        assert np.array_equal(o_l.cpu().numpy(), want.layers) and np.array_equal(o_r.cpu().numpy(), want.ranks)
