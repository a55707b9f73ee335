"""Exact k-NN behind the matrix-core screen (csrc/exact_screen.hip, include/hnsw_mi355x_exact_screen.h): the answers are the CPU
oracle's lexsort byte for byte (never the existing device path's), the certificate refuses where it must, and the screen's lower
bound itself -- hnswxs_screen_matrix -- lies below the oracle's f32 distance for every pair and not uselessly far below.
Indexes are hand-written dumps (tests/dump_writer.py).  The bound of DESIGN.md 15.13 is restated in `bound_terms`."""
import ctypes as C
import functools

import numpy as np
import pytest

import f64_reference as F
from conftest import normalized, uniform
from dump_writer import dump_order, write_dump
from test_gpu_exact_knn import _assert_answers
from test_gpu_exact_knn_hostile import N as NH, _assert_hostile, _case

gpu = pytest.mark.gpu
MARGIN = 54                      # SCREEN_MARGIN of exact_screen.hip
METRICS = ("DistL2", "DistDot", "DistCosine")
DIMS = (1, 3, 30, 33, 128, 130)  # every residue of the 8-element MFMA group and of the 32-element chunk that matters, one and two chunks
SHAPES = ((700, 37), (5000, 150))  # one slab and five; part-filled query tiles and row blocks
U = 2.0 ** -24
NORM_LO, NORM_HI = 2.0 ** -40, 2.0 ** 40
# DistCosine at d = 1: every distance is 0 or 2, so no seed leaves fewer than MARGIN rows at the k-th distance: answers only
DEGENERATE = {("DistCosine", 1)}


def _benign(metric, n, d, seed):
    return normalized(n, d, seed) if metric == "DistDot" and d >= 3 else uniform(n, d, seed)


def bound_terms(metric, Q, X):
    """(pre, E, finish) in f64: the quantity the screen bounds (squared distance, inner product, cosine), the documented error
    term for every pair, and the way from a bound of that quantity to a bound of the distance"""
    Q, X = Q.astype(np.float64), X.astype(np.float64)
    d = Q.shape[1]
    S, nq, nx = Q @ X.T, (Q * Q).sum(1)[:, None], (X * X).sum(1)[None, :]
    if metric == "DistL2":
        return nq + nx - 2 * S, (4 * d + 32) * U * (nq + nx), lambda lo: np.sqrt(np.maximum(lo, 0))
    if metric == "DistDot":
        return S, (d + 32) * U * (nq + nx), lambda hi: np.maximum(1 - hi, 0)
    return S / np.sqrt(nq * nx), (2 * d + 32) * U + 0 * S, lambda hi: np.maximum(1 - hi, 0)


def lowest_possible(metric, Q, X):
    """the smallest bound the documented error term allows the kernel: the truth moved by 2 E"""
    pre, E, finish = bound_terms(metric, Q, X)
    return finish(pre - 2 * E if metric == "DistL2" else pre + 2 * E)


class Benign:
    def __init__(self, metric, d, n, nq):
        self.metric, self.d, self.n = metric, d, n
        self.X, self.Q = _benign(metric, n, d, 100 + d), _benign(metric, nq, d, 200 + d)
        self.ids = np.arange(n, dtype=np.uint64)     # (F.check_exact_knn: origin ids are rows)
        self.levels = np.zeros(n, np.int64)
        p = np.random.default_rng(d).permutation(n)
        self.levels[p[:40]], self.levels[p[40:45]] = 1, 2

    def load(self, native, tmp_path):
        _, self.pids = write_dump(tmp_path, "screen", self.X, self.ids, self.levels, self.metric)
        h = native.HnswIo(tmp_path, "screen").load_hnsw(self.metric)
        h.upload(0)
        return h


@functools.lru_cache(maxsize=2)
def _benign_case(metric, d, n, nq):
    return Benign(metric, d, n, nq)


def _ks(n):
    return (1, 10, 100, n + 5)


def _crowded(case, D, k):
    """per query: rows outside the top k whose lowest possible bound is at or below the exact k-th distance"""
    lb = lowest_possible(case.metric, case.Q, case.X)
    kth = np.sort(D, axis=1)[:, min(k, case.n) - 1].astype(np.float64)
    return (lb <= kth[:, None]).sum(1) - min(k, case.n)


@pytest.mark.parametrize("n,nq", SHAPES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_benign_inputs_can_be_certified(oracle, metric, d, n, nq):
    """the condition of the bit-exact test, on the oracle's matrix alone (no device)"""
    case = _benign_case(metric, d, n, nq)
    D = oracle.dist_matrix(metric, case.Q, case.X)
    for k in _ks(n):
        worst = int(_crowded(case, D, k).max())
        assert (metric, d) in DEGENERATE or k >= n or worst < MARGIN, (k, worst)


@gpu
@pytest.mark.parametrize("n,nq", SHAPES)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("metric", METRICS)
def test_benign_bit_exact_and_certified(native, oracle, tmp_path, metric, d, n, nq):
    case = _benign_case(metric, d, n, nq)
    h = case.load(native, tmp_path)
    for k in _ks(n):
        if k > 4096:                             # n + 5 at n = 5000: refused, in the existing call's words
            with pytest.raises(native.HnswError, match="knbn above 4096"):
                h.exact_search_screened_flat(case.Q, k)
            continue
        res, stats = h.exact_search_screened_flat(case.Q, k)
        what = f"{metric} d {d} n {n} k {k} stats {stats.tolist()}"
        _assert_answers(oracle, metric, res, case.Q, case.X, case.ids, k, what=what)
        c = min(k, n)
        want_pids = [[case.pids[int(r)] for r in row[:c]] for row in res.ids]
        assert [list(zip(res.layers[q, :c].tolist(), res.ranks[q, :c].tolist())) for q in range(nq)] == want_pids, what
        assert int(stats.sum()) == nq and stats[2] == 0, what
        if (metric, d) not in DEGENERATE:
            assert stats[1] == 0, what           # the fallback may not hide the screen
        if k == 10:
            assert not F.check_exact_knn(metric, case.X, case.Q, res.ids, res.dists, res.counts, k, range(n))[:4], what


@gpu
@pytest.mark.parametrize("d", (3, 33, 128))
@pytest.mark.parametrize("metric", METRICS)
def test_hostile_bit_exact(native, oracle, tmp_path, metric, d):
    """F.hostile_sweep as queries and rows: whatever mix of certified and fallen-back queries, the oracle's answers; a NaN last
    and canonical (_assert_hostile)"""
    case = _case(metric, d)
    h = case.load(native, tmp_path)
    for k in (1, 10, 300, NH - 1, NH + 5):
        res, stats = h.exact_search_screened_flat(case.Q, k)
        assert int(stats.sum()) == len(case.Q)
        _assert_hostile(oracle, case, res, k, what=f"{metric} d {d} k {k} stats {stats.tolist()}")


@gpu
@pytest.mark.parametrize("metric", METRICS)
def test_the_certificate_refuses_a_crowd_of_copies(native, oracle, tmp_path, metric):
    """200 exact copies of one vector among 700 rows and queries next to them, k = 10: the copies share one screen value, the
    C-th bound cannot exceed the k-th distance, and the answer is cut by DataId rank like the oracle's"""
    n, d, k = 700, 30, 10
    X = _benign(metric, n, d, 7)
    copies = np.random.default_rng(8).choice(n, 200, replace=False)
    X[copies] = X[copies[0]]
    near = X[copies[:5]] * np.float32(1.0) + np.float32(1e-3) * uniform(5, d, 9)
    Q = np.ascontiguousarray(np.concatenate([near, _benign(metric, 32, d, 10)]))
    ids = np.random.default_rng(11).permutation(n).astype(np.uint64) * 5 + 2
    write_dump(tmp_path, "copies", X, ids, np.zeros(n, np.int64), metric)
    h = native.HnswIo(tmp_path, "copies").load_hnsw(metric)
    h.upload(0)
    res, stats = h.exact_search_screened_flat(Q, k)
    _assert_answers(oracle, metric, res, Q, X, ids, k, what=f"copies {metric} {stats.tolist()}")
    assert stats[1] >= 1 and int(stats.sum()) == len(Q), stats
    assert set(res.ids[0].tolist()) <= set(ids[copies].tolist())


@gpu
def test_filters_unscreened_metric_f16_and_the_device_entry(native, oracle, tmp_path):
    import torch
    import hnsw_rs_amd._native as N_
    case = _benign_case("DistL2", 33, 700, 37)
    h = case.load(native, tmp_path)
    rng = np.random.default_rng(5)
    for rows, k in ((np.sort(rng.choice(700, 210, replace=False)), 10), (np.array([3, 99, 500, 650]), 10)):
        res, stats = h.exact_search_screened_flat(case.Q, k, np.sort(case.ids[rows]))
        _assert_answers(oracle, "DistL2", res, case.Q, case.X, case.ids, k, rows, what=f"filter of {len(rows)}")
        assert stats[1] == 0 and stats[2] == 0
    # the _device entry on a stream of the caller's
    L, nq, k = native.lib(), len(case.Q), 10
    want, _ = h.exact_search_screened_flat(case.Q, k)
    dq = torch.from_numpy(case.Q).cuda()
    o_ids = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
    o_d = torch.full((nq, k), -1.0, dtype=torch.float32, device="cuda")
    o_l = torch.full((nq, k), 9, dtype=torch.uint8, device="cuda")
    o_r = torch.full((nq, k), -1, dtype=torch.int32, device="cuda")
    o_c = torch.full((nq,), -1, dtype=torch.int32, device="cuda")
    stats = np.full(3, 99, np.uint64)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc = L.hnswxs_exact_search_batch_device(h.handle, C.c_void_p(dq.data_ptr()), nq, 33, k, None, 0, C.c_void_p(o_ids.data_ptr()),
                                                      C.c_void_p(o_d.data_ptr()), C.c_void_p(o_l.data_ptr()), C.c_void_p(o_r.data_ptr()),
                                                      C.c_void_p(o_c.data_ptr()), stats.ctypes.data_as(C.c_void_p), C.c_void_p(stream.cuda_stream))
    assert rc == 0 and stats.tolist() == [nq, 0, 0]
    assert np.array_equal(o_ids.cpu().numpy().astype(np.uint64), want.ids) and np.array_equal(o_d.cpu().numpy().view(np.uint32), want.dists.view(np.uint32))
    assert np.array_equal(o_c.cpu().numpy().astype(np.uint32), want.counts)
    assert np.array_equal(o_l.cpu().numpy(), want.layers) and np.array_equal(o_r.cpu().numpy(), want.ranks)
    # a distance without a screen: the same answers, nothing screened
    X1, Q1 = uniform(700, 30, 21), uniform(37, 30, 22)
    write_dump(tmp_path, "l1", X1, np.arange(700), np.zeros(700, np.int64), "DistL1")
    h1 = native.HnswIo(tmp_path, "l1").load_hnsw("DistL1")
    h1.upload(0)
    res, stats = h1.exact_search_screened_flat(Q1, 10)
    _assert_answers(oracle, "DistL1", res, Q1, X1, np.arange(700), 10, what="DistL1")
    assert stats.tolist() == [0, 0, 37]
    # F16 storage: refused like the existing call
    hf = native.Hnsw(8, 64, 16, 16, "DistL2")
    hf.parallel_insert(native.round_to_f16(uniform(64, 8, 23)))
    hf.set_storage("f16")
    with pytest.raises(native.HnswError) as err:
        hf.exact_search_screened_flat(uniform(2, 8, 24), 3)
    assert err.value.code == N_.ERR_ARG


@gpu
@pytest.mark.parametrize("hostile", (False, True))
@pytest.mark.parametrize("metric", METRICS)
def test_the_bound_itself(native, oracle, tmp_path, metric, hostile):
    """37 x 700: every bound is a number >= +0 and <= the oracle's f32 distance; a pair whose oracle distance is NaN or whose f32
    norms (summed as the kernels sum them) leave [2^-40, 2^40] carries +0; benign: the bound is within 2 E of the truth"""
    case = _case(metric, 33) if hostile else _benign_case(metric, 33, 700, 37)
    h = case.load(native, tmp_path)
    by_position = h.exact_screen_matrix(case.Q)
    lb = np.empty_like(by_position)
    lb[:, np.asarray(dump_order(case.levels)[0])] = by_position   # column p of the matrix is the row at dump position p
    D = oracle.dist_matrix(metric, case.Q, case.X)
    assert lb.shape == D.shape and not np.isnan(lb).any() and (lb >= 0).all() and not np.signbit(lb).any()
    ok = ~np.isnan(D)
    assert (lb[ok] <= D[ok]).all(), (metric, float((lb[ok] - D[ok]).max()))
    with np.errstate(all="ignore"):
        nq = np.cumsum(case.Q * case.Q, axis=1, dtype=np.float32)[:, -1][:, None]
        nx = np.cumsum(case.X * case.X, axis=1, dtype=np.float32)[:, -1][None, :]
        inside = (nq >= NORM_LO) & (nq <= NORM_HI) & (nx >= NORM_LO) & (nx <= NORM_HI)
    assert not lb[~ok].view(np.uint32).any() and not lb[~(inside & np.ones_like(ok))].view(np.uint32).any()
    if hostile:
        assert (~inside).any() and inside.any()
    else:
        assert inside.all()
        floor = lowest_possible(metric, case.Q, case.X)
        assert (lb.astype(np.float64) >= floor * (1 - 2.0 ** -22) - 2.0 ** -140).all(), (metric, float((floor - lb).max()))
