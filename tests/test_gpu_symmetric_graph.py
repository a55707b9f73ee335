"""The symmetrised k-NN graph on the device (Hnsw.symmetric_knn_graph_flat -> hnswgpu_symmetric_graph / _device,
csrc/symmetric_graph.hip): the directed k-NN graph of every indexed point made undirected, UNION or MUTUAL, in CSR.

The expected answers never come from the code under test: D is what the existing public calls return for every point
(exact_knn_graph_flat / knn_graph_flat with point_ids None), the neighbours' p_ids become positions through the layer sizes and one
exact search that lists every point (tests/test_symmetric_graph_abi.py: position_table), and `symmetrise` builds both answers with
dictionaries.  Every comparison is exact: offsets, positions, ids, p_ids, and the distances as u32.  What the inputs must contain (a
hub row longer than 4 k, pairs whose two directions differ in their bits) is asserted on D, never on the output under test."""
import ctypes as C
import threading

import numpy as np
import pytest

from conftest import normalized, uniform
from test_symmetric_graph_abi import position_table, symmetrise

pytestmark = pytest.mark.gpu
MODES = ("union", "mutual")
MODE_CODE = {"union": 0, "mutual": 1}
EFS = (None, 32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def positive(n, d, seed):
    """probability vectors without zeros: what DistJeffreys and DistJensenShannon are defined on"""
    x = np.random.default_rng(seed).random((n, d), dtype=np.float32) + np.float32(1e-3)
    return np.ascontiguousarray((x / x.sum(1, dtype=np.float32)[:, None]).astype(np.float32))


class Index:
    """an index built by the oracle (M = 8), dumped, loaded by the product and uploaded; D and the model's answers computed once per
    (k, ef) and shared, never modified"""

    def __init__(self, native, oracle, tmp, X, ids=None, metric="DistL2", upload=True):
        self.X, self.n, self.metric = X, len(X), metric
        o = oracle.OracleHnsw(8, self.n, 16, 48, metric)
        o.insert_batch(X, ids)
        o.file_dump(str(tmp), "g")
        self.h = native.HnswIo(str(tmp), "g").load_hnsw(metric)
        if upload:
            self.h.upload(0)
        self._D, self._want = {}, {}

    def table(self):
        """per position: DataId and p_id; per flat id: its position"""
        if not hasattr(self, "_table"):
            h, n = self.h, self.n
            every = h.exact_search_flat(self.X[:1], n)          # one exact search with k = n lists every point once
            assert every.counts[0] == n
            pos_of_flat, layer_offset = position_table([h.get_layer_nb_point(l) for l in range(16)], every.ids[0], every.layers[0], every.ranks[0])
            at = pos_of_flat[layer_offset[every.layers[0].astype(np.int64)] + every.ranks[0]]
            id_at, layer_at, rank_at = np.zeros(n, np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.int32)
            id_at[at], layer_at[at], rank_at[at] = every.ids[0], every.layers[0], every.ranks[0]
            assert (np.diff(id_at.astype(np.int64)) >= 0).all()
            self._table = (pos_of_flat, layer_offset, id_at, layer_at, rank_at)
        return self._table

    def D(self, k, ef):
        """the directed graph from the EXISTING public call, and its neighbours' positions"""
        if (k, ef) not in self._D:
            res = self.h.exact_knn_graph_flat(k) if ef is None else self.h.knn_graph_flat(k, ef)
            pos_of_flat, layer_offset = self.table()[:2]
            pos = pos_of_flat[layer_offset[res.layers.astype(np.int64)] + res.ranks]
            self._D[(k, ef)] = (res, pos)
        return self._D[(k, ef)]

    def want(self, k, ef, mode):
        """(offsets, pos, ids, dist bits, layers, ranks) of the model"""
        if (k, ef, mode) not in self._want:
            res, pos = self.D(k, ef)
            _, _, id_at, layer_at, rank_at = self.table()
            offsets, cols, bits, _, _ = symmetrise(self.n, res.counts, pos, res.dists, mode)
            c = cols.astype(np.int64)
            self._want[(k, ef, mode)] = (offsets, cols, id_at[c], bits, layer_at[c], rank_at[c])
        return self._want[(k, ef, mode)]


def _same(res, want, what=""):
    offsets, cols, ids, bits, layers, ranks = want
    assert res.offsets.dtype == np.uint64 and np.array_equal(res.offsets, offsets), (what, "offsets", res.offsets[:8], offsets[:8])
    assert len(res.pos) == len(cols) and np.array_equal(res.pos, cols), (what, "positions", np.flatnonzero(res.pos != cols)[:4])
    assert np.array_equal(res.ids, ids), (what, "ids")
    assert np.array_equal(res.dists.view(np.uint32), bits), (what, "f32 bits", np.flatnonzero(res.dists.view(np.uint32) != bits)[:4])
    assert np.array_equal(res.layers, layers) and np.array_equal(res.ranks, ranks), (what, "p_ids")


def _raw(native, ix, k, ef, mode, cap, with_arrays=True):
    """the host entry itself on out arrays filled with a pattern: (rc, message, offsets, pos, ids, dists, layers, ranks)"""
    L = native.lib()
    offs = np.full(ix.n + 1, 0x7777, np.uint64)
    m = max(cap, 1)
    out = (np.full(m, 0xA5A5A5A5, np.uint32), np.full(m, 0xA5A5, np.uint64), np.full(m, -3.0, np.float32), np.full(m, 9, np.uint8), np.full(m, -7, np.int32))
    a = [_p(o) for o in out] if with_arrays else [None] * 5
    rc = L.hnswgpu_symmetric_graph(ix.h.handle, k, 0 if ef is None else ef, MODE_CODE[mode], cap, _p(offs), *a)
    return (rc, native._native.last_error(), offs) + out


def _untouched(out, start):
    pos, ids, dists, layers, ranks = out
    return ((pos[start:] == 0xA5A5A5A5).all() and (ids[start:] == 0xA5A5).all() and (dists[start:] == -3.0).all() and (layers[start:] == 9).all()
            and (ranks[start:] == -7).all())


def _check_all(native, ix, k, what, efs=EFS):
    """both modes and both sources against the model, through the Python method; and the host entry with room to spare: nothing is
    written behind the total"""
    for ef in efs:
        for mode in MODES:
            want = ix.want(k, ef, mode)
            _same(ix.h.symmetric_knn_graph_flat(k, ef, mode), want, f"{what} k {k} ef {ef} {mode}")
        total = int(want[0][-1])
        r = _raw(native, ix, k, ef, "mutual", total + 9)
        assert r[0] == 0, r[1]
        assert np.array_equal(r[2], want[0]) and np.array_equal(r[3][:total], want[1]) and _untouched(r[3:], total), (what, "behind the total")


# ----------------------------------------------------------------------------------------------------- 1. sizes
@pytest.mark.parametrize("n", [1, 2, 3])
def test_small_indexes(native, oracle, tmp_path, n):
    """k = 1 and k = 5 > n: D's rows hold n - 1 entries, the slots behind them write nothing"""
    ix = Index(native, oracle, tmp_path, uniform(n, 8, 10 + n))
    for k in (1, 5):
        _check_all(native, ix, k, f"n {n}")
        res, _ = ix.D(k, None)
        assert res.counts.tolist() == [min(k, n - 1)] * n
        for mode in MODES:
            g = ix.h.symmetric_knn_graph_flat(k, None, mode)
            if n < 3 or k == 5:                                 # every point names every other: the complete graph, both ways
                assert g.counts.tolist() == [n - 1] * n
    assert ix.h.symmetric_knn_graph(5) == [[(nb.d_id, nb.distance, nb.p_id) for nb in row] for row in ix.h.symmetric_knn_graph(5, None, "mutual")]
    assert [len(row) for row in ix.h.symmetric_knn_graph(5)] == [n - 1] * n


_UNIFORM = {}


def _uniform_index(native, oracle, tmp_factory, n):
    """n uniform points of dimension 8 under permuted ids 5, 8, 11, ...: built once per n and shared by the tests below"""
    if n not in _UNIFORM:
        _UNIFORM[n] = Index(native, oracle, tmp_factory.mktemp(f"u{n}"), uniform(n, 8, n), np.random.default_rng(n).permutation(n).astype(np.uint64) * 3 + 5)
    return _UNIFORM[n]


@pytest.mark.parametrize("n,k", [(63, 3), (64, 3), (65, 3), (130, 3), (257, 3), (3000, 5), (3000, 16)])
def test_wave_and_block_edges(native, oracle, tmp_path_factory, n, k):
    """one wavefront less one, one, one more; a block and a bit; 2 n k records around 256-thread blocks; many blocks"""
    _check_all(native, _uniform_index(native, oracle, tmp_path_factory, n), k, f"n {n}")


def test_counting_identities(native, oracle, tmp_path_factory):
    """total(UNION) + total(MUTUAL) = 2 sum(counts of D): a mutual pair is two slots of D, two UNION entries and two MUTUAL ones; a
    one-sided pair one slot, two UNION entries.  A MUTUAL row is no longer than its D row.  Both answers are symmetric as sets."""
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    for ef in EFS:
        res, _ = ix.D(16, ef)
        u, m = ix.h.symmetric_knn_graph_flat(16, ef, "union"), ix.h.symmetric_knn_graph_flat(16, ef, "mutual")
        assert int(u.offsets[-1]) + int(m.offsets[-1]) == 2 * int(res.counts.sum())
        assert (m.counts <= res.counts).all() and (u.counts >= res.counts).all()
        assert int(m.offsets[-1]) < int(res.counts.sum()) < int(u.offsets[-1])      # (the data has one-sided pairs: D's side)
        for g in (u, m):
            rows = np.repeat(np.arange(ix.n, dtype=np.int64), g.counts.astype(np.int64))
            edges = set(zip(rows.tolist(), g.pos.tolist()))
            assert len(edges) == len(g.pos) and all((j, i) in edges for i, j in edges) and all(i != j for i, j in edges)


# ----------------------------------------------------------------------------------------------------- 2. a hub
HUB_SEED, HUB_K = 2, 110


def hub_data(seed=HUB_SEED):
    """2000 points in 40 tight clusters of 50 around uniform centres, and point 2000 at the centroid of all of them.  Seed 2, checked
    with the f64 reference (tests/f64_reference.py: truth) when this test was written: with k = 110 a cluster point names its 49
    cluster mates, the 50 points of the nearest other cluster and 11 more -- 550 of the 2000 rows name the hub, each with a relative
    gap of at least 0.8 % between the hub's distance and its row's k-th / (k + 1)-th distance (f32 rounding is 1e-7), while the hub
    names only 110.  (Seeds 1 and 3 give 500 and 350 rows; k = 60 gives at most 200, below 4 k.)"""
    rng = np.random.default_rng(seed)
    centres = rng.random((40, 8), dtype=np.float32)
    X = np.repeat(centres, 50, axis=0) + (rng.random((2000, 8), dtype=np.float32) - np.float32(0.5)) * np.float32(0.002)
    hub = X.astype(np.float64).mean(0).astype(np.float32)
    return np.ascontiguousarray(np.vstack([X, hub[None]]).astype(np.float32))


def test_a_hub_row_is_longer_than_4k(native, oracle, tmp_path):
    ix = Index(native, oracle, tmp_path, hub_data())
    k = HUB_K
    res, pos = ix.D(k, None)
    hub = 2000                                                  # (ids are 0 .. n - 1: position = id)
    named_by = int(np.count_nonzero((pos == hub) & (np.arange(k)[None, :] < res.counts[:, None])))
    assert named_by > 4 * k and res.counts[hub] == k, named_by   # the precondition, on D
    want = ix.want(k, None, "union")
    assert int(want[0][hub + 1] - want[0][hub]) > 4 * k
    u = ix.h.symmetric_knn_graph_flat(k, None, "union")
    assert int(u.counts[hub]) > 4 * k
    _same(u, want, "hub union")
    _same(ix.h.symmetric_knn_graph_flat(k, None, "mutual"), ix.want(k, None, "mutual"), "hub mutual")
    _same(ix.h.symmetric_knn_graph_flat(k, 128, "union"), ix.want(k, 128, "union"), "hub union ef 128")


# ----------------------------------------------------------------------------------------------------- 3. duplicates
@pytest.mark.parametrize("shared", [False, True])
def test_exact_copies_and_repeated_ids(native, oracle, tmp_path, shared):
    """400 points x 3 exact copies.  Distinct DataIds: the copies of a point are three vertices at distance 0 of each other, the tie
    cut by position.  Shared DataIds: the three copies carry ONE id, and positions still name them apart."""
    base = uniform(400, 8, 31)
    perm = np.random.default_rng(32).permutation(1200)
    X = np.ascontiguousarray(np.tile(base, (3, 1))[perm])
    ids = (np.arange(1200, dtype=np.uint64) % 400 if shared else np.arange(1200, dtype=np.uint64) * 2 + 1)[perm]
    ids = np.ascontiguousarray(ids)
    ix = Index(native, oracle, tmp_path, X, ids)
    _, _, id_at, _, _ = ix.table()
    assert len(np.unique(id_at)) == (400 if shared else 1200)
    res, pos = ix.D(5, None)
    assert (res.dists[:, :2] == 0).all() and (res.dists[:, 2] > 0).all()             # on D: every point finds its two copies first
    if shared:
        assert (res.ids[:, 0] == res.ids[:, 1]).all() and (pos[:, 0] != pos[:, 1]).all()
    for k in (1, 5):                                            # k = 1: the tie between the two copies is cut by position in D itself
        _check_all(native, ix, k, f"copies shared {shared}")
    u = ix.h.symmetric_knn_graph_flat(5, None, "mutual")
    for i in (0, 599, 1199):                                    # a row starts with its two copies, ascending position
        p, d = u.of(i)[0], u.of(i)[2]
        assert d[0] == 0 and d[1] == 0 and p[0] < p[1] and i not in p.tolist()


# ----------------------------------------------------------------------------------------------------- 4. distance bits
def _metric_data(metric, n, d, seed):
    if metric in ("DistDot", "DistCosine"):
        return normalized(n, d, seed)
    if metric in ("DistHellinger", "DistJeffreys", "DistJensenShannon"):
        return positive(n, d, seed)
    return uniform(n, d, seed)


@pytest.mark.parametrize("metric", ["DistL2", "DistL1", "DistDot", "DistCosine", "DistHellinger"])
def test_symmetric_metrics_carry_equal_bits_in_both_rows(native, oracle, tmp_path, metric):
    ix = Index(native, oracle, tmp_path, _metric_data(metric, 300, 8, 0), metric=metric)
    for ef in EFS:
        u = ix.h.symmetric_knn_graph_flat(5, ef, "union")
        _same(u, ix.want(5, ef, "union"), metric)
        rows = np.repeat(np.arange(ix.n, dtype=np.int64), u.counts.astype(np.int64))
        bits = dict(zip(zip(rows.tolist(), u.pos.tolist()), u.dists.view(np.uint32).tolist()))
        assert all(bits[(j, i)] == b for (i, j), b in bits.items()), metric


@pytest.mark.parametrize("metric", ["DistJeffreys", "DistJensenShannon"])
def test_asymmetric_metrics_keep_each_rows_own_bits(native, oracle, tmp_path, metric):
    """positive data that sums to 1, seed 0 (the oracle's matrix has hundreds of mutual pairs whose directions differ at d = 8)"""
    ix = Index(native, oracle, tmp_path, _metric_data(metric, 300, 8, 0), metric=metric)
    res, pos = ix.D(5, None)
    slot = {(i, int(pos[i, s])): int(res.dists[i, s].view(np.uint32)) for i in range(ix.n) for s in range(int(res.counts[i]))}
    differing = [(i, j) for (i, j), b in slot.items() if (j, i) in slot and slot[(j, i)] != b]
    assert len(differing) >= 2, "the data must hold a pair whose two directions differ in their bits"     # on D
    for ef in EFS:
        for mode in MODES:
            _same(ix.h.symmetric_knn_graph_flat(5, ef, mode), ix.want(5, ef, mode), f"{metric} ef {ef} {mode}")
    u = ix.h.symmetric_knn_graph_flat(5, None, "union")
    rows = np.repeat(np.arange(ix.n, dtype=np.int64), u.counts.astype(np.int64))
    got = dict(zip(zip(rows.tolist(), u.pos.tolist()), u.dists.view(np.uint32).tolist()))
    for (i, j), b in got.items():                               # own row first, else the other row
        assert b == (slot[(i, j)] if (i, j) in slot else slot[(j, i)])
    i, j = differing[0]
    assert got[(i, j)] != got[(j, i)]


# ----------------------------------------------------------------------------------------------------- 5. capacity, entries
def test_capacity(native, oracle, tmp_path_factory):
    NN = native._native
    ix = _uniform_index(native, oracle, tmp_path_factory, 257)
    for ef in EFS:
        want = ix.want(3, ef, "union")
        total = int(want[0][-1])
        r = _raw(native, ix, 3, ef, "union", total - 1)
        assert r[0] == NN.ERR_CAPACITY and str(total) in r[1], r[:2]
        assert np.array_equal(r[2], want[0]) and _untouched(r[3:], 0)       # offsets complete, no out slot touched
        r = _raw(native, ix, 3, ef, "union", 0, with_arrays=False)            # count-only: NULL arrays
        assert r[0] == NN.ERR_CAPACITY and str(total) in r[1] and np.array_equal(r[2], want[0])
        r = _raw(native, ix, 3, ef, "union", total)
        assert r[0] == NN.OK, r[1]
        assert np.array_equal(r[2], want[0]) and np.array_equal(r[3], want[1]) and np.array_equal(r[4], want[2])
        assert np.array_equal(r[5].view(np.uint32), want[3]) and np.array_equal(r[6], want[4]) and np.array_equal(r[7], want[5])
    # out_ids, out_layer and out_rank may each be NULL
    L = native.lib()
    offs, pos, dists = np.zeros(258, np.uint64), np.zeros(total, np.uint32), np.zeros(total, np.float32)
    assert L.hnswgpu_symmetric_graph(ix.h.handle, 3, 32, 0, total, _p(offs), _p(pos), None, _p(dists), None, None) == NN.OK
    assert np.array_equal(pos, want[1]) and np.array_equal(dists.view(np.uint32), want[3])


def test_device_entry_on_a_stream(native, oracle, tmp_path_factory, tmp_path):
    import torch
    NN = native._native
    L = native.lib()
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    stream = torch.cuda.Stream()

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None
    for ef in EFS:
        for mode in MODES:
            want = ix.want(5, ef, mode)
            total = int(want[0][-1])
            cap = total + 5
            offs = torch.full((ix.n + 1,), -1, dtype=torch.int64, device="cuda")
            b = (torch.full((cap,), -1, dtype=torch.int32, device="cuda"), torch.full((cap,), -1, dtype=torch.int64, device="cuda"),
                 torch.full((cap,), -3.0, dtype=torch.float32, device="cuda"), torch.full((cap,), 9, dtype=torch.uint8, device="cuda"),
                 torch.full((cap,), -7, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            sp = C.c_void_p(stream.cuda_stream)
            rc = L.hnswgpu_symmetric_graph_device(ix.h.handle, 5, 0 if ef is None else ef, MODE_CODE[mode], total - 1, ptr(offs), *[ptr(t) for t in b], sp)
            assert rc == NN.ERR_CAPACITY and str(total) in NN.last_error()
            assert np.array_equal(offs.cpu().numpy().astype(np.uint64), want[0])
            assert (b[0] == -1).all() and (b[1] == -1).all() and (b[2] == -3.0).all() and (b[3] == 9).all() and (b[4] == -7).all()
            rc = L.hnswgpu_symmetric_graph_device(ix.h.handle, 5, 0 if ef is None else ef, MODE_CODE[mode], cap, ptr(offs), *[ptr(t) for t in b], sp)
            assert rc == NN.OK, NN.last_error()
            got = [t.cpu().numpy() for t in b]
            assert np.array_equal(offs.cpu().numpy().astype(np.uint64), want[0])
            assert np.array_equal(got[0][:total].view(np.uint32), want[1]) and np.array_equal(got[1][:total].astype(np.uint64), want[2])
            assert np.array_equal(got[2][:total].view(np.uint32), want[3]) and np.array_equal(got[3][:total], want[4]) and np.array_equal(got[4][:total], want[5])
            assert (got[0][total:] == -1).all() and (got[1][total:] == -1).all() and (got[2][total:] == -3.0).all() and (got[3][total:] == 9).all()
    cold = Index(native, oracle, tmp_path, uniform(65, 8, 65), upload=False)               # never uploaded
    offs = torch.zeros(66, dtype=torch.int64, device="cuda")
    rc = L.hnswgpu_symmetric_graph_device(cold.h.handle, 3, 0, 0, 0, ptr(offs), None, None, None, None, None, None)
    assert rc == NN.ERR_DEVICE and "upload" in NN.last_error()


def _bytes(res):
    return b"".join(a.tobytes() for a in (res.offsets, res.pos, res.ids, res.dists, res.layers, res.ranks))


def test_the_same_call_gives_the_same_bytes(native, oracle, tmp_path_factory, knob):
    """twice in a row; and with D arriving in many chunks (HNSWGPU_GRAPH_CHUNK = 97: 31 chunks, the last partial)"""
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    for mode in MODES:
        first = {ef: _bytes(ix.h.symmetric_knn_graph_flat(16, ef, mode)) for ef in EFS}
        for ef in EFS:
            assert _bytes(ix.h.symmetric_knn_graph_flat(16, ef, mode)) == first[ef]
        knob("HNSWGPU_GRAPH_CHUNK", 97)
        try:
            for ef in EFS:
                assert _bytes(ix.h.symmetric_knn_graph_flat(16, ef, mode)) == first[ef], (mode, ef, "chunks of 97")
        finally:
            knob("HNSWGPU_GRAPH_CHUNK", None)


def test_two_threads_on_one_handle(native, oracle, tmp_path_factory):
    ix = _uniform_index(native, oracle, tmp_path_factory, 3000)
    jobs = {"a": (5, None, "union"), "b": (16, 32, "mutual")}
    want = {name: ix.want(*j) for name, j in jobs.items()}
    out, errs = {}, []

    def run(name):
        try:
            out[name] = [ix.h.symmetric_knn_graph_flat(*jobs[name]) for _ in range(3)]
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=(name,)) for name in jobs]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    assert not errs, errs
    for name in jobs:
        for got in out[name]:
            _same(got, want[name], name)
