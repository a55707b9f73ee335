"""Half-precision storage on the device (hnswgpu_set_storage(F16): rows stored as binary16, widened by the search kernels' row
loads).  binary16 -> binary32 is exact, so every search-path answer of an F16 replica is by definition the answer of the same index
at F32 -- and the yardstick is the one the suite already has: the oracle on the same dump, bit for bit (ids, f32 distance bits,
p_ids, counts, per-query work counters).  Every comparison here is exact.

Data: round_to_f16 of the suite's generators (DistDot rows normalised and THEN rounded); queries stay f32 with any values.  The
seeds are ones for which the oracle builds each index without a refused insertion (checked on the CPU when this file was written;
insert_batch raises otherwise).  tests/test_storage_abi.py checks the contract's refusals without a device."""
import ctypes as C
import threading

import numpy as np
import pytest

import f64_reference as F
from conftest import normalized, uniform
from test_gpu_counters import _device_search, _launch_lines, assert_same_counters
from test_gpu_filter_set import _assert_equal, _oracle_answers, _subset, _torch_call
from test_gpu_parity import _tie_heavy, assert_same
from test_gpu_relaunch import _assert_three_launches, _forced_bits
from test_range_search_abi import range_rule

pytestmark = pytest.mark.gpu


def _r16(native, x):
    return native.round_to_f16(x)


def _to(h, storage):
    """the handle at `storage` with a fresh replica of that kind on device 0"""
    h.set_storage(storage)
    assert h.get_storage() == storage
    h.upload(0)
    return h


# ------------------------------------------------------------------------------------------------------- 1. the routine
HALF_SPECIALS = np.array([0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14, -2.0 ** -14, 65504.0, -65504.0, 1.0], np.float32)


def _sweep_inputs(native, metric, d):
    """4 f32 queries (uniform; one representable, to be copied; one of mixed magnitudes; one with zeros) and 70 representable rows:
    rounded uniform rows, the specials of binary16 spread over the row -- its last element, the row tail, included --, an exact copy
    of a query, rows with zeros inside, a zero row"""
    rng = np.random.default_rng([11, d, F.METRICS.index(metric)])
    Q = rng.uniform(-1, 1, (4, d)).astype(np.float32)
    Q[1] = _r16(native, Q[1])
    Q[2] = (np.exp2(rng.uniform(-20, 4, d)) * rng.choice([-1.0, 1.0], d)).astype(np.float32)
    Q[3, rng.random(d) < 0.4] = 0.0
    R = _r16(native, rng.uniform(-1, 1, (70, d)).astype(np.float32))
    for j in range(20):                                        # specials at moving places, the last element always one of them
        R[j, (np.arange(len(HALF_SPECIALS)) * 7 + j) % d] = np.roll(HALF_SPECIALS, j)[:len(HALF_SPECIALS)]
        R[j, d - 1] = HALF_SPECIALS[j % len(HALF_SPECIALS)]
    R[20] = Q[1]                                               # an exact copy of a query
    R[21:29][rng.random((8, d)) < 0.5] = 0.0                   # zeros inside a row
    R[29] = 0.0
    R[30] = HALF_SPECIALS[np.arange(d) % len(HALF_SPECIALS)]   # nothing but specials
    if metric == "DistDot":                                    # its domain: |x| about 1 -- the large specials go, the small ones stay
        R[np.abs(R) > 2.0] = np.float32(0.5)
    assert native.f16_representable(R) == (0, None)
    return np.ascontiguousarray(Q), np.ascontiguousarray(R)


@pytest.mark.parametrize("metric", ["DistL2", "DistCosine", "DistDot", "DistL1"])
def test_routine_sweep(native, oracle, metric):
    """eval_distance_matrix(storage="f16") == the oracle's distances on the same f32 values, every dimension of the sweep, rows in
    batches of 1, 16, 17, 32, 33 and 64 (the lane-group branches) at the dimensions that run them all; and == storage="f32" """
    from test_gpu_f64_reference import ALL_BATCHES_D
    fails = []
    for d in F.SWEEP_D:
        Q, R = _sweep_inputs(native, metric, d)
        want = oracle.dist_matrix(metric, Q, R).view(np.uint32)
        for nf in ((1, 16, 17, 32, 33, 64) if d in ALL_BATCHES_D else (17, 64)):
            got = native.eval_distance_matrix(metric, Q, R, nf, storage="f16").view(np.uint32)
            bad = np.argwhere(got != want)
            fails += [f"d {d} batch {nf}: query {q} row {r}: {got[q, r]:#x} != {want[q, r]:#x}" for q, r in bad[:3]]
        assert np.array_equal(native.eval_distance_matrix(metric, Q, R, 17, storage="f32").view(np.uint32), want), d
        assert len(fails) < 8, fails
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------- 2. search parity
SHAPES = {  # name: dist, n, d, M, ef_c, seed
    "l2_25": ("DistL2", 4000, 25, 16, 100, 1),        # one 64-byte row
    "l2_128": ("DistL2", 3000, 128, 16, 100, 2),
    "l2_784": ("DistL2", 1200, 784, 32, 100, 3),      # rounds of 8 repeated, the longest lists
    "cos_30": ("DistCosine", 3000, 30, 16, 100, 4),   # at F32 the norm rides in the row's last chunk
    "cos_33": ("DistCosine", 3000, 33, 16, 100, 5),
    "dot_25": ("DistDot", 3000, 25, 16, 100, 6),
    "l1_100": ("DistL1", 2000, 100, 16, 100, 7),
}
EFS = (24, 100, 200, 600, 1100)                       # S = 1, 2, 4, 16; the literal-heap kernel


def _data(native, dist, n, d, seed):
    return _r16(native, normalized(n, d, seed) if dist == "DistDot" else uniform(n, d, seed))


def _queries(dist, nq, d, seed):
    return normalized(nq, d, seed) if dist == "DistDot" else uniform(nq, d, seed)


_built = {}


@pytest.fixture
def pair(native, oracle, tmp_path_factory):
    """pair(name) -> (X, oracle index, product handle reloaded from the oracle's dump, Q); built once per module"""
    def get(name):
        if name not in _built:
            dist, n, d, m, efc, seed = SHAPES[name]
            X = _data(native, dist, n, d, 500 + seed)
            o = oracle.OracleHnsw(m, n, 16, efc, dist)
            o.insert_batch(X)                                  # (raises on a refused insertion)
            tmp = tmp_path_factory.mktemp("f16_" + name)
            o.file_dump(tmp, name)
            h = native.HnswIo(tmp, name).load_hnsw(dist)
            _built[name] = (X, o, h, _queries(dist, 300, d, 600 + seed), tmp)
        X, o, h, Q, tmp = _built[name]
        h.set_strict_ties(True)
        return X, o, _to(h, "f32"), Q
    return get


def _same_bits(a, b, what):
    """two device results of one handle: answers, counts, the work counters, status and the tie flag, bit for bit"""
    assert np.array_equal(a.counts, b.counts), what
    live = np.arange(a.ids.shape[1])[None, :] < a.counts.astype(np.int64)[:, None]
    for name in ("ids", "layers", "ranks"):
        assert np.array_equal(getattr(a, name)[live], getattr(b, name)[live]), (what, name)
    assert np.array_equal(a.dists.view(np.uint32)[live], b.dists.view(np.uint32)[live]), (what, "f32 bits")
    assert np.array_equal(a.st[:, :4], b.st[:, :4]), (what, "n_dist, n_expand, n_ids_read, status")
    assert np.array_equal(a.st[:, 7] & 1, b.st[:, 7] & 1), (what, "tie flags")
    assert np.array_equal(a.st[:, 7] >> 8, b.st[:, 7] >> 8), (what, "descent counters")


@pytest.mark.parametrize("ef", EFS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_search_parity(native, pair, knob, capfd, name, ef):
    """the same handle at F32, at F16, at F32 again: strict, all three are the oracle's answer with its per-query counters; lean,
    F16 equals F32 bit for bit, tie flags and tie count included"""
    X, o, h, Q = pair(name)
    k = 10
    ref = o.parallel_search(Q, k, ef, want_counters="per_query")
    strict, lean, ties = {}, {}, {}
    for step, storage in enumerate(("f32", "f16", "f32")):
        _to(h, storage)
        knob("HNSWGPU_TRACE_LAUNCH", "1")
        capfd.readouterr()
        res = _device_search(native, h, Q, k, ef)
        lines = _launch_lines(capfd)
        knob("HNSWGPU_TRACE_LAUNCH", None)
        what = f"{name} ef {ef} {storage} (step {step})"
        assert_same(res, ref)
        assert_same_counters(res.st, ref, what)
        if ef > 1024:
            assert any("literal kernel" in ln for ln in lines), (what, lines)
        else:
            slots = 1 if ef <= 64 else 2 if ef <= 128 else 4 if ef <= 256 else 16
            assert any(f"slots {slots}," in ln for ln in lines), (what, lines)
        strict[step] = (res, h.last_tie_count())
        h.set_strict_ties(False)
        try:
            lean[step] = _device_search(native, h, Q, k, ef)
            ties[step] = h.last_tie_count()
        finally:
            h.set_strict_ties(True)
    for step in (1, 2):
        _same_bits(strict[step][0], strict[0][0], f"{name} ef {ef} strict step {step}")
        assert strict[step][1] == strict[0][1], "strict tie count"
        _same_bits(lean[step], lean[0], f"{name} ef {ef} lean step {step}")
        assert ties[step] == ties[0], "lean tie count"


def test_lazy_upload_in_front_of_a_search_makes_the_new_kind(native, pair):
    """no explicit upload after set_storage: the host-buffer search uploads the replica of the new kind itself"""
    X, o, h, Q = pair("l2_128")
    ref = o.parallel_search(Q, 10, 64)
    b32 = h.device_bytes(0)
    h.set_storage("f16")
    with pytest.raises(native.HnswError):                      # the replica is stale, like after an insert
        h.device_bytes(0)
    assert_same(h.parallel_search_flat(Q, 10, 64), ref)
    b16 = h.device_bytes(0)
    h.set_storage("f32")
    assert_same(h.parallel_search_flat(Q, 10, 64), ref)
    assert h.device_bytes(0) == b32
    # 7. the bytes: the rows halve, nothing else moves (DistL2: no norms)
    assert b32 - b16 == 3000 * 128 * 2


def test_cosine_bytes_the_norms_move_beside_the_rows(native, pair):
    """d = 30: at F32 the norm rides in the row (no side array); at F16 always beside it: rows halve, n f64 norms come"""
    X, o, h, Q = pair("cos_30")
    b32 = h.device_bytes(0)
    b16 = _to(h, "f16").device_bytes(0)
    assert b32 - b16 == 3000 * 32 * 2 - 3000 * 8


# ------------------------------------------------------------------------------------------------------- 3. ties
@pytest.mark.parametrize("kind,dist,d,ef", [("duplicates", "DistL2", 6, 32), ("grid", "DistL2", 8, 32), ("grid", "DistL1", 8, 100),
                                            ("duplicates", "DistCosine", 6, 32), ("grid", "DistL2", 8, 200)])
def test_ties(native, oracle, tmp_path, kind, dist, d, ef):
    """_tie_heavy data, rounded, every vector three times (the F16 grid at d = 8 is itself a source of ties: few distinct
    coordinates, few distinct distances): equal distances straddle position k in at least a tenth of the ORACLE's answers, and the
    strict search at F16 is the oracle's answer all the same; lean F16 == lean F32"""
    n, k = 1200, 10
    base = _r16(native, _tie_heavy(kind, n // 3, d, 77))
    X = np.ascontiguousarray(np.concatenate([base, base, base])[np.random.default_rng(5).permutation(n)])
    o = oracle.OracleHnsw(8, n, 16, 40, dist)
    o.insert_batch(X)
    o.file_dump(tmp_path, "ties")
    h = native.HnswIo(tmp_path, "ties").load_hnsw(dist)
    Q = _r16(native, _tie_heavy(kind, 200, d, 78))
    wide = o.parallel_search(Q, k + 1, max(ef, k + 1))
    straddle = (wide.counts > k) & (wide.dists[:, k - 1].view(np.uint32) == wide.dists[:, k].view(np.uint32))
    assert straddle.mean() >= 0.1, straddle.mean()
    ref = o.parallel_search(Q, k, ef, want_counters="per_query")
    res = {}
    for storage in ("f32", "f16"):
        _to(h, storage)
        r = _device_search(native, h, Q, k, ef)
        assert_same(r, ref)
        assert_same_counters(r.st, ref, f"{kind} {dist} {storage}")
        assert h.last_tie_count() > 20
        h.set_strict_ties(False)
        try:
            res[storage] = (_device_search(native, h, Q, k, ef), h.last_tie_count())
        finally:
            h.set_strict_ties(True)
    _same_bits(res["f16"][0], res["f32"][0], f"{kind} {dist} lean")
    assert res["f16"][1] == res["f32"][1] > 0


# ------------------------------------------------------------------------------------------------------- 4. driver paths
def test_one_slice_relaunch(native, oracle, tmp_path, knob, capfd):
    """HNSWGPU_BITMAP_SLICES=1 and a forced first table (the b of tests/test_gpu_relaunch.py, on its data, rounded): three launches
    of the one-query kernels on the F16 replica"""
    from test_gpu_relaunch import _spread
    X = _r16(native, _spread(4000, 16, 21))
    o = oracle.OracleHnsw(16, 4000, 16, 100, "DistL2")
    o.insert_batch(X)
    o.file_dump(tmp_path, "rl")
    h = _to(native.HnswIo(tmp_path, "rl").load_hnsw("DistL2"), "f16")
    Q = _spread(600, 16, 22)
    ref = o.parallel_search(Q, 10, 100, want_counters="per_query")
    b = _forced_bits(ref)
    knob("HNSWGPU_HASH_BITS", b)
    knob("HNSWGPU_BITMAP_SLICES", 1)
    knob("HNSWGPU_TRACE_LAUNCH", "1")
    capfd.readouterr()
    res = _device_search(native, h, Q, 10, 100)
    lines = _launch_lines(capfd)
    _, launches = h.last_kernel_ms()
    _assert_three_launches(lines, b, len(Q), launches, "f16 one slice")
    assert_same(res, ref)
    assert_same_counters(res.st, ref, "f16 one slice")


def test_exact_first_and_capped_workgroups(native, pair, knob):
    X, o, h, Q = pair("cos_33")
    _to(h, "f16")
    ref = o.parallel_search(Q, 10, 100, want_counters="per_query")
    knob("HNSWGPU_EXACT_FIRST", "1")
    res = _device_search(native, h, Q, 10, 100)
    assert_same(res, ref)
    assert_same_counters(res.st, ref, "exact first")
    knob("HNSWGPU_EXACT_FIRST", None)
    for wg in (1, 3):
        knob("HNSWGPU_MAX_WG", wg)
        res = _device_search(native, h, Q, 10, 100)
        assert_same(res, ref)
        assert_same_counters(res.st, ref, f"max wg {wg}")


def test_32_bit_cells_lean_l1_two_slots(native, oracle, tmp_path, knob, capfd):
    """The one instantiation that is built for another occupancy than its f32 twin (DistL1 on half rows, S = 2, 32-bit cells, lean:
    search_lb_waves): 66 000 points are 17 id bits, which a first table of 2^6 cells cannot keep in 16-bit cells, ef = 100 is two
    result slots per lane.  Lean F16 == lean F32 bit for bit and sound against the oracle; strict (its strict twin) == the oracle."""
    from test_gpu_counters import assert_lean_sound
    from test_gpu_relaunch import _spread
    X = _r16(native, _spread(66000, 8, 51))
    o = oracle.OracleHnsw(6, 66000, 16, 16, "DistL1")
    o.insert_batch(X)
    o.file_dump(tmp_path, "c32")
    h = native.HnswIo(tmp_path, "c32").load_hnsw("DistL1")
    Q = _spread(300, 8, 52)
    ref = o.parallel_search(Q, 10, 100, want_counters="per_query")
    knob("HNSWGPU_HASH_BITS", 6)
    lean = {}
    for storage in ("f32", "f16"):
        _to(h, storage)
        res = _device_search(native, h, Q, 10, 100)
        assert_same(res, ref)
        assert_same_counters(res.st, ref, f"cell32 strict {storage}")
        h.set_strict_ties(False)
        try:
            knob("HNSWGPU_TRACE_LAUNCH", "1")
            capfd.readouterr()
            lean[storage] = _device_search(native, h, Q, 10, 100)
            lines = _launch_lines(capfd)
            knob("HNSWGPU_TRACE_LAUNCH", None)
        finally:
            h.set_strict_ties(True)
        first = [ln for ln in lines if "visited set" in ln][0]
        assert "visited set cell32" in first and "slots 2," in first and "strict 0" in first, lines
        assert_lean_sound(lean[storage], ref, False, f"cell32 lean {storage}")
    _same_bits(lean["f16"], lean["f32"], "cell32 lean")


# ------------------------------------------------------------------------------------------------------- 5. filters
def test_filters(native, pair):
    X, o, h, Q = pair("l2_25")
    _to(h, "f16")
    Q = Q[:60]
    origin = np.arange(4000, dtype=np.uint64)
    f1, f30, none = _subset(origin, 0.01, 8), _subset(origin, 0.3, 9), np.zeros(0, np.uint64)
    for name, f in (("1 %", f1), ("30 %", f30), ("empty", none)):
        for k, ef in ((10, 48), (1, 1)):                       # (k = ef = 1: the reference's panic case)
            ref = _oracle_answers(o, Q, k, ef, [f], np.zeros(len(Q), np.uint32))
            got = h.parallel_search_filters_flat(Q, k, ef, [f], np.zeros(len(Q), np.uint32))
            _assert_equal(got, ref, f"{name} k {k} ef {ef} (set of one)")
            if not ref.status.any():
                one = h.parallel_search_filter_flat(Q, k, ef, f)
                one.status = np.zeros(len(Q), np.uint8) if one.status is None else one.status
                _assert_equal(one, ref, f"{name} k {k} ef {ef}")
    filters = [f1, f30, origin]
    filter_of = (np.arange(len(Q)) % 3).astype(np.uint32)
    ref = _oracle_answers(o, Q, 10, 100, filters, filter_of)
    _assert_equal(h.parallel_search_filters_flat(Q, 10, 100, filters, filter_of), ref, "set of three")
    import torch
    rc, a, panics = _torch_call(native, h, Q, 10, 100, filters, filter_of, torch.cuda.Stream(torch.device("cuda", 0)))
    assert rc == 0 and panics == int(ref.status.sum())
    _assert_equal(a, ref, "set of three, device entry")
    rc, a, panics = _torch_call(native, h, Q, 10, 100, [f30], filter_of, torch.cuda.Stream(torch.device("cuda", 0)), one_filter=True)
    assert rc == 0
    _assert_equal(a, _oracle_answers(o, Q, 10, 100, [f30], np.zeros(len(Q), np.uint32)), "one filter, device entry")


# ------------------------------------------------------------------------------------------------------- 6. composition
def test_range_search_composes(native, pair):
    X, o, h, Q = pair("l2_25")
    _to(h, "f16")
    Q = Q[:80]
    D = oracle_dists(o, Q, X)
    radii = np.array([np.quantile(D[i].astype(np.float64), (0.0005, 0.002, 0.01, 0.05)[i % 4]) for i in range(len(Q))]).astype(np.float32)
    radii[0::8] = 0.0
    want = range_rule(o.parallel_search, Q, radii, 8, 256)
    assert len(set(want.ef.tolist())) >= 3 and (want.counts == 0).any()
    got = h.range_search_flat(Q, radii, 8, 256)
    assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.ef, want.ef) and np.array_equal(got.flags, want.flags)
    assert np.array_equal(got.ids, want.ids) and np.array_equal(got.dists.view(np.uint32), want.dists.view(np.uint32))
    assert np.array_equal(got.layers, want.layers) and np.array_equal(got.ranks, want.ranks)


def oracle_dists(o, Q, X):
    import oracle_lib
    return oracle_lib.dist_matrix(o.dist, Q, X)


def test_ticket_pair_on_a_torch_stream(native, pair):
    import torch
    X, o, h, Q = pair("dot_25")
    _to(h, "f16")
    ref = o.parallel_search(Q, 10, 64)
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(dev)
    nq, d = Q.shape
    with torch.cuda.stream(s):
        q = torch.from_numpy(np.ascontiguousarray(Q)).to(dev)
        ids = torch.zeros((nq, 10), dtype=torch.int64, device=dev)
        dd = torch.zeros((nq, 10), dtype=torch.float32, device=dev)
        lay = torch.zeros((nq, 10), dtype=torch.uint8, device=dev)
        rk = torch.zeros((nq, 10), dtype=torch.int32, device=dev)
        cnt = torch.zeros((nq,), dtype=torch.int32, device=dev)
        st = torch.zeros((nq, 8), dtype=torch.int32, device=dev)
    s.synchronize()
    t = C.c_void_p()
    L = native.lib()
    assert L.hnswgpu_search_batch_device_begin(h.handle, q.data_ptr(), nq, d, 10, 64, ids.data_ptr(), dd.data_ptr(), lay.data_ptr(), rk.data_ptr(),
                                               cnt.data_ptr(), st.data_ptr(), s.cuda_stream, C.byref(t)) == 0 and t.value
    assert L.hnswgpu_search_batch_end(t) == 0, native._native.last_error()
    s.synchronize()
    got = type("R", (), dict(ids=ids.cpu().numpy().view(np.uint64), dists=dd.cpu().numpy(), layers=lay.cpu().numpy(), ranks=rk.cpu().numpy(),
                             counts=cnt.cpu().numpy().view(np.uint32)))
    assert_same(got, ref)


def test_two_shards_on_device_0(native, pair):
    X, o, h, Q = pair("l1_100")
    _to(h, "f16")
    ref = o.parallel_search(Q[:299], 10, 64)
    assert_same(h.parallel_search_sharded_flat(Q[:299], 10, 64, [0, 0]), ref)


def test_reference_ffi_searches_an_f16_index(native, pair, monkeypatch):
    X, o, h, Q = pair("l2_128")
    monkeypatch.chdir(_built["l2_128"][4])
    L = native.lib()
    io = L.get_hnswio(len(b"l2_128"), b"l2_128")
    api = L.load_hnswdump_f32_DistL2(io)
    assert api
    try:
        assert L.hnswgpu_set_storage(L.hnswgpu_from_api(api), 1) == 0, native._native.last_error()
        Qs = Q[:40]
        ref = o.parallel_search(Qs, 6, 30)
        ptrs = (C.c_void_p * 40)(*[Qs[i].ctypes.data for i in range(40)])
        res = L.parallel_search_neighbours_f32(api, 40, 128, ptrs, 6, 30)
        assert res and res.contents.len == 40
        for i in range(40):
            nb = res.contents.ptr[i]
            assert nb.nbgh == ref.counts[i]
            for j in range(nb.nbgh):
                assert nb.neighbours[j].id == ref.ids[i, j] and nb.neighbours[j].d == ref.dists[i, j]
        one = L.search_neighbours_f32(api, 128, Qs[3].ctypes.data, 6, 30)
        assert one and [one.contents.neighbours[j].id for j in range(one.contents.nbgh)] == ref.ids[3, :ref.counts[3]].tolist()
        L.hnswgpu_free_neighbourhood(one)
        L.hnswgpu_free_neighbourhood_vec(res)
    finally:
        L.drop_hnsw_f32(api)
        L.hnswgpu_free_hnswio(io)


def test_two_threads_on_the_f16_replica(native, pair):
    X, o, h, Q = pair("cos_30")
    _to(h, "f16")
    batches = [Q[:170], Q[130:]]
    refs = [o.parallel_search(b, 10, 48) for b in batches]
    out, errs = [None, None], []

    def work(t):
        try:
            for _ in range(3):
                out[t] = h.parallel_search_flat(batches[t], 10, 48)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    for t in range(2):
        assert_same(out[t], refs[t])


# ------------------------------------------------------------------------------------------------------- 8. insert, then search
def test_insert_then_search(native, oracle, tmp_path):
    X = _r16(native, uniform(2500, 16, 81))
    o = oracle.OracleHnsw(10, 2500, 16, 60, "DistL2")
    o.insert_batch(X[:2000])
    o.file_dump(tmp_path, "part")
    h = native.HnswIo(tmp_path, "part").load_hnsw("DistL2")
    _to(h, "f16")
    Q = uniform(100, 16, 82)
    assert_same(h.parallel_search_flat(Q, 10, 40), o.parallel_search(Q, 10, 40))
    o2 = oracle.OracleHnsw.load(tmp_path, "part", "DistL2")
    ids = np.arange(2000, 2500)
    o2.insert_batch(X[2000:], ids=ids)
    h.insert_serial(X[2000:], ids=ids)                         # the host builder, one thread
    assert h.get_nb_point() == 2500 and h.get_storage() == "f16"
    res = h.parallel_search_flat(Q, 10, 40)                    # answered by a fresh replica, of the F16 kind
    assert_same(res, o2.parallel_search(Q, 10, 40))
    assert (res.ids >= 2000).any()
    b16 = h.device_bytes(0)
    assert _to(h, "f32").device_bytes(0) - b16 == 2500 * 32 * 2


# ------------------------------------------------------------------------------------------------------- 9. refusals, device present
def test_row_readers_refuse_with_a_device_present(native, pair):
    from test_storage_abi import _row_readers
    N = native._native
    X, o, h, Q = pair("l2_25")
    _to(h, "f16")
    calls, out = _row_readers(native, h, d=25)
    for name, call in calls:
        assert call() == N.ERR_ARG, (name, N.last_error())
        assert "HNSWGPU_STORAGE_F32" in N.last_error(), (name, N.last_error())
    for o_ in out.values():
        assert (o_ == 5).all()                                 # the outputs are left poisoned
    _to(h, "f32")
    assert h.exact_search_flat(Q[:4], 5).counts.tolist() == [5] * 4     # and at F32 they answer
