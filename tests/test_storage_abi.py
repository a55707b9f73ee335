"""Half-precision storage (hnswgpu_set_storage, csrc/f16_storage.hpp) as far as a box without a GPU can see it: the representability
routine against numpy, every refusal of the contract, the inserts on an F16 index, the calls that read rows outside the search
path, and the dump, which stays f32.  CPU only; tests/test_gpu_f16_storage.py checks the answers of an F16 replica."""
import ctypes as C

import numpy as np
import pytest


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _api():
    import hnsw_rs_amd.api as A
    return A


def _numpy_bad(x):
    """what numpy says is NOT representable: NaN, or the round trip through float16 changes a bit"""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        back = x.astype(np.float16).astype(np.float32)
    return np.isnan(x) | (back.view(np.uint32) != x.view(np.uint32))


def _check_against_numpy(x):
    A = _api()
    want = _numpy_bad(x)
    bad, first = A.f16_representable(x)
    assert bad == int(want.sum())
    assert first == (int(np.flatnonzero(want)[0]) if want.any() else None)
    return want


ALL_HALVES = np.arange(65536, dtype=np.uint16).view(np.float16).astype(np.float32)


def test_every_half_is_representable_except_the_nans(native):
    want = _check_against_numpy(ALL_HALVES)
    assert int(want.sum()) == int(np.isnan(ALL_HALVES).sum()) == 2 * 1023
    finite = ALL_HALVES[~np.isnan(ALL_HALVES)]
    assert _api().f16_representable(finite) == (0, None)     # +-0, the subnormals, +-65504, +-inf among them


@pytest.mark.parametrize("step", [1, -1])
def test_one_f32_ulp_beside_every_half(native, step):
    bits = ALL_HALVES.view(np.uint32).astype(np.int64) + step
    x = (bits & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    want = _check_against_numpy(x)
    assert want.sum() > 60000                                # (a neighbour of a half is a half only around zero / NaN patterns)
    # element by element too, on a part: the count alone could hide two errors that cancel
    A = _api()
    for i in range(0, 65536, 257):
        assert (A.f16_representable(x[i:i + 1])[0] == 1) == bool(want[i]), (i, x[i])


def test_a_million_random_bit_patterns(native):
    x = np.random.default_rng(5).integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32).view(np.float32)
    want = _check_against_numpy(x)
    assert 0 < (~want).sum() < want.sum()
    # and the count splits over any cut
    A = _api()
    assert A.f16_representable(x[:1000])[0] + A.f16_representable(x[1000:])[0] == int(want.sum())


def test_round_to_f16_is_always_representable(native):
    A = _api()
    rng = np.random.default_rng(6)
    x = np.concatenate([rng.standard_normal(100000).astype(np.float32) * np.float32(50.0),
                        rng.random(1000, dtype=np.float32) * np.float32(1e-6),     # into the subnormals and to zero
                        np.array([1e9, -1e9, 65519.9, 65520.0, 0.0, -0.0, np.inf, -np.inf], np.float32)])
    r = A.round_to_f16(x.reshape(-1, 8))
    assert r.dtype == np.float32 and r.flags.c_contiguous and r.shape == (len(x) // 8, 8)
    assert A.f16_representable(r) == (0, None)
    assert A.f16_representable(x)[0] > 90000
    assert np.array_equal(A.round_to_f16(r).view(np.uint32), r.view(np.uint32))   # idempotent


def _built(native, dist="DistL2", n=60, d=8, seed=1, rounded=True):
    A = _api()
    X = np.random.default_rng(seed).random((n, d), dtype=np.float32)
    if dist in ("DistHellinger", "DistJeffreys", "DistJensenShannon"):
        X = np.ascontiguousarray(X / X.sum(1, dtype=np.float32)[:, None])
    if rounded:
        X = A.round_to_f16(X)
    h = native.Hnsw(8, n, 16, 32, dist)
    h.set_build_options(nthreads=1)
    h.parallel_insert(X, ids=np.arange(1000, 1000 + n, dtype=np.uint64))
    return X, h


def _raises_arg(native, fn, *words):
    with pytest.raises(native.HnswError) as e:
        fn()
    assert e.value.code == _N().ERR_ARG, e.value
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_default_and_round_trip(native):
    X, h = _built(native)
    assert h.get_storage() == "f32"
    h.set_storage("f16")
    assert h.get_storage() == "f16"
    h.set_storage("f16")
    h.set_storage("f32")                                     # always allowed
    assert h.get_storage() == "f32"


def test_unknown_storage(native):
    N = _N()
    X, h = _built(native)
    assert native.lib().hnswgpu_set_storage(h.handle, 2) == N.ERR_ARG and "unknown storage" in N.last_error()
    assert native.lib().hnswgpu_set_storage(h.handle, -1) == N.ERR_ARG
    assert native.lib().hnswgpu_set_storage(None, 1) == N.ERR_ARG
    assert h.get_storage() == "f32"


@pytest.mark.parametrize("dist", ["DistHellinger", "DistJeffreys", "DistJensenShannon"])
def test_probability_metrics_are_refused(native, dist):
    X, h = _built(native, dist)
    _raises_arg(native, lambda: h.set_storage("f16"), "DistL2")
    assert h.get_storage() == "f32"


@pytest.mark.parametrize("dist", ["DistL2", "DistCosine", "DistDot", "DistL1"])
def test_the_four_metrics_are_accepted(native, dist):
    X, h = _built(native, dist)
    h.set_storage("f16")
    assert h.get_storage() == "f16"


def test_simd8_and_f16_exclude_each_other(native):
    X, h = _built(native)
    h.set_arithmetic("simd8")
    _raises_arg(native, lambda: h.set_storage("f16"), "SIMD8")
    assert h.get_storage() == "f32"
    h.set_arithmetic("scalar")
    h.set_storage("f16")
    _raises_arg(native, lambda: h.set_arithmetic("simd8"), "STORAGE_F16")
    h.set_arithmetic("scalar")                               # the scalar arithmetic is what an F16 index runs
    h.set_storage("f32")
    h.set_arithmetic("simd8")                                # and back at F32 the other one is allowed again


def test_a_non_representable_element_names_its_point(native):
    A = _api()
    X, h = _built(native, n=60, d=8, rounded=True)
    Y = X.copy()
    Y[37, 5] = np.float32(0.1)                               # not a half
    Y[37, 6] = np.float32(1e-9)
    Y[50, 0] = np.float32(70000.0)
    assert A.f16_representable(Y) == (3, 37 * 8 + 5)
    g = native.Hnsw(8, 60, 16, 32, "DistL2")
    g.set_build_options(nthreads=1)
    g.parallel_insert(Y, ids=np.arange(1000, 1060, dtype=np.uint64))
    # the scan runs in dump order (layer by layer), so which bad point comes FIRST depends on the levels: name it from the dump's
    # own order -- the point whose bad element the message names must be one of the two, with its own dimension
    with pytest.raises(native.HnswError) as e:
        g.set_storage("f16")
    msg = str(e.value)
    assert e.value.code == _N().ERR_ARG
    assert "3 vector elements" in msg
    assert ("DataId 1037" in msg and "dimension 5" in msg) or ("DataId 1050" in msg and "dimension 0" in msg), msg
    assert g.get_storage() == "f32"
    # one bad point only: no choice left
    Z = X.copy()
    Z[12, 7] = np.float32(np.nan)
    g = native.Hnsw(8, 60, 16, 32, "DistL2")
    g.set_build_options(nthreads=1)
    g.parallel_insert(Z, ids=np.arange(1000, 1060, dtype=np.uint64))
    _raises_arg(native, lambda: g.set_storage("f16"), "1 vector elements", "DataId 1012", "dimension 7")
    assert g.get_storage() == "f32"


def test_inserts_on_an_f16_index(native):
    A = _api()
    N = _N()
    X, h = _built(native)
    h.set_storage("f16")
    n0 = h.get_nb_point()
    more = A.round_to_f16(np.random.default_rng(9).random((10, 8), dtype=np.float32))
    bad = more.copy()
    bad[4, 2] = np.float32(1.0) / np.float32(3.0)
    ids = np.arange(5000, 5010, dtype=np.uint64)
    _raises_arg(native, lambda: h.parallel_insert(bad, ids=ids), "DataId 5004", "dimension 2", "nothing was inserted")
    assert h.get_nb_point() == n0
    _raises_arg(native, lambda: h.insert_serial(bad, ids=ids), "DataId 5004")
    assert h.get_nb_point() == n0
    # the GPU-assisted insert checks before it looks for a device
    rc = native.lib().hnswgpu_insert_gpu(h.handle, _p(bad), 10, 8, _p(ids), 1, 0, 0)
    assert rc == N.ERR_ARG and "DataId 5004" in N.last_error()
    assert h.get_nb_point() == n0
    # representable vectors go in
    h.parallel_insert(more, ids=ids)
    assert h.get_nb_point() == n0 + 10
    assert h.get_storage() == "f16"
    # at F32 the same vectors are no one's business
    h.set_storage("f32")
    h.parallel_insert(bad, ids=ids + 100)
    assert h.get_nb_point() == n0 + 20
    _raises_arg(native, lambda: h.set_storage("f16"), "DataId 5104", "dimension 2")


def test_ffi_inserts_on_an_f16_index_log_and_insert_nothing(native):
    """insert_f32 / parallel_insert_f32 return nothing: the refusal is readable through hnswgpu_last_error"""
    A = _api()
    N = _N()
    L = native.lib()
    api = L.new_hnsw_f32(8, 32, 6, b"DistL2", 100, 16)
    assert api
    try:
        idx = L.hnswgpu_from_api(api)
        good = A.round_to_f16(np.random.default_rng(3).random((12, 8), dtype=np.float32))
        bad = good.copy()
        bad[4, 2] = np.float32(1.0) / np.float32(3.0)
        for i in range(4):
            L.insert_f32(api, 8, _p(np.ascontiguousarray(good[i])), 100 + i)
        assert L.hnswgpu_nb_point(idx) == 4
        assert L.hnswgpu_set_storage(idx, N.HEADER.constants["HNSWGPU_STORAGE_F16"]) == N.OK
        L.insert_f32(api, 8, _p(np.ascontiguousarray(bad[4])), 7000)
        assert "DataId 7000" in N.last_error() and "dimension 2" in N.last_error() and L.hnswgpu_nb_point(idx) == 4
        ptrs = (C.c_void_p * 12)(*[bad[i].ctypes.data for i in range(12)])
        ffi_ids = (C.c_size_t * 12)(*range(8000, 8012))
        L.parallel_insert_f32(api, 12, 8, ptrs, ffi_ids)
        assert "DataId 8004" in N.last_error() and L.hnswgpu_nb_point(idx) == 4
        ptrs = (C.c_void_p * 12)(*[good[i].ctypes.data for i in range(12)])
        L.parallel_insert_f32(api, 12, 8, ptrs, ffi_ids)
        assert L.hnswgpu_nb_point(idx) == 16
        L.insert_f32(api, 8, _p(np.ascontiguousarray(good[5])), 7001)
        assert L.hnswgpu_nb_point(idx) == 17 and L.hnswgpu_get_storage(idx) == 1
    finally:
        L.drop_hnsw_f32(api)


def _row_readers(native, h, d=8):
    """the entries that read rows outside the search path, host and device forms, as (name, call); outputs poisoned"""
    L = native.lib()
    q = np.zeros((3, d), np.float32)
    rad = np.ones(3, np.float32)
    pts = np.array([1000, 1001, 1002], np.uint64)
    fo = np.zeros(3, np.uint32)
    fids, foffs = np.array([1000, 1001], np.uint64), np.array([0, 2], np.uint64)
    out = dict(oi=np.full(30, 5, np.uint64), od=np.full(30, 5, np.float32), oc=np.full(3, 5, np.uint32), oo=np.full(4, 5, np.uint64))
    oi, od, oc, oo = (_p(out[k]) for k in ("oi", "od", "oc", "oo"))
    H = h.handle
    calls = [
        ("exact_search_batch", lambda: L.hnswgpu_exact_search_batch(H, _p(q), 3, d, 10, None, 0, oi, od, None, None, oc)),
        ("exact_search_batch_device", lambda: L.hnswgpu_exact_search_batch_device(H, _p(q), 3, d, 10, None, 0, oi, od, None, None, oc, None)),
        ("exact_search_batch_filter_set", lambda: L.hnswgpu_exact_search_batch_filter_set(H, _p(q), 3, d, 10, _p(fids), _p(foffs), 1, _p(fo), oi, od,
                                                                                          None, None, oc)),
        ("exact_search_batch_filter_set_device", lambda: L.hnswgpu_exact_search_batch_filter_set_device(H, _p(q), 3, d, 10, _p(fids), _p(foffs), 1,
                                                                                                        _p(fo), oi, od, None, None, oc, None)),
        ("exact_range_search_batch", lambda: L.hnswgpu_exact_range_search_batch(H, _p(q), 3, d, _p(rad), None, 0, 30, oo, oi, od, None, None)),
        ("exact_range_search_batch_device", lambda: L.hnswgpu_exact_range_search_batch_device(H, _p(q), 3, d, _p(rad), None, 0, 30, oo, oi, od, None,
                                                                                              None, None)),
        ("exact_graph_batch", lambda: L.hnswgpu_exact_graph_batch(H, _p(pts), 3, 10, None, 0, oi, od, None, None, oc)),
        ("exact_graph_batch_device", lambda: L.hnswgpu_exact_graph_batch_device(H, _p(pts), 3, 10, None, 0, oi, od, None, None, oc, None)),
        ("graph_search_batch", lambda: L.hnswgpu_graph_search_batch(H, _p(pts), 3, 10, 32, oi, od, None, None, oc)),
        ("graph_search_batch_device", lambda: L.hnswgpu_graph_search_batch_device(H, _p(pts), 3, 10, 32, oi, od, None, None, oc, None)),
    ]
    return calls, out


def test_the_row_readers_refuse_an_f16_index(native):
    """HNSWGPU_ERR_ARG from all of them, host and device forms, before the device check (this box may have none) and with the
    outputs untouched; the message says what to do; back at F32 the same calls get past the argument checks"""
    N = _N()
    X, h = _built(native)
    h.set_storage("f16")
    calls, out = _row_readers(native, h)
    for name, call in calls:
        assert call() == N.ERR_ARG, (name, N.last_error())
        assert "HNSWGPU_STORAGE_F16" in N.last_error() and "HNSWGPU_STORAGE_F32" in N.last_error(), (name, N.last_error())
    for o in out.values():
        assert (o == 5).all()
    for m in (lambda: h.exact_search_flat(X[:3], 5), lambda: h.exact_range_search_flat(X[:3], 0.5), lambda: h.exact_knn_graph_flat(3),
              lambda: h.knn_graph_flat(3, 32)):
        _raises_arg(native, m, "HNSWGPU_STORAGE_F16")
    h.set_storage("f32")
    if native.lib().hnswgpu_device_count() == 0:
        for name, call in calls:
            assert call() == N.ERR_DEVICE, (name, N.last_error())


def test_device_bytes_needs_a_resident_replica(native):
    N = _N()
    X, h = _built(native)
    n = C.c_uint64(7)
    assert native.lib().hnswgpu_device_bytes(h.handle, 0, None) == N.ERR_ARG
    if native.lib().hnswgpu_device_count() == 0:
        assert native.lib().hnswgpu_device_bytes(h.handle, 0, C.byref(n)) == N.ERR_DEVICE and n.value == 7
        with pytest.raises(native.HnswError) as e:
            h.device_bytes()
        assert e.value.code == N.ERR_DEVICE


def test_eval_hook_refuses_what_a_half_cannot_hold(native):
    A = _api()
    N = _N()
    q = np.ones((2, 8), np.float32)
    rows = A.round_to_f16(np.random.default_rng(2).random((4, 8), dtype=np.float32))
    rows[2, 3] = np.float32(0.1)
    with pytest.raises(native.HnswError) as e:
        native.eval_distance_matrix("DistL2", q, rows, 4, storage="f16")
    assert e.value.code == N.ERR_ARG and "element 3 of row 2" in str(e.value)
    with pytest.raises(native.HnswError) as e:
        native.eval_distance_matrix("DistHellinger", q, A.round_to_f16(rows), 4, storage="f16")
    assert e.value.code == N.ERR_ARG
    with pytest.raises(native.HnswError) as e:
        native.eval_distance_matrix("DistL2", q, A.round_to_f16(rows), 4, arithmetic="simd8", storage="f16")
    assert e.value.code == N.ERR_ARG
    out = np.zeros((2, 4), np.float32)
    good = A.round_to_f16(rows)
    assert native.lib().hnswgpu_eval_distance_matrix_storage(N.DIST["DistL2"], 3, _p(q), 2, _p(good), 4, 8, 4, _p(out)) == N.ERR_ARG


R128_ONLY = "HNSWGPU_EVAL_R128 serves DistL2 on HNSWGPU_STORAGE_F32 rows of 97 .. 128 elements only"
VARIANT_REFUSALS = [  # dist, storage, variant bits, d, the complete message
    ("DistL2", 0, 1 | 2, 128, "HNSWGPU_EVAL_DEEP with HNSWGPU_EVAL_PIPE: no search kernel has both"),
    ("DistL2", 0, 1 | 2 | 4, 128, "HNSWGPU_EVAL_DEEP with HNSWGPU_EVAL_PIPE: no search kernel has both"),
    ("DistL2", 0, 2 | 4, 128, "HNSWGPU_EVAL_R128 with HNSWGPU_EVAL_PIPE: no search kernel has both"),
    ("DistL2", 0, 8, 128, "unknown variant bits: HNSWGPU_EVAL_DEEP, HNSWGPU_EVAL_PIPE and HNSWGPU_EVAL_R128 are defined"),
    ("DistL2", 0, 8 | 1, 128, "unknown variant bits: HNSWGPU_EVAL_DEEP, HNSWGPU_EVAL_PIPE and HNSWGPU_EVAL_R128 are defined"),
    ("DistL2", 0, -1, 128, "unknown variant bits: HNSWGPU_EVAL_DEEP, HNSWGPU_EVAL_PIPE and HNSWGPU_EVAL_R128 are defined"),
    ("DistL2", 0, 4, 96, R128_ONLY),
    ("DistL2", 0, 4, 129, R128_ONLY),
    ("DistL2", 0, 4 | 1, 96, R128_ONLY),
    ("DistL2", 1, 4, 128, R128_ONLY),
    ("DistL1", 0, 4, 128, R128_ONLY),
    ("DistCosine", 0, 4 | 1, 100, R128_ONLY),
    ("DistL2", 3, 1, 128, "unknown storage"),
    ("DistHellinger", 1, 2, 128, "HNSWGPU_STORAGE_F16 serves DistL2, DistCosine, DistDot and DistL1 only"),
]


@pytest.mark.parametrize("dist, storage, variant, d, msg", VARIANT_REFUSALS)
def test_eval_variant_refusals(native, dist, storage, variant, d, msg):
    """hnswgpu_eval_distance_matrix_variant: the combinations no search kernel has are HNSWGPU_ERR_ARG with their message -- checked in
    front of the device, so without one too -- and the output is not touched: never the plain routine in a variant's place"""
    N = _N()
    q = np.ones((2, d), np.float32)
    rows = _api().round_to_f16(np.random.default_rng(3).random((4, d), dtype=np.float32))
    out = np.full((2, 4), np.float32(-7.0))
    rc = native.lib().hnswgpu_eval_distance_matrix_variant(N.DIST[dist], storage, variant, _p(q), 2, _p(rows), 4, d, 4, _p(out))
    assert rc == N.ERR_ARG and N.last_error() == msg
    assert np.all(out == np.float32(-7.0))


def test_eval_variant_argument_checks_and_python_names(native):
    N, A = _N(), _api()
    assert A.EVAL_VARIANT == {"plain": 0, "deep": 1, "pipe": 2, "r128": 4, "deep+r128": 5}
    assert (N.HEADER.constants["HNSWGPU_EVAL_DEEP"], N.HEADER.constants["HNSWGPU_EVAL_PIPE"], N.HEADER.constants["HNSWGPU_EVAL_R128"]) == (1, 2, 4)
    q, rows, out = np.ones((2, 128), np.float32), np.ones((4, 128), np.float32), np.zeros((2, 4), np.float32)
    call = native.lib().hnswgpu_eval_distance_matrix_variant
    for args in ((None, 2, _p(rows), 4, 128, 4, _p(out)), (_p(q), 2, None, 4, 128, 4, _p(out)), (_p(q), 2, _p(rows), 4, 128, 4, None)):
        assert call(N.DIST["DistL2"], 0, 1, *args) == N.ERR_ARG and N.last_error() == "bad argument"
    assert call(7, 0, 1, _p(q), 2, _p(rows), 4, 128, 4, _p(out)) == N.ERR_ARG
    # the half-storage scan runs for a variant as it does without one
    rows[2, 3] = np.float32(0.1)
    with pytest.raises(native.HnswError) as e:
        native.eval_distance_matrix("DistL2", q, rows, 4, storage="f16", variant="pipe")
    assert e.value.code == N.ERR_ARG and "element 3 of row 2" in str(e.value)
    # the Python wrapper: scalar arithmetic only, the names of the table only
    with pytest.raises(native.HnswError) as e:
        native.eval_distance_matrix("DistL2", q, np.ones((4, 128), np.float32), 4, arithmetic="simd8", variant="deep")
    assert e.value.code == N.ERR_ARG
    with pytest.raises(KeyError):
        native.eval_distance_matrix("DistL2", q, np.ones((4, 128), np.float32), 4, variant="deep+pipe")
    # a well-formed variant call gets as far as the device: with none it answers "no device", it does not compute on the host
    if native.lib().hnswgpu_device_count() == 0:
        for variant in ("deep", "pipe", "r128", "deep+r128"):
            with pytest.raises(native.HnswError) as e:
                native.eval_distance_matrix("DistL2", q, np.ones((4, 128), np.float32), 4, variant=variant)
            assert e.value.code == N.ERR_DEVICE


def test_file_dump_of_an_f16_index_is_the_f32_dump(native, tmp_path):
    X, h = _built(native, "DistCosine", n=80, d=9)
    h.file_dump(tmp_path, "a32")
    h.set_storage("f16")
    h.file_dump(tmp_path, "a16")
    for ext in (".hnsw.graph", ".hnsw.data"):
        assert (tmp_path / ("a16" + ext)).read_bytes() == (tmp_path / ("a32" + ext)).read_bytes(), ext
    # a reloaded dump starts at F32 again, and takes F16 as the index that wrote it did
    g = native.HnswIo(tmp_path, "a16").load_hnsw("DistCosine")
    assert g.get_storage() == "f32"
    g.set_storage("f16")
    assert g.get_storage() == "f16"
