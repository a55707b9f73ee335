"""The C ABI of the screened exact DBSCAN for long rows (include/hnsw_mi355x_dbscan_long.h) where no device is needed: the twelfth
header against the registered symbols and against the hnswxd_ three it mirrors, the other headers' sets, the package's copy, the
refusals -- those of hnswxd_exact(_device) as (code, message) pairs -- and the answers that need no device."""
import os

import numpy as np

from test_dbscan_screen_abi import _p

ENTRIES = ("hnswxdl_exact", "hnswxdl_exact_device", "hnswxdl_bounds_matrix")
MIRRORED = ("hnswxd_exact", "hnswxd_exact_device", "hnswxd_bounds_matrix")


def test_header_declares_the_three_symbols(native):
    import hnsw_rs_amd._native as N
    protos = N.DBSCAN_LONG_HEADER.prototypes
    assert tuple(protos) == ENTRIES and tuple(N.DBSCAN_LONG_SYMBOLS) == ENTRIES
    sizes = [len(s) for s in (N.SYMBOLS, N.HDBSCAN_SYMBOLS, N.SELECT_SYMBOLS, N.PREDICT_SYMBOLS, N.DBSCAN_SYMBOLS, N.SCREEN_SYMBOLS,
                              N.RANGE_SCREEN_SYMBOLS, N.DBSCAN_SCREEN_SYMBOLS, N.LONG_SYMBOLS, N.GRAPH_SCREEN_SYMBOLS, N.RANGE_LONG_SYMBOLS)]
    assert sizes == [102, 5, 2, 6, 4, 3, 2, 3, 3, 3, 2], sizes                          # the eleven other headers keep their sets
    for new, old in zip(ENTRIES, MIRRORED):
        assert getattr(native.lib(), new) is not None and not any(new in s for s in (N.SYMBOLS, N.DBSCAN_SCREEN_SYMBOLS))
        assert protos[new][:3] == N.DBSCAN_SCREEN_HEADER.prototypes[old][:3], new       # result, argument types, argument names
    assert hasattr(native.Hnsw, "dbscan_screened_long") and hasattr(native.Hnsw, "dbscan_long_bounds_matrix")
    tree = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnsw_mi355x_dbscan_long.h")
    assert N.DBSCAN_LONG_HEADER_PATH == tree
    assert open(os.path.join(N.PKG_DIR, "hnsw_mi355x_dbscan_long.h"), "rb").read() == open(tree, "rb").read()


def test_refusals_are_the_resident_calls_and_no_device_comes_last(native):
    import hnsw_rs_amd._native as N
    L = native.lib()
    h = native.Hnsw(8, 50, 16, 32, "DistL2")
    h.set_build_options(nthreads=1)
    h.parallel_insert(np.random.default_rng(1).random((50, 8), dtype=np.float32))
    hf = native.Hnsw(8, 50, 16, 32, "DistL2")
    hf.parallel_insert(native.round_to_f16(np.random.default_rng(2).random((50, 8), dtype=np.float32)))
    hf.set_storage("f16")
    label, c, stats = np.full(50, 7, np.int32), np.full(1, 7, np.uint64), np.full(4, 7, np.uint64)
    Q, lb, ub = np.zeros((2, 8), np.float32), np.full((2, 50), 7, np.float32), np.full((2, 50), 7, np.float32)

    def call(new, dev, **kw):
        a = dict(idx=h.handle, eps=0.5, ms=3, label=label, c=c)
        a.update(kw)
        f = getattr(L, ("hnswxdl_" if new else "hnswxd_") + "exact" + ("_device" if dev else ""))
        return f(a["idx"], a["eps"], a["ms"], _p(a["label"]), None, None, None, _p(a["c"]), _p(stats), *((None,) if dev else ())), N.last_error()

    def bounds(new, **kw):
        a = dict(idx=h.handle, q=Q, d=8, lb=lb, ub=ub)
        a.update(kw)
        return getattr(L, ("hnswxdl_" if new else "hnswxd_") + "bounds_matrix")(a["idx"], _p(a["q"]), 2, a["d"], _p(a["lb"]), _p(a["ub"])), N.last_error()

    faults = [dict(idx=None), dict(ms=0), dict(eps=float("nan")), dict(label=None), dict(c=None), dict(idx=hf.handle), dict(ms=0, label=None),
              dict(idx=hf.handle, c=None)]                                          # (the last two: the order of the refusals)
    matrix_faults = [dict(idx=None), dict(q=None), dict(lb=None), dict(ub=None), dict(d=9), dict(idx=hf.handle), dict(q=None, d=9)]
    for dev in (False, True):
        for kw in faults:
            want = call(False, dev, **kw)
            assert call(True, dev, **kw) == want and want[0] == N.ERR_ARG, (dev, list(kw), want)
    for kw in matrix_faults:
        want = bounds(False, **kw)
        assert bounds(True, **kw) == want and want[0] == N.ERR_ARG, (list(kw), want)
    h.set_arithmetic("simd8")
    try:
        for want, got in ((call(False, False), call(True, False)), (call(False, True), call(True, True)), (bounds(False), bounds(True))):
            assert got == want and want[0] == N.ERR_ARG and "SIMD8" in want[1]
    finally:
        h.set_arithmetic("scalar")
    assert all((x == 7).all() for x in (label, c, stats, lb, ub))                   # nothing written by a refusal
    # behind the checks: an index without a point needs no device and screens nothing
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    e.parallel_insert(np.zeros((0, 8), np.float32))
    res, st = e.dbscan_screened_long(0.5, 3)
    assert res.n_clusters == 0 and len(res.labels) == 0 and st.tolist() == [0, 0, 0, 0]
    assert call(True, False, idx=e.handle)[0] == 0 and c[0] == 0 and stats.tolist() == [0, 0, 0, 0]
    assert bounds(True, idx=e.handle)[0] == 0 and (lb == 7).all()
    # the device form asks for a resident replica; without a GPU, "no HIP device" is the last refusal of the host forms
    want = call(False, True)
    assert call(True, True) == want and want[0] == N.ERR_DEVICE and "hnswgpu_upload" in want[1]
    import torch
    if not torch.cuda.is_available():
        for want, got in ((call(False, False), call(True, False)), (bounds(False), bounds(True))):
            assert got == want and want[0] == N.ERR_DEVICE and "no HIP device" in want[1]
