"""The C ABI of the screened exact k-NN for long rows (include/hnsw_mi355x_exact_long.h) where no device is needed: the ninth header
against the registered symbols and against the hnswxs_ three it mirrors, the other headers' sets, the package's copy, the refusals --
those of hnswgpu_exact_search_batch as (code, message) pairs -- and the "no device" answer behind them."""
import ctypes as C
import os

import numpy as np
import pytest

from test_exact_screen_abi import _N, _p, _small

ENTRIES = ("hnswxl_exact_search_batch", "hnswxl_exact_search_batch_device", "hnswxl_screen_matrix")
MIRRORED = ("hnswxs_exact_search_batch", "hnswxs_exact_search_batch_device", "hnswxs_screen_matrix")


def test_header_declares_the_three_symbols(native):
    N = _N()
    protos = N.LONG_HEADER.prototypes
    assert tuple(protos) == ENTRIES and tuple(N.LONG_SYMBOLS) == ENTRIES
    sizes = [len(s) for s in (N.SYMBOLS, N.HDBSCAN_SYMBOLS, N.SELECT_SYMBOLS, N.PREDICT_SYMBOLS, N.DBSCAN_SYMBOLS, N.SCREEN_SYMBOLS,
                              N.RANGE_SCREEN_SYMBOLS, N.DBSCAN_SCREEN_SYMBOLS)]
    assert sizes[0] == 102 and sizes[4:] == [4, 3, 2, 3], sizes                     # the other headers keep their sets
    for new, old in zip(ENTRIES, MIRRORED):
        assert getattr(native.lib(), new) is not None and not any(new in s for s in (N.SYMBOLS, N.SCREEN_SYMBOLS, N.DBSCAN_SCREEN_SYMBOLS))
        assert protos[new][:3] == N.SCREEN_HEADER.prototypes[old][:3], new         # result, argument types, argument names
    assert hasattr(native.Hnsw, "exact_search_long_flat") and hasattr(native.Hnsw, "exact_long_matrix")


def test_package_copy_of_the_header_equals_the_tree(native):
    N = _N()
    tree = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnsw_mi355x_exact_long.h")
    assert N.LONG_HEADER_PATH == tree
    assert open(os.path.join(N.PKG_DIR, "hnsw_mi355x_exact_long.h"), "rb").read() == open(tree, "rb").read()


def test_refusals_are_the_existing_calls_and_no_device_comes_last(native):
    N, L = _N(), native.lib()
    h = _small(native)
    Q = np.zeros((2, 8), np.float32)
    ids, dists, counts = np.full((2, 3), 7, np.uint64), np.full((2, 3), 7, np.float32), np.full(2, 7, np.uint32)
    stats, lb = np.full(3, 7, np.uint64), np.full((2, 50), 7, np.float32)

    def call(new, dev, **kw):
        a = dict(idx=h.handle, q=Q, nq=2, d=8, k=3, allowed=None, n_allowed=0, ids=ids)
        a.update(kw)
        f = getattr(L, ("hnswxl" if new else "hnswgpu") + "_exact_search_batch" + ("_device" if dev else ""))
        tail = (_p(a["allowed"]), a["n_allowed"], _p(a["ids"]), _p(dists), None, None, _p(counts)) + ((_p(stats),) if new else ())
        return f(a["idx"], _p(a["q"]), a["nq"], a["d"], a["k"], *tail, *((None,) if dev else ())), N.last_error()

    faults = [dict(idx=None), dict(q=None), dict(ids=None), dict(k=0), dict(k=4097), dict(d=9), dict(allowed=None, n_allowed=2), dict(k=0, d=9)]
    hf = native.Hnsw(8, 50, 16, 32, "DistL2")
    hf.parallel_insert(native.round_to_f16(np.random.default_rng(2).random((50, 8), dtype=np.float32)))
    hf.set_storage("f16")
    for dev in (False, True):
        for kw in faults + [dict(idx=hf.handle)] + ([] if dev else [dict(allowed=np.array([5, 2], np.uint64), n_allowed=2)]):
            old, new = call(False, dev, **kw), call(True, dev, **kw)
            assert new == old and new[0] == N.ERR_ARG, (dev, kw.keys(), old, new)
        h.set_arithmetic("simd8")
        try:
            assert call(True, dev) == call(False, dev) and "SIMD8" in N.last_error()
            assert L.hnswxl_screen_matrix(h.handle, _p(Q), 2, 8, _p(lb)) == N.ERR_ARG and "SIMD8" in N.last_error()
        finally:
            h.set_arithmetic("scalar")
    for args in ((h.handle, _p(Q), 2, 9, _p(lb)), (h.handle, None, 2, 8, _p(lb)), (hf.handle, _p(Q), 2, 8, _p(lb))):
        assert (L.hnswxl_screen_matrix(*args), N.last_error()) == (L.hnswxs_screen_matrix(*args), N.last_error()) and L.hnswxl_screen_matrix(*args) == N.ERR_ARG
    assert (ids == 7).all() and (dists == 7).all() and (counts == 7).all() and (stats == 7).all() and (lb == 7).all()
    # behind the checks: an index without a point needs no device, a resident replica is asked for, and without a GPU "no device"
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    r, st = e.exact_search_long_flat(Q, 3)
    assert r.counts.tolist() == [0, 0] and st.tolist() == [0, 0, 2] and e.exact_long_matrix(Q).shape == (2, 0)
    assert call(True, True)[0] == N.ERR_DEVICE and "hnswgpu_upload" in N.last_error()
    import torch
    if not torch.cuda.is_available():
        for rc in (call(True, False)[0], L.hnswxl_screen_matrix(h.handle, _p(Q), 2, 8, _p(lb))):
            assert rc == N.ERR_DEVICE and "no HIP device" in N.last_error(), N.last_error()
        with pytest.raises(native.HnswError):
            h.exact_search_long_flat(Q, 3)
