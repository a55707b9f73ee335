"""The C ABI of the screened exact k-NN (include/hnsw_mi355x_exact_screen.h) where no device is needed: the header against the
registered symbols, the package's copy of the header, the refusals -- those of hnswgpu_exact_search_batch, word for word -- and the
"no device" answer behind them."""
import ctypes as C
import os

import numpy as np
import pytest

ENTRIES = ("hnswxs_exact_search_batch", "hnswxs_exact_search_batch_device", "hnswxs_screen_matrix")


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _small(native, n=50, d=8):
    h = native.Hnsw(8, n, 16, 32, "DistL2")
    h.set_build_options(nthreads=1)
    h.parallel_insert(np.random.default_rng(1).random((n, d), dtype=np.float32))
    return h


def test_header_declares_the_three_symbols(native):
    N = _N()
    protos = N.SCREEN_HEADER.prototypes
    assert tuple(protos) == ENTRIES and tuple(N.SCREEN_SYMBOLS) == ENTRIES
    assert len(N.SYMBOLS) == 102 and len(N.DBSCAN_SYMBOLS) == 4          # the other headers keep their sets
    for name in ENTRIES:
        assert protos[name][0] is C.c_int and getattr(native.lib(), name) is not None and name not in N.SYMBOLS
    old = N.HEADER.prototypes
    for new, base in ((ENTRIES[0], "hnswgpu_exact_search_batch"), (ENTRIES[1], "hnswgpu_exact_search_batch_device")):
        names, args = list(old[base][2]), list(old[base][1])             # the existing call's arguments, plus out_stats
        at = len(names) - (1 if names[-1] == "stream" else 0)
        names.insert(at, "out_stats")
        args.insert(at, protos[new][1][at])
        assert protos[new][2] == names and list(protos[new][1]) == args
    assert protos[ENTRIES[2]][2] == ["idx", "queries", "nq", "d", "out_lb"]
    assert hasattr(native.Hnsw, "exact_search_screened_flat") and hasattr(native.Hnsw, "exact_screen_matrix")


def test_package_copy_of_the_header_equals_the_tree(native):
    N = _N()
    tree = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnsw_mi355x_exact_screen.h")
    assert N.SCREEN_HEADER_PATH == tree
    assert open(os.path.join(N.PKG_DIR, "hnsw_mi355x_exact_screen.h"), "rb").read() == open(tree, "rb").read()


def test_refusals_are_the_existing_calls_and_no_device_comes_last(native):
    N, L = _N(), native.lib()
    h = _small(native)
    Q = np.zeros((2, 8), np.float32)
    ids, dists, counts = np.full((2, 3), 7, np.uint64), np.full((2, 3), 7, np.float32), np.full(2, 7, np.uint32)
    stats, lb = np.full(3, 7, np.uint64), np.full((2, 50), 7, np.float32)

    def old(dev, **kw):
        a = dict(idx=h.handle, q=Q, nq=2, d=8, k=3, allowed=None, n_allowed=0, ids=ids)
        a.update(kw)
        tail = (_p(a["allowed"]), a["n_allowed"], _p(a["ids"]), _p(dists), None, None, _p(counts))
        f = L.hnswgpu_exact_search_batch_device if dev else L.hnswgpu_exact_search_batch
        return f(a["idx"], _p(a["q"]), a["nq"], a["d"], a["k"], *tail, *((None,) if dev else ()))

    def new(dev, **kw):
        a = dict(idx=h.handle, q=Q, nq=2, d=8, k=3, allowed=None, n_allowed=0, ids=ids)
        a.update(kw)
        tail = (_p(a["allowed"]), a["n_allowed"], _p(a["ids"]), _p(dists), None, None, _p(counts), _p(stats))
        f = L.hnswxs_exact_search_batch_device if dev else L.hnswxs_exact_search_batch
        return f(a["idx"], _p(a["q"]), a["nq"], a["d"], a["k"], *tail, *((None,) if dev else ()))

    unsorted = np.array([5, 2], np.uint64)
    faults = [dict(idx=None), dict(q=None), dict(ids=None), dict(k=0), dict(k=4097), dict(d=9), dict(allowed=None, n_allowed=2), dict(k=0, d=9)]
    for dev in (False, True):
        for kw in faults + ([] if dev else [dict(allowed=unsorted, n_allowed=2)]):
            rc_old, msg_old = old(dev, **kw), N.last_error()
            rc_new, msg_new = new(dev, **kw), N.last_error()
            assert rc_new == rc_old == N.ERR_ARG and msg_new == msg_old, (dev, kw.keys(), msg_old, msg_new)
        h.set_arithmetic("simd8")
        try:
            assert new(dev) == old(dev) == N.ERR_ARG and "SIMD8" in N.last_error()
            assert L.hnswxs_screen_matrix(h.handle, _p(Q), 2, 8, _p(lb)) == N.ERR_ARG and "SIMD8" in N.last_error()
        finally:
            h.set_arithmetic("scalar")
    assert L.hnswxs_screen_matrix(h.handle, _p(Q), 2, 9, _p(lb)) == N.ERR_ARG and "dimension" in N.last_error()
    assert L.hnswxs_screen_matrix(h.handle, None, 2, 8, _p(lb)) == N.ERR_ARG
    hf = native.Hnsw(8, 50, 16, 32, "DistL2")
    hf.parallel_insert(native.round_to_f16(np.random.default_rng(2).random((50, 8), dtype=np.float32)))
    hf.set_storage("f16")
    for dev in (False, True):
        assert new(dev, idx=hf.handle) == old(dev, idx=hf.handle) == N.ERR_ARG and "HNSWGPU_STORAGE_F16" in N.last_error()
    assert L.hnswxs_screen_matrix(hf.handle, _p(Q), 2, 8, _p(lb)) == N.ERR_ARG
    assert (ids == 7).all() and (dists == 7).all() and (counts == 7).all() and (stats == 7).all() and (lb == 7).all()
    # behind the checks: an index without a point needs no device, a resident replica is asked for, and without a GPU "no device"
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    r, st = e.exact_search_screened_flat(Q, 3)
    assert r.counts.tolist() == [0, 0] and st.tolist() == [0, 0, 2]
    assert new(True) == N.ERR_DEVICE and "hnswgpu_upload" in N.last_error()
    import torch
    if not torch.cuda.is_available():
        for rc in (new(False), L.hnswxs_screen_matrix(h.handle, _p(Q), 2, 8, _p(lb))):
            assert rc == N.ERR_DEVICE and "no HIP device" in N.last_error(), N.last_error()
        with pytest.raises(native.HnswError):
            h.exact_search_screened_flat(Q, 3)
