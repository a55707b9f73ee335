"""The C ABI of the screened exact DBSCAN (include/hnsw_mi355x_dbscan_screen.h) where no device is needed: the header against the
registered symbols, the package's copy of the header, the refusals -- those of hnswdbs_exact, word for word -- and the answers that
need no device."""
import ctypes as C
import os

import numpy as np

ENTRIES = ("hnswxd_exact", "hnswxd_exact_device", "hnswxd_bounds_matrix")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_header_declares_the_three_symbols(native):
    import hnsw_rs_amd._native as N
    protos, old = N.DBSCAN_SCREEN_HEADER.prototypes, N.DBSCAN_HEADER.prototypes
    assert tuple(protos) == ENTRIES and tuple(N.DBSCAN_SCREEN_SYMBOLS) == ENTRIES
    assert (len(N.SYMBOLS), len(N.DBSCAN_SYMBOLS), len(N.SCREEN_SYMBOLS), len(N.RANGE_SCREEN_SYMBOLS)) == (102, 4, 3, 2)   # the others keep their sets
    for new, base in zip(ENTRIES, ("hnswdbs_exact", "hnswdbs_exact_device")):
        names, args = list(old[base][2]), list(old[base][1])                 # the existing call's arguments, plus out_stats
        at = len(names) - (1 if names[-1] == "stream" else 0)
        names.insert(at, "out_stats")
        args.insert(at, args[names.index("out_n_clusters")])                 # uint64_t*, like the number of clusters
        assert protos[new][0] is C.c_int and protos[new][2] == names and list(protos[new][1]) == args
    screen = N.SCREEN_HEADER.prototypes["hnswxs_screen_matrix"]               # shaped like it: one more matrix
    assert protos[ENTRIES[2]][2] == list(screen[2]) + ["out_ub"] and list(protos[ENTRIES[2]][1]) == list(screen[1]) + [screen[1][-1]]
    for name in ENTRIES:
        assert getattr(native.lib(), name) is not None and not any(name in s for s in (N.SYMBOLS, N.DBSCAN_SYMBOLS, N.RANGE_SCREEN_SYMBOLS))
    assert hasattr(native.Hnsw, "dbscan_screened") and hasattr(native.Hnsw, "dbscan_bounds_matrix")
    tree = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnsw_mi355x_dbscan_screen.h")
    assert N.DBSCAN_SCREEN_HEADER_PATH == tree
    assert open(os.path.join(N.PKG_DIR, "hnsw_mi355x_dbscan_screen.h"), "rb").read() == open(tree, "rb").read()
    assert "HNSWGPU_DBSCAN_SCREEN_CAP" in open(N.HEADER_PATH).read()


def test_refusals_are_the_existing_calls(native):
    import hnsw_rs_amd._native as N
    L = native.lib()
    h = native.Hnsw(8, 50, 16, 32, "DistL2")
    h.set_build_options(nthreads=1)
    h.parallel_insert(np.random.default_rng(1).random((50, 8), dtype=np.float32))
    hf = native.Hnsw(8, 50, 16, 32, "DistL2")
    hf.parallel_insert(native.round_to_f16(np.random.default_rng(2).random((50, 8), dtype=np.float32)))
    hf.set_storage("f16")
    label, c, stats = np.full(50, 7, np.int32), np.full(1, 7, np.uint64), np.full(4, 7, np.uint64)

    def call(screened, dev, **kw):
        a = dict(idx=h.handle, eps=0.5, ms=3, label=label, c=c)
        a.update(kw)
        name = ("hnswxd_" if screened else "hnswdbs_") + "exact" + ("_device" if dev else "")
        tail = ((_p(stats),) if screened else ()) + ((None,) if dev else ())
        rc = getattr(L, name)(a["idx"], a["eps"], a["ms"], _p(a["label"]), None, None, None, _p(a["c"]), *tail)
        return rc, N.last_error()

    for dev in (False, True):
        for kw in (dict(idx=None), dict(ms=0), dict(eps=float("nan")), dict(label=None), dict(c=None), dict(idx=hf.handle)):
            want = call(False, dev, **kw)
            assert call(True, dev, **kw) == want and want[0] == N.ERR_ARG, (dev, list(kw), want)
        h.set_arithmetic("simd8")
        try:
            want = call(False, dev)
            assert call(True, dev) == want and want[0] == N.ERR_ARG and "SIMD8" in want[1]
        finally:
            h.set_arithmetic("scalar")
    assert (label == 7).all() and (c == 7).all() and (stats == 7).all()     # nothing written by a refusal
    # behind the checks: an index without a point needs no device; the device form asks for a resident replica
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    e.parallel_insert(np.zeros((0, 8), np.float32))
    res, st = e.dbscan_screened(0.5, 3)
    assert res.n_clusters == 0 and len(res.labels) == 0 and st.tolist() == [0, 0, 0, 0]
    assert call(True, False, idx=e.handle)[0] == 0 and c[0] == 0 and stats.tolist() == [0, 0, 0, 0]
    want = call(False, True)
    assert call(True, True) == want and want[0] == N.ERR_DEVICE and "hnswgpu_upload" in want[1]
    import torch
    if not torch.cuda.is_available():
        want = call(False, False)
        assert call(True, False) == want and want[0] == N.ERR_DEVICE and "no HIP device" in want[1]
