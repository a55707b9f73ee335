"""The C ABI of the screened exact range search (include/hnsw_mi355x_exact_range_screen.h) where no device is needed: the header
against the registered symbols, the package's copy of the header, the refusals -- those of hnswgpu_exact_range_search_batch, word for
word -- and the answers that need no device."""
import ctypes as C
import os

import numpy as np

ENTRIES = ("hnswxr_exact_range_search_batch", "hnswxr_exact_range_search_batch_device")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def test_header_declares_the_two_symbols(native):
    import hnsw_rs_amd._native as N
    protos, old = N.RANGE_SCREEN_HEADER.prototypes, N.HEADER.prototypes
    assert tuple(protos) == ENTRIES and tuple(N.RANGE_SCREEN_SYMBOLS) == ENTRIES
    assert len(N.SYMBOLS) == 102 and len(N.SCREEN_SYMBOLS) == 3 and len(N.DBSCAN_SYMBOLS) == 4     # the other headers keep their sets
    for new, base in zip(ENTRIES, ("hnswgpu_exact_range_search_batch", "hnswgpu_exact_range_search_batch_device")):
        names, args = list(old[base][2]), list(old[base][1])                 # the existing call's arguments, plus out_stats
        at = len(names) - (1 if names[-1] == "stream" else 0)
        names.insert(at, "out_stats")
        args.insert(at, args[names.index("out_offsets" if "out_offsets" in names else "d_out_offsets")])     # uint64_t*, like the offsets
        assert protos[new][0] is C.c_int and protos[new][2] == names and list(protos[new][1]) == args
        assert getattr(native.lib(), new) is not None and new not in N.SYMBOLS
    assert hasattr(native.Hnsw, "exact_range_search_screened_flat")
    tree = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnsw_mi355x_exact_range_screen.h")
    assert N.RANGE_SCREEN_HEADER_PATH == tree
    assert open(os.path.join(N.PKG_DIR, "hnsw_mi355x_exact_range_screen.h"), "rb").read() == open(tree, "rb").read()
    hooks = open(N.HEADER_PATH).read()
    assert "HNSWGPU_RANGE_SCREEN_CAP" in hooks and "HNSWGPU_RANGE_SCREEN_TILES" in hooks


def test_refusals_are_the_existing_calls(native):
    import hnsw_rs_amd._native as N
    L = native.lib()
    h = native.Hnsw(8, 50, 16, 32, "DistL2")
    h.set_build_options(nthreads=1)
    h.parallel_insert(np.random.default_rng(1).random((50, 8), dtype=np.float32))
    hf = native.Hnsw(8, 50, 16, 32, "DistL2")
    hf.parallel_insert(native.round_to_f16(np.random.default_rng(2).random((50, 8), dtype=np.float32)))
    hf.set_storage("f16")
    Q, radii = np.zeros((2, 8), np.float32), np.ones(2, np.float32)
    offs, ids, dists, stats = np.full(3, 7, np.uint64), np.full(4, 7, np.uint64), np.full(4, 7, np.float32), np.full(3, 7, np.uint64)

    def call(screened, dev, **kw):
        a = dict(idx=h.handle, q=Q, d=8, radii=radii, allowed=None, n_allowed=0, cap=4, offs=offs, ids=ids)
        a.update(kw)
        name = ("hnswxr_" if screened else "hnswgpu_") + "exact_range_search_batch" + ("_device" if dev else "")
        tail = ((_p(stats),) if screened else ()) + ((None,) if dev else ())
        rc = getattr(L, name)(a["idx"], _p(a["q"]), 2, a["d"], _p(a["radii"]), _p(a["allowed"]), a["n_allowed"], a["cap"], _p(a["offs"]), _p(a["ids"]),
                              _p(dists), None, None, *tail)
        return rc, N.last_error()

    faults = [dict(idx=None), dict(offs=None), dict(q=None), dict(radii=None), dict(ids=None), dict(d=9), dict(allowed=None, n_allowed=2),
              dict(idx=hf.handle)]
    for dev in (False, True):
        for kw in faults + ([] if dev else [dict(allowed=np.array([5, 2], np.uint64), n_allowed=2)]):
            want = call(False, dev, **kw)
            assert call(True, dev, **kw) == want and want[0] == N.ERR_ARG, (dev, list(kw), want)
        h.set_arithmetic("simd8")
        try:
            want = call(False, dev)
            assert call(True, dev) == want and want[0] == N.ERR_ARG and "SIMD8" in want[1]
        finally:
            h.set_arithmetic("scalar")
    assert (offs == 7).all() and (ids == 7).all() and (dists == 7).all() and (stats == 7).all()     # nothing written by a refusal
    # behind the checks: an index without a point needs no device; the device form asks for a resident replica
    res, st = native.Hnsw(8, 10, 16, 32, "DistL2").exact_range_search_screened_flat(Q, 1.0)
    assert res.offsets.tolist() == [0, 0, 0] and st.tolist() == [0, 0, 2]
    want = call(False, True)
    assert call(True, True) == want and want[0] == N.ERR_DEVICE and "hnswgpu_upload" in want[1]
    import torch
    if not torch.cuda.is_available():
        want = call(False, False)
        assert call(True, False) == want and want[0] == N.ERR_DEVICE and "no HIP device" in want[1]
