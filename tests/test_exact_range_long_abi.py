"""The C ABI of the screened exact range search for long rows (include/hnsw_mi355x_exact_range_long.h) where no device is needed: the
eleventh header against the registered symbols and against the hnswxr_ two it mirrors, the other headers' sets, the package's copy,
the refusals -- those of hnswxr_exact_range_search_batch(_device) as (code, message) pairs -- and the answers that need no device."""
import os

import numpy as np

from test_exact_range_screen_abi import _p

ENTRIES = ("hnswxrl_exact_range_search_batch", "hnswxrl_exact_range_search_batch_device")
MIRRORED = ("hnswxr_exact_range_search_batch", "hnswxr_exact_range_search_batch_device")


def test_header_declares_the_two_symbols(native):
    import hnsw_rs_amd._native as N
    protos = N.RANGE_LONG_HEADER.prototypes
    assert tuple(protos) == ENTRIES and tuple(N.RANGE_LONG_SYMBOLS) == ENTRIES
    sizes = [len(s) for s in (N.SYMBOLS, N.HDBSCAN_SYMBOLS, N.SELECT_SYMBOLS, N.PREDICT_SYMBOLS, N.DBSCAN_SYMBOLS, N.SCREEN_SYMBOLS,
                              N.RANGE_SCREEN_SYMBOLS, N.DBSCAN_SCREEN_SYMBOLS, N.LONG_SYMBOLS, N.GRAPH_SCREEN_SYMBOLS)]
    assert sizes == [102, 5, 2, 6, 4, 3, 2, 3, 3, 3], sizes                            # the ten other headers keep their sets
    for new, old in zip(ENTRIES, MIRRORED):
        assert getattr(native.lib(), new) is not None and not any(new in s for s in (N.SYMBOLS, N.RANGE_SCREEN_SYMBOLS))
        assert protos[new][:3] == N.RANGE_SCREEN_HEADER.prototypes[old][:3], new       # result, argument types, argument names
    assert hasattr(native.Hnsw, "exact_range_search_long_flat")
    tree = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnsw_mi355x_exact_range_long.h")
    assert N.RANGE_LONG_HEADER_PATH == tree
    assert open(os.path.join(N.PKG_DIR, "hnsw_mi355x_exact_range_long.h"), "rb").read() == open(tree, "rb").read()


def test_refusals_are_the_resident_calls_and_no_device_comes_last(native):
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

    def call(new, dev, **kw):
        a = dict(idx=h.handle, q=Q, d=8, radii=radii, allowed=None, n_allowed=0, cap=4, offs=offs, ids=ids)
        a.update(kw)
        f = getattr(L, ("hnswxrl_" if new else "hnswxr_") + "exact_range_search_batch" + ("_device" if dev else ""))
        rc = f(a["idx"], _p(a["q"]), 2, a["d"], _p(a["radii"]), _p(a["allowed"]), a["n_allowed"], a["cap"], _p(a["offs"]), _p(a["ids"]), _p(dists), None, None,
               _p(stats), *((None,) if dev else ()))
        return rc, N.last_error()

    faults = [dict(idx=None), dict(offs=None), dict(q=None), dict(radii=None), dict(ids=None), dict(d=9), dict(allowed=None, n_allowed=2),
              dict(idx=hf.handle), dict(q=None, d=9), dict(idx=hf.handle, d=9)]     # (the last two: the order of the refusals)
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
    # behind the checks: an index without a point and a call without a query need no device and screen nothing
    for hh, q in ((native.Hnsw(8, 10, 16, 32, "DistL2"), Q), (h, Q[:0])):
        (res, st), (old, old_st) = hh.exact_range_search_long_flat(q, 1.0), hh.exact_range_search_screened_flat(q, 1.0)
        assert not res.offsets.any() and len(res.ids) == 0 and st.tolist() == old_st.tolist() == [0, 0, len(q)]
        assert np.array_equal(res.offsets, old.offsets)
    # the device form asks for a resident replica; without a GPU, "no HIP device" is the last refusal of the host form
    want = call(False, True)
    assert call(True, True) == want and want[0] == N.ERR_DEVICE and "hnswgpu_upload" in want[1]
    import torch
    if not torch.cuda.is_available():
        want = call(False, False)
        assert call(True, False) == want and want[0] == N.ERR_DEVICE and "no HIP device" in want[1]
