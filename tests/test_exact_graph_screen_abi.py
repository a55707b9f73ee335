"""The C ABI of the screened exact graph (include/hnsw_mi355x_exact_graph_screen.h) where no device is needed: the tenth header against
hnswgpu_exact_graph_batch(_device), the other nine headers' sets, the package's copy, the refusals -- that call's (code, message) pairs,
nothing written -- and the "no device" answer behind them."""
import os

import numpy as np
import pytest

from test_exact_screen_abi import _N, _p, _small

ENTRIES = ("hnswxg_exact_graph_batch", "hnswxg_exact_graph_batch_device", "hnswxg_screen_matrix")


def test_header_declares_the_three_symbols_and_the_package_has_its_copy(native):
    N = _N()
    protos, old = N.GRAPH_SCREEN_HEADER.prototypes, N.HEADER.prototypes
    assert tuple(protos) == ENTRIES and tuple(N.GRAPH_SCREEN_SYMBOLS) == ENTRIES
    sizes = [len(s) for s in (N.SYMBOLS, N.HDBSCAN_SYMBOLS, N.SELECT_SYMBOLS, N.PREDICT_SYMBOLS, N.DBSCAN_SYMBOLS, N.SCREEN_SYMBOLS,
                              N.RANGE_SCREEN_SYMBOLS, N.DBSCAN_SCREEN_SYMBOLS, N.LONG_SYMBOLS)]
    assert sizes == [102, 5, 2, 6, 4, 3, 2, 3, 3], sizes                            # the other nine headers keep their sets
    for new, base in zip(ENTRIES[:2], ("hnswgpu_exact_graph_batch", "hnswgpu_exact_graph_batch_device")):
        names, args = list(old[base][2]), list(old[base][1])                        # the existing call's arguments, plus out_stats
        at = len(names) - (1 if names[-1] == "stream" else 0)
        names.insert(at, "out_stats")
        args.insert(at, protos[new][1][at])
        assert protos[new][2] == names and list(protos[new][1]) == args and protos[new][0] is old[base][0]
    assert protos[ENTRIES[2]][2] == ["idx", "point_ids", "np", "out_lb"]
    assert all(getattr(native.lib(), e) is not None and e not in N.SYMBOLS and e not in N.LONG_SYMBOLS for e in ENTRIES)
    assert hasattr(native.Hnsw, "exact_knn_graph_screened_flat") and hasattr(native.Hnsw, "exact_graph_screen_matrix")
    tree = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hnsw_mi355x_exact_graph_screen.h")
    assert N.GRAPH_SCREEN_HEADER_PATH == tree
    assert open(os.path.join(N.PKG_DIR, "hnsw_mi355x_exact_graph_screen.h"), "rb").read() == open(tree, "rb").read()


def test_refusals_are_the_existing_calls_and_no_device_comes_last(native):
    N, L = _N(), native.lib()
    h = _small(native)
    pts = np.arange(2, dtype=np.uint64)
    ids, dists, counts = np.full((2, 3), 7, np.uint64), np.full((2, 3), 7, np.float32), np.full(2, 7, np.uint32)
    stats, lb = np.full(3, 7, np.uint64), np.full((2, 50), 7, np.float32)

    def call(new, dev, **kw):
        a = dict(idx=h.handle, pts=pts, np=2, k=3, allowed=None, n_allowed=0, ids=ids)
        a.update(kw)
        f = getattr(L, ("hnswxg" if new else "hnswgpu") + "_exact_graph_batch" + ("_device" if dev else ""))
        tail = (_p(a["allowed"]), a["n_allowed"], _p(a["ids"]), _p(dists), None, None, _p(counts)) + ((_p(stats),) if new else ())
        return f(a["idx"], _p(a["pts"]), a["np"], a["k"], *tail, *((None,) if dev else ())), N.last_error()

    hf = native.Hnsw(8, 50, 16, 32, "DistL2")
    hf.parallel_insert(native.round_to_f16(np.random.default_rng(2).random((50, 8), dtype=np.float32)))
    hf.set_storage("f16")
    faults = [dict(idx=None), dict(ids=None), dict(pts=None), dict(k=0), dict(k=4097), dict(allowed=None, n_allowed=2), dict(pts=None, k=0),
              dict(np=0xFFFFFFF1), dict(idx=hf.handle)]
    for dev in (False, True):
        for kw in faults + ([] if dev else [dict(allowed=np.array([5, 2], np.uint64), n_allowed=2)]):
            old, new = call(False, dev, **kw), call(True, dev, **kw)
            assert new == old and new[0] == N.ERR_ARG, (dev, kw.keys(), old, new)
        h.set_arithmetic("simd8")
        try:
            assert call(True, dev) == call(False, dev) and "SIMD8" in N.last_error()
            assert L.hnswxg_screen_matrix(h.handle, _p(pts), 2, _p(lb)) == N.ERR_ARG and "SIMD8" in N.last_error()
        finally:
            h.set_arithmetic("scalar")
    for args, word in (((None, _p(pts), 2, _p(lb)), "null argument"), ((h.handle, _p(pts), 2, None), "null buffer"),
                       ((h.handle, None, 2, _p(lb)), "np must be nb_point = 50"), ((hf.handle, _p(pts), 2, _p(lb)), "HNSWGPU_STORAGE_F16")):
        assert L.hnswxg_screen_matrix(*args) == N.ERR_ARG and word in N.last_error(), (word, N.last_error())
    assert (ids == 7).all() and (dists == 7).all() and (counts == 7).all() and (stats == 7).all() and (lb == 7).all()
    # behind the checks: no point named and an index without a point need no device, a resident replica is asked for, "no device" last
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    r, st = e.exact_knn_graph_screened_flat(3)
    assert r.counts.shape == (0,) and st.tolist() == [0, 0, 0] and e.exact_graph_screen_matrix().shape == (0, 0)
    assert call(True, False, np=0)[0] == call(False, False, np=0)[0] == N.OK and stats.tolist() == [0, 0, 0]
    with pytest.raises(native.HnswError, match="2 of the 2 point_ids name no point"):
        e.exact_knn_graph_screened_flat(3, pts)
    assert call(True, True)[0] == N.ERR_DEVICE and "hnswgpu_upload" in N.last_error()
    import torch
    if not torch.cuda.is_available():
        for rc in (call(True, False)[0], L.hnswxg_screen_matrix(h.handle, _p(pts), 2, _p(lb))):
            assert rc == N.ERR_DEVICE and "no HIP device" in N.last_error(), N.last_error()
