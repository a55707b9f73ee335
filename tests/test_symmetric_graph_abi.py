"""The symmetrised k-NN graph entries (hnswgpu_symmetric_graph / _device, csrc/symmetric_graph.hip) as far as a box without a GPU
can see them: the ABI, every argument check that is answered before a device is needed, the empty index -- and `symmetrise`, the
contract restated in Python over ANY directed graph D given as rows of neighbour positions and f32 distances.
tests/test_gpu_symmetric_graph.py imports symmetrise and position_table to build its expected answers from the existing public graph
calls, never from the code under test.  Here the model is checked on hand-made graphs.  CPU only."""
import ctypes as C

import numpy as np
import pytest

ENTRIES = ("hnswgpu_symmetric_graph", "hnswgpu_symmetric_graph_device")


def _N():
    import hnsw_rs_amd._native as N
    return N


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


# ----------------------------------------------------------------------------------------------------- the model
def order_key(dist):
    """the exact k-NN key's upper half: the distance as an f32 value, -0 folded into +0, NaN last (then the position decides)"""
    v = np.float32(dist)
    if np.isnan(v):
        return (1, 0.0)
    return (0, float(v) + 0.0)


def position_table(layer_sizes, ids, layers, ranks):
    """pos_of_flat for an index whose EVERY point is listed once as (DataId, layer, rank): flat id = the points of the layers below
    + rank (dump order); position = place in the ascending (DataId, dump order) order.  positions[layer_offset[l] + r] is the
    position of p_id (l, r); the second result is layer_offset."""
    layer_offset = np.concatenate([[0], np.cumsum(layer_sizes)]).astype(np.int64)
    n = int(layer_offset[-1])
    flat = layer_offset[np.asarray(layers, np.int64)] + np.asarray(ranks, np.int64)
    assert len(flat) == n and np.array_equal(np.sort(flat), np.arange(n))
    id_of = np.zeros(n, np.uint64)
    id_of[flat] = ids
    order = np.lexsort((np.arange(n), id_of))
    pos_of_flat = np.empty(n, np.int64)
    pos_of_flat[order] = np.arange(n)
    return pos_of_flat, layer_offset


def symmetrise(n, counts, pos, dists, mode):
    """The contract: D's row i holds pos[i, :counts[i]] at distances dists[i, :counts[i]] (f32).  Returns (offsets u64, cols,
    dist bits u32, source rows, source slots): entry (i, j) of the answer with the bits of D's slot (source row, source slot) --
    i's own slot when i -> j, else j's slot for i.  Rows ascend by (distance value with -0 = +0 and NaN last, position)."""
    fwd = [dict() for _ in range(n)]
    for i in range(n):
        for s in range(int(counts[i])):
            j = int(pos[i, s])
            assert j != i and j not in fwd[i]
            fwd[i][j] = s
    named_by = [[] for _ in range(n)]                              # named_by[i]: the rows j with j -> i
    for j in range(n):
        for i in fwd[j]:
            named_by[i].append(j)
    offsets = np.zeros(n + 1, np.uint64)
    cols, bits, srow, sslot = [], [], [], []
    for i in range(n):
        row = {}
        for j, s in fwd[i].items():
            if mode == "union" or i in fwd[j]:
                row[j] = (i, s)
        if mode == "union":
            for j in named_by[i]:
                if j not in row:
                    row[j] = (j, fwd[j][i])
        entries = sorted(row.items(), key=lambda e: (order_key(dists[e[1][0], e[1][1]]), e[0]))
        for j, (r, s) in entries:
            cols.append(j)
            bits.append(int(np.asarray(dists[r, s], np.float32).view(np.uint32)))
            srow.append(r)
            sslot.append(s)
        offsets[i + 1] = len(cols)
    return offsets, np.array(cols, np.uint32), np.array(bits, np.uint32), np.array(srow, np.int64), np.array(sslot, np.int64)


def test_model_on_a_hand_made_graph():
    """0 -> 1, 2; 1 -> 0; 2 -> 3; 3 -> (nothing): union and mutual, the own row's distance first, -0 and NaN in the order"""
    counts = np.array([2, 1, 1, 0])
    pos = np.array([[1, 2], [0, 0], [3, 0], [0, 0]])
    d = np.array([[0.5, -0.0], [0.75, 0], [np.nan, 0], [0, 0]], np.float32)
    offs, cols, bits, srow, _ = symmetrise(4, counts, pos, d, "union")
    assert offs.tolist() == [0, 2, 3, 5, 6]
    assert cols.tolist() == [2, 1, 0, 0, 3, 2]                 # row 0: -0 (as +0) before 0.5; row 2: -0 from row 0, then its NaN
    assert srow.tolist() == [0, 0, 1, 0, 2, 2]                 # (1, 0) has its own 0.75, not row 0's 0.5
    f = lambda x: int(np.float32(x).view(np.uint32))
    assert bits.tolist()[:4] == [f(-0.0), f(0.5), f(0.75), f(-0.0)] and bits[4] == bits[5] == d[2, 0].view(np.uint32)
    offs, cols, bits, srow, _ = symmetrise(4, counts, pos, d, "mutual")
    assert offs.tolist() == [0, 1, 2, 2, 2] and cols.tolist() == [1, 0] and bits.tolist() == [f(0.5), f(0.75)]
    # positions: ids 7, 3, 7, 3 in dump order on two layers -> (3, flat 1), (3, flat 3), (7, flat 0), (7, flat 2)
    table, off = position_table([3, 1], [7, 3, 7, 3], [0, 0, 0, 1], [0, 1, 2, 0])
    assert table.tolist() == [2, 0, 3, 1] and off.tolist() == [0, 3, 4]


# ----------------------------------------------------------------------------------------------------- the ABI
def _small(native, n=50, d=8, f16=False):
    X = np.random.default_rng(1).random((n, d), dtype=np.float32)
    if f16:
        X = native.round_to_f16(X)
    h = native.Hnsw(8, n, 16, 32, "DistL2")
    h.set_build_options(nthreads=1)
    h.parallel_insert(X)
    return X, h


def test_header_declares_both_symbols_and_the_constants(native):
    N = _N()
    protos = N.HEADER.prototypes
    for name in ENTRIES:
        assert name in protos and name in N.SYMBOLS, name
        assert protos[name][0] is C.c_int
        assert getattr(native.lib(), name) is not None
    host, dev = protos[ENTRIES[0]][2], protos[ENTRIES[1]][2]
    assert host == ["idx", "k", "ef", "mode", "cap", "out_offsets", "out_pos", "out_ids", "out_dists", "out_layer", "out_rank"]
    assert dev == ["idx", "k", "ef", "mode", "cap", "d_out_offsets", "d_out_pos", "d_out_ids", "d_out_dists", "d_out_layer", "d_out_rank", "stream"]
    assert protos[ENTRIES[0]][1][3] is C.c_uint32
    assert N.HEADER.constants["HNSWGPU_SYM_UNION"] == 0 and N.HEADER.constants["HNSWGPU_SYM_MUTUAL"] == 1
    text = open(N.HEADER_PATH).read()
    doc = text[text.index("the symmetrised k-NN graph"):text.index("int hnswgpu_symmetric_graph_device")]
    for word in ("DistJeffreys", "DistJensenShannon", "NO fixed scratch budget", "2^30", "Out of scope", "connected components", "48 S"):
        assert word in doc, word
    for method in ("symmetric_knn_graph_flat", "symmetric_knn_graph"):
        assert hasattr(native.Hnsw, method), method
    r = native.GraphCsrResult(np.array([0, 2], np.uint64), *[np.arange(2)] * 5)
    assert r.counts.tolist() == [2] and [a.tolist() for a in r.of(0)] == [[0, 1]] * 5


def test_every_argument_error_is_answered_before_a_device_is_needed(native):
    N = _N()
    L = native.lib()
    X, h = _small(native)
    offs = np.full(51, 77, np.uint64)
    pos, dists = np.full(16, 5, np.uint32), np.full(16, 5, np.float32)

    def host(idx=h.handle, k=3, ef=0, mode=0, cap=16, of=offs, op=pos, od=dists):
        return L.hnswgpu_symmetric_graph(idx, k, ef, mode, cap, _p(of), _p(op), None, _p(od), None, None)

    def dev(idx=h.handle, k=3, ef=0, mode=0, cap=16, of=offs, op=pos, od=dists):
        return L.hnswgpu_symmetric_graph_device(idx, k, ef, mode, cap, _p(of), _p(op), None, _p(od), None, None, None)

    for call in (host, dev):
        def refused(word, **kw):
            rc = call(**kw)
            assert rc == N.ERR_ARG, (kw.keys(), rc, N.last_error())
            assert word in N.last_error(), (word, N.last_error())
        refused("null", idx=None)
        refused("out_offsets", of=None)
        for ef in (0, 32):
            refused("knbn", k=0, ef=ef)
            refused("mode", mode=2, ef=ef)
            refused("mode", mode=0xFFFFFFFF, ef=ef)
            refused("out_pos", op=None, ef=ef)                  # cap > 0 with NULL out arrays
            refused("out_dists", od=None, ef=ef)
            big = (1 << 30) // 50 + 1                           # 50 points x 21474837 = 1073741850 slots
            refused(str(50 * big), k=big, ef=ef)
            refused("2^30", k=1 << 40, ef=ef)
        refused("4096", k=4097)                                # the exact graph's own limit ...
        # ... and not the approximate one's.  Calls that are NOT refused go through the host entry only: on a box with a GPU they are
        # served, and the device entry must never be handed these host arrays
        spare = np.zeros(51, np.uint64)
        if call is host:
            assert call(k=4097, ef=32, cap=0, op=None, od=None, of=spare) != N.ERR_ARG or "4096" not in N.last_error()
        h.set_arithmetic("simd8")
        try:
            refused("SIMD8")                                   # ef == 0 only: the graph search serves either arithmetic
            if call is host:
                rc = call(ef=32, cap=0, op=None, od=None, of=spare)
                assert rc != N.ERR_ARG or "SIMD8" not in N.last_error()
        finally:
            h.set_arithmetic("scalar")
    assert (offs == 77).all() and (pos == 5).all() and (dists == 5).all()      # nothing was written by a refused call
    Xh, hh = _small(native, f16=True)
    hh.set_storage("f16")
    for ef in (0, 32):
        for rc in (L.hnswgpu_symmetric_graph(hh.handle, 3, ef, 0, 16, _p(offs), _p(pos), None, _p(dists), None, None),
                   L.hnswgpu_symmetric_graph_device(hh.handle, 3, ef, 0, 16, _p(offs), _p(pos), None, _p(dists), None, None, None)):
            assert rc == N.ERR_ARG and "HNSWGPU_STORAGE_F16" in N.last_error() and "HNSWGPU_STORAGE_F32" in N.last_error(), N.last_error()
    assert (offs == 77).all()
    for bad in (dict(knbn=0), dict(knbn=3, mode="both"), dict(knbn=3, ef=0)):  # the Python method hands the refusals on
        with pytest.raises(native.HnswError) as err:
            h.symmetric_knn_graph_flat(**bad)
        assert err.value.code == N.ERR_ARG


def test_empty_index_and_one_point_answer_without_a_device(native):
    N = _N()
    e = native.Hnsw(8, 10, 16, 32, "DistL2")
    for mode in ("union", "mutual"):
        for ef in (None, 16):
            res = e.symmetric_knn_graph_flat(5, ef, mode)
            assert res.offsets.tolist() == [0] and len(res.pos) == len(res.ids) == len(res.dists) == len(res.layers) == len(res.ranks) == 0
            assert res.offsets.dtype == np.uint64 and res.pos.dtype == np.uint32
            assert e.symmetric_knn_graph(5, ef, mode) == []
    X, h = _small(native, n=1)
    offs = np.full(2, 9, np.uint64)
    rc = native.lib().hnswgpu_symmetric_graph(h.handle, 4, 0, 1, 0, _p(offs), None, None, None, None, None)
    assert rc == N.OK and offs.tolist() == [0, 0]
    assert h.symmetric_knn_graph(4) == [[]]


def test_without_a_device_a_well_formed_call_reports_no_device(native):
    N = _N()
    X, h = _small(native)
    if native.lib().hnswgpu_device_count() > 0:                # a box with a GPU answers (tests/test_gpu_symmetric_graph.py checks the answer)
        res = h.symmetric_knn_graph_flat(3)
        assert (res.counts >= 3).all()
        return
    with pytest.raises(native.HnswError) as e:
        h.symmetric_knn_graph_flat(3)
    assert e.value.code == N.ERR_DEVICE
    offs = np.zeros(51, np.uint64)
    rc = native.lib().hnswgpu_symmetric_graph_device(h.handle, 3, 0, 0, 0, _p(offs), None, None, None, None, None, None)
    assert rc == N.ERR_DEVICE and N.last_error()
