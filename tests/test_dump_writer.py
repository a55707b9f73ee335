"""tests/dump_writer.py: a dump packed by hand is a dump both readers take -- the product's and the oracle's -- with the points
where the writer says they are and every vector bit for bit.  CPU only."""
import struct

import numpy as np
import pytest

import f64_reference as F
from conftest import same_dump_after_reload, uniform
from dump_writer import dump_order, write_dump


def _hostile_bits(n, d, seed):
    """f32 rows of arbitrary bit patterns: NaNs with payloads and signs, infinities, -0.0, subnormals, the sweep's magnitudes"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 2 ** 32, (n, d), dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
    special = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF], np.uint32)
    X[0, :min(d, 8)] = special.view(np.float32)[:min(d, 8)]
    return X


def _entry_of(graph_path):
    return struct.unpack("=QBi", open(graph_path, "rb").read()[-13:])


@pytest.mark.parametrize("metric,d", [("DistL2", 33), ("DistCosine", 30), ("DistJensenShannon", 1), ("DistL1", 7)])
def test_both_readers_accept_a_hand_written_dump(native, oracle, tmp_path, metric, d):
    n = 300
    if metric == "DistL1":
        X = _hostile_bits(n, d, 5)
    else:
        X = uniform(n, d, 5)
        Rh = F.hostile_sweep(metric, d, 7)[1]                              # the rows the device tests write
        X[np.arange(len(Rh)) * 4] = Rh
    rng = np.random.default_rng(6)
    ids = rng.permutation(n).astype(np.uint64) * 3 + 1
    levels = np.zeros(n, np.int64)
    p = rng.permutation(n)
    levels[p[:30]] = 1
    levels[p[30:35]] = 2
    order, pids = write_dump(tmp_path, "hand", X, ids, levels, metric)
    assert sorted(order) == list(range(n)) and order != list(range(n))
    assert [pids[r] for r in order] == sorted(pids)                        # (layer, rank) order
    assert pids[order[-5]] == (2, 0) and order[-5] == int(np.flatnonzero(levels == 2)[0])
    h = native.HnswIo(tmp_path, "hand").load_hnsw(metric)
    o = oracle.OracleHnsw.load(tmp_path, "hand", metric)
    assert h.get_nb_point() == o.get_nb_point() == n
    assert h.get_max_level_observed() == o.get_max_level_observed() == 2
    for l in range(16):
        assert h.get_layer_nb_point(l) == o.get_layer_nb_point(l) == int((levels == l).sum())
    entry = (int(ids[order[-5]]), 2, 0)                                    # the first row of the highest level
    ep_origin, (ep_layer, ep_rank) = h.get_entry_point()
    assert (ep_origin, ep_layer, ep_rank) == entry
    # both readers write back what they read: the same files, but for the level scale a reloaded index dumps (conftest)
    h.file_dump(tmp_path, "prod")
    o.file_dump(tmp_path, "orc")
    for again in ("prod", "orc"):
        assert same_dump_after_reload(tmp_path / "hand.hnsw.graph", tmp_path / f"{again}.hnsw.graph"), again
        assert open(tmp_path / f"{again}.hnsw.data", "rb").read() == open(tmp_path / "hand.hnsw.data", "rb").read(), again
        assert _entry_of(tmp_path / f"{again}.hnsw.graph") == entry
    for L, r in ((0, 0), (1, 3), (2, 4)):
        assert all(len(h.get_neighbours(L, r, l)[0]) == 0 for l in range(16))   # the lists are empty
    dm = native.DataMap.from_hnswdump(tmp_path, "hand")
    assert dm.get_nb_data() == n and dm.get_dimension() == d and dm.get_distname().endswith(metric)
    assert dm.get_dataid_iter() == [int(ids[r]) for r in order]            # file order = dump order
    for i in range(n):
        assert np.array_equal(np.asarray(dm.get_data(int(ids[i]))).view(np.uint32), X[i].view(np.uint32)), i


def test_repeated_origin_ids_are_accepted_by_both_readers(native, oracle, tmp_path):
    n, d = 60, 4
    X = uniform(n, d, 8)
    ids = np.arange(n, dtype=np.uint64) // 3
    levels = np.arange(n) % 3
    order, pids = write_dump(tmp_path, "rep", X, ids, levels, "DistL2")
    h = native.HnswIo(tmp_path, "rep").load_hnsw("DistL2")
    o = oracle.OracleHnsw.load(tmp_path, "rep", "DistL2")
    assert h.get_nb_point() == o.get_nb_point() == n
    assert [h.get_layer_nb_point(l) for l in range(3)] == [o.get_layer_nb_point(l) for l in range(3)] == [20, 20, 20]
    assert h.get_entry_point() == (0, (2, 0))                              # row 2 bears id 0
    h.file_dump(tmp_path, "again")
    assert open(tmp_path / "again.hnsw.data", "rb").read() == open(tmp_path / "rep.hnsw.data", "rb").read()


def test_dump_order():
    order, pids = dump_order([0, 2, 0, 1, 2, 0, 1])
    assert order == [0, 2, 5, 3, 6, 1, 4]
    assert pids == [(0, 0), (2, 0), (0, 1), (1, 0), (2, 1), (0, 2), (1, 1)]
    with pytest.raises(AssertionError):
        dump_order([0, 16])


def test_five_points_equal_the_product_writers_bytes(native, tmp_path):
    """the five points of test_hnswio.py::test_byte_layout_matches_appendix_a, their lists read back with get_neighbours and handed
    to the writer: the two files of the product's own writer, byte for byte"""
    import oracle_lib
    X = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 2.0], [3.0, 3.0], [0.5, 0.5]], np.float32)
    ids = [10, 11, 12, 13, 14]
    h = native.Hnsw(4, 5, 16, 10, "DistL1")
    h.insert_serial(X, ids=ids)
    h.file_dump(tmp_path, "tiny")
    lv = oracle_lib.levels(4, 5)
    _, pids = dump_order(lv)
    row_of = {p: i for i, p in enumerate(pids)}
    nbs, edges = {}, 0
    for i, (layer, rank) in enumerate(pids):
        for l in range(16):
            nid, nl, nr, nd = h.get_neighbours(layer, rank, l)
            nbs[(i, l)] = [(row_of[(int(a), int(b))], c) for a, b, c in zip(nl, nr, nd)]
            assert [ids[r] for r, _ in nbs[(i, l)]] == nid.tolist()
            edges += len(nid)
    assert edges > 0
    write_dump(tmp_path, "hand", X, ids, lv, "DistL1", m=4, ef_construction=10, neighbours=nbs)
    for ext in (".hnsw.graph", ".hnsw.data"):
        assert open(tmp_path / ("hand" + ext), "rb").read() == open(tmp_path / ("tiny" + ext), "rb").read(), ext
