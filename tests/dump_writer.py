"""An hnswio dump written BY HAND: arbitrary vectors, origin ids and levels, no builder involved.

TEST INFRASTRUCTURE ONLY.  The exhaustive exact k-NN search (csrc/exact_knn.hip) reads the vectors, the origin ids and the layer
offsets of an index and never its graph, so the index for its hostile-value tests need not be a graph anyone could search -- and
it cannot be built: the reference refuses a NaN distance during insertion and asserts the domain of DistCosine / DistHellinger
on row-to-row pairs.  This module packs the two files of a dump (format v4, DumpMode::Full) following SURVEY.md Appendix A field
by field, as test_hnswio.py::test_byte_layout_matches_appendix_a does for five points.

Ranks: the rank of a row within its layer is its input order among the rows of that level.  Entry point: the first row of the
highest level.

Neighbour lists: EMPTY by default (16 lists of length 0 per point).  Both readers -- the product's (HnswIo.load_hnsw) and the
oracle's (OracleHnsw.load) -- accept them; tests/test_dump_writer.py holds them to it.  A search of such an index would stop at
its entry point; nothing in the tests that use this writer searches it.  `neighbours` lets a test hand in real lists (the
byte-for-byte comparison with the product's own writer needs them)."""
import math
import os
import struct

import numpy as np

MAGICDESCR_4, MAGICLAYER, MAGICPOINT, MAGICDATAP = 0x002a6779, 0x000a676f, 0x000a678f, 0xa67f0000
NB_LAYER_MAX = 16


def dump_order(levels):
    """(order, pids): order = the row indices in (layer, rank) order -- the order of the records in both files and the flat order
    of the loaded index; pids[row] = (layer, rank) of every row"""
    levels = np.asarray(levels, np.int64)
    assert levels.ndim == 1 and len(levels) > 0 and levels.min() >= 0 and levels.max() < NB_LAYER_MAX
    order = np.argsort(levels, kind="stable")          # layer ascending, input order within a layer
    pids = [None] * len(levels)
    seen = [0] * NB_LAYER_MAX
    for row in order:
        L = int(levels[row])
        pids[row] = (L, seen[L])
        seen[L] += 1
    return [int(r) for r in order], pids


def write_dump(directory, basename, X, ids, levels, metric, m=8, ef_construction=16, neighbours=None):
    """Writes <basename>.hnsw.graph and <basename>.hnsw.data into `directory`: row i of X (f32, any bit pattern) is the point of
    origin id ids[i] (any u64, repeats allowed) on layer levels[i].  metric: a short distance name ("DistL2", ...).
    neighbours: None (every list empty) or {(row, l): [(neighbour row, stored f32 distance), ...]}.
    Returns (order, pids) of dump_order(levels)."""
    X = np.ascontiguousarray(X)
    assert X.dtype == np.float32 and X.ndim == 2 and X.shape[1] > 0
    n, d = X.shape
    ids = [int(v) for v in ids]
    assert len(ids) == n and len(levels) == n and 0 < m < 256
    order, pids = dump_order(levels)
    neighbours = neighbours or {}
    distname = ("anndists::dist::distances::" + metric).encode()
    g = bytearray()
    g += struct.pack("=I", MAGICDESCR_4)
    g += struct.pack("=BB", 1, m)                                    # dumpmode Full, max_nb_connection as u8
    g += struct.pack("=d", 1.0 / math.log(float(m)))                 # level_scale: the absolute scale 1 / ln(M)
    g += struct.pack("=B", NB_LAYER_MAX)                             # nb_layer
    g += struct.pack("=QQQ", ef_construction, n, d)                  # ef_construction, nb_point, dimension
    g += struct.pack("=Q", len(distname)) + distname
    g += struct.pack("=Q", 3) + b"f32"
    g += struct.pack("=B", NB_LAYER_MAX)                             # points_by_layer.len()
    dt = bytearray(struct.pack("=IQ", MAGICDATAP, d))
    at = 0
    for layer in range(NB_LAYER_MAX):
        end = at
        while end < n and pids[order[end]][0] == layer:
            end += 1
        g += struct.pack("=IQ", MAGICLAYER, end - at)                # nb points whose own level is `layer`
        for row in order[at:end]:
            g += struct.pack("=IQ", MAGICPOINT, ids[row])
            g += struct.pack("=Bi", *pids[row])                      # p_id
            for l in range(NB_LAYER_MAX):                            # always 16 lists
                lst = neighbours.get((row, l), ())
                g += struct.pack("=Q", len(lst))
                for nb, dist in lst:                                 # 17 bytes per edge
                    g += struct.pack("=QBi", ids[nb], *pids[nb]) + np.float32(dist).tobytes()
            dt += struct.pack("=IQQ", MAGICDATAP, ids[row], 4 * d) + X[row].tobytes()
        at = end
    assert at == n
    top = pids[order[-1]][0]
    entry = next(r for r in order if pids[r][0] == top)              # the first row of the highest level
    g += struct.pack("=QBi", ids[entry], *pids[entry])
    with open(os.path.join(str(directory), basename + ".hnsw.graph"), "wb") as f:
        f.write(bytes(g))
    with open(os.path.join(str(directory), basename + ".hnsw.data"), "wb") as f:
        f.write(bytes(dt))
    return order, pids
