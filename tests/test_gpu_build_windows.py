"""GPU-assisted construction with REAL windows (hundreds of points per launch of hnsw_build_search_kernel /
hnsw_build_select_kernel), byte for byte against a CPU model of the same protocol.

With nthreads=1 a windowed build is deterministic: the device's answer for a point depends only on the snapshot frozen when
the window began, and the host links the window's points in input order.  The oracle's insert_window (oracle/hnsw_oracle.hpp,
composed of its own search_layer / select_neighbours / reverse update, nothing shared with csrc/) restates that protocol;
build_windowed_oracle below restates the window schedule.  The model itself is pinned without a GPU: one point per window
equals insert_batch (tests/test_oracle.py) and windows of 200 equal the product's host side over a mock device
(tests/test_cpp_mirror.py).

Every case asserts, from the oracle's window statistics, that its input reaches the kernel path it is there for: many points
per persistent wavefront (HNSWGPU_BUILD_WG), migration of the visited table to the HBM bitmap (HNSWGPU_BUILD_HASH_BITS),
2 / 4 / 16 result slots per lane, rows of more than 64 ids, selections of more than 64 rows, a point above the frozen entry
point, host-side selection, a second batch, the growing-window rule.

Tie behaviour is not claimed: the build kernel is the lean form by design (equal distances in arrival order, where the
reference's order is its heap's).  The data is continuous, but two of the 300 f32 distances of a candidate list do coincide now
and then; such a pair shows in a graph only when both are selected.  Every case therefore asserts, from the oracle alone, that
no selected list of its build holds the same distance twice (selected_ties == 0), and the seeds are chosen on the CPU for that.
"""
import numpy as np
import pytest

from conftest import normalized, probability, uniform

N_DEFAULT, W_DEFAULT = 2500, 256


# ------------------------------------------------------------------------------------------------- the window schedule
def window_schedule(first, n_new, gpu_window):
    """(points inserted serially, [window sizes]) of GraphBuilder::insert_batch_gpu for a batch of n_new points on an index
    of `first` points.  builder.cpp:739-745: gpu_window 0 means 16384, and the host inserts serially until the index holds
    max(first, 1024) points (max(first, 1) with one point per window) -- so a batch on an index of >= 1024 points starts
    with windows at once.  builder.cpp:818-819: a window holds min(n - start, gpu_window, max(256, start // 8)) points."""
    max_window = gpu_window if gpu_window else 16384
    n = first + n_new
    start = min(n, max(first, 1 if max_window == 1 else 1024))
    boot = start - first
    sizes = []
    while start < n:
        grown = 1 if max_window == 1 else max(256, start // 8)
        sizes.append(min(n - start, max_window, grown))
        start += sizes[-1]
    return boot, sizes


def build_windowed_oracle(o, X, gpu_window):
    """Inserts the rows of X into the oracle index `o` as the product's GPU-assisted builder does with that gpu_window; origin
    ids continue from the number of points, as the product's do.  Returns the window sizes."""
    first = o.get_nb_point()
    boot, sizes = window_schedule(first, len(X), gpu_window)
    ids = np.arange(first, first + len(X), dtype=np.uint64)
    if boot:
        o.insert_batch(X[:boot], ids[:boot])
    at = boot
    for count in sizes:
        o.insert_window(X[at:at + count], ids[at:at + count])
        at += count
    assert at == len(X)
    return sizes


# ------------------------------------------------------------------------------------------------- the two builds
def _configure(index, cfg):
    if cfg.get("scale") is not None:
        index.modify_level_scale(cfg["scale"])
    if cfg.get("keep_pruned"):
        index.set_keeping_pruned(True)
    if cfg.get("extend"):
        index.set_extend_candidates(True)


def _data(cfg):
    gen = {"uniform": uniform, "normalized": normalized, "probability": probability}[cfg.get("data", "uniform")]
    return gen(cfg.get("n", N_DEFAULT), cfg["d"], cfg.get("seed", 191))


_ORACLE_CACHE = {}


@pytest.fixture(scope="module")
def oracle_build(oracle, tmp_path_factory):
    """oracle_build(cfg) -> (directory, basename, window statistics, window sizes, X): the windowed oracle build of a
    configuration, made once per module and left unchanged (cases 1 and 2 share one)."""
    def get(cfg):
        key = tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in cfg.items()))
        if key not in _ORACLE_CACHE:
            X = _data(cfg)
            o = oracle.OracleHnsw(cfg["m"], len(X), 16, cfg["efc"], cfg["dist"])
            _configure(o, cfg)
            sizes = []
            at = 0
            for part in cfg.get("batches") or [len(X)]:
                sizes += build_windowed_oracle(o, X[at:at + part], cfg.get("window", W_DEFAULT))
                at += part
            directory = tmp_path_factory.mktemp("oracle_windows")
            o.file_dump(directory, "orc")
            _ORACLE_CACHE[key] = (directory, "orc", o.window_stats(), sizes, X)
        return _ORACLE_CACHE[key]
    yield get
    _ORACLE_CACHE.clear()


def _device_build(native, cfg, X, directory, basename):
    """The product's build: one host thread, searches (and select_neighbours, where the configuration allows) on device 0."""
    before = native._native.last_error()
    h = native.Hnsw(cfg["m"], len(X), 16, cfg["efc"], cfg["dist"])
    _configure(h, cfg)
    h.set_build_options(nthreads=1, gpu_device=0, gpu_window=cfg.get("window", W_DEFAULT))
    at = 0
    for part in cfg.get("batches") or [len(X)]:
        h.parallel_insert(X[at:at + part])
        at += part
    assert h.get_nb_point() == len(X)
    # a build that fell back to the host builder succeeds and says so in the last message (GraphBuilder::last_warning):
    # a silent fall-back must not pass for the device
    assert native._native.last_error() == before, native._native.last_error()
    h.file_dump(directory, basename)


def first_difference(native, directory, name_a, name_b, dist, levels):
    """Reloads two dumps and names the first point in insertion order, and its first layer, whose lists differ."""
    a = native.HnswIo(directory, name_a).load_hnsw(dist)
    b = native.HnswIo(directory, name_b).load_hnsw(dist)
    seen = [0] * 16
    for i, level in enumerate(int(v) for v in levels):
        rank = seen[level]
        seen[level] += 1
        for l in range(15, -1, -1):   # (a point holds lists above its level too: the ef = 1 hits, and what a reverse update put there)
            la, lb = a.get_neighbours(level, rank, l), b.get_neighbours(level, rank, l)
            if not (np.array_equal(la[0], lb[0]) and np.array_equal(la[3].view(np.uint32), lb[3].view(np.uint32))):
                return (f"point {i} (level {level}, rank {rank}), layer {l}:\n  {name_a}: ids {la[0].tolist()} dists {la[3].tolist()}\n"
                        f"  {name_b}: ids {lb[0].tolist()} dists {lb[3].tolist()}")
    return "no list differs (the files differ elsewhere: header, entry point or vectors)"


def _assert_same_dumps(native, oracle, directory, cfg, n):
    same = all(open(directory / ("orc" + ext), "rb").read() == open(directory / ("gpu" + ext), "rb").read()
               for ext in (".hnsw.graph", ".hnsw.data"))
    if not same:
        levels = oracle.levels(cfg["m"], n, cfg.get("scale") or 1.0)
        pytest.fail("the device-built graph differs from the windowed oracle's; " + first_difference(native, directory, "orc", "gpu", cfg["dist"], levels))


def _case(native, oracle_build, oracle, cfg, knob=None, knobs=()):
    directory, _, stats, sizes, X = oracle_build(cfg)
    for name, value in knobs:
        knob(name, value)
    _device_build(native, cfg, X, directory, "gpu")
    _assert_same_dumps(native, oracle, directory, cfg, len(X))
    assert stats["points"] == sum(sizes) and stats["windows"] == len(sizes) and stats["selected_ties"] == 0, (stats, sizes)
    return stats, sizes


PLAIN = dict(dist="DistL2", d=16, m=12, efc=60)


# ------------------------------------------------------------------------------------------------- the cases
@pytest.mark.gpu
def test_plain_windows_on_the_default_grid(native, oracle, oracle_build):
    """Case 1: windows of 256 points, one workgroup per point as a real build launches them: window indexing (slot0[wi] + l,
    slot * ef_c + j, wi * NB_LAYER_MAX + l, slot_nb, sel_stride) and scatter_lists_kernel with the records of 256 points."""
    stats, sizes = _case(native, oracle_build, oracle, PLAIN)
    assert sizes == [256] * 5 + [196]
    assert stats["selections_pruned"] > 1000 and stats["max_candidates"] == 60, stats


@pytest.mark.gpu
@pytest.mark.parametrize("hash_bits", [None, 8])
def test_many_points_per_wavefront_and_migration_to_the_bitmap(native, oracle, oracle_build, knob, hash_bits):
    """Case 2: the same build on 4 workgroups, so every persistent wavefront of both kernels handles about 64 points of a
    window one after the other -- what is carried from point to point (failed, use_bm, the visited table and its clearing, the
    query tile, ids_lds, sel_lds / seld_lds, the CAND_DISCARDED flags, the fences between points) now matters.  With a visited
    table of 2^8 cells the searches also migrate to the HBM bitmap: the oracle's largest visit count exceeds the table's limit
    of 0.75 * 2^8 minus the 64 ids of one batch."""
    knobs = [("HNSWGPU_BUILD_WG", 4)] + ([("HNSWGPU_BUILD_HASH_BITS", hash_bits)] if hash_bits else [])
    stats, _ = _case(native, oracle_build, oracle, PLAIN, knob, knobs)
    assert stats["max_visited"] > 0.75 * 2 ** 8 - 64, stats


@pytest.mark.gpu
@pytest.mark.parametrize("d,keep_pruned", [(25, True), (32, False)])
def test_cosine_with_the_norm_in_the_padding_and_beside_the_row(native, oracle, oracle_build, knob, d, keep_pruned):
    """Case 3: DistCosine at d = 25 (the stored norm lives in the row's padding) and d = 32 (the row is full: a norm array beside
    it), ef_construction 100 = two result slots per lane, keep_pruned in the first."""
    cfg = dict(dist="DistCosine", d=d, m=8, efc=100, keep_pruned=keep_pruned, seed=192)   # (seed 191: a tie among the selected at d = 25)
    stats, _ = _case(native, oracle_build, oracle, cfg, knob, [("HNSWGPU_BUILD_WG", 4)])
    assert stats["max_candidates"] == 100 and stats["selections_pruned"] > 1000, stats


@pytest.mark.gpu
def test_dot_with_four_result_slots(native, oracle, oracle_build):
    """Case 4: DistDot on normalized data, ef_construction 250 = four result slots per lane, all of them in use."""
    cfg = dict(dist="DistDot", d=12, m=6, efc=250, data="normalized")
    stats, _ = _case(native, oracle_build, oracle, cfg)
    assert stats["max_candidates"] == 250 and stats["selections_pruned"] > 1000, stats


@pytest.mark.gpu
@pytest.mark.parametrize("dist,d,keep_pruned", [("DistJeffreys", 12, False), ("DistJensenShannon", 9, True)])
def test_probability_distances(native, oracle, oracle_build, knob, dist, d, keep_pruned):
    """Case 5: the two f32::ln distances; select_neighbours evaluates dist(e, selected) with e FIRST (src/hnsw.rs:1373-1375),
    which shows in the last bits of these sums, and the heuristic runs for nearly every point."""
    cfg = dict(dist=dist, d=d, m=8, efc=60, data="probability", keep_pruned=keep_pruned)
    stats, _ = _case(native, oracle_build, oracle, cfg, knob, [("HNSWGPU_BUILD_WG", 4)])
    assert stats["selections_pruned"] > 1000, stats


WIDE_D, WIDE_SEED = 32, 195   # chosen on the CPU with the oracle alone: the heuristic keeps up to 70 rows, no tie among the selected


@pytest.mark.gpu
def test_sixteen_slots_wide_rows_and_long_selections(native, oracle, oracle_build, knob):
    """Case 6: M = 40 -- rows of 80 ids at layer 0 (two 64-lane batches per expanded row, nb = 80) --, ef_construction 300 =
    sixteen result slots per lane, and a dimension at which select_neighbours keeps more than 64 rows at least once, so the
    select kernel compares a candidate with a second 64-chunk of selected rows."""
    cfg = dict(dist="DistL2", d=WIDE_D, m=40, efc=300, seed=WIDE_SEED)
    stats, _ = _case(native, oracle_build, oracle, cfg, knob, [("HNSWGPU_BUILD_WG", 8)])
    assert stats["max_candidates"] == 300 and stats["max_kept"] > 64, stats


LEVEL_M, LEVEL_SCALE, LEVEL_N = 10, 0.6, 5300   # chosen on the CPU from oracle.levels, see the test


@pytest.mark.gpu
def test_points_above_the_frozen_entry_point(native, oracle, oracle_build):
    """Case 7: DistL1 with a modified level scale: after the bootstrap a window holds a point above the frozen entry point's
    level with further points behind it in the same window, which still start from the old entry point.

    The level stream is fixed (SplitMix64(397)) and every (M, scale) maps the same draws to levels monotonically, so WHERE a
    new highest level can appear does not depend on them: after draw 45 the next record is draw 5026.  No (M, scale) with M in
    4..48 and scale in 0.3..1.0 puts a point above the entry point into a window of the first 2500 points, so this case alone
    uses 5300 points; with M = 10 and scale 0.6 point 5026 has level 2 over an entry point of level 1, in the last window.  No
    pair of that grid also leaves a layer empty in a frozen mask at this size (the oracle reports 0 skipped layers for all of
    them), so only the first statistic is asserted."""
    cfg = dict(dist="DistL1", d=10, m=LEVEL_M, efc=40, scale=LEVEL_SCALE, n=LEVEL_N)
    levels = oracle.levels(LEVEL_M, LEVEL_N, LEVEL_SCALE).astype(int)
    boot, sizes = window_schedule(0, LEVEL_N, W_DEFAULT)
    start, followed = boot, 0
    for count in sizes:
        above = np.nonzero(levels[start:start + count] > levels[:start].max())[0]
        followed += int(above.size > 0 and above[0] < count - 1)
        start += count
    assert followed > 0
    stats, _ = _case(native, oracle_build, oracle, cfg)
    assert stats["above_entry"] > 0, stats


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["extend_candidates", "HNSWGPU_HOST_SELECT"])
def test_host_side_selection_from_device_candidates(native, oracle, oracle_build, knob, how):
    """Case 8: select_neighbours on the host from the candidates the device returns (the out.selected == false branch of
    apply_window_point), with many points per window: extend_candidates, which reads the live lists, and the knob that keeps
    the selection on the host for a plain index."""
    if how == "extend_candidates":
        cfg, knobs = dict(PLAIN, extend=True), []
    else:
        cfg, knobs = PLAIN, [("HNSWGPU_HOST_SELECT", 1)]
    stats, _ = _case(native, oracle_build, oracle, cfg, knob, knobs)
    assert stats["selections_pruned"] > 1000, stats


@pytest.mark.gpu
def test_second_batch_on_the_same_handle(native, oracle, oracle_build):
    """Case 9: 1500 points, then 1000 more on the same handle: the second call has no host bootstrap, its first window is
    searched in the snapshot uploaded from the finished first batch."""
    cfg = dict(PLAIN, batches=[1500, 1000])
    stats, sizes = _case(native, oracle_build, oracle, cfg)
    assert sizes == [256, 220, 256, 256, 256, 232] and window_schedule(1500, 1000, W_DEFAULT)[0] == 0


@pytest.mark.gpu
def test_windows_grow_with_the_index(native, oracle, oracle_build):
    """Case 10: gpu_window 4096 on 6000 points: windows of 256 until start // 8 exceeds that, then start // 8."""
    cfg = dict(dist="DistL2", d=8, m=6, efc=40, n=6000, window=4096)
    stats, sizes = _case(native, oracle_build, oracle, cfg)
    start = 1024
    for count in sizes[:-1]:
        assert count == max(256, start // 8), (start, sizes)
        start += count
    assert sizes[:6] == [256] * 5 + [288] and sizes[-2] > 600 and start + sizes[-1] == 6000, sizes
