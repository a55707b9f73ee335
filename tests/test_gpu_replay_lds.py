"""The replay of a strict query's heap-operation log on LDS-only heap operations (csrc/search_kernels.inc: heap_push_lds,
heap_pop_lds, and literal_candidate_pop, which takes them for every chunk of the log that leaves the candidate heap within its
LDS part and the general memory heap otherwise).

* Lane lab (mode 0, p1 = 2 / 3, p2 = 2): the new operations themselves against the oracle's RustBinaryHeap -- every popped entry
  and the final array (into_sorted_vec); the pop that does not report its root (the form a replayed pop takes) is checked through
  the final array alone.  Scripts sit on the pop's round boundaries (63 / 64 and 2 047 / 2 048 entries), empty the heap and fill it
  again, and run at every size of the LDS part the search can have.
* End to end, strict, against the oracle: answers, distance bits, counts and the per-query work counters on data full of equal
  distances, with the replay taken from the first tie on (HNSWGPU_EXACT_FIRST=1) through the general operations, the LDS-only
  ones, and both within one replay (HNSWGPU_CAND_LDS), and as the library runs by default.
"""
import random

import numpy as np
import pytest

from test_gpu_counters import _device_search, _pair, check
from test_gpu_lane_lab import POP, PUSH, check_heap, f2u, heap_case, keys, run_lab

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ lane lab
def hold_case(rnd, lo, hi, n_ops, ties):
    """pushes up to `lo` entries, then n_ops pushes and pops that keep the length within [lo, hi]; then pops down to a few"""
    ops, vals, tags, is_pop = [], [], [], []
    ks = keys(rnd, lo + n_ops + 8, ties)
    size, tag = 0, 0

    def push():
        nonlocal size, tag
        k = ks[tag]
        ops.append((PUSH, f2u(k), tag, 0)); vals.append(float(k)); tags.append(tag); is_pop.append(0)
        size += 1
        tag += 1

    def pop():
        nonlocal size
        ops.append((POP, 0, 0, 0)); vals.append(0.0); tags.append(0); is_pop.append(1)
        size -= 1

    while size < lo:
        push()
    for _ in range(n_ops):
        if size <= lo or (size < hi and rnd.random() < 0.5):
            push()
        else:
            pop()
    return ops, [], vals, tags, is_pop


def drain_case(rnd, n, ties):
    """fill, pop to empty, refill, pop half: the one-entry and the empty heap on the way"""
    ops, vals, tags, is_pop = [], [], [], []
    ks = keys(rnd, 3 * n, ties)
    ki = 0
    for count, is_p in ((n, 0), (n, 1), (n // 2 + 1, 0), (n // 4, 1), (n // 3, 0)):
        for _ in range(count):
            if is_p:
                ops.append((POP, 0, 0, 0)); vals.append(0.0); tags.append(0); is_pop.append(1)
            else:
                ops.append((PUSH, f2u(ks[ki]), ki, 0)); vals.append(float(ks[ki])); tags.append(ki); is_pop.append(0)
                ki += 1
    return ops, [], vals, tags, is_pop


def lds_scripts(rnd, lds_cap, ties):
    yield heap_case(rnd, 2000, ties, batches=False, cap=lds_cap)           # random: about 0.3 pops per operation, the heap grows
    yield drain_case(rnd, min(lds_cap, 400), ties)
    if lds_cap >= 66:
        yield hold_case(rnd, 61, 66, 2000, ties)                           # one round / two rounds of the pop
    else:
        yield hold_case(rnd, 60, 64, 2000, ties)
    if lds_cap >= 2050:
        yield hold_case(rnd, 2045, 2050, 2000, ties)                       # two rounds / three rounds
    elif lds_cap >= 2048:
        yield hold_case(rnd, 2044, 2048, 2000, ties)
    if lds_cap >= 256:
        yield hold_case(rnd, lds_cap - 3, lds_cap, 1000, ties)             # the last entries of the LDS part


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("lds_cap", [64, 256, 512, 2048, 4096])
def test_lds_only_heap_equals_std_binaryheap(native, oracle, lds_cap, ties):
    """heap_push_lds / heap_pop_lds on the device == Rust's BinaryHeap, equal keys included: every popped entry, and the final
    array; the pop without a root (p1 = 3) reports nothing and shows in the final array."""
    rnd = random.Random(5000 + 10 * lds_cap + int(ties))
    for ops, _lanes, vals, tags, is_pop in lds_scripts(rnd, lds_cap, ties):
        n_pops = sum(is_pop)
        words = 4 * len(ops) + 64
        check_heap(run_lab(native, 0, lds_cap, 2, 2, ops, out_words=words), oracle, vals, tags, is_pop)
        check_heap(run_lab(native, 0, lds_cap, 3, 2, ops, out_words=words), oracle, vals, tags, is_pop, silent_pops=set(range(n_pops)))
        # next to the general operations on the same array, as a replay that changes path from chunk to chunk
        check_heap(run_lab(native, 0, lds_cap, 2, 1, ops, out_words=words), oracle, vals, tags, is_pop)
        check_heap(run_lab(native, 0, lds_cap, 1, 2, ops, out_words=words), oracle, vals, tags, is_pop)


def test_lab_refuses_a_script_that_outgrows_the_lds_part(native):
    """the LDS-only operations address LDS alone: a script that would push entry lds_cap + 1 never reaches the device"""
    lib = native.lib()
    ops = np.array([(PUSH, f2u(float(i)), i, 0) for i in range(65)] + [(POP, 0, 0, 0)], dtype=np.uint32)
    lanes = np.zeros((0, 64, 2), np.uint32)
    out = np.zeros(1024, np.uint32)
    for p1, p2 in ((2, 2), (3, 0), (0, 2)):
        assert lib.hnswgpu_lane_lab(0, 0, 64, p1, p2, ops.ctypes.data, len(ops), lanes.ctypes.data, 0, out.ctypes.data, len(out)) != 0
        assert "LDS-only" in native._native.last_error()
    assert lib.hnswgpu_lane_lab(0, 0, 64, 1, 1, ops.ctypes.data, len(ops), lanes.ctypes.data, 0, out.ctypes.data, len(out)) == 0
    assert lib.hnswgpu_lane_lab(0, 0, 65, 2, 2, ops.ctypes.data, len(ops), lanes.ctypes.data, 0, out.ctypes.data, len(out)) == 0


# ------------------------------------------------------------------------------------------------------------------ end to end
N, D, M, EFC, NQ, NQ_STORED = 20000, 16, 8, 40, 256, 64


def _l2_normalize(x):
    import oracle_lib
    for row in x:  # the crate's l2_normalize, f32, in place
        oracle_lib.lib().orc_l2_normalize(row.ctypes.data, x.shape[1])


def tie_data(dist):
    """20 000 x 16 f32; every tenth point is there three times (two more copies, ids of their own): equal distances wherever a
    search meets one of them.  256 queries, 64 of them stored points (one in two of those a point with copies)."""
    rng = np.random.default_rng(2024)
    base = rng.random((16666, D), dtype=np.float32)
    if dist == "DistDot":   # defined on L2-normalised vectors
        _l2_normalize(base)
    tenth = base[::10]
    X = np.concatenate([base, tenth, tenth])
    assert X.shape == (N, D)
    X = np.ascontiguousarray(X[rng.permutation(N)])
    Q = rng.random((NQ, D), dtype=np.float32)
    if dist == "DistDot":
        _l2_normalize(Q)
    Q[:NQ_STORED // 2] = tenth[rng.choice(len(tenth), NQ_STORED // 2, replace=False)]
    Q[NQ_STORED // 2:NQ_STORED] = X[rng.choice(N, NQ_STORED // 2, replace=False)]
    return X, np.ascontiguousarray(Q[rng.permutation(NQ)])


@pytest.fixture(scope="module")
def tie_index(native, oracle, tmp_path_factory):
    built = {}

    def get(dist):
        if dist not in built:
            X, Q = tie_data(dist)
            o, h = _pair(native, oracle, tmp_path_factory.mktemp("replay_" + dist), X, M, EFC, dist, "replay")
            built[dist] = (o, h, Q)
        return built[dist]
    return get


@pytest.mark.parametrize("ef", [10, 64, 100])
@pytest.mark.parametrize("dist", ["DistL2", "DistDot"])
def test_replay_paths_match_the_oracle(native, tie_index, knob, dist, ef):
    """strict answers, distance bits, counts and work counters == the oracle's: by default (a quarter of the queries at least
    must have been resolved with the literal heaps, status 3: else the case tests nothing), with every chunk of every query's log
    replayed from the first tie on through the LDS-only operations (512 entries in LDS), and with 64 entries in LDS (most chunks
    through the general operations, and both kinds within one replay)."""
    o, h, Q = tie_index(dist)
    res, ref = check(native, h, o, Q, 10, ef, f"{dist} ef {ef} default", lean=False)
    n3 = int((res.st[:, 3] == 3).sum())
    print(f"{dist} ef {ef}: {n3} of {NQ} queries resolved with the literal heaps (status 3)")
    assert 4 * n3 >= NQ, f"{dist} ef {ef}: only {n3} of {NQ} queries replayed their log"
    knob("HNSWGPU_EXACT_FIRST", "1")
    for cand_lds in (512, 64):
        knob("HNSWGPU_CAND_LDS", cand_lds)
        res = _device_search(native, h, Q, 10, ef)
        n3 = int((res.st[:, 3] == 3).sum())
        print(f"{dist} ef {ef} exact first, {cand_lds} entries in LDS: {n3} of {NQ} queries with status 3")
        check(native, h, o, Q, 10, ef, f"{dist} ef {ef} exact first, cand_lds {cand_lds}", lean=False, res=res)
    knob("HNSWGPU_CAND_LDS", None)
    knob("HNSWGPU_EXACT_FIRST", None)
