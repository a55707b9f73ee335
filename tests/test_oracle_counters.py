"""The oracle's per-query work counters (OracleHnsw.parallel_search / parallel_search_filter with want_counters="per_query"):
what the algorithmic bytes of SURVEY.md section 8(d) are computed from, and what the device's stats words are checked against
(tests/test_gpu_counters.py).  Rows = (n_dist, n_expand, n_ids_read, descent n_dist, descent n_expand)."""
import numpy as np
import pytest

from conftest import uniform


def _same_answers(a, b):
    assert np.array_equal(a.counts, b.counts)
    assert np.array_equal(a.ids, b.ids)
    assert np.array_equal(a.dists.view(np.uint32), b.dists.view(np.uint32))
    assert np.array_equal(a.ranks, b.ranks)


@pytest.fixture(scope="module")
def small(oracle):
    X = uniform(1500, 12, 301)
    X[1000:1200] = X[:200]  # duplicates: searches through equal distances too
    o = oracle.OracleHnsw(10, len(X), 16, 60, "DistL2")
    o.insert_batch(X)
    return o, uniform(90, 12, 302)


@pytest.mark.parametrize("k,ef", [(10, 10), (10, 64), (40, 20)])
def test_per_query_rows_sum_to_the_batch_totals(small, k, ef):
    o, Q = small
    tot = o.parallel_search(Q, k, ef, nthreads=3, want_counters=True)
    pq = o.parallel_search(Q, k, ef, nthreads=3, want_counters="per_query")
    _same_answers(tot, pq)
    assert pq.per_query.shape == (len(Q), 5) and pq.per_query.dtype == np.uint64
    s = pq.per_query.sum(0)
    assert [int(s[0]), int(s[1]), int(s[2])] == [tot.counters["n_dist"], tot.counters["n_expand"], tot.counters["n_ids_read"]]
    d_dist, d_exp = pq.per_query[:, 3].astype(np.int64), pq.per_query[:, 4].astype(np.int64)
    top = o.get_max_level_observed()
    assert np.all(d_exp == top)                        # one list per upper layer
    assert np.all(d_dist >= 1) and np.all(d_dist < pq.per_query[:, 0].astype(np.int64))
    assert np.all(pq.per_query[:, 1] > pq.per_query[:, 4])   # search_layer pops at least its entry point


@pytest.mark.parametrize("density", [0.01, 0.3, 1.0])
def test_filtered_per_query_rows_sum_to_the_batch_totals(small, density):
    o, Q = small
    rng = np.random.default_rng(int(density * 100))
    n = o.get_nb_point()
    allowed = np.sort(rng.choice(n, max(1, int(n * density)), replace=False)).astype(np.uint64)
    tot = o.parallel_search_filter(Q, 10, 20, allowed, nthreads=3, want_counters=True)
    pq = o.parallel_search_filter(Q, 10, 20, allowed, nthreads=3, want_counters="per_query")
    _same_answers(tot, pq)
    assert np.array_equal(tot.status, pq.status)
    assert np.array_equal(pq.per_query[:, :3].sum(0), tot.counters)
    if density == 1.0:  # everything allowed: the filter never returns early, so the walk is at least the unfiltered one
        un = o.parallel_search(Q, 10, 20, nthreads=3, want_counters="per_query")
        assert np.array_equal(un.per_query[:, 3:], pq.per_query[:, 3:])
        assert np.all(pq.per_query[:, 1] >= un.per_query[:, 1])


def test_single_point_index_by_hand(oracle):
    """One point at level L: the descent evaluates it once and reads its L empty upper lists; search_layer (on layer L when the
    lower layers are empty, :1534-1540) evaluates it again (:952) and reads one more empty list."""
    for seed in range(4):
        o = oracle.OracleHnsw(8, 1, 16, 20, "DistL2")
        o.insert_batch(uniform(1, 5, 400 + seed))
        L = o.get_max_level_observed()
        r = o.parallel_search(uniform(6, 5, 410), 3, 10, nthreads=1, want_counters="per_query")
        assert np.all(r.counts == 1)
        assert r.per_query.tolist() == [[2, L + 1, 0, 1, L]] * 6


def test_one_layer_index_by_hand(oracle):
    """Points 0, 1, 2 on a line, every point on layer 0 (max_layer 1), lists 0: [1, 2], 1: [0, 2], 2: [1, 0].  Query 2.2, ef 1:
    descent = eval(0) and no list; search_layer: eval(0) again (:952), pop 0, read [1, 2] and evaluate both (ret ends at {2}),
    pop 2, read [1, 0] (both visited), nothing left -> n_dist 4, n_expand 2, n_ids_read 4."""
    o = oracle.OracleHnsw(4, 3, 1, 10, "DistL2")
    o.insert_batch(np.array([[0.0], [1.0], [2.0]], np.float32))
    assert o.get_max_level_observed() == 0 and o.get_layer_nb_point(0) == 3
    r = o.parallel_search(np.array([[2.2]], np.float32), 1, 1, nthreads=1, want_counters="per_query")
    assert int(r.ids[0, 0]) == 2
    assert r.per_query.tolist() == [[4, 2, 4, 1, 0]]
    # query at 0.1, ef 1: eval(0) twice, pop 0, read [1, 2]: 1 at 0.9 and 2 at 1.9 are both farther than 0 with ret full -> no
    # push; the candidate heap is empty -> n_dist 4, n_expand 1, n_ids_read 2
    r = o.parallel_search(np.array([[0.1]], np.float32), 1, 1, nthreads=1, want_counters="per_query")
    assert int(r.ids[0, 0]) == 0
    assert r.per_query.tolist() == [[4, 1, 2, 1, 0]]
