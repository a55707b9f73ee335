"""bench.py --dump-outputs on CPU: what dump_outputs writes (names, dtypes, the slots past a query's count, the seeded sample of an
output above the size cap) and that --steps below 1 is refused before anything runs."""
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT


def _answers(nq, k, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, k + 1, nq).astype(np.int32)
    counts[0] = k
    return {"ids": rng.integers(0, 1 << 40, (nq, k)).astype(np.int64), "dists": rng.random((nq, k), dtype=np.float32),
            "counts": counts, "layers": rng.integers(0, 4, (nq, k)).astype(np.uint8),
            "ranks": rng.integers(0, 1 << 20, (nq, k)).astype(np.int32)}


def test_dump_outputs_writes_what_the_caller_gets(tmp_path):
    import bench
    a = _answers(200, 10, 1)
    names = bench.dump_outputs(str(tmp_path / "out"), a)
    assert names == ["counts", "dists", "ids", "layers", "ranks"]
    got = {n: np.load(tmp_path / "out" / (n + ".npy")) for n in names}
    assert got["dists"].dtype == np.float32 and all(got[n].dtype == np.float64 for n in ("ids", "counts", "layers", "ranks"))
    assert np.array_equal(got["counts"], a["counts"])
    for i, c in enumerate(a["counts"]):
        assert np.array_equal(got["ids"][i, :c], a["ids"][i, :c]) and (got["ids"][i, c:] == -1).all()
        assert np.array_equal(got["dists"][i, :c].view(np.uint32), a["dists"][i, :c].view(np.uint32))
        assert np.isinf(got["dists"][i, c:]).all()
        assert np.array_equal(got["ranks"][i, :c], a["ranks"][i, :c]) and (got["layers"][i, c:] == -1).all()


def test_dump_outputs_samples_the_same_rows_above_the_cap(tmp_path):
    import bench
    a = _answers(5000, 10, 2)
    cap = 200_000
    for run in ("one", "two"):
        names = bench.dump_outputs(str(tmp_path / run), a, max_bytes=cap)
        assert "rows" in names
        assert sum(os.path.getsize(tmp_path / run / (n + ".npy")) - 128 for n in names) <= cap  # (128: the .npy header)
    rows = np.load(tmp_path / "one" / "rows.npy")
    assert np.array_equal(rows, np.load(tmp_path / "two" / "rows.npy")) and len(rows) < 5000
    assert np.all(np.diff(rows) > 0)
    r = rows.astype(np.int64)
    c = a["counts"][r]
    assert np.array_equal(np.load(tmp_path / "one" / "counts.npy"), c)
    ids = np.load(tmp_path / "one" / "ids.npy")
    assert np.array_equal(ids[c > 0, 0], a["ids"][r][c > 0, 0].astype(np.float64))


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
