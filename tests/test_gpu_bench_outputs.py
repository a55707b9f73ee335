"""bench.py --dump-outputs on the device: the same arguments give the timed steps the same inputs -- two runs that each build
their own graph (separate caches) build the same one and dump the same answers -- and what is dumped is what the last timed
step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(args, timeout=420):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, (json.loads(lines[-1]) if lines else None)


def test_dump_outputs_same_arguments_same_answers(tmp_path):
    common = ["--gpus", "1", "--n", "20000", "--nq", "1000", "--warmup", "1", "--no-cpu-baseline", "--no-recall", "--no-concurrent",
              "--no-boundary", "--no-traffic"]
    runs = []
    # 5 timed steps over 4 batches: the last one searches batch 0 again, as does the only step of the second run
    for name, steps in (("a", 5), ("b", 1)):
        cache, out = tmp_path / ("cache_" + name), tmp_path / ("out_" + name)
        r, j = _bench(common + ["--steps", str(steps), "--cache-dir", str(cache), "--dump-outputs", str(out),
                                "--dump-answers", str(tmp_path / (name + ".npz"))])
        assert r.returncode == 0 and j is not None, r.stdout[-2000:] + r.stderr[-4000:]
        assert j["steps"] == steps and j["ms_per_step"] > 0
        assert len(j["roofline"]["kernel_ms_by_batch_min_median_max"]) == min(steps, 4)  # one kernel time per timed step
        runs.append((cache, out))
    (ca, oa), (cb, ob) = runs
    for f in sorted(os.listdir(ca)):
        if f.endswith((".graph", ".data")):
            assert (ca / f).read_bytes() == (cb / f).read_bytes(), f + ": the two builds of the graph differ"
    names = sorted(os.listdir(oa))
    assert names == ["counts.npy", "dists.npy", "ids.npy", "layers.npy", "ranks.npy"] and sorted(os.listdir(ob)) == names
    for f in names:
        a, b = np.load(oa / f), np.load(ob / f)
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype
        assert np.array_equal(a, b), f + " differs between the two runs"
    ans = np.load(tmp_path / "a.npz")  # batch 0 once more after everything else: the same answers
    c = ans["counts"].astype(np.int64)
    assert np.array_equal(np.load(oa / "counts.npy"), c)
    valid = np.arange(ans["ids"].shape[1])[None, :] < c[:, None]
    assert np.array_equal(np.load(oa / "ids.npy")[valid], ans["ids"][valid].astype(np.float64))
    assert np.array_equal(np.load(oa / "dists.npy")[valid].view(np.uint32), ans["dists"][valid].view(np.uint32))
