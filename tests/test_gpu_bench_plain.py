"""bench.py without --full measures the headline figure only, and --full adds every other leg without changing it: the same
arguments time the same steps and dump the same answers either way."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "config")


def _bench(args, timeout=420):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    return r, (json.loads(lines[-1]) if lines else None)


def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    common = ["--gpus", "1", "--n", "20000", "--nq", "1000", "--steps", "6", "--warmup", "2"]
    runs = {}
    for name, extra in (("plain", []), ("full", ["--full", "--no-traffic", "--cpu-seconds", "1"])):
        out = tmp_path / ("out_" + name)
        r, j = _bench(common + extra + ["--cache-dir", str(tmp_path / ("cache_" + name)), "--dump-outputs", str(out)])
        assert r.returncode == 0 and j is not None, r.stdout[-2000:] + r.stderr[-4000:]
        runs[name] = (j, out, r.stderr)
    (p, po, perr), (f, fo, _) = runs["plain"], runs["full"]

    assert p["full"] is False and f["full"] is True
    for key in HEADLINE:
        assert p[key] == f[key], key
    for j in (p, f):
        assert j["value"] > 0 and j["ms_per_step"] > 0
        assert abs(j["value"] - 1000 * 1e3 / j["ms_per_step"]) <= 1e-2 * j["value"]  # value and ms_per_step: one measurement
        assert j["roofline"]["kernel_ms"] > 0 and len(j["roofline"]["kernel_ms_by_batch_min_median_max"]) == 4

    # the plain run: nothing beyond the timed steps
    assert p["recall_at_10"] is None and p["cpu_baseline"] is None and p["parity_vs_oracle"] is None and p["boundary"] is None
    assert p["strict_ties"]["fast_mode_queries_per_s"] is None and p["simd_order_queries_per_s"] is None
    assert p["two_caller_threads_queries_per_s"] is None and p["one_caller_two_tickets_queries_per_s"] is None
    assert p["roofline"]["achieved"] is None and p["roofline"]["frac"] is None and "per_query" not in p["roofline"]
    assert "oracle" not in perr and "roofline.traffic" not in perr

    # --full: every leg there, and the device still answers as the oracle does
    assert f["recall_at_10"]["by_id"] > 0.5 and f["boundary"]["host_buffers_queries_per_s"] > 0
    assert f["strict_ties"]["fast_mode_queries_per_s"] > 0 and f["simd_order_queries_per_s"] > 0
    assert f["two_caller_threads_queries_per_s"] > 0
    assert f["roofline"]["frac"] > 0 and f["roofline"]["per_query"]["n_dist"] > 0
    assert f["cpu_baseline"]["value"] > 0 and f["parity_vs_oracle"]["tie_free_ids_identical"]

    names = sorted(os.listdir(po))
    assert names == ["counts.npy", "dists.npy", "ids.npy", "layers.npy", "ranks.npy"] and sorted(os.listdir(fo)) == names
    for n in names:
        assert np.array_equal(np.load(po / n), np.load(fo / n)), n + " differs between the plain and the --full run"
