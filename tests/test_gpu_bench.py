"""bench.py's two modes on the device: a plain run prints the contract and nothing that takes work of its own; `--full` adds the
secondary figures (here without its child runs, CPU baseline and training step, which the --no-* options take out)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup")
FULL_ONLY = ("value_range_check_deferred", "roofline", "kernels", "other_kernels_ms_per_step", "sum_kernel_ms", "value_unprimed",
             "value_ragged_masks", "cpu_baseline", "train_step")


def _run(flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1"] + flags,
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(rows) == 1, r.stdout[-2000:]
    return json.loads(rows[0])


def test_plain_run_prints_the_contract_only():
    d = _run([])
    assert all(k in d for k in CONTRACT), sorted(d)
    assert d["metric"] == "EGNN.forward graphs/sec" and d["unit"] == "graphs/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 4 and d["warmup"] == 1 and d["n_gpus"] == 1
    # value = graphs of the K steps / their time
    graphs = d["config"]["global_batch"]
    assert abs(d["value"] - graphs / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"] + 0.02, (d["value"], d["ms_per_step"])
    assert not [k for k in FULL_ONLY if k in d], sorted(d)


def test_full_run_adds_the_secondary_figures():
    d = _run(["--full", "--no-cpu-baseline", "--no-train-step", "--no-live-traffic"])
    assert all(k in d for k in CONTRACT) and d["value"] > 0
    assert d["value_range_check_deferred"] > 0
    assert d["roofline"]["kernel"] in {k["kernel"] for k in d["kernels"]} and d["sum_kernel_ms"] > 0
    assert not [k for k in ("cpu_baseline", "train_step", "value_unprimed", "value_ragged_masks") if k in d], sorted(d)
