"""bench.py --full: a plain run prints the headline line without the legs that take runs of their own; --full adds them after the
timed steps and the dump, so both runs write the very same --dump-outputs arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("graph_replay_ms_per_step", "dp_path_ms_per_step", "train_loop", "val_auroc", "stress", "binning", "cpu_baseline")


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--prewarm-s", "0",
           "--dump-outputs", str(out_dir)] + list(extra)
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_legs(tmp_path):
    plain = _bench(tmp_path / "plain")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert k in plain, k
    assert plain["steps"] == 3 and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert not [k for k in LEGS if k in plain]
    # (the CPU baseline and the entrypoint's AUROC are the slow legs: left out by their own options; the training loop kept short)
    full = _bench(tmp_path / "full", "--full", "--no-cpu-baseline", "--no-val-auroc", "--train-loop-steps", "20", "--train-loop-genes", "1024")
    for k in ("graph_replay_ms_per_step", "dp_path_ms_per_step", "train_loop", "stress", "binning"):
        assert k in full, k
    assert "cpu_baseline" not in full and "val_auroc" not in full
    assert full["train_loop"]["steps"] == 20 and full["stress"]["genes_per_s"] > 0 and full["binning"]["achieved"] > 0
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == ["logits.npy", "loss.npy", "params.npy"] and sorted(os.listdir(tmp_path / "full")) == files
    for f in files:
        assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)), f
