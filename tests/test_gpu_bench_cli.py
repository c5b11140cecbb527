"""bench.py as a program: a plain run does its timed steps and prints the headline line and nothing that belongs behind --full, and
--dump-outputs writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("other_schedule", "other_input_feed", "random_init", "other_configs", "cpu_baseline", "graph_replay", "data_parallel")


def test_plain_run_prints_the_headline_line_and_dumps_the_last_steps_outputs(tmp_path):
    out_dir = str(tmp_path / "arrays")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--pretrain-steps", "5", "--dump-outputs", out_dir]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 1, out.stdout[:2000]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "windows/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(8 * 1e3 / d["ms_per_step"], rel=1e-6)      # PEMS04: 8 windows per step
    assert d["roofline"]["launches_in_timed_region"] == 3                                                  # --steps IS the number of timed steps
    assert d["roofline"]["ms_per_launch_alone"] is None and not [k for k in FULL_ONLY if k in d], sorted(d)
    got = {f: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    assert sorted(got) == ["adj_knn.npy", "grad_norm.npy", "loss.npy", "prediction.npy", "theta.npy"]
    assert got["prediction.npy"].shape == (8, 12, 307, 1) and got["theta.npy"].shape == (8, 307, 307)
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert float(got["loss.npy"].reshape(-1)[0]) == pytest.approx(d["config"]["final_loss"], rel=1e-6)
    assert sum(a.nbytes for a in got.values()) <= 64e6


def _rel_l2(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(a), 1e-30))


def test_two_runs_with_the_same_arguments_dump_the_same_outputs(tmp_path):
    """Two plain runs with the same arguments must write the same arrays up to rounding.  The bound: every array is f32 and, for equal parameters
    and inputs, the bf16-mode forward is bit-reproducible (tests/test_gpu_step.py::test_wavenet_phase_5_plus_6_is_phase_1 asserts it), so all that
    may differ is the order of f32 additions in reductions of up to ~1e4 terms: 6e-8 * sqrt(1e4) = 6e-6 -> rel-L2 1e-5 per array; adj_knn
    (a 0/1 mask) equal.  What makes it hold although the weight-gradient kernels sum with floating-point atomics (two pre-training runs: all
    parameters 4.8e-9 apart after one step, 5.9e-4 after twenty; two benchmark runs that train 25 steps from random initialisation: prediction
    1.6e-2 apart): the checkpoint is a stored run of the recipe (bench.stored_checkpoint) and the last timed step starts from the seeded
    initial state (bench.InitialState)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    got = []
    for tag in ("a", "b"):
        out_dir = str(tmp_path / tag)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", out_dir]
        out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        got.append({f: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))})
    assert sorted(got[0]) == sorted(got[1])
    err = {f: _rel_l2(got[0][f], got[1][f]) for f in got[0]}
    print("run-to-run rel-L2:", err)
    assert np.array_equal(got[0]["adj_knn.npy"], got[1]["adj_knn.npy"]), err
    assert all(e < 1e-5 for e in err.values()), err
