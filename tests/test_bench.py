"""bench.py's command line: a plain run is the headline only, --steps is the exact number of timed closure evaluations,
--dump-outputs writes what the last timed step handed its caller."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)


def test_bench_refuses_zero_steps():
    r = _bench(["--gpus", "1", "--steps", "0"])
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_plain_bench_run_times_exact_steps_and_dumps_outputs(tmp_path):
    """An odd --steps under L-BFGS as the reference constructs it (2 closure evaluations per optimiser step): the timed
    region still holds exactly that many evaluations; the plain record carries no --full measurement."""
    out = tmp_path / "dump"
    r = _bench(["--gpus", "1", "--levels", "2", "--steps", "5", "--warmup", "3", "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in rec, key
    assert rec["unit"] == "iters/s" and rec["higher_is_better"] is True
    assert rec["steps"] == 5
    assert rec["value"] == pytest.approx(1e3 / rec["ms_per_step"], rel=1e-6)
    for key in ("roofline", "kernel_ms_per_closure", "cpu_baseline", "sustained", "exact_f32", "progressing_job",
                "direct_convolution"):
        assert key not in rec, key
    image = np.load(out / "image.npy")
    rows = np.load(out / "loss_rows.npy")
    assert image.dtype == np.float32 and image.shape == (512, 768, 3) and np.isfinite(image).all()
    # two evaluations of the last optimiser step, then the trailing single one; a row is 4 per level + the grand total
    assert rows.dtype == np.float32 and rows.shape == (3, 4 * 2 + 1) and np.isfinite(rows).all() and (rows[:, -1] > 0).all()
    assert sorted(os.listdir(out)) == ["image.npy", "loss_rows.npy"]
