"""bench.py's plain run on the MI355X: the headline alone, --steps timed steps, and --dump-outputs writing the latents the timed
path left -- the same ones from run to run with the same arguments, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"loopA_surfPos": (512, 30, 6), "loopB_surfPos": (512, 60, 6), "loopC_surfZ": (512, 60, 48)}


def _run(out_dir, steps=7, warmup=2):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0]), {k: np.load(os.path.join(out_dir, k + ".npy")) for k in SHAPES}


@pytest.mark.gpu
def test_plain_run_headline_and_dumped_outputs(tmp_path):
    line, outs = _run(tmp_path / "a")
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert line[key] is not None, key
    assert line["steps"] == 7 and sum(line["config"]["steps_per_loop"].values()) == 7 and line["full"] is False
    assert line["higher_is_better"] is True and line["dtype"] == "bf16" and line["config"]["finite"]
    assert abs(line["value"] * line["ms_per_step"] - 1e3) < 2.0                # one GPU: steps/s = 1000 / ms per step
    assert line["extra"] == {} and line["roofline"] is None and "cpu_baseline" not in line    # side measurements: --full only
    for k, shape in SHAPES.items():
        assert outs[k].shape == shape and outs[k].dtype == np.float32 and np.isfinite(outs[k]).all(), k
    assert sum(v.nbytes for v in outs.values()) <= 64 << 20
    _, again = _run(tmp_path / "b")
    for k in SHAPES:
        assert np.array_equal(outs[k], again[k]), k
