"""bench.py's launch contract on CPU: `python bench.py --gpus N` run bare spawns N ranks itself (one per GPU under
torch.distributed.run, rendezvous on 127.0.0.1) and refuses a WORLD_SIZE / --gpus mismatch loudly."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    return env


@pytest.mark.timeout(600)
def test_bare_launch_spawns_one_rank_per_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--dry-run"], capture_output=True, text=True, env=_env(), timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout                      # rank 0 prints ONE JSON line
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["ranks_seen"] == 2 and line["steps"] == 3 and line["dry_run"] is True


def test_world_size_mismatch_fails_loudly():
    env = _env()
    env.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry-run"], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_more_gpus_than_the_node_has_fails_loudly():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True,
                       env=_env(), timeout=300)
    assert r.returncode != 0 and "exposes" in (r.stderr + r.stdout)


def test_every_tool_script_compiles():
    """tools/*.py run on the GPU box only; a syntax error there costs a gpurun call -- compile them all here."""
    import glob
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "tools", "*.py")))
    assert len(files) >= 20
    for f in files:
        compile(open(f).read(), f, "exec")


def test_full_and_dump_outputs_options():
    """A plain run times the headline alone; --full adds the side measurements, --dump-outputs writes the timed path's latents.
    --steps sets the number of timed steps, so a run without any is refused."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--dry-run"], capture_output=True, text=True,
                       env=_env(), timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr


def test_split_steps_sums_to_steps():
    sys.path.insert(0, ROOT)
    import bench
    for k in range(1, 1000):
        ka, kb, kc = bench.split_steps(k)
        assert ka + kb + kc == k and min(ka, kb, kc) >= 0
        if k >= 3:
            assert min(ka, kb, kc) >= 1


def test_dump_outputs_float32_and_capped(tmp_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    small = {"a": torch.randn(3, 4, dtype=torch.bfloat16), "b": torch.arange(6.0, dtype=torch.float64).reshape(2, 3)}
    bench.dump_outputs(str(tmp_path / "small"), small)
    for k, v in small.items():
        got = np.load(tmp_path / "small" / (k + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, v.float().numpy())
    big = {"x": torch.randn(6000, 60, 48), "y": torch.randn(6000, 60, 6)}      # 77.8 MB: sampled down to the cap
    for d in ("big1", "big2"):
        bench.dump_outputs(str(tmp_path / d), big)
    x1, y1 = np.load(tmp_path / "big1" / "x.npy"), np.load(tmp_path / "big1" / "y.npy")
    assert 0 < x1.nbytes + y1.nbytes <= bench.DUMP_BYTES and x1.shape[0] == y1.shape[0] < 6000
    assert np.array_equal(x1, np.load(tmp_path / "big2" / "x.npy"))            # the sample is fixed
    assert any(np.array_equal(x1[0], r) for r in big["x"].numpy()[:x1.shape[0] + 1000])
