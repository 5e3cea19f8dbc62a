"""bench.py's result line and --dump-outputs: a plain run times exactly --steps steps and measures nothing else (the CPU baseline and
the context legs come with --full); the dumped arrays are what the timed path returned, within a 64 MiB budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_within_budget_is_exact_and_keeps_shapes(tmp_path):
    a = torch.randn(3, 4, 5)
    b = torch.randn(7, dtype=torch.float64)
    c = torch.randn(6).to(torch.bfloat16)
    bench.dump_outputs({"a": a, "b": b, "c": c}, str(tmp_path))
    ra, rb, rc = (np.load(tmp_path / f"{n}.npy") for n in "abc")
    assert ra.dtype == np.float32 and ra.shape == (3, 4, 5) and np.array_equal(ra, a.numpy())
    assert rb.dtype == np.float64 and np.array_equal(rb, b.numpy())
    assert rc.dtype == np.float32 and np.array_equal(rc, c.float().numpy())


def test_dump_over_budget_is_a_fixed_sample(tmp_path):
    big = torch.arange(20 << 20, dtype=torch.float32)          # 80 MiB on its own
    small = torch.arange(1 << 20, dtype=torch.float64)         # 8 MiB
    for d in ("x", "y"):
        bench.dump_outputs({"big": big, "small": small}, str(tmp_path / d))
    total = sum(os.path.getsize(tmp_path / "x" / f"{n}.npy") for n in ("big", "small"))
    assert total <= bench.DUMP_BUDGET_BYTES + 1024             # (two .npy headers)
    for n, src in (("big", big), ("small", small)):
        x, y = np.load(tmp_path / "x" / f"{n}.npy"), np.load(tmp_path / "y" / f"{n}.npy")
        assert np.array_equal(x, y) and x.dtype == src.numpy().dtype
        assert x.ndim == 1 and 0 < len(x) < src.numel() and np.all(np.diff(x) >= 0)   # sorted flat indices of an arange
        assert np.isin(x, src.numpy()).all()


@pytest.mark.gpu
@pytest.mark.parametrize("train", [False, True])
def test_plain_run_times_steps_and_dumps_the_last_step(cuda, tmp_path, train):
    B, T = 4, 4
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(B),
           "--frames", str(T), "--dump-outputs", str(tmp_path / "out")] + (["--train"] if train else [])
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and rec["dtype"] == "f32" and rec["higher_is_better"] is True
    assert abs(rec["value"] - B * T / (rec["ms_per_step"] * 1e-3)) <= 1e-6 * rec["value"]
    assert rec["median_ms_per_step"] is None and rec["cpu_baseline"] is None
    assert rec["train"] is None and rec["config0"] is None and rec["model"] is None
    traj = np.load(tmp_path / "out" / "trajectory.npy")
    z0 = torch.randn(B, 64, 16, 16, generator=torch.Generator().manual_seed(1234)) * 0.5     # bench.py's z0 on rank 0
    assert traj.dtype == np.float32 and traj.shape == (T, B, 64, 16, 16)
    assert np.array_equal(traj[0], z0.numpy()) and np.isfinite(traj).all() and not np.array_equal(traj[-1], traj[0])
    names = sorted(os.listdir(tmp_path / "out"))
    if train:
        assert "grad_z0.npy" in names and np.load(tmp_path / "out" / "grad_z0.npy").shape == (B, 64, 16, 16)
        assert len([n for n in names if n.startswith("grad_gradient_net_")]) == 10      # 5 convs x (weight, bias)
    else:
        assert names == ["trajectory.npy"]
