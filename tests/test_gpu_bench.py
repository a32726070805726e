"""GPU: bench.py's plain run -- exactly --steps timed steps, the headline fields, no other leg, and --dump-outputs
writing what the last timed step returned (bitwise what the same seeded steps give through the library here)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("roofline", "exact_f32_mfma", "batch_sweep", "configs", "replay_sampler", "learner", "train_loop", "icem",
        "cpu_baseline", "single_env")


def test_plain_run_dumps_last_timed_step(tmp_path):
    steps, warmup = 3, 2
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup
    assert d["unit"] == "plan-steps/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(d["config"]["envs_per_gpu"] * 1e3 / d["ms_per_step"], rel=1e-3)
    assert all(d.get(k) is None for k in LEGS), [k for k in LEGS if d.get(k) is not None]
    assert sorted(os.listdir(out)) == ["actions.npy", "metrics.npy"]
    a, m = np.load(out / "actions.npy"), np.load(out / "metrics.npy")

    # the same seeded steps in this process: the dump is the (warmup + steps)-th call's result
    import bench
    from tdmpc_amd.config import bench_cfg
    from tdmpc_amd.parallel import EnvShardedPlanner
    cfg = bench_cfg("humanoid-run")
    cfg.device = "cuda:0"
    B = d["config"]["envs_per_gpu"]
    np.random.seed(2)
    agent = bench.make_agent(cfg, B, "fused", True, 1)
    obs = torch.from_numpy(bench.synthetic_obs(cfg, B, seed=0)).to("cuda:0")
    sharded = EnvShardedPlanner(B, cfg.action_dim, agent=agent)
    for i in range(warmup + steps):
        ra, rm = sharded.plan(obs, 10**6, t0=(i % 100 == 0))
    assert a.dtype == np.float32 and a.shape == (B, cfg.action_dim) and m.shape == (B, 2)
    assert np.isfinite(a).all() and np.isfinite(m).all()
    assert np.array_equal(a, ra.cpu().numpy()) and np.array_equal(m, rm.cpu().numpy())
