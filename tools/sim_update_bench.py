"""Time of the similarity TD-MPC agent's update on one MI355X: the whole `SimLearner` update on the learner engine
against its PyTorch path on the same GPU, with the stock TOLD engine update at the same shape beside them for scale.

    python tools/sim_update_bench.py [--out profiles/r12/sim_update_bench.json] [--reps 7] [--calls 20]   (--out '' writes no file)

The humanoid shape (L 100, A 21, mlp_dim 512, enc_dim 256), B = 512, H = 5, weights synthetic_icem_mlp_state_dict seeds
0 / 1 (the TOLD engine: synthetic_state_dict seeds 0 / 1), a fixed batch:
  engine_eager / engine_graph:  `SimLearner.update` on the engine path (tdmpc_amd/sim_engine.py), eagerly launched and
                                as graph replay;
  torch_eager / torch_graph:    the same class built with TDMPC_SIM_LEARNER_ENGINE=0 -- the reference's order of
                                operations on PyTorch-ROCm -- eagerly launched and as graph replay. The parent commit has
                                no such update to compare with;
  told_engine_graph:            `learner.Learner.update` (TDMPC.update on the stock engine: the plain encoder, the
                                consistency term) as graph replay, in the same run.
A warm-up, then `reps` timed batches of `calls` calls between HIP events, the sides alternating batch by batch; the
median is the figure, min / max the spread. No GPU: it fails.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tdmpc_amd.config import make_cfg  # noqa: E402


def bench_cfg():
    return make_cfg("humanoid", horizon=5, batch_size=512, optim_id="adamw")


class FixedBatch:
    """A replay buffer that hands out one batch (the update's cost does not depend on which)."""
    graph_safe = True
    idx, _full = 0, False

    def __init__(self, cfg, seed=0):
        rs = np.random.RandomState(seed)
        B, H, O, A = cfg.batch_size, cfg.horizon, cfg.obs_shape[0], cfg.action_dim
        f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).cuda()  # noqa: E731
        self.b = (f(B, O), f(H + 1, B, O), f(H + 1, B, A).clamp(-1, 1), f(H + 1, B, 1),
                  torch.arange(B, device="cuda"), torch.from_numpy(rs.uniform(0.5, 1, B).astype(np.float32)).cuda())
        self.prio = None

    def sample(self):
        return self.b

    def update_priorities(self, idxs, p):
        self.prio = p


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3   # us per call


def summary(us):
    med = statistics.median(us)
    return {"us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
            "spread_frac": round((max(us) - min(us)) / med, 4), "batches": len(us)}


def alternate(sides, reps, calls, warm=5):
    for _ in range(warm):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in sides}
    for _ in range(reps):
        for k, fn in sides.items():
            us[k].append(timed(fn, calls))
    return {k: summary(v) for k, v in us.items()}


def counted(ln, buf):
    count = [0]

    def update():
        count[0] += 1
        return ln.update(buf, 100000 + count[0])
    return update


def sim_learner(cfg, engine, graph):
    from tdmpc_amd.icem_mlp import IcemMlpModel, synthetic_icem_mlp_state_dict
    from tdmpc_amd.sim_learner import SimLearner
    ms = []
    for seed in (0, 1):
        m = IcemMlpModel(cfg, init="none")
        m.load_state_dict(synthetic_icem_mlp_state_dict(cfg, seed))
        ms.append(m.cuda().eval())
    agent = SimpleNamespace(cfg=cfg, model=ms[0], model_target=ms[1], device=torch.device("cuda"), planner=None)
    old = os.environ.get(SimLearner.ENGINE_ENV)
    os.environ[SimLearner.ENGINE_ENV] = "1" if engine else "0"
    try:
        ln = SimLearner(agent, graph=graph, warmup=3)
    finally:
        if old is None:
            del os.environ[SimLearner.ENGINE_ENV]
        else:
            os.environ[SimLearner.ENGINE_ENV] = old
    assert ln.path == ("engine" if engine else "torch")
    return ln, counted(ln, FixedBatch(cfg))


def told_learner(cfg):
    """TDMPC.update on the stock engine, without a planner to repack."""
    from tdmpc_amd.learner import Learner
    from tdmpc_amd.told import TOLD, synthetic_state_dict
    ms = []
    for seed in (0, 1):
        m = TOLD(cfg, init="none")
        m.load_state_dict(synthetic_state_dict(cfg, seed))
        ms.append(m.cuda().eval())
    planner = SimpleNamespace(_packed_model=None, _ptr_arr=None, _packed_key=None, pack=lambda model: None)
    agent = SimpleNamespace(cfg=cfg, model=ms[0], model_target=ms[1], device=torch.device("cuda"), planner=planner)
    ln = Learner(agent, graph=True, warmup=3)
    assert ln.engine is not None
    return ln, counted(ln, FixedBatch(cfg))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r12", "sim_update_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sim_update_bench needs a GPU: nothing is measured without one")
    cfg = bench_cfg()
    H, B, L, A = cfg.horizon, cfg.batch_size, cfg.latent_dim, cfg.action_dim
    out = {"shape": f"humanoid L{L} A{A} M{cfg.mlp_dim} E{cfg.enc_dim} B{B} H{H}",
           "device": torch.cuda.get_device_name(0), "calls_per_batch": args.calls}
    sides, learners = {}, {}
    for name, engine, graph in (("engine_eager", True, False), ("engine_graph", True, True),
                                ("torch_eager", False, False), ("torch_graph", False, True)):
        learners[name], sides[name] = sim_learner(cfg, engine, graph)
    learners["told_engine_graph"], sides["told_engine_graph"] = told_learner(cfg)
    res = alternate(sides, args.reps, args.calls)
    for name in ("engine_graph", "torch_graph", "told_engine_graph"):
        assert learners[name]._graphs, f"{name}: never replayed a captured graph"
    us = {k: v["us_median"] for k, v in res.items()}
    out["update"] = {**res,
                     "torch_eager_over_engine_eager": round(us["torch_eager"] / us["engine_eager"], 3),
                     "torch_graph_over_engine_graph": round(us["torch_graph"] / us["engine_graph"], 3),
                     "torch_eager_over_engine_graph": round(us["torch_eager"] / us["engine_graph"], 3),
                     "engine_graph_over_told_engine_graph": round(us["engine_graph"] / us["told_engine_graph"], 3)}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
