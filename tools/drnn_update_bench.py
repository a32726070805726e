"""Time of the DSSM update on one MI355X: the segmented intrinsic-reward pass against separate passes, and the whole
`DssmLearner` update on its HIP path against its PyTorch path on the same GPU.

    python tools/drnn_update_bench.py [--out profiles/r09/drnn_update_bench.json] [--reps 7] [--calls 20]   (--out '' writes no file)

The humanoid shape (L 100, A 21, Hd 128, mlp_dim 512), B = 512, H = 5, weights synthetic_dssm_state_dict seeds 0 / 1, a
fixed batch:
  intrinsic:  `DssmTrainStep.intrinsic_loss` with S = H + 1 = 6 segments (one launch chain over 3072 rows, both
              BatchNorms per segment) against six `next` (h = zeros) + `similarity_loss` forward calls of 512 rows;
              the two sides' losses are compared bitwise before timing.
  update:     `DssmLearner.update` on the HIP path, eagerly launched and as graph replay, against the same class built
              with TDMPC_DSSM_LEARNER_HIP=0 (the reference's order of operations on PyTorch-ROCm, eagerly launched and
              as graph replay), and against `dssm_engine.DssmEngineLearner`, the same update on the explicit learner
              engine, eagerly launched and as graph replay, all six legs in the same run.
Per leg and side: a warm-up, then `reps` timed batches of `calls` calls between HIP events, the sides alternating batch
by batch; the median is the figure, min / max the spread. No GPU: it fails.
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
    return make_cfg("humanoid", hidden_dim=128, norm_cell=True, plan2expl=False, warmup_len=0, horizon=5,
                    batch_size=512, optim_id="adamw")


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


def models(cfg):
    from tdmpc_amd.dssm import DSSM, synthetic_dssm_state_dict
    out = []
    for seed in (0, 1):
        m = DSSM(cfg, init="none")
        m.load_state_dict(synthetic_dssm_state_dict(cfg, seed))
        out.append(m.cuda().eval())
    return out


def learner(cfg, hip, graph):
    from tdmpc_amd.drnn_learner import DssmLearner
    model, target = models(cfg)
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cuda"), planner=None)
    old = os.environ.get("TDMPC_DSSM_LEARNER_HIP")
    os.environ["TDMPC_DSSM_LEARNER_HIP"] = "1" if hip else "0"
    try:
        ln = DssmLearner(agent, graph=graph, warmup=3)
    finally:
        if old is None:
            del os.environ["TDMPC_DSSM_LEARNER_HIP"]
        else:
            os.environ["TDMPC_DSSM_LEARNER_HIP"] = old
    assert ln.hip == hip
    buf = FixedBatch(cfg)
    count = [0]

    def update():
        count[0] += 1
        return ln.update(buf, 100000 + count[0])
    return ln, update


def engine_learner(cfg, graph):
    from tdmpc_amd.dssm_engine import DssmEngineLearner
    model, target = models(cfg)
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cuda"), planner=None)
    ln = DssmEngineLearner(agent, graph=graph, warmup=3)
    buf = FixedBatch(cfg)
    count = [0]

    def update():
        count[0] += 1
        return ln.update(buf, 100000 + count[0])
    return ln, update


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r09", "drnn_update_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("drnn_update_bench needs a GPU: nothing is measured without one")
    from tdmpc_amd.dssm_train import DssmTrainStep
    cfg = bench_cfg()
    H, B, L, A, Hd = cfg.horizon, cfg.batch_size, cfg.latent_dim, cfg.action_dim, cfg.hidden_dim
    S = H + 1
    out = {"shape": f"humanoid L{L} A{A} Hd{Hd} M{cfg.mlp_dim} B{B} H{H}", "device": torch.cuda.get_device_name(0),
           "calls_per_batch": args.calls}

    # ---- the intrinsic pass
    model = models(cfg)[0].train()
    step = DssmTrainStep(model, max_rows=B, max_steps=1, max_loss_rows=B, max_losses=1)
    rs = np.random.RandomState(0)
    f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).cuda()  # noqa: E731
    z, a, keys = f(S * B, L), f(S * B, A).clamp(-1, 1), f(S * B, L)
    h0 = torch.zeros(B, Hd, device="cuda")
    stats = [t for k, t in model.state_dict().items() if k.endswith(("running_mean", "running_var"))]
    kept = [t.clone() for t in stats]

    def restore():
        for t, k in zip(stats, kept):
            t.copy_(k)

    def segmented():
        return step.intrinsic_loss(z, a, keys, S)

    @torch.no_grad()
    def separate():
        return torch.cat([step.similarity_loss(step.next(z[s * B:(s + 1) * B], a[s * B:(s + 1) * B], h0)[0],
                                               keys[s * B:(s + 1) * B]) for s in range(S)])
    restore()
    got = segmented()
    restore()
    want = separate()
    torch.cuda.synchronize()
    res = alternate({"segmented": segmented, "separate": separate}, args.reps, args.calls)
    out["intrinsic"] = {"segments": S, "rows_per_segment": B, "bitwise_equal": bool(torch.equal(got, want)),
                        "launches": {"segmented": 11, "separate": S * (7 + 5)}, **res,
                        "separate_over_segmented": round(res["separate"]["us_median"] /
                                                         res["segmented"]["us_median"], 3)}
    print(json.dumps({"intrinsic": out["intrinsic"]}), flush=True)

    # ---- the whole update
    sides, learners = {}, {}
    for name, hip, graph in (("hip_eager", True, False), ("hip_graph", True, True), ("torch_eager", False, False),
                             ("torch_graph", False, True)):
        learners[name], sides[name] = learner(cfg, hip, graph)
    for name, graph in (("engine_eager", False), ("engine_graph", True)):
        learners[name], sides[name] = engine_learner(cfg, graph)
    res = alternate(sides, args.reps, args.calls)
    for name in ("hip_graph", "torch_graph", "engine_graph"):
        assert learners[name]._graphs, f"{name}: never replayed a captured graph"
    out["update"] = {**res,
                     "hip_graph_over_engine_graph": round(res["hip_graph"]["us_median"] /
                                                          res["engine_graph"]["us_median"], 3),
                     "hip_eager_over_engine_eager": round(res["hip_eager"]["us_median"] /
                                                          res["engine_eager"]["us_median"], 3),
                     "torch_eager_over_hip_eager": round(res["torch_eager"]["us_median"] /
                                                         res["hip_eager"]["us_median"], 3),
                     "torch_graph_over_hip_graph": round(res["torch_graph"]["us_median"] /
                                                         res["hip_graph"]["us_median"], 3),
                     "torch_eager_over_hip_graph": round(res["torch_eager"]["us_median"] /
                                                         res["hip_graph"]["us_median"], 3)}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
