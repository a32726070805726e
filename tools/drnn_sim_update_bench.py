"""Time of the MPC DSSM agent's update on one MI355X: the intrinsic chain pass with the recurrence as a launch chain
(mode 0), in one launch (mode 1) and as separate calls, and the whole `DssmSimLearner` update on its HIP path against
its PyTorch path on the same GPU.

    python tools/drnn_sim_update_bench.py [--out profiles/r10/drnn_sim_update_bench.json] [--reps 7] [--calls 20]   (--out '' writes no file)

The humanoid shape (L 100, A 21, Hd 128, mlp_dim 512), B = 512, H = 5, W = warmup_len = 2, weights
synthetic_dssm_state_dict seeds 0 / 1, a fixed batch:
  intrinsic:  `DssmTrainStep.intrinsic_chain_loss` with S = H + 1 = 6 segments in mode 0 and in mode 1 against six
              `next` calls with the hidden state handed on + four `similarity_loss` forward calls of 512 rows; mode 0 is
              compared with the separate calls bitwise, mode 1 by its largest difference, before timing.
  update:     `DssmSimLearner.update` on the HIP path, eagerly launched and as graph replay, against the same class
              built with TDMPC_DSSM_LEARNER_HIP=0 (the reference's order of operations on PyTorch-ROCm, eagerly
              launched and as graph replay). The parent commit has no such update to compare with.
Method as tools/drnn_update_bench.py (whose helpers this uses): per leg and side a warm-up, then `reps` timed batches of
`calls` calls between HIP events, the sides alternating batch by batch; the median is the figure, min / max the
spread. No GPU: it fails.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from drnn_update_bench import FixedBatch, alternate, models  # noqa: E402
from tdmpc_amd.config import make_cfg  # noqa: E402


def bench_cfg():
    return make_cfg("humanoid", hidden_dim=128, norm_cell=True, plan2expl=False, warmup_len=2, horizon=5,
                    batch_size=512, optim_id="adamw", similarity_horizon=1)


def learner(cfg, hip, graph):
    from tdmpc_amd.drnn_learner import DssmSimLearner
    model, target = models(cfg)
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cuda"), planner=None)
    old = os.environ.get("TDMPC_DSSM_LEARNER_HIP")
    os.environ["TDMPC_DSSM_LEARNER_HIP"] = "1" if hip else "0"
    try:
        ln = DssmSimLearner(agent, graph=graph, warmup=3)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r10", "drnn_sim_update_bench.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("drnn_sim_update_bench needs a GPU: nothing is measured without one")
    from tdmpc_amd.dssm_train import CHAIN_MODE, DssmTrainStep
    cfg = bench_cfg()
    H, W, B, L, A, Hd = cfg.horizon, cfg.warmup_len, cfg.batch_size, cfg.latent_dim, cfg.action_dim, cfg.hidden_dim
    S = H + 1
    out = {"tool": "tools/drnn_sim_update_bench.py", "shape": f"humanoid L{L} A{A} Hd{Hd} M{cfg.mlp_dim} B{B} H{H} W{W}",
           "device": torch.cuda.get_device_name(0), "calls_per_batch": args.calls, "batches": args.reps,
           "default_chain_mode": CHAIN_MODE}

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

    def mode0():
        return step.intrinsic_chain_loss(z, a, keys, S, W, mode=0)

    def mode1():
        return step.intrinsic_chain_loss(z, a, keys, S, W, mode=1)

    @torch.no_grad()
    def separate():
        h, out_ = h0, [torch.zeros(W * B, device="cuda")]
        for s in range(S):
            rows = slice(s * B, (s + 1) * B)
            zo, h, _ = step.next(z[rows], a[rows], h)
            if s >= W:
                out_.append(step.similarity_loss(zo, keys[rows]))
        return torch.cat(out_)
    got = {}
    for name, fn in (("mode0", mode0), ("mode1", mode1), ("separate", separate)):
        restore()
        got[name] = fn().clone()
    torch.cuda.synchronize()
    res = alternate({"mode0": mode0, "mode1": mode1, "separate": separate}, args.reps, args.calls)
    out["intrinsic"] = {"segments": S, "warm": W, "rows_per_segment": B,
                        "mode0_bitwise_equal_separate": bool(torch.equal(got["mode0"], got["separate"])),
                        "mode1_max_abs_diff_mode0": float((got["mode1"] - got["mode0"]).abs().max()),
                        "launches": {"mode0": 1 + (1 + 2 * (S - 1)) + 1 + 3 + 1 + 6, "mode1": 1 + 1 + 1 + 3 + 1 + 6,
                                     "separate": S * 7 + (S - W) * 5},
                        **res,
                        "mode0_over_mode1": round(res["mode0"]["us_median"] / res["mode1"]["us_median"], 3),
                        "separate_over_mode0": round(res["separate"]["us_median"] / res["mode0"]["us_median"], 3),
                        "separate_over_mode1": round(res["separate"]["us_median"] / res["mode1"]["us_median"], 3)}
    print(json.dumps({"intrinsic": out["intrinsic"]}), flush=True)

    # ---- the whole update
    sides, learners = {}, {}
    for name, hip, graph in (("hip_graph", True, True), ("hip_eager", True, False), ("torch_graph", False, True),
                             ("torch_eager", False, False)):
        learners[name], sides[name] = learner(cfg, hip, graph)
    out["update_chain_mode"] = learners["hip_graph"].train_step.chain_mode
    res = alternate(sides, args.reps, args.calls)
    for name in ("hip_graph", "torch_graph"):
        assert learners[name]._graphs, f"{name}: never replayed a captured graph"
    out["update"] = {**res,
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
