"""Time of the DSSM learner kernels on one MI355X against PyTorch-ROCm autograd over the eager `tdmpc_amd.dssm` modules
on the same GPU.

    python tools/drnn_train_bench.py [--out profiles/r08/drnn_train_bench.json] [--reps 9] [--calls 50]   (--out '' writes no file)

Two legs at the humanoid shape (L 100, A 21, Hd 128, mlp_dim 512), weights synthetic_dssm_state_dict seed 0:
  next:  one `next` forward + backward (all three upstream gradients, gradients of z, a, h and the 20 parameter
         tensors) at R = 512, the learner's batch size;
  loss:  one `similarity_loss` forward + backward (gradients of the queries and the 6 parameter tensors) at R = 2560,
         five steps' predictions.
Each leg runs `DssmTrainStep` (csrc/drnn_learner.hip) and the eager modules in train() mode, both eagerly launched
(no graph), through `torch.autograd.grad`. Per leg and side: a warm-up, then `reps` timed batches of `calls`
forward + backward passes between HIP events, the two sides alternating batch by batch; the median is the figure,
min / max the spread. The two sides' outputs and gradients are compared on the timed inputs before timing (max
|ours - eager| / max |eager| per tensor). No GPU: it fails.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from tdmpc_amd.config import make_cfg  # noqa: E402


def bench_cfg():
    return make_cfg("humanoid", hidden_dim=128, norm_cell=True, plan2expl=False, warmup_len=0)


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3   # us per pass


def summary(us):
    med = statistics.median(us)
    return {"us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
            "spread_frac": round((max(us) - min(us)) / med, 4), "batches": len(us)}


def alternate(ours, eager, reps, calls, warm=10):
    for _ in range(warm):
        ours()
        eager()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):
        a.append(timed(ours, calls))
        b.append(timed(eager, calls))
    return summary(a), summary(b)


def worst_figure(got, want, skip):
    """max over the tensors of max |ours - eager| / max |eager|, without tensor `skip`: the bias in front of the
    train-mode BatchNorm, whose gradient is zero in exact arithmetic and rounding noise on both sides."""
    return max(float((g - w).abs().max() / w.abs().max().clamp_min(1e-30))
               for i, (g, w) in enumerate(zip(got, want)) if i != skip)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "r08", "drnn_train_bench.json"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--next-rows", type=int, default=512)
    ap.add_argument("--loss-rows", type=int, default=2560)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("drnn_train_bench needs a GPU: nothing is measured without one")
    from tdmpc_amd.dssm import DSSM, synthetic_dssm_state_dict
    from tdmpc_amd.dssm_train import LOSS_PARAMS, NEXT_PARAMS, DssmTrainStep
    cfg = bench_cfg()
    model = DSSM(cfg, init="none")
    model.load_state_dict(synthetic_dssm_state_dict(cfg, 0))
    model = model.cuda().train()
    step = DssmTrainStep(model, max_rows=args.next_rows, max_loss_rows=args.loss_rows)
    named = dict(model.named_parameters())
    pn, pl = [named[k] for k in NEXT_PARAMS], [named[k] for k in LOSS_PARAMS]
    rs = np.random.RandomState(0)
    f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).cuda()
    R, Rl, L, A, Hd = args.next_rows, args.loss_rows, cfg.latent_dim, cfg.action_dim, cfg.hidden_dim
    z, a, h = f(R, L).requires_grad_(True), f(R, A).clamp(-1, 1).requires_grad_(True), f(R, Hd).tanh().requires_grad_(True)
    up = (f(R, L), f(R, Hd), f(R, 1))
    q, k, dl = f(Rl, L).requires_grad_(True), f(Rl, L), f(Rl)

    def next_pass(fn):
        outs = fn(z, a, h)
        total = sum((o * u).sum() for o, u in zip(outs, up))
        return list(outs) + list(torch.autograd.grad(total, [z, a, h] + pn))

    def eager_loss(qq, kk):
        qn = F.normalize(model._predictor(qq), dim=-1, p=2)
        return 2.0 - 2.0 * (qn * F.normalize(kk, dim=-1, p=2)).sum(dim=-1)

    def loss_pass(fn):
        loss = fn(q, k)
        return [loss] + list(torch.autograd.grad((loss * dl).sum(), [q] + pl))

    out = {"shape": f"humanoid L{L} A{A} Hd{Hd} M{cfg.mlp_dim}", "device": torch.cuda.get_device_name(0),
           "calls_per_batch": args.calls}
    # (skip: the position of prior_mlp.0.bias / _predictor.0.bias in a pass's list)
    for name, rows, ours, eager, skip in (
            ("next", R, lambda: next_pass(step.next), lambda: next_pass(model.next), 3 + 3 + 1),
            ("similarity_loss", Rl, lambda: loss_pass(step.similarity_loss), lambda: loss_pass(eager_loss), 1 + 1 + 1)):
        fig = worst_figure(ours(), eager(), skip)
        o, e = alternate(ours, eager, args.reps, args.calls)
        out[name] = {"rows": rows, "hip_fwd_bwd": o, "eager_autograd_fwd_bwd": e,
                     "eager_over_hip": round(e["us_median"] / o["us_median"], 3),
                     "worst_figure_hip_vs_eager": fig}
        print(json.dumps({name: out[name]}), flush=True)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
