"""Shared by tests/test_gpu_learner_widths.py, tests/test_learner.py and tests/test_learner_widths_cpu.py: the state
learner's update at every admitted hidden width against the float64 oracle (oracle/learner_ref.py::RefLearner with
dtype=float64 and explicit TruncatedNormal draws). Cases, the oracle runs, the figures per class, and the float32 CPU
floors the GPU bounds are derived from. Nothing here touches the GPU."""
import functools

import numpy as np
import torch

from learner_io import METRICS, batch
from oracle.learner_ref import RefLearner
from tdmpc_amd.config import make_cfg
from tdmpc_amd.told import synthetic_state_dict

PLAN = dict(num_samples=64, num_elites=32, iterations=3)
# name: (task, mlp_dim, batch, horizon, grad_clip_norm, model seed, target seed, batch seed, noise seed)
CASES = {
    "w256-ragged": ("cartpole", 256, 52, 5, 10, 21, 22, 5, 0),    # one-wide action; H B = 260 is no multiple of 4
    "w256-split": ("cheetah", 256, 256, 4, 10, 21, 22, 5, 0),     # R = 1024: the split-K (sp = 4) weight gradients
    "w512-ragged": ("cheetah", 512, 52, 5, 10, 21, 22, 5, 0),     # the stock width at a ragged batch
    "w1024-ragged": ("cheetah", 1024, 52, 3, 10, 21, 22, 5, 0),
    "w1024-split": ("cheetah", 1024, 256, 4, 10, 21, 22, 5, 0),   # R1 = 1280 > 1024: lg_rows_bwd<16, 4> strides twice
    "w512-clipped": ("cheetah", 512, 52, 5, 0.5, 21, 22, 5, 0),   # the clip coefficient is below 1
    "w384-autograd": ("cheetah", 384, 52, 3, 10, 21, 22, 5, 0),   # off the engine's widths: the autograd learner
    # the existing tests' cases (tests/test_learner.py), whose first update's gradients are compared too
    "golden-cartpole": ("cartpole", 512, 64, 5, 10, 21, 22, 5, 0),
    "full-humanoid": ("humanoid", 512, 512, 5, 10, 31, 32, 9, 1),
    "full-dog": ("dog", 512, 512, 5, 10, 31, 32, 9, 1),
    "full-cheetah": ("cheetah", 512, 512, 5, 10, 31, 32, 9, 1),
}
WIDTH_CASES = [k for k in CASES if k.startswith("w")]
GRAD_ONLY_CASES = [k for k in CASES if not k.startswith("w")]
CLASSES = ("metrics", "prio", "grad")


def case_cfg(name):
    task, mlp, B, H, clip = CASES[name][:5]
    return make_cfg(task, horizon=H, batch_size=B, mlp_dim=mlp, grad_clip_norm=clip, **PLAN)


def case_inputs(name, updates=2):
    """-> cfg, model / target state dicts, the batch, and per update the 2H + 1 draws [B, A] in the oracle's order."""
    cfg = case_cfg(name)
    sm, st, sb, sn = CASES[name][5:]
    g = torch.Generator().manual_seed(sn)   # (the global generator's stream from this seed, without touching it)
    noise = [[torch.empty(cfg.batch_size, cfg.action_dim).normal_(generator=g) for _ in range(2 * cfg.horizon + 1)]
             for _ in range(updates)]
    return cfg, synthetic_state_dict(cfg, sm), synthetic_state_dict(cfg, st), batch(cfg, seed=sb), noise


def snapshot(metrics, prio, named_grads, sd, sdt):
    """One update's observable state, detached on the CPU."""
    f = lambda d: {k: v.detach().cpu().clone() for k, v in d.items()}   # noqa: E731
    return {"metrics": np.array([float(metrics[n]) for n in METRICS], dtype=np.float64),
            "prio": prio.detach().cpu().clone(), "grad": f(named_grads), "params": f(sd), "target": f(sdt)}


def run_oracle(name, dtype, updates=2):
    cfg, sd, sdt, b, noise = case_inputs(name, updates)
    ref = RefLearner(cfg, sd, sdt, dtype=dtype)
    out = []
    for k in range(updates):
        m, prio = ref.update(b, k + 1, noise=noise[k])
        p, pt = ref.state_dicts()
        out.append(snapshot(m, prio, {n: v.grad for n, v in ref.p.items()}, p, pt))
    return out


@functools.lru_cache(maxsize=None)
def oracle64(name, updates=2):
    return run_oracle(name, torch.float64, updates)


def tensor_fig(got, ref):
    got, ref = got.double(), ref.double()
    top = float(ref.abs().max())
    if top == 0.0:
        return 0.0 if float(got.abs().max()) == 0.0 else float("inf")
    return float((got - ref).abs().max()) / top


def figures(got, ref):
    """{class: figure} of one update's snapshot against the float64 one: the seven metrics' largest relative error,
    the priorities' and every gradient's max |got - f64| / max |f64| (the largest over the tensors, with its name)."""
    assert list(got["grad"]) == list(ref["grad"])
    g = {k: tensor_fig(got["grad"][k], ref["grad"][k]) for k in ref["grad"]}
    worst = max(g, key=g.get)
    return {"metrics": float((np.abs(got["metrics"] - ref["metrics"]) / np.abs(ref["metrics"])).max()),
            "prio": tensor_fig(got["prio"], ref["prio"]), "grad": g[worst]}, worst


def tight_share(got, ref):
    """The smallest per-tensor share of elements with |got - f64| <= 1e-6 + 1e-4 |f64|, over parameters and target."""
    s = 1.0
    for which in ("params", "target"):
        for k, w in ref[which].items():
            d = (got[which][k].double() - w.double()).abs()
            s = min(s, float((d <= 1e-6 + 1e-4 * w.double().abs()).double().mean()))
    return s


def params_close(got, ref, lr, share):
    """_params_close's structure (tests/test_learner.py) against float64: <= 2 lr + 1e-6 everywhere, and at least
    `share` of every tensor's elements inside 1e-6 + 1e-4 |f64|."""
    for which in ("params", "target"):
        for k, w in ref[which].items():
            w = w.double()
            d = (got[which][k].double() - w).abs()
            assert (d <= 2 * lr + 1e-6).all(), (which, k, float(d.max()))
            frac = float((d <= 1e-6 + 1e-4 * w.abs()).double().mean())
            assert frac >= share, (which, k, frac)


def measure_floors(threads=(1, 2, 4, 8), cases=None):
    """-> {case: {class + update number ("grad1", "metrics2", ...): the largest figure of float32 RefLearner against
    float64 over the thread counts}}, {case: the smallest tight share}. The second update has a class of its own: it
    starts from parameters that already differ by Adam's first step on the elements whose gradient is ~0, so its floor
    is far above the first's. The existing tests' cases run one update (their gradient only)."""
    floors, shares = {}, {}
    keep = torch.get_num_threads()
    try:
        for name in cases or CASES:
            n = 2 if name in WIDTH_CASES else 1
            ref = oracle64(name, n)
            fl, sh = {f"{c}{k + 1}": 0.0 for c in CLASSES for k in range(n)}, 1.0
            for t in threads:
                torch.set_num_threads(t)
                got = run_oracle(name, torch.float32, n)
                for k, (a, b) in enumerate(zip(got, ref)):
                    f, _ = figures(a, b)
                    for c in CLASSES:
                        fl[f"{c}{k + 1}"] = max(fl[f"{c}{k + 1}"], f[c])
                    sh = min(sh, tight_share(a, b))
            floors[name], shares[name] = fl, sh
    finally:
        torch.set_num_threads(keep)
    return floors, shares
