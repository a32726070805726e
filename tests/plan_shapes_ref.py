"""Shared by tests/test_gpu_plan_shapes.py and tests/test_plan_shapes_cpu.py: the TOLD planner at latent, action and
encoder widths no task has, at the stock mlp_dim 512. CPU only (the oracle, oracle/tdmpc_ref.py).

Twelve shapes, a to l: (task whose observations are used, action_dim, latent_dim, enc_dim). An action width no task
has (c, j) is set on the cfg namespace after make_cfg; the oracle, synthetic_state_dict and TDMPC read it from there.
What each row is there for is in tests/test_gpu_plan_shapes.py's docstring.

Inputs, seeds and the near-tie vetting are tests/plan_widths_ref.py's: every env of a batch draws its observations and
noise from a seed of its own, and a committed seed leaves, for both call patterns an env slot can see, a gap of more
than 2 (1e-5 + 1e-4 max |v|) at the elite cut-off of every CEM iteration of the oracle's own trace (SEEDS was filled
with find_seeds, which asks for 1.5 times that)."""
import functools

import torch

import plan_widths_ref as W
from oracle import tdmpc_ref
from plan_widths_ref import PATTERNS, SIZE, WSEED, env_inputs   # noqa: F401  (the tests' names)
from tdmpc_amd.config import make_cfg
from tdmpc_amd.told import synthetic_state_dict

# letter -> (task, action_dim, latent_dim, enc_dim)
SHAPES = {
    "a": ("cartpole", 1, 8, 64),
    "b": ("cheetah", 6, 90, 96),
    "c": ("cheetah", 64, 128, 256),
    "d": ("humanoid", 21, 129, 256),
    "e": ("dog", 38, 200, 256),
    "f": ("dog", 38, 256, 256),
    "g": ("humanoid", 21, 300, 256),
    "h": ("cheetah", 6, 440, 256),
    "i": ("humanoid", 21, 509, 256),
    "j": ("cheetah", 72, 50, 256),
    "k": ("humanoid", 21, 520, 256),
    "l": ("humanoid", 21, 1000, 1000),
}
# the per-env seeds, in slot order; batches of 1 and 3 take the first ones, 32 envs at b and d only
SEEDS = {
    "a": [12, 19, 20],
    "b": [0, 1, 3, 4, 7, 9, 12, 14, 15, 18, 19, 21, 23, 27, 28, 30, 31, 33, 35, 38, 39, 42, 44, 45, 46, 48, 49, 51, 53,
          54, 56, 59],
    "c": [1, 3, 4],
    "d": [0, 4, 5, 7, 8, 10, 11, 12, 17, 18, 19, 20, 21, 22, 25, 28, 30, 31, 32, 33, 35, 37, 38, 39, 40, 41, 42, 44, 45,
          46, 48, 49],
    "e": [0, 1, 2],
    "f": [0, 1, 2],
    "g": [0, 1, 3],
    "h": [4, 5, 7],
    "i": [0, 1, 3],
    "j": [0, 1, 5],
    "k": [0, 1, 4],
    "l": [0, 1, 2],
}
BATCHES = {s: ([1, 3, 32] if s in "bd" else [1, 3]) for s in SHAPES}


def shape_cfg(shape):
    task, A, L, E = SHAPES[shape]
    cfg = make_cfg(task, latent_dim=L, enc_dim=E, **SIZE)
    assert cfg.mlp_dim == 512
    cfg.action_dim = A
    return cfg


def derived(shape):
    """The padded widths the kernels switch on (make_layout, csrc/tdmpc_kernels.hip)."""
    _, A, L, _ = SHAPES[shape]
    rup = lambda x, m: -(-x // m) * m
    d = dict(A=A, L=L, Ap=rup(A, 8), Lp=rup(L, 8), Ar=rup(A, 32), Lr=rup(L, 32))
    d["Kx"] = d["Ap"] + d["Lp"]
    return d


@functools.lru_cache(maxsize=None)
def told_of(shape, wseed=WSEED):
    cfg = shape_cfg(shape)
    return tdmpc_ref.RefTOLD(synthetic_state_dict(cfg, wseed), cfg)


def min_gap_ratio(shape, seed, pattern):
    return W.gap_ratio(shape_cfg(shape), told_of(shape), seed, pattern)


find_seeds = functools.partial(W.find_seeds, ratio=min_gap_ratio)


def oracle_fp32_share(shape, wseed=7):
    """How much of parity_util.close's bound (1e-5 + 1e-4 |ref|) the fp32 oracle's own rounding uses at this shape:
    max over the rows of |G_fp32 - G_fp64| / (1e-5 + 1e-4 |G_fp64|), on the inputs and weights of
    test_gpu_plan._estimate_value_matches_oracle (weight seed 7, generator seed 3, T = 192 rows, horizon 3)."""
    cfg = shape_cfg(shape)
    T, H, A, L = cfg.num_samples + int(cfg.mixture_coef * cfg.num_samples), cfg.horizon, cfg.action_dim, cfg.latent_dim
    g = torch.Generator().manual_seed(3)
    z0 = torch.randn(1, L, generator=g)
    actions = torch.rand(1, H, T, A, generator=g) * 2 - 1
    eps = torch.randn(1, T, A, generator=g)
    told = told_of(shape, wseed)
    told64 = tdmpc_ref.RefTOLD(synthetic_state_dict(cfg, wseed), cfg)
    told64.sd = {k: t.double() for k, t in told64.sd.items()}
    G32 = tdmpc_ref.estimate_value(told, cfg, z0.repeat(T, 1), actions[0], H, eps[0])[0][:, 0].double()
    G64 = tdmpc_ref.estimate_value(told64, cfg, z0.double().repeat(T, 1), actions[0].double(), H, eps[0].double())[0][:, 0]
    return float(((G32 - G64).abs() / (1e-5 + 1e-4 * G64.abs())).max())
