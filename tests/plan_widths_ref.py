"""Shared by tests/test_gpu_plan_widths.py and tests/test_plan_widths_cpu.py: the planner's cases at hidden widths 256,
384 and 1024, and their inputs. CPU only (the oracle, oracle/tdmpc_ref.py).

Every env of a batch gets its observations and its noise from a seed of its own, and the committed seeds are those
for which the oracle's own trace has, at every CEM iteration of every call, a gap larger than
2 (1e-5 + 1e-4 max |v|) between its num_elites-th and its next-best value. Two value vectors that are each within the
parity contract's `close` (1e-5 + 1e-4 |ref|) of the oracle's can then not disagree on the elite set, so none of
these comparisons can escape on a near tie (tests/test_zz_parity_budget.py). A seed is vetted for both call patterns
an env slot can see: cold, warm, cold (even slots of the mixed call restart) and cold, warm, warm."""
import functools

import numpy as np
import torch

from oracle import tdmpc_ref
from tdmpc_amd.config import make_cfg
from tdmpc_amd.told import synthetic_state_dict

SIZE = dict(num_samples=128, num_elites=16, iterations=3, horizon=3)
WSEED = 21
STEP = 10 ** 6
# (task, mlp_dim): the per-env seeds, in slot order; batches of 1 and 3 take the first ones, 32 once per width
SEEDS = {
    ("cheetah", 256): [0, 2, 6, 8, 9, 11, 12, 14, 15, 16, 17, 18, 20, 21, 23, 24, 25, 28, 30, 31, 32, 34, 35, 38, 39, 40,
                       41, 42, 43, 44, 47, 48],
    ("cartpole", 256): [0, 9, 35],
    ("cheetah", 1024): [0, 3, 5, 6, 7, 10, 12, 13, 14, 15, 16, 17, 19, 20, 22, 28, 29, 30, 31, 34, 35, 36, 37, 38, 41,
                        43, 45, 46, 47, 48, 49, 51],
    ("cartpole", 1024): [2, 5, 26],
    ("humanoid", 1024): [0, 1, 2],
    ("cheetah", 384): [1, 4, 6, 7, 9, 10, 11, 12, 13, 15, 16, 17, 20, 22, 23, 24, 28, 29, 33, 38, 40, 42, 43, 44, 45, 47,
                       49, 50, 51, 52, 53, 54],
}
SHAPES = list(SEEDS)
BATCHES = {shape: ([1, 3, 32] if len(s) >= 32 else [1, 3]) for shape, s in SEEDS.items()}
PATTERNS = ((True, False, True), (True, False, False))


def shape_cfg(shape):
    task, mlp = shape
    return make_cfg(task, mlp_dim=mlp, **SIZE)


@functools.lru_cache(maxsize=None)
def told_of(shape):
    cfg = shape_cfg(shape)
    return tdmpc_ref.RefTOLD(synthetic_state_dict(cfg, WSEED), cfg)


def env_inputs(cfg, seed, ncalls=3):
    """[(obs, NoiseBundle)] of one env's calls, from its own seed."""
    rs = np.random.RandomState(seed)
    torch.manual_seed(seed)
    np.random.seed(seed)
    return [(rs.standard_normal(tuple(cfg.obs_shape)).astype(np.float32), tdmpc_ref.draw_noise(cfg, STEP, False))
            for _ in range(ncalls)]


def calls_of(B):
    """The t0 pattern of each call: cold, warm and (B > 1) mixed, as test_gpu_configs._plan_calls_match_oracle."""
    calls = [[True] * B, [False] * B]
    if B > 1:
        calls.append([e % 2 == 0 for e in range(B)])
    return calls


def gap_ratio(cfg, told, seed, pattern):
    """The oracle's trace of one env over the calls of `pattern` (its t0 flags): the smallest ratio, over every
    iteration of every call, of (K-th best value - next best) to 2 (1e-5 + 1e-4 max |v|). Above 1: no near tie."""
    state, worst = tdmpc_ref.PlanState(0.05), np.inf
    for (obs, nb), t0 in zip(env_inputs(cfg, seed), pattern):
        tr = {}
        tdmpc_ref.plan(told, cfg, state, obs, nb, eval_mode=False, step=STEP, t0=t0, trace=tr)
        for v in tr["value"]:
            v = np.sort(v.squeeze(-1).double().numpy())[::-1]
            K = cfg.num_elites
            worst = min(worst, (v[K - 1] - v[K]) / (2 * (1e-5 + 1e-4 * np.abs(v).max())))
    return worst


def min_gap_ratio(shape, seed, pattern):
    return gap_ratio(shape_cfg(shape), told_of(shape), seed, pattern)


def find_seeds(shape, n, start=0, ratio=min_gap_ratio):
    """The first n seeds from `start` on that pass both patterns (how SEEDS was filled); ratio: the shape family's
    min_gap_ratio (tests/plan_shapes_ref.py passes its own)."""
    out, s = [], start
    while len(out) < n:
        if all(ratio(shape, s, p) > 1.5 for p in PATTERNS):   # (a margin over the test's 1.0)
            out.append(s)
        s += 1
    return out
