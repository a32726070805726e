"""GPU: the planner at hidden widths 256, 384 and 1024 (every other test plans at 512).

Shapes: cheetah (latent 50, 6 actions) and cartpole (1 action) at mlp_dim 256 and 1024, humanoid (latent 100, 21
actions) at 1024, cheetah at 384 (no multiple of 256: the layered kernels only). 128 samples, 16 elites, 3 iterations,
horizon 3; 1 and 3 envs per call, and 32 once per width, where the auto path's row-count thresholds are crossed.

* estimate_value on every path against the oracle (test_gpu_plan.py's comparison).
* Whole plans (cold, warm, mixed t0) on auto / layered / chain / chain16 / chain32 / chain_x6 against the oracle with
  test_gpu_configs._plan_calls_match_oracle: values 1e-5 + 1e-4 |ref|, action / mean / std / metrics 2e-5. The seeds
  (tests/plan_widths_ref.py) leave no near tie in the oracle's trace (tests/test_plan_widths_cpu.py), so every
  comparison must run to the end: compare_iterations returns True for every call.
* The kernels that ran, by name, per (width, path, envs): KERNELS below, read from use_chain / chain_rb / use_x6 /
  chain_shape_ok / chain16_shape_ok / pick_cfg (csrc/tdmpc_kernels.hip) and asserted with the library's profiler. A
  chain launch is named by tdmpc_profile_kernel; the layered linear kernels carry no name there, so a layered step
  is pinned as: no chain / wide launch of that head, and launches of the hidden mlp_dim x mlp_dim layer on the tile
  configuration pick_cfg gives (1: 32 x 32 latency tile, 2: 32 x 64, 3: LDS throughput tile).
"""
import ctypes as C

import numpy as np
import pytest

import plan_widths_ref as P
from test_gpu_configs import _agent, _plan_calls_match_oracle
from test_gpu_plan import PATHS, _estimate_value_matches_oracle
from tdmpc_amd import _lib

pytestmark = pytest.mark.gpu

PLAN_PATHS = ["auto", "layered", "chain", "chain16", "chain32", "chain_x6"]
IDS = dict(ids=lambda s: f"{s[0]}-{s[1]}" if isinstance(s, tuple) else str(s))


def _profile(agent, obs, prof_cfg, kdim=0):
    """(launch count, kernel name) the library's profiler saw for prof_cfg over one eager warm plan of the batch."""
    L = _lib.lib()
    graph, agent.graph = agent.graph, False
    try:
        _lib.check(L.tdmpc_profile_begin(prof_cfg, -1, kdim, 0, 256), "profile_begin")
        agent.plan_batch(obs, step=P.STEP, t0=False, sync_metrics=False)
        n = C.c_int32()
        _lib.check(L.tdmpc_profile_end(C.byref(n), None, None), "profile_end")
    finally:
        agent.graph = graph
    return n.value, (L.tdmpc_profile_kernel().decode() if n.value else None)


def observed(agent, cfg, B):
    """(step kernel, Q kernel) of one plan: a chain kernel's name, or "linear<id, ..>" with the tile configurations the
    hidden mlp_dim x mlp_dim layers ran on where no chain launch of that head was seen."""
    obs = np.random.RandomState(1).standard_normal((B,) + tuple(cfg.obs_shape)).astype(np.float32)
    step, q = _profile(agent, obs, 4)[1], _profile(agent, obs, 6)[1]
    if step is None or q is None:
        ids = [i for i in (1, 2, 3) if _profile(agent, obs, i, kdim=cfg.mlp_dim)[0] > 0]
        lin = "linear<" + ", ".join(map(str, ids)) + ">"
        step, q = step or lin, q or lin
    return step, q


# (mlp_dim, path, envs) -> (step kernel, Q kernel), the same for every task above. With 64 policy rows beside the 128
# sampled ones a head launch has 192 rows per env: the auto path takes the chain kernels from 64 32-row blocks x
# heads for the step (32 for Q: chain_wgs_kind), so at 3 envs (576 rows, 18 blocks x 2 heads) only Q runs there, and
# chain_rb gives 16-row blocks up to half the CUs' worth of 32-row blocks where chain16_shape_ok (256 and 512 only).
_S16, _Q16 = "chain16_kernel<CH_STEP, f32>", "chain16_kernel<CH_Q, f32>"     # chain16_kernel<.., NT = 2> at 256
_S32, _Q32 = "chain_kernel<CH_STEP, f32>", "chain_kernel<CH_Q, f32>"         # chain_kernel<.., TN = 1 | 4> at 256 | 1024
_L12, _L23 = "linear<1, 2>", "linear<2, 3>"   # pick_cfg: < 512 rows latency tiles (2: the LayerNorm layers' 64-column
#                                               blocks); 2048 policy rows 32 x 64, >= 4096 rows the LDS tile
KERNELS = {
    (256, "auto", 1): (_L12, _L12), (256, "auto", 3): (_L12, _Q16), (256, "auto", 32): (_S32, _Q32),
    (256, "layered", 1): (_L12, _L12), (256, "layered", 3): (_L12, _L12), (256, "layered", 32): (_L23, _L23),
    (256, "chain", 1): (_S16, _Q16), (256, "chain", 3): (_S16, _Q16), (256, "chain", 32): (_S32, _Q32),
    (256, "chain16", 1): (_S16, _Q16), (256, "chain16", 3): (_S16, _Q16), (256, "chain16", 32): (_S16, _Q16),
    (256, "chain32", 1): (_S32, _Q32), (256, "chain32", 3): (_S32, _Q32), (256, "chain32", 32): (_S32, _Q32),
    # chain_x6: the x6 products are instantiated at 512 only (use_x6 returns 0 elsewhere): the f32 MFMA chain kernel
    (256, "chain_x6", 1): (_S32, _Q32), (256, "chain_x6", 3): (_S32, _Q32), (256, "chain_x6", 32): (_S32, _Q32),
    (1024, "auto", 1): (_L12, _L12), (1024, "auto", 3): (_L12, _Q32), (1024, "auto", 32): (_S32, _Q32),
    (1024, "layered", 1): (_L12, _L12), (1024, "layered", 3): (_L12, _L12), (1024, "layered", 32): (_L23, _L23),
    # chain16: chain16_shape_ok admits 256 and 512 only, so chain_rb gives 32-row blocks: chain_kernel, as documented
    # there -- never chain16_kernel at 1024
    **{(1024, p, B): (_S32, _Q32) for p in ("chain", "chain16", "chain32", "chain_x6") for B in (1, 3, 32)},
    # 384 is no multiple of 256: chain_shape_ok is false and every path runs the layered kernels
    **{(384, p, B): ((_L23, _L23) if B == 32 else (_L12, _L12)) for p in PLAN_PATHS for B in (1, 3, 32)},
}


@pytest.mark.parametrize("shape", P.SHAPES, **IDS)
def test_estimate_value_at_other_widths(shape):
    """Every path (and auto) at T = 192 rows, horizon 3: z_H, the last reward and the values against the oracle."""
    cfg = P.shape_cfg(shape)
    for path in PATHS + ["auto"]:
        _estimate_value_matches_oracle(cfg, _agent(cfg, 7, path=path), cfg.horizon)


def _inputs(cfg, shape, B):
    per_env = [P.env_inputs(cfg, s) for s in P.SEEDS[shape][:B]]
    return lambda ci: (np.stack([e[ci][0] for e in per_env]), [e[ci][1] for e in per_env])


_ORACLE = {}     # (shape, B) -> the oracle's plans, shared by the paths


@pytest.mark.parametrize("path", PLAN_PATHS)
@pytest.mark.parametrize("shape,B", [(s, B) for s in P.SHAPES for B in P.BATCHES[s]], **IDS)
def test_plan_at_other_widths(shape, B, path):
    """Cold, warm and mixed-t0 plans against the oracle, no near-tie escape, and the kernels that ran, by name.
    Every chain instance is reached here: chain_kernel TN = 1 (256) and TN = 4 (1024), chain16_kernel NT = 2 (256)."""
    cfg = P.shape_cfg(shape)
    agent = _agent(cfg, P.WSEED, B=B, path=path)
    name = f"{shape[0]}-m{shape[1]}-{path}"
    sames = _plan_calls_match_oracle(name, cfg, agent, B, inputs=_inputs(cfg, shape, B),
                                     ref_cache=_ORACLE.setdefault((shape, B), {}))
    assert len(sames) == B * (3 if B > 1 else 2) and all(sames), (name, B, sames)   # no near-tie escape
    got = observed(agent, cfg, B)
    assert got == KERNELS[(shape[1], path, B)], (name, B, got)
    if shape[1] == 384:
        assert got[0].startswith("linear") and got[1].startswith("linear"), got
    assert not (shape[1] == 1024 and "chain16_kernel" in "".join(got)), got
