"""GPU: the TOLD planner at latent, action and encoder widths no task has, at the stock mlp_dim 512.

check_dims / make_layout (csrc/tdmpc_kernels.hip) admit any latent_dim and enc_dim up to 1024, any action_dim up to
256 and any Kx = Ap + Lp up to 1024; every other plan test at mlp_dim 512 runs latent 50 / 100 / 512, 1 / 6 / 12 / 21 /
38 actions and enc_dim 256, and the kernels branch on exactly these numbers. The shapes (tests/plan_shapes_ref.py), with
Ap = rup(A, 8), Lp = rup(L, 8), Ar = rup(A, 32), Lr = rup(L, 32), nb3 = Lr / 32 the dynamics head's last-layer column
blocks, NW = 8 waves (4 in the default x6 form):

     obs / A        L     enc   derived                  what it is there for
  a  cartpole / 1   8     64    Lr 32, Kx 16             nb3 = 1: every wave a K part of the one block (ks 8 / 4); chain16
                                                         2 tiles, ks 4; plan1 with Lr / 16 = 2 and a first layer that is
                                                         almost all padding; z0c not eligible (rup(Ap, 16) = rup(Kx, 16))
  b  cheetah / 6    90    96    Lp = Lr = 96, Kx 104     nb3 = 3: idle waves (f32 6 items on 8 waves, x6 3 on 4); chain16 and
                                                         plan1 6 tiles; 6 pad columns; Kx % 16 = 8; encoder
                                                         np = 1024 / 96 = 10
  c  cheetah / 64   128   256   Ap = Ar = 64, Lr 128,    the pi noise prefetch at its limit (Ap / 4 * 32 = 512 quads); plan1
                                Kx 192                   at all its limits at once (12 k-groups, KS 6, Lr 128); no padding
  d  humanoid / 21  129   256   Lp 136, Lr 160, Kx 160   nb3 = 5; the x6 form's second pass with one wave; chain16 10 tiles;
                                                         plan1 refused (Lr > 128): one env takes the launches; 7 pad columns
  e  dog / 38       200   256   Lr 224, Kx 240           nb3 = 7: x6 second pass 3 of 4 waves; auto's split still admitted
  f  dog / 38       256   256   Lr 256, Kx 296           nb3 = 8 = NW (f32), two full passes (x6); auto's split refused for
                                                         the step (rup(Kx, 16) > 256), still admitted for pi (Lp = 256)
  g  humanoid / 21  300   256   Lp 304, Lr 320, Kx 328   nb3 = 10: f32 second pass 2 waves, x6 third pass 2 waves
  h  cheetah / 6    440   256   Lr 448, Kx 448           nb3 = 14: x6 fourth pass 2 of 4 waves; chain16 28 tiles
  i  humanoid / 21  509   256   Lp = Lr = 512, Kx 536    the fold layout (Lp == Lr == mlp_dim) over 3 pad columns; the wide
                                                         step kernel's instance (17, 32): path wide runs it, folded
  j  cheetah / 72   50    256   Ap 72, Ar 96, Kx 128     chain_shape_ok false (Ap > 64): no chain kernel on any path; plan1
                                                         still eligible, with 6 policy tiles
  k  humanoid / 21  520   256   Lr 544, Kx 544           17 last-layer blocks: chain and chain16 refused, no wide instance
  l  humanoid / 21  1000  1000  Lr 1024, Kx 1024         check_dims' and launch_lin's K limit (8 chunks of 128); the split
                                                         kernel's LDS refuses; encoder np = 1 at a width that is no power
                                                         of two

(No row had to be moved: every purpose stated above was checked against the predicates, and plan1 is resident at c --
its LDS is 151 KB of 160 at 64 actions, horizon 3, 16 elites.)

128 samples + 64 policy rows (T = 192 rows per env), 16 elites, 3 iterations, horizon 3, as tests/test_gpu_plan_widths.py.

* estimate_value on every path of test_gpu_plan.PATHS and auto against the oracle (test_gpu_plan's comparison).
* Whole plans (cold, warm, mixed t0) at 1 and 3 envs (32 at b and d) against the oracle with
  test_gpu_configs._plan_calls_match_oracle: values 1e-5 + 1e-4 |ref|, action / mean / std / metrics 2e-5. The seeds
  leave no near tie in the oracle's trace (tests/test_plan_shapes_cpu.py), so every comparison runs to the end.
* The kernels that ran, by name: KERNELS below, written from the predicates (use_plan1 / p1_dims_ok, use_wide /
  wide_instance, use_chain / chain_shape_ok, chain_rb / chain16_shape_ok, use_x6, use_split / use_split_pi, pick_cfg) and
  asserted with the library's profiler as test_gpu_plan_widths.observed does; the persistent plan is named by profiler
  cfg 8. split_step_kernel carries no profiler name: a split step shows as no chain / wide launch and no hidden
  512 x 512 layer on the linear tiles but the ones the layered heads of that plan run ("linear<>" where there is none).
* tdmpc_encode at a, b and l against the oracle's h().

Tolerances are the project's standing ones, unchanged (parity_util.close). The fp32 oracle itself sits well inside
them at these first-layer widths: its estimate_value (T = 192, horizon 3) against the same oracle in float64, weights
and inputs cast, uses at most this share of `close` (plan_shapes_ref.oracle_fp32_share; weight seeds 7 | 21):

  a 0.09 | 0.11   b 0.02 | 0.17   c 0.04 | 0.12   d 0.12 | 0.11   e 0.13 | 0.12   f 0.04 | 0.05
  g 0.05 | 0.09   h 0.13 | 0.16   i 0.11 | 0.04   j 0.09 | 0.08   k 0.01 | 0.05   l 0.03 | 0.12

No shape uses more than 0.18 of the bound, so no row was moved to a smaller L. Measured on the GPU, max |gpu - oracle|
of estimate_value's values over the paths stays below 4.8e-6 at every shape, at most 0.35 of `close` (h; DESIGN.md has
the rows).

What these tests found: at i on path wide the plan's values were off by up to 1.5. With T = 192 rows per env the
launch over all rows at t = 0 of iteration 0 carries the z0c first layer, which the wide kernel takes only for
T % 128 == 0, so that one step ran on the chain kernel and stored z' where the folded first layers of t = 1 read h2.
step_next now splits that launch by role (wide kernel for the sampled rows, chain kernel for the policy rows), as it
does at every other t.
"""
import numpy as np
import pytest
import torch

import plan_shapes_ref as S
import test_gpu_plan_widths as W
from oracle import tdmpc_ref
from parity_util import close
from test_gpu_configs import _agent, _plan_calls_match_oracle
from test_gpu_plan import PATHS, _estimate_value_matches_oracle
from tdmpc_amd.told import synthetic_state_dict

pytestmark = pytest.mark.gpu

CHAIN_SHAPES, LAYERED_SHAPES = "abcdefghi", "jkl"      # chain_shape_ok true | false
PLAN_PATHS = ["auto", "layered", "chain", "chain16", "chain32", "chain_x6", "split", "split_x6", "wide"]
LAYERED_PATHS = ["auto", "layered", "chain_x6", "split"]
P1_PROF_CFG = 8     # tdmpc_profile_begin: the persistent plan's launch


def observed(agent, cfg, B):
    """(step kernel, Q kernel) of one plan: the persistent plan's name for both where it ran, else
    test_gpu_plan_widths.observed's pair."""
    obs = np.random.RandomState(1).standard_normal((B,) + tuple(cfg.obs_shape)).astype(np.float32)
    n, name = W._profile(agent, obs, P1_PROF_CFG)
    if n:
        assert n == 1, n
        return name, name
    return W.observed(agent, cfg, B)


# (shape, path, envs) -> (step kernel, Q kernel), from the predicates. A head launch has 192 rows per env (6 32-row
# blocks); the last step launch the profiler names is iteration 2's, over the 128 sampled rows per env.
_S16, _Q16 = "chain16_kernel<CH_STEP, x6>", "chain16_kernel<CH_Q, x6>"
_S16F, _Q16F = "chain16_kernel<CH_STEP, f32>", "chain16_kernel<CH_Q, f32>"
_S32, _Q32 = "chain_kernel<CH_STEP, x6>", "chain_kernel<CH_Q, x6>"
_S32F, _Q32F = "chain_kernel<CH_STEP, f32>", "chain_kernel<CH_Q, f32>"
# pick_cfg for the hidden 512 x 512 layers: < 512 rows the 32 x 32 latency tile (1), from 512 rows and for the Q heads'
# LayerNorm layers 32 x 64 (2), from 4096 rows the LDS tile (3)
_L0, _L2, _L3, _L12, _L23 = "linear<>", "linear<2>", "linear<3>", "linear<1, 2>", "linear<2, 3>"
_P4, _P6 = "plan1_kernel<4>", "plan1_kernel<6>"          # p1_ks: (Kx + 31) / 32 <= 4 ? 4 : 6


def _chain_shape_rows(s):
    out = {}
    for B in S.BATCHES[s]:
        big = B == 32
        # layered: the step's and pi's hidden layers on tile 1 (2 from 512 rows), the Q heads' on 2; at 32 envs 2048
        # policy rows on 2, everything else (>= 4096 rows) on 3
        out[(s, "layered", B)] = (_L23, _L23) if big else (_L12, _L12)
        # chain: chain_rb gives 16-row blocks up to num_cus / 2 = 128 32-row blocks x heads (8 B for the step's last
        # launch, 12 B for Q), x6 by default
        out[(s, "chain", B)] = (_S32, _Q32) if big else (_S16, _Q16)
        out[(s, "chain16", B)] = (_S16F, _Q16F)           # the forced row blocks keep the exact f32 MFMA
        out[(s, "chain32", B)] = (_S32F, _Q32F)
        out[(s, "chain_x6", B)] = (_S32, _Q32)
        # split / split_x6: the step and pi on split_step_kernel (no name), the Q heads layered (tile 2). At 32 envs
        # the 6144-row launches exceed the split's 4096 partial rows: iteration 0's steps, the terminal pi and Q are
        # layered on tile 3, the 2048 policy rows' pi and the later 4096-row steps split
        out[(s, "split", B)] = out[(s, "split_x6", B)] = (_L3, _L3) if big else (_L2, _L2)
        # wide without an instance (wide_instance: (rup(Kx, 32) / 32, rup(L, 16) / 16) is in the table at i only):
        # the 32-row x6 chain kernel
        out[(s, "wide", B)] = (_S32, _Q32)
    d = S.derived(s)
    step_split, pi_split = -(-d["Kx"] // 16) * 16 <= 256, -(-d["Lp"] // 16) * 16 <= 256     # use_split / use_split_pi, auto
    p1 = d["Kx"] <= 192 and d["Lp"] <= 192 and d["Lr"] <= 128 and d["Ar"] <= 128            # p1_dims_ok
    # auto, one env: the persistent plan where p1_dims_ok; else 12 blocks x heads are under every chain threshold
    # (64, Q 32): split where admitted, else layered
    if p1:
        one = (_P4, _P4) if -(-d["Kx"] // 32) <= 4 else (_P6, _P6)
    else:
        one = (_L2, _L2) if step_split else (_L12, _L12)
    out[(s, "auto", 1)] = out[(s, "persist", 1)] = one
    # auto, 3 envs: Q's 36 blocks x heads reach its threshold 32 (16-row blocks, x6), the step's 36 / 24 do not reach 64
    out[(s, "auto", 3)] = (_L0 if step_split and pi_split else _L12, _Q16)
    if 32 in S.BATCHES[s]:
        out[(s, "auto", 32)] = (_S32, _Q32)               # 256 / 384 blocks x heads: chain, 32-row blocks
    return out


KERNELS = {}
for _s in CHAIN_SHAPES:
    KERNELS.update(_chain_shape_rows(_s))
# i: path wide runs wide_step_kernel<17, 32> (17 first-layer 32-k groups of Kx 536: x streamed, XS), the sampled rows'
# rollout through the folded first layer (h2 out, OUTH, at the last step too: the terminal heads are folded chain
# launches); Q on the x6 chain kernel
KERNELS[("i", "wide", 1)] = KERNELS[("i", "wide", 3)] = ("wide_step_kernel<17, 32, XS|OUTH>", _Q32)
assert {k: v[0][:5] for k, v in KERNELS.items() if k[1] in ("chain", "chain16", "chain32", "chain_x6")} == \
    {(s, p, B): "chain" for s in CHAIN_SHAPES for p in ("chain", "chain16", "chain32", "chain_x6") for B in S.BATCHES[s]}
# the auto rows spelled out, as a check of the rules above against the table in the docstring
assert {s: KERNELS[(s, "auto", 1)][0] for s in CHAIN_SHAPES} == dict(a=_P4, b=_P4, c=_P6, d=_L2, e=_L2, f=_L12, g=_L12,
                                                                     h=_L12, i=_L12)
assert {s: KERNELS[(s, "auto", 3)][0] for s in CHAIN_SHAPES} == dict(a=_L0, b=_L0, c=_L0, d=_L0, e=_L0, f=_L12, g=_L12,
                                                                     h=_L12, i=_L12)
# j, k, l: chain_shape_ok is false (j: Ap > 64; k, l: 17 / 32 last-layer blocks), so every chain path is layered. j is
# plan1-eligible at one env (KS 4) and split-eligible (Kx 128); k (Kx 544) only where the split is forced; at l
# (Kx 1024) the split's LDS (77 KB > 64 KB) refuses it there too
KERNELS.update({
    ("j", "auto", 1): (_P4, _P4), ("j", "persist", 1): (_P4, _P4), ("j", "auto", 3): (_L2, _L2),
    **{("j", p, B): (_L12, _L12) for p in ("layered", "chain_x6") for B in (1, 3)},
    **{("j", "split", B): (_L2, _L2) for B in (1, 3)},
    **{("k", p, B): (_L12, _L12) for p in ("auto", "layered", "chain_x6", "persist") for B in (1, 3)},
    **{("k", "split", B): (_L2, _L2) for B in (1, 3)},
    **{("l", p, B): (_L12, _L12) for p in ("auto", "layered", "chain_x6", "split", "persist") for B in (1, 3)},
})
CASES = [(s, B, p) for s in S.SHAPES for B in S.BATCHES[s] for p in (PLAN_PATHS if s in CHAIN_SHAPES else LAYERED_PATHS)]
CASES += [(s, 1, "persist") for s in S.SHAPES]
assert all((s, p, B) in KERNELS for s, B, p in CASES)


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_estimate_value_at_other_shapes(shape):
    """Every path (and auto) at T = 192 rows, horizon 3: z_H, the last reward and the values against the oracle."""
    cfg = S.shape_cfg(shape)
    for path in PATHS + ["auto"]:
        _estimate_value_matches_oracle(cfg, _agent(cfg, 7, path=path), cfg.horizon)


def _inputs(cfg, shape, B):
    per_env = [S.env_inputs(cfg, s) for s in S.SEEDS[shape][:B]]
    return lambda ci: (np.stack([e[ci][0] for e in per_env]), [e[ci][1] for e in per_env])


_ORACLE = {}     # (shape, B) -> the oracle's plans, shared by the paths


@pytest.mark.parametrize("shape,B,path", CASES, ids=lambda v: str(v))
def test_plan_at_other_shapes(shape, B, path):
    """Cold, warm and mixed-t0 plans against the oracle, no near-tie escape, and the kernels that ran, by name."""
    cfg = S.shape_cfg(shape)
    agent = _agent(cfg, S.WSEED, B=B, path=path)
    name = f"shape-{shape}-{path}"
    sames = _plan_calls_match_oracle(name, cfg, agent, B, inputs=_inputs(cfg, shape, B),
                                     ref_cache=_ORACLE.setdefault((shape, B), {}))
    assert len(sames) == B * (3 if B > 1 else 2) and all(sames), (name, B, sames)   # no near-tie escape
    assert int(agent.planner.status.item()) == 0
    got = observed(agent, cfg, B)
    assert got == KERNELS[(shape, path, B)], (name, B, got)
    if shape in LAYERED_SHAPES and not got[0].startswith("plan1"):
        assert got[0].startswith("linear") and got[1].startswith("linear"), got
    if (shape, path) == ("i", "wide"):
        assert got[0].startswith("wide_step_kernel<17, 32"), got
    if path in ("persist", "auto") and B == 1:      # the persistent plan where p1_dims_ok, its refusal elsewhere
        assert got[0].startswith("plan1_kernel") == (shape in "abcj"), got


@pytest.mark.parametrize("shape", ["a", "b", "l"])
def test_encoder_at_other_shapes(shape):
    """tdmpc_encode against the oracle's h(): enc_matvec shares its 1024 threads as np = 1024 / nout per output, at
    nout = enc_dim | latent_dim = 64 | 8 (a), 96 | 90 (b: np = 10 | 11) and 1000 | 1000 (l: np = 1)."""
    cfg = S.shape_cfg(shape)
    agent = _agent(cfg, 11, B=3)
    pl = agent.planner
    pl.pack(agent.model)
    obs = torch.from_numpy(np.random.RandomState(0).standard_normal((3,) + tuple(cfg.obs_shape)).astype(np.float32))
    z = pl.encode(obs).cpu().numpy()
    zr = tdmpc_ref.RefTOLD(synthetic_state_dict(cfg, 11), cfg).h(obs).numpy()
    assert z.shape == zr.shape == (3, cfg.latent_dim)
    assert close(z, zr, atol=1e-5, rtol=1e-4).all(), np.abs(z - zr).max()
