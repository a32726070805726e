"""GPU: drnn_step_kernel and the DSSM pack over every shape branch drnn_check admits, against the float64 restatement
(tests/drnn_ref.py with dtype=torch.float64). tests/test_gpu_drnn.py runs the two stock shapes against the fp32 CPU
restatement; here each (task, latent_dim, hidden_dim) is picked for a branch of the kernel or the packer:

  task (A -> Ap)         L    Hd   hits
  cartpole (1 -> 8)      8    32   Kx = 16: one k-group of W_ih; one gate wave; nb3 = 1 (8 k-slices of the prior)
  cheetah (6 -> 8)       64   96   Kx = 72: 5 k-groups, the last 8 k zero-staged and zero-packed; 3 gate waves
  quadruped (12 -> 16)   90   160  Kx = 112: 7 k-groups; nb3 = 3 (6 of 8 waves busy); 5 gate waves; 6 pad columns
  dog (38 -> 40)         100  128  Kx = 144: 9 k-groups -- the reference's dog configuration
  humanoid (21 -> 24)    129  224  Lr = 160: nb3 = 5 (one k-slice); 7 pad columns; 7 gate waves
  humanoid               200  192  nb3 = 7; 6 gate waves
  dog                    256  256  Kx = 296: 19 k-groups with padding; nb3 = 8; the largest LDS footprint

(tdmpc_drnn_sizes_for accepts all seven as listed, so none is replaced. Hd 32, 96, 160 and 224 are also the widths at
which the six LayerNorm vectors of the pack do not start on multiples of 64 floats: tests/test_cpu_pack.py holds the
pack's jobs to disjoint ranges there.)

Tolerances are the project's standing ones (tests/test_gpu_plan.py's header), here against float64: latents, hidden
states, rewards and values within 1e-5 + 1e-4 |ref| (parity_util.close), actions within atol 2e-5. On these shapes and
inputs the fp32 CPU restatement itself uses at most 0.07 of `close` against float64 (0.30 on the stressed inputs, 0.09
at H = 16), so the yardstick sits far inside the bound. Every comparison prints max |gpu - f64| beside
max |fp32cpu - f64| (DESIGN.md's DSSM section quotes them).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import drnn_ref
from drnn_io import drnn_cfg
from parity_util import close, near_tie, record
from test_gpu_drnn import _agent, _next_raw
from tdmpc_amd.dssm import synthetic_dssm_state_dict

pytestmark = pytest.mark.gpu

SHAPES = [("cartpole", 8, 32), ("cheetah", 64, 96), ("quadruped", 90, 160), ("dog", 100, 128),
          ("humanoid", 129, 224), ("humanoid", 200, 192), ("dog", 256, 256)]
STRESSED = [("cheetah", 64, 96), ("humanoid", 200, 192), ("dog", 256, 256)]
E_DIMS = -1   # TDMPC_E_DIMS (include/tdmpc_hip.h)


def _cfg(task, L, Hd, **kw):
    # T = 48 rows per env (N = 32, P = 16); max_batch 2 -> the X panel holds 96 rows
    kw.setdefault("iterations", 1)
    return drnn_cfg(task, latent_dim=L, hidden_dim=Hd, num_samples=32, num_elites=8, regularization_schedule="0.5", **kw)


_PLANNERS = {}


def _shape(task, L, Hd):
    """One planner (seed-7 weights) and its fp32 / fp64 restatements per shape, shared and left unchanged."""
    key = (task, L, Hd)
    if key not in _PLANNERS:
        cfg = _cfg(task, L, Hd)
        agent, sd = _agent(cfg, 7, max_batch=2)
        _PLANNERS[key] = (cfg, agent, drnn_ref.RefDSSM(sd, cfg), drnn_ref.RefDSSM(sd, cfg, torch.float64))
    return _PLANNERS[key]


def _inputs(rs, rows, cfg):
    z = torch.from_numpy(rs.standard_normal((rows, cfg.latent_dim)).astype(np.float32))
    a = torch.from_numpy(rs.uniform(-1, 1, (rows, cfg.action_dim)).astype(np.float32))
    h = torch.from_numpy(rs.uniform(-1, 1, (rows, cfg.hidden_dim)).astype(np.float32))
    return z, a, h


def _check_next(tag, pl, ref32, ref64, z, a, h):
    """One tdmpc_drnn_next over the rows of (z, a, h) against float64; returns the GPU outputs."""
    rows = z.shape[0]
    want = ref64.next(z.double(), a.double(), h.double())
    cpu = ref32.next(z, a, h)
    got = _next_raw(pl, z.cuda(), a.cuda(), h.cuda(), rows)
    for name, g, w, c in zip(("z", "h", "r"), got, want, cpu):
        g, w, c = g.numpy().reshape(rows, -1), w.numpy().reshape(rows, -1), c.numpy().reshape(rows, -1)
        print(f"{tag} rows {rows} {name}: max |gpu - f64| {np.abs(g - w).max():.3e}, "
              f"max |fp32cpu - f64| {np.abs(c - w).max():.3e}")
        bad = ~close(g, w)
        assert not bad.any(), (tag, rows, name, np.abs(g - w).max(), np.argwhere(bad)[:4].tolist())
    return got


@pytest.mark.parametrize("task,L,Hd", SHAPES)
def test_next_matches_float64(task, L, Hd):
    """DSSM.next at each shape: one row, a ragged second block, two full blocks and the largest row count the entry
    point accepts (the X panel's 96 rows); one row more is TDMPC_E_DIMS and nothing is launched."""
    cfg, agent, ref32, ref64 = _shape(task, L, Hd)
    pl = agent.planner
    assert (pl.dims.latent_dim, pl.hidden_dim, pl.dims.action_dim) == (L, Hd, cfg.action_dim)
    xrows = (2 * pl.T + 31) // 32 * 32
    assert xrows == 96
    rs = np.random.RandomState(3)
    for rows in (1, 33, 64, xrows):
        z, a, h = _inputs(rs, rows, cfg)
        _check_next(f"{task} L {L} Hd {Hd}", pl, ref32, ref64, z, a, h)
    rows = xrows + 1
    z, a, h = (t.cuda() for t in _inputs(rs, rows, cfg))
    S = 12345.0
    zo, ho, ro = (torch.full(s, S, device="cuda") for s in ((rows, L), (rows, Hd), (rows,)))
    vp = C.c_void_p
    rc = pl.L.tdmpc_drnn_next(C.byref(pl.ddims), vp(pl.packed.data_ptr()), vp(z.data_ptr()), vp(a.data_ptr()),
                              vp(h.data_ptr()), rows, vp(zo.data_ptr()), vp(ho.data_ptr()), vp(ro.data_ptr()),
                              vp(pl.workspace.data_ptr()), pl.workspace.numel() * 4,
                              vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == E_DIMS and pl.L.tdmpc_last_error()
    assert all(bool((t == S).all()) for t in (zo, ho, ro)), "a refused call wrote its outputs"


def _stressed_sd(cfg, seed):
    """The synthetic weights with the GRU cell's three LayerNorms' gains and shifts x 4: about 12 % of h' saturates
    beyond |0.99|. (x 30 would break the tolerance in the fp32 restatement itself: conditioning, not the kernel.)"""
    sd = synthetic_dssm_state_dict(cfg, seed)
    for k in sd:
        if k.startswith("_dynamics.gru_cell.ln_"):
            sd[k] = sd[k] * 4
    return sd


@pytest.mark.parametrize("task,L,Hd", STRESSED)
def test_next_stressed_inputs_match_float64(task, L, Hd):
    """Saturated gates and degenerate rows in one 40-row call: z x 10; h = 0; z = a = 0; h = 1 everywhere (a constant
    row into W_hh: the variance-near-zero edge of the two-pass LayerNorm); h x 1e-3; z and a x 1e-3."""
    from tdmpc_amd.drnn import TdMpcDrnn
    cfg = _cfg(task, L, Hd)
    agent = TdMpcDrnn(cfg, max_batch=2)
    sd = _stressed_sd(cfg, 7)
    agent.model.load_state_dict(sd)
    agent.planner.pack(agent.model)
    z, a, h = _inputs(np.random.RandomState(5), 40, cfg)
    z[0:8] *= 10
    h[8:16] = 0
    z[16:24] = 0
    a[16:24] = 0
    h[24:32] = 1.0
    h[32:36] *= 1e-3
    z[36:40] *= 1e-3
    a[36:40] *= 1e-3
    got = _check_next(f"stressed {task} L {L} Hd {Hd}", agent.planner, drnn_ref.RefDSSM(sd, cfg),
                      drnn_ref.RefDSSM(sd, cfg, torch.float64), z, a, h)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    print(f"stressed {task} L {L} Hd {Hd}: {float((got[1].abs() > 0.99).float().mean()):.3f} of h' beyond |0.99|")


def test_next_nonfinite_rows_stay_alone_at_an_odd_shape():
    """quadruped L 90 Hd 160 (7 k-groups, two idle waves in the prior's last layer, 5 gate waves), 70 rows: a NaN in z
    of row 33, an Inf in h of row 2 and a NaN in a of row 69. Every other row, the other rows of all three blocks
    included, equals the clean run bitwise in z', h' and r; the three dirty rows are non-finite in h'."""
    cfg, agent, _, _ = _shape("quadruped", 90, 160)
    pl = agent.planner
    rows = 70
    z, a, h = (t.cuda() for t in _inputs(np.random.RandomState(4), rows, cfg))
    clean = _next_raw(pl, z, a, h, rows)
    z2, a2, h2 = z.clone(), a.clone(), h.clone()
    z2[33, 57] = float("nan")
    h2[2, 131] = float("inf")
    a2[69, 11] = float("nan")
    dirty = _next_raw(pl, z2, a2, h2, rows)
    keep = np.array([i for i in range(rows) if i not in (2, 33, 69)])
    for c, d in zip(clean, dirty):
        assert torch.isfinite(c).all()
        assert torch.equal(c[keep], d[keep])
    for i in (2, 33, 69):
        assert not torch.isfinite(dirty[1][i]).all(), i


_H16 = {}


def _h16():
    if not _H16:
        cfg = _cfg("quadruped", 90, 160, horizon=16)
        agent, sd = _agent(cfg, 7, max_batch=2)
        _H16["v"] = (cfg, agent, drnn_ref.RefDSSM(sd, cfg), drnn_ref.RefDSSM(sd, cfg, torch.float64))
    return _H16["v"]


def test_estimate_value_at_the_longest_horizon():
    """estimate_value at H = 16 (max_horizon's cap: 16 hidden ping-pongs, 17 X panels, 16 G accumulations), two envs
    with their own z0 and h0, T = 48 candidates each, against float64. A candidate with a NaN action at the last step
    is worth exactly 0; the last step's reward is compared where the restatement's is finite."""
    cfg, agent, ref32, ref64 = _h16()
    pl = agent.planner
    B, H, T, A, L, Hd = 2, 16, pl.T, cfg.action_dim, cfg.latent_dim, cfg.hidden_dim
    assert T == 48 and pl.dims.max_horizon == 16
    rs = np.random.RandomState(16)
    z0 = torch.from_numpy(rs.standard_normal((B, L)).astype(np.float32))
    h0 = torch.from_numpy(rs.uniform(-1, 1, (B, Hd)).astype(np.float32))
    act = torch.from_numpy(rs.uniform(-1, 1, (B, H, T, A)).astype(np.float32))
    eps = torch.from_numpy(rs.standard_normal((B, T, A)).astype(np.float32))
    act[1, 15, 5, 3] = float("nan")
    vg, rg = pl.estimate_value(z0, h0, act, eps, H)
    vg, rg = vg.cpu().numpy(), rg.cpu().numpy()
    for e in range(B):
        tr = {}
        v64, _ = drnn_ref.estimate_value(ref64, cfg, z0[e:e + 1].double().repeat(T, 1), act[e].double(),
                                         h0[e:e + 1].double().repeat(T, 1), H, eps[e].double(), trace=tr)
        v32, _ = drnn_ref.estimate_value(ref32, cfg, z0[e:e + 1].repeat(T, 1), act[e], h0[e:e + 1].repeat(T, 1), H,
                                         eps[e])
        v64, v32 = v64.squeeze(1).numpy(), v32.squeeze(1).numpy()
        print(f"estimate_value H 16 env {e}: max |G_gpu - G_f64| {np.abs(vg[e] - v64).max():.3e}, "
              f"max |G_fp32cpu - G_f64| {np.abs(v32 - v64).max():.3e}")
        assert close(vg[e], v64).all(), (e, np.abs(vg[e] - v64).max())
        rl = tr["reward_last"].squeeze(1).numpy()
        fin = np.isfinite(rl)
        assert fin.sum() == T - (e == 1)
        assert np.array_equal(np.isfinite(rg[e]), fin), e
        print(f"estimate_value H 16 env {e}: max |r_last gpu - f64| {np.abs(rg[e][fin] - rl[fin]).max():.3e}")
        assert close(rg[e][fin], rl[fin]).all(), (e, np.abs(rg[e][fin] - rl[fin]).max())
    assert vg[1, 5] == 0.0
    assert np.isfinite(vg).all()


def test_pi_rollout_at_the_longest_horizon():
    """pi_rollout at H = 16: the policy rows' 15 carried-hidden steps, two envs, against float64 at atol 2e-5."""
    cfg, agent, ref32, ref64 = _h16()
    pl = agent.planner
    B, H, P, A = 2, 16, pl.P, cfg.action_dim
    assert P == 16
    rs = np.random.RandomState(17)
    z0 = torch.from_numpy(rs.standard_normal((B, cfg.latent_dim)).astype(np.float32))
    h0 = torch.from_numpy(rs.uniform(-1, 1, (B, cfg.hidden_dim)).astype(np.float32))
    eps = torch.from_numpy(rs.standard_normal((B, H, P, A)).astype(np.float32))
    got = pl.pi_rollout(z0, h0, eps, H).cpu().numpy()
    for e in range(B):
        w64 = drnn_ref.pi_rollout(ref64, cfg, z0[e:e + 1].double(), h0[e:e + 1].double(), H, P, eps[e].double()).numpy()
        w32 = drnn_ref.pi_rollout(ref32, cfg, z0[e:e + 1], h0[e:e + 1], H, P, eps[e]).numpy()
        print(f"pi_rollout H 16 env {e}: max |a_gpu - a_f64| {np.abs(got[e] - w64).max():.3e}, "
              f"max |a_fp32cpu - a_f64| {np.abs(w32 - w64).max():.3e}")
        np.testing.assert_allclose(got[e], w64, atol=2e-5, rtol=0)


DOG_WSEED, DOG_ISEED = 7, 36   # see test_plan_at_the_dog_shape


def test_plan_at_the_dog_shape():
    """Two TdMpcDrnn.plan calls (an episode start, then a warm start) at the reference's dog configuration (L 100,
    A 38: Kx = 144, 9 k-groups of W_ih) with the restatement's explicit draws, compared as
    test_plan_matches_restatement_on_recorded_calls does. Weight seed 7 and input seed 36 (draw seeds 300 + call /
    400 + call) keep the K-th and (K+1)-th values of every iteration at least 1e-3 (1 + |cut|) apart in the fp32 CPU
    restatement alone (checked below before anything is compared), so no near-tie escape is expected."""
    cfg = drnn_cfg("dog", num_samples=32, num_elites=8, iterations=2, horizon=3)
    assert (cfg.latent_dim, cfg.action_dim, cfg.hidden_dim) == (100, 38, 128)
    agent, sd = _agent(cfg, DOG_WSEED, graph=False)
    ref = drnn_ref.RefDSSM(sd, cfg)
    st = drnn_ref.DrnnState(0.05, cfg.warmup_len)
    rs = np.random.RandomState(DOG_ISEED)
    obs = rs.standard_normal((2, cfg.obs_shape[0])).astype(np.float32)
    hidden = rs.uniform(-1, 1, (1, cfg.hidden_dim)).astype(np.float32)
    K, step = cfg.num_elites, 10**6
    for ci, t0 in enumerate((True, False)):
        torch.manual_seed(300 + ci)
        np.random.seed(400 + ci)
        nz = drnn_ref.draw_drnn_noise(cfg, st, step, t0, False)
        rtr, gtr = {}, {}
        ra, rm = drnn_ref.plan(ref, cfg, st, obs[ci], hidden, nz, step=step, t0=t0, trace=rtr)
        ga, gm = agent.plan(obs[ci], hidden, step=step, t0=t0, noise=nz, trace=gtr)
        assert agent.plan_horizon == st.plan_horizon == 3 and agent.planner.P == 16
        same = True
        for i, rv in enumerate(rtr["value"]):
            rv = rv.squeeze(1).numpy()
            srt = np.sort(rv.astype(np.float64))[::-1]
            assert srt[K - 1] - srt[K] >= 1e-3 * (1 + abs(srt[K - 1])), ("the seeds leave a near tie", ci, i)
            gv = gtr["value"][0, i].cpu().numpy()
            assert gv.shape == rv.shape
            print(f"dog call {ci} iteration {i}: max |dG| {np.abs(gv - rv).max():.3e}")
            assert close(gv, rv).all(), (ci, i, np.abs(gv - rv).max())
            eg = set(np.argsort(-gv, kind="stable")[:K]); er = set(np.argsort(-rv, kind="stable")[:K])
            if eg != er:
                assert near_tie(rv, eg, er, K), (ci, i, "elite sets differ away from the cut-off")
                same = False
                break
        record(same, f"drnn/dog/call{ci}")
        if not same:
            break
        np.testing.assert_allclose(ga.cpu().numpy(), ra.numpy(), atol=2e-5, rtol=0)
        np.testing.assert_allclose(agent._prev_mean.cpu().numpy(), st.prev_mean.numpy(), atol=2e-5, rtol=0)
        assert gm["intrinsic_reward_mean"] == 0.0
        np.testing.assert_allclose([gm["external_reward_mean"], gm["current_std"]],
                                   [rm["external_reward_mean"], rm["current_std"]], atol=2e-5, rtol=0)


def test_repack_leaves_nothing_behind():
    """cheetah L 64 Hd 96 (the shape with padded k): a planner that packed seed-7 weights, ran next, then loaded and
    packed seed-8 weights computes next bitwise like a fresh planner that only ever saw seed 8."""
    cfg = _cfg("cheetah", 64, 96)
    used, _ = _agent(cfg, 7, max_batch=2)
    z, a, h = (t.cuda() for t in _inputs(np.random.RandomState(6), 40, cfg))
    first = _next_raw(used.planner, z, a, h, 40)
    sd8 = synthetic_dssm_state_dict(cfg, 8)
    used.model.load_state_dict(sd8)
    used.planner.pack(used.model)
    again = _next_raw(used.planner, z, a, h, 40)
    fresh, _ = _agent(cfg, 8, max_batch=2)
    want = _next_raw(fresh.planner, z, a, h, 40)
    for f, g, w in zip(first, again, want):
        assert not torch.equal(f, w), "the two weight sets give the same output"
        assert torch.equal(g, w)
