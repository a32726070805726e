"""GPU: the recurrent-latent (DSSM) planner (include/tdmpc_drnn.h, tdmpc_amd/drnn.py) against the CPU restatement
tests/drnn_ref.py, which tests/test_drnn_cpu.py pins to the reference bit for bit.

Tolerances are the project's own (tests/test_gpu_plan.py's header): values, latents, hidden states and rewards within
1e-5 + 1e-4 |ref| (parity_util.close); actions, prev_mean and metrics within atol 2e-5 while every iteration's elite set
agrees, near-tie escapes counted through parity_util.record (the recorded inputs keep the K-th and (K+1)-th values
1e-3 (1 + |cut|) apart, so none is expected).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import drnn_ref
from drnn_io import case_inputs, cases, drnn_cfg
from parity_util import close, near_tie, record
from tdmpc_amd import _lib
from tdmpc_amd.dssm import synthetic_dssm_state_dict

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _agent(cfg, wseed, max_batch=1, **kw):
    from tdmpc_amd.drnn import TdMpcDrnn
    agent = TdMpcDrnn(cfg, max_batch=max_batch, **kw)
    sd = synthetic_dssm_state_dict(cfg, wseed)
    agent.model.load_state_dict(sd)
    agent.std = 0.05
    agent.planner.pack(agent.model)
    return agent, sd


def _unit_cfg(task, Hd):
    # N = 64, mixture 0.5 -> T = 96 rows per env
    return drnn_cfg(task, hidden_dim=Hd, num_samples=64, num_elites=16, iterations=2, horizon=5,
                    regularization_schedule="0.5")


_UNIT = {}


def _unit(task, Hd):
    """One planner and restatement per (task, Hd), shared by the unit tests."""
    if (task, Hd) not in _UNIT:
        cfg = _unit_cfg(task, Hd)
        agent, sd = _agent(cfg, 7, max_batch=3)
        _UNIT[(task, Hd)] = (cfg, agent, drnn_ref.RefDSSM(sd, cfg))
    return _UNIT[(task, Hd)]


def _next_raw(pl, z, a, h, rows, pad=8):
    """tdmpc_drnn_next through the raw ABI into sentinel-filled outputs with `pad` spare rows."""
    dev, L, Hd = pl.device, pl.dims.latent_dim, pl.hidden_dim
    S = 12345.0
    zo = torch.full((rows + pad, L), S, device=dev)
    ho = torch.full((rows + pad, Hd), S, device=dev)
    ro = torch.full((rows + pad,), S, device=dev)
    vp = C.c_void_p
    rc = pl.L.tdmpc_drnn_next(C.byref(pl.ddims), vp(pl.packed.data_ptr()), vp(z.data_ptr()), vp(a.data_ptr()),
                              vp(h.data_ptr()), rows, vp(zo.data_ptr()), vp(ho.data_ptr()), vp(ro.data_ptr()),
                              vp(pl.workspace.data_ptr()), pl.workspace.numel() * 4,
                              vp(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "tdmpc_drnn_next")
    torch.cuda.synchronize()
    for t in (zo, ho, ro):
        assert bool((t[rows:] == S).all()), "wrote past `rows`"
    return zo[:rows].cpu(), ho[:rows].cpu(), ro[:rows].cpu()


@pytest.mark.parametrize("task,Hd", [("humanoid", 128), ("cheetah", 128), ("humanoid", 64), ("cheetah", 256)])
def test_next_matches_restatement(task, Hd):
    """DSSM.next on drnn_step_kernel: full blocks, ragged tails, one row, several blocks."""
    cfg, agent, ref = _unit(task, Hd)
    pl = agent.planner
    rs = np.random.RandomState(3)
    for rows in (1, 31, 32, 33, 160):
        z = torch.from_numpy(rs.standard_normal((rows, cfg.latent_dim)).astype(np.float32))
        a = torch.from_numpy(rs.uniform(-1, 1, (rows, cfg.action_dim)).astype(np.float32))
        h = torch.from_numpy(rs.uniform(-1, 1, (rows, Hd)).astype(np.float32))
        zr, hr, rr = ref.next(z, a, h)
        zg, hg, rg = _next_raw(pl, z.cuda(), a.cuda(), h.cuda(), rows)
        for name, g, r in (("z", zg, zr), ("h", hg, hr), ("r", rg, rr.squeeze(1))):
            err = np.abs(g.numpy() - r.numpy()).max()
            print(f"{task} Hd {Hd} rows {rows} {name}: max |d| {err:.3e}")
            assert close(g.numpy(), r.numpy()).all(), (rows, name, err)


def test_next_nonfinite_rows_stay_alone():
    """A NaN hidden state in one row and an Inf action in another: every other row equals the clean run bitwise."""
    cfg, agent, ref = _unit("humanoid", 128)
    pl = agent.planner
    rs = np.random.RandomState(4)
    rows = 70
    z = torch.from_numpy(rs.standard_normal((rows, cfg.latent_dim)).astype(np.float32)).cuda()
    a = torch.from_numpy(rs.uniform(-1, 1, (rows, cfg.action_dim)).astype(np.float32)).cuda()
    h = torch.from_numpy(rs.uniform(-1, 1, (rows, 128)).astype(np.float32)).cuda()
    clean = _next_raw(pl, z, a, h, rows)
    h2, a2 = h.clone(), a.clone()
    h2[5, 17] = float("nan")
    a2[40, 3] = float("inf")
    dirty = _next_raw(pl, z, a2, h2, rows)
    keep = np.array([i for i in range(rows) if i not in (5, 40)])
    for c, d in zip(clean, dirty):
        assert torch.equal(c[keep], d[keep])
    assert not torch.isfinite(dirty[1][5]).all() and not torch.isfinite(dirty[1][40]).all()


@pytest.mark.parametrize("H", [1, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_estimate_value_matches_restatement(B, H):
    """estimate_value for T = 96 candidates per env (N = 64, P = 32), each env from its own latent and hidden state;
    a candidate with a non-finite action is worth 0 (nan_to_num). For B = 3, H = 5 the float64 restatement's distance
    to both fp32 forms is printed (DESIGN.md quotes it)."""
    cfg, agent, ref = _unit("humanoid", 128)
    pl = agent.planner
    T, A, L = pl.T, cfg.action_dim, cfg.latent_dim
    assert T == 96
    rs = np.random.RandomState(10 * B + H)
    z0 = torch.from_numpy(rs.standard_normal((B, L)).astype(np.float32))
    h0 = torch.from_numpy(rs.uniform(-1, 1, (B, 128)).astype(np.float32))
    act = torch.from_numpy(rs.uniform(-1, 1, (B, H, T, A)).astype(np.float32))
    eps = torch.from_numpy(rs.standard_normal((B, T, A)).astype(np.float32))
    act[0, 0, 7, 2] = float("nan")
    act[B - 1, H - 1, 50, 0] = float("inf")
    vg, rg = pl.estimate_value(z0, h0, act, eps, H)
    vg, rg = vg.cpu().numpy(), rg.cpu().numpy()
    ref64 = drnn_ref.RefDSSM(ref.sd, cfg, torch.float64)
    e32 = e64 = 0.0
    for e in range(B):
        tr = {}
        v, _ = drnn_ref.estimate_value(ref, cfg, z0[e:e + 1].repeat(T, 1), act[e], h0[e:e + 1].repeat(T, 1), H, eps[e],
                                       trace=tr)
        v = v.squeeze(1).numpy()
        assert close(vg[e], v).all(), (e, np.abs(vg[e] - v).max())
        # the last step's reward per row (NaN where the restatement's is NaN: the non-finite candidates)
        rl = tr["reward_last"].squeeze(1).numpy()
        fin = np.isfinite(rl)
        assert np.array_equal(np.isfinite(rg[e]), fin), e
        assert close(rg[e][fin], rl[fin]).all(), (e, np.abs(rg[e][fin] - rl[fin]).max())
        v64, _ = drnn_ref.estimate_value(ref64, cfg, z0[e:e + 1].double().repeat(T, 1), act[e].double(),
                                         h0[e:e + 1].double().repeat(T, 1), H, eps[e].double())
        v64 = v64.squeeze(1).numpy()
        e32 = max(e32, np.abs(v - v64).max())
        e64 = max(e64, np.abs(vg[e] - v64).max())
    print(f"estimate_value B {B} H {H}: max |G_gpu - G_fp64| {e64:.3e}, max |G_fp32cpu - G_fp64| {e32:.3e}")
    assert vg[0, 7] == 0.0 and vg[B - 1, 50] == 0.0
    assert np.isfinite(vg).all()


def test_pi_rollout_matches_restatement():
    cfg, agent, ref = _unit("cheetah", 128)
    pl = agent.planner
    B, H, P, A = 2, 4, pl.P, cfg.action_dim
    rs = np.random.RandomState(6)
    z0 = torch.from_numpy(rs.standard_normal((B, cfg.latent_dim)).astype(np.float32))
    h0 = torch.from_numpy(rs.uniform(-1, 1, (B, 128)).astype(np.float32))
    eps = torch.from_numpy(rs.standard_normal((B, H, P, A)).astype(np.float32))
    got = pl.pi_rollout(z0, h0, eps, H).cpu().numpy()
    for e in range(B):
        want = drnn_ref.pi_rollout(ref, cfg, z0[e:e + 1], h0[e:e + 1], H, P, eps[e]).numpy()
        np.testing.assert_allclose(got[e], want, atol=2e-5, rtol=0)


@pytest.mark.parametrize("name", ["humanoid", "cheetah", "horizon"])
def test_plan_matches_restatement_on_recorded_calls(name):
    """The recorded call sequences through TdMpcDrnn.plan with the restatement's draws (which are the reference's:
    tests/test_drnn_cpu.py): t0 / warm / eval calls, a memory that fills and wraps, the horizon schedule."""
    cfg, wseed, iseed, calls = cases()[name]
    agent, sd = _agent(cfg, wseed, graph=False)
    ref = drnn_ref.RefDSSM(sd, cfg)
    st = drnn_ref.DrnnState(0.05, cfg.warmup_len)
    obs, hidden = case_inputs(cfg, iseed, len(calls))
    K = cfg.num_elites
    for ci, (step, t0, ev) in enumerate(calls):
        torch.manual_seed(300 + ci)
        np.random.seed(400 + ci)
        nz = drnn_ref.draw_drnn_noise(cfg, st, step, t0, ev)
        rtr, gtr = {}, {}
        ra, rm = drnn_ref.plan(ref, cfg, st, obs[ci], hidden, nz, eval_mode=ev, step=step, t0=t0, trace=rtr)
        ga, gm = agent.plan(obs[ci], hidden, eval_mode=ev, step=step, t0=t0, noise=nz, trace=gtr)
        assert agent.plan_horizon == st.plan_horizon
        same = True
        for i, rv in enumerate(rtr["value"]):
            rv = rv.squeeze(1).numpy()
            gv = gtr["value"][0, i].cpu().numpy()
            assert gv.shape == rv.shape
            print(f"{name} call {ci} iteration {i}: max |dG| {np.abs(gv - rv).max():.3e}")
            assert close(gv, rv).all(), (ci, i, np.abs(gv - rv).max())
            eg = set(np.argsort(-gv, kind="stable")[:K]); er = set(np.argsort(-rv, kind="stable")[:K])
            if eg != er:
                assert near_tie(rv, eg, er, K), (ci, i, "elite sets differ away from the cut-off")
                same = False
                break
        record(same, f"drnn/{name}/call{ci}")
        if not same:
            break
        np.testing.assert_allclose(ga.cpu().numpy(), ra.numpy(), atol=2e-5, rtol=0)
        np.testing.assert_allclose(agent._prev_mean.cpu().numpy(), st.prev_mean.numpy(), atol=2e-5, rtol=0)
        assert gm["intrinsic_reward_mean"] == 0.0
        np.testing.assert_allclose([gm["external_reward_mean"], gm["current_std"]],
                                   [rm["external_reward_mean"], rm["current_std"]], atol=2e-5, rtol=0)
        assert len(agent.memory_latents) == len(st.memory)
        for (gz, gact), (rz, ract) in zip(agent.memory_latents, st.memory):
            assert close(gz.cpu().numpy(), rz[0].numpy()).all()
            np.testing.assert_allclose(gact.cpu().numpy(), ract[0].numpy(), atol=2e-5, rtol=0)


def test_plan_inside_the_mixture_ramp_matches_restatement():
    """regularization_schedule ramping over the calls: num_pi of a call (4, 8, then the planner's largest, 16) is below
    what the buffers are sized for, so the noise layout, the row maps and the workspace views change per call. Explicit
    draws against the restatement, then the same steps through graph replay (one graph per num_pi), whose values must
    be finite and whose draws are the restatement's."""
    cfg = drnn_cfg("cheetah", num_samples=32, num_elites=8, iterations=2, horizon=4,
                   regularization_schedule="linear(0.0, 0.5, 20000, 0)", horizon_schedule="4")
    agent, sd = _agent(cfg, 112, graph=False)
    assert agent.planner.pmax == 16
    ref = drnn_ref.RefDSSM(sd, cfg)
    st = drnn_ref.DrnnState(0.05, 0)
    rs = np.random.RandomState(31)
    hidden = rs.uniform(-1, 1, (1, cfg.hidden_dim)).astype(np.float32)
    K = cfg.num_elites
    torch.manual_seed(70)
    np.random.seed(71)
    for ci, (step, P) in enumerate([(5000, 4), (10000, 8), (10**6, 16)]):
        obs = rs.standard_normal(cfg.obs_shape).astype(np.float32)
        nz = drnn_ref.draw_drnn_noise(cfg, st, step, ci == 0, False)
        rtr, gtr = {}, {}
        ra, rm = drnn_ref.plan(ref, cfg, st, obs, hidden, nz, step=step, t0=ci == 0, trace=rtr)
        ga, gm = agent.plan(obs, hidden, step=step, t0=ci == 0, noise=nz, trace=gtr)
        assert agent.planner.P == P and gtr["value"].shape[-1] == 32 + P
        same = True
        for i, rv in enumerate(rtr["value"]):
            rv = rv.squeeze(1).numpy()
            gv = gtr["value"][0, i].cpu().numpy()
            assert close(gv, rv).all(), (ci, i, np.abs(gv - rv).max())
            eg = set(np.argsort(-gv, kind="stable")[:K]); er = set(np.argsort(-rv, kind="stable")[:K])
            if eg != er:
                assert near_tie(rv, eg, er, K), (ci, i, "elite sets differ away from the cut-off")
                same = False
                break
        record(same, f"drnn/ramp/call{ci}")
        if not same:
            break
        np.testing.assert_allclose(ga.cpu().numpy(), ra.numpy(), atol=2e-5, rtol=0)
        np.testing.assert_allclose(agent._prev_mean.cpu().numpy(), st.prev_mean.numpy(), atol=2e-5, rtol=0)
        np.testing.assert_allclose([gm["external_reward_mean"], gm["current_std"]],
                                   [rm["external_reward_mean"], rm["current_std"]], atol=2e-5, rtol=0)
    # graph replay: one captured plan per num_pi, each consuming the reference-order draws of its own layout
    g_agent, _ = _agent(cfg, 112)
    st2 = drnn_ref.DrnnState(0.05, 0)
    st2.plan_horizon = 4
    pl = g_agent.planner
    for step, P in [(5000, 4), (10000, 8), (5000, 4)]:
        torch.manual_seed(80)
        np.random.seed(81)
        nz = drnn_ref.draw_drnn_noise(cfg, st2, step, True, False, device="cuda")
        torch.manual_seed(80)
        np.random.seed(81)
        a, _ = g_agent.plan(obs, hidden, step=step, t0=True)
        assert torch.isfinite(a).all() and pl.P == P
        got = pl.noise_view(4, cfg.iterations, 1)[0].clone()
        pl.noise_flat.zero_()
        pl.load_noise(0, 4, cfg.iterations, nz.eps_pi, nz.eps_cem, nz.eps_term, nz.eps_act)
        assert torch.equal(got, pl.noise_view(4, cfg.iterations, 1)[0])
    assert len(pl._graphs) == 2


def test_reference_rng_draws_equal_restatement():
    """rng='reference' (one tdmpc_reference_normals launch from torch's generator state, numpy's uniform on the host)
    consumes exactly the restatement's torch / numpy draws: a t0 call and a warm eval call, graph replay included."""
    cfg, wseed, iseed, calls = cases()["humanoid"]
    agent, sd = _agent(cfg, wseed)
    st = drnn_ref.DrnnState(0.05, cfg.warmup_len)
    st.plan_horizon = 5
    obs, hidden = case_inputs(cfg, iseed, 2)
    pl = agent.planner
    for ci, (t0, ev) in enumerate([(True, False), (False, True)]):
        torch.manual_seed(50 + ci)
        np.random.seed(60 + ci)
        nz = drnn_ref.draw_drnn_noise(cfg, st, 10**6, t0, ev, device="cuda")
        after = (torch.randn(4, device="cuda"), np.random.random_sample())
        torch.manual_seed(50 + ci)
        np.random.seed(60 + ci)
        agent.plan(obs[ci], hidden, eval_mode=ev, step=10**6, t0=t0)
        H, I = 5, cfg.iterations
        got = pl.noise_view(H, I, 1)[0].clone()
        u = float(pl.u[0].cpu())
        pl.noise_flat.zero_()
        pl.load_noise(0, H, I, nz.eps_pi, nz.eps_cem, nz.eps_term, nz.eps_act)
        want = pl.noise_view(H, I, 1)[0]
        n = pl.noise_layout(H, I)["act_off"] + (0 if ev else cfg.action_dim)
        assert torch.equal(got[:n], want[:n])
        assert u == nz.u
        assert torch.equal(torch.randn(4, device="cuda"), after[0])
        assert np.random.random_sample() == after[1]


def test_plan_batch_equals_single_env_plans():
    """Three envs with their own hidden states, memories of different lengths (0, 1 and 2 entries of warmup_len 2) and
    mixed t0 in one plan_batch call agree with three single-env agents on the same draws."""
    cfg = drnn_cfg("cheetah", num_samples=32, num_elites=8, iterations=2, horizon=4, warmup_len=2)
    B, step = 3, 10**6
    batched, sd = _agent(cfg, 112, max_batch=B, graph=False)
    singles = [_agent(cfg, 112, graph=False)[0] for _ in range(B)]
    st = drnn_ref.DrnnState(0.05, 2)
    st.plan_horizon = 4
    rs = np.random.RandomState(8)
    hidden = rs.uniform(-1, 1, (B, cfg.hidden_dim)).astype(np.float32)
    torch.manual_seed(21)
    np.random.seed(22)
    # env 1 plans once, env 2 twice, on their own: memories of 0 / 1 / 2 entries before the batched call
    pre = {1: 1, 2: 2}
    for e, n in pre.items():
        for k in range(n):
            ob = rs.standard_normal(cfg.obs_shape).astype(np.float32)
            nz = drnn_ref.draw_drnn_noise(cfg, st, step, k == 0, False)
            a1, _ = singles[e].plan(ob, hidden[e:e + 1], step=step, t0=k == 0, noise=nz)
            # the batched agent's env e: the same history
            batched._memories[e].append((singles[e].memory_latents[-1][0].clone(), a1.clone()))
            batched._plan_H[e] = 4
            batched._has_prev[e], batched._prev_H[e] = True, 4
            batched.planner.prev_mean_view(4, B)[e].copy_(singles[e]._prev_mean)
    obs = rs.standard_normal((B, cfg.obs_shape[0])).astype(np.float32)
    t0s = [True, False, False]
    nzs = [drnn_ref.draw_drnn_noise(cfg, st, step, t0s[e], False) for e in range(B)]
    ab, mb = batched.plan_batch(obs, hidden, step=step, t0=t0s, noise=nzs)
    for e in range(B):
        a1, m1 = singles[e].plan(obs[e], hidden[e:e + 1], step=step, t0=t0s[e], noise=nzs[e])
        np.testing.assert_allclose(ab[e].cpu().numpy(), a1.cpu().numpy(), atol=2e-5, rtol=0, err_msg=f"env {e}")
        np.testing.assert_allclose([mb[e]["external_reward_mean"], mb[e]["current_std"]],
                                   [m1["external_reward_mean"], m1["current_std"]], atol=2e-5, rtol=0)
        np.testing.assert_allclose(batched.planner.prev_mean_view(4, B)[e].cpu().numpy(),
                                   singles[e]._prev_mean.cpu().numpy(), atol=2e-5, rtol=0)
        assert len(batched._memories[e]) == len(singles[e].memory_latents)


def test_captured_plan_replays_equal_eager():
    """One tdmpc_drnn_plan captured on a single stream and replayed twice with new observations, hidden states and
    noise: each replay equals the eager call on the same inputs bitwise."""
    cfg, wseed, iseed, _ = cases()["humanoid"]
    agent, sd = _agent(cfg, wseed, graph=False)
    pl = agent.planner
    H, I, B = 5, cfg.iterations, 1
    pl.set_num_pi(32)
    pl.set_call_state(0.05, [False])
    prm = pl.device_state_params(pl.params(H, I, B, False, False, 0.05))
    rs = np.random.RandomState(9)

    def inputs():
        pl.obs_buf[:B].copy_(torch.from_numpy(rs.standard_normal((B, cfg.obs_shape[0])).astype(np.float32)))
        pl.hidden_buf[:B].copy_(torch.from_numpy(rs.uniform(-1, 1, (B, cfg.hidden_dim)).astype(np.float32)))
        pl.noise_view(H, I, B).copy_(torch.from_numpy(
            rs.standard_normal(tuple(pl.noise_view(H, I, B).shape)).astype(np.float32)))
        pl.u[:B].copy_(torch.from_numpy(rs.uniform(0, 1, B)))

    def outputs():
        torch.cuda.synchronize()
        assert int(pl.status.item()) == 0
        return (pl.action[:B].clone(), pl.metrics[:B].clone(), pl.prev_mean_view(H, B).clone(), pl.z_in[:B].clone())

    inputs()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.graph(g, stream=s):
        pl.launch(prm)
    for _ in range(2):
        inputs()
        pl.launch(prm)
        eager = outputs()
        pl.action.zero_(); pl.metrics.zero_(); pl.prev_mean_flat.zero_(); pl.z_in.zero_()
        g.replay()
        for x, y in zip(eager, outputs()):
            assert torch.equal(x, y)
            assert torch.isfinite(x).all()


def test_stale_pack_raises_through_status_word():
    """A graph captured over a DSSM pack, replayed after the buffer was re-keyed (tdmpc_pack_forget + a pack from other
    tensors), finds another job table: the next plan raises TDMPC_STATUS_PACK_STALE, and a fresh pack recovers."""
    cfg, wseed, iseed, _ = cases()["horizon"]
    agent, sd = _agent(cfg, wseed, graph=False)
    pl = agent.planner
    obs, hidden = case_inputs(cfg, iseed, 1)
    a0, _ = agent.plan(obs[0], hidden, step=10**6, t0=True)
    assert torch.isfinite(a0).all()
    n = len(pl._pack_stage)
    arr = (C.c_void_p * n)(*[t.data_ptr() for t in pl._pack_stage])

    def pack(arr_, stream):
        return pl.L.tdmpc_drnn_pack_weights(C.byref(pl.ddims), arr_, n, C.c_void_p(pl.packed.data_ptr()),
                                            pl.packed.numel() * 4, C.c_void_p(stream))
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.graph(g, stream=s):
        _lib.check(pack(arr, torch.cuda.current_stream().cuda_stream), "captured pack")
    g.replay()
    assert torch.isfinite(agent.plan(obs[0], hidden, step=10**6, t0=True)[0]).all()
    copies = [t.clone() for t in pl._pack_stage]
    arr2 = (C.c_void_p * n)(*[t.data_ptr() for t in copies])
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="captured graph"):
        _lib.check(pack(arr2, stream), "re-keying pack")
    pl.L.tdmpc_pack_forget(C.c_void_p(pl.packed.data_ptr()))
    _lib.check(pack(arr2, stream), "pack after forget")
    assert torch.isfinite(agent.plan(obs[0], hidden, step=10**6, t0=True)[0]).all()
    g.replay()
    with pytest.raises(RuntimeError, match="job table"):
        agent.plan(obs[0], hidden, step=10**6, t0=True)
    pl.L.tdmpc_pack_forget(C.c_void_p(pl.packed.data_ptr()))
    pl._packed_key = None
    a1, _ = agent.plan(obs[0], hidden, step=10**6, t0=True)
    assert torch.isfinite(a1).all()
    torch.cuda.synchronize()
    del copies


def test_reference_checkpoint_loads_and_plans(tmp_path):
    """A reference-format checkpoint (torch.save({'model': sd, 'model_target': sd})) loads with strict keys and plans
    like the agent the weights came from."""
    from tdmpc_amd.drnn import TdMpcDrnn
    cfg, wseed, iseed, _ = cases()["horizon"]
    sd = synthetic_dssm_state_dict(cfg, wseed)
    fp = str(tmp_path / "dssm.pt")
    torch.save({"model": sd, "model_target": sd}, fp)
    a = TdMpcDrnn(cfg)
    a.load(fp)
    a.std = 0.05
    b, _ = _agent(cfg, wseed)
    obs, hidden = case_inputs(cfg, iseed, 1)
    outs = []
    for ag in (a, b):
        torch.manual_seed(3)
        np.random.seed(4)
        outs.append(ag.plan(obs[0], hidden, step=10**6, t0=True)[0])
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    bad = dict(sd)
    bad.pop("_predictor.3.bias")
    torch.save({"model": bad, "model_target": bad}, fp)
    with pytest.raises(RuntimeError, match="_predictor.3.bias"):
        a.load(fp)
