"""GPU: the recurrent-latent iCEM planner (tdmpc_drnn_plan_icem / tdmpc_drnn_colored_noise, tdmpc_amd/drnn_icem.py)
against the CPU restatement tests/drnn_icem_ref.py, which tests/test_drnn_icem_cpu.py pins to the reference bit for bit.

Tolerances are the project's standing ones (tests/test_gpu_plan.py's header): values within 1e-5 + 1e-4 |ref|
(parity_util.close); actions, hidden states, prev_mean, kept elites and metrics within atol 2e-5. The recorded inputs
keep the K-th and (K+1)-th values 1e-3 (1 + |cut|) apart (the generator's tie guard), so the elite sets must be equal
outright: there is no near-tie escape here, and every comparison is recorded as run to the end.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import drnn_icem_ref as ref
import drnn_ref
from drnn_icem_io import case_inputs, cases, load
from parity_util import close, elites, record
from tdmpc_amd import _lib
from tdmpc_amd.colored_noise import irfft_matrices, spectrum_rows
from tdmpc_amd.dssm import synthetic_dssm_state_dict

pytestmark = pytest.mark.gpu
ATOL = dict(atol=2e-5, rtol=0)


def _agent(cfg, wseed, max_batch=1, **kw):
    from tdmpc_amd.drnn_icem import TdIcemDrnn
    agent = TdIcemDrnn(cfg, max_batch=max_batch, **kw)
    sd = synthetic_dssm_state_dict(cfg, wseed)
    agent.model.load_state_dict(sd)
    agent.std = 0.05
    agent.planner.pack(agent.model)
    return agent, sd


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("name", ["humanoid", "cheetah"])
def test_plan_matches_restatement_on_recorded_calls(name):
    """The recorded call sequences through TdIcemDrnn.plan with the restatement's draws (which are the reference's):
    an episode start, warm calls with the time-shifted elite reuse, an eval call (humanoid, coloured noise); a second
    episode start with elites and a grown horizon (cheetah, white noise)."""
    cfg, wseed, iseed, base, calls = cases()[name]
    G = load(name)
    agent, sd = _agent(cfg, wseed, graph=False)
    model = drnn_ref.RefDSSM(sd, cfg)
    st = ref.IcemDrnnState(0.05)
    obs, hidden = case_inputs(cfg, iseed, len(calls))
    K = cfg.num_elites
    for ci, (step, t0, ev) in enumerate(calls):
        torch.manual_seed(base + ci)
        np.random.seed(base + 100 + ci)
        nz = ref.draw_noise(cfg, st, step, t0, ev)
        rtr, gtr = {}, {}
        ra, rh, rm = ref.plan(model, cfg, st, obs[ci], hidden, nz, eval_mode=ev, step=step, t0=t0, trace=rtr)
        # the reference's own recorded action (bit for bit where it was recorded: tests/test_drnn_icem_cpu.py; another
        # host's float32 kernels may round differently)
        np.testing.assert_allclose(ra.numpy(), G[f"c{ci}_action"], err_msg=f"call {ci} fixture", **ATOL)
        np.testing.assert_allclose(rh.numpy(), G[f"c{ci}_hidden"], err_msg=f"call {ci} fixture", **ATOL)
        ga, gh, gm = agent.plan(obs[ci], hidden, eval_mode=ev, step=step, t0=t0, noise=nz, trace=gtr)
        assert agent.plan_horizon == st.plan_horizon == int(G[f"c{ci}_horizon"])
        assert [n + e + p for n, p, e in gtr["counts"]] == G[f"c{ci}_nvals"].tolist()
        for i, rv in enumerate(rtr["value"]):
            rv = rv.squeeze(1).numpy()
            gv = _np(gtr["value"][i][0])
            assert gv.shape == rv.shape
            print(f"{name} call {ci} iteration {i}: max |dG| {np.abs(gv - rv).max():.3e}")
            assert close(gv, rv).all(), (ci, i, np.abs(gv - rv).max())
            assert elites(gv, K) == elites(rv, K), (ci, i, "elite sets differ")
        record(True, f"drnn_icem/{name}/call{ci}")
        for what, g, r in (("action", ga, ra), ("hidden", gh, rh), ("prev_mean", agent._prev_mean, st.prev_mean),
                           ("elites", agent._elite_actions, st.elite_actions)):
            print(f"{name} call {ci} {what}: max |d| {np.abs(_np(g) - r.numpy()).max():.3e}")
            np.testing.assert_allclose(_np(g), r.numpy(), err_msg=f"call {ci} {what}", **ATOL)
        assert gh.shape == (1, cfg.hidden_dim) and ga.shape == (cfg.action_dim,)
        assert close(_np(gtr["z_in"]), rtr["z_in"].numpy()).all()
        np.testing.assert_allclose([gm["external_reward_mean"], gm["current_std"]],
                                   [rm["external_reward_mean"], rm["current_std"]], **ATOL)
        assert sorted(gm) == ["current_std", "external_reward_mean"]


def test_returned_hidden_is_next_of_the_returned_action():
    """hidden_out = DSSM.next(z0, action, hidden)[1] with the returned, noised action (:267)."""
    cfg, wseed, iseed, base, calls = cases()["humanoid"]
    agent, sd = _agent(cfg, wseed, graph=False)
    obs, hidden = case_inputs(cfg, iseed, 2)
    pl = agent.planner
    torch.manual_seed(5)
    np.random.seed(6)
    for ci, t0 in enumerate((True, False)):
        a, h, _ = agent.plan(obs[ci], hidden, step=10**6, t0=t0)
        z = pl.z_in[:1].clone()
        _, want, _ = pl.next(z, a[None], torch.from_numpy(hidden))
        assert torch.isfinite(h).all() and float((h - torch.from_numpy(hidden).cuda()).abs().max()) > 1e-3
        assert close(_np(h), _np(want)).all(), np.abs(_np(h) - _np(want)).max()


def test_plan_batch_equals_single_env_plans():
    """Three envs with their own observations and hidden states in one plan_batch call agree with three single-env
    agents on the same explicit draws: an episode start, then a warm call with elite reuse (55- and 44-row candidate
    blocks that straddle the envs' 32-row tiles)."""
    cfg, wseed, iseed, _, _ = cases()["humanoid"]
    B, step = 3, 10**6
    batched, sd = _agent(cfg, wseed, max_batch=B, graph=False)
    singles = [_agent(cfg, wseed, graph=False)[0] for _ in range(B)]
    rs = np.random.RandomState(8)
    hidden = rs.uniform(-1, 1, (B, cfg.hidden_dim)).astype(np.float32)
    st = ref.IcemDrnnState(0.05)
    st.plan_horizon = 5
    torch.manual_seed(21)
    np.random.seed(22)
    for t0 in (True, False):
        obs = rs.standard_normal((B, cfg.obs_shape[0])).astype(np.float32)
        nzs = [ref.draw_noise(cfg, st, step, t0, False) for _ in range(B)]
        ab, hb, mb = batched.plan_batch(obs, hidden, step=step, t0=t0, noise=nzs)
        assert ab.shape == (B, cfg.action_dim) and hb.shape == (B, cfg.hidden_dim)
        for e in range(B):
            a1, h1, m1 = singles[e].plan(obs[e], hidden[e:e + 1], step=step, t0=t0, noise=nzs[e])
            np.testing.assert_allclose(_np(ab[e]), _np(a1), err_msg=f"env {e}", **ATOL)
            np.testing.assert_allclose(_np(hb[e]), _np(h1[0]), err_msg=f"env {e}", **ATOL)
            np.testing.assert_allclose([mb[e]["external_reward_mean"], mb[e]["current_std"]],
                                       [m1["external_reward_mean"], m1["current_std"]], **ATOL)
            np.testing.assert_allclose(_np(batched.planner.prev_mean_view(5, B)[e]), _np(singles[e]._prev_mean), **ATOL)
            np.testing.assert_allclose(_np(batched.elites[e, :5]), _np(singles[e]._elite_actions), **ATOL)
        assert float((ab[0] - ab[1]).abs().max()) > 1e-3   # the envs do differ
        st.elite_actions = torch.zeros(5, cfg.num_elites, cfg.action_dim)   # (the next call's draws include the reuse tail)


@pytest.mark.parametrize("name", ["humanoid", "cheetah"])
def test_reference_rng_draws_equal_restatement(name):
    """rng='reference' consumes exactly the restatement's torch / numpy draws -- coloured sequences from numpy
    (humanoid), white ones from torch (cheetah): an episode start and a warm eval call with the reuse tail, through the
    graph cache; both generators end where the restatement leaves them."""
    cfg, wseed, iseed, _, calls = cases()[name]
    agent, sd = _agent(cfg, wseed)
    step = calls[0][0]
    st = ref.IcemDrnnState(0.05)
    obs, hidden = case_inputs(cfg, iseed, 2)
    pl = agent.planner
    for ci, (t0, ev) in enumerate([(True, False), (False, True)]):
        torch.manual_seed(50 + ci)
        np.random.seed(60 + ci)
        nz = ref.draw_noise(cfg, st, step, t0, ev, device="cuda")
        after = (torch.randn(4, device="cuda"), np.random.random_sample())
        has = st.elite_actions is not None
        H = ref.call_horizon(cfg, st, step, t0)
        torch.manual_seed(50 + ci)
        np.random.seed(60 + ci)
        a, h, _ = agent.plan(obs[ci], hidden, eval_mode=ev, step=step, t0=t0)
        assert torch.isfinite(a).all() and torch.isfinite(h).all() and agent.plan_horizon == H
        cts = agent.counts(agent.mixture_coef, has, t0)
        reuse = ref.reuses(cfg, st, t0)
        assert reuse == (ci == 1)
        off = agent.layout(H, cts, reuse)
        got = pl.noise_flat[:off["total"]].clone()
        u = float(pl.u[0].cpu())
        pl.noise_flat.zero_()
        assert agent._load(0, H, cts, off, reuse, nz) == nz.u == u
        n = off["act"] + (0 if ev else cfg.action_dim)
        assert torch.equal(got[:n], pl.noise_flat[:n])
        assert torch.equal(torch.randn(4, device="cuda"), after[0])
        assert np.random.random_sample() == after[1]
        st.plan_horizon = H
        st.elite_actions = torch.zeros(H, cfg.num_elites, cfg.action_dim)


def test_device_rng_graph_replay_equals_eager():
    """rng='device': the draws (two normal_, the coloured-noise kernel, the uniforms) and the plan captured in one
    graph. After identical seeding the first call (capture + replay), a second call on the same key (a replay) and
    warm calls with reuse equal the eager agent's bit for bit: noise stream, action, hidden, metrics, state."""
    cfg, wseed, iseed, _, _ = cases()["humanoid"]
    ag, _ = _agent(cfg, wseed, rng="device", graph=True)
    ae, _ = _agent(cfg, wseed, rng="device", graph=False)
    obs, hidden = case_inputs(cfg, iseed, 4)
    for ci, t0 in enumerate((True, True, False, False)):
        outs = []
        for agent in (ag, ae):
            torch.manual_seed(90 + ci)
            a, h, m = agent.plan(obs[ci], hidden, step=10**6, t0=t0)
            torch.cuda.synchronize()
            pl = agent.planner
            cts = agent.counts(agent.mixture_coef, ci > 0, t0)
            S = agent.layout(5, cts, not t0)["total"]
            outs.append((pl.noise_flat[:S].clone(), a, h, agent._prev_mean.clone(), agent._elite_actions.clone(),
                         torch.tensor([m["external_reward_mean"], m["current_std"]]), pl.u[:1].clone()))
        for k, (x, y) in enumerate(zip(*outs)):
            assert torch.isfinite(x).all()
            assert torch.equal(x, y), (ci, k, float((x - y).abs().max()))
        # the coloured blocks are not the white draw they replaced: unit variance, strongly correlated along t
        noise = outs[0][0]
        off = ag.layout(5, cts, not t0)
        n0, A = cts[0][0], cfg.action_dim
        blk = noise[off["samp"][0]:off["samp"][0] + 5 * n0 * A].view(5, n0 * A)
        assert 0.7 < float(blk.std()) < 1.3
        assert float((blk[0] * blk[1]).mean()) > 0.3
    assert len(ag.planner._graphs) == 2 and not ae.planner._graphs


def _noise_case(L, beta, A, seed):
    """Two envs; three jobs per env: a column range of a wider block, a whole multi-workgroup block, a reuse tail on a
    second spectrum. Returns the params, the normals, the stream and the float64 expectation."""
    from tdmpc_amd.drnn_icem import colored_noise_params
    F = L // 2 + 1
    beta2 = 1.0 if beta != 1.0 else 2.5
    shapes = [(0, 20, 37, 5), (0, 70, 70, 0), (1, 4, 4, 0)]   # (spectrum, n, rows, c0)
    gaps = [7, 3, 11, 5]
    jobs, dst, src = [], gaps[0], 0
    for k, (sp, n, rows, c0) in enumerate(shapes):
        jobs.append((sp, n, rows, c0, dst, src))
        dst += L * rows * A + gaps[k + 1]
        src += 2 * F * n * A
    S, Z, B = dst, src + 9, 2
    prm = colored_noise_params(L, A, B, S, Z, jobs, [beta, beta2])
    rs = np.random.RandomState(seed)
    z = rs.standard_normal(B * Z).astype(np.float32)
    SENT = 12345.0
    want = np.full(B * S, SENT, np.float64)
    Cm = np.concatenate(irfft_matrices(L))                        # [2F, L]
    for e in range(B):
        for sp, n, rows, c0, d, s in jobs:
            re, im, inv = spectrum_rows([beta, beta2][sp], L)
            fac = np.concatenate([re, im]) * inv                  # [2F]
            zz = z[e * Z + s:e * Z + s + 2 * F * n * A].astype(np.float64).reshape(2 * F, n * A)
            y = (zz * fac[:, None]).T @ Cm                        # [n A, L]
            blk = want[e * S + d:e * S + d + L * rows * A].reshape(L, rows, A)
            blk[:, c0:c0 + n, :] = y.reshape(n, A, L).transpose(2, 0, 1)
    return prm, z, S, SENT, want


@pytest.mark.parametrize("A", [1, 6, 21])
@pytest.mark.parametrize("beta", [0.0, 1.0, 2.5])
@pytest.mark.parametrize("L", [2, 3, 5, 8, 16])
def test_colored_noise_kernel_matches_float64(L, beta, A):
    """drnn_colored_noise_kernel against spectrum_rows x irfft_matrices in float64: even lengths with the Nyquist bin,
    odd ones, the longest; every stream float outside the jobs' blocks keeps its sentinel."""
    from tdmpc_amd.drnn_icem import colored_noise
    prm, z, S, SENT, want = _noise_case(L, beta, A, 100 * L + A)
    zd = torch.from_numpy(z).cuda()
    noise = torch.full((2 * S + 64,), SENT, device="cuda")
    colored_noise(_lib.lib(), prm, zd, noise[:2 * S])
    torch.cuda.synchronize()
    got = noise.cpu().numpy().astype(np.float64)
    assert (got[2 * S:] == SENT).all(), "wrote past the streams"
    got = got[:2 * S]
    outside = want == SENT
    assert (got[outside] == SENT).all(), "wrote outside the jobs' blocks"
    assert (~outside).sum() == 2 * L * (20 + 70 + 4) * A
    err = np.abs(got[~outside] - want[~outside]).max()
    print(f"L {L} beta {beta} A {A}: max |d| {err:.3e}")
    assert close(got[~outside], want[~outside]).all(), err
    if beta == 0.0 and L == 16:
        assert 0.8 < got[~outside].std() < 1.2   # white: unit variance


def test_stale_pack_raises_through_status_word():
    """test_gpu_drnn.py's scenario on this agent: a graph captured over a DSSM pack, replayed after the buffer was
    re-keyed, finds another job table: the next plan raises TDMPC_STATUS_PACK_STALE, and a fresh pack recovers."""
    cfg, wseed, iseed, _, _ = cases()["cheetah"]
    agent, sd = _agent(cfg, wseed, graph=False)
    pl = agent.planner
    obs, hidden = case_inputs(cfg, iseed, 1)

    def plan():
        return agent.plan(obs[0], hidden, step=10**6, t0=True)[0]
    assert torch.isfinite(plan()).all()
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
    assert torch.isfinite(plan()).all()
    copies = [t.clone() for t in pl._pack_stage]
    arr2 = (C.c_void_p * n)(*[t.data_ptr() for t in copies])
    stream = torch.cuda.current_stream().cuda_stream
    with pytest.raises(RuntimeError, match="captured graph"):
        _lib.check(pack(arr2, stream), "re-keying pack")
    pl.L.tdmpc_pack_forget(C.c_void_p(pl.packed.data_ptr()))
    _lib.check(pack(arr2, stream), "pack after forget")
    assert torch.isfinite(plan()).all()
    g.replay()
    with pytest.raises(RuntimeError, match="job table"):
        plan()
    pl.L.tdmpc_pack_forget(C.c_void_p(pl.packed.data_ptr()))
    pl._packed_key = None
    assert torch.isfinite(plan()).all()
    torch.cuda.synchronize()
    del copies
