"""iCEM planner: TdICemSimMlp.plan (tdmpc_icem_similarity_mlp.py:160-265).

* The oracle (oracle/icem_ref.py) reproduces the reference planner bit for bit on the CPU over six calls
  (t0 / warm start / horizon growth with the time-shifted elite reuse / eval), tests/golden/icem_humanoid.npz.
* The GPU planner (tdmpc_amd.icem, chain and layered kernels) against the oracle on identical noise; tolerance as in
  tests/test_gpu_plan.py (values 1e-5 + 1e-4 |ref|; action / mean atol 2e-5 while the elite sets agree).
* Coloured-noise generator: restated, unpinned (colorednoise is absent and unpinned); its spectrum is checked.
"""
import os

import numpy as np
import pytest

from parity_util import near_tie, record
import torch

from icem_io import CALLS, icem_cfg
from oracle import icem_ref
from oracle.tdmpc_ref import RefTOLD
from tdmpc_amd.told import synthetic_state_dict

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "icem_humanoid.npz"))


def test_oracle_icem_matches_reference():
    cfg = icem_cfg()
    told = RefTOLD(synthetic_state_dict(cfg, 31, enc_norm=True), cfg)
    st = icem_ref.IcemState(0.05)
    for ci, (step, t0, ev) in enumerate(CALLS):
        torch.manual_seed(100 + ci)
        np.random.seed(200 + ci)
        nz = icem_ref.draw_icem_noise(cfg, st, step, t0, ev)
        tr = {}
        a, m = icem_ref.plan(told, cfg, st, G[f"c{ci}_obs"], nz, eval_mode=ev, step=step, t0=t0, trace=tr)
        vals = torch.cat([v.squeeze(1) for v in tr["value"]]).numpy()
        assert np.array_equal(vals, G[f"c{ci}_values"]), ci
        assert np.array_equal(a.numpy(), G[f"c{ci}_action"]), ci
        assert np.array_equal(np.array([m["external_reward_mean"], m["current_std"]]), G[f"c{ci}_metrics"]), ci
        assert np.array_equal(st.elite_actions.numpy(), G[f"c{ci}_elites"]), ci
        assert np.array_equal(st.prev_mean.numpy(), G[f"c{ci}_prev_mean"]), ci


def test_colored_noise_spectrum():
    """powerlaw_psd_gaussian(beta): unit variance and log-log PSD slope ~ -beta (numpy and device forms)."""
    from tdmpc_amd.colored_noise import powerlaw_psd_gaussian
    rs = np.random.RandomState(0)
    for beta in (1.0, 2.5):
        y = powerlaw_psd_gaussian(beta, (2000, 256), rs)
        assert abs(y.std() - 1.0) < 0.1 if beta < 2 else 0.2
        psd = (np.abs(np.fft.rfft(y, axis=-1)) ** 2).mean(0)[1:64]
        f = np.fft.rfftfreq(256)[1:64]
        slope = np.polyfit(np.log(f), np.log(psd), 1)[0]
        assert abs(slope + beta) < 0.15, (beta, slope)


def _close(a, b, atol=1e-5, rtol=1e-4):
    return np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) <= atol + rtol * np.abs(np.asarray(b, np.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["chain16", "chain32", "layered", "split", "chain_x6", "split_x6", "chain"])
def test_gpu_icem_matches_oracle(path):
    """The golden call sequence on the GPU planner with the oracle's draws: per-iteration values within the fp32
    tolerance; actions, metrics, prev_mean and the kept elites while every iteration's elite set agrees."""
    from tdmpc_amd.icem import TdICEM
    cfg = icem_cfg()
    sd = synthetic_state_dict(cfg, 31, enc_norm=True)
    agent = TdICEM(cfg, path=path)
    agent.model.load_state_dict(sd)
    agent.std = 0.05
    told = RefTOLD(sd, cfg)
    st = icem_ref.IcemState(0.05)
    for ci, (step, t0, ev) in enumerate(CALLS):
        torch.manual_seed(100 + ci)
        np.random.seed(200 + ci)
        nz = icem_ref.draw_icem_noise(cfg, st, step, t0, ev)
        rtr, gtr = {}, {}
        ra, rm = icem_ref.plan(told, cfg, st, G[f"c{ci}_obs"], nz, eval_mode=ev, step=step, t0=t0, trace=rtr)
        ga, gm = agent.plan(G[f"c{ci}_obs"], eval_mode=ev, step=step, t0=t0, noise=nz, trace=gtr)
        same = True
        for i, rv in enumerate(rtr["value"]):
            gv = gtr["value"][i].cpu().numpy()
            rv = rv.squeeze(1).numpy()
            assert gv.shape == rv.shape
            assert _close(gv, rv).all(), (ci, i, np.abs(gv - rv).max())
            K = cfg.num_elites
            eg = set(np.argsort(-gv, kind="stable")[:K]); er = set(np.argsort(-rv, kind="stable")[:K])
            if eg != er:
                assert near_tie(rv, eg, er, K), (ci, i, "elite sets differ away from the cut-off")
                same = False
                break
        record(same, f"icem/{path}/call{ci}")
        if not same:
            break   # near-tie swap: this and the later (warm-started) calls diverge legitimately
        np.testing.assert_allclose(ga.cpu().numpy(), ra.numpy(), atol=2e-5, rtol=0)
        np.testing.assert_allclose(agent._prev_mean.cpu().numpy(), st.prev_mean.numpy(), atol=2e-5, rtol=0)
        np.testing.assert_allclose(agent._elite_actions.cpu().numpy(), st.elite_actions.numpy(), atol=2e-5, rtol=0)
        np.testing.assert_allclose([gm["external_reward_mean"], gm["current_std"]],
                                   [rm["external_reward_mean"], rm["current_std"]], atol=2e-5, rtol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("reuse,extend", [(False, False), (True, False), (True, True)])
def test_gpu_icem_draw_order(reuse, extend):
    """TdICEM's own draws (rng 'reference': batched host coloured noise, one pinned copy, torch draws on the
    device) equal the oracle's reference-order draws from the same torch / numpy seeds, element for element."""
    from tdmpc_amd.config import linear_schedule
    from tdmpc_amd.icem import TdICEM
    cfg = icem_cfg()
    agent = TdICEM(cfg)
    st = icem_ref.IcemState(0.05)
    step = 17000 if extend else 10**6
    st.plan_horizon = 3 if extend else cfg.horizon
    if reuse:
        st.elite_actions = torch.zeros(st.plan_horizon, cfg.num_elites, cfg.action_dim)
    H, ext = icem_ref.next_horizon(cfg, st, step, True)
    assert ext == extend
    cts = agent.counts(linear_schedule(cfg.regularization_schedule, step), reuse)
    off = agent._layout(H, cts, reuse)
    S = off["total"]
    for ev in (False, True):
        torch.manual_seed(7)
        np.random.seed(8)
        nz = icem_ref.draw_icem_noise(cfg, st, step, True, ev, device="cuda")
        after_ref = (torch.randn(4, device="cuda"), np.random.random_sample())
        agent.planner.noise_flat.zero_()
        agent._load(0, H, cts, off, reuse, nz)
        want = agent.planner.noise_flat[:S].clone()
        torch.manual_seed(7)
        np.random.seed(8)
        agent.planner.noise_flat.zero_()
        u = agent._draw(0, H, cts, off, reuse, ev)
        assert u == nz.u
        assert torch.equal(agent.planner.noise_flat[:S], want)
        # both generators are left where the reference's draws leave them
        assert torch.equal(torch.randn(4, device="cuda"), after_ref[0])
        assert np.random.random_sample() == after_ref[1]


@pytest.mark.gpu
def test_gpu_icem_device_rng():
    """rng 'device' (coloured noise and the pick's uniform drawn on the device): seeded runs repeat exactly and
    the plan is well formed (the distribution is the reference's; the numbers are not numpy's)."""
    from tdmpc_amd.icem import TdICEM
    cfg = icem_cfg()
    sd = synthetic_state_dict(cfg, 31, enc_norm=True)
    outs = []
    for _ in range(2):
        agent = TdICEM(cfg, rng="device")
        agent.model.load_state_dict(sd)
        agent.std = 0.05
        torch.manual_seed(3)
        acts = [agent.plan(G[f"c{ci}_obs"], eval_mode=ev, step=step, t0=t0)[0].cpu()
                for ci, (step, t0, ev) in enumerate(CALLS)]
        outs.append(torch.stack(acts))
    assert torch.equal(outs[0], outs[1])
    assert torch.isfinite(outs[0]).all()
    ev_calls = [ci for ci, (_, _, ev) in enumerate(CALLS) if ev]
    assert ev_calls and outs[0][ev_calls].abs().max() <= 1   # no exploration noise: an elite's action


def test_batched_colored_noise_spectrum():
    """BatchedColoredNoise (the fused-RNG form: matmul irfft, per-row spectrum factors) has the generator's
    statistics: unit variance, log-log PSD slope ~ -beta, per spec of a mixed batch."""
    from tdmpc_amd.colored_noise import BatchedColoredNoise
    torch.manual_seed(0)
    L, A = 256, 4
    gen = BatchedColoredNoise([(1.0, 500), (2.5, 500)], A, L, L, "cpu")
    y = gen.draw().double().numpy()
    for k, beta in enumerate((1.0, 2.5)):
        yk = y[k * 500 * A:(k + 1) * 500 * A]
        assert abs(yk.std() - 1.0) < (0.1 if beta < 2 else 0.2)
        psd = (np.abs(np.fft.rfft(yk, axis=-1)) ** 2).mean(0)[1:64]
        f = np.fft.rfftfreq(L)[1:64]
        slope = np.polyfit(np.log(f), np.log(psd), 1)[0]
        assert abs(slope + beta) < 0.15, (beta, slope)


def test_device_rng_positions_cover_colored_slots():
    """The fused-RNG stream plan writes every coloured third and reuse-tail slot exactly once and nothing else
    (checked against the layout the kernels read, on the CPU)."""
    from tdmpc_amd.icem import TdICEM, _thirds
    cfg = icem_cfg()
    cfg.device = "cpu"
    agent = TdICEM(cfg, rng="device")
    A, H = cfg.action_dim, cfg.horizon
    cts = agent.counts(0.5, True)
    off = agent._layout(H, cts, True)
    want = set()
    for i, (n, p, e) in enumerate(cts):
        n0, n1, n2 = _thirds(n)
        for t in range(H):
            for r in range(n0, n):
                want.update(off["samp"][i] + t * n * A + r * A + a for a in range(A))
    if cfg.noise_beta > 0:
        ne = cts[0][2]
        want.update(off["reuse"] + j for j in range(H * ne * A))
    got = np.concatenate([pos.numpy().reshape(-1) for _, pos in agent._device_plan(H, cts, off, True)])
    assert len(got) == len(set(got.tolist())) == len(want)
    assert set(got.tolist()) == want
    # B envs: env e's slots shifted by e streams, each exactly once
    got3 = np.concatenate([pos.numpy().reshape(-1) for _, pos in agent._device_plan(H, cts, off, True, B=3)])
    want3 = {w + e * off["total"] for e in range(3) for w in want}
    assert len(got3) == len(set(got3.tolist())) == len(want3) and set(got3.tolist()) == want3


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["chain16", "layered", "split", "chain_x6"])
def test_gpu_icem_batched_equals_single(path):
    """TdICEM.plan_batch over 3 envs (each its own observation and noise stream) equals 3 single-env plans on the
    same draws, bitwise, over a cold call and a warm call with elite reuse (forced kernel path: the same kernels
    at both widths)."""
    from tdmpc_amd.icem import TdICEM
    cfg = icem_cfg()
    sd = synthetic_state_dict(cfg, 41, enc_norm=True)
    B, step = 3, 10**6
    rs = np.random.RandomState(5)
    obs = rs.standard_normal((B, cfg.obs_shape[0])).astype(np.float32)
    st = icem_ref.IcemState(0.05)
    st.plan_horizon = icem_ref.next_horizon(cfg, st, step, True)[0]
    torch.manual_seed(12)
    np.random.seed(13)
    calls = []
    for t0 in (True, False):
        calls.append((t0, [icem_ref.draw_icem_noise(cfg, st, step, t0, False, device="cuda") for _ in range(B)]))
        st.elite_actions = torch.zeros(st.plan_horizon, cfg.num_elites, cfg.action_dim)
    batched = TdICEM(cfg, max_batch=B, path=path)
    singles = [TdICEM(cfg, path=path) for _ in range(B)]
    for ag in [batched] + singles:
        ag.model.load_state_dict(sd)
        ag.std = 0.05
    for t0, nzs in calls:
        a, _ = batched._plan_envs(torch.from_numpy(obs), False, step, t0, nzs, None)
        for e in range(B):
            a1, _ = singles[e].plan(obs[e], step=step, t0=t0, noise=nzs[e])
            assert torch.equal(a[e], a1), (t0, e)
        assert torch.equal(batched.elites[:B, :batched._elite_H], torch.stack([s.elites[0, :s._elite_H] for s in singles]))


@pytest.mark.gpu
def test_gpu_icem_batch32_matches_oracle():
    """The bench's vectorised iCEM leg (`icem.batch32`: humanoid-run, N = 512 shrinking by 1.25 per iteration, H = 5,
    6 iterations, K = 64 with 16 elites reused, 32 envs in one TdICEM.plan_batch call, the auto kernel path) against
    the oracle (tdmpc_icem_similarity_mlp.py:160-265), every env on its own oracle planner and draws: a cold call,
    then a warm call with the time-shifted elite reuse. Per env and iteration the values within 1e-5 + 1e-4 |ref|
    while the elite sets agree; an env whose elite set differs only by a near-tie swap at the cut-off leaves the
    comparison (its later iterations and calls diverge legitimately). At least B - 2 envs must be compared in full on
    both calls: action, prev_mean, kept elites and metrics."""
    from tdmpc_amd.config import bench_cfg
    from tdmpc_amd.icem import TdICEM
    cfg = bench_cfg("humanoid-run")
    B, step, K = 32, 10**6, cfg.num_elites
    sd = synthetic_state_dict(cfg, 0, enc_norm=True)
    agent = TdICEM(cfg, max_batch=B)
    agent.model.load_state_dict(sd)
    agent.std = 0.05
    told = RefTOLD(sd, cfg)
    obs = np.random.RandomState(0).standard_normal((B, cfg.obs_shape[0])).astype(np.float32)
    sts = [icem_ref.IcemState(0.05) for _ in range(B)]
    torch.manual_seed(12)
    np.random.seed(13)
    live = [True] * B
    for t0 in (True, False):
        nzs = [icem_ref.draw_icem_noise(cfg, sts[e], step, t0, False) for e in range(B)]
        gtr = {}
        ga, gm = agent._plan_envs(torch.from_numpy(obs), False, step, t0, nzs, gtr)
        ga, gm = ga.cpu().numpy(), gm.cpu().numpy()
        vall = gtr["value_all"].cpu().numpy()
        H = agent.plan_horizon
        pm = agent.planner.prev_mean_flat[:B * H * cfg.action_dim].view(B, H, -1).cpu().numpy()
        el = agent.elites[:B, :agent._elite_H].cpu().numpy()
        for e in range(B):
            rtr = {}
            ra, rm = icem_ref.plan(told, cfg, sts[e], obs[e], nzs[e], eval_mode=False, step=step, t0=t0, trace=rtr)
            if not live[e]:
                continue
            for i, rv in enumerate(rtr["value"]):
                rv = rv.squeeze(1).numpy()
                gv = vall[e, i, :rv.shape[0]]
                assert _close(gv, rv).all(), (t0, e, i, np.abs(gv - rv).max())
                eg = set(np.argsort(-gv, kind="stable")[:K]); er = set(np.argsort(-rv, kind="stable")[:K])
                if eg != er:
                    assert near_tie(rv, eg, er, K), (t0, e, i, "elite sets differ away from the cut-off")
                    live[e] = False
                    break
            record(live[e], f"icem/batch32/t0={t0}/env{e}")
            if not live[e]:
                continue
            np.testing.assert_allclose(ga[e], ra.numpy(), atol=2e-5, rtol=0, err_msg=f"t0={t0} env {e}")
            np.testing.assert_allclose(pm[e], sts[e].prev_mean.numpy(), atol=2e-5, rtol=0)
            np.testing.assert_allclose(el[e], sts[e].elite_actions.numpy(), atol=2e-5, rtol=0)
            np.testing.assert_allclose(gm[e], [rm["external_reward_mean"], rm["current_std"]], atol=2e-5, rtol=1e-4)
        assert sum(live) >= B - 2, (t0, sum(live))
