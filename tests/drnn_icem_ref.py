"""Test infrastructure only: CPU restatement of the reference's recurrent-latent iCEM planner with explicit noise.

Restates `TdICemSimDssm.plan` / `estimate_value` / `sample_action_sequence`
(src/algorithm/tdmpc_icem_similarity_drnn.py:124-146, :169-272) on tests/drnn_ref.py's `RefDSSM`, every random number
taken from an `IcemNoise` (oracle/icem_ref.py's container: eps_pi [H, P0, A], samp[i] [H, N_i, A], reuse [H, E, A],
term[i] [T_i, A], u, eps_act [A]). `draw_noise` reproduces the reference's draw order on torch's and numpy's global
generators: the pre-rollout's H TruncatedNormal draws; per iteration the sample noise (coloured through
tdmpc_amd.colored_noise on numpy's generator when cfg.noise_beta > 0, torch.randn otherwise), in the first iteration
of a call that reuses elites their fresh sequence, the terminal policy draw; np.random.choice's uniform; the action
noise. `dtype`: torch.float32 restates the reference bit for bit (tests/test_drnn_icem_cpu.py against the recorded
fixtures); torch.float64 is the same code as an accuracy yardstick.

Where it differs from the MLP agent's restatement (oracle/icem_ref.py): the hidden state rides along, reused elites
enter only when `not t0` (:210, :224), all samples come from `sample_action_sequence` with sequence length
plan_horizon (:135-146), and plan returns the GRU state after DSSM.next(z, a, hidden) (:267).
"""
from __future__ import annotations

import numpy as np
import torch

from drnn_ref import RefDSSM
from oracle.icem_ref import IcemNoise
from oracle.tdmpc_ref import choice_index, linear_schedule


class IcemDrnnState:
    """What the reference agent keeps on `self`: std, plan_horizon, _prev_mean, _elite_actions."""

    def __init__(self, std):
        self.std = std
        self.plan_horizon = 1
        self.prev_mean = None
        self.elite_actions = None


def call_horizon(cfg, state, step, t0):
    """:179-182 (no state change)."""
    horizon = int(min(cfg.horizon, linear_schedule(cfg.horizon_schedule, step)))
    return horizon if (horizon != state.plan_horizon and t0) else state.plan_horizon


def counts(cfg, mixture, has_elites, t0):
    """Per-iteration (N_i, P_i, E_i) of the reference loop (:205-215)."""
    out, n = [], cfg.num_samples
    for i in range(cfg.iterations):
        if i > 0:
            n = max(2 * cfg.num_elites, int(n / cfg.factor_decrease_num))
        p = int(mixture * n)
        e = int(cfg.fraction_elites_reused * cfg.num_elites) if (
            cfg.fraction_elites_reused > 0 and (has_elites or i > 0) and not t0) else 0
        out.append((n, p, e))
    return out


def reuses(cfg, state, t0):
    """Whether the first iteration takes the previous plan's elites (:224)."""
    return bool(cfg.shift_elites_over_time and state.elite_actions is not None and not t0)


def layout(cfg, H, cts, reuse):
    """The per-env noise stream the draws fill in order (floats)."""
    A = cfg.action_dim
    off = {"pi": 0, "samp": [], "term": [], "reuse": 0}
    o = H * cts[0][1] * A
    for i, (n, p, e) in enumerate(cts):
        off["samp"].append(o)
        o += H * n * A
        if i == 0 and reuse:
            off["reuse"] = o
            o += H * e * A
        off["term"].append(o)
        o += (n + e + p) * A
    off["act"] = o
    off["total"] = o + A
    return off


def draw_noise(cfg, state, step, t0, eval_mode, device="cpu") -> IcemNoise:
    """The reference's draws for this call from torch's / numpy's global generators, in its order."""
    from tdmpc_amd.colored_noise import powerlaw_psd_gaussian
    H = call_horizon(cfg, state, step, t0)
    A = cfg.action_dim
    mixture = linear_schedule(cfg.regularization_schedule, step)
    cts = counts(cfg, mixture, state.elite_actions is not None, t0)
    P0 = cts[0][1]
    nz = IcemNoise(eps_pi=torch.stack([torch.empty(P0, A, device=device).normal_() for _ in range(H)]))

    def seq(n):   # sample_action_sequence's noise (:136-144)
        if cfg.noise_beta > 0.:
            y = powerlaw_psd_gaussian(cfg.noise_beta, (n, A, H))
            return torch.from_numpy(y).float().to(device).permute(2, 0, 1)
        return torch.randn(H, n, A, device=device)

    for i, (n, p, e) in enumerate(cts):
        nz.samp.append(seq(n))
        if i == 0 and reuses(cfg, state, t0):
            nz.reuse = seq(int(cfg.fraction_elites_reused * cfg.num_elites))
        nz.term.append(torch.empty(n + e + p, A, device=device).normal_())
    nz.u = float(np.random.random_sample())
    if not eval_mode:
        nz.eps_act = torch.randn(A, device=device)
    return nz


@torch.no_grad()
def estimate_value(model: RefDSSM, cfg, z, actions, hidden, horizon, eps_term):
    """:124-133."""
    G, discount = 0, 1
    for t in range(horizon):
        z, hidden, reward = model.next(z, actions[t], hidden)
        G += discount * reward
        discount *= cfg.discount
    G += discount * torch.min(*model.Q(z, model.pi(z, cfg.min_std, eps_term)))
    return G.nan_to_num_(0), float(reward.mean().item())


@torch.no_grad()
def plan(model: RefDSSM, cfg, state: IcemDrnnState, obs, hidden, noise: IcemNoise, eval_mode=False, step=None,
         t0=True, trace=None):
    """:169-272 with explicit noise. hidden: [1, Hd]. Returns (action [A], hidden [1, Hd], metrics)."""
    dt = model.dtype
    metrics = {"external_reward_mean": 0.0, "current_std": 0.0}
    extend = False
    horizon = int(min(cfg.horizon, linear_schedule(cfg.horizon_schedule, step)))
    if horizon != state.plan_horizon and t0:
        state.plan_horizon, extend = horizon, True
    H = state.plan_horizon
    mixture = linear_schedule(cfg.regularization_schedule, step)
    A, K = cfg.action_dim, cfg.num_elites
    mean = torch.zeros(H, A, dtype=dt)
    std = 0.5 * torch.ones(H, A, dtype=dt)
    if not t0 and state.prev_mean is not None:
        mean[:-1] = state.prev_mean[1:]
        mean[-1] = state.prev_mean[-1]
    num_samples = cfg.num_samples
    num_pi = int(mixture * num_samples)
    assert num_pi > 0
    obs = torch.tensor(np.asarray(obs), dtype=dt).unsqueeze(0)
    hidden = torch.as_tensor(hidden).to(dt)
    z = model.h(obs)
    pi_actions = torch.empty(H, num_pi, A, dtype=dt)
    zs_pi = z.repeat(num_pi, 1)
    hidden_pi = hidden.repeat(num_pi, 1)
    for t in range(H):
        pi_actions[t] = model.pi(zs_pi, cfg.min_std, noise.eps_pi[t])
        zs_pi, hidden_pi, _ = model.next(zs_pi, pi_actions[t], hidden_pi)
    has = state.elite_actions is not None
    for i in range(cfg.iterations):
        if i > 0:
            num_samples = max(2 * K, int(num_samples / cfg.factor_decrease_num))
            num_pi = int(mixture * num_samples)
            assert num_pi > 0
        if cfg.fraction_elites_reused > 0 and (has or i > 0) and not t0:
            num_elite = int(cfg.fraction_elites_reused * K)
        else:
            num_elite = 0
        num_trajs = num_samples + num_pi + num_elite
        zs_plan = z.repeat(num_trajs, 1)
        hidden_plan = hidden.repeat(num_trajs, 1)
        sampled = torch.clamp(mean.unsqueeze(1) + std.unsqueeze(1) * noise.samp[i].to(dt), -1, 1)
        if i == cfg.iterations - 1:
            sampled[:, 0] = mean
        if i == 0 and cfg.shift_elites_over_time and has and not t0:
            ne = int(cfg.fraction_elites_reused * K)
            reused = state.elite_actions[1:, :ne]
            last = torch.clamp(mean.unsqueeze(1) + std.unsqueeze(1) * noise.reuse.to(dt), -1, 1)
            reused = torch.cat([reused, last[-2:] if extend else last[-1:]], dim=0)
        if i > 0 and cfg.keep_previous_elites:
            reused = state.elite_actions[:, :num_elite]
        if num_elite > 0:
            actions = torch.cat([sampled, reused, pi_actions[:, :num_pi]], dim=1)
        else:
            actions = torch.cat([sampled, pi_actions[:, :num_pi]], dim=1)
        value, reward_mean = estimate_value(model, cfg, zs_plan, actions, hidden_plan, H, noise.term[i])
        elite_idxs = torch.topk(value.squeeze(1), K, dim=0).indices
        elite_value, elite_actions = value[elite_idxs], actions[:, elite_idxs]
        state.elite_actions = elite_actions
        max_value = elite_value.max(0)[0]
        score = torch.exp(cfg.temperature * (elite_value - max_value))
        score /= score.sum(0)
        _mean = torch.sum(score.unsqueeze(0) * elite_actions, dim=1) / (score.sum(0) + 1e-9)
        _std = torch.sqrt(torch.sum(score.unsqueeze(0) * (elite_actions - _mean.unsqueeze(1)) ** 2, dim=1) /
                          (score.sum(0) + 1e-9))
        _std = _std.clamp_(state.std, 2)
        mean, std = cfg.momentum * mean + (1 - cfg.momentum) * _mean, _std
        if trace is not None:
            trace.setdefault("value", []).append(value.clone())
            trace.setdefault("mean", []).append(mean.clone())
            trace.setdefault("std", []).append(std.clone())
    score = score.squeeze(1).cpu().numpy()
    j = choice_index(score, noise.u)
    state.prev_mean = mean
    # `actions = elite_actions[:, j]`, `a = actions[0]`: integer-indexed views of the stored elites, so the in-place
    # action noise lands in _elite_actions[0, j] and rides into the next plan
    a = elite_actions[:, j][0]
    s0 = _std[0]
    if not eval_mode:
        a += s0 * noise.eps_act.to(dt)
    z, hidden, _ = model.next(z[0:1], a.unsqueeze(0), hidden)
    if trace is not None:
        trace["z_in"] = model.h(obs).clone()
    metrics.update({"external_reward_mean": reward_mean, "current_std": s0.mean().item()})
    return a, hidden, metrics
