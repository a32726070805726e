"""Test infrastructure only: CPU restatement of the reference's recurrent-latent (DSSM) planner with explicit noise.

What it restates (`src/algorithm/tdmpc_similarity_drnn.py`):
  * `DSSM.h / next / pi / Q`            :45-81, with `NormGRUCell.forward` (models/rnns.py:19-29), `DGruDyna.forward`
                                        (models/gru_dyna.py:25-29) and `helper.mlp_norm` with BatchNorm1d in eval mode
  * `TdMpcSimDssm.estimate_value`       :136-144
  * `TdMpcSimDssm.plan`                 :184-267 (memory replay, pre-rollout, CEM), every draw from a `NoiseBundle`
The draw order is `TDMPC.plan`'s, so `oracle.tdmpc_ref.draw_noise` (with cfg.mixture_coef set to the call's schedule
value) draws what the reference draws from the same seeds. `dtype`: torch.float32 restates the reference bit for bit
(tests/test_drnn_cpu.py against the recorded fixtures); torch.float64 is the same code as the accuracy yardstick.
"""
from __future__ import annotations

from collections import deque
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle.tdmpc_ref import NoiseBundle, choice_index, draw_noise, linear_schedule  # noqa: F401


class RefDSSM:
    """Functional DSSM over a reference-layout state_dict (CPU, `dtype`)."""

    def __init__(self, sd: dict, cfg, dtype=torch.float32):
        self.sd = {k: (v.detach().to("cpu", dtype) if v.is_floating_point() else v) for k, v in sd.items()}
        self.cfg = cfg
        self.dtype = dtype

    def _lin(self, x, name):
        return F.linear(x, self.sd[name + ".weight"], self.sd.get(name + ".bias"))

    def _ln(self, x, name, eps):
        return F.layer_norm(x, (x.shape[-1],), self.sd[name + ".weight"], self.sd[name + ".bias"], eps)

    def _mlp(self, x, pre):
        x = F.elu(self._lin(x, pre + ".0"))
        x = F.elu(self._lin(x, pre + ".2"))
        return self._lin(x, pre + ".4")

    def _q(self, x, pre):
        x = torch.tanh(self._ln(self._lin(x, pre + ".0"), pre + ".1", 1e-5))
        x = F.elu(self._ln(self._lin(x, pre + ".3"), pre + ".4", 1e-5))
        return self._lin(x, pre + ".6")

    def h(self, obs):
        x = self._ln(self._lin(obs, "_encoder.0"), "_encoder.1", 1e-5)
        return self._lin(F.elu(x), "_encoder.3")

    def gru(self, x, state):
        g = "_dynamics.gru_cell."
        gates_i = self._lin(x, g + "weight_ih")
        gates_h = self._lin(state, g + "weight_hh")
        reset_i, update_i, newval_i = gates_i.chunk(3, 1)
        reset_h, update_h, newval_h = gates_h.chunk(3, 1)
        reset = torch.sigmoid(self._ln(reset_i + reset_h, g + "ln_reset", 1e-3))
        update = torch.sigmoid(self._ln(update_i + update_h, g + "ln_update", 1e-3))
        newval = torch.tanh(self._ln(newval_i + reset * newval_h, g + "ln_newval", 1e-3))
        return update * newval + (1 - update) * state

    def next(self, z, a, h_prev):
        p = "_dynamics.prior_mlp."
        hidden = self.gru(torch.cat([z, a], dim=-1), h_prev)
        x = self._lin(hidden, p + "0")
        x = F.batch_norm(x, self.sd[p + "1.running_mean"], self.sd[p + "1.running_var"], self.sd[p + "1.weight"],
                         self.sd[p + "1.bias"], False, 0.1, 1e-5)
        z = self._lin(F.elu(x), p + "3")
        return z, hidden, self._mlp(hidden, "_reward")

    def pi(self, z, std, eps):
        mu = torch.tanh(self._mlp(z, "_pi"))
        if std > 0:
            scale = torch.ones_like(mu) * std
            eps = eps.to(self.dtype).clone()
            eps *= scale
            eps = torch.clamp(eps, -0.3, 0.3)
            x = mu + eps
            clamped = torch.clamp(x, -1.0 + 1e-6, 1.0 - 1e-6)
            return x - x.detach() + clamped.detach()
        return mu

    def Q(self, z, a):
        x = torch.cat([z, a], dim=-1)
        return self._q(x, "_Q1"), self._q(x, "_Q2")


class DrnnState:
    """What the reference agent keeps on `self`: std, plan_horizon, _prev_mean, memory_latents."""

    def __init__(self, std, warmup_len):
        self.std = std
        self.plan_horizon = 1
        self.prev_mean = None
        self.memory = deque(maxlen=warmup_len)


def call_cfg(cfg, step):
    """cfg with mixture_coef at this step's regularization_schedule value (what plan() reads, :196-197)."""
    c = SimpleNamespace(**vars(cfg))
    c.mixture_coef = linear_schedule(cfg.regularization_schedule, step)
    return c


def call_horizon(cfg, state: DrnnState, step, t0):
    """The horizon plan() will use (:193-195): the schedule moves it only at an episode start."""
    horizon = int(min(cfg.horizon, linear_schedule(cfg.horizon_schedule, step)))
    return horizon if (horizon != state.plan_horizon and t0) else state.plan_horizon


def draw_drnn_noise(cfg, state: DrnnState, step, t0, eval_mode=False, device="cpu") -> NoiseBundle:
    """The reference's draws for this call from torch's / numpy's global generators."""
    c = call_cfg(cfg, step)
    H = call_horizon(cfg, state, step, t0)
    c.horizon, c.horizon_schedule = H, str(float(H))   # draw_noise sizes its draws by plan_horizon(cfg, step)
    return draw_noise(c, step, eval_mode, device)


@torch.no_grad()
def estimate_value(model: RefDSSM, cfg, z, actions, hidden, horizon, eps_term, trace=None):
    """:136-144. trace: a dict that receives the last step's per-row reward ('reward_last')."""
    G, discount = 0, 1
    for t in range(horizon):
        z, hidden, reward = model.next(z, actions[t], hidden)
        G += discount * reward
        discount *= cfg.discount
    G += discount * torch.min(*model.Q(z, model.pi(z, cfg.min_std, eps_term)))
    if trace is not None:
        trace["reward_last"] = reward.clone()
    return G.nan_to_num_(0), float(reward.mean().item())


@torch.no_grad()
def pi_rollout(model: RefDSSM, cfg, z_in, hidden, horizon, num_pi, eps_pi):
    """:203-209."""
    pi_actions = torch.empty(horizon, num_pi, cfg.action_dim, dtype=model.dtype)
    z_pi = z_in.repeat(num_pi, 1)
    hidden_pi = hidden.repeat(num_pi, 1)
    for t in range(horizon):
        pi_actions[t] = model.pi(z_pi, cfg.min_std, eps_pi[t])
        z_pi, hidden_pi, _ = model.next(z_pi, pi_actions[t], hidden_pi)
    return pi_actions


@torch.no_grad()
def plan(model: RefDSSM, cfg, state: DrnnState, obs, hidden, noise: NoiseBundle, eval_mode=False, step=None, t0=True,
         trace=None):
    """:184-267 with explicit noise. hidden: [1, Hd]. Returns (action [A], metrics dict)."""
    dt = model.dtype
    plan_metrics = {"intrinsic_reward_mean": 0.0, "external_reward_mean": 0.0, "current_std": 0.0}
    if step < cfg.seed_steps and not eval_mode:
        return noise.seed_action.clone(), plan_metrics
    obs = torch.tensor(np.asarray(obs), dtype=dt).unsqueeze(0)
    hidden = torch.as_tensor(hidden).to(dt)
    state.plan_horizon = call_horizon(cfg, state, step, t0)
    H = state.plan_horizon
    mixture_coef = linear_schedule(cfg.regularization_schedule, step)
    num_pi = int(mixture_coef * cfg.num_samples)
    for z, a in state.memory:
        _, hidden, _ = model.next(z, a, hidden)
    z_in = model.h(obs)
    A = cfg.action_dim
    if num_pi > 0:
        pi_actions = pi_rollout(model, cfg, z_in, hidden, H, num_pi, noise.eps_pi)
    mean = torch.zeros(H, A, dtype=dt)
    std = 2 * torch.ones(H, A, dtype=dt)
    if not t0 and state.prev_mean is not None:
        mean[:-1] = state.prev_mean[1:]
    reward_mean = 0
    for i in range(cfg.iterations):
        actions = torch.clamp(mean.unsqueeze(1) + std.unsqueeze(1) * noise.eps_cem[i].to(dt), -1, 1)
        z_plan = z_in.repeat(cfg.num_samples, 1)
        hidden_plan = hidden.repeat(cfg.num_samples, 1)
        if num_pi > 0:
            actions = torch.cat([actions, pi_actions], dim=1)
            z_plan = z_in.repeat(cfg.num_samples + num_pi, 1)
            hidden_plan = hidden.repeat(cfg.num_samples + num_pi, 1)
        value, reward_mean = estimate_value(model, cfg, z_plan, actions, hidden_plan, H, noise.eps_term[i])
        elite_idxs = torch.topk(value.squeeze(1), cfg.num_elites, dim=0).indices
        elite_value, elite_actions = value[elite_idxs], actions[:, elite_idxs]
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
            trace.setdefault("actions", []).append(actions.clone())
            trace.setdefault("mean", []).append(mean.clone())
            trace.setdefault("std", []).append(std.clone())
    score = score.squeeze(1).cpu().numpy()
    j = choice_index(score, noise.u)
    actions = elite_actions[:, j]
    state.prev_mean = mean
    mean, std = actions[0], _std[0]
    a = mean
    if not eval_mode:
        a += std * noise.eps_act.to(dt)
    state.memory.append((z_in, a.unsqueeze(0)))
    if trace is not None:
        trace["z_in"] = z_in.clone()
        trace["hidden"] = hidden.clone()
    plan_metrics.update({"intrinsic_reward_mean": 0, "external_reward_mean": reward_mean,
                         "current_std": std.mean().item()})
    return a, plan_metrics
