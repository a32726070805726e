"""The yardstick of the MLP iCEM update (tdmpc_amd/icem_learner.py): the reference's `TdICemSimMlp.update`,
`intrinsic_rewards`, `_td_target`, `similarity_loss` and `update_pi` (src/algorithm/tdmpc_icem_similarity_mlp.py:267-428)
restated in plain PyTorch over the project's eager `tdmpc_amd.icem_mlp.IcemMlpModel`, operation by operation in the
reference's order, generic in the dtype.

In float32 on the CPU it equals the recorded reference run (tests/golden/icem_update/*.npz, written by
tests/golden/make_icem_update_golden.py) bit for bit: tests/test_icem_update_cpu.py. In float64 it is what
tests/test_gpu_icem_update.py compares the GPU with, and float32 against float64 is the noise floor those bounds are
derived from.

The RunningMeanStd restatement, the NumPy arithmetic of the reward normalisation, the fixed batch, the summaries and the
comparison by class are tests/drnn_update_ref.py's (the DSSM iCEM agent's update shares them); this file holds what
differs: the model, the cases, the update itself and the zero-mean bias of the one train-mode BatchNorm.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import drnn_update_ref as D
from drnn_update_ref import (FakeBuffer, METRICS, STEPS, TIE, batch, bound, draws, figure, grads_of, record,  # noqa: F401
                             rms_update_from_moments, summarize)
from tdmpc_amd.config import linear_schedule, make_cfg
from tdmpc_amd.icem_mlp import IcemMlpModel, synthetic_icem_mlp_state_dict

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "icem_update")

# name -> (task, latent_dim, horizon, batch_size, model seed, target seed, batch seed, torch seed)
#   cheetah: L50 A6, H = 3, B = 33 (one partial BatchNorm chunk per segment)
#   tiny:    (L, A) = (8, 1), H = 2, B = 2: the two-row BatchNorm
#   wide:    cheetah with B = 130 (two chunks per segment, every later segment off the 128-row grid); not recorded
CASES = {
    "cheetah": ("cheetah", 50, 3, 33, 51, 52, 61, 0),
    "tiny": ("cartpole", 8, 2, 2, 53, 54, 62, 0),
    "wide": ("cheetah", 50, 3, 130, 55, 56, 63, 0),
}
RECORDED = ("cheetah", "tiny")
INIT_SEED = 3   # torch.manual_seed before the recorded construction of the reference model (golden/icem_update/init.npz)
RHO = 0.5   # cfgs/default.yaml has 1.0, at which the reference's `rho ** t` is invisible


def case_cfg(name):
    task, L, H, B = CASES[name][:4]
    return make_cfg(task, latent_dim=L, horizon=H, batch_size=B, optim_id="adam", rho=RHO, train_steps=100000,
                    episode_length=500)


def case_batch(name):
    return batch(case_cfg(name), CASES[name][6])


def case_draws(name, k):
    return draws(case_cfg(name), 1000 + 10 * CASES[name][7] + k)


def make_models(cfg, name, dtype=torch.float32, device="cpu"):
    out = []
    for seed in CASES[name][4:6]:
        m = IcemMlpModel(cfg, init="none")
        m.load_state_dict(synthetic_icem_mlp_state_dict(cfg, seed))
        out.append(m.to(device=device, dtype=dtype).eval())
    return out


class RefAgent:
    """The reference agent's learning state: model, target, the two Adam optimisers, reward_rms."""

    def __init__(self, cfg, name, dtype=torch.float32):
        self.cfg, self.dtype = cfg, dtype
        self.model, self.model_target = make_models(cfg, name, dtype)
        self.optim = torch.optim.Adam(self.model.parameters(), lr=cfg.lr)
        self.pi_optim = torch.optim.Adam(self.model._pi.parameters(), lr=cfg.pi_lr)
        self.rms = [np.float64(0.0), np.float64(1.0), np.float64(1e-4)]   # RunningMeanStd(): mean, var, count
        self.pi_tie = np.inf

    def pi(self, z, eps):
        return self.model.pi(z, self.cfg.min_std, eps=eps)

    def update_pi(self, zs, eps):
        """:267-284."""
        self.pi_optim.zero_grad(set_to_none=True)
        self.model.track_q_grad(False)
        pi_loss = 0
        for t, z in enumerate(zs):
            a = self.pi(z, eps[t])
            q1, q2 = self.model.Q(z, a)
            Q = torch.min(q1, q2)
            with torch.no_grad():
                margin = ((q1 - q2).abs() / (1 + Q.abs())).min()
                self.pi_tie = min(self.pi_tie, float(margin))
            pi_loss += -Q.mean()
        pi_loss.backward()
        torch.nn.utils.clip_grad_norm_(self.model._pi.parameters(), self.cfg.grad_clip_norm, error_if_nonfinite=False)
        self.pi_optim.step()
        self.model.track_q_grad(True)
        return pi_loss.item()

    @torch.no_grad()
    def _td_target(self, next_z, reward, eps):
        """:286-292."""
        q = torch.min(*self.model_target.Q(next_z, self.pi(next_z, eps)))
        return reward + self.cfg.discount * q

    def similarity_loss(self, queries, keys):
        """:294-300."""
        queries = torch.cat(queries, dim=0)
        queries = self.model.pred_z(queries)
        keys = torch.cat(keys, dim=0)
        queries_norm = F.normalize(queries, dim=-1, p=2)
        keys_norm = F.normalize(keys, dim=-1, p=2)
        return 2.0 - 2.0 * (queries_norm * keys_norm).sum(dim=-1)

    @torch.no_grad()
    def intrinsic_rewards(self, obs, next_obses, actions):
        """:313-344."""
        cfg, m = self.cfg, self.model
        zs_target = self.model_target.h(next_obses)
        z_traj = m.h(torch.cat([obs.unsqueeze(0), next_obses], dim=0))
        unc = torch.zeros((cfg.horizon + 1, cfg.horizon + 1, cfg.batch_size, 1), dtype=self.dtype)
        for t in range(0, z_traj.shape[0] - 1):
            z, _ = m.next(z_traj[t], actions[t:t + 1][0])
            zs_latent = torch.stack([z], dim=0)
            zs_pred = m.pred_z(zs_latent.squeeze(0))
            zs_pred = F.normalize(zs_pred.unsqueeze(0), dim=-1, p=2)
            target = F.normalize(zs_target[t:t + 1], dim=-1, p=2)
            unc[t][t:t + 1] = 2.0 - 2.0 * (zs_pred * target).sum(dim=-1, keepdim=True)
        raw = torch.sum(unc, dim=0).numpy()
        self.raw_uncertainty = raw.copy()
        bm, bs = np.mean(raw), np.std(raw)
        self.rms = rms_update_from_moments(self.rms, np.float64(bm), np.float64(bs ** 2))
        sd = np.sqrt(self.rms[1])
        x = (raw.astype(np.float64) / sd).astype(raw.dtype)
        x = np.maximum(x.astype(np.float64) - self.rms[0] / sd, 0)
        return torch.from_numpy(x).to(self.dtype)

    def update(self, b, step, noise):
        """:346-428 on the batch b -> dict(metrics [9] (METRICS), prio, intrinsic, rms, grads, tie). noise: the 2H + 1
        TruncatedNormal draws in the reference's order (H TD targets, H + 1 update_pi)."""
        cfg, m, mt, dt = self.cfg, self.model, self.model_target, self.dtype
        H = cfg.horizon
        obs, next_obses, action, reward = (t.to(dt) for t in b[:4])
        weights = b[5].to(dt)
        noise = [n.to(dt) for n in noise]
        m.train()
        self.optim.zero_grad(set_to_none=True)
        z = m.h(obs)
        next_zs = mt.h(next_obses)
        online_next_zs = m.h(next_obses)
        zs = [z.detach()]
        explore_coef = linear_schedule(cfg.explore_schedule, step)
        intrinsic = self.intrinsic_rewards(obs, next_obses, action)
        reward_pi = explore_coef * intrinsic + reward

        similarity_loss, reward_loss, value_loss, priority_loss = 0, 0, 0, 0
        zs_query, zs_key = [], []
        for t in range(H):
            rho = (cfg.rho ** t)
            Q1, Q2 = m.Q(z, action[t])
            z, reward_pred = m.next(z, action[t])
            with torch.no_grad():
                td_target = self._td_target(online_next_zs[t], reward_pi[t], noise[t])
            reward_loss += (F.mse_loss(reward_pred, reward[t], reduction="none")) * rho
            value_loss += (F.mse_loss(Q1, td_target, reduction="none") +
                           F.mse_loss(Q2, td_target, reduction="none")) * rho
            priority_loss += (F.l1_loss(Q1, td_target, reduction="none") +
                              F.l1_loss(Q2, td_target, reduction="none")) * rho
            zs_query.append(z)
            zs_key.append(next_zs[t].detach())
            zs.append(z.detach())
        similarity_loss += self.similarity_loss(zs_query, zs_key).reshape(H, cfg.batch_size, -1).sum(dim=0)

        total_loss = cfg.similarity_coef * similarity_loss.clamp(max=1e4) + \
            cfg.reward_coef * reward_loss.clamp(max=1e4) + \
            cfg.value_coef * value_loss.clamp(max=1e4)
        weighted_loss = (total_loss * weights).mean()
        weighted_loss.register_hook(lambda grad: grad * (1 / H))
        weighted_loss.backward()
        grad_norm = torch.nn.utils.clip_grad_norm_(m.parameters(), cfg.grad_clip_norm, error_if_nonfinite=False)
        self.optim.step()
        prio = priority_loss.clamp(max=1e4).detach()

        pi_loss = self.update_pi(zs, noise[H:])
        if step % cfg.update_freq == 0:
            with torch.no_grad():
                for p, p_target in zip(m.parameters(), mt.parameters()):
                    p_target.data.lerp_(p.data, cfg.tau)
        m.eval()
        metrics = np.array([float(similarity_loss.mean().item()), float(reward_loss.mean().item()),
                            float(value_loss.mean().item()), pi_loss, float(total_loss.mean().item()),
                            float(weighted_loss.mean().item()), float(grad_norm), intrinsic.mean().item(),
                            explore_coef], dtype=np.float64)
        return dict(metrics=metrics, prio=prio.numpy().copy(), intrinsic=intrinsic.numpy().copy(),
                    rms=np.array([float(v) for v in self.rms]), grads=grads_of(m), tie=self.pi_tie)


def run_case(name, dtype=torch.float32, noise=None):
    """The case's two consecutive updates -> (agent, [result per update], the recording's arrays)."""
    cfg = case_cfg(name)
    agent = RefAgent(cfg, name, dtype)
    b = case_batch(name)
    out, res = {}, []
    for k, step in enumerate(STEPS):
        r = agent.update(b, step, noise[k] if noise is not None else case_draws(name, k))
        record(out, k, r, agent.model, agent.model_target)
        res.append(r)
    return agent, res, out


def load(name):
    return np.load(os.path.join(GOLD_DIR, f"{name}.npz"))


def gold_noise(g, cfg):
    return D.gold_noise(g, cfg)


def case_noise(name):
    """The draws of the case's two updates: the recording's where there is one."""
    if name in RECORDED:
        return gold_noise(load(name), case_cfg(name))
    return [case_draws(name, k) for k in range(len(STEPS))]


# ---------------------------------------------------------------------------------------------------------------------
# Comparing two runs of an update: drnn_update_ref's classes with this model's one zero-mean bias
# ---------------------------------------------------------------------------------------------------------------------
ZERO_MEAN = {"_predictor.0.bias": "_predictor.0"}
CLASSES = D.CLASSES


class PreBNScales(D.PreBNScales):
    """drnn_update_ref.PreBNScales over `_predictor.0`, the one Linear that feeds a train-mode BatchNorm here."""

    def __init__(self, model):
        self.outs = {k: [] for k in ZERO_MEAN}
        mods = dict(model.named_modules())
        self.hooks = [mods[m].register_forward_hook(self._hook(k)) for k, m in ZERO_MEAN.items()]


snapshot = D.snapshot   # (its zero-mean split names `_predictor.0.bias`; the DSSM's other such bias does not exist here)
figures = D.figures


def run_ref(name, dtype, noise=None, scales=False):
    """The case's two updates on the yardstick -> [snapshot per update] (and, float64 only, [scales per update])."""
    cfg = case_cfg(name)
    agent = RefAgent(cfg, name, dtype)
    pre = PreBNScales(agent.model) if scales else None
    b = case_batch(name)
    snaps, scs = [], []
    for k, step in enumerate(STEPS):
        r = agent.update(b, step, noise[k] if noise is not None else case_draws(name, k))
        snaps.append(snapshot(r, agent.model, agent.model_target))
        if pre:
            scs.append(pre.take())
    if pre:
        pre.close()
    return (snaps, scs) if scales else snaps
