"""The DSSM agents' learners. `DssmLearner`, the iCEM agent's: `TdICemSimDssm.update / update_pi / intrinsic_rewards`
on the GPU.

Reference: src/algorithm/tdmpc_icem_similarity_drnn.py:367-384 (update_pi), :421-443 (intrinsic_rewards), :445-553
(update). The math is the reference's (tests/drnn_update_ref.py restates it and is pinned bit for bit to the reference
on the CPU; tests/test_gpu_drnn_update.py holds this module to it), including its quirks: no `rho` anywhere (the
discount of later steps is computed and not used), the similarity term in the place of TOLD's consistency term, the
weighting `mean(model_loss [B, 1] * weights [B]) + mean(td_loss)` whose first term is a mean over the [B, B] broadcast
(= mean(model_loss) * mean(weights)), TD-lambda value targets from `reward + explore_coef * intrinsic`, the online
encoder and policy with the target Q in those targets, and intrinsic rewards normalised by a running mean / std.

`DssmLearner(agent, graph=True, warmup=3)` has two paths.

The HIP path (the model on the GPU) orders one update for the device:
  * the online encoder on `obs` with grad; the online and target encoders on `next_obses` once, without grad (the
    reference encodes them twice with identical results);
  * the intrinsic rewards -- in the reference H + 1 separate train-mode `next` + `pred_z` passes, each normalising its
    BatchNorms over its own B rows, then a `.cpu()` round trip through a float64 RunningMeanStd -- as ONE segmented
    launch chain and one finishing kernel on a device-resident RunningMeanStd (DssmTrainStep.intrinsic_rewards);
  * the target-Q minimum of all H steps in one H B-row pass;
  * the H-step rollout through `DssmTrainStep.next`, Q1 / Q2 on (z_t, a_t) for all t in one pass, `similarity_loss`
    over the H B concatenated rows, the loss composition with its TD-lambda recursion as `_DssmFusedLoss`;
  * backward, `clip_grad_norm_19`, the optimiser step, the priority write-back, and `update_pi` over the H + 1 latents in
    one pass: `learner.GraphLearner`'s `_optimize`, `_finish` and `_update_pi`, which every learner's update ends with.
The first three items are `_hip_prelude`, which `icem_learner.IcemMlpLearner` runs as it stands; `DssmSimLearner`, whose
warm-up steps come between the encoders and the intrinsic rewards, takes its two parts `_encode_next` and
`_min_target_q`.
Nothing synchronises with the host. After `warmup` eager updates one update per (buffer.idx, buffer._full) is captured
into a HIP graph and replayed by `learner.GraphLearner`, the base shared with the TOLD learner; the explore coefficient
changes every step, so it lives in a device scalar that `update` writes before each replay. The encoder, Q and pi MLPs
run on PyTorch-ROCm autograd here (float32 matmul precision pinned); `dssm_engine.DssmEngineLearner` is the same update
on tdmpc_lg_gemm / tdmpc_lg_rows_* without autograd, opt-in.

The PyTorch path is the reference's own order of operations, call by call, in plain PyTorch. It runs when the model is on
the CPU (tests/test_drnn_update_cpu.py holds it bit for bit to the restatement) and on the GPU with
TDMPC_DSSM_LEARNER_HIP=0 (tools/drnn_update_bench.py's comparison leg: the PyTorch-ROCm update on the same GPU, its
RunningMeanStd on the device as well, so that it synchronises no more than the HIP path).

`DssmSimLearner(DssmLearner)` is the MPC agent's (`TdMpcSimDssm.update / intrinsic_rewards`,
src/algorithm/tdmpc_similarity_drnn.py:373-496; tests/drnn_sim_update_ref.py restates it). It shares the
optimisers, `update_pi`, the EMA, the graph driver and the RunningMeanStd state, and differs in three parts: the
intrinsic rewards carry ONE hidden state through the H + 1 closed-loop steps, of which the first `warmup_len` only
advance it (DssmTrainStep.intrinsic_chain_rewards); the update is `warmup_len` closed-loop `next` calls from the online
encodings (gradient into the encoder) followed by `horizon - warmup_len` open-loop steps, every predicted latent
augmented with Gaussian noise of scale 0.1; one-step TD targets, reward / value / priority sums over the open-loop
steps only, the similarity sum over all H, and every term under the priority weights (`_DssmSimFusedLoss`). The
reference admits 1 <= warmup_len <= horizon - 1 (it raises on an empty `torch.cat` at either end) and this class
refuses the rest, and similarity_horizon != 1, by name.

Optimisers (`learner.make_optimizer`, called by `GraphLearner`): the reference builds them with rlpyt's
`create_optimizer(model, optim_id, lr)`, a package that is not available to check its defaults against. Here `cfg.optim_id` 'adam' gives `torch.optim.Adam` and 'adamw'
`torch.optim.AdamW`, with lr = cfg.lr (model) / cfg.pi_lr (policy), weight_decay = getattr(cfg, 'weight_decay', 0.0)
(cfgs/default.yaml: 0.0, at which AdamW and Adam take the same step) and torch's other defaults; `capturable=graph`.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .config import linear_schedule
from .dssm import check_dssm_cfg
from .dssm_train import DssmTrainStep, _DssmFusedLoss, _DssmSimFusedLoss, new_rms_state
from .learner import GraphLearner, check_batch_size, check_optim_id

METRICS = ("consistency_loss", "reward_loss", "value_loss", "pi_loss", "total_loss", "weighted_loss", "grad_norm",
           "intrinsic_batch_reward_mean")


def check_update_cfg(cfg, who):
    """Raise for what no similarity learner with intrinsic rewards covers (`who`: the class the message names)."""
    B, H = int(cfg.batch_size), int(cfg.horizon)
    check_batch_size(cfg, who)
    if (H + 1) * B > _lib.DT_MAX_ROWS:
        raise ValueError(f"{who}: (horizon + 1) * batch_size = {(H + 1) * B} rows exceed {_lib.DT_MAX_ROWS} "
                         f"(horizon={H}, batch_size={B}): the intrinsic-reward pass and its normalisation take at most "
                         f"that many rows")
    check_optim_id(cfg, who)


def check_learner_cfg(cfg):
    """Raise for what the DSSM learner does not cover, each setting named, before anything touches the device."""
    check_dssm_cfg(cfg)
    check_update_cfg(cfg, "DssmLearner")


class RewardRms:
    """The reference's `reward_rms` (gym's RunningMeanStd) as a view of the learner's device state [mean, var, count];
    reading an attribute synchronises."""

    def __init__(self, state):
        self.state = state

    mean = property(lambda self: float(self.state[0]))
    var = property(lambda self: float(self.state[1]))
    count = property(lambda self: float(self.state[2]))


def rms_update(state, x):
    """gym's RunningMeanStd.update_from_moments(mean(x), var(x), 1) on state = float64 [mean, var, count], in place
    (tdmpc_icem_similarity_drnn.py:436-438). On the CPU the moments are numpy's, in x's precision, as the reference
    takes them; on the GPU float64 device reductions (no host round trip)."""
    if x.device.type == "cpu":
        arr = x.detach().numpy()
        bm = torch.tensor(float(np.mean(arr)), dtype=torch.float64)
        bv = torch.tensor(float(np.std(arr) ** 2), dtype=torch.float64)
    else:
        xd = x.detach().double()
        bm, bv = xd.mean(), xd.var(unbiased=False)
    mean, var, count = state[0].clone(), state[1].clone(), state[2].clone()
    delta = bm - mean
    tot = count + 1
    state[0] = mean + delta / tot
    state[1] = (var * count + bv + delta * delta * count / tot) / tot
    state[2] = tot


def rms_normalize(state, x):
    """:439-441 as the reference's NumPy computes it on a float32 array against the float64 state: the division in
    float64 rounded to x's precision, the threshold subtracted in float64, max(., 0), back to x's precision."""
    sd = torch.sqrt(state[1])
    y = (x.double() / sd).to(x.dtype)
    return torch.clamp_min(y.double() - state[0] / sd, 0).to(x.dtype)


def cosine_loss(model, z_pred, target):
    """The reference's similarity term per row: 2 - 2 <normalize(pred_z(z_pred)), normalize(target)> -> [..., 1]."""
    pred = F.normalize(model.pred_z(z_pred), dim=-1, p=2)
    return 2.0 - 2.0 * (pred * F.normalize(target, dim=-1, p=2)).sum(dim=-1, keepdim=True)


class DssmLearner(GraphLearner):
    """Owns the optimisers, the RunningMeanStd state and (in graph mode) the captured update graphs of one DSSM iCEM
    agent (`agent`: cfg, model, model_target, device and, when it plans, planner)."""

    METRICS = METRICS
    MAX_LOSSES = 1   # live similarity_loss calls of one update
    HIP_ENV = "TDMPC_DSSM_LEARNER_HIP"   # "0": the PyTorch path on the GPU
    check_cfg = staticmethod(check_learner_cfg)

    def __init__(self, agent, graph: bool = True, warmup: int = 3):
        cfg = agent.cfg
        self.check_cfg(cfg)
        super().__init__(agent, graph, warmup)
        self.hip = self.on_gpu and os.environ.get(self.HIP_ENV, "1") != "0"
        self.rms = new_rms_state(self.device)
        self.reward_rms = RewardRms(self.rms)
        self.coef = torch.zeros(1, dtype=torch.float32 if self.hip else self.dtype, device=self.device)
        self.train_step = None
        if self.hip:
            self.train_step = self._make_train_step(agent.model, int(cfg.batch_size), int(cfg.horizon))

    def _make_train_step(self, model, B, H):
        return DssmTrainStep(model, max_rows=B, max_steps=H, max_loss_rows=H * B, max_losses=self.MAX_LOSSES)

    def update_pi(self, zs, eps=None):
        """:367-384 -> pi_loss (tensor). zs: the detached latents; eps: optional [B, A] TruncatedNormal draws, one per
        latent. No rho, as the reference's live line; the HIP path takes the latents in one pass."""
        return self._update_pi(zs, eps, batched=self.hip)

    # ------------------------------------------------------------------ one update
    def step(self, buffer, noise=None):
        """One `TdICemSimDssm.update` without the EMA -> metrics tensor [8] (METRICS order), no synchronisation.
        noise: optional list of 2H + 1 [B, A] TruncatedNormal draws (H for the value targets, H + 1 for update_pi).
        The explore coefficient is read from `self.coef` (`update` writes it)."""
        return self._step_hip(buffer, noise) if self.hip else self._step_torch(buffer, noise)

    @torch.no_grad()
    def _encode_next(self, next_obses):
        """The online and the target encoder on the H + 1 next observations, once each -> two [(H + 1) B, L]."""
        flat = next_obses.reshape(next_obses.shape[0] * next_obses.shape[1], -1)
        return self.agent.model.h(flat), self.agent.model_target.h(flat)

    @torch.no_grad()
    def _min_target_q(self, nz_on, lo, hi, B, eps):
        """The min target Q at the online next latents of steps [lo, hi) under the online policy, every step at once
        -> [hi - lo, B]. eps: the steps' explicit draws or None."""
        m, n = self.agent.model, hi - lo
        x = nz_on[lo * B:hi * B]
        act = m.pi(x, self.cfg.min_std, eps=None if eps is None else torch.cat(list(eps[:n])))
        return torch.min(*self.agent.model_target.Q(x, act)).view(n, B)

    def _intrinsic_kw(self):
        return {}

    def _hip_prelude(self, buffer, noise):
        """What the HIP paths of the two iCEM learners do before their rollouts -> (the batch, z = h(obs) with grad, the
        target encodings [(H + 1) B, L], intrinsic [(H + 1) B], reward_pi [(H + 1) B], next_q [H, B])."""
        a, H = self.agent, int(self.cfg.horizon)
        batch = buffer.sample()
        obs, next_obses, action, reward = batch[:4]
        B = obs.shape[0]
        a.optim.zero_grad(set_to_none=True)
        z = a.model.h(obs)
        nz_on, nz_tg = self._encode_next(next_obses)
        with torch.no_grad():
            # rollout t starts at z_traj[t] = (z, online next latents)[t] and is compared with target[t]
            z_traj = torch.cat([z.detach(), nz_on[:H * B]])
            intrinsic, reward_pi = self.train_step.intrinsic_rewards(
                z_traj, action.reshape((H + 1) * B, -1), nz_tg, H + 1, self.rms, self.coef, reward.reshape(-1),
                **self._intrinsic_kw())
        return batch, z, nz_tg, intrinsic, reward_pi, self._min_target_q(nz_on, 0, H, B, noise)

    def _finish_hip(self, buffer, idxs, scal, rows, zs, noise, n, grad_norm, intrinsic):
        """`_finish` on a fused loss's outputs: scal = (the four means, weighted, ...), rows[3] the priorities."""
        B = rows.shape[1]
        return self._finish(buffer, idxs, rows[3].view(B, 1), [t.detach() for t in zs], noise, n,
                            (scal[0], scal[1], scal[2], scal[3]), scal[4], grad_norm, intrinsic.view(-1, B, 1))

    def _step_hip(self, buffer, noise):
        cfg, m, ts = self.cfg, self.agent.model, self.train_step
        H = int(cfg.horizon)
        (obs, _, action, reward, idxs, weights), z, nz_tg, intrinsic, reward_pi, next_q = self._hip_prelude(buffer, noise)
        B = obs.shape[0]
        hidden = m.init_hidden_state(B, z.device)
        zt, zs, rps = z, [z], []
        for t in range(H):
            zt, hidden, r = ts.next(zt, action[t], hidden)
            zs.append(zt)
            rps.append(r)
        x = torch.cat([torch.stack(zs[:H]), action[:H]], dim=-1).view(H * B, -1)
        Q1, Q2 = m._Q1(x).view(H, B), m._Q2(x).view(H, B)
        sim = ts.similarity_loss(zs[1:], nz_tg[:H * B])
        scal, rows, _ = _DssmFusedLoss.apply(
            sim.view(H, B), Q1, Q2, torch.stack(rps).view(H, B), reward[:H].reshape(H, B),
            reward_pi.view(H + 1, B)[:H], next_q, weights,
            (float(cfg.similarity_coef), float(cfg.reward_coef), float(cfg.value_coef), float(cfg.discount),
             float(cfg.td_lambda)))
        grad_norm = self._optimize(scal[4])
        return self._finish_hip(buffer, idxs, scal, rows, zs, noise, H, grad_norm, intrinsic)

    def _rollout_one(self, z, a):
        """One `next` from a fresh hidden state -> the predicted latent."""
        m = self.agent.model
        return m.next(z, a, m.init_hidden_state(z.shape[0], z.device).to(z.dtype))[0]

    def _intrinsic_torch(self, obs, next_obses, action):
        """:421-443 call by call (H + 1 train-mode `next` + `pred_z` passes), the RunningMeanStd by `rms_update`."""
        m, mt, H = self.agent.model, self.agent.model_target, int(self.cfg.horizon)
        with torch.no_grad():
            zs_target = mt.h(next_obses)
            z_traj = m.h(torch.cat([obs.unsqueeze(0), next_obses], dim=0))
            raw = torch.stack([cosine_loss(m, self._rollout_one(z_traj[t], action[t]), zs_target[t])
                               for t in range(H + 1)])              # [H + 1, B, 1]
            rms_update(self.rms, raw)
            return rms_normalize(self.rms, raw)

    def _similarity_torch(self, queries, keys, n):
        loss = cosine_loss(self.agent.model, torch.cat(queries, dim=0), torch.cat(keys, dim=0))
        return loss.reshape(n, self.cfg.batch_size, -1).sum(dim=0)

    def _step_torch(self, buffer, noise):
        cfg, m, mt = self.cfg, self.agent.model, self.agent.model_target
        H = int(cfg.horizon)
        obs, next_obses, action, reward, idxs, weights = buffer.sample()
        B = obs.shape[0]
        self.agent.optim.zero_grad(set_to_none=True)
        z = m.h(obs)
        next_zs = mt.h(next_obses)
        online_next_zs = m.h(next_obses)
        zs = [z.detach()]
        intrinsic = self._intrinsic_torch(obs, next_obses, action)
        reward_pi = self.coef * intrinsic + reward
        rewards = reward_pi[:H]
        discounts = torch.ones_like(rewards) * cfg.discount
        next_q = []
        for t in range(H):
            with torch.no_grad():
                nz = online_next_zs[t]
                next_q.append(torch.min(*mt.Q(nz, m.pi(nz, cfg.min_std, eps=None if noise is None else noise[t]))))
        next_q = torch.stack(next_q, dim=0)
        last = next_q[-1]
        inputs = rewards + discounts * next_q * (1 - cfg.td_lambda)
        outputs = []
        for index in reversed(range(H)):
            last = inputs[index] + discounts[index] * last * cfg.td_lambda
            outputs.append(last)
        td = torch.stack(list(reversed(outputs)), dim=0)
        reward_loss, value_loss, priority_loss = 0, 0, 0
        hidden = m.init_hidden_state(B, z.device).to(z.dtype)
        queries, keys = [], []
        for t in range(H):
            Q1, Q2 = m.Q(z, action[t])
            z, hidden, reward_pred = m.next(z, action[t], hidden)
            reward_loss += F.mse_loss(reward_pred, reward[t], reduction="none")
            value_loss += F.mse_loss(Q1, td[t], reduction="none") + F.mse_loss(Q2, td[t], reduction="none")
            priority_loss += F.l1_loss(Q1, td[t], reduction="none") + F.l1_loss(Q2, td[t], reduction="none")
            queries.append(z)
            keys.append(next_zs[t].detach())
            zs.append(z.detach())
        similarity_loss = 0 + self._similarity_torch(queries, keys, H)
        model_loss = cfg.similarity_coef * similarity_loss.clamp(max=1e4) + cfg.reward_coef * reward_loss.clamp(max=1e4)
        td_loss = cfg.value_coef * value_loss.clamp(max=1e4)
        total_loss = model_loss + td_loss
        weighted = (model_loss * weights).mean() + td_loss.mean()   # the reference's [B, B] broadcast, literally
        grad_norm = self._optimize(weighted)
        return self._finish(buffer, idxs, priority_loss.clamp(max=1e4).detach(), zs, noise, H,
                            (similarity_loss.mean(), reward_loss.mean(), value_loss.mean(), total_loss.mean()),
                            weighted, grad_norm, intrinsic)

    def update(self, buffer, step, noise=None):
        """`TdICemSimDssm.update` semantics -> (metrics tensor [8] on the device, explore_coef); no synchronisation."""
        coef = linear_schedule(self.cfg.explore_schedule, step)
        self.coef.fill_(coef)
        return super().update(buffer, step, noise), coef


def check_sim_learner_cfg(cfg):
    """`check_learner_cfg` and what `TdMpcSimDssm.update` itself admits, each setting named."""
    check_learner_cfg(cfg)
    H, W = int(cfg.horizon), int(getattr(cfg, "warmup_len", 0))
    if not 1 <= W <= H - 1:
        raise ValueError(f"DssmSimLearner: warmup_len={W} is not in [1, horizon - 1 = {H - 1}]: the reference's update "
                         f"concatenates an empty list of latents at warmup_len = 0 and at warmup_len = horizon")
    sh = int(getattr(cfg, "similarity_horizon", 1))
    if sh != 1:
        raise NotImplementedError(f"DssmSimLearner: similarity_horizon={sh} is not supported (1 only: longer rollouts "
                                  f"hand their last hidden state to the next start)")


class DssmSimLearner(DssmLearner):
    """The learner of `TdMpcDrnn` (`TdMpcSimDssm.update`, tdmpc_similarity_drnn.py:373-496). `step(buffer, noise)`:
    noise = (2 (H - W) + 1 [B, A] TruncatedNormal draws -- H - W for the TD targets, H - W + 1 for update_pi --, H
    [B, L] augmentation noises, added as they are: the reference's Normal(0, 0.1) samples), or None to draw on the
    device."""

    MAX_LOSSES = 2
    check_cfg = staticmethod(check_sim_learner_cfg)
    AUG_SCALE = 0.1   # helper.RandomAdditiveGaussianNoiseAug(cfg, scale=0.1), :103

    def _draws(self, noise, B):
        H, L = int(self.cfg.horizon), int(self.cfg.latent_dim)
        if noise is not None:
            return noise[0], list(noise[1])
        return None, list((torch.randn(H, B, L, dtype=self.dtype, device=self.device) * self.AUG_SCALE).unbind(0))

    def _step_hip(self, buffer, noise):
        cfg, m, ts = self.cfg, self.agent.model, self.train_step
        H, W = int(cfg.horizon), int(cfg.warmup_len)
        N = H - W
        obs, next_obses, action, reward, idxs, weights = buffer.sample()
        B = obs.shape[0]
        eps, aug = self._draws(noise, B)
        self.agent.optim.zero_grad(set_to_none=True)
        # the latents the gradient reaches: obs and next_obses[:W] (zs_traj[0 .. W]); the later online encodings feed
        # only no_grad consumers
        zg = m.h(torch.cat([obs.unsqueeze(0), next_obses[:W]]).reshape((W + 1) * B, -1)).view(W + 1, B, -1)
        nz_on, nz_tg = self._encode_next(next_obses)               # [(H + 1) B, L]: online, target
        # :428-434: the closed-loop warm-up and its similarity loss
        hidden = m.init_hidden_state(B, obs.device)
        queries = []
        for i in range(W):
            zp, hidden, _ = ts.next(zg[i], action[i], hidden)
            queries.append(zp + aug[i])
        sim_w = ts.similarity_loss(queries, nz_tg[:W * B])
        with torch.no_grad():
            # :373-402, one hidden state through the H + 1 steps
            z_traj = torch.cat([zg[0].detach(), nz_on[:H * B]])
            intrinsic, reward_pi = ts.intrinsic_chain_rewards(z_traj, action.reshape((H + 1) * B, -1), nz_tg, H + 1, W,
                                                              self.rms, self.coef, reward.reshape(-1))
        next_q = self._min_target_q(nz_on, W, H, B, eps)            # :339-344, the shoot steps at once
        # :443-455: the open-loop shoot
        zt, zin, zout, rps = zg[W], [], [], []
        for t in range(W, H):
            zin.append(zt)
            zt, hidden, r = ts.next(zt, action[t], hidden)
            zt = zt + aug[t]
            zout.append(zt)
            rps.append(r)
        x = torch.cat([torch.stack(zin), action[W:H]], dim=-1).view(N * B, -1)
        Q1, Q2 = m._Q1(x).view(N, B), m._Q2(x).view(N, B)
        sim_s = ts.similarity_loss(zout, nz_tg[W * B:H * B])
        scal, rows, _ = _DssmSimFusedLoss.apply(
            torch.cat([sim_w, sim_s]).view(H, B), Q1, Q2, torch.stack(rps).view(N, B), reward[W:H].reshape(N, B),
            reward_pi.view(H + 1, B)[W:H], next_q, weights,
            (float(cfg.similarity_coef), float(cfg.reward_coef), float(cfg.value_coef), float(cfg.discount)))
        grad_norm = self._optimize(scal[4])
        return self._finish_hip(buffer, idxs, scal, rows, [zg[W]] + zout, eps, N, grad_norm, intrinsic)

    def _intrinsic_torch(self, obs, next_obses, action):
        """:373-402 call by call at similarity_horizon 1, the RunningMeanStd by `rms_update`."""
        m, mt, cfg = self.agent.model, self.agent.model_target, self.cfg
        H, W = int(cfg.horizon), int(cfg.warmup_len)
        with torch.no_grad():
            zs_target = mt.h(next_obses)
            zs_traj = m.h(torch.cat([obs.unsqueeze(0), next_obses], dim=0))
            hidden = m.init_hidden_state(obs.shape[0], obs.device).to(obs.dtype)
            out = []
            for i in range(W):
                _, hidden, _ = m.next(zs_traj[i], action[i], hidden)
                out.append(torch.zeros(obs.shape[0], 1, dtype=obs.dtype, device=obs.device))
            for t in range(W, H + 1):
                zl, hidden, _ = m.next(zs_traj[t], action[t], hidden)
                out.append(cosine_loss(m, zl, zs_target[t]))
            raw = torch.stack(out)                                   # [H + 1, B, 1], zeros in the warm-up rows
            rms_update(self.rms, raw)
            return rms_normalize(self.rms, raw)

    def _step_torch(self, buffer, noise):
        cfg, m, mt = self.cfg, self.agent.model, self.agent.model_target
        H, W = int(cfg.horizon), int(cfg.warmup_len)
        N = H - W
        obs, next_obses, action, reward, idxs, weights = buffer.sample()
        B = obs.shape[0]
        eps, aug = self._draws(noise, B)
        self.agent.optim.zero_grad(set_to_none=True)
        z = m.h(obs)
        online_next_zs = m.h(next_obses)
        target_next_zs = mt.h(next_obses)
        zs_traj = torch.cat([z.unsqueeze(0), online_next_zs], dim=0)
        similarity_loss, reward_loss, value_loss, priority_loss = 0, 0, 0, 0
        hidden = m.init_hidden_state(B, z.device).to(z.dtype)
        queries, keys = [], []
        for i in range(W):
            z_pred, hidden, _ = m.next(zs_traj[i], action[i], hidden)
            queries.append(z_pred + aug[i])
            keys.append(target_next_zs[i].detach())
        similarity_loss += self._similarity_torch(queries, keys, W)
        intrinsic = self._intrinsic_torch(obs, next_obses, action)
        reward_pi = self.coef * intrinsic + reward
        queries, keys = [], []
        z_shoot = zs_traj[W]
        zs = [z_shoot.detach()]
        for t in range(W, H):
            Q1, Q2 = m.Q(z_shoot, action[t])
            z_shoot, hidden, reward_pred = m.next(z_shoot, action[t], hidden)
            z_shoot = z_shoot + aug[t]
            queries.append(z_shoot)
            keys.append(target_next_zs[t].detach())
            zs.append(z_shoot.detach())
            with torch.no_grad():
                nz = online_next_zs[t]
                e = None if eps is None else eps[t - W]
                td = reward_pi[t] + cfg.discount * torch.min(*mt.Q(nz, m.pi(nz, cfg.min_std, eps=e)))
            reward_loss += F.mse_loss(reward_pred, reward[t], reduction="none")
            value_loss += F.mse_loss(Q1, td, reduction="none") + F.mse_loss(Q2, td, reduction="none")
            priority_loss += F.l1_loss(Q1, td, reduction="none") + F.l1_loss(Q2, td, reduction="none")
        similarity_loss += self._similarity_torch(queries, keys, N)
        total_loss = cfg.similarity_coef * similarity_loss.clamp(max=1e4) + \
            cfg.reward_coef * reward_loss.clamp(max=1e4) + cfg.value_coef * value_loss.clamp(max=1e4)
        weighted = (total_loss * weights).mean()                    # the reference's [B, B] broadcast, literally
        grad_norm = self._optimize(weighted)
        return self._finish(buffer, idxs, priority_loss.clamp(max=1e4).detach(), zs, eps, N,
                            (similarity_loss.mean(), reward_loss.mean(), value_loss.mean(), total_loss.mean()),
                            weighted, grad_norm, intrinsic)
