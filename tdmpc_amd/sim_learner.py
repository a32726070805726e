"""The similarity TD-MPC agent's learner: `TDMPCSIM.update / update_pi / _td_target / similarity_loss`.

Reference: src/algorithm/tdmpc_similarity.py:202-218 (update_pi), :220-226 (_td_target), :228-234 (similarity_loss),
:298-375 (update). It is `TDMPC.update` with the consistency term replaced by the similarity head -- `_predictor` on the
H B predicted latents as ONE train-mode BatchNorm batch, F.normalize on both sides, 2 - 2 cos against the target
encoder's latents -- and keeps TDMPC's quirks: reward, value, priority and `update_pi` terms weighted by `rho ** t` (the
similarity term not); `(total_loss [B, 1] * weights [B]).mean()`, a mean over the [B, B] broadcast (= mean(total) *
mean(weights); tests/golden/sim_update confirms it); the gradient of the weighted loss divided by the horizon; the TD
target from the ONLINE encoder and policy with the target Q. The optimisers are drnn_learner.make_optimizer's at cfg.lr
(model) and cfg.pi_lr (policy), as the reference's `create_optimizer` calls.

`SimLearner(agent, graph=True, warmup=3)` is a `learner.GraphLearner` with two paths, as `learner.Learner` has:

  * the engine path (tdmpc_amd/sim_engine.py: explicit forward and backward HIP passes over flat parameters, no autograd
    and no hipBLASLt; one HIP graph per buffer fill, every reduction in a fixed order) -- the default on the GPU for the
    cfgs `sim_engine.supported` admits (TDMPC_SIM_LEARNER_ENGINE=0 turns it off: tools/sim_update_bench.py's comparison
    leg);
  * the PyTorch path: the reference's order of operations, call by call, in float32. It runs on the CPU
    (tests/test_sim_update_cpu.py holds it bit for bit to the recorded reference run) and on the GPU for every cfg the
    engine does not admit (another mlp_dim, more than 4096 rollout rows, weight decay), as other mlp_dims do in
    `Learner`.

Pixels and normalize=False are refused by name before anything touches the device: the reference's pixel encoder is
rlpyt's, and the BatchNorm-free predictor with the plain encoder is a model nobody trains here.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from . import sim_engine
from .drnn_learner import make_optimizer
from .learner import GraphLearner, clip_grad_norm_19

METRICS = ("consistency_loss", "reward_loss", "value_loss", "pi_loss", "total_loss", "weighted_loss", "grad_norm")


def check_sim_learner_cfg(cfg):
    """Raise for what neither path covers, each setting named, before anything touches the device."""
    if getattr(cfg, "modality", "state") != "state":
        raise NotImplementedError(f"SimLearner: modality={cfg.modality!r} is not supported (state observations only: "
                                  f"the reference's pixel encoder is rlpyt's)")
    if not getattr(cfg, "normalize", True):
        raise NotImplementedError("SimLearner: normalize=False is not supported (the BatchNorm-free predictor and the "
                                  "plain encoder)")
    if getattr(cfg, "norm_type", "ln") != "ln":
        raise NotImplementedError(f"SimLearner: norm_type={cfg.norm_type!r} is not supported ('ln' only)")
    if int(cfg.batch_size) < 2:
        raise ValueError(f"SimLearner: batch_size={cfg.batch_size} is not supported (train-mode BatchNorm needs two rows)")
    if str(getattr(cfg, "optim_id", "adamw")).lower() not in ("adam", "adamw"):
        raise ValueError(f"SimLearner: optim_id={cfg.optim_id!r} is not supported ('adam' or 'adamw')")


class SimLearner(GraphLearner):
    """Owns the optimisers and (in graph mode) the captured update graphs of one `TdMpcSim` agent (`agent`: cfg, model,
    model_target, device and, when it plans, planner). `update(buffer, step, noise)` -> metrics tensor [7] (METRICS) on
    the model's device, no synchronisation; noise: 2H + 1 [B, A] TruncatedNormal draws (H for the TD targets, H + 1 for
    update_pi) or None to draw on the device. `path`: "engine" or "torch"."""

    ENGINE_ENV = "TDMPC_SIM_LEARNER_ENGINE"   # "0": the PyTorch path on the GPU

    def __init__(self, agent, graph: bool = True, warmup: int = 3):
        cfg = agent.cfg
        check_sim_learner_cfg(cfg)
        p0 = next(agent.model.parameters())
        self.device, self.dtype = p0.device, p0.dtype
        on_gpu = self.device.type == "cuda"
        super().__init__(agent, bool(graph) and on_gpu, warmup)
        self.engine = None
        if on_gpu and sim_engine.supported(cfg) and os.environ.get(self.ENGINE_ENV, "1") != "0":
            self.engine = sim_engine.SimEngine(agent)
            agent.optim, agent.pi_optim = self.engine.opt_main, self.engine.opt_pi
            planner = getattr(agent, "planner", None)
            if planner is not None:
                # the engine moved every parameter into its flat buffer: a pack made before (a plan() ahead of the first
                # update) holds the old tensors, and so do the pointers repack_live would read
                planner._packed_key = None
                planner._ptr_arr = None
        else:
            agent.optim = make_optimizer(self.params, cfg, cfg.lr, capturable=self.graph)          # :96-97
            agent.pi_optim = make_optimizer(self.pi_params, cfg, cfg.pi_lr, capturable=self.graph)  # :98-99
        self.path = "engine" if self.engine is not None else "torch"
        self._live_pack = False
        self.last = {}   # the last eager step's priorities (tests)

    # ------------------------------------------------------------------ reference math
    @torch.no_grad()
    def td_target(self, next_obs, reward, eps=None):
        """:220-226."""
        a, cfg = self.agent, self.cfg
        next_z = a.model.h(next_obs)
        return reward + cfg.discount * torch.min(*a.model_target.Q(next_z, a.model.pi(next_z, cfg.min_std, eps=eps)))

    def similarity_loss(self, queries, keys):
        """:228-234 -> [rows]."""
        queries = self.agent.model.pred_z(torch.cat(queries, dim=0))
        keys = torch.cat(keys, dim=0)
        return 2.0 - 2.0 * (F.normalize(queries, dim=-1, p=2) * F.normalize(keys, dim=-1, p=2)).sum(dim=-1)

    def update_pi(self, zs, eps=None):
        """:202-218 -> pi_loss (tensor). zs: the detached latents; eps: optional [B, A] draws, one per latent."""
        a, cfg, m = self.agent, self.cfg, self.agent.model
        if self.engine is not None:
            return self.engine.update_pi(zs, eps)
        a.pi_optim.zero_grad(set_to_none=True)
        m.track_q_grad(False)
        pi_loss = 0
        for t, z in enumerate(zs):
            act = m.pi(z, cfg.min_std, eps=None if eps is None else eps[t])
            pi_loss += -torch.min(*m.Q(z, act)).mean() * (cfg.rho ** t)
        pi_loss.backward()
        clip_grad_norm_19(self.pi_params, cfg.grad_clip_norm)
        a.pi_optim.step()
        m.track_q_grad(True)
        return pi_loss.detach()

    # ------------------------------------------------------------------ one update
    def step(self, buffer, noise=None):
        """One `TDMPCSIM.update` without the EMA -> metrics tensor [7] (METRICS order), no synchronisation."""
        if self.engine is None:
            return self._step_torch(buffer, noise)
        m = self.engine.update(buffer, noise)
        self.agent.model._predictor[1].num_batches_tracked += 1   # (the engine moves the running statistics itself)
        planner = getattr(self.agent, "planner", None)
        if planner is not None:
            from .tdmpc import repack_live
            # the planner's packed weights straight from the engine's flat buffer, as learner.Learner.step does
            self._live_pack = repack_live(planner, self.agent.model)
        return m

    def _step_torch(self, buffer, noise):
        a, cfg, m, mt = self.agent, self.cfg, self.agent.model, self.agent.model_target
        H = int(cfg.horizon)
        obs, next_obses, action, reward, idxs, weights = buffer.sample()
        B = obs.shape[0]
        a.optim.zero_grad(set_to_none=True)
        z = m.h(obs)                                                 # (the state modality's aug is the identity)
        zs = [z.detach()]
        queries, keys = [], []
        reward_loss, value_loss, priority_loss = 0, 0, 0
        for t in range(H):
            Q1, Q2 = m.Q(z, action[t])
            z, reward_pred = m.next(z, action[t])
            with torch.no_grad():
                next_z = mt.h(next_obses[t])
                td = self.td_target(next_obses[t], reward[t], eps=None if noise is None else noise[t])
            queries.append(z)
            keys.append(next_z.detach())
            zs.append(z.detach())
            rho = cfg.rho ** t
            reward_loss += rho * F.mse_loss(reward_pred, reward[t], reduction="none")
            value_loss += rho * (F.mse_loss(Q1, td, reduction="none") + F.mse_loss(Q2, td, reduction="none"))
            priority_loss += rho * (F.l1_loss(Q1, td, reduction="none") + F.l1_loss(Q2, td, reduction="none"))
        similarity_loss = self.similarity_loss(queries, keys).reshape(H, B, -1).sum(dim=0)
        total_loss = cfg.similarity_coef * similarity_loss.clamp(max=1e4) + \
            cfg.reward_coef * reward_loss.clamp(max=1e4) + cfg.value_coef * value_loss.clamp(max=1e4)
        weighted = (total_loss * weights).mean()                    # the reference's [B, B] broadcast, literally
        weighted.register_hook(lambda grad: grad * (1 / H))
        weighted.backward()
        grad_norm = clip_grad_norm_19(self.params, cfg.grad_clip_norm)
        a.optim.step()
        prio = priority_loss.clamp(max=1e4).detach()
        buffer.update_priorities(idxs, prio)
        pi_loss = self.update_pi(zs, eps=None if noise is None else noise[H:])
        self.last = dict(prio=prio)
        return torch.stack([similarity_loss.mean(), reward_loss.mean(), value_loss.mean(), pi_loss.to(weighted.dtype),
                            total_loss.mean(), weighted.detach(), grad_norm]).detach()

    def update(self, buffer, step, noise=None):
        # (on the CPU nothing follows the matmul precision the driver pins)
        run = super().update if self.device.type == "cuda" else self._update
        return run(buffer, step, noise)

    @torch.no_grad()
    def ema(self):
        """helper.py:48-52 over the parameters (the BatchNorm's buffers are not part of it)."""
        return self.engine.ema(self.cfg.tau) if self.engine is not None else super().ema()

    def _before_capture(self):
        if self.engine is not None and getattr(self.agent, "planner", None) is not None:
            # the captured update repacks the planner from the engine's buffer (repack_live): pack once now so the
            # planner holds the live tensors and the pack's job table exists before the capture
            self.agent.planner.pack(self.agent.model)

    def _after_update(self):
        if not self._live_pack:   # (the update itself repacked from the engine's buffer)
            super()._after_update()
