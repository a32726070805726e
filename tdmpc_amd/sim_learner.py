"""The similarity TD-MPC agent's learner: `TDMPCSIM.update / update_pi / _td_target / similarity_loss`.

Reference: src/algorithm/tdmpc_similarity.py:202-218 (update_pi), :220-226 (_td_target), :228-234 (similarity_loss),
:298-375 (update). It is `TDMPC.update` with the consistency term replaced by the similarity head -- `_predictor` on the
H B predicted latents as ONE train-mode BatchNorm batch, F.normalize on both sides, 2 - 2 cos against the target
encoder's latents -- and keeps TDMPC's quirks: reward, value, priority and `update_pi` terms weighted by `rho ** t` (the
similarity term not); `(total_loss [B, 1] * weights [B]).mean()`, a mean over the [B, B] broadcast (= mean(total) *
mean(weights); tests/golden/sim_update confirms it); the gradient of the weighted loss divided by the horizon; the TD
target from the ONLINE encoder and policy with the target Q. The optimisers are learner.make_optimizer's at cfg.lr
(model) and cfg.pi_lr (policy), as the reference's `create_optimizer` calls (:96-99).

`SimLearner(agent, graph=True, warmup=3)` is a `learner.EngineLearner`, as `learner.Learner` is, and states only what
differs from it: its engine, its environment variable, the BatchNorm's batch counter after an engine step and

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

import torch
import torch.nn.functional as F

from . import sim_engine
from .drnn_learner import cosine_loss
from .learner import METRICS, EngineLearner, check_batch_size, check_optim_id, check_state_ln  # noqa: F401


def check_sim_learner_cfg(cfg):
    """Raise for what neither path covers, each setting named, before anything touches the device."""
    check_state_ln(cfg, "SimLearner", ": the reference's pixel encoder is rlpyt's")
    check_batch_size(cfg, "SimLearner")
    check_optim_id(cfg, "SimLearner")


class SimLearner(EngineLearner):
    """Owns the optimisers and (in graph mode) the captured update graphs of one `TdMpcSim` agent (`agent`: cfg, model,
    model_target, device and, when it plans, planner). `update(buffer, step, noise)` -> metrics tensor [7] (METRICS) on
    the model's device, no synchronisation; noise: 2H + 1 [B, A] TruncatedNormal draws (H for the TD targets, H + 1 for
    update_pi) or None to draw on the device. `path`: "engine" or "torch"."""

    ENGINE_ENV, ENGINE, ENGINE_CLASS = "TDMPC_SIM_LEARNER_ENGINE", sim_engine, "SimEngine"

    def __init__(self, agent, graph: bool = True, warmup: int = 3):
        check_sim_learner_cfg(agent.cfg)
        super().__init__(agent, graph, warmup)

    def _after_engine_step(self):
        self.agent.model._predictor[1].num_batches_tracked += 1   # (the engine moves the running statistics itself)

    def similarity_loss(self, queries, keys):
        """:228-234 -> [rows]."""
        return cosine_loss(self.agent.model, torch.cat(queries, dim=0), torch.cat(keys, dim=0)).squeeze(-1)

    def _torch_update_pi(self, zs, eps):
        """:202-218: the reference's loop, each term weighted by rho ** t."""
        return self._update_pi(zs, eps, batched=False, rho=self.cfg.rho)

    def _step_torch(self, buffer, noise):
        cfg, m, mt = self.cfg, self.agent.model, self.agent.model_target
        H = int(cfg.horizon)
        obs, next_obses, action, reward, idxs, weights = buffer.sample()
        B = obs.shape[0]
        self.agent.optim.zero_grad(set_to_none=True)
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
        grad_norm = self._optimize(weighted)
        return self._finish(buffer, idxs, priority_loss.clamp(max=1e4).detach(), zs, noise, H,
                            (similarity_loss.mean(), reward_loss.mean(), value_loss.mean(), total_loss.mean()),
                            weighted, grad_norm)
