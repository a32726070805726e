"""The MLP iCEM agent's learner: `TdICemSimMlp.update / update_pi / intrinsic_rewards` on the GPU.

Reference: src/algorithm/tdmpc_icem_similarity_mlp.py:267-284 (update_pi), :286-292 (_td_target), :294-300
(similarity_loss), :313-344 (model_rollout, intrinsic_rewards), :346-428 (update). The math is the reference's
(tests/icem_update_ref.py restates it and is pinned bit for bit to the reference on the CPU;
tests/test_gpu_icem_update.py holds this module to it), including its quirks: one-step TD targets from `reward +
explore_coef * intrinsic` at the online next latents under the online policy with the target Q; reward, value and
priority terms weighted by `rho ** t`, the similarity term and `update_pi` not; `(total_loss [B, 1] * weights [B])
.mean()`, a mean over the [B, B] broadcast (= mean(total) * mean(weights)); the gradient of the weighted loss divided by
the horizon; intrinsic rewards normalised by a running mean / std.

`IcemMlpLearner(DssmLearner)` shares the optimisers, `update_pi`, the EMA, the RunningMeanStd state, the graph driver, the
update's tail (`learner.GraphLearner`), the HIP path's prelude up to the rollout (`DssmLearner._hip_prelude`: the first
three items below) and the PyTorch path's intrinsic-reward and similarity code with the DSSM learners
(tdmpc_amd/drnn_learner.py) and has their two paths; `IcemTrainStep(LossStep)` and `_IcemFusedLoss(_StepFusedLoss)` are
its variants of their HIP wrappers (tdmpc_amd/dssm_train.py).

The HIP path (the model on the GPU) orders one update for the device:
  * the online encoder on `obs` with grad; the online and target encoders on `next_obses` once, without grad (the
    reference encodes them three times with identical results);
  * the intrinsic rewards -- in the reference H + 1 separate train-mode `next` + `pred_z` passes, then a `.cpu()` round
    trip through a float64 RunningMeanStd -- as ONE segmented launch chain (tdmpc_icem_intrinsic_fwd: the dynamics MLP
    over all (H + 1) B rows, `_predictor`'s BatchNorm per segment of B rows) and tdmpc_drnn_intrinsic_finish on the
    device-resident RunningMeanStd;
  * the target-Q minimum of all H steps in one H B-row pass;
  * the H-step rollout of `_dynamics`; `_reward`, Q1 and Q2 on all (z_t, a_t) in one pass; `similarity_loss` over the
    H B concatenated rows on the HIP autograd function; the loss composition as `_IcemFusedLoss`, whose backward
    carries the 1 / horizon hook;
  * backward, `clip_grad_norm_19`, the optimiser step, the priority write-back, `update_pi` over the H + 1 latents.
Nothing synchronises with the host; after `warmup` eager updates one update per buffer fill is captured into a HIP graph
and replayed. The encoder, dynamics, reward, Q and pi MLPs run on PyTorch-ROCm autograd (float32 matmul precision
pinned); tdmpc_amd/icem_engine.py runs the same update on tdmpc_lg_gemm / tdmpc_lg_rows_*, opt-in.

The PyTorch path is the reference's own order of operations, call by call. It runs when the model is on the CPU
(tests/test_icem_update_cpu.py holds it bit for bit to the restatement) and on the GPU with TDMPC_ICEM_LEARNER_HIP=0
(tools/icem_update_bench.py's comparison leg, its RunningMeanStd on the device as well).
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn.functional as F

from . import _lib
from ._lib import IcemLossArgs, IcemSimlossSizes, call, dims_from_cfg, ptr
from .drnn_learner import DssmLearner, check_update_cfg
from .dssm_train import LossStep, _StepFusedLoss, _table, intrinsic_finish
from .learner import check_state_ln

DYN_PARAMS = tuple(f"_dynamics.{k}" for k in ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"))
SEGMENTED = True   # `step`'s intrinsic pass: one segmented call (the faster form) or S one-segment calls


def check_icem_learner_cfg(cfg):
    """Raise for what the MLP iCEM learner does not cover, each setting named, before anything touches the device."""
    check_state_ln(cfg, "IcemMlpLearner")
    L, M = int(cfg.latent_dim), int(cfg.mlp_dim)
    if M != 512:
        raise ValueError(f"IcemMlpLearner: mlp_dim={M} is not supported (512 only)")
    if L > 256:
        raise ValueError(f"IcemMlpLearner: latent_dim={L} is not supported (at most 256)")
    check_update_cfg(cfg, "IcemMlpLearner")


class _IcemFusedLoss(_StepFusedLoss):
    """TdICemSimMlp.update's loss composition (:384-411): coefs = (similarity_coef, reward_coef, value_coef, discount,
    rho); scal = (mean similarity, mean reward, mean value, mean total, weighted = mean(total) mean(w), mean w), rows =
    (similarity, reward, value, clamped priority, total) per batch row, td = the one-step TD targets. The gradient
    includes the reference's hook: it is divided by H."""
    ABI, ARGS, ROWS, SCAL = "tdmpc_icem_", IcemLossArgs, 5, 6


class IcemTrainStep(LossStep):
    """The HIP parts of the MLP iCEM update for `model` (a `tdmpc_amd.icem_mlp.IcemMlpModel` on the GPU, fp32):
    `similarity_loss` (through tdmpc_icem_simloss_*), `intrinsic_loss` / `intrinsic_rewards`. The MLP dynamics themselves
    run on PyTorch autograd (model.next). max_loss_rows: the most rows of one `similarity_loss`."""

    LOSS_ABI = "tdmpc_icem_simloss_"

    def __init__(self, model, max_loss_rows: int, max_losses: int = 1):
        super().__init__(model, dims_from_cfg(model.cfg, enc_norm=True), max_loss_rows)
        if _lib.lib().tdmpc_icem_learner_version() != _lib.ICEM_LEARNER_VERSION:
            raise RuntimeError("libtdmpc_hip: tdmpc_icem_learner_version mismatch")
        sl = IcemSimlossSizes()
        call("tdmpc_icem_simloss_sizes_for", self.dims, self.max_loss_rows, sl)
        self._dyn_params = self._params(DYN_PARAMS)
        self._loss_buffers(max_losses, sl.loss_saved_floats, sl.workspace_floats)

    @torch.no_grad()
    def intrinsic_loss(self, z, a, keys, segments):
        """`segments` independent `pred_z(next(z, a))` passes and their similarity losses against `keys` over the row
        blocks [s B, (s + 1) B) of z [S B, L], a [S B, A], keys [S B, L] as one launch chain -> loss [S B]. Forward only.
        Each segment normalises `_predictor`'s BatchNorm over its own B rows and moves its running statistics once, in
        segment order: bitwise what S one-segment calls on the segments give."""
        z, a, keys, S, B = self._segments("intrinsic_loss", z, a, keys, segments)
        ws = self._segment_workspace("tdmpc_icem_intrinsic_workspace_floats", S, B)
        loss = z.new_empty(S * B)
        dtab = (C.c_void_p * len(self._dyn_params))(*[ptr(t) for t in self._dyn_params])
        ltab, nl = _table(self._loss_params, self._loss_stats)
        call("tdmpc_icem_intrinsic_fwd", self.dims, dtab, len(self._dyn_params), ltab, nl, z, a, keys, S, B, loss,
             ws, ws.numel(), torch.cuda.current_stream().cuda_stream)
        self.model._predictor[1].num_batches_tracked += S
        return loss

    @torch.no_grad()
    def intrinsic_rewards(self, z, a, keys, segments, rms, coef, reward, segmented=True):
        """The reference's `intrinsic_rewards` on the device: `intrinsic_loss` (segmented=False: as S one-segment calls,
        the same bits), then tdmpc_drnn_intrinsic_finish -> (intrinsic [S B], reward_pi [S B])."""
        if segmented:
            loss = self.intrinsic_loss(z, a, keys, segments)
        else:
            B = z.shape[0] // int(segments)
            loss = torch.cat([self.intrinsic_loss(z[s * B:(s + 1) * B], a[s * B:(s + 1) * B], keys[s * B:(s + 1) * B], 1)
                              for s in range(int(segments))])
        return intrinsic_finish(loss, rms, coef, reward)


class IcemMlpLearner(DssmLearner):
    """Owns the optimisers, the RunningMeanStd state and (in graph mode) the captured update graphs of one MLP iCEM
    agent (`agent`: cfg, model, model_target, device and, when it plans, planner). `step(buffer, noise)`: noise = 2H + 1
    [B, A] TruncatedNormal draws (H for the TD targets, H + 1 for update_pi) or None to draw on the device."""

    check_cfg = staticmethod(check_icem_learner_cfg)
    HIP_ENV = "TDMPC_ICEM_LEARNER_HIP"

    def _make_train_step(self, model, B, H):
        return IcemTrainStep(model, max_loss_rows=H * B, max_losses=self.MAX_LOSSES)

    def _intrinsic_kw(self):
        return dict(segmented=SEGMENTED)

    def _step_hip(self, buffer, noise):
        cfg, m, ts = self.cfg, self.agent.model, self.train_step
        H = int(cfg.horizon)
        # (:323-335 the intrinsic rewards, :286-292 the min target Q)
        (obs, _, action, reward, idxs, weights), z, nz_tg, intrinsic, reward_pi, next_q = self._hip_prelude(buffer, noise)
        B = obs.shape[0]
        zs = [z]
        for t in range(H):
            zs.append(m._dynamics(torch.cat([zs[-1], action[t]], dim=-1)))
        x = torch.cat([torch.stack(zs[:H]), action[:H]], dim=-1).view(H * B, -1)
        Q1, Q2, rp = m._Q1(x).view(H, B), m._Q2(x).view(H, B), m._reward(x).view(H, B)
        sim = ts.similarity_loss(zs[1:], nz_tg[:H * B])
        scal, rows, _ = _IcemFusedLoss.apply(
            sim.view(H, B), Q1, Q2, rp, reward[:H].reshape(H, B), reward_pi.view(H + 1, B)[:H], next_q, weights,
            (float(cfg.similarity_coef), float(cfg.reward_coef), float(cfg.value_coef), float(cfg.discount),
             float(cfg.rho)))
        grad_norm = self._optimize(scal[4], hook=False)              # (the 1 / H hook is in the kernel)
        return self._finish_hip(buffer, idxs, scal, rows, zs, noise, H, grad_norm, intrinsic)

    def _rollout_one(self, z, a):
        return self.agent.model.next(z, a)[0]

    def _step_torch(self, buffer, noise):
        cfg, m, mt = self.cfg, self.agent.model, self.agent.model_target
        H = int(cfg.horizon)
        obs, next_obses, action, reward, idxs, weights = buffer.sample()
        self.agent.optim.zero_grad(set_to_none=True)
        z = m.h(obs)
        next_zs = mt.h(next_obses)
        online_next_zs = m.h(next_obses)
        zs = [z.detach()]
        intrinsic = self._intrinsic_torch(obs, next_obses, action)
        reward_pi = self.coef * intrinsic + reward
        reward_loss, value_loss, priority_loss = 0, 0, 0
        queries, keys = [], []
        for t in range(H):
            rho = cfg.rho ** t
            Q1, Q2 = m.Q(z, action[t])
            z, reward_pred = m.next(z, action[t])
            with torch.no_grad():
                nz = online_next_zs[t]
                e = None if noise is None else noise[t]
                td = reward_pi[t] + cfg.discount * torch.min(*mt.Q(nz, m.pi(nz, cfg.min_std, eps=e)))
            reward_loss += F.mse_loss(reward_pred, reward[t], reduction="none") * rho
            value_loss += (F.mse_loss(Q1, td, reduction="none") + F.mse_loss(Q2, td, reduction="none")) * rho
            priority_loss += (F.l1_loss(Q1, td, reduction="none") + F.l1_loss(Q2, td, reduction="none")) * rho
            queries.append(z)
            keys.append(next_zs[t].detach())
            zs.append(z.detach())
        similarity_loss = 0 + self._similarity_torch(queries, keys, H)
        total_loss = cfg.similarity_coef * similarity_loss.clamp(max=1e4) + \
            cfg.reward_coef * reward_loss.clamp(max=1e4) + cfg.value_coef * value_loss.clamp(max=1e4)
        weighted = (total_loss * weights).mean()                    # the reference's [B, B] broadcast, literally
        grad_norm = self._optimize(weighted)
        return self._finish(buffer, idxs, priority_loss.clamp(max=1e4).detach(), zs, noise, H,
                            (similarity_loss.mean(), reward_loss.mean(), value_loss.mean(), total_loss.mean()),
                            weighted, grad_norm, intrinsic)
