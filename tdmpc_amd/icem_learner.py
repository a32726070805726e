"""The MLP iCEM agent's learner: `TdICemSimMlp.update / update_pi / intrinsic_rewards` on the GPU.

Reference: src/algorithm/tdmpc_icem_similarity_mlp.py:267-284 (update_pi), :286-292 (_td_target), :294-300
(similarity_loss), :313-344 (model_rollout, intrinsic_rewards), :346-428 (update). The math is the reference's
(tests/icem_update_ref.py restates it and is pinned bit for bit to the reference on the CPU;
tests/test_gpu_icem_update.py holds this module to it), including its quirks: one-step TD targets from `reward +
explore_coef * intrinsic` at the online next latents under the online policy with the target Q; reward, value and
priority terms weighted by `rho ** t`, the similarity term and `update_pi` not; `(total_loss [B, 1] * weights [B])
.mean()`, a mean over the [B, B] broadcast (= mean(total) * mean(weights)); the gradient of the weighted loss divided by
the horizon; intrinsic rewards normalised by a running mean / std.

`IcemMlpLearner(DssmLearner)` shares the optimisers, `update_pi`, the EMA, the RunningMeanStd state and the graph driver
with the DSSM learners (tdmpc_amd/drnn_learner.py) and has their two paths.

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
pinned); moving them onto tdmpc_lg_gemm / tdmpc_lg_rows_* is the follow-up.

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
from .drnn_learner import DssmLearner, rms_normalize, rms_update
from .dssm_train import LOSS_PARAMS, DssmTrainStep, _f32c, _Pool, _table, intrinsic_finish
from .learner import clip_grad_norm_19

DYN_PARAMS = tuple(f"_dynamics.{k}" for k in ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"))
SEGMENTED = True   # `step`'s intrinsic pass: one segmented call (the faster form) or S one-segment calls


def check_icem_learner_cfg(cfg):
    """Raise for what the MLP iCEM learner does not cover, each setting named, before anything touches the device."""
    if getattr(cfg, "modality", "state") != "state":
        raise NotImplementedError(f"IcemMlpLearner: modality={cfg.modality!r} is not supported (state observations only)")
    if not getattr(cfg, "normalize", True):
        raise NotImplementedError("IcemMlpLearner: normalize=False is not supported (the BatchNorm-free predictor and "
                                  "the plain encoder)")
    if getattr(cfg, "norm_type", "ln") != "ln":
        raise NotImplementedError(f"IcemMlpLearner: norm_type={cfg.norm_type!r} is not supported ('ln' only)")
    B, H, L, M = int(cfg.batch_size), int(cfg.horizon), int(cfg.latent_dim), int(cfg.mlp_dim)
    if M != 512:
        raise ValueError(f"IcemMlpLearner: mlp_dim={M} is not supported (512 only)")
    if L > 256:
        raise ValueError(f"IcemMlpLearner: latent_dim={L} is not supported (at most 256)")
    if B < 2:
        raise ValueError(f"IcemMlpLearner: batch_size={B} is not supported (train-mode BatchNorm needs two rows)")
    if (H + 1) * B > _lib.DT_MAX_ROWS:
        raise ValueError(f"IcemMlpLearner: (horizon + 1) * batch_size = {(H + 1) * B} rows exceed {_lib.DT_MAX_ROWS} "
                         f"(horizon={H}, batch_size={B}): the intrinsic-reward pass and its normalisation take at most "
                         f"that many rows")
    if str(getattr(cfg, "optim_id", "adamw")).lower() not in ("adam", "adamw"):
        raise ValueError(f"IcemMlpLearner: optim_id={cfg.optim_id!r} is not supported ('adam' or 'adamw')")


class _IcemFusedLoss(torch.autograd.Function):
    """TdICemSimMlp.update's loss composition (:384-411) and its backward as HIP kernels (tdmpc_icem_loss_forward /
    _backward): forward(sim, q1, q2, rp, rw, rwpi, nq [H, B], w [B], coefs = (similarity_coef, reward_coef, value_coef,
    discount, rho)) -> (scal [6], rows [5, B], td [H, B]); scal = (mean similarity, mean reward, mean value, mean total,
    weighted = mean(total) mean(w), mean w), rows = (similarity, reward, value, clamped priority, total) per batch row,
    td = the one-step TD targets. Only scal[4] carries a gradient, to sim, q1, q2 and rp, and that gradient includes the
    reference's hook: it is divided by H."""

    @staticmethod
    def _args(ins, H, B, coefs):
        return IcemLossArgs(*[t.data_ptr() for t in ins], H, B, *[float(c) for c in coefs])

    @staticmethod
    def forward(ctx, sim, q1, q2, rp, rw, rwpi, nq, w, coefs):
        H, B = sim.shape
        ins = [_f32c(t) for t in (sim, q1, q2, rp, rw, rwpi, nq, w)]
        for t in ins[:7]:
            if tuple(t.shape) != (H, B):
                raise ValueError(f"_IcemFusedLoss: every operand but w must be [{H}, {B}], got {tuple(t.shape)}")
        if tuple(ins[7].shape) != (B,):
            raise ValueError(f"_IcemFusedLoss: w must be [{B}], got {tuple(ins[7].shape)}")
        td, rows, scal = sim.new_empty(H, B), sim.new_empty(5, B), sim.new_empty(6)
        call("tdmpc_icem_loss_forward", _IcemFusedLoss._args(ins, H, B, coefs), td, rows, scal,
             torch.cuda.current_stream().cuda_stream)
        ctx.save_for_backward(*ins, td, rows, scal)
        ctx.coefs = coefs
        ctx.mark_non_differentiable(rows, td)
        return scal, rows, td

    @staticmethod
    def backward(ctx, g_scal, g_rows, g_td):
        *ins, td, rows, scal = ctx.saved_tensors
        H, B = ins[0].shape
        g = g_scal.contiguous()
        need = ctx.needs_input_grad
        dsim, dq1, dq2, drp = (torch.empty_like(ins[i]) if need[i] else None for i in range(4))
        call("tdmpc_icem_loss_backward", _IcemFusedLoss._args(ins, H, B, ctx.coefs), td, rows, scal,
             g.data_ptr() + 16, ptr(dsim), ptr(dq1), ptr(dq2), ptr(drp), torch.cuda.current_stream().cuda_stream)
        return dsim, dq1, dq2, drp, None, None, None, None, None


class IcemTrainStep(DssmTrainStep):
    """The HIP parts of the MLP iCEM update for `model` (a `tdmpc_amd.icem_mlp.IcemMlpModel` on the GPU, fp32):
    `similarity_loss` (DssmTrainStep's, through tdmpc_icem_simloss_*), `intrinsic_loss` / `intrinsic_rewards`.
    max_loss_rows: the most rows of one `similarity_loss`."""

    LOSS_ABI = "tdmpc_icem_simloss_"

    def __init__(self, model, max_loss_rows: int, max_losses: int = 1):
        cfg = model.cfg
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("IcemTrainStep: the model must be on the GPU (there is no CPU path)")
        self.model, self.cfg = model, cfg
        self.L, self.A = int(cfg.latent_dim), int(cfg.action_dim)
        self.max_loss_rows = int(max_loss_rows)
        self.dims = dims_from_cfg(cfg, enc_norm=True)
        if _lib.lib().tdmpc_icem_learner_version() != _lib.ICEM_LEARNER_VERSION:
            raise RuntimeError("libtdmpc_hip: tdmpc_icem_learner_version mismatch")
        sl = IcemSimlossSizes()
        call("tdmpc_icem_simloss_sizes_for", self.dims, self.max_loss_rows, sl)
        named, bufs = dict(model.named_parameters()), dict(model.named_buffers())
        self._dyn_params = tuple(named[k] for k in DYN_PARAMS)
        self._loss_params = tuple(named[k] for k in LOSS_PARAMS)
        for p in self._dyn_params + self._loss_params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("IcemTrainStep: the model's parameters must be contiguous float32")
        self._loss_stats = (bufs["_predictor.1.running_mean"], bufs["_predictor.1.running_var"])
        self._loss_pool = _Pool(int(max_losses), sl.loss_saved_floats, dev, "max_losses")
        self._ws = torch.empty(sl.workspace_floats, dtype=torch.float32, device=dev)
        self._iws = {}   # (segments, rows per segment) -> the workspace of intrinsic_loss

    def next(self, *a, **k):
        raise NotImplementedError("IcemTrainStep: the MLP dynamics run on PyTorch autograd (model.next)")

    intrinsic_chain_loss = intrinsic_chain_rewards = next

    @torch.no_grad()
    def intrinsic_loss(self, z, a, keys, segments):
        """`segments` independent `pred_z(next(z, a))` passes and their similarity losses against `keys` over the row
        blocks [s B, (s + 1) B) of z [S B, L], a [S B, A], keys [S B, L] as one launch chain -> loss [S B]. Forward only.
        Each segment normalises `_predictor`'s BatchNorm over its own B rows and moves its running statistics once, in
        segment order: bitwise what S one-segment calls on the segments give."""
        R = z.shape[0]
        S = int(segments)
        if S < 1 or R % S:
            raise ValueError(f"IcemTrainStep.intrinsic_loss: {R} rows do not split into {S} segments")
        self._check("intrinsic_loss", R, _lib.DT_MAX_ROWS, ("z", z, self.L), ("a", a, self.A), ("keys", keys, self.L))
        z, a, keys = _f32c(z), _f32c(a), _f32c(keys)
        ws = self._iws.get((S, R // S))
        if ws is None:
            n = C.c_size_t()
            call("tdmpc_icem_intrinsic_workspace_floats", self.dims, S, R // S, C.byref(n))
            ws = self._iws[(S, R // S)] = torch.empty(n.value, dtype=torch.float32, device=z.device)
        loss = z.new_empty(R)
        dtab = (C.c_void_p * len(self._dyn_params))(*[ptr(t) for t in self._dyn_params])
        ltab, nl = _table(self._loss_params, self._loss_stats)
        call("tdmpc_icem_intrinsic_fwd", self.dims, dtab, len(self._dyn_params), ltab, nl, z, a, keys, S, R // S, loss,
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

    def _step_hip(self, buffer, noise):
        a, cfg, m, mt, ts = self.agent, self.cfg, self.agent.model, self.agent.model_target, self.train_step
        H = int(cfg.horizon)
        obs, next_obses, action, reward, idxs, weights = buffer.sample()
        B = obs.shape[0]
        a.optim.zero_grad(set_to_none=True)
        z = m.h(obs)
        with torch.no_grad():
            flat = next_obses.reshape((H + 1) * B, -1)
            nz_on, nz_tg = m.h(flat), mt.h(flat)                    # [(H + 1) B, L]: online, target
            # :323-335: rollout t starts at z_traj[t] = (z, online next latents)[t] and is compared with target[t]
            z_traj = torch.cat([z.detach(), nz_on[:H * B]])
            intrinsic, reward_pi = ts.intrinsic_rewards(z_traj, action.reshape((H + 1) * B, -1), nz_tg, H + 1,
                                                        self.rms, self.coef, reward.reshape(-1), segmented=SEGMENTED)
            # :286-292: min target Q at the online next latents under the online policy, every step at once
            x = nz_on[:H * B]
            act = m.pi(x, cfg.min_std, eps=None if noise is None else torch.cat(list(noise[:H])))
            next_q = torch.min(*mt.Q(x, act)).view(H, B)
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
        weighted = scal[4]
        weighted.backward()                                          # (the 1 / H hook is in the kernel)
        grad_norm = clip_grad_norm_19(self.params, cfg.grad_clip_norm)
        a.optim.step()
        return self._finish(buffer, idxs, rows[3].view(B, 1), [t.detach() for t in zs], noise, H,
                            (scal[0], scal[1], scal[2], scal[3]), weighted, grad_norm, intrinsic.view(H + 1, B, 1))

    def _intrinsic_torch(self, obs, next_obses, action):
        """:323-344 call by call (H + 1 train-mode `next` + `pred_z` passes), the RunningMeanStd by `rms_update`."""
        m, mt, H = self.agent.model, self.agent.model_target, int(self.cfg.horizon)
        with torch.no_grad():
            zs_target = mt.h(next_obses)
            z_traj = m.h(torch.cat([obs.unsqueeze(0), next_obses], dim=0))
            out = []
            for t in range(H + 1):
                zl, _ = m.next(z_traj[t], action[t])
                pred = F.normalize(m.pred_z(zl).unsqueeze(0), dim=-1, p=2)
                target = F.normalize(zs_target[t:t + 1], dim=-1, p=2)
                out.append((2.0 - 2.0 * (pred * target).sum(dim=-1, keepdim=True))[0])
            raw = torch.stack(out)                                   # [H + 1, B, 1]
            rms_update(self.rms, raw)
            return rms_normalize(self.rms, raw)

    def _step_torch(self, buffer, noise):
        a, cfg, m, mt = self.agent, self.cfg, self.agent.model, self.agent.model_target
        H = int(cfg.horizon)
        obs, next_obses, action, reward, idxs, weights = buffer.sample()
        B = obs.shape[0]
        a.optim.zero_grad(set_to_none=True)
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
        q = F.normalize(m.pred_z(torch.cat(queries, dim=0)), dim=-1, p=2)
        k = F.normalize(torch.cat(keys, dim=0), dim=-1, p=2)
        similarity_loss = 0 + (2.0 - 2.0 * (q * k).sum(dim=-1)).reshape(H, B, -1).sum(dim=0)
        total_loss = cfg.similarity_coef * similarity_loss.clamp(max=1e4) + \
            cfg.reward_coef * reward_loss.clamp(max=1e4) + cfg.value_coef * value_loss.clamp(max=1e4)
        weighted = (total_loss * weights).mean()                    # the reference's [B, B] broadcast, literally
        weighted.register_hook(lambda grad: grad * (1 / H))
        weighted.backward()
        grad_norm = clip_grad_norm_19(self.params, cfg.grad_clip_norm)
        a.optim.step()
        return self._finish(buffer, idxs, priority_loss.clamp(max=1e4).detach(), zs, noise, H,
                            (similarity_loss.mean(), reward_loss.mean(), value_loss.mean(), total_loss.mean()),
                            weighted, grad_norm, intrinsic)
