"""The DSSM learner's two differentiable parts on HIP: `DSSM.next` in train mode and `similarity_loss`.

`DssmTrainStep(model, max_rows)` wraps the passes of include/tdmpc_drnn_learner.h (csrc/drnn_learner.hip) as
`torch.autograd.Function`s over a `tdmpc_amd.dssm.DSSM` on the GPU, so a DSSM update written in PyTorch runs its
recurrent step and its similarity loss on the hand-written kernels while autograd chains the steps through time:

    step = DssmTrainStep(model, max_rows=512)
    z1, h1, r1 = step.next(z0, a0, h0)          # DSSM.next under model.train(): batch-statistics BatchNorm
    loss = step.similarity_loss(z1, keys).mean() + r1.sum()
    loss.backward()                             # .grad of the 20 + 6 parameter tensors, as from the eager modules

The kernels read the model's own fp32 parameter tensors (no packed copy: they change every optimiser step), update the
BatchNorms' running statistics in place as `nn.BatchNorm1d` does, and run every reduction in a fixed order. Each live
`next` call (one whose backward has not run yet) holds one saved-activation buffer of the pool; the pool has
`max_steps` of them (default `cfg.horizon + 1`) and `max_losses` for the loss (default 2).

Two more pieces serve the DSSM update (tdmpc_amd/drnn_learner.py), both forward-only or elementwise:
`step.intrinsic_rewards(...)` runs `intrinsic_rewards`' H + 1 independent one-step rollouts and their similarity losses
as ONE launch chain whose BatchNorms normalise per segment of B rows (tdmpc_drnn_intrinsic_fwd), then normalises the
result against a device-resident float64 RunningMeanStd (tdmpc_drnn_intrinsic_finish) without a host round trip;
`_DssmFusedLoss` is the update's loss composition with its TD-lambda targets and its backward.

For the MPC agent's update (`TdMpcSimDssm.update`, tdmpc_amd/drnn_learner.py::DssmSimLearner):
`step.intrinsic_chain_rewards(...)` is the intrinsic-reward pass with ONE hidden state carried through the H + 1
closed-loop steps (tdmpc_drnn_intrinsic_chain_fwd; `chain_mode` 0 runs the recurrence as a launch chain, 1 in one
launch; the default is TDMPC_DSSM_CHAIN_MODE or CHAIN_MODE below), and `_DssmSimFusedLoss` that update's loss composition.

`LossStep` is what `DssmTrainStep` shares with the MLP iCEM agent's `icem_learner.IcemTrainStep` (`similarity_loss`, the
operand checks, the segmented passes' workspaces), and `_StepFusedLoss` the one body of the three updates' fused loss
Functions (`_DssmFusedLoss`, `_DssmSimFusedLoss`, `icem_learner._IcemFusedLoss`).

There is no eager fall-back: a missing library or an unsupported shape raises. The update itself (optimisers, replay,
the encoder / Q / pi passes) is `tdmpc_amd.drnn_learner.DssmLearner`.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib
from ._lib import DrnnLossArgs, DrnnSimLossArgs, DrnnTrainSizes, call, drnn_dims_from_cfg, ptr

CHAIN_MODE = 1   # the recurrence of intrinsic_chain_loss: the faster form at the bench shape

NEXT_PARAMS = tuple(f"_dynamics.prior_mlp.{k}" for k in ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight",
                                                         "3.bias")) + \
    tuple(f"_dynamics.gru_cell.{k}" for k in ("weight_ih.weight", "weight_hh.weight", "ln_reset.weight",
                                              "ln_reset.bias", "ln_update.weight", "ln_update.bias",
                                              "ln_newval.weight", "ln_newval.bias")) + \
    tuple(f"_reward.{k}" for k in ("0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"))
LOSS_PARAMS = tuple(f"_predictor.{k}" for k in ("0.weight", "0.bias", "1.weight", "1.bias", "3.weight", "3.bias"))
_STATS_AT = 4   # running_mean / running_var follow the BatchNorm's weight and bias in state_dict order


def _table(params, stats):
    """The C pointer table: the parameters with the BatchNorm's running statistics at slots 4 and 5."""
    ts = list(params[:_STATS_AT]) + list(stats) + list(params[_STATS_AT:])
    return (C.c_void_p * len(ts))(*[ptr(t) for t in ts]), len(ts)


class _Slot:
    """One saved-activation buffer of a pool, handed back when the backward has run or the graph is dropped."""
    live = False

    def __init__(self, pool, what):
        if not pool.free:
            raise RuntimeError(
                f"DssmTrainStep: more than {len(pool.bufs)} {what} calls are live (forward done, backward pending); "
                f"construct it with a larger {pool.knob}")
        self.pool, self.idx = pool, pool.free.pop()
        self.buf = pool.bufs[self.idx]
        self.live = True

    def release(self):
        if self.live:
            self.live = False
            self.pool.free.append(self.idx)

    def __del__(self):
        self.release()


class _Pool:
    def __init__(self, n, floats, device, knob):
        self.bufs = [torch.empty(floats, dtype=torch.float32, device=device) for _ in range(n)]
        self.free = list(range(n))[::-1]
        self.knob = knob


def _f32c(t):
    return None if t is None else t.detach().to(torch.float32).contiguous()


class _NextFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, step, z, a, h, *params):
        z, a, h = _f32c(z), _f32c(a), _f32c(h)
        R = z.shape[0]
        slot = _Slot(step._next_pool, "next")
        zo, ho, ro = z.new_empty(R, step.L), z.new_empty(R, step.Hd), z.new_empty(R)
        tab, n = _table(params, step._next_stats)
        try:
            call("tdmpc_drnn_next_fwd", step.dims, tab, n, z, a, h, R, zo, ho, ro, slot.buf, slot.buf.numel(),
                 step._ws, step._ws.numel(), torch.cuda.current_stream().cuda_stream)
        except Exception:
            slot.release()
            raise
        ctx.step, ctx.slot = step, slot
        ctx.save_for_backward(z, a, h, *params)
        ctx.set_materialize_grads(False)
        return zo, ho, ro

    @staticmethod
    def backward(ctx, dzo, dho, dro):
        step, slot = ctx.step, ctx.slot
        if not slot.live:
            raise RuntimeError("DssmTrainStep.next: this call's saved activations were released by an earlier backward")
        z, a, h, *params = ctx.saved_tensors
        R = z.shape[0]
        dzo, dho, dro = _f32c(dzo), _f32c(dho), _f32c(dro)
        need = ctx.needs_input_grad
        dz, da, dh = (torch.empty_like(t) if need[1 + i] else None for i, t in enumerate((z, a, h)))
        grads = [torch.empty_like(p) for p in params]
        tab, n = _table(params, step._next_stats)
        gtab, _ = _table(grads, (None, None))
        call("tdmpc_drnn_next_bwd", step.dims, tab, n, z, a, h, R, slot.buf, slot.buf.numel(), ptr(dzo), ptr(dho),
             ptr(dro), ptr(dz), ptr(da), ptr(dh), gtab, step._ws, step._ws.numel(),
             torch.cuda.current_stream().cuda_stream)
        slot.release()
        return (None, dz, da, dh) + tuple(g if need[4 + i] else None for i, g in enumerate(grads))


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, step, q, k, *params):
        q, k = _f32c(q), _f32c(k)
        R = q.shape[0]
        slot = _Slot(step._loss_pool, "similarity_loss")
        loss = q.new_empty(R)
        tab, n = _table(params, step._loss_stats)
        try:
            call(step.LOSS_ABI + "fwd", step.dims, tab, n, q, k, R, loss, slot.buf, slot.buf.numel(), step._ws,
                 step._ws.numel(), torch.cuda.current_stream().cuda_stream)
        except Exception:
            slot.release()
            raise
        ctx.step, ctx.slot = step, slot
        ctx.save_for_backward(q, k, *params)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        step, slot = ctx.step, ctx.slot
        if not slot.live:
            raise RuntimeError("DssmTrainStep.similarity_loss: this call's saved activations were released by an "
                               "earlier backward")
        q, k, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        dq = torch.empty_like(q) if need[1] else None
        grads = [torch.empty_like(p) for p in params]
        tab, n = _table(params, step._loss_stats)
        gtab, _ = _table(grads, (None, None))
        call(step.LOSS_ABI + "bwd", step.dims, tab, n, q, k, q.shape[0], slot.buf, slot.buf.numel(),
             _f32c(dloss), ptr(dq), gtab, step._ws, step._ws.numel(), torch.cuda.current_stream().cuda_stream)
        slot.release()
        return (None, dq, None) + tuple(g if need[3 + i] else None for i, g in enumerate(grads))


class _StepFusedLoss(torch.autograd.Function):
    """One update's loss composition and its backward as HIP kernels (`ABI`loss_forward / _backward), written once for
    the three variants below: forward(sim [H, B], q1, q2, rp, rw, rwpi, nq [N, B], w [B], coefs) -> (scal [SCAL],
    rows [ROWS, B], td [N, B]); N = H unless the variant is SHOOT. Only scal[4] (the weighted loss) carries a gradient,
    to sim, q1, q2 and rp. A variant names its entry points, its ctypes struct and `_args`, how H / N / B go into it."""

    ABI = ARGS = ROWS = SCAL = None
    SHOOT = False   # q1 .. nq cover the N = H - W shoot steps only

    @classmethod
    def _args(cls, ins, H, N, B, coefs):
        return cls.ARGS(*[t.data_ptr() for t in ins], H, B, *[float(c) for c in coefs])

    @classmethod
    def forward(cls, ctx, sim, q1, q2, rp, rw, rwpi, nq, w, coefs):
        H, B = sim.shape
        N = q1.shape[0] if cls.SHOOT else H
        ins = [_f32c(t) for t in (sim, q1, q2, rp, rw, rwpi, nq, w)]
        if cls.SHOOT and not 1 <= N < H:
            raise ValueError(f"{cls.__name__}: {N} shoot steps of {H} (1 <= horizon - warmup_len <= horizon - 1)")
        for t in ins[1:7]:
            if tuple(t.shape) != (N, B):
                raise ValueError(f"{cls.__name__}: {'q1 .. nq' if cls.SHOOT else 'every operand but w'} must be "
                                 f"[{N}, {B}], got {tuple(t.shape)}")
        if tuple(ins[7].shape) != (B,):
            raise ValueError(f"{cls.__name__}: w must be [{B}], got {tuple(ins[7].shape)}")
        td, rows, scal = sim.new_empty(N, B), sim.new_empty(cls.ROWS, B), sim.new_empty(cls.SCAL)
        call(cls.ABI + "loss_forward", cls._args(ins, H, N, B, coefs), td, rows, scal,
             torch.cuda.current_stream().cuda_stream)
        ctx.save_for_backward(*ins, td, rows, scal)
        ctx.coefs = coefs
        ctx.mark_non_differentiable(rows, td)
        return scal, rows, td

    @classmethod
    def backward(cls, ctx, g_scal, g_rows, g_td):
        *ins, td, rows, scal = ctx.saved_tensors
        (H, B), N = ins[0].shape, ins[1].shape[0]
        g = g_scal.contiguous()
        need = ctx.needs_input_grad
        dsim, dq1, dq2, drp = (torch.empty_like(ins[i]) if need[i] else None for i in range(4))
        call(cls.ABI + "loss_backward", cls._args(ins, H, N, B, ctx.coefs), td, rows, scal, g.data_ptr() + 16, ptr(dsim),
             ptr(dq1), ptr(dq2), ptr(drp), torch.cuda.current_stream().cuda_stream)
        return dsim, dq1, dq2, drp, None, None, None, None, None


class _DssmFusedLoss(_StepFusedLoss):
    """TdICemSimDssm.update's loss composition (tdmpc_icem_similarity_drnn.py:471-485, :497-499, :522-530): coefs =
    (similarity_coef, reward_coef, value_coef, discount, td_lambda); scal = (mean similarity, mean reward, mean value,
    mean total, weighted, mean w, mean model_loss, mean td_loss), rows = (similarity, reward, value, clamped priority,
    model_loss, td_loss) per batch row, td = the TD-lambda targets."""
    ABI, ARGS, ROWS, SCAL = "tdmpc_drnn_", DrnnLossArgs, 6, 8


class _DssmSimFusedLoss(_StepFusedLoss):
    """TdMpcSimDssm.update's loss composition (tdmpc_similarity_drnn.py:447-471): q1 .. nq over the H - W shoot steps;
    coefs = (similarity_coef, reward_coef, value_coef, discount); scal = (mean similarity, mean reward, mean value,
    mean total, weighted = mean(total) mean(w), mean w), rows = (similarity, reward, value, clamped priority, total) per
    batch row, td = the one-step TD targets."""
    ABI, ARGS, ROWS, SCAL, SHOOT = "tdmpc_drnn_sim_", DrnnSimLossArgs, 5, 6, True

    @classmethod
    def _args(cls, ins, H, N, B, coefs):
        return cls.ARGS(*[t.data_ptr() for t in ins], H, H - N, B, *[float(c) for c in coefs])


def new_rms_state(device):
    """gym's RunningMeanStd() as a float64 [mean, var, count] tensor (tdmpc_drnn_intrinsic_finish's device state)."""
    return torch.tensor([0.0, 1.0, 1e-4], dtype=torch.float64, device=device)


@torch.no_grad()
def intrinsic_finish(loss, rms, coef, reward):
    """tdmpc_drnn_intrinsic_finish: the RunningMeanStd update of `rms` from the losses' mean and population variance,
    then (intrinsic, reward_pi) -- see DssmTrainStep.intrinsic_rewards."""
    if rms.dtype != torch.float64 or rms.numel() != 3 or not rms.is_cuda or not rms.is_contiguous():
        raise ValueError("intrinsic_finish: rms must be new_rms_state()'s float64 [3] device tensor")
    loss, reward = _f32c(loss).view(-1), _f32c(reward).view(-1)
    if reward.numel() != loss.numel() or coef.dtype != torch.float32 or not coef.is_cuda:
        raise ValueError("intrinsic_finish: reward must match the losses and coef be a float32 device scalar")
    intrinsic, reward_pi = torch.empty_like(loss), torch.empty_like(loss)
    call("tdmpc_drnn_intrinsic_finish", loss, loss.numel(), rms, coef, reward, intrinsic, reward_pi,
         torch.cuda.current_stream().cuda_stream)
    return intrinsic, reward_pi


class LossStep:
    """What the train steps of the similarity learners share (`DssmTrainStep`; `icem_learner.IcemTrainStep`): the
    reference's `similarity_loss` on HIP, differentiable in the queries and `_predictor`'s parameters (entry points
    LOSS_ABI + fwd / bwd), with its saved-activation pool and workspace; the checks of every pass's operands; the
    workspaces of the segmented intrinsic-reward passes."""

    LOSS_ABI = None

    def __init__(self, model, dims, max_loss_rows):
        self.device = next(model.parameters()).device
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}: the model must be on the GPU (there is no CPU path)")
        self.model, self.cfg, self.dims = model, model.cfg, dims
        self.L, self.A = int(model.cfg.latent_dim), int(model.cfg.action_dim)
        self.max_loss_rows = int(max_loss_rows)
        self._loss_params = self._params(LOSS_PARAMS)
        bufs = dict(model.named_buffers())
        self._loss_stats = (bufs["_predictor.1.running_mean"], bufs["_predictor.1.running_var"])
        self._seg_ws = {}   # (entry point, segments, rows per segment) -> the workspace of a segmented pass

    def _params(self, names):
        named = dict(self.model.named_parameters())
        params = tuple(named[k] for k in names)
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"{type(self).__name__}: the model's parameters must be contiguous float32")
        return params

    def _loss_buffers(self, max_losses, saved_floats, workspace_floats):
        self._loss_pool = _Pool(int(max_losses), saved_floats, self.device, "max_losses")
        self._ws = torch.empty(workspace_floats, dtype=torch.float32, device=self.device)

    def _check(self, what, rows, cap, *shaped):
        name = type(self).__name__
        if not self.model.training:
            raise RuntimeError(f"{name}.{what}: the model is in eval() mode; these passes run the BatchNorms on "
                               "batch statistics (model.train()). For inference use DrnnPlanner.next")
        if rows > cap:
            raise ValueError(f"{name}.{what}: {rows} rows, sized for {cap}")
        for arg, t, width in shaped:
            if t.dim() != 2 or t.shape[0] != rows or t.shape[1] != width or not t.is_cuda:
                raise ValueError(f"{name}.{what}: {arg} must be a GPU tensor of shape [{rows}, {width}], got "
                                 f"{tuple(t.shape)} on {t.device}")

    def similarity_loss(self, queries, keys):
        """The reference's `similarity_loss(queries, keys)` -> [R]: 2 - 2 cos(_predictor(queries), keys) per row, the
        keys detached. `queries` and `keys` may be lists of per-step [B, L] tensors (concatenated, as the reference does)."""
        if isinstance(queries, (list, tuple)):
            queries = torch.cat(list(queries), dim=0)
        if isinstance(keys, (list, tuple)):
            keys = torch.cat(list(keys), dim=0)
        self._check("similarity_loss", queries.shape[0], self.max_loss_rows, ("queries", queries, self.L),
                    ("keys", keys, self.L))
        loss = _LossFn.apply(self, queries, keys.detach(), *self._loss_params)
        self.model._predictor[1].num_batches_tracked += 1
        return loss

    def _segments(self, what, z, a, keys, segments):
        """The operands of a segmented pass over the row blocks [s B, (s + 1) B) of z [S B, L], a [S B, A] and keys
        [S B, L], checked -> (z, a, keys as contiguous float32, S, B)."""
        R, S = z.shape[0], int(segments)
        if S < 1 or R % S:
            raise ValueError(f"{type(self).__name__}.{what}: {R} rows do not split into {S} segments")
        self._check(what, R, _lib.DT_MAX_ROWS, ("z", z, self.L), ("a", a, self.A), ("keys", keys, self.L))
        return _f32c(z), _f32c(a), _f32c(keys), S, R // S

    def _segment_workspace(self, entry, S, B):
        """The workspace of a pass over S segments of B rows, sized by the entry point `entry` and kept."""
        ws = self._seg_ws.get((entry, S, B))
        if ws is None:
            n = C.c_size_t()
            call(entry, self.dims, S, B, C.byref(n))
            ws = self._seg_ws[(entry, S, B)] = torch.empty(n.value, dtype=torch.float32, device=self.device)
        return ws


class DssmTrainStep(LossStep):
    """Differentiable `DSSM.next` (train mode) and `similarity_loss` on HIP for `model` (a `tdmpc_amd.dssm.DSSM` on the
    GPU, fp32). max_rows: the largest batch of `next`; max_loss_rows: of `similarity_loss` (default
    min(4096, max_rows * max_steps): the reference concatenates the per-step predictions)."""

    LOSS_ABI = "tdmpc_drnn_simloss_"

    def __init__(self, model, max_rows: int, max_steps: int | None = None, max_loss_rows: int | None = None,
                 max_losses: int = 2):
        cfg = model.cfg
        self.max_rows = int(max_rows)
        self.max_steps = int(max_steps if max_steps is not None else cfg.horizon + 1)
        super().__init__(model, drnn_dims_from_cfg(cfg), max_loss_rows if max_loss_rows is not None
                         else min(_lib.DT_MAX_ROWS, self.max_rows * self.max_steps))
        self.Hd = int(cfg.hidden_dim)
        if _lib.lib().tdmpc_drnn_train_version() != _lib.DRNN_TRAIN_VERSION:
            raise RuntimeError("libtdmpc_hip: tdmpc_drnn_train_version mismatch")
        sn, sl = DrnnTrainSizes(), DrnnTrainSizes()
        call("tdmpc_drnn_train_sizes_for", self.dims, self.max_rows, sn)
        call("tdmpc_drnn_train_sizes_for", self.dims, self.max_loss_rows, sl)
        self._next_params = self._params(NEXT_PARAMS)
        bufs = dict(model.named_buffers())
        self._next_stats = (bufs["_dynamics.prior_mlp.1.running_mean"], bufs["_dynamics.prior_mlp.1.running_var"])
        self._next_pool = _Pool(self.max_steps, sn.next_saved_floats, self.device, "max_steps")
        self._loss_buffers(max_losses, sl.loss_saved_floats, max(sn.workspace_floats, sl.workspace_floats))
        self.chain_mode = int(os.environ.get("TDMPC_DSSM_CHAIN_MODE", CHAIN_MODE))

    def next(self, z, a, h):
        """`DSSM.next(z, a, h)` under `model.train()`: (z' [R, L], h' [R, Hd], r [R, 1]), differentiable in z, a, h and
        the 20 parameter tensors of `_dynamics` and `_reward`. Moves prior_mlp's running statistics."""
        self._check("next", z.shape[0], self.max_rows, ("z", z, self.L), ("a", a, self.A), ("h", h, self.Hd))
        zo, ho, ro = _NextFn.apply(self, z, a, h, *self._next_params)
        self.model._dynamics.prior_mlp[1].num_batches_tracked += 1
        return zo, ho, ro.unsqueeze(1)

    @torch.no_grad()
    def intrinsic_loss(self, z, a, keys, segments):
        """`segments` independent `next(z, a, 0)` + `similarity_loss(z', keys)` passes over the row blocks
        [s B, (s + 1) B) of z [S B, L], a [S B, A], keys [S B, L] as one launch chain -> loss [S B]. Forward only. Each
        segment normalises both BatchNorms over its own B rows and moves their running statistics once, in segment
        order: bitwise what S pairs of `next` / `similarity_loss` calls on the segments give."""
        z, a, keys, S, B = self._segments("intrinsic_loss", z, a, keys, segments)
        ws = self._segment_workspace("tdmpc_drnn_intrinsic_workspace_floats", S, B)
        loss = z.new_empty(S * B)
        ntab, nn_ = _table(self._next_params, self._next_stats)
        ltab, nl = _table(self._loss_params, self._loss_stats)
        call("tdmpc_drnn_intrinsic_fwd", self.dims, ntab, nn_, ltab, nl, z, a, keys, S, B, loss, ws, ws.numel(),
             torch.cuda.current_stream().cuda_stream)
        self.model._dynamics.prior_mlp[1].num_batches_tracked += S
        self.model._predictor[1].num_batches_tracked += S
        return loss

    @torch.no_grad()
    def intrinsic_rewards(self, z, a, keys, segments, rms, coef, reward):
        """The reference's `intrinsic_rewards` on the device: `intrinsic_loss`, then the RunningMeanStd update of `rms`
        (`new_rms_state`) from the losses' mean and population variance and intrinsic = max(loss / sqrt(var) -
        mean / sqrt(var), 0) -> (intrinsic [S B], reward_pi [S B] = coef * intrinsic + reward). coef: a one-element
        float32 device tensor (the explore schedule's value of this step); reward [S B]."""
        return intrinsic_finish(self.intrinsic_loss(z, a, keys, segments), rms, coef, reward)

    @torch.no_grad()
    def intrinsic_chain_loss(self, z, a, keys, segments, warm, mode=None, hidden=False):
        """`TdMpcSimDssm.intrinsic_rewards`' model uncertainty (similarity_horizon 1) -> loss [S B]: one hidden state
        runs from zeros through the S closed-loop steps `next(z[s], a[s], h)`; the first `warm` steps only advance it
        (loss 0 there, but prior_mlp's BatchNorm statistics move), the others compare `pred_z(z')` with keys[s]. mode: 0
        the recurrence as a launch chain (bitwise S `next` calls + `similarity_loss` on the later segments), 1 in one
        launch; default `self.chain_mode`. hidden=True: -> (loss, h_out [B, Hd], every segment's hidden state
        [S, B, Hd], a view of the workspace that the next call overwrites)."""
        z, a, keys, S, B = self._segments("intrinsic_chain_loss", z, a, keys, segments)
        R, W = S * B, int(warm)
        if not 0 <= W < S:
            raise ValueError(f"DssmTrainStep.intrinsic_chain_loss: warm={W} is not in [0, {S})")
        ws = self._segment_workspace("tdmpc_drnn_intrinsic_chain_workspace_floats", S, B)
        loss, h_out = z.new_empty(R), z.new_empty(B, self.Hd)
        ntab, nn_ = _table(self._next_params, self._next_stats)
        ltab, nl = _table(self._loss_params, self._loss_stats)
        call("tdmpc_drnn_intrinsic_chain_fwd", self.dims, ntab, nn_, ltab, nl, z, a, keys, S, B, W,
             self.chain_mode if mode is None else int(mode), loss, h_out, ws, ws.numel(),
             torch.cuda.current_stream().cuda_stream)
        self.model._dynamics.prior_mlp[1].num_batches_tracked += S
        self.model._predictor[1].num_batches_tracked += S - W
        return (loss, h_out, ws[:R * self.Hd].view(S, B, self.Hd)) if hidden else loss

    @torch.no_grad()
    def intrinsic_chain_rewards(self, z, a, keys, segments, warm, rms, coef, reward):
        """`TdMpcSimDssm.intrinsic_rewards` on the device: `intrinsic_chain_loss`, then `intrinsic_finish` over all
        S B values (the zero rows of the warm-up segments enter the moments, as in the reference) ->
        (intrinsic [S B], reward_pi [S B])."""
        return intrinsic_finish(self.intrinsic_chain_loss(z, a, keys, segments, warm), rms, coef, reward)
