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


class _DssmFusedLoss(torch.autograd.Function):
    """TdICemSimDssm.update's loss composition (tdmpc_icem_similarity_drnn.py:471-485, :497-499, :522-530) and its
    backward as HIP kernels (tdmpc_drnn_loss_forward / _backward): forward(sim, q1, q2, rp, rw, rwpi, nq [H, B], w [B],
    coefs = (similarity_coef, reward_coef, value_coef, discount, td_lambda)) -> (scal [8], rows [6, B], td [H, B]);
    scal = (mean similarity, mean reward, mean value, mean total, weighted, mean w, mean model_loss, mean td_loss),
    rows = (similarity, reward, value, clamped priority, model_loss, td_loss) per batch row, td = the TD-lambda targets.
    Only scal[4] (the weighted loss) carries a gradient, to sim, q1, q2 and rp."""

    @staticmethod
    def forward(ctx, sim, q1, q2, rp, rw, rwpi, nq, w, coefs):
        H, B = sim.shape
        ins = [_f32c(t) for t in (sim, q1, q2, rp, rw, rwpi, nq, w)]
        for t in ins[:7]:
            if tuple(t.shape) != (H, B):
                raise ValueError(f"_DssmFusedLoss: every operand but w must be [{H}, {B}], got {tuple(t.shape)}")
        if tuple(ins[7].shape) != (B,):
            raise ValueError(f"_DssmFusedLoss: w must be [{B}], got {tuple(ins[7].shape)}")
        args = DrnnLossArgs(*[t.data_ptr() for t in ins], H, B, *[float(c) for c in coefs])
        td, rows, scal = sim.new_empty(H, B), sim.new_empty(6, B), sim.new_empty(8)
        call("tdmpc_drnn_loss_forward", args, td, rows, scal, torch.cuda.current_stream().cuda_stream)
        ctx.save_for_backward(*ins, td, rows, scal)
        ctx.coefs = coefs
        ctx.mark_non_differentiable(rows, td)
        return scal, rows, td

    @staticmethod
    def backward(ctx, g_scal, g_rows, g_td):
        *ins, td, rows, scal = ctx.saved_tensors
        H, B = ins[0].shape
        args = DrnnLossArgs(*[t.data_ptr() for t in ins], H, B, *[float(c) for c in ctx.coefs])
        g = g_scal.contiguous()
        need = ctx.needs_input_grad
        dsim, dq1, dq2, drp = (torch.empty_like(ins[0]) if need[i] else None for i in range(4))
        call("tdmpc_drnn_loss_backward", args, td, rows, scal, g.data_ptr() + 16, ptr(dsim), ptr(dq1), ptr(dq2),
             ptr(drp), torch.cuda.current_stream().cuda_stream)
        return dsim, dq1, dq2, drp, None, None, None, None, None


class _DssmSimFusedLoss(torch.autograd.Function):
    """TdMpcSimDssm.update's loss composition (tdmpc_similarity_drnn.py:447-471) and its backward as HIP kernels
    (tdmpc_drnn_sim_loss_forward / _backward): forward(sim [H, B], q1, q2, rp, rw, rwpi, nq [H - W, B] (the shoot steps),
    w [B], coefs = (similarity_coef, reward_coef, value_coef, discount)) -> (scal [6], rows [5, B], td [H - W, B]);
    scal = (mean similarity, mean reward, mean value, mean total, weighted = mean(total) mean(w), mean w), rows =
    (similarity, reward, value, clamped priority, total) per batch row, td = the one-step TD targets. Only scal[4]
    carries a gradient, to sim, q1, q2 and rp."""

    @staticmethod
    def _args(ins, H, N, B, coefs):
        return DrnnSimLossArgs(*[t.data_ptr() for t in ins], H, H - N, B, *[float(c) for c in coefs])

    @staticmethod
    def forward(ctx, sim, q1, q2, rp, rw, rwpi, nq, w, coefs):
        H, B = sim.shape
        N = q1.shape[0]
        ins = [_f32c(t) for t in (sim, q1, q2, rp, rw, rwpi, nq, w)]
        if not 1 <= N < H:
            raise ValueError(f"_DssmSimFusedLoss: {N} shoot steps of {H} (1 <= horizon - warmup_len <= horizon - 1)")
        for t in ins[1:7]:
            if tuple(t.shape) != (N, B):
                raise ValueError(f"_DssmSimFusedLoss: q1 .. nq must be [{N}, {B}], got {tuple(t.shape)}")
        if tuple(ins[7].shape) != (B,):
            raise ValueError(f"_DssmSimFusedLoss: w must be [{B}], got {tuple(ins[7].shape)}")
        td, rows, scal = sim.new_empty(N, B), sim.new_empty(5, B), sim.new_empty(6)
        call("tdmpc_drnn_sim_loss_forward", _DssmSimFusedLoss._args(ins, H, N, B, coefs), td, rows, scal,
             torch.cuda.current_stream().cuda_stream)
        ctx.save_for_backward(*ins, td, rows, scal)
        ctx.coefs = coefs
        ctx.mark_non_differentiable(rows, td)
        return scal, rows, td

    @staticmethod
    def backward(ctx, g_scal, g_rows, g_td):
        *ins, td, rows, scal = ctx.saved_tensors
        (H, B), N = ins[0].shape, ins[1].shape[0]
        g = g_scal.contiguous()
        need = ctx.needs_input_grad
        dsim, dq1, dq2, drp = (torch.empty_like(ins[i]) if need[i] else None for i in range(4))
        call("tdmpc_drnn_sim_loss_backward", _DssmSimFusedLoss._args(ins, H, N, B, ctx.coefs), td, rows, scal,
             g.data_ptr() + 16, ptr(dsim), ptr(dq1), ptr(dq2), ptr(drp), torch.cuda.current_stream().cuda_stream)
        return dsim, dq1, dq2, drp, None, None, None, None, None


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


class DssmTrainStep:
    """Differentiable `DSSM.next` (train mode) and `similarity_loss` on HIP for `model` (a `tdmpc_amd.dssm.DSSM` on the
    GPU, fp32). max_rows: the largest batch of `next`; max_loss_rows: of `similarity_loss` (default
    min(4096, max_rows * max_steps): the reference concatenates the per-step predictions)."""

    LOSS_ABI = "tdmpc_drnn_simloss_"   # _LossFn's entry points (tdmpc_amd.icem_learner.IcemTrainStep: the tdmpc_dims ones)

    def __init__(self, model, max_rows: int, max_steps: int | None = None, max_loss_rows: int | None = None,
                 max_losses: int = 2):
        cfg = model.cfg
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("DssmTrainStep: the model must be on the GPU (there is no CPU path)")
        self.model, self.cfg = model, cfg
        self.L, self.A, self.Hd = int(cfg.latent_dim), int(cfg.action_dim), int(cfg.hidden_dim)
        self.max_rows = int(max_rows)
        self.max_steps = int(max_steps if max_steps is not None else cfg.horizon + 1)
        self.max_loss_rows = int(max_loss_rows if max_loss_rows is not None
                                 else min(_lib.DT_MAX_ROWS, self.max_rows * self.max_steps))
        self.dims = drnn_dims_from_cfg(cfg)
        _lib.lib()
        if _lib.lib().tdmpc_drnn_train_version() != _lib.DRNN_TRAIN_VERSION:
            raise RuntimeError("libtdmpc_hip: tdmpc_drnn_train_version mismatch")
        sn, sl = DrnnTrainSizes(), DrnnTrainSizes()
        call("tdmpc_drnn_train_sizes_for", self.dims, self.max_rows, sn)
        call("tdmpc_drnn_train_sizes_for", self.dims, self.max_loss_rows, sl)
        named = dict(model.named_parameters())
        bufs = dict(model.named_buffers())
        self._next_params = tuple(named[k] for k in NEXT_PARAMS)
        self._loss_params = tuple(named[k] for k in LOSS_PARAMS)
        for p in self._next_params + self._loss_params:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("DssmTrainStep: the model's parameters must be contiguous float32")
        self._next_stats = (bufs["_dynamics.prior_mlp.1.running_mean"], bufs["_dynamics.prior_mlp.1.running_var"])
        self._loss_stats = (bufs["_predictor.1.running_mean"], bufs["_predictor.1.running_var"])
        self._next_pool = _Pool(self.max_steps, sn.next_saved_floats, dev, "max_steps")
        self._loss_pool = _Pool(int(max_losses), sl.loss_saved_floats, dev, "max_losses")
        self._ws = torch.empty(max(sn.workspace_floats, sl.workspace_floats), dtype=torch.float32, device=dev)
        self._iws = {}   # (segments, rows per segment) -> the workspace of intrinsic_loss
        self._cws = {}   # likewise of intrinsic_chain_loss
        self.chain_mode = int(os.environ.get("TDMPC_DSSM_CHAIN_MODE", CHAIN_MODE))

    def _check(self, what, rows, cap, *shaped):
        if not self.model.training:
            raise RuntimeError(f"DssmTrainStep.{what}: the model is in eval() mode; these passes run the BatchNorms on "
                               "batch statistics (model.train()). For inference use DrnnPlanner.next")
        if rows > cap:
            raise ValueError(f"DssmTrainStep.{what}: {rows} rows, sized for {cap}")
        for name, t, width in shaped:
            if t.dim() != 2 or t.shape[0] != rows or t.shape[1] != width or not t.is_cuda:
                raise ValueError(f"DssmTrainStep.{what}: {name} must be a GPU tensor of shape [{rows}, {width}], got "
                                 f"{tuple(t.shape)} on {t.device}")

    def next(self, z, a, h):
        """`DSSM.next(z, a, h)` under `model.train()`: (z' [R, L], h' [R, Hd], r [R, 1]), differentiable in z, a, h and
        the 20 parameter tensors of `_dynamics` and `_reward`. Moves prior_mlp's running statistics."""
        self._check("next", z.shape[0], self.max_rows, ("z", z, self.L), ("a", a, self.A), ("h", h, self.Hd))
        zo, ho, ro = _NextFn.apply(self, z, a, h, *self._next_params)
        self.model._dynamics.prior_mlp[1].num_batches_tracked += 1
        return zo, ho, ro.unsqueeze(1)

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

    @torch.no_grad()
    def intrinsic_loss(self, z, a, keys, segments):
        """`segments` independent `next(z, a, 0)` + `similarity_loss(z', keys)` passes over the row blocks
        [s B, (s + 1) B) of z [S B, L], a [S B, A], keys [S B, L] as one launch chain -> loss [S B]. Forward only. Each
        segment normalises both BatchNorms over its own B rows and moves their running statistics once, in segment
        order: bitwise what S pairs of `next` / `similarity_loss` calls on the segments give."""
        R = z.shape[0]
        S = int(segments)
        if S < 1 or R % S:
            raise ValueError(f"DssmTrainStep.intrinsic_loss: {R} rows do not split into {S} segments")
        self._check("intrinsic_loss", R, _lib.DT_MAX_ROWS, ("z", z, self.L), ("a", a, self.A), ("keys", keys, self.L))
        z, a, keys = _f32c(z), _f32c(a), _f32c(keys)
        ws = self._iws.get((S, R // S))
        if ws is None:
            n = C.c_size_t()
            call("tdmpc_drnn_intrinsic_workspace_floats", self.dims, S, R // S, C.byref(n))
            ws = self._iws[(S, R // S)] = torch.empty(n.value, dtype=torch.float32, device=z.device)
        loss = z.new_empty(R)
        ntab, nn_ = _table(self._next_params, self._next_stats)
        ltab, nl = _table(self._loss_params, self._loss_stats)
        call("tdmpc_drnn_intrinsic_fwd", self.dims, ntab, nn_, ltab, nl, z, a, keys, S, R // S, loss, ws, ws.numel(),
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
        R = z.shape[0]
        S, W = int(segments), int(warm)
        if S < 1 or R % S:
            raise ValueError(f"DssmTrainStep.intrinsic_chain_loss: {R} rows do not split into {S} segments")
        if not 0 <= W < S:
            raise ValueError(f"DssmTrainStep.intrinsic_chain_loss: warm={W} is not in [0, {S})")
        self._check("intrinsic_chain_loss", R, _lib.DT_MAX_ROWS, ("z", z, self.L), ("a", a, self.A),
                    ("keys", keys, self.L))
        z, a, keys = _f32c(z), _f32c(a), _f32c(keys)
        B = R // S
        ws = self._cws.get((S, B))
        if ws is None:
            n = C.c_size_t()
            call("tdmpc_drnn_intrinsic_chain_workspace_floats", self.dims, S, B, C.byref(n))
            ws = self._cws[(S, B)] = torch.empty(n.value, dtype=torch.float32, device=z.device)
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
