"""The similarity TD-MPC agent's update on the learner engine: one TDMPCSIM.update (tdmpc_similarity.py:298-375) as
explicit forward and backward passes of HIP kernels, no autograd graph and no hipBLASLt.

`SimEngine(Engine)` is tdmpc_amd/learner_engine.py's engine with three parts replaced through its hooks; the heads'
forward and backward, the latent rollout and its backward, the side-stream pairing, `_update_pi`, tdmpc_lg_finalize and
tdmpc_lg_adam are the stock engine's.

  * The flat layout holds encoder, dynamics, reward, Q1, Q2, `_predictor` | pi -- the model's PARAMETERS: the
    BatchNorm's running_mean / running_var / num_batches_tracked are buffers and stay the module's own tensors, out of
    P / G / Adam and out of the EMA, which the reference takes over `parameters()` (helper.py:48-52). The policy
    optimiser steps at cfg.pi_lr (:98-99).
  * The LayerNorm state encoder (helper.dmlab_enc_norm: Linear(O -> E), LayerNorm(E), ELU, Linear(E -> L)): the first
    product without an epilogue, then tdmpc_lg_rows_fwd at m = enc_dim (LayerNorm + ELU; on obs it saves xhat / rstd /
    the ELU output), then the second product. The target and the online encoder on next_obses share both grouped
    launches and the row launch. Backward: dX of the second Linear, tdmpc_lg_rows_bwd (ELU', LayerNorm backward, the
    gain / shift gradients as per-workgroup partials for tdmpc_lg_finalize), the two dW in the `main` grouped launch.
  * The similarity head in the place of the consistency term: `_predictor` over the H B predicted latents b["ZP"] (one
    train-mode BatchNorm batch: the running statistics move once per update) against the target latents b["NZ"] --
    product, tdmpc_sim_bn_fwd, product, tdmpc_sim_cos_fwd -> sim [H B]; tdmpc_sim_loss_forward / _backward over the
    engine's TD targets (rho ** t, the 1e4 clamps, weighted = mean(total) mean(w), the 1 / horizon hook); then
    tdmpc_sim_cos_bwd, dX, tdmpc_sim_bn_bwd, dX into b["dZP"][B L:], where the stock rollout backward reads the
    consistency gradient. The two dW ride in the `main` grouped launch as split-K slices, the BatchNorm's gain / shift
    gradients reach tdmpc_lg_finalize as one-slice sources, so the one global norm and the one tdmpc_lg_adam pass cover
    the head (include/tdmpc_sim_learner.h).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .learner_engine import ELU, EPI_NONE, ROWS_NWG, Engine, _p, _seg

ENC_DIMS = (256, 512, 1024)   # the row kernels' widths (the encoder's LayerNorm)
BN_WIDTH = 512                # tdmpc_sim_bn_*'s columns: `_predictor`'s hidden width


def supported(cfg) -> bool:
    """What SimEngine admits (every other cfg the PyTorch path can run goes there): state observations, the LayerNorm
    encoder at a row-kernel width, `_predictor` at the BatchNorm kernels' width, latent_dim <= 256 (the cosine kernels'
    one wave per row), 2 <= batch_size, horizon * batch_size <= 4096 (TDMPC_DT_MAX_ROWS), Adam / AdamW without weight
    decay (where both take tdmpc_lg_adam's step)."""
    return (getattr(cfg, "modality", "state") == "state" and bool(getattr(cfg, "normalize", True)) and
            getattr(cfg, "norm_type", "ln") == "ln" and int(cfg.mlp_dim) == BN_WIDTH and
            int(cfg.enc_dim) in ENC_DIMS and 1 <= int(cfg.latent_dim) <= 256 and int(cfg.batch_size) >= 2 and
            int(cfg.horizon) * int(cfg.batch_size) <= _lib.DT_MAX_ROWS and
            str(getattr(cfg, "optim_id", "adamw")).lower() in ("adam", "adamw") and
            float(getattr(cfg, "weight_decay", 0.0)) == 0.0)


class SimEngine(Engine):
    ORDER = ("_encoder", "_dynamics", "_reward", "_Q1", "_Q2", "_predictor", "_pi")

    def __init__(self, agent):
        if not supported(agent.cfg):
            raise ValueError("SimEngine: the cfg is not admitted (sim_engine.supported)")
        super().__init__(agent)
        if self.lib.tdmpc_sim_learner_version() != _lib.SIM_LEARNER_VERSION:
            raise RuntimeError("libtdmpc_hip: tdmpc_sim_learner_version mismatch")
        self.one = torch.ones(1, device=self.dev)   # dL / dweighted (the 1 / horizon hook is in tdmpc_sim_loss_backward)
        bn = agent.model._predictor[1]
        self.bn_mean, self.bn_var = bn.running_mean, bn.running_var

    def _tensors(self, model):
        return dict(model.named_parameters())

    def _pi_lr(self):
        return float(self.cfg.pi_lr)

    def bufs(self, B):
        new = B not in self._bufs
        b = super().bufs(B)
        if new:
            H, L, M, E = self.H, self.L, self.M, self.E
            R = H * B
            z = lambda *s: torch.zeros(*s, device=self.dev)  # noqa: E731
            n = C.c_size_t()
            _lib.call("tdmpc_sim_bn_part_floats", R, C.byref(n))
            b.update(
                # the LayerNorm encoders: the first Linear's outputs (TD: target, online; main), xhat / 1 / std of
                # the main one, the gradient of its ELU output
                Pt1=z(R, E), Po1=z(R, E), Pe1=z(B, E), XHe=z(B, E), RSe=z(B), dAe=z(B, E),
                pe=z(ROWS_NWG, 2 * E),
                # the similarity head: _predictor.0's output, the BatchNorm's xhat / 1 / std / ELU output, the
                # prediction, the loss per row; their gradients (dSE: of the ELU output, then in place of SP1)
                SP1=z(R, M), SXH=z(R, M), SRS=z(M), SE=z(R, M), SPR=z(R, L), sim=z(R),
                dsim=z(R), dSPR=z(R, L), dSE=z(R, M), bnpart=z(n.value), dgb=z(2, M),
            )
        return b

    # ------------------------------------------------------------------------------------------- the encoder
    def _ln_heads(self, pairs, grad=None):
        """tdmpc_lg_rows heads of `_encoder.1` + ELU for (x, y, target) triples; grad: (xhat, rstd) to save."""
        heads = []
        for x, y, target in pairs:
            h = dict(x=_p(x), y=_p(y), ln=1, g=self.w("_encoder.1.weight", target),
                     beta=self.w("_encoder.1.bias", target), act=ELU)
            if grad is not None:
                h.update(xhat=_p(grad[0]), rstd=_p(grad[1]))
            heads.append(h)
        return heads

    def _enc_td_steps(self, b, nxo_t, R, z2=None):
        """z2: a dense [R, L] second copy of the online latents (an engine built on this one: icem_engine.py)."""
        O, E, L, LAP = self.O, self.E, self.L, self.LAP
        w, wt = self.w, (lambda k: self.w(k, True))
        nxo = _p(nxo_t)
        self.gemm([dict(segs=[_seg(nxo, O, wt("_encoder.0.weight"), O, O)], m=R, n=E, c=_p(b["Pt1"]), ldc=E,
                        bias=wt("_encoder.0.bias")),
                   dict(segs=[_seg(nxo, O, w("_encoder.0.weight"), O, O)], m=R, n=E, c=_p(b["Po1"]), ldc=E,
                        bias=w("_encoder.0.bias"))])
        yield
        self.rows(self._ln_heads([(b["Pt1"], b["Yt1"], True), (b["Po1"], b["Yo1"], False)]), R, m=E)
        yield
        self.gemm([dict(segs=[_seg(_p(b["Yt1"]), E, wt("_encoder.3.weight"), E, E)], m=R, n=L, c=_p(b["NZ"]),
                        ldc=L, bias=wt("_encoder.3.bias")),
                   dict(segs=[_seg(_p(b["Yo1"]), E, w("_encoder.3.weight"), E, E)], m=R, n=L, c=_p(b["Xtd"]),
                        ldc=LAP, bias=w("_encoder.3.bias"), c2=z2, ldc2=L)])
        yield

    def _enc_fwd_steps(self, b, obs, B, z2=None):
        """z2: a dense [B, L] second copy of z_0."""
        O, E, L, LAP = self.O, self.E, self.L, self.LAP
        w = self.w
        self.gemm([dict(segs=[_seg(_p(obs), O, w("_encoder.0.weight"), O, O)], m=B, n=E, c=_p(b["Pe1"]), ldc=E,
                        bias=w("_encoder.0.bias"))])
        yield
        self.rows(self._ln_heads([(b["Pe1"], b["Ye1"], False)], grad=(b["XHe"], b["RSe"])), B, m=E)
        yield
        self.gemm([dict(segs=[_seg(_p(b["Ye1"]), E, w("_encoder.3.weight"), E, E)], m=B, n=L, c=_p(b["X0"]),
                        ldc=LAP, bias=w("_encoder.3.bias"), c2=z2, ldc2=L)])
        yield

    def _enc_bwd(self, b, obs, B):
        O, E, L = self.O, self.E, self.L
        w, DZ0 = self.w, b["DZ0"]
        self.gemm([dict(segs=[_seg(_p(DZ0), L, w("_encoder.3.weight"), E, L, bmode=1)], m=B, n=E, c=_p(b["dAe"]),
                        ldc=E)])
        self.rows([dict(x=_p(b["dAe"]), y=_p(b["dP1e"]), yact=_p(b["Ye1"]), xhat=_p(b["XHe"]), rstd=_p(b["RSe"]),
                        ln=1, g=w("_encoder.1.weight"), act=ELU, part=_p(b["pe"]))], B, bwd=True, m=E)
        return [("_encoder.3", L, E, [_seg(_p(DZ0), L, _p(b["Ye1"]), E, B, 1, 1, E)], 1),
                ("_encoder.0", E, O, [_seg(_p(b["dP1e"]), E, _p(obs), O, B, 1, 1, O)], 1)], {}

    # ------------------------------------------------------------------------------------------- the similarity head
    def _sim_fwd(self, b, B):
        """`_predictor` + cosine over b["ZP"] against b["NZ"] -> b["sim"] [H B]."""
        H, L, M = self.H, self.L, self.M
        R = H * B
        w, st, lib = self.w, self._stream(), self.lib
        ZP, NZ = b["ZP"], b["NZ"]
        self.gemm([dict(segs=[_seg(_p(ZP), L, w("_predictor.0.weight"), L, L)], m=R, n=M, c=_p(b["SP1"]), ldc=M,
                        bias=w("_predictor.0.bias"))])
        _lib.check(lib.tdmpc_sim_bn_fwd(_p(b["SP1"]), w("_predictor.1.weight"), w("_predictor.1.bias"),
                                        _p(self.bn_mean), _p(self.bn_var), _p(b["SXH"]), _p(b["SRS"]), _p(b["SE"]),
                                        _p(b["bnpart"]), R, st), "tdmpc_sim_bn_fwd")
        self.gemm([dict(segs=[_seg(_p(b["SE"]), M, w("_predictor.3.weight"), M, M)], m=R, n=L, c=_p(b["SPR"]), ldc=L,
                        bias=w("_predictor.3.bias"))])
        _lib.check(lib.tdmpc_sim_cos_fwd(_p(b["SPR"]), _p(NZ), _p(b["sim"]), R, L, st), "tdmpc_sim_cos_fwd")

    def _loss(self, b, rew, weights, B):
        """The similarity head, the loss composition and their backward -> b["lrows"], b["scal"], b["dq"], and the
        queries' gradient in b["dZP"][B L:]."""
        cfg, H, Q, dq = self.cfg, self.H, b["Q"], b["dq"]
        st, lib = self._stream(), self.lib
        self._sim_fwd(b, B)
        la = _lib.SimLossArgs(_p(b["sim"]), _p(Q[0]), _p(Q[1]), _p(Q[2]), rew, _p(b["TD"]), _p(weights), H, B,
                              float(cfg.similarity_coef), float(cfg.reward_coef), float(cfg.value_coef),
                              float(cfg.rho))
        _lib.check(lib.tdmpc_sim_loss_forward(C.byref(la), _p(b["lrows"]), _p(b["scal"]), st), "tdmpc_sim_loss_forward")
        _lib.check(lib.tdmpc_sim_loss_backward(C.byref(la), _p(b["lrows"]), _p(b["scal"]), _p(self.one), _p(b["dsim"]),
                                               _p(dq[0]), _p(dq[1]), _p(dq[2]), st), "tdmpc_sim_loss_backward")
        self._sim_bwd(b, B)

    def _sim_bwd(self, b, B):
        """b["dsim"] [H B] back through the cosine and `_predictor` -> the queries' gradient in b["dZP"][B L:]."""
        H, L, M = self.H, self.L, self.M
        R = H * B
        w, st, lib = self.w, self._stream(), self.lib
        NZ = b["NZ"]
        _lib.check(lib.tdmpc_sim_cos_bwd(_p(b["SPR"]), _p(NZ), _p(b["dsim"]), _p(b["dSPR"]), R, L, st),
                   "tdmpc_sim_cos_bwd")
        self.gemm([dict(segs=[_seg(_p(b["dSPR"]), L, w("_predictor.3.weight"), M, L, bmode=1)], m=R, n=M,
                        c=_p(b["dSE"]), ldc=M, epi=EPI_NONE)])
        _lib.check(lib.tdmpc_sim_bn_bwd(_p(b["dSE"]), w("_predictor.1.weight"), _p(b["SXH"]), _p(b["SRS"]),
                                        _p(b["SE"]), _p(b["bnpart"]), _p(b["dSE"]), _p(b["dgb"][0]), _p(b["dgb"][1]),
                                        R, st), "tdmpc_sim_bn_bwd")
        self.gemm([dict(segs=[_seg(_p(b["dSE"]), M, w("_predictor.0.weight"), L, M, bmode=1)], m=R, n=L,
                        c=_p(b["dZP"], B * L), ldc=L)])

    def _main_dw_extra(self, b, B, sp):
        L, M, R = self.L, self.M, self.H * B
        return [("_predictor.3", L, M, [_seg(_p(b["dSPR"]), L, _p(b["SE"]), M, R, 1, 1, M)], sp),
                ("_predictor.0", M, L, [_seg(_p(b["dSE"]), M, _p(b["ZP"]), L, R, 1, 1, L)], sp)]

    def _src_extra(self, b):
        E, M = self.E, self.M
        return {"_encoder.1.weight": (_p(b["pe"]), 1, E, E, ROWS_NWG, 2 * E),
                "_encoder.1.bias": (_p(b["pe"], E), 1, E, E, ROWS_NWG, 2 * E),
                "_predictor.1.weight": (_p(b["dgb"][0]), 1, M, M, 1, M),
                "_predictor.1.bias": (_p(b["dgb"][1]), 1, M, M, 1, M)}
