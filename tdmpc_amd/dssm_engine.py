"""The DSSM iCEM agent's update on the learner engine: one TdICemSimDssm.update
(tdmpc_icem_similarity_drnn.py:367-384, :421-553) as explicit forward and backward passes of HIP kernels over flat
parameters, no autograd graph and no hipBLASLt. Opt-in: `TdIcemDrnn(cfg, engine=True)` or
TDMPC_DSSM_LEARNER_ENGINE=1; the default stays `drnn_learner.DssmLearner`.

`DssmEngine(IcemEngine)` inherits the flat layout with the BatchNorm buffers outside P / G / Adam / EMA (here both
`_predictor.1`'s and `_dynamics.prior_mlp.1`'s), the LayerNorm encoder on the row kernels, both encoders over all H + 1
next observations, the Q heads, the similarity head over the H B predicted latents, `update_pi` without `rho`,
tdmpc_lg_finalize / tdmpc_lg_adam, the device RunningMeanStd and the explore-coefficient scalar. It replaces, through
the engines' hooks:

  * The intrinsic pass: tdmpc_drnn_intrinsic_fwd (S = H + 1 one-step rollouts from a zero hidden state) over the flat
    views of `_dynamics.*` / `_reward.*` / `_predictor.*` and the modules' own running statistics.
  * The rollout, per step t: [z_t | a_t] weight_ih^T and, for t > 0, h_t weight_hh^T as two jobs of one grouped launch;
    tdmpc_drnn_gate_fwd (a null hidden state at t = 0); prior_mlp.0; tdmpc_sim_bn_fwd; prior_mlp.3 writing z_{t+1} where
    the Q heads, `update_pi` and the similarity head read it. Every step's saved regions go to step-indexed slots of
    [H B, .] buffers.
  * The reward head reads the new hidden states: `_reward` once over the H B rows of hn, in the Q heads' grouped
    launches.
  * The TD pass writes nq = min target Q at the online next latents under the online policy (the row kernel's
    reward + gamma min Q with a zero reward and gamma 1); tdmpc_drnn_loss_forward / _backward compose the TD-lambda
    targets from reward_pi and the loss mean(model_loss) mean(w) + mean(td_loss) over the extrinsic reward, with the
    1 / horizon hook as the gradient's seed (the engine's `gw`).
  * The rollout's backward, newest step first, data gradients only: dz' W_p3; tdmpc_sim_bn_bwd; dL/dh' = de W_p0 +
    (the reward head's dP1) W_r0 + dgh_{t+1} W_hh + the direct path dhd_{t+1}, one product of three segments and a
    residual; tdmpc_drnn_gate_bwd; dz_t = dgi W_ih[:, :L] + the heads' and the similarity head's gradient of z_t.
  * Every `_dynamics` / `_reward` weight gradient once over all steps' rows in the `main` grouped split-K launch (the
    bias as the ones column; weight_hh over steps 1 .. H - 1), prior_mlp.1's gain / shift gradients as H one-slice
    sources and the LayerNorm-affine partials of all steps as slices of one source (the six vectors lie side by side in
    the flat layout as in a slice: one tdmpc_lg_finalize tensor, which keeps the main range's 52 tensors within its 48):
    one global norm and one Adam pass, no per-step unpack.

Ordering. `_dynamics.prior_mlp.1`'s running statistics have two writers: the intrinsic pass moves them H + 1 times in
segment order, then the rollout H times. r <- 0.9 r + 0.1 m does not commute, so the main stream waits for the side
stream's intrinsic pass (an event) before the rollout's first launch: simple, at the price of running the two one
after the other. `_predictor.1` moves H + 1 times there and once in the similarity head, which follows the join.

`DssmEngineLearner(EngineLearner)` is the learner around it with `DssmLearner.update`'s signature and return value. It
has no PyTorch path: a cfg `reason` names, or a model on the CPU, is refused at construction. After every update the
planner's pack is dropped, so the next `plan()` packs the new weights.
"""
from __future__ import annotations

import ctypes as C
import sys

import torch

from . import _lib, sim_engine
from .config import linear_schedule
from .drnn_learner import METRICS, RewardRms, check_learner_cfg
from .dssm_train import NEXT_PARAMS, new_rms_state
from .icem_engine import IcemEngine
from .learner import EngineLearner
from .learner_engine import _p, _seg

WHO = "DssmEngineLearner"
ENGINE_ENV = "TDMPC_DSSM_LEARNER_ENGINE"   # "1": TdIcemDrnn builds DssmEngineLearner
P0, P1, P3 = "_dynamics.prior_mlp.0", "_dynamics.prior_mlp.1", "_dynamics.prior_mlp.3"
CELL = "_dynamics.gru_cell."
WIH, WHH = CELL + "weight_ih", CELL + "weight_hh"
LN = tuple(CELL + k for k in ("ln_reset.weight", "ln_reset.bias", "ln_update.weight", "ln_update.bias",
                              "ln_newval.weight", "ln_newval.bias"))


def reason(cfg):
    """None where the engine admits cfg, else the first setting that fails, named as `check_learner_cfg` names them."""
    try:
        check_learner_cfg(cfg)
    except (ValueError, NotImplementedError, AttributeError) as e:
        return str(e).replace("DssmLearner", WHO)
    Hd = int(cfg.hidden_dim)
    if Hd < 32 or Hd > 256 or Hd % 32:
        return f"{WHO}: hidden_dim={Hd} is not supported (a multiple of 32 up to 256: the gate kernels)"
    if int(cfg.mlp_dim) != sim_engine.BN_WIDTH:
        return f"{WHO}: mlp_dim={int(cfg.mlp_dim)} is not supported ({sim_engine.BN_WIDTH} only: the BatchNorm kernels)"
    if not 1 <= int(cfg.latent_dim) <= 256:
        return f"{WHO}: latent_dim={int(cfg.latent_dim)} is not supported (1 to 256: the cosine kernels)"
    if int(cfg.enc_dim) not in sim_engine.ENC_DIMS:
        return f"{WHO}: enc_dim={int(cfg.enc_dim)} is not supported (256, 512 or 1024: the encoder's LayerNorm kernels)"
    wd = float(getattr(cfg, "weight_decay", 0.0))
    if wd != 0.0:
        return f"{WHO}: weight_decay={wd} is not supported (0 only: the engine's Adam step has no decay)"
    assert sim_engine.supported(cfg)
    return None


class DssmEngine(IcemEngine):
    REASON = staticmethod(reason)
    INTRINSIC = "tdmpc_drnn_intrinsic"

    def _intrinsic_setup(self):
        if self.lib.tdmpc_drnn_engine_version() != _lib.DRNN_ENGINE_VERSION:
            raise RuntimeError("libtdmpc_hip: tdmpc_drnn_engine_version mismatch")
        self.Hd = int(self.cfg.hidden_dim)
        bn = self.agent.model._dynamics.prior_mlp[1]
        self.dbn_mean, self.dbn_var = bn.running_mean, bn.running_var
        tab = [self.w(k) for k in NEXT_PARAMS]
        tab[4:4] = [_p(self.dbn_mean), _p(self.dbn_var)]   # (the statistics follow prior_mlp.1's weight and bias)
        self.lntab = (C.c_void_p * 6)(*[self.w(k) for k in LN])
        self._intr = torch.cuda.Event()                    # the intrinsic pass has moved the running statistics (side)
        self._intr_set = False
        return _lib.drnn_dims_from_cfg(self.cfg), (C.c_void_p * len(tab))(*tab)

    def bufs(self, B):
        new = B not in self._bufs
        b = super().bufs(B)
        if new:
            H, M, Hd = self.H, self.M, self.Hd
            R = H * B
            z = lambda *s: torch.zeros(*s, device=self.dev)  # noqa: E731
            n, npart = C.c_size_t(), C.c_size_t()
            _lib.call("tdmpc_sim_bn_part_floats", B, C.byref(n))
            _lib.call("tdmpc_drnn_gate_part_floats", B, Hd, C.byref(npart))
            b.update(
                # the rollout's saved regions, one slot of B rows per step: the gate products, the cell's saved
                # regions and new hidden states, prior_mlp.0's output, the BatchNorm's xhat / 1 / std / ELU output
                GI=z(R, 3 * Hd), GH=z(R, 3 * Hd), GATE=z(R, 3 * Hd), LNX=z(R, 3 * Hd), LNR=z(R, 4), HN=z(R, Hd),
                DP1=z(R, M), DXH=z(R, M), DRS=z(H, M), DE=z(R, M), dbnpart=z(n.value),
                # its backward: the gradient of the ELU output, then (in place) of prior_mlp.0's output; dL/dh' of the
                # step under way; the gate's gradients; the affine partials of every step
                dDE=z(R, M), dHN=z(B, Hd), dGI=z(R, 3 * Hd), dGH=z(R, 3 * Hd), dHD=z(R, Hd),
                lnpart=z(H * npart.value), ddgb=z(H, 2, M),
                # the TD-lambda targets, the loss rows and scalars of tdmpc_drnn_loss_*, a zero reward for the TD pass
                TDL=z(R), lrows=z(6, B), scal=z(8), zero=z(R),
            )
            b["lnslices"] = H * (npart.value // (6 * Hd))
        return b

    # ------------------------------------------------------------------------------------------- the TD pass
    def _intrinsic_steps(self, b, B):
        yield from super()._intrinsic_steps(b, B)
        self._intr.record()
        self._intr_set = True

    def _td_steps(self, b, nxo_t, rew, R, eps):
        """b["TD"] = min target Q at the online next latents under the online policy (:212-216)."""
        yield from self._enc_td_steps(b, nxo_t, R)
        yield from self._intrinsic_steps(b, R // self.H)
        yield from self._td_head_steps(b, _p(b["zero"]), R, eps, gamma=1.0)

    # ------------------------------------------------------------------------------------------- the rollout
    def _rollout_fwd_steps(self, b, B):
        H, L, M, LA, LAP, Hd = self.H, self.L, self.M, self.LA, self.LAP, self.Hd
        w, X0, st = self.w, b["X0"], self._stream
        while not self._intr_set:   # (the side stream's passes are issued in turn with these: a few turns)
            yield
        torch.cuda.current_stream(self.dev).wait_event(self._intr)
        for t in range(H):
            r3, r1, rm = t * B * 3 * Hd, t * B * Hd, t * B * M
            jobs = [dict(segs=[_seg(_p(X0, t * B * LAP), LAP, w(WIH + ".weight"), LA, LA)], m=B, n=3 * Hd,
                         c=_p(b["GI"], r3), ldc=3 * Hd)]
            if t:
                jobs.append(dict(segs=[_seg(_p(b["HN"], r1 - B * Hd), Hd, w(WHH + ".weight"), Hd, Hd)], m=B, n=3 * Hd,
                                 c=_p(b["GH"], r3), ldc=3 * Hd))
            self.gemm(jobs)
            yield
            _lib.check(self.lib.tdmpc_drnn_gate_fwd(
                _p(b["GI"], r3), _p(b["GH"], r3) if t else None, _p(b["HN"], r1 - B * Hd) if t else None, self.lntab,
                _p(b["GATE"], r3), _p(b["LNX"], r3), _p(b["LNR"], t * B * 4), _p(b["HN"], r1), B, Hd, st()),
                "tdmpc_drnn_gate_fwd")
            yield
            self.gemm([dict(segs=[_seg(_p(b["HN"], r1), Hd, w(P0 + ".weight"), Hd, Hd)], m=B, n=M, c=_p(b["DP1"], rm),
                            ldc=M, bias=w(P0 + ".bias"))])
            yield
            _lib.check(self.lib.tdmpc_sim_bn_fwd(
                _p(b["DP1"], rm), w(P1 + ".weight"), w(P1 + ".bias"), _p(self.dbn_mean), _p(self.dbn_var),
                _p(b["DXH"], rm), _p(b["DRS"], t * M), _p(b["DE"], rm), _p(b["dbnpart"]), B, st()), "tdmpc_sim_bn_fwd")
            yield
            self.gemm([dict(segs=[_seg(_p(b["DE"], rm), M, w(P3 + ".weight"), M, M)], m=B, n=L,
                            c=_p(X0, (t + 1) * B * LAP), ldc=LAP, bias=w(P3 + ".bias"), c2=_p(b["ZP"], t * B * L),
                            ldc2=L)])
            yield

    def _reward_in(self, b, R):
        return [(b["HN"][:R], 0, self.Hd)]

    def _reward_dz_segs(self, b):
        return []   # (the reward head reads h', not z: its input gradient enters the rollout's backward)

    def _reward0_dw(self, b, R, sp):
        M, Hd = self.M, self.Hd
        return ("_reward.0", M, Hd, [_seg(_p(b["dP1"][2]), M, _p(b["HN"]), Hd, R, 1, 1, Hd)], sp)

    def _loss(self, b, rew, weights, B):
        """The similarity head, the TD-lambda targets and the loss composition (:217-245), and their backward ->
        b["lrows"], b["scal"], b["dq"], the queries' gradient in b["dZP"][B L:]."""
        cfg, H, Q, dq = self.cfg, self.H, b["Q"], b["dq"]
        st, lib = self._stream(), self.lib
        self._sim_fwd(b, B)
        la = _lib.DrnnLossArgs(_p(b["sim"]), _p(Q[0]), _p(Q[1]), _p(Q[2]), rew, _p(b["reward_pi"]), _p(b["TD"]),
                               _p(weights), H, B, float(cfg.similarity_coef), float(cfg.reward_coef),
                               float(cfg.value_coef), float(cfg.discount), float(cfg.td_lambda))
        _lib.check(lib.tdmpc_drnn_loss_forward(C.byref(la), _p(b["TDL"]), _p(b["lrows"]), _p(b["scal"]), st),
                   "tdmpc_drnn_loss_forward")
        _lib.check(lib.tdmpc_drnn_loss_backward(C.byref(la), _p(b["TDL"]), _p(b["lrows"]), _p(b["scal"]),
                                                _p(self.gw), _p(b["dsim"]), _p(dq[0]), _p(dq[1]), _p(dq[2]), st),
                   "tdmpc_drnn_loss_backward")
        self._sim_bwd(b, B)

    def _rollout_bwd_steps(self, b, B):
        """Newest step first, data gradients only: b["S"] (the Q heads' and the similarity head's gradient of z_t),
        b["dZP"] and b["dP1"][2] (the reward head's first layer) -> b["DG"] / b["DZ0"], and per step b["dDE"],
        b["dGI"], b["dGH"], the affine partials."""
        H, L, M, LA, Hd = self.H, self.L, self.M, self.LA, self.Hd
        w, st = self.w, self._stream
        S, dZP, DG, dPr = b["S"], b["dZP"], b["DG"], b["dP1"][2]
        npart = b["lnpart"].numel() // H
        for t in range(H - 1, -1, -1):
            r3, r1, rm = t * B * 3 * Hd, t * B * Hd, t * B * M
            g_t = _p(dZP, H * B * L) if t == H - 1 else _p(DG, t * B * L)     # d loss / d z_{t+1}
            self.gemm([dict(segs=[_seg(g_t, L, w(P3 + ".weight"), M, L, bmode=1)], m=B, n=M, c=_p(b["dDE"], rm),
                            ldc=M)])
            yield
            _lib.check(self.lib.tdmpc_sim_bn_bwd(
                _p(b["dDE"], rm), w(P1 + ".weight"), _p(b["DXH"], rm), _p(b["DRS"], t * M), _p(b["DE"], rm),
                _p(b["dbnpart"]), _p(b["dDE"], rm), _p(b["ddgb"][t][0]), _p(b["ddgb"][t][1]), B, st()),
                "tdmpc_sim_bn_bwd")
            yield
            job = dict(segs=[_seg(_p(b["dDE"], rm), M, w(P0 + ".weight"), Hd, M, bmode=1),
                             _seg(_p(dPr, rm), M, w("_reward.0.weight"), Hd, M, bmode=1)], m=B, n=Hd, c=_p(b["dHN"]),
                       ldc=Hd)
            if t < H - 1:   # the next step's gradient of this h': through weight_hh, and its direct (1 - update) path
                job["segs"].append(_seg(_p(b["dGH"], r3 + B * 3 * Hd), 3 * Hd, w(WHH + ".weight"), Hd, 3 * Hd,
                                        bmode=1))
                job["res"], job["ldres"] = _p(b["dHD"], r1 + B * Hd), Hd
            self.gemm([job])
            yield
            _lib.check(self.lib.tdmpc_drnn_gate_bwd(
                _p(b["dHN"]), _p(b["GH"], r3) if t else None, _p(b["HN"], r1 - B * Hd) if t else None, self.lntab,
                _p(b["GATE"], r3), _p(b["LNX"], r3), _p(b["LNR"], t * B * 4), _p(b["dGI"], r3),
                _p(b["dGH"], r3) if t else None, _p(b["dHD"], r1) if t else None, _p(b["lnpart"], t * npart), B, Hd,
                st()), "tdmpc_drnn_gate_bwd")
            yield
            out = _p(DG, (t - 1) * B * L) if t > 0 else _p(b["DZ0"])
            self.gemm([dict(segs=[_seg(_p(b["dGI"], r3), 3 * Hd, w(WIH + ".weight"), LA, 3 * Hd, bmode=1)], m=B, n=L,
                            c=out, ldc=L, res=_p(S, t * B * L), ldres=L)])
            yield

    def _rollout_dw(self, b, B, sp):
        H, L, M, LA, Hd = self.H, self.L, self.M, self.LA, self.Hd
        R = H * B
        dw = [(P3, L, M, self._last_step_segs(b, B, b["DE"]), sp),
              (P0, M, Hd, [_seg(_p(b["dDE"]), M, _p(b["HN"]), Hd, R, 1, 1, Hd)], sp),
              # (weight_ih / weight_hh have no bias: the ones column's sums find no tensor in tdmpc_lg_finalize)
              (WIH, 3 * Hd, LA, [_seg(_p(b["dGI"]), 3 * Hd, _p(b["X0"]), self.LAP, R, 1, 1, LA)], sp)]
        if H > 1:   # step t > 0 reads h_t = hn of step t - 1; step 0's hidden state is zero
            dw.append((WHH, 3 * Hd, Hd, [_seg(_p(b["dGH"], B * 3 * Hd), 3 * Hd, _p(b["HN"]), Hd, R - B, 1, 1, Hd)],
                       sp))
        return dw

    def _src_extra(self, b):
        M, Hd, H = self.M, self.Hd, self.H
        src = super()._src_extra(b)
        # the model's main range has 52 tensors and tdmpc_lg_finalize takes 48: prior_mlp.1's gain and shift, and the six
        # LayerNorm-affine vectors, lie side by side in the flat layout as in their slices, and go as one source each
        src[P1 + ".weight"] = (_p(b["ddgb"]), 1, 2 * M, 2 * M, H, 2 * M, (P1 + ".bias",))
        src[LN[0]] = (_p(b["lnpart"]), 1, 6 * Hd, 6 * Hd, b["lnslices"], 6 * Hd, LN[1:])
        return src

    def update(self, buffer, noise=None):
        """One TdICemSimDssm.update without the EMA -> metrics [8] (drnn_learner.METRICS order)."""
        self._intr_set = False
        return super().update(buffer, noise)


class DssmEngineLearner(EngineLearner):
    """Owns the engine, the RunningMeanStd state and (in graph mode) the captured update graphs of one DSSM iCEM agent
    (`agent`: cfg, model, model_target, device and, when it plans, planner). `update(buffer, step, noise)` ->
    (metrics tensor [8] (METRICS) on the device, explore_coef), as `DssmLearner.update`; noise: 2H + 1 [B, A]
    TruncatedNormal draws (H for the value targets, H + 1 for update_pi) or None to draw on the device."""

    METRICS = METRICS
    ENGINE, ENGINE_CLASS = sys.modules[__name__], "DssmEngine"

    def __init__(self, agent, graph: bool = True, warmup: int = 3):
        why = reason(agent.cfg)
        if why is not None:
            raise ValueError(why)                                          # before it looks at the model
        device = next(agent.model.parameters()).device
        if device.type != "cuda":
            raise ValueError(f"{WHO}: the model is on the {device.type.upper()} (the engine runs on the GPU and has no "
                             f"PyTorch path)")
        self.rms = new_rms_state(device)
        self.reward_rms = RewardRms(self.rms)
        self.coef = torch.zeros(1, dtype=torch.float32, device=device)
        super().__init__(agent, graph, warmup)
        self.engine.rms, self.engine.coef = self.rms, self.coef

    def _use_engine(self):
        return True

    def step(self, buffer, noise=None):
        m = self.engine.update(buffer, noise)
        H, b, model = int(self.cfg.horizon), self.engine.last, self.agent.model
        # (the engine moves the running statistics itself: the intrinsic pass H + 1 times each, the rollout
        # prior_mlp.1's H times, the similarity head `_predictor.1`'s once)
        model._dynamics.prior_mlp[1].num_batches_tracked += 2 * H + 1
        model._predictor[1].num_batches_tracked += H + 2
        self.last = dict(intrinsic=b["intrinsic"].view(H + 1, -1, 1), prio=b["lrows"][3].view(-1, 1))
        return m   # (`_after_update` drops the planner's pack: the next plan() packs the new weights)

    def _before_capture(self):
        """Nothing to prepare: the captured update does not repack the planner."""

    def update(self, buffer, step, noise=None):
        """`TdICemSimDssm.update` semantics -> (metrics tensor [8] on the device, explore_coef); no synchronisation."""
        coef = linear_schedule(self.cfg.explore_schedule, step)
        self.coef.fill_(coef)
        return super().update(buffer, step, noise), coef
