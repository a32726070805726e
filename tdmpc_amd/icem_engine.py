"""The MLP iCEM agent's update on the learner engine: one TdICemSimMlp.update (tdmpc_icem_similarity_mlp.py:346-428) as
explicit forward and backward passes of HIP kernels, no autograd graph and no hipBLASLt. Opt-in:
`TdIcemMlp(cfg, engine=True)` or TDMPC_ICEM_LEARNER_ENGINE=1; the default stays `icem_learner.IcemMlpLearner`.

`IcemEngine(SimEngine)` is tdmpc_amd/sim_engine.py's engine -- the flat layout with `_predictor` in the main range and
the BatchNorm's buffers outside it, the LayerNorm encoder, the similarity head and its loss, the policy optimiser at
cfg.pi_lr (what `IcemMlpLearner`'s `learner.make_optimizer(pi_params, cfg, cfg.pi_lr)` steps at) -- with the three
things in which the reference's update differs from `TDMPCSIM.update`:

  * The intrinsic rewards (:323-344). Both encoders run once over all H + 1 next observations (the TD heads and the
    similarity head keep reading the first H B rows). The online encoder's second product also writes its latents
    densely into b["ZI"] behind z_0, which the main stream's encoder writes there the same way, so z [S B, L] = (z_0,
    the online next latents of steps 0 .. H - 1), a = action[0 .. H] and keys = the target latents b["NZ"], S = H + 1,
    go to tdmpc_icem_intrinsic_fwd as they lie, its pointer tables built once over the flat views of `_dynamics.*` and
    `_predictor.*` and the module's own running statistics. tdmpc_drnn_intrinsic_finish then runs on the learner's
    device RunningMeanStd and explore coefficient -> b["intrinsic"], b["reward_pi"] [S B]. The TD heads' last launch
    takes b["reward_pi"] as its reward; the loss keeps the extrinsic one.
  * `update_pi` is not weighted by rho ** t: `self.rho`, which feeds only tdmpc_lg_pi_loss and the pi rows' backward
    here (the loss kernels take cfg.rho itself), is all ones.
  * `_predictor`'s BatchNorm moves its running statistics H + 2 times per update, H + 1 times in the intrinsic pass in
    segment order and then once in the similarity head.

Ordering. The intrinsic pass runs on the side stream between the encoders and the TD heads of `_td_steps`: after the
main stream's z_0 (an event recorded behind the main encoder, the mechanism of `_pair`'s wait_stream), before the TD
heads' last launch, and before the main stream's `_loss` (which follows the join of the side stream), so the BatchNorm's
two writers run in the reference's order; tdmpc_lg_adam, which writes the `_dynamics` weights the pass reads, follows
the same join, and the next update's fork follows it. Nothing synchronises with the host.

`IcemEngineLearner(EngineLearner)` is the learner around it (the capture-and-replay driver, the EMA on the engine, the
planner's live repack inside the captured graph) with `IcemMlpLearner.update`'s signature and return value. It has no
PyTorch path: a cfg `reason` names, or a model on the CPU, is refused at construction.
"""
from __future__ import annotations

import ctypes as C
import sys

import torch

from . import _lib, sim_engine
from .config import linear_schedule
from .drnn_learner import METRICS, RewardRms
from .dssm_train import LOSS_PARAMS, new_rms_state
from .icem_learner import DYN_PARAMS, check_icem_learner_cfg
from .learner import EngineLearner
from .learner_engine import _p
from .sim_engine import SimEngine

WHO = "IcemEngineLearner"
ENGINE_ENV = "TDMPC_ICEM_LEARNER_ENGINE"   # "1": TdIcemMlp builds IcemEngineLearner


def supported(cfg) -> bool:
    """What IcemEngine admits: `sim_engine.supported` and the intrinsic pass's (horizon + 1) * batch_size rows within
    TDMPC_DT_MAX_ROWS."""
    return sim_engine.supported(cfg) and (int(cfg.horizon) + 1) * int(cfg.batch_size) <= _lib.DT_MAX_ROWS


def reason(cfg):
    """None where `supported(cfg)`, else the first setting that fails, named as `check_icem_learner_cfg` names them."""
    try:
        check_icem_learner_cfg(cfg)
    except (ValueError, NotImplementedError) as e:
        return str(e).replace("IcemMlpLearner", WHO)
    if int(cfg.latent_dim) < 1:
        return f"{WHO}: latent_dim={int(cfg.latent_dim)} is not supported (at least 1)"
    if int(cfg.enc_dim) not in sim_engine.ENC_DIMS:
        return f"{WHO}: enc_dim={int(cfg.enc_dim)} is not supported (256, 512 or 1024: the encoder's LayerNorm kernels)"
    wd = float(getattr(cfg, "weight_decay", 0.0))
    if wd != 0.0:
        return f"{WHO}: weight_decay={wd} is not supported (0 only: the engine's Adam step has no decay)"
    assert supported(cfg)
    return None


class IcemEngine(SimEngine):
    # hooks of the engine built on this one (tdmpc_amd/dssm_engine.py): what refuses a cfg, and the intrinsic pass's
    # entry points, dims and dynamics pointer table
    REASON = staticmethod(reason)
    INTRINSIC = "tdmpc_icem_intrinsic"   # <INTRINSIC>_workspace_floats, <INTRINSIC>_fwd

    def _intrinsic_setup(self):
        """-> (the intrinsic pass's dims, its dynamics pointer table over the flat views)."""
        if self.lib.tdmpc_icem_learner_version() != _lib.ICEM_LEARNER_VERSION:
            raise RuntimeError("libtdmpc_hip: tdmpc_icem_learner_version mismatch")
        return (_lib.dims_from_cfg(self.cfg, enc_norm=True),
                (C.c_void_p * len(DYN_PARAMS))(*[self.w(k) for k in DYN_PARAMS]))

    def __init__(self, agent):
        why = self.REASON(agent.cfg)
        if why is not None:
            raise ValueError(why)
        super().__init__(agent)
        self.rho = torch.ones(self.H + 1, dtype=torch.float32, device=self.dev)   # update_pi: no rho ** t (:267-284)
        self.dims, self.dtab = self._intrinsic_setup()
        w = self.w
        loss = [w(k) for k in LOSS_PARAMS]
        # (the BatchNorm's running statistics follow its weight and bias, include/tdmpc_icem_learner.h)
        loss[4:4] = [_p(self.bn_mean), _p(self.bn_var)]
        self.ltab = (C.c_void_p * len(loss))(*loss)
        self.rms = self.coef = None        # the learner's device RunningMeanStd and explore coefficient (it sets them)
        self._z0 = torch.cuda.Event()      # z_0 is in b["ZI"] (main stream)
        self._z0_set = False

    def bufs(self, B):
        new = B not in self._bufs
        b = super().bufs(B)
        if new:
            H, L, E, LAP = self.H, self.L, self.E, self.LAP
            S = H + 1
            z = lambda *s: torch.zeros(*s, device=self.dev)  # noqa: E731
            n = C.c_size_t()
            _lib.call(self.INTRINSIC + "_workspace_floats", self.dims, S, B, C.byref(n))
            b.update(
                # both encoders over all H + 1 next observations
                Pt1=z(S * B, E), Po1=z(S * B, E), Yt1=z(S * B, E), Yo1=z(S * B, E), NZ=z(S * B, L), Xtd=z(S * B, LAP),
                # the intrinsic pass: z_0 and the online next latents, dense (the last B rows are not read); the raw
                # losses, the normalised rewards, reward + explore_coef * them; the pass's scratch
                ZI=z((S + 1) * B, L), iloss=z(S * B), intrinsic=z(S * B), reward_pi=z(S * B), iws=z(n.value),
            )
        return b

    # ------------------------------------------------------------------------------------------- the passes
    def _td_obs(self, b, next_obses, action, reward):
        S = self.H + 1
        b["act"], b["rew"] = action[:S].contiguous(), reward[:S].contiguous()
        self.last = b   # (the buffers of the update under way: `update` reads b["intrinsic"])
        return next_obses[:S].contiguous()

    def _enc_fwd_steps(self, b, obs, B):
        yield from super()._enc_fwd_steps(b, obs, B, z2=_p(b["ZI"]))
        self._z0.record()
        self._z0_set = True

    def _enc_td_steps(self, b, nxo_t, R):
        B = R // self.H
        return super()._enc_td_steps(b, nxo_t, R + B, z2=_p(b["ZI"], B * self.L))

    def _intrinsic_steps(self, b, B):
        """:323-344 -> b["intrinsic"], b["reward_pi"]. A generator: yields after each call (see _pair)."""
        S, st = self.H + 1, self._stream
        while not self._z0_set:   # (the main stream's encoder is issued first: at most a turn or two)
            yield
        torch.cuda.current_stream(self.dev).wait_event(self._z0)
        ws = b["iws"]
        _lib.call(self.INTRINSIC + "_fwd", self.dims, self.dtab, len(self.dtab), self.ltab, len(self.ltab), b["ZI"],
                  b["act"], b["NZ"], S, B, b["iloss"], ws, ws.numel(), st())
        yield
        _lib.call("tdmpc_drnn_intrinsic_finish", b["iloss"], S * B, self.rms, self.coef, b["rew"], b["intrinsic"],
                  b["reward_pi"], st())
        yield

    def _td_steps(self, b, nxo_t, rew, R, eps):
        """The TD targets from reward_pi = explore_coef * intrinsic + reward (:286-292, :376)."""
        yield from self._enc_td_steps(b, nxo_t, R)
        yield from self._intrinsic_steps(b, R // self.H)
        yield from self._td_head_steps(b, _p(b["reward_pi"]), R, eps)

    def update(self, buffer, noise=None):
        """One TdICemSimMlp.update without the EMA -> metrics [8] (drnn_learner.METRICS order)."""
        if self.rms is None or self.coef is None:
            raise RuntimeError("IcemEngine: the learner's RunningMeanStd state and explore coefficient are not set")
        self._z0_set = False
        m = super().update(buffer, noise)
        return torch.cat([m, self.last["intrinsic"].mean().view(1)])


class IcemEngineLearner(EngineLearner):
    """Owns the engine, the RunningMeanStd state and (in graph mode) the captured update graphs of one MLP iCEM agent
    (`agent`: cfg, model, model_target, device and, when it plans, planner). `update(buffer, step, noise)` ->
    (metrics tensor [8] (METRICS) on the device, explore_coef), as `IcemMlpLearner.update`; noise: 2H + 1 [B, A]
    TruncatedNormal draws (H for the TD targets, H + 1 for update_pi) or None to draw on the device."""

    METRICS = METRICS
    ENGINE, ENGINE_CLASS = sys.modules[__name__], "IcemEngine"

    def __init__(self, agent, graph: bool = True, warmup: int = 3):
        why = reason(agent.cfg)
        if why is not None:
            raise ValueError(why)                                          # before it looks at the model
        device = next(agent.model.parameters()).device
        if device.type != "cuda":
            raise ValueError(f"{WHO}: the model is on the {device.type.upper()} (the engine runs on the GPU and has no "
                             f"PyTorch path)")
        # the state `DssmLearner` keeps: the device RunningMeanStd behind `agent.reward_rms`, and the explore
        # coefficient as a device scalar, written before every step (a captured graph reads it)
        self.rms = new_rms_state(device)
        self.reward_rms = RewardRms(self.rms)
        self.coef = torch.zeros(1, dtype=torch.float32, device=device)
        super().__init__(agent, graph, warmup)
        self.engine.rms, self.engine.coef = self.rms, self.coef

    def _use_engine(self):
        return True

    def step(self, buffer, noise=None):
        m = super().step(buffer, noise)
        H, b = int(self.cfg.horizon), self.engine.last
        self.last = dict(intrinsic=b["intrinsic"].view(H + 1, -1, 1), prio=b["lrows"][3].view(-1, 1))
        return m

    def _after_engine_step(self):
        # (the engine moves the running statistics itself: H + 1 times in the intrinsic pass, once in the head)
        self.agent.model._predictor[1].num_batches_tracked += int(self.cfg.horizon) + 2

    def update(self, buffer, step, noise=None):
        """`TdICemSimMlp.update` semantics -> (metrics tensor [8] on the device, explore_coef); no synchronisation."""
        coef = linear_schedule(self.cfg.explore_schedule, step)
        self.coef.fill_(coef)
        return super().update(buffer, step, noise), coef
