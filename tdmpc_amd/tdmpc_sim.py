"""`TdMpcSim`: the reference's similarity TD-MPC agent (`TDMPCSIM`, src/algorithm/tdmpc_similarity.py:75-375), the second
of the two agents its training scripts build -- `TDMPC`'s planner over the reference's similarity model, and its update.

The model is that file's `TOLD` (:13-72): dynamics, reward, pi, Q1, Q2, the encoder (helper.dmlab_enc_norm's LayerNorm
state encoder under cfg.normalize) and `_predictor`, in that order -- `icem_mlp.IcemMlpModel`, whose state_dict has the
same names, shapes and order (tests/golden/tdmpc_sim_layout.json, recorded from the reference model), so a checkpoint
written by `TDMPCSIM.save` loads under strict key matching. cfg.normalize=False gives the reference's other branch (the
plain encoder, a BatchNorm-free `_predictor`), which constructs, loads and plans; `update` refuses it by name.

Planning is `TDMPC`'s, unchanged: the CEM of :136-200 is tdmpc.py's, so `plan` / `plan_batch` are inherited and run the
same kernels; `SimPlanner` only tells the packer about the encoder's LayerNorm and packs the TOLD tensors selected by
name in TOLD's order (`_predictor.*`, its integer `num_batches_tracked` included, never reaches the packer). As in
`TDMPC` the policy trajectories are cfg.mixture_coef of the samples and the horizon follows horizon_schedule at every
call; the reference's `regularization_schedule` ramp of that share and its episode-start latch of the horizon (:151-154)
are not reproduced, and `mixture_coef` keeps the schedule's value at step 0 (:82), which is what `update` reports.

Learning -- `update(replay_buffer, step)`, `update_pi(zs)`, `optim` / `pi_optim` -- is run by
`tdmpc_amd.sim_learner.SimLearner`, built on first use: an agent that only plans allocates none of it, and a cfg the
learner refuses still constructs and plans.

Out of scope: `finetune()` with a demo buffer; `dream` / `dream_loss` (the latter calls a `_td_target_latent` that the
reference does not define); pixel observations (the reference's pixel encoder is rlpyt's; a pixel cfg constructs with
helper.enc's conv stack and plans, `update` refuses it); norm_type other than 'ln'.
"""
from __future__ import annotations

import numpy as np
import torch

from .config import linear_schedule
from .drnn import DssmLearning
from .icem_mlp import IcemMlpModel
from .tdmpc import TDMPC, HipPlanner, pack_weights
from .told import TOLD
from . import _lib


class SimPlanner(HipPlanner):
    """HipPlanner over an `IcemMlpModel` (or a TOLD with the same encoder): the dims carry the encoder's LayerNorm, and
    `pack` takes the TOLD tensors by name in the packer's order (TOLD's state_dict order)."""

    def _make_dims(self, cfg, max_batch):
        self.enc_norm = cfg.modality != "pixels" and bool(getattr(cfg, "normalize", True))
        return _lib.dims_from_cfg(cfg, max_batch=max_batch, enc_norm=self.enc_norm)

    def told_keys(self):
        if getattr(self, "_told_keys", None) is None:
            with torch.device("meta"):
                self._told_keys = list(TOLD(self.cfg, init="none", enc_norm=self.enc_norm).state_dict().keys())
        return self._told_keys

    def pack_tensors(self, model):
        """The tensors handed to the packer, in its order."""
        sd = model.state_dict()
        return [sd[k] for k in self.told_keys()]

    def pack(self, model):
        pack_weights(self, model, self.pack_tensors, "tdmpc_", self.dims, False)


class TdMpcSim(DssmLearning, TDMPC):
    """Drop-in for the reference `TDMPCSIM` (tdmpc_similarity.py:75-375): plan, update, update_pi, save / load."""

    LEARNER, LEARNER_MODULE = "SimLearner", "sim_learner"

    def __init__(self, cfg, max_batch: int = 1, rng: str = "reference", graph: bool = True, path: str = "auto"):
        if bool(getattr(cfg, "normalize", True)) and getattr(cfg, "norm_type", "ln") != "ln":
            raise NotImplementedError(f"TdMpcSim: norm_type={cfg.norm_type!r} is not supported (the LayerNorm state "
                                      f"encoder, norm_type 'ln', only)")
        self._init_agent(cfg, IcemMlpModel, rng, graph)                        # :83-87
        self.mixture_coef = linear_schedule(cfg.regularization_schedule, 0)   # :82
        self.plan_horizon = 1                                                  # :89
        self.batch_size = cfg.batch_size                                       # :90
        self.planner = SimPlanner(cfg, max_batch=max_batch, device=self.device, path=path)
        from .learner import RandomShiftsAug
        self.aug = RandomShiftsAug(cfg)                                        # :85 (the identity on state observations)
        self._learner = None
        self._has_prev = np.zeros(max_batch, dtype=bool)
        self._prev_H = np.zeros(max_batch, dtype=np.int64)

    # ------------------------------------------------------------------ learning (:202-226, :298-375)
    def update(self, replay_buffer, step, sync_metrics=True, noise=None):
        """:298-375 -> the reference's metrics dict (floats; sync_metrics=False: 0-d device tensors, no
        synchronisation). noise: optional 2H + 1 [B, A] TruncatedNormal draws (H TD targets, H + 1 update_pi)."""
        from .sim_learner import METRICS
        self.std = linear_schedule(self.cfg.std_schedule, step)              # :302
        m = self.learner.update(replay_buffer, step, noise)
        out = dict(zip(METRICS, m.tolist() if sync_metrics else list(m.unbind(0))))
        out["mixture_coef"] = self.mixture_coef
        return out

    def _td_target(self, next_obs, reward):
        """:220-226."""
        return self.learner.td_target(next_obs, reward)
