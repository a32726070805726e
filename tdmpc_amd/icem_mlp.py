"""`TdIcemMlp`: the reference's MLP iCEM agent with its update -- `TdICEM`'s planner over the reference's full model.

Reference: src/algorithm/tdmpc_icem_similarity_mlp.py. `IcemMlpModel` is its `DSSM` (:14-74; the file reuses the name
for a model without a recurrent state): TOLD with the LayerNorm state encoder plus `_predictor`, the similarity head
(`helper.mlp_norm`: Linear, BatchNorm1d, ELU, Linear -- the module `tdmpc_amd.dssm.DSSM` has), in the reference's
construction order, so that its state_dict has the reference's keys, shapes and order and a checkpoint written by
`TdICemSimMlp.save` loads under strict key matching. `TdICEM.model` is a plain `TOLD` and stays one.

`TdIcemMlp(TdICEM)` plans as `TdICEM` does (the planner packs the TOLD tensors, selected by name in the packer's order;
`_predictor.*` plays no part in planning) and adds the reference's learning interface -- `update(replay_buffer, step)`,
`update_pi(zs)`, `optim` / `pi_optim`, `reward_rms`, `explore_coef` (:267-428) -- run by
`tdmpc_amd.icem_learner.IcemMlpLearner`, which is built on first use: an agent that only plans allocates none of it,
and a cfg the learner refuses still constructs and plans. `TdIcemMlp(cfg, engine=True)` or the environment variable
TDMPC_ICEM_LEARNER_ENGINE=1 selects `tdmpc_amd.icem_engine.IcemEngineLearner` instead: the same update as explicit HIP
passes over flat parameters, `optim` / `pi_optim` the engine's two Adam states.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from .config import linear_schedule
from .drnn import DssmLearning
from .dssm import _mlp_bn
from .icem import IcemPlanner, TdICEM
from .tdmpc import pack_weights
from .told import TOLD, _enc, _mlp, _orthogonal_init, _q


class IcemMlpModel(TOLD):
    """tdmpc_icem_similarity_mlp.py:14-74: the same state_dict keys, shapes and order. cfg.normalize=False gives the
    reference's other branch (plain encoder, `_predictor` a BatchNorm-free `helper.mlp`), which plans and loads but
    which the learner refuses."""

    def __init__(self, cfg, init: str = "reference"):
        nn.Module.__init__(self)
        self.cfg = cfg
        norm = bool(getattr(cfg, "normalize", True))
        L, A, M = cfg.latent_dim, cfg.action_dim, cfg.mlp_dim
        self._dynamics = _mlp(L + A, M, L)
        self._reward = _mlp(L + A, M, 1)
        self._pi = _mlp(L, M, A)
        self._Q1, self._Q2 = _q(cfg), _q(cfg)
        self._encoder = _enc(cfg, enc_norm=norm)
        self._predictor = _mlp_bn(L, M, L) if norm else _mlp(L, M, L)
        if init == "reference":
            self.apply(_orthogonal_init)
            for m in (self._reward, self._Q1, self._Q2):
                m[-1].weight.data.fill_(0)
                m[-1].bias.data.fill_(0)

    def track_model_grad(self, enable=True):
        for m in (self._Q1, self._Q2, self._reward, self._dynamics):
            for p in m.parameters():
                p.requires_grad_(enable)

    def pred_z(self, z):
        return self._predictor(z)


def synthetic_icem_mlp_state_dict(cfg, seed: int = 0) -> dict:
    """Deterministic non-degenerate `IcemMlpModel` weights, as dssm.synthetic_dssm_state_dict: tensor i of the
    state_dict from `np.random.RandomState(seed * 1000 + i)`. Linear weights N(0, 1/fan_in), the zero-initialised last
    layers of R / Q1 / Q2 included; biases N(0, 0.05^2); LayerNorm and BatchNorm gains 1 + N(0, 0.1^2), shifts
    N(0, 0.1^2); BatchNorm running_mean N(0, 0.1^2) and running_var uniform in [0.5, 1.5]."""
    model = IcemMlpModel(cfg, init="none")
    norm = ["_Q1.1.", "_Q1.4.", "_Q2.1.", "_Q2.4."]
    if bool(getattr(cfg, "normalize", True)):
        norm += ["_encoder.1.", "_predictor.1."]
    norm = tuple(norm)
    sd = {}
    for i, (k, v) in enumerate(model.state_dict().items()):
        rs = np.random.RandomState(seed * 1000 + i)
        shape = tuple(v.shape)
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(1000, dtype=torch.int64)
            continue
        if k.endswith("running_mean"):
            arr = 0.1 * rs.standard_normal(shape)
        elif k.endswith("running_var"):
            arr = rs.uniform(0.5, 1.5, shape)
        elif k.startswith(norm) and k.endswith("weight"):
            arr = 1.0 + 0.1 * rs.standard_normal(shape)
        elif k.startswith(norm):
            arr = 0.1 * rs.standard_normal(shape)
        elif k.endswith("weight"):
            arr = rs.standard_normal(shape) / np.sqrt(int(np.prod(shape[1:])))
        else:
            arr = 0.05 * rs.standard_normal(shape)
        sd[k] = torch.from_numpy(arr.astype(np.float32))
    return sd


class IcemMlpPlanner(IcemPlanner):
    """IcemPlanner over an `IcemMlpModel`: packs the TOLD tensors, selected by name in the packer's order (TOLD's
    state_dict order); `_predictor.*`, its integer `num_batches_tracked` included, is not packed."""

    def __init__(self, cfg, **kw):
        super().__init__(cfg, **kw)
        enc_norm = bool(getattr(cfg, "normalize", False))
        with torch.device("meta"):
            self.told_keys = list(TOLD(cfg, init="none", enc_norm=enc_norm).state_dict().keys())

    def pack(self, model):
        def tensors(m):
            sd = m.state_dict()
            return [sd[k] for k in self.told_keys]
        pack_weights(self, model, tensors, "tdmpc_", self.dims, False)


class TdIcemMlp(DssmLearning, TdICEM):
    """Drop-in for the reference `TdICemSimMlp` (tdmpc_icem_similarity_mlp.py:77-428): plan, update, update_pi."""

    LEARNER, LEARNER_MODULE = "IcemMlpLearner", "icem_learner"

    def __init__(self, cfg, max_batch: int = 1, rng: str = "reference", path: str = "auto", graph: bool = True,
                 engine: bool = False):
        self.use_engine = bool(engine)
        if getattr(cfg, "modality", "state") != "state":
            raise NotImplementedError("iCEM drop-in: state observations (the pixel DSSM encoder is rlpyt's)")
        if bool(getattr(cfg, "normalize", False)) and getattr(cfg, "norm_type", "ln") != "ln":
            raise NotImplementedError("iCEM drop-in: the LayerNorm state encoder (norm_type 'ln')")
        self._init_agent(cfg, IcemMlpModel, rng, graph)                        # :83-88
        self.mixture_coef = linear_schedule(cfg.regularization_schedule, 0)   # :82
        self.plan_horizon = 1                                                  # :90
        pl = self.planner = IcemMlpPlanner(cfg, max_batch=max_batch, device=self.device, path=path)
        self.P_max, self.E_max, self.elites = pl.pmax, pl.E_max, pl.elites
        self._dev_plans = {}
        self._has_prev = False
        self._has_elites = False
        self._elite_H = 0
        self.explore_coef = 0
        self._learner = None

    @property
    def learner(self):
        """`IcemMlpLearner`, or with engine=True or TDMPC_ICEM_LEARNER_ENGINE=1 when it is first built
        `icem_engine.IcemEngineLearner` (the update on the learner engine), which raises for a cfg or
        a device it does not admit: the agent then still plans."""
        if self._learner is None and (self.use_engine or os.environ.get("TDMPC_ICEM_LEARNER_ENGINE", "0") == "1"):
            self.LEARNER, self.LEARNER_MODULE = "IcemEngineLearner", "icem_engine"
        return DssmLearning.learner.fget(self)

    def update(self, replay_buffer, step, sync_metrics=True, noise=None):
        """:346-428 -> the reference's metrics dict (floats; sync_metrics=False: 0-d device tensors, no
        synchronisation). noise: optional 2H + 1 [B, A] TruncatedNormal draws (H TD targets, H + 1 update_pi)."""
        out, self.explore_coef = self._learn(replay_buffer, step, sync_metrics, noise)
        out["current_explore_coef"] = self.explore_coef
        out["mixture_coef"] = self.mixture_coef
        return out
