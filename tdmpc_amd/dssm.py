"""DSSM parameter container with the reference's module tree and state_dict key names.

Reference: `DSSM` in `src/algorithm/tdmpc_similarity_drnn.py:15-84`: dynamics = `DGruDyna` (`models/gru_dyna.py:11-29`:
a `NormGRUCell`, `models/rnns.py:8-29`, followed by `prior_mlp = helper.mlp_norm(hidden_dim, mlp_dim, latent_dim)`,
whose norm is BatchNorm1d because DGruDyna passes no norm_type), a reward MLP on the GRU hidden state, and pi / Q1 / Q2 /
the state `dmlab_enc_norm` encoder as in TOLD; `_predictor` (the similarity head) is in the state_dict but unused by
planning.

Restricted to what the HIP planner runs: state observations, `norm_cell=True`, `normalize=True`, `norm_type='ln'`,
`plan2expl=False`; anything else raises at construction with the setting named. Planning does NOT run these modules
(`TdMpcDrnn.plan` packs the parameters and runs the HIP kernels); the eager `next` is the reference's forward,
kept for users of the module tree (tests/test_drnn_cpu.py holds it to the restatement the planner is checked with).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from .told import _enc, _mlp, _orthogonal_init, _q, truncated_normal_sample


def check_dssm_cfg(cfg):
    """Raise for the settings the DSSM planner does not cover (each named)."""
    if not hasattr(cfg, "hidden_dim"):
        raise AttributeError("DSSM: cfg.hidden_dim (the GRU cell's width; the reference's default is 128) is not set")
    if getattr(cfg, "modality", "state") != "state":
        raise NotImplementedError(f"DSSM: modality={cfg.modality!r} is not supported (state observations only; the "
                                  "reference's pixel encoder lives in a package that is not part of it)")
    if not getattr(cfg, "norm_cell", True):
        raise NotImplementedError("DSSM: norm_cell=False (the plain nn.GRUCell variant) is not supported")
    if getattr(cfg, "plan2expl", False):
        raise NotImplementedError("DSSM: plan2expl=True (plan2explore ensembles) is not supported")
    if not getattr(cfg, "normalize", True):
        raise NotImplementedError("DSSM: normalize=False is not supported (the LayerNorm state encoder only)")
    if getattr(cfg, "norm_type", "ln") != "ln":
        raise NotImplementedError(f"DSSM: norm_type={cfg.norm_type!r} is not supported ('ln' only)")


class NormGRUCell(nn.Module):
    """models/rnns.py:8-29."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.weight_ih = nn.Linear(input_size, 3 * hidden_size, bias=False)
        self.weight_hh = nn.Linear(hidden_size, 3 * hidden_size, bias=False)
        self.ln_reset = nn.LayerNorm(hidden_size, eps=1e-3)
        self.ln_update = nn.LayerNorm(hidden_size, eps=1e-3)
        self.ln_newval = nn.LayerNorm(hidden_size, eps=1e-3)

    def forward(self, input, state):
        gates_i = self.weight_ih(input)
        gates_h = self.weight_hh(state)
        reset_i, update_i, newval_i = gates_i.chunk(3, 1)
        reset_h, update_h, newval_h = gates_h.chunk(3, 1)
        reset = torch.sigmoid(self.ln_reset(reset_i + reset_h))
        update = torch.sigmoid(self.ln_update(update_i + update_h))
        newval = torch.tanh(self.ln_newval(newval_i + reset * newval_h))
        return update * newval + (1 - update) * state


def _mlp_bn(in_dim, hidden_dim, out_dim) -> nn.Sequential:
    """helper.mlp_norm with its default norm_type 'bn' (helper.py:179-184)."""
    return nn.Sequential(nn.Linear(in_dim, hidden_dim), nn.BatchNorm1d(hidden_dim), nn.ELU(),
                         nn.Linear(hidden_dim, out_dim))


class DGruDyna(nn.Module):
    """models/gru_dyna.py:11-29 (norm_cell=True)."""

    def __init__(self, cfg):
        super().__init__()
        self.prior_mlp = _mlp_bn(cfg.hidden_dim, cfg.mlp_dim, cfg.latent_dim)
        self.gru_cell = NormGRUCell(cfg.latent_dim + cfg.action_dim, cfg.hidden_dim)
        self.hidden_dim = cfg.hidden_dim

    def init_hidden_state(self, batch_size, device):
        return torch.zeros((batch_size, self.hidden_dim), device=device)

    def forward(self, obs_embed, action, h_prev):
        h = self.gru_cell(torch.cat([obs_embed, action], dim=-1), h_prev)
        return self.prior_mlp(h), h


class DSSM(nn.Module):
    """tdmpc_similarity_drnn.py:15-84: the same state_dict keys, shapes and order."""

    def __init__(self, cfg, init: str = "reference"):
        super().__init__()
        check_dssm_cfg(cfg)
        self.cfg = cfg
        self._dynamics = DGruDyna(cfg)
        self._reward = _mlp(cfg.hidden_dim, cfg.mlp_dim, 1)
        self._pi = _mlp(cfg.latent_dim, cfg.mlp_dim, cfg.action_dim)
        self._Q1, self._Q2 = _q(cfg), _q(cfg)
        self._encoder = _enc(cfg, enc_norm=True)
        self._predictor = _mlp_bn(cfg.latent_dim, cfg.mlp_dim, cfg.latent_dim)
        if init == "reference":
            self.apply(_orthogonal_init)
            for m in (self._reward, self._Q1, self._Q2):
                m[-1].weight.data.fill_(0)
                m[-1].bias.data.fill_(0)

    def h(self, obs):
        return self._encoder(obs)

    def next(self, z, a, h_prev):
        z, hidden = self._dynamics(z, a, h_prev)
        return z, hidden, self._reward(hidden)

    def init_hidden_state(self, batch_size, device):
        return self._dynamics.init_hidden_state(batch_size, device)

    def Q(self, z, a):
        x = torch.cat([z, a], dim=-1)
        return self._Q1(x), self._Q2(x)

    # What the learner (tdmpc_amd/drnn_learner.py) differentiates besides `next` (tdmpc_icem_similarity_drnn.py:36-78)
    def track_q_grad(self, enable=True):
        for m in (self._Q1, self._Q2):
            for p in m.parameters():
                p.requires_grad_(enable)

    def track_model_grad(self, enable=True):
        for m in (self._Q1, self._Q2, self._reward, self._dynamics):
            for p in m.parameters():
                p.requires_grad_(enable)

    def pi(self, z, std=0, eps=None):
        """tanh(pi(z)), plus a TruncatedNormal(mu, std).sample(clip=0.3) when std > 0 (`eps`: the N(0, 1) draw to use
        instead of drawing one -- parity tests)."""
        mu = torch.tanh(self._pi(z))
        if std > 0:
            return truncated_normal_sample(mu, torch.ones_like(mu) * std, clip=0.3, noise=eps)
        return mu

    def pred_z(self, z):
        return self._predictor(z)


def float_tensors(sd: dict) -> list:
    """The floating-point tensors of a DSSM state_dict in its order (tdmpc_drnn_pack_weights' argument): everything but
    the BatchNorms' num_batches_tracked."""
    return [v for k, v in sd.items() if not k.endswith("num_batches_tracked")]


def synthetic_dssm_state_dict(cfg, seed: int = 0) -> dict:
    """Deterministic non-degenerate DSSM weights, in the style of told.synthetic_state_dict: tensor i of the state_dict
    from `np.random.RandomState(seed * 1000 + i)`. Linear weights N(0, 1/fan_in), the zero-initialised last layers of
    R / Q1 / Q2 included; biases N(0, 0.05^2); LayerNorm and BatchNorm gains 1 + N(0, 0.1^2), shifts N(0, 0.1^2);
    BatchNorm running_mean N(0, 0.1^2) and running_var uniform in [0.5, 1.5], so the BatchNorm is not an identity."""
    model = DSSM(cfg, init="none")
    sd = {}
    norm = ("_dynamics.prior_mlp.1.", "_dynamics.gru_cell.ln_", "_predictor.1.", "_encoder.1.",
            "_Q1.1.", "_Q1.4.", "_Q2.1.", "_Q2.4.")
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
