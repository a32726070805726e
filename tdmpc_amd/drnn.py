"""`TdMpcDrnn`: the reference's recurrent-latent (DSSM) agent's planning API on MI355X.

Reference: `TdMpcSimDssm` in src/algorithm/tdmpc_similarity_drnn.py:87-267. Same constructor argument (a cfg
namespace), attributes (`cfg`, `device`, `std`, `mixture_coef`, `model`, `model_target`, `plan_horizon`,
`memory_latents`, `_prev_mean`), `plan(obs, hidden, eval_mode=False, step=None, t0=True) -> (action [A], metrics)`
and `state_dict / save / load`. Planning runs in the HIP library (include/tdmpc_drnn.h): the rollout step is
drnn_step_kernel (a fused layer-normed GRU cell + prior MLP + reward MLP), everything else -- the encoder, the
terminal pi / Q chain kernels, the CEM kernel, the noise layout and the reference-order draws -- is the TDMPC
planner's. plan2explore is not part of this class.

Learning: `update(replay_buffer, step)`, `update_pi(zs)`, `optim` / `pi_optim` and `reward_rms` as the reference's
(:269-286, :373-496), run by `tdmpc_amd.drnn_learner.DssmSimLearner` through `DssmLearning`, the block of lazily built
learner state that this agent and `TdIcemDrnn` share: an agent that only plans allocates none of it, and a cfg the
learner refuses (cfgs/default.yaml's `warmup_len: 0`, the dog task's batch of 2048) still plans.

`plan_batch(obs[B], hidden[B], ...)` plans B environments in one call, each with its own memory, `_prev_mean` and
plan horizon; the envs of one call must agree on the horizon (the kernels take one).
"""
from __future__ import annotations

import importlib
from collections import deque

import numpy as np
import torch

from . import _lib
from .config import linear_schedule
from .dssm import DSSM, check_dssm_cfg, float_tensors
from .tdmpc import Agent, HipPlanner, pack_weights


def _schedule_ends(schdl):
    """The two end values of a schedule string (a constant gives one)."""
    import re
    try:
        return [float(schdl)]
    except (TypeError, ValueError):
        m = re.match(r"linear\((.+),(.+),(.+),(.+)\)", schdl)
        if not m:
            raise NotImplementedError(schdl)
        return [float(m.group(1)), float(m.group(2))]


class DrnnPlanner(HipPlanner):
    """Device buffers of one DSSM planner and the calls into include/tdmpc_drnn.h. `dims` is the planner part of
    `ddims` (shared memory): its num_pi follows the call's regularization_schedule value (`set_num_pi`), the buffers
    are sized for the largest."""

    def __init__(self, cfg, max_batch: int = 1, device=None):
        super().__init__(cfg, max_batch=max_batch, device=device, path="chain_x6")
        self.hidden_dim = int(cfg.hidden_dim)
        self.hidden_buf = torch.zeros(max_batch, self.hidden_dim, dtype=torch.float32, device=self.device)
        self.z_in = torch.zeros(max_batch, self.dims.latent_dim, dtype=torch.float32, device=self.device)
        self._ref_adv_by_p = {}
        self.set_num_pi(self.P)

    def _make_dims(self, cfg, max_batch):
        N = int(cfg.num_samples)
        pmax = max(int(m * N) for m in _schedule_ends(cfg.regularization_schedule))
        self.pmax = pmax
        self.ddims = _lib.drnn_dims_from_cfg(cfg, max_batch=max_batch, num_pi=pmax)
        return self.ddims.base

    entry, sizes_abi = "tdmpc_drnn_plan", "tdmpc_drnn_sizes_for"

    def abi_dims(self):
        return self.ddims

    def set_num_pi(self, P: int):
        self.ddims.base.num_pi = int(P)
        self.P, self.T = int(P), self.N + int(P)
        self._ref_adv = self._ref_adv_by_p.setdefault(int(P), {})

    def pack(self, model: DSSM):
        """Pack the DSSM's floating-point tensors (state_dict order) when any of them changed, always through device
        fp32 copies kept per planner."""
        pack_weights(self, model, lambda m: float_tensors(m.state_dict()), "tdmpc_drnn_", self.ddims, True)

    # ------------------------------------------------------------------ calls
    def _plan_io(self, obs_is_u8):
        return self.hidden_buf, (self.z_in,)

    def next(self, z, a, h, h_out=None):
        """DSSM.next for rows of (z [R, L], a [R, A], h [R, Hd]) -> (z' [R, L], h' [R, Hd], reward [R])."""
        dev = self.device
        z, a, h = (t.to(dev, torch.float32).contiguous() for t in (z, a, h))
        R = z.shape[0]
        zo = torch.empty(R, self.dims.latent_dim, device=dev)
        ho = torch.empty(R, self.hidden_dim, device=dev) if h_out is None else h_out
        ro = torch.empty(R, device=dev)
        _lib.call("tdmpc_drnn_next", self.ddims, self.packed, z, a, h, R, zo, ho, ro, *self._ws(), self._stream())
        return zo, ho, ro

    def estimate_value(self, z0, h0, actions, eps_term, H: int):
        """TdMpcSimDssm.estimate_value for B envs: z0 [B, L], h0 [B, Hd], actions [B, H, T, A], eps_term [B, T, A]
        -> (value [B, T], reward at t = H-1 [B, T])."""
        B, dev = z0.shape[0], self.device
        value, rlast = torch.empty(B, self.T, device=dev), torch.empty(B, self.T, device=dev)
        self._call("tdmpc_drnn_estimate_value", H, 0.05, (z0, h0, actions, eps_term), self.T, value, rlast)
        return value, rlast

    def pi_rollout(self, z0, h0, eps_pi, H: int):
        """The policy pre-rollout for B envs: z0 [B, L], h0 [B, Hd], eps_pi [B, H, P, A] -> pi_actions [B, H, P, A]."""
        out = torch.empty(z0.shape[0], H, self.P, self.A, device=self.device)
        self._call("tdmpc_drnn_pi_rollout", H, 0.05, (z0, h0, eps_pi), out)
        return out


class DssmLearning:
    """The learning half of an agent with a similarity head: `learner` (the class named by LEARNER in the module
    tdmpc_amd.<LEARNER_MODULE>) is built on first use and sets `optim` / `pi_optim`; reading either, or `reward_rms`,
    builds it."""

    LEARNER, LEARNER_MODULE = "DssmLearner", "drnn_learner"
    _learner = None

    @property
    def learner(self):
        if self._learner is None:
            module = importlib.import_module("." + self.LEARNER_MODULE, __package__)
            self._learner = getattr(module, self.LEARNER)(self, graph=self.graph)   # sets optim / pi_optim
        return self._learner

    @property
    def reward_rms(self):
        return self.learner.reward_rms

    def _optim_get(name):
        def get(self):
            self.learner
            return self.__dict__["_" + name]
        return property(get, lambda self, v: self.__dict__.__setitem__("_" + name, v))

    optim, pi_optim = _optim_get("optim"), _optim_get("pi_optim")
    del _optim_get

    def update_pi(self, zs):
        """The reference's `update_pi` -> pi_loss (float; synchronises)."""
        try:
            return float(self.learner.update_pi(zs))
        finally:
            self.planner._packed_key = None   # the policy changed in place: the next plan() repacks

    def _learn(self, replay_buffer, step, sync_metrics, noise):
        """One update -> ({metric: value}, explore_coef): floats, or with sync_metrics=False 0-d device tensors and no
        synchronisation. Sets `std` from std_schedule as the reference's update does."""
        from .drnn_learner import METRICS
        self.std = linear_schedule(self.cfg.std_schedule, step)
        m, coef = self.learner.update(replay_buffer, step, noise)
        return dict(zip(METRICS, m.tolist() if sync_metrics else list(m.unbind(0)))), coef


class TdMpcDrnn(DssmLearning, Agent):
    """Drop-in for the reference `TdMpcSimDssm` (tdmpc_similarity_drnn.py:87-496): plan, update, update_pi."""

    LEARNER = "DssmSimLearner"

    MAX_GRAPHS = 8   # captured plans kept per agent (one per (horizon, iterations, batch, num_pi, eval_mode))
    METRICS0 = {"intrinsic_reward_mean": 0.0, "external_reward_mean": 0.0, "current_std": 0.0}

    def __init__(self, cfg, max_batch: int = 1, rng: str = "reference", graph: bool = True):
        check_dssm_cfg(cfg)
        self._init_agent(cfg, DSSM, rng, graph)                                      # :93, :95
        self.mixture_coef = linear_schedule(cfg.regularization_schedule, 0)          # :94
        self.planner = DrnnPlanner(cfg, max_batch=max_batch, device=self.device)
        wl = int(getattr(cfg, "warmup_len", 0))
        self._memories = [deque(maxlen=wl) for _ in range(max_batch)]               # :109, one per env
        self._plan_H = np.ones(max_batch, dtype=np.int64)                            # :108, one per env
        self._has_prev = np.zeros(max_batch, dtype=bool)
        self._prev_H = np.zeros(max_batch, dtype=np.int64)

    # ------------------------------------------------------------------ learning (:269-286, :373-496)
    def update(self, replay_buffer, step, sync_metrics=True, noise=None):
        """:404-496 -> the reference's metrics dict and `intrinsic_batch_reward_mean` (floats; sync_metrics=False: 0-d
        device tensors, no synchronisation). noise: optional explicit draws (DssmSimLearner; parity tests)."""
        out, _ = self._learn(replay_buffer, step, sync_metrics, noise)
        out["mixture_coef"] = self.mixture_coef
        return out

    # ------------------------------------------------------------------ reference API
    @property
    def memory_latents(self):
        return self._memories[0]

    @property
    def plan_horizon(self):
        return int(self._plan_H[0])

    @property
    def _prev_mean(self):
        if not self._has_prev[0]:
            raise AttributeError("_prev_mean")
        return self.planner.prev_mean_view(int(self._prev_H[0]), 1)[0]

    @torch.no_grad()
    def plan(self, obs, hidden, eval_mode=False, step=None, t0=True, noise=None, trace=None):
        """:184-267. hidden: the caller's GRU state [1, Hd] (or [Hd]); the memory of the last warmup_len
        (latent, action) pairs is replayed from it before planning. Returns (action [A], the three metrics)."""
        if self._seed_step(step, eval_mode):
            return self._seed_return()
        hidden = torch.as_tensor(hidden, dtype=torch.float32).reshape(1, -1)
        a, m = self._plan_envs(np.asarray(obs)[None], hidden, eval_mode, step, [t0],
                               None if noise is None else [noise], trace)
        return a[0].clone(), m[0]

    @torch.no_grad()
    def plan_batch(self, obs, hidden, eval_mode=False, step=None, t0=True, noise=None, trace=None):
        """B environments at once: obs [B, obs_dim], hidden [B, Hd], t0 a bool or a per-env sequence. Equivalent to B
        reference agents sharing weights, the draws taken env by env in reference order."""
        obs = obs if torch.is_tensor(obs) else np.asarray(obs)
        B = obs.shape[0]
        if self._seed_step(step, eval_mode):
            return self._seed_return(B)
        hidden = torch.as_tensor(hidden, dtype=torch.float32).reshape(B, -1)
        return self._plan_envs(obs, hidden, eval_mode, step, self._per_env(t0, B), noise, trace)

    # ------------------------------------------------------------------ internals
    def _replay_memory(self, hidden, B):
        """hidden [B, Hd] advanced through each env's memory (:198-200); envs with shorter memories sit a step out."""
        pl = self.planner
        h = hidden.to(self.device, torch.float32).contiguous().clone()
        steps = max((len(self._memories[e]) for e in range(B)), default=0)
        for j in range(steps):
            act = [e for e in range(B) if len(self._memories[e]) > j]
            z = torch.stack([self._memories[e][j][0] for e in act])
            a = torch.stack([self._memories[e][j][1] for e in act])
            if len(act) == B:
                pl.next(z, a, h, h_out=h)
            else:
                idx = torch.tensor(act, device=self.device)
                h[idx] = pl.next(z, a, h[idx])[1]
        return h

    def _plan_envs(self, obs, hidden, eval_mode, step, t0s, noise=None, trace=None):
        cfg, pl = self.cfg, self.planner
        B = obs.shape[0]
        self._check_call(B, hidden)
        # :193-197: the schedule moves an env's plan horizon only at its episode start
        horizon = self.horizon(step)
        for e in range(B):
            if horizon != self._plan_H[e] and t0s[e]:
                self._plan_H[e] = horizon
        H = int(self._plan_H[0])
        if any(int(self._plan_H[e]) != H for e in range(B)):
            raise ValueError(f"the envs of one plan_batch call must share the plan horizon, not {self._plan_H[:B]}")
        self.mixture_coef = linear_schedule(cfg.regularization_schedule, step)
        P = int(self.mixture_coef * cfg.num_samples)
        if P > pl.pmax:
            raise ValueError(f"{P} policy trajectories exceed the planner's buffers ({pl.pmax})")
        pl.set_num_pi(P)
        I = int(cfg.iterations)
        warm = self._warm(t0s, H)
        pl.pack(self.model)
        pl.hidden_buf[:B].copy_(self._replay_memory(hidden, B))
        reference = self.rng == "reference"
        one_launch = noise is None and reference
        pl.stage_call(obs, B, H, I, eval_mode, self.std, warm, noise, reference, one_launch)

        def device_work():
            if noise is None:
                if one_launch:
                    pl.launch_reference_draws(B, H, I, eval_mode)
                else:
                    pl.noise_view(H, I, B).normal_()
                    pl.u[:B].uniform_()
            pl.launch(pl.device_state_params(pl.params(H, I, B, warm[0], eval_mode, self.std)), False, trace)

        # a ramping regularization_schedule gives a new P (a new graph) per step: keep the latest few
        captured = self.graph and noise is None and trace is None
        pl.run(device_work, (H, I, B, P, bool(eval_mode), self.rng) if captured else None, self.MAX_GRAPHS)
        self._has_prev[:B] = True
        self._prev_H[:B] = H
        m = self._metrics(B)
        actions = pl.action[:B].clone()
        z_in = pl.z_in[:B].clone()
        for e in range(B):   # :261: the latent and the (noised) action, for the next call's replay
            self._memories[e].append((z_in[e], actions[e]))
        return actions, m
