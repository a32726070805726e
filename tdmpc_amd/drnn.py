"""`TdMpcDrnn`: the reference's recurrent-latent (DSSM) agent's planning API on MI355X.

Reference: `TdMpcSimDssm` in src/algorithm/tdmpc_similarity_drnn.py:87-267. Same constructor argument (a cfg
namespace), attributes (`cfg`, `device`, `std`, `mixture_coef`, `model`, `model_target`, `plan_horizon`,
`memory_latents`, `_prev_mean`), `plan(obs, hidden, eval_mode=False, step=None, t0=True) -> (action [A], metrics)`
and `state_dict / save / load`. Planning runs in the HIP library (include/tdmpc_drnn.h): the rollout step is
drnn_step_kernel (a fused layer-normed GRU cell + prior MLP + reward MLP), everything else -- the encoder, the
terminal pi / Q chain kernels, the CEM kernel, the noise layout and the reference-order draws -- is the TDMPC
planner's. The learner (`update`, the similarity loss) and plan2explore are not part of this class.

`plan_batch(obs[B], hidden[B], ...)` plans B environments in one call, each with its own memory, `_prev_mean` and
plan horizon; the envs of one call must agree on the horizon (the kernels take one).
"""
from __future__ import annotations

import ctypes as C
from collections import deque
from copy import deepcopy

import numpy as np
import torch

from . import _lib
from .config import linear_schedule
from .dssm import DSSM, check_dssm_cfg, float_tensors
from .tdmpc import Checkpointed, HipPlanner


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

    def _query_sizes(self):
        sz = _lib.Sizes()
        _lib.check(self.L.tdmpc_drnn_sizes_for(C.byref(self.ddims), C.byref(sz)), "tdmpc_drnn_sizes_for")
        return sz

    def set_num_pi(self, P: int):
        self.ddims.base.num_pi = int(P)
        self.P, self.T = int(P), self.N + int(P)
        self._ref_adv = self._ref_adv_by_p.setdefault(int(P), {})

    # ------------------------------------------------------------------ weights
    def pack(self, model: DSSM):
        """Pack the DSSM's floating-point tensors (state_dict order) when any of them changed."""
        if self._packed_key is not None and self._packed_model is model:
            key = tuple((p.data_ptr(), p._version) for p in self._packed_params)
            if key == self._packed_key:
                return
        params = float_tensors(model.state_dict())
        if self._packed_model is not None and self._packed_model is not model:
            self.L.tdmpc_pack_forget(C.c_void_p(self.packed.data_ptr()))
        self._packed_model, self._packed_params = model, params
        key = tuple((p.data_ptr(), p._version) for p in params)
        n = self.L.tdmpc_drnn_num_param_tensors(C.byref(self.ddims))
        if n != len(params):
            raise ValueError(f"DSSM has {len(params)} float tensors, the packer expects {n}")
        # device fp32 copies kept per planner, so the pointer set (the key of the library's job-table record) is the
        # same from one repack to the next
        stage = getattr(self, "_pack_stage", None)
        if stage is None:
            stage = self._pack_stage = [torch.empty(p.shape, dtype=torch.float32, device=self.device) for p in params]
        for s, p in zip(stage, params):
            s.copy_(p.detach())
        arr = (C.c_void_p * n)(*[s.data_ptr() for s in stage])
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self.L.tdmpc_drnn_pack_weights(C.byref(self.ddims), arr, n, C.c_void_p(self.packed.data_ptr()),
                                                  self.packed.numel() * 4, C.c_void_p(stream)),
                   "tdmpc_drnn_pack_weights")
        self._packed_key = key

    # ------------------------------------------------------------------ calls
    def _ws(self):
        return C.c_void_p(self.workspace.data_ptr()), self.workspace.numel() * 4

    def launch(self, prm, obs_is_u8: bool = False, trace: dict | None = None):
        stream = torch.cuda.current_stream(self.device).cuda_stream
        B, H, I, K = prm.batch, prm.horizon, prm.iterations, self.dims.num_elites
        outs = {}
        if trace is not None:
            outs = dict(elite=torch.zeros(B, H, K, self.A, device=self.device),
                        score=torch.zeros(B, K, device=self.device),
                        value=torch.zeros(B, I, self.T, device=self.device),
                        mean=torch.zeros(B, I, H, self.A, device=self.device),
                        std=torch.zeros(B, I, H, self.A, device=self.device))
            trace.update(outs)
        g = outs.get
        vp = C.c_void_p
        ws, wsb = self._ws()
        rc = self.L.tdmpc_drnn_plan(C.byref(self.ddims), C.byref(prm), vp(self.packed.data_ptr()),
                                    vp(self.obs_buf.data_ptr()), vp(self.hidden_buf.data_ptr()),
                                    vp(self.noise_flat.data_ptr()), vp(self.u.data_ptr()),
                                    vp(self.prev_mean_flat.data_ptr()), vp(self.action.data_ptr()),
                                    vp(self.metrics.data_ptr()), vp(self.z_in.data_ptr()),
                                    vp(_lib.ptr(g("elite"))), vp(_lib.ptr(g("score"))), vp(_lib.ptr(g("value"))),
                                    vp(_lib.ptr(g("mean"))), vp(_lib.ptr(g("std"))), ws, wsb, vp(stream))
        _lib.check(rc, "tdmpc_drnn_plan")

    def next(self, z, a, h, h_out=None):
        """DSSM.next for rows of (z [R, L], a [R, A], h [R, Hd]) -> (z' [R, L], h' [R, Hd], reward [R])."""
        dev = self.device
        z = z.to(dev, torch.float32).contiguous()
        a = a.to(dev, torch.float32).contiguous()
        h = h.to(dev, torch.float32).contiguous()
        R = z.shape[0]
        zo = torch.empty(R, self.dims.latent_dim, device=dev)
        ho = torch.empty(R, self.hidden_dim, device=dev) if h_out is None else h_out
        ro = torch.empty(R, device=dev)
        vp = C.c_void_p
        ws, wsb = self._ws()
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self.L.tdmpc_drnn_next(C.byref(self.ddims), vp(self.packed.data_ptr()), vp(z.data_ptr()), vp(a.data_ptr()),
                                    vp(h.data_ptr()), R, vp(zo.data_ptr()), vp(ho.data_ptr()), vp(ro.data_ptr()),
                                    ws, wsb, vp(stream))
        _lib.check(rc, "tdmpc_drnn_next")
        return zo, ho, ro

    def estimate_value(self, z0, h0, actions, eps_term, H: int):
        """TdMpcSimDssm.estimate_value for B envs: z0 [B, L], h0 [B, Hd], actions [B, H, T, A], eps_term [B, T, A]
        -> (value [B, T], reward at t = H-1 [B, T])."""
        B = z0.shape[0]
        prm = self.params(H, 1, B, False, True, 0.05)
        dev = self.device
        z0, h0, actions, eps_term = (t.to(dev, torch.float32).contiguous() for t in (z0, h0, actions, eps_term))
        value = torch.empty(B, self.T, device=dev)
        rlast = torch.empty(B, self.T, device=dev)
        vp = C.c_void_p
        ws, wsb = self._ws()
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self.L.tdmpc_drnn_estimate_value(C.byref(self.ddims), C.byref(prm), vp(self.packed.data_ptr()),
                                              vp(z0.data_ptr()), vp(h0.data_ptr()), vp(actions.data_ptr()),
                                              vp(eps_term.data_ptr()), self.T, vp(value.data_ptr()),
                                              vp(rlast.data_ptr()), ws, wsb, vp(stream))
        _lib.check(rc, "tdmpc_drnn_estimate_value")
        return value, rlast

    def pi_rollout(self, z0, h0, eps_pi, H: int):
        """The policy pre-rollout for B envs: z0 [B, L], h0 [B, Hd], eps_pi [B, H, P, A] -> pi_actions [B, H, P, A]."""
        B = z0.shape[0]
        prm = self.params(H, 1, B, False, True, 0.05)
        dev = self.device
        z0, h0, eps_pi = (t.to(dev, torch.float32).contiguous() for t in (z0, h0, eps_pi))
        out = torch.empty(B, H, self.P, self.A, device=dev)
        vp = C.c_void_p
        ws, wsb = self._ws()
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self.L.tdmpc_drnn_pi_rollout(C.byref(self.ddims), C.byref(prm), vp(self.packed.data_ptr()),
                                          vp(z0.data_ptr()), vp(h0.data_ptr()), vp(eps_pi.data_ptr()),
                                          vp(out.data_ptr()), ws, wsb, vp(stream))
        _lib.check(rc, "tdmpc_drnn_pi_rollout")
        return out


class TdMpcDrnn(Checkpointed):
    """Drop-in for the reference `TdMpcSimDssm` planning interface (tdmpc_similarity_drnn.py:87-267)."""

    MAX_GRAPHS = 8   # captured plans kept per agent (one per (horizon, iterations, batch, num_pi, eval_mode))
    METRICS0 = {"intrinsic_reward_mean": 0.0, "external_reward_mean": 0.0, "current_std": 0.0}

    def __init__(self, cfg, max_batch: int = 1, rng: str = "reference", graph: bool = True):
        check_dssm_cfg(cfg)
        self.cfg = cfg
        self.device = torch.device(cfg.device)
        self.std = linear_schedule(cfg.std_schedule, 0)                              # :93
        self.mixture_coef = linear_schedule(cfg.regularization_schedule, 0)          # :94
        self.model = DSSM(cfg).to(self.device)                                       # :95
        self.model_target = deepcopy(self.model)
        self.model.eval()
        self.model_target.eval()
        if rng not in ("reference", "fused"):
            raise ValueError(rng)
        self.rng = rng
        self.graph = graph
        self.planner = DrnnPlanner(cfg, max_batch=max_batch, device=self.device)
        self.max_batch = max_batch
        wl = int(getattr(cfg, "warmup_len", 0))
        self._memories = [deque(maxlen=wl) for _ in range(max_batch)]               # :109, one per env
        self._plan_H = np.ones(max_batch, dtype=np.int64)                            # :108, one per env
        self._has_prev = np.zeros(max_batch, dtype=bool)
        self._prev_H = np.zeros(max_batch, dtype=np.int64)

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
        cfg = self.cfg
        if step < cfg.seed_steps and not eval_mode:
            return (torch.empty(cfg.action_dim, dtype=torch.float32, device=self.device).uniform_(-1, 1),
                    dict(self.METRICS0))
        hidden = torch.as_tensor(hidden, dtype=torch.float32).reshape(1, -1)
        a, m = self._plan_envs(np.asarray(obs)[None], hidden, eval_mode, step, [t0],
                               None if noise is None else [noise], trace)
        return a[0].clone(), m[0]

    @torch.no_grad()
    def plan_batch(self, obs, hidden, eval_mode=False, step=None, t0=True, noise=None, trace=None):
        """B environments at once: obs [B, obs_dim], hidden [B, Hd], t0 a bool or a per-env sequence. Equivalent to B
        reference agents sharing weights, the draws taken env by env in reference order."""
        cfg = self.cfg
        obs = obs if torch.is_tensor(obs) else np.asarray(obs)
        B = obs.shape[0]
        if step < cfg.seed_steps and not eval_mode:
            a = torch.empty(B, cfg.action_dim, dtype=torch.float32, device=self.device)
            for e in range(B):
                a[e].uniform_(-1, 1)
            return a, [dict(self.METRICS0) for _ in range(B)]
        t0s = [t0] * B if isinstance(t0, (bool, int, np.bool_)) else list(t0)
        hidden = torch.as_tensor(hidden, dtype=torch.float32).reshape(B, -1)
        return self._plan_envs(obs, hidden, eval_mode, step, t0s, noise, trace)

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
        if B > pl.max_batch:
            raise ValueError(f"batch {B} > max_batch {pl.max_batch}")
        if hidden.shape != (B, pl.hidden_dim):
            raise ValueError(f"hidden must be [{B}, {pl.hidden_dim}], not {tuple(hidden.shape)}")
        # :193-197: the schedule moves an env's plan horizon only at its episode start
        horizon = int(min(cfg.horizon, linear_schedule(cfg.horizon_schedule, step)))
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
        warm = []
        for e in range(B):
            w = (not t0s[e]) and bool(self._has_prev[e])
            if w and self._prev_H[e] != H:
                raise RuntimeError(f"shape mismatch: prev_mean horizon {self._prev_H[e]} vs {H}")
            warm.append(w)
        pl.pack(self.model)
        pl.hidden_buf[:B].copy_(self._replay_memory(hidden, B))
        host = not torch.is_tensor(obs) or obs.device.type == "cpu"
        if pl._h2d_done is not None:
            pl._h2d_done.synchronize()
        if host:
            pl._h_obs[:B] = np.asarray(obs, dtype=np.float32).reshape(B, -1)
        else:
            pl.obs_buf[:B].copy_(obs.to(self.device, torch.float32).view(B, -1))
        pl.set_call_state(self.std, warm)
        if noise is not None:
            for e, nb in enumerate(noise):
                pl.load_noise(e, H, I, nb.eps_pi, nb.eps_cem, nb.eps_term, nb.eps_act)
                pl._h_u[e] = float(nb.u)
        elif self.rng == "reference":
            for e in range(B):
                pl._h_u[e] = np.random.random_sample()   # np.random.choice's uniform (:254)
        one_launch = noise is None and self.rng == "reference"
        if one_launch:
            pl.stage_reference_state(B, H, I, eval_mode)
        lo = 0 if host else pl._u_off
        pl._stage_d[lo:].copy_(pl._stage_h[lo:], non_blocking=True)
        if pl._h2d_done is not None:
            pl._h2d_done.record()

        def device_work():
            if noise is None:
                if one_launch:
                    pl.launch_reference_draws(B, H, I, eval_mode)
                else:
                    pl.noise_view(H, I, B).normal_()
                    pl.u[:B].uniform_()
            pl.launch(pl.device_state_params(pl.params(H, I, B, warm[0], eval_mode, self.std)), False, trace)

        if self.graph and noise is None and trace is None:
            key = (H, I, B, P, bool(eval_mode), self.rng)
            g = pl._graphs.get(key)
            if g is None:
                # a ramping regularization_schedule gives a new P (a new graph) per step: keep the latest few
                while len(pl._graphs) >= self.MAX_GRAPHS:
                    pl._graphs.pop(next(iter(pl._graphs)))
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    device_work()
                pl._graphs[key] = g
            g.replay()
        else:
            device_work()
        self._has_prev[:B] = True
        self._prev_H[:B] = H
        if pl._h2d_done is not None:   # status + metrics: one copy into pinned memory, as TDMPC does
            pl._pin_ms[:4 + 2 * B].copy_(pl._ms_dev[:4 + 2 * B], non_blocking=True)
            torch.cuda.current_stream(self.device).synchronize()
            ms = pl._pin_ms
        else:
            ms = pl._ms_dev[:4 + 2 * B].cpu()
        pl.raise_status(int(ms[:1].view(torch.int32)[0]))
        m = ms[4:4 + 2 * B].view(B, 2).double().tolist()
        actions = pl.action[:B].clone()
        z_in = pl.z_in[:B].clone()
        for e in range(B):   # :261: the latent and the (noised) action, for the next call's replay
            self._memories[e].append((z_in[e], actions[e]))
        return actions, [{"intrinsic_reward_mean": 0.0, "external_reward_mean": float(r), "current_std": float(s)}
                         for r, s in m]
