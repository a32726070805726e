"""`TdIcemDrnn`: the reference's recurrent-latent iCEM agent's planning API on MI355X.

Reference: `TdICemSimDssm` in src/algorithm/tdmpc_icem_similarity_drnn.py:81-272 (built by train_icem_drnn.py,
train_icem_dyna_episode_drnn.py and train_multi_experiments.py). Same constructor argument, the same model
(`tdmpc_amd.dssm.DSSM`), checkpoint `load / save / state_dict`, planner state (`plan_horizon`, `mixture_coef`, `std`,
`_prev_mean`, `_elite_actions`) and `plan(obs, hidden, eval_mode=False, step=None, t0=True) -> (action [A],
hidden [1, Hd], metrics)`. The whole plan is one `tdmpc_drnn_plan_icem` call (include/tdmpc_drnn.h): the iCEM order
of work of `TdICEM` with the rollout step on drnn_step_kernel from the env's GRU state, and at the end the GRU state
after `DSSM.next(z0, action, hidden)` with the returned action (:267).

Where this agent's file differs from the MLP one (tdmpc_icem_similarity_mlp.py) and this class follows it (:204-234):
reused elites enter only when `not t0`, in every iteration (E_i = 0 for the whole call at an episode start); all N_i
samples of an iteration come from `sample_action_sequence` -- coloured with cfg.noise_beta over plan_horizon samples
when it is > 0, white otherwise -- not from white / pink / brown thirds; `extend_horizon` can only be set on a t0
call and reuse happens only on a non-t0 call, so the elite horizon at reuse always equals the plan horizon.

Randomness: `rng="reference"` consumes torch's device generator and numpy's global generator in the reference's
order (the coloured sequences through tdmpc_amd.colored_noise, as `TdICEM`); `rng="device"` draws the call's streams
with one normal_, the spectrum normals with another and turns them into every coloured block of every env with one
`tdmpc_drnn_colored_noise` launch; `plan(..., noise=IcemNoise-like)` takes explicit draws (parity tests).

Learning: `update(replay_buffer, step)`, `update_pi(zs)`, `optim` / `pi_optim`, `explore_coef` and `reward_rms` as the
reference's (:367-384, :421-553), run by `tdmpc_amd.drnn_learner.DssmLearner` through `tdmpc_amd.drnn.DssmLearning`,
which builds it on first use (an agent that only plans allocates none of it, and a cfg the learner refuses -- the dog
task's batch of 2048 -- still plans). Opt-in, `TdIcemDrnn(cfg, engine=True)` or TDMPC_DSSM_LEARNER_ENGINE=1 when the
learner is first built: `tdmpc_amd.dssm_engine.DssmEngineLearner`, the same update on the explicit learner engine
(DESIGN.md §7 f14). `TdMpcDrnn` does not read the variable.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from .colored_noise import irfft_matrices, powerlaw_psd_gaussian, spectrum_rows
from .config import linear_schedule
from .drnn import DrnnPlanner, DssmLearning
from .dssm import DSSM, check_dssm_cfg
from .icem import (IcemBuffers, icem_counts, icem_draw_reference, icem_layout, icem_load, icem_params,
                   icem_trace_values)
from .tdmpc import Agent


def colored_noise_params(L, A, batch, env_stride, normals_env, jobs, betas):
    """tdmpc_colored_noise_params for sequences of L samples: jobs = [(spectrum, n, rows, c0, dst, src)], betas = the
    spectra's exponents. Factor rows and the inverse-DFT matrix are computed in float64 and passed as float32."""
    if not 2 <= L <= 16:
        raise ValueError(f"coloured noise needs 2..16 samples per sequence, not {L}")
    if len(jobs) > _lib.NOISE_MAX_JOBS or len(betas) > _lib.NOISE_MAX_SPECTRA:
        raise ValueError(f"{len(jobs)} jobs / {len(betas)} spectra (at most {_lib.NOISE_MAX_JOBS} / "
                         f"{_lib.NOISE_MAX_SPECTRA})")
    p = _lib.ColoredNoiseParams()
    p.L, p.A, p.batch, p.n_jobs, p.n_spectra = L, A, batch, len(jobs), len(betas)
    p.env_stride, p.normals_env = env_stride, normals_env
    for j, (sp, n, rows, c0, dst, src) in enumerate(jobs):
        J = p.jobs[j]
        J.spectrum, J.n, J.rows, J.c0, J.dst, J.src = sp, n, rows, c0, dst, src
    F = L // 2 + 1
    for s, beta in enumerate(betas):
        re, im, inv = spectrum_rows(beta, L)
        for k in range(F):
            p.re[s][k] = float(re[k] * inv)
            p.im[s][k] = float(im[k] * inv)
    Cr, Ci = irfft_matrices(L)
    for k, row in enumerate(np.concatenate([Cr, Ci])):
        for t in range(L):
            p.dft[k][t] = float(row[t])
    return p


def colored_noise(L_lib, params, normals, noise, stream=None):
    """One tdmpc_drnn_colored_noise launch: normals (flat float32 device tensor) -> blocks of `noise` (flat). L_lib:
    the loaded library (`_lib.lib()`), which `_lib.call` reaches on its own; kept in the signature for its callers."""
    if stream is None:
        stream = torch.cuda.current_stream(noise.device).cuda_stream
    _lib.call("tdmpc_drnn_colored_noise", params, normals, normals.numel(), noise, noise.numel(), stream)


class IcemDrnnPlanner(IcemBuffers, DrnnPlanner):
    """DrnnPlanner with the iCEM workspace (N + K + num_pi rows per env) and noise stream bound; `ddims.base.num_pi`
    stays at the schedule's largest value (the calls pass their own counts in tdmpc_icem_params)."""

    entry, sizes_abi = "tdmpc_drnn_plan_icem", "tdmpc_drnn_icem_sizes_for"


class TdIcemDrnn(DssmLearning, Agent):
    """Drop-in for the reference `TdICemSimDssm` planning interface (tdmpc_icem_similarity_drnn.py:81-272)."""

    MAX_GRAPHS = 8   # captured plans kept per agent
    RNGS = ("reference", "device")
    HIDDEN = True

    def __init__(self, cfg, max_batch: int = 1, rng: str = "reference", graph: bool = True, engine: bool = False):
        self.use_engine = bool(engine)
        check_dssm_cfg(cfg)
        if not 1 <= int(cfg.iterations) <= 16:
            raise ValueError("iCEM: 1..16 iterations")
        self._init_agent(cfg, DSSM, rng, graph)                               # :87, :89
        self.mixture_coef = linear_schedule(cfg.regularization_schedule, 0)   # :88
        self.plan_horizon = 1                                                 # :98
        pl = self.planner = IcemDrnnPlanner(cfg, max_batch=max_batch, device=self.device)
        dev = self.device
        A, K, N, H = cfg.action_dim, cfg.num_elites, cfg.num_samples, cfg.horizon
        self.P_max, self.E_max, self.elites = pl.pmax, pl.E_max, pl.elites
        self.Tw = N + K + self.P_max
        self.hidden_out = torch.zeros(max_batch, pl.hidden_dim, dtype=torch.float32, device=dev)
        # spectrum normals of one call (rng 'device')
        self._normals = torch.zeros(max_batch * 2 * (H // 2 + 1) * (cfg.iterations * N + self.E_max) * A,
                                    dtype=torch.float32, device=dev)
        self._noise_params = {}
        self._has_prev = False
        self._has_elites = False
        self.explore_coef = 0                                                 # :99
        self._learner = None

    # ------------------------------------------------------------------ learning (:367-384, :421-553)
    @property
    def learner(self):
        """`DssmLearner`, or with engine=True or TDMPC_DSSM_LEARNER_ENGINE=1 when it is first built
        `dssm_engine.DssmEngineLearner` (the update on the learner engine), which raises for a cfg or
        a device it does not admit: the agent then still plans."""
        if self._learner is None and (self.use_engine or os.environ.get("TDMPC_DSSM_LEARNER_ENGINE", "0") == "1"):
            self.LEARNER, self.LEARNER_MODULE = "DssmEngineLearner", "dssm_engine"
        return DssmLearning.learner.fget(self)

    def update(self, replay_buffer, step, sync_metrics=True, noise=None):
        """:445-553 -> the reference's metrics dict (floats; sync_metrics=False: 0-d device tensors, no
        synchronisation). noise: optional 2H + 1 [B, A] TruncatedNormal draws (parity tests)."""
        out, self.explore_coef = self._learn(replay_buffer, step, sync_metrics, noise)   # (:449: std)
        out["current_explore_coef"] = self.explore_coef
        out["mixture_coef"] = self.mixture_coef
        return out

    # ------------------------------------------------------------------ reference state
    @property
    def _prev_mean(self):
        if not self._has_prev:
            raise AttributeError("_prev_mean")
        return self.planner.prev_mean_view(self.plan_horizon, 1)[0]

    @property
    def _elite_actions(self):
        if not self._has_elites:
            raise AttributeError("_elite_actions")
        return self.elites[0, :self.plan_horizon]

    # ------------------------------------------------------------------ counts and layout (tdmpc_amd.icem's)
    def counts(self, mixture, has_elites, t0):
        """(N_i, P_i, E_i) per iteration (:205-215): reused elites only inside an episode."""
        return icem_counts(self.cfg, self.E_max, mixture, has_elites, reuse_ok=not t0)

    def layout(self, H, cts, reuse):
        return icem_layout(self.cfg.action_dim, H, cts, reuse)

    def _colored_blocks(self, H, cts, off, reuse):
        """The coloured blocks of one env's stream in draw order: (n, stream offset)."""
        out = []
        for i, (n, p, e) in enumerate(cts):
            out.append((n, off["samp"][i]))
            if i == 0 and reuse:
                out.append((e, off["reuse"]))
        return out

    # ------------------------------------------------------------------ draws
    def _draw_device(self, B, H, cts, off, reuse):
        """rng 'device': the B streams white in one draw; with noise_beta > 0 the spectrum normals in a second draw and
        one tdmpc_drnn_colored_noise launch over every sample block and reuse tail of every env; the picks' uniforms."""
        pl, cfg = self.planner, self.cfg
        S = off["total"]
        pl.noise_flat[:B * S].normal_()
        if cfg.noise_beta > 0:
            key = (H, tuple(cts), reuse, B)
            ent = self._noise_params.get(key)
            if ent is None:
                A, F = cfg.action_dim, H // 2 + 1
                jobs, src = [], 0
                for n, dst in self._colored_blocks(H, cts, off, reuse):
                    jobs.append((0, n, n, 0, dst, src))
                    src += 2 * F * n * A
                ent = (colored_noise_params(H, A, B, S, src, jobs, [cfg.noise_beta]), src)
                if len(self._noise_params) > 16:
                    self._noise_params.clear()
                self._noise_params[key] = ent
            prm, per_env = ent
            z = self._normals[:B * per_env]
            z.normal_()
            colored_noise(pl.L, prm, z, pl.noise_flat[:B * S])
        pl.u[:B].uniform_()

    def _draw_reference(self, e, H, cts, off, reuse, eval_mode):
        """Env e's stream in the reference's order (icem_draw_reference): every sample block and the reuse tail are
        numpy's coloured sequences when noise_beta > 0, torch's white draws otherwise."""
        cfg, A, dev = self.cfg, self.cfg.action_dim, self.device
        colored = cfg.noise_beta > 0

        def draw_host():
            if not colored:
                return None, None
            ns = [n for n, _ in self._colored_blocks(H, cts, off, reuse)]
            host = [powerlaw_psd_gaussian(cfg.noise_beta, (n, A, H)).astype(np.float32).transpose(2, 0, 1).reshape(-1)
                    for n in ns]
            return ns, np.concatenate(host) if host else np.zeros(0, np.float32)

        def compose(buf, i, n, ne, cols):
            for cnt, o in [(n, off["samp"][i])] + ([(ne, off["reuse"])] if i == 0 and reuse else []):
                blk = next(cols) if colored else torch.randn(H, cnt, A, device=dev)
                buf[o:o + H * cnt * A].copy_(blk.view(-1))

        return icem_draw_reference(self.planner, e, H, cts, off, eval_mode, draw_host, compose, False)

    def _load(self, e, H, cts, off, reuse, nz):
        S = off["total"]
        return icem_load(self.planner.noise_flat[e * S:(e + 1) * S], self.cfg.action_dim, H, cts, off, reuse, nz)

    # ------------------------------------------------------------------ plan
    @torch.no_grad()
    def plan(self, obs, hidden, eval_mode=False, step=None, t0=True, noise=None, trace=None):
        """:169-272 -> (action [A], hidden [1, Hd], metrics); at seed steps (uniform action, None, zero metrics)."""
        if self._seed_step(step, eval_mode):
            return self._seed_return()
        obs = torch.as_tensor(np.asarray(obs), dtype=torch.float32).view(1, -1)
        hidden = torch.as_tensor(hidden, dtype=torch.float32).reshape(1, -1)
        a, h, m = self._plan_envs(obs, hidden, eval_mode, step, t0, None if noise is None else [noise], trace)
        return a[0], h, m[0]

    @torch.no_grad()
    def plan_batch(self, obs, hidden, eval_mode=False, step=None, t0=True, noise=None, trace=None):
        """B environments at the same step / t0: obs [B, obs_dim], hidden [B, Hd] -> (actions [B, A], hidden [B, Hd],
        metrics list). Equivalent to B reference agents sharing weights, the draws taken env by env."""
        obs = torch.as_tensor(np.asarray(obs) if not torch.is_tensor(obs) else obs, dtype=torch.float32)
        B = obs.shape[0]
        if self._seed_step(step, eval_mode):
            return self._seed_return(B)
        hidden = torch.as_tensor(hidden, dtype=torch.float32).reshape(B, -1)
        return self._plan_envs(obs.view(B, -1), hidden, eval_mode, step, bool(t0), noise, trace)

    def _plan_envs(self, obs, hidden, eval_mode, step, t0, noise, trace):
        cfg, pl = self.cfg, self.planner
        B = obs.shape[0]
        self._check_call(B, hidden)
        if t0:   # :179-182: the schedule moves the plan horizon only at an episode start
            self.plan_horizon = self.horizon(step)
        H = self.plan_horizon
        self.mixture_coef = linear_schedule(cfg.regularization_schedule, step)
        cts = self.counts(self.mixture_coef, self._has_elites, t0)
        if any(p <= 0 for _, p, _ in cts):
            raise AssertionError("num_pi_trajs > 0")   # the reference asserts this (:193, :209)
        if cts[0][1] > self.P_max:
            raise ValueError("mixture_coef above the schedule's maximum")
        if any(e > 0 for _, _, e in cts[1:]) and not cfg.keep_previous_elites:
            # the reference would re-use the first iteration's `reused_actions` (a stale loop variable), or none
            raise NotImplementedError("fraction_elites_reused > 0 needs keep_previous_elites")
        if cts[0][2] > 0 and not cfg.shift_elites_over_time:
            raise NotImplementedError("fraction_elites_reused > 0 needs shift_elites_over_time once elites exist "
                                      "(the reference's `reused_actions` is unbound there)")
        if cfg.noise_beta > 0 and H < 2:
            raise ValueError("coloured noise (noise_beta > 0) has no spectrum for a plan horizon of 1: the generator "
                             "raises at one sample; use noise_beta = 0 or a horizon_schedule starting at 2")
        reuse = cts[0][2] > 0
        warm = (not t0) and self._has_prev
        off = self.layout(H, cts, reuse)
        if B * off["total"] > pl.noise_flat.numel():
            raise ValueError("noise stream exceeds the planner's buffer")
        pl.pack(self.model)
        pl.hidden_buf[:B].copy_(hidden.to(self.device))
        pl.obs_buf[:B].copy_(obs.to(self.device))
        if noise is not None:
            us = [self._load(e, H, cts, off, reuse, nz) for e, nz in enumerate(noise)]
            pl.u[:B].copy_(torch.tensor(us, dtype=torch.float64))
        elif self.rng == "reference":
            us = [self._draw_reference(e, H, cts, off, reuse, eval_mode) for e in range(B)]
            pl.u[:B].copy_(torch.tensor(us, dtype=torch.float64))
        # (elite_horizon = H: reuse happens inside an episode only, where the horizon does not move)
        p = icem_params(cfg, B, H, cts, off, reuse, warm, eval_mode, self.std, pl.status, "chain_x6", H)
        outs = {}
        if trace is not None:
            I, A, dev = cfg.iterations, cfg.action_dim, self.device
            outs = dict(value=torch.zeros(B, I, self.Tw, device=dev), mean=torch.zeros(B, I, H, A, device=dev),
                        std=torch.zeros(B, I, H, A, device=dev))
        g = outs.get

        def device_work():
            if noise is None and self.rng == "device":
                self._draw_device(B, H, cts, off, reuse)
            _lib.call("tdmpc_drnn_plan_icem", pl.ddims, p, pl.packed, pl.obs_buf, pl.hidden_buf, pl.noise_flat, pl.u,
                      pl.prev_mean_flat, pl.elites, pl.action, pl.metrics, self.hidden_out, pl.z_in, g("value"),
                      g("mean"), g("std"), *pl._ws(), pl._stream())

        captured = self.graph and noise is None and trace is None
        key = (H, B, tuple(cts), reuse, warm, bool(eval_mode), float(self.std), self.rng)
        pl.run(device_work, key if captured else None, self.MAX_GRAPHS)
        if trace is not None:
            trace.update(value=icem_trace_values(outs["value"], cts),
                         mean=outs["mean"], std=outs["std"], counts=cts, z_in=pl.z_in[:B].clone())
        self._has_prev = True
        self._has_elites = True
        m = self._metrics(B)
        return pl.action[:B].clone(), self.hidden_out[:B].clone(), m
