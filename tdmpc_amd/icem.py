"""`TdICEM`: drop-in for the reference iCEM agent's planning API on MI355X.

Reference: `TdICemSimMlp` in /root/reference/src/algorithm/tdmpc_icem_similarity_mlp.py:74-265 (driven by
src/train_icem_mlp.py). Same `plan(obs, eval_mode=False, step=None, t0=True) -> (action [A], metrics)`, the same
planner state (`plan_horizon`, `mixture_coef`, `std`, `_prev_mean`, `_elite_actions`) and the same model heads
(TOLD with the DSSM's LayerNorm state encoder when cfg.normalize / norm_type 'ln'). The whole plan -- encoder, the
policy pre-rollout, every iteration's rollout of [sampled | reused elites] candidates, terminal policy + Q,
top-k / softmax refit, elite reuse bookkeeping, the final pick -- is one `tdmpc_plan_icem` call on the chain
kernels (include/tdmpc_hip.h); Python draws the random numbers and lays out their per-env stream.

Differences from TDMPC.plan that the kernels follow: N shrinks per iteration (N_i = max(2K, int(N_{i-1} /
factor_decrease_num))), P_i = int(mixture_coef(step) * N_i) (regularization_schedule), std starts at 0.5, a warm
start keeps mean[-1] = prev_mean[-1], int(fraction_elites_reused * K) elites are re-evaluated (time-shifted from
the previous plan in the first iteration with a fresh coloured tail, the previous iteration's afterwards), the last
iteration's sample 0 is the mean, and the sample noise is white / pink (beta 1) / brown (beta 2.5) thirds.

Randomness (`rng="reference"`): torch's and numpy's global generators in the reference's order; the coloured
thirds come from tdmpc_amd.colored_noise on numpy's global RandomState (the reference's `colorednoise` is
absent and unpinned; 2.x seeds each call from OS entropy, so its stream is not reproducible anyway).
`rng="device"` draws everything on the device in ~8 launches (the stream white in one draw, every coloured third
and reuse tail from one batched spectrum draw per sample length with the irfft as a matmul, the pick's uniform):
same distributions, no host work. `plan(..., noise=IcemNoise)` takes explicit draws (parity tests).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .colored_noise import BatchedColoredNoise, _scales as _spectrum
from .config import linear_schedule
from .tdmpc import Agent, HipPlanner, _discount_pows
from .told import TOLD


def _thirds(n):
    q, r = divmod(n, 3)
    return [q, q, q] if r == 0 else ([q, q + 1, q] if r == 1 else [q, q + 1, q + 1])


# ---------------------------------------------------------------------- bookkeeping shared with drnn_icem.TdIcemDrnn
def icem_counts(cfg, E_max, mixture, has_elites, reuse_ok=True):
    """(N_i, P_i, E_i) per iteration (tdmpc_icem_similarity_mlp.py:201-210, _drnn.py:205-215). reuse_ok: this call may
    re-evaluate elites at all (the recurrent agent's file allows it only inside an episode: `not t0`)."""
    out, n = [], cfg.num_samples
    for i in range(cfg.iterations):
        if i > 0:
            n = max(2 * cfg.num_elites, int(n / cfg.factor_decrease_num))
        p = int(mixture * n)
        e = E_max if (cfg.fraction_elites_reused > 0 and reuse_ok and (has_elites or i > 0)) else 0
        out.append((n, p, e))
    return out


def icem_layout(A, H, cts, reuse):
    """Per-env noise stream offsets (floats): the pre-rollout's draws, per iteration [samples | at i = 0 with reuse
    the fresh elite tail | terminal policy noise], the action noise."""
    off = {"pi": 0, "samp": [], "term": [], "reuse": 0}
    o = H * cts[0][1] * A
    for i, (n, p, e) in enumerate(cts):
        off["samp"].append(o)
        o += H * n * A
        if i == 0 and reuse:
            off["reuse"] = o
            o += H * e * A
        off["term"].append(o)
        o += (n + e + p) * A
    off["act"] = o
    off["total"] = o + A
    return off


def icem_load(buf, A, H, cts, off, reuse, nz):
    """Explicit draws (oracle IcemNoise: eps_pi [H, P0, A], samp[i] [H, N_i, A], reuse [H, E, A], term[i] [T_i, A], u,
    eps_act [A]) into one env's stream `buf`; returns u."""
    def put(o, count, t):   # (a draw of another size than the layout's fails in copy_)
        buf[o:o + count].copy_(t.reshape(-1).to(buf.device, torch.float32))
    put(0, H * cts[0][1] * A, nz.eps_pi)
    for i, (n, p, e) in enumerate(cts):
        put(off["samp"][i], H * n * A, nz.samp[i])
        if i == 0 and reuse:
            put(off["reuse"], H * e * A, nz.reuse)
        put(off["term"][i], (n + e + p) * A, nz.term[i])
    if nz.eps_act is not None:
        put(off["act"], A, nz.eps_act)
    return float(nz.u)


def icem_params(cfg, B, H, cts, off, reuse, warm, eval_mode, std, status, path, elite_horizon):
    """tdmpc_icem_params of one call (status: the agent's device status word)."""
    p = _lib.IcemParams()
    p.horizon, p.iterations, p.batch = H, cfg.iterations, B
    p.warm_start, p.eval_mode, p.has_elites = int(warm), int(eval_mode), int(reuse)
    p.elite_horizon = elite_horizon
    p.n_pi0 = cts[0][1]
    p.path = _lib.PATHS[path]
    for i, (n, pp, e) in enumerate(cts):
        p.n_samples[i], p.n_pi[i], p.n_elite[i] = n, pp, e
        p.samp_off[i], p.term_off[i] = off["samp"][i], off["term"][i]
    p.reuse_off, p.pi_off, p.act_off, p.env_stride = off["reuse"], 0, off["act"], off["total"]
    p.min_std, p.temperature, p.momentum = cfg.min_std, cfg.temperature, cfg.momentum
    p.one_minus_momentum = float(1 - cfg.momentum)
    p.std_floor, p.init_std = float(std), 0.5
    for t, v in enumerate(_discount_pows(cfg.discount, H)):
        p.discount_pow[t] = v
    p.status = status.data_ptr()
    return p


def icem_trace_values(value, cts):
    """value_out [B, I, Tw] -> per iteration the values of its T_i = N_i + E_i + P_i candidates, [B, T_i]."""
    return [value[:, i, :n + e + pp] for i, (n, pp, e) in enumerate(cts)]


def icem_draw_reference(pl, e, H, cts, off, eval_mode, draw_host, compose, act_in_place):
    """Env e's stream in the reference's draw order on torch's (device) and numpy's global generators. The two
    generators are independent, so numpy's draws run first on the host -- draw_host() -> (row counts n of the coloured
    [H, n, A] blocks in draw order, their float32 values or None), then the pick's uniform, which is returned -- and
    travel in ONE pinned async copy; torch's follow in order: the pre-rollout's normals, per iteration whatever
    compose(buf, i, n, ne, cols) draws while it fills the sample block and the reuse tail (cols: an iterator over the
    device copies of the coloured blocks) and the terminal policy noise, then the action noise."""
    A, S = pl.A, off["total"]
    buf = pl.noise_flat[e * S:(e + 1) * S]
    ns, host = draw_host()
    u = float(np.random.random_sample())
    cols = []
    if host is not None and host.size:
        dst, o = pl.stage_colored(host), 0
        for n in ns:
            cols.append(dst[o:o + H * n * A].view(H, n, A))
            o += H * n * A
    cols = iter(cols)
    P0 = cts[0][1]
    for t in range(H):
        buf[t * P0 * A:(t + 1) * P0 * A].view(P0, A).normal_()
    for i, (n, p, ne) in enumerate(cts):
        compose(buf, i, n, ne, cols)
        buf[off["term"][i]:off["term"][i] + (n + ne + p) * A].view(n + ne + p, A).normal_()
    if not eval_mode:
        act = buf[off["act"]:off["act"] + A]
        if act_in_place:
            act.normal_()
        else:
            act.copy_(torch.randn(A, device=pl.device))
    return u


class IcemBuffers:
    """What both iCEM planners hold beside their base planner's buffers: the elites kept from call to call and the
    hand-over of the host-drawn coloured blocks (rng 'reference')."""

    def __init__(self, cfg, **kw):
        super().__init__(cfg, **kw)
        A, K, N, H, dev = cfg.action_dim, cfg.num_elites, cfg.num_samples, cfg.horizon, self.device
        self.E_max = int(cfg.fraction_elites_reused * K)
        self.elites = torch.zeros(self.max_batch, H, K, A, dtype=torch.float32, device=dev)
        self.col_max = cfg.iterations * H * N * A + H * self.E_max * A   # coloured floats of one env and call
        self._col_d = torch.empty(self.col_max, dtype=torch.float32, device=dev)
        self._col_h = torch.empty(self.col_max, dtype=torch.float32, pin_memory=dev.type == "cuda")
        self._col_done = None

    def stage_colored(self, host):
        """One env's host-drawn coloured floats -> their device copy, through the pinned block (one async copy)."""
        if self._col_done is not None:
            self._col_done.synchronize()   # the previous copy has left the pinned buffer
        stage = self._col_h[:host.size]
        stage.numpy()[:] = host
        dst = self._col_d[:host.size]
        dst.copy_(stage, non_blocking=True)
        self._col_done = torch.cuda.Event()
        self._col_done.record()
        return dst


class IcemPlanner(IcemBuffers, HipPlanner):
    """HipPlanner with the iCEM workspace (N + K + num_pi rows per env; num_pi: the regularization_schedule's largest
    value, the calls pass their own counts in tdmpc_icem_params) and a noise stream sized here: tdmpc_icem_sizes_for
    reports none, the stream's layout being the caller's."""

    entry, sizes_abi = "tdmpc_plan_icem", "tdmpc_icem_sizes_for"
    # TdICEM launches eagerly and then waits for the plan: there the pinned copy + stream synchronize came out at
    # 1.90 or 1.97-2.05 ms per one-env plan() depending on the core the process sat on, the blocking copy at 1.91-1.95
    pin_read_back = False

    def _make_dims(self, cfg, max_batch):
        rs = str(cfg.regularization_schedule)
        mix_max = max(linear_schedule(rs, 0), linear_schedule(rs, 10**12))
        self.pmax = max(1, int(mix_max * cfg.num_samples))
        d = _lib.dims_from_cfg(cfg, max_batch=max_batch, enc_norm=bool(getattr(cfg, "normalize", False)))
        d.num_pi = self.pmax
        return d

    def _noise_floats(self, sz):
        cfg = self.cfg
        A, N, H = cfg.action_dim, cfg.num_samples, cfg.horizon
        E = int(cfg.fraction_elites_reused * cfg.num_elites)
        # per-env stream upper bound: pre-rollout + per iteration (samples + terminal) + reuse tail + action
        return H * self.pmax * A + cfg.iterations * (H * N * A + (N + E + self.pmax) * A) + H * E * A + A


class TdICEM(Agent):
    RNGS = ("reference", "device")

    def __init__(self, cfg, max_batch: int = 1, rng: str = "reference", path: str = "auto"):
        if getattr(cfg, "modality", "state") != "state":
            raise NotImplementedError("iCEM drop-in: state observations (the pixel DSSM encoder is rlpyt's)")
        enc_norm = bool(getattr(cfg, "normalize", False))
        if enc_norm and getattr(cfg, "norm_type", "ln") != "ln":
            raise NotImplementedError("iCEM drop-in: the LayerNorm state encoder (norm_type 'ln')")
        self._init_agent(cfg, lambda c: TOLD(c, enc_norm=enc_norm), rng)        # :84, :86-87
        self.mixture_coef = linear_schedule(cfg.regularization_schedule, 0)   # :85
        self.plan_horizon = 1                                                  # :93
        pl = self.planner = IcemPlanner(cfg, max_batch=max_batch, device=self.device, path=path)
        self.P_max, self.E_max, self.elites = pl.pmax, pl.E_max, pl.elites
        self._dev_plans = {}
        self._has_prev = False
        self._has_elites = False
        self._elite_H = 0

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
        return self.elites[0, :self._elite_H]

    # ------------------------------------------------------------------ plan
    def counts(self, mixture, has_elites):
        return icem_counts(self.cfg, self.E_max, mixture, has_elites)

    def _layout(self, H, cts, reuse):
        return icem_layout(self.cfg.action_dim, H, cts, reuse)

    def _colored_specs(self, H, cts, reuse):
        """The coloured-noise draws of one plan call in the reference's order: (beta, n, length, kind, i)."""
        cfg, out = self.cfg, []
        for i, (n, p, ne) in enumerate(cts):
            n0, n1, n2 = _thirds(n)
            out += [(1.0, n1, cfg.horizon, "samp", i), (2.5, n2, cfg.horizon, "samp", i)]
            if i == 0 and reuse and cfg.noise_beta > 0:
                out.append((cfg.noise_beta, ne, H, "reuse", i))
        return out

    def _colored_host(self, specs, H):
        """All of a call's coloured noise on the host -> float32 [sum_k H * n_k * A] ([H][n][A] per draw).
        Numbers identical to consecutive powerlaw_psd_gaussian calls on numpy's global RandomState: one
        standard_normal draw of the whole call (the legacy generator's stream does not depend on how it is
        chunked; normal(scale=s) is s * standard_normal), one irfft per spectrum length (row-independent)."""
        A = self.cfg.action_dim
        sizes = [n * A * ((L // 2) + 1) for _, n, L, _, _ in specs]
        z = np.random.standard_normal(2 * sum(sizes))
        parts, o = [], 0
        for (beta, n, L, _, _), sz in zip(specs, sizes):
            sc, sigma = _spectrum(beta, L)
            sr = z[o:o + sz].reshape(n, A, -1) * sc
            si = z[o + sz:o + 2 * sz].reshape(n, A, -1) * sc
            o += 2 * sz
            if not L % 2:
                si[..., -1] = 0
                sr[..., -1] *= np.sqrt(2)
            si[..., 0] = 0
            sr[..., 0] *= np.sqrt(2)
            parts.append((sr + 1j * si, sigma))
        out = []
        for L in sorted({s[2] for s in specs}):
            idx = [k for k, s in enumerate(specs) if s[2] == L]
            y = np.fft.irfft(np.concatenate([parts[k][0] for k in idx]), n=L, axis=-1)
            r = 0
            for k in idx:
                n = specs[k][1]
                out.append((k, (y[r:r + n] / parts[k][1]).astype(np.float32)[:, :, :H].transpose(2, 0, 1)))
                r += n
        out.sort(key=lambda t: t[0])
        return np.concatenate([a.reshape(-1) for _, a in out]) if out else np.zeros(0, np.float32)

    def _device_plan(self, H, cts, off, reuse, B=1):
        """rng 'device': per sample length, a BatchedColoredNoise over that length's coloured specs of B envs and
        the stream positions [R, H] its rows land on (samp thirds [H][n][A] at their column offset, reuse tail;
        env e's stream at e * off['total'])."""
        key = (H, tuple(cts), reuse, B)
        plan = self._dev_plans.get(key)
        if plan is not None:
            return plan
        A = self.cfg.action_dim
        groups = {}
        for beta, n, L, kind, i in self._colored_specs(H, cts, reuse):
            nt = cts[i][0]
            n0, n1, _ = _thirds(nt)
            if kind == "samp":
                base, rows, c0 = off["samp"][i], nt, (n0 if beta == 1.0 else n0 + n1)
            else:
                base, rows, c0 = off["reuse"], n, 0
            t = np.arange(H)[None, None, :]
            r = np.arange(n)[:, None, None]
            a = np.arange(A)[None, :, None]
            pos = base + t * rows * A + (c0 + r) * A + a                   # [n, A, H]
            g = groups.setdefault(L, ([], []))
            for e in range(B):
                g[0].append((beta, n))
                g[1].append(pos.reshape(n * A, H) + e * off["total"])
        plan = []
        for L, (sp, pos) in sorted(groups.items()):
            plan.append((BatchedColoredNoise(sp, A, L, H, self.device),
                         torch.as_tensor(np.concatenate(pos), dtype=torch.int64, device=self.device)))
        if len(self._dev_plans) > 16:
            self._dev_plans.clear()
        self._dev_plans[key] = plan
        return plan

    def _draw_device(self, B, H, cts, off, reuse):
        """rng 'device' for B envs: the B streams white in one draw, every coloured third / reuse tail overwritten
        from one batched spectrum draw per sample length, the picks' uniforms: ~8 launches per call."""
        noise = self.planner.noise_flat
        noise[:B * off["total"]].normal_()
        for gen, pos in self._device_plan(H, cts, off, reuse, B):
            noise[pos] = gen.draw()
        self.planner.u[:B].uniform_()

    def _draw(self, e, H, cts, off, reuse, eval_mode):
        """Env e's stream in the reference's order (icem_draw_reference): numpy draws the pink and brown thirds and
        the reused elites' tail, torch the white third (and a white tail when noise_beta is 0)."""
        cfg, A, dev = self.cfg, self.cfg.action_dim, self.device
        specs = self._colored_specs(H, cts, reuse)

        def compose(buf, i, n, ne, cols):
            n0, n1, _ = _thirds(n)
            samp = buf[off["samp"][i]:off["samp"][i] + H * n * A].view(H, n, A)
            samp[:, :n0].copy_(torch.randn(H, n0, A, device=dev))
            samp[:, n0:n0 + n1].copy_(next(cols))
            samp[:, n0 + n1:].copy_(next(cols))
            if i == 0 and reuse:
                r = buf[off["reuse"]:off["reuse"] + H * ne * A].view(H, ne, A)
                r.copy_(next(cols) if cfg.noise_beta > 0 else torch.randn(H, ne, A, device=dev))

        return icem_draw_reference(self.planner, e, H, cts, off, eval_mode,
                                   lambda: ([sp[1] for sp in specs], self._colored_host(specs, H)), compose, True)

    def _load(self, e, H, cts, off, reuse, nz):
        S = off["total"]
        return icem_load(self.planner.noise_flat[e * S:(e + 1) * S], self.cfg.action_dim, H, cts, off, reuse, nz)

    @torch.no_grad()
    def plan(self, obs, eval_mode=False, step=None, t0=True, noise=None, trace=None):
        """tdmpc_icem_similarity_mlp.py:160-265 -> (action tensor [A], metrics dict)."""
        if self._seed_step(step, eval_mode):
            return self._seed_return()
        obs = torch.as_tensor(np.asarray(obs), dtype=torch.float32).view(1, -1)
        a, _ = self._plan_envs(obs, eval_mode, step, t0, [noise] if noise is not None else None, trace)
        return a[0].clone(), self._metrics(1)[0]

    @torch.no_grad()
    def plan_batch(self, obs, eval_mode=False, step=None, t0=True, sync_metrics=True):
        """B independent iCEM plans in one call (vectorised envs, all at the same step / t0): obs [B, obs_dim] ->
        (actions [B, A], metrics). Env e's result equals a single-env plan() on its own noise stream
        (tests/test_icem.py::test_gpu_icem_batched_equals_single). Seed steps are not batched. sync_metrics=False
        returns the metrics tensor [B, 2] without a host sync: a device failure then shows at check_status() only."""
        if self._seed_step(step, eval_mode):
            raise ValueError("plan_batch: seed steps draw uniform actions; call plan() per env")
        obs = torch.as_tensor(obs, dtype=torch.float32)
        a, m = self._plan_envs(obs.view(obs.shape[0], -1), eval_mode, step, t0, None, None)
        return a, (self._metrics(obs.shape[0]) if sync_metrics else m)

    def check_status(self):
        """Synchronising check of the sticky device status word (for plan_batch(sync_metrics=False) callers)."""
        self.planner.check_status()

    def _plan_envs(self, obs, eval_mode, step, t0, noise, trace):
        cfg, pl = self.cfg, self.planner
        B = obs.shape[0]
        self._check_call(B)
        if t0:   # :172-175: the schedule moves the plan horizon only at an episode start
            self.plan_horizon = self.horizon(step)
        H = self.plan_horizon
        self.mixture_coef = linear_schedule(cfg.regularization_schedule, step)
        cts = self.counts(self.mixture_coef, self._has_elites)
        if cts[0][1] <= 0 or any(p <= 0 for _, p, _ in cts):
            raise AssertionError("num_pi_trajs > 0")   # the reference asserts this (:187, :205)
        if cts[0][1] > self.P_max:
            raise ValueError("mixture_coef above the schedule's maximum")
        if cfg.iterations > 1 and cts[1][2] > 0 and not cfg.keep_previous_elites:
            # the reference would then re-use the first iteration's `reused_actions` (a stale loop variable)
            raise NotImplementedError("fraction_elites_reused > 0 needs keep_previous_elites")
        reuse = self._has_elites and cfg.shift_elites_over_time and cts[0][2] > 0
        if reuse and self._elite_H not in (H, H - 1):
            raise RuntimeError("elite horizon mismatch")   # the reference's torch.cat would fail here
        off = self._layout(H, cts, reuse)
        pl.pack(self.model)
        pl.obs_buf[:B].copy_(obs.to(self.device))
        if noise is not None:
            for e, nz in enumerate(noise):
                pl.u[e:e + 1].fill_(self._load(e, H, cts, off, reuse, nz))
        elif self.rng == "device":
            self._draw_device(B, H, cts, off, reuse)
        else:
            us = [self._draw(e, H, cts, off, reuse, eval_mode) for e in range(B)]
            pl.u[:B].copy_(torch.tensor(us, dtype=torch.float64))
        p = icem_params(cfg, B, H, cts, off, reuse, (not t0) and self._has_prev, eval_mode, self.std, pl.status,
                        pl.path, self._elite_H if reuse else H)
        dev = self.device
        value_out = mean_out = std_out = None
        if trace is not None:
            Tw = cfg.num_samples + cfg.num_elites + self.P_max
            value_out = torch.zeros(B, cfg.iterations, Tw, device=dev)
            mean_out = torch.zeros(B, cfg.iterations, H, cfg.action_dim, device=dev)
            std_out = torch.zeros_like(mean_out)
        _lib.call("tdmpc_plan_icem", pl.dims, p, pl.packed, pl.obs_buf, 0, pl.noise_flat, pl.u, pl.prev_mean_flat,
                  pl.elites, pl.action, pl.metrics, value_out, mean_out, std_out, *pl._ws(), pl._stream())
        if trace is not None:
            trace.update(value=[v[0] for v in icem_trace_values(value_out, cts)],
                         mean=mean_out[0], std=std_out[0], counts=cts,
                         value_all=value_out, mean_all=mean_out, std_all=std_out)   # (every env: [B, I, ...])
        self._has_prev = True
        self._has_elites = True
        self._elite_H = H
        return pl.action[:B], pl.metrics[:B]
