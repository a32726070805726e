"""The yardstick of the DSSM update (tdmpc_amd/drnn_learner.py): the reference's `TdICemSimDssm.update`,
`intrinsic_rewards` and `update_pi` (src/algorithm/tdmpc_icem_similarity_drnn.py:367-384, :421-553) restated in plain
PyTorch over the project's eager `tdmpc_amd.dssm.DSSM` module tree, operation by operation in the reference's order,
generic in the dtype.

In float32 on the CPU it equals the recorded reference run (tests/golden/drnn_update/*.npz, written by
tests/golden/make_drnn_update_golden.py) bit for bit: tests/test_drnn_update_cpu.py. In float64 it is what
tests/test_gpu_drnn_update.py compares the GPU with, and float32 against float64 is the noise floor those bounds are
derived from.

Restated beside the update: gym's `RunningMeanStd.update_from_moments` with batch_count 1 (the package is not a
dependency), and the NumPy arithmetic of :435-441 as the NumPy that recorded the golden performs it on a float32 array
against the float64 running moments -- the division computed in float64 and stored back as float32, the threshold
subtracted in float64 -- with the result returned in the model's precision (the recording wraps `intrinsic_rewards` in
`.float()` for the same reason: the reference's pinned stack keeps float32 there).

Cases, the fixed batch, the steps and the summaries of the recorded tensors live here so that the maker and the tests
share them.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from drnn_io import drnn_cfg
from tdmpc_amd.config import linear_schedule
from tdmpc_amd.dssm import DSSM, synthetic_dssm_state_dict

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drnn_update")
METRICS = ("consistency_loss", "reward_loss", "value_loss", "pi_loss", "total_loss", "weighted_loss", "grad_norm",
           "intrinsic_batch_reward_mean", "current_explore_coef")
STEPS = (20000, 20001)   # the first with the EMA (update_freq 2), the second without; explore_coef > 0 at both
TIE = 1e-4               # update_pi: |Q1 - Q2| > TIE (1 + |Q|) on every row (torch.min's gradient takes one side)

# name -> (task, latent_dim, hidden_dim, horizon, batch_size, model seed, target seed, batch seed, torch seed)
#   cheetah: L50 A6 Hd128, H = 3, B = 33 (a short single BatchNorm chunk per segment)
#   tiny:    (L, Hd, A) = (8, 32, 1), H = 2, B = 2: the two-row BatchNorm
#   wide:    cheetah with B = 130 (two chunks per segment, every later segment off the 128-row grid); not recorded
CASES = {
    "cheetah": ("cheetah", 50, 128, 3, 33, 31, 32, 41, 0),
    "tiny": ("cartpole", 8, 32, 2, 2, 33, 34, 42, 0),
    "wide": ("cheetah", 50, 128, 3, 130, 35, 36, 43, 0),
}
RECORDED = ("cheetah", "tiny")


def case_cfg(name):
    task, L, Hd, H, B = CASES[name][:5]
    return drnn_cfg(task, latent_dim=L, hidden_dim=Hd, horizon=H, batch_size=B, optim_id="adam",
                    train_steps=100000, episode_length=500)


def batch(cfg, seed):
    """(obs [B, obs], next_obses [H+1, B, obs], action [H+1, B, A], reward [H+1, B, 1], idxs [B], weights [B])"""
    rs = np.random.RandomState(seed)
    B, H, O, A = cfg.batch_size, cfg.horizon, cfg.obs_shape[0], cfg.action_dim
    f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))  # noqa: E731
    obs = f(B, O)
    next_obses = f(H + 1, B, O)
    action = torch.from_numpy(rs.uniform(-1, 1, (H + 1, B, A)).astype(np.float32))
    reward = f(H + 1, B, 1)
    idxs = torch.arange(B, dtype=torch.int64)
    weights = torch.from_numpy(rs.uniform(0.5, 1.0, B).astype(np.float32))
    return obs, next_obses, action, reward, idxs, weights


def case_batch(name):
    return batch(case_cfg(name), CASES[name][7])


def draws(cfg, seed):
    """2H + 1 [B, A] standard normal draws of one update (cases without a recording)."""
    rs = np.random.RandomState(seed)
    return [torch.from_numpy(rs.standard_normal((cfg.batch_size, cfg.action_dim)).astype(np.float32))
            for _ in range(2 * cfg.horizon + 1)]


class FakeBuffer:
    """Hands `update` a fixed batch and keeps the priorities it is given."""
    graph_safe = True
    idx, _full = 0, False

    def __init__(self, b):
        self.b = b
        self.prios = []

    def sample(self):
        return self.b

    def update_priorities(self, idxs, p):
        self.prios.append(p.detach().clone())


def probe(n_elems, k=64, seed=0):
    return np.random.RandomState(seed).randint(0, n_elems, size=k)


def summarize(tensors):
    """Per tensor (a dict's values in order; None counts as zeros of one element): float64 sum, sum of squares and 64
    fixed elements -- the full tensors of a DSSM are megabytes."""
    s, ss, pr = [], [], []
    for i, v in enumerate(tensors.values()):
        v = torch.zeros(1) if v is None else v
        v = v.detach().double().reshape(-1).cpu()
        s.append(float(v.sum()))
        ss.append(float((v ** 2).sum()))
        pr.append(v[torch.from_numpy(probe(v.numel(), seed=i))].numpy())
    return np.array(s), np.array(ss), np.stack(pr)


def make_models(cfg, name, dtype=torch.float32, device="cpu"):
    wseed, tseed = CASES[name][5:7]
    out = []
    for seed in (wseed, tseed):
        m = DSSM(cfg, init="none")
        m.load_state_dict(synthetic_dssm_state_dict(cfg, seed))
        out.append(m.to(device=device, dtype=dtype).eval())
    return out


def rms_update_from_moments(rms, batch_mean, batch_var):
    """gym.wrappers.normalize.update_mean_var_count_from_moments with batch_count = 1, on float64 scalars."""
    mean, var, count = rms
    delta = batch_mean - mean
    tot = count + 1
    new_mean = mean + delta / tot
    m2 = var * count + batch_var + delta * delta * count / tot
    return [new_mean, m2 / tot, tot]


class RefAgent:
    """The reference agent's learning state: model, target, the two Adam optimisers, reward_rms."""

    def __init__(self, cfg, name, dtype=torch.float32):
        self.cfg, self.dtype = cfg, dtype
        self.model, self.model_target = make_models(cfg, name, dtype)
        self.optim = torch.optim.Adam(self.model.parameters(), lr=cfg.lr)
        self.pi_optim = torch.optim.Adam(self.model._pi.parameters(), lr=cfg.pi_lr)
        self.rms = [np.float64(0.0), np.float64(1.0), np.float64(1e-4)]   # RunningMeanStd(): mean, var, count
        self.pi_tie = np.inf

    def pi(self, z, eps):
        return self.model.pi(z, self.cfg.min_std, eps=eps)

    def update_pi(self, zs, eps):
        """:367-384."""
        self.pi_optim.zero_grad(set_to_none=True)
        self.model.track_q_grad(False)
        pi_loss = 0
        for t, z in enumerate(zs):
            a = self.pi(z, eps[t])
            q1, q2 = self.model.Q(z, a)
            Q = torch.min(q1, q2)
            with torch.no_grad():
                margin = ((q1 - q2).abs() / (1 + Q.abs())).min()
                self.pi_tie = min(self.pi_tie, float(margin))
            pi_loss += -Q.mean()
        pi_loss.backward()
        torch.nn.utils.clip_grad_norm_(self.model._pi.parameters(), self.cfg.grad_clip_norm, error_if_nonfinite=False)
        self.pi_optim.step()
        self.model.track_q_grad(True)
        return pi_loss.item()

    @torch.no_grad()
    def intrinsic_rewards(self, obs, next_obses, actions):
        """:421-443."""
        cfg, m = self.cfg, self.model
        zs_target = self.model_target.h(next_obses)
        z_traj = m.h(torch.cat([obs.unsqueeze(0), next_obses], dim=0))
        unc = torch.zeros((cfg.horizon + 1, cfg.horizon + 1, cfg.batch_size, 1), dtype=self.dtype)
        for t in range(0, z_traj.shape[0] - 1):
            hidden = m.init_hidden_state(z_traj[t].shape[0], obs.device).to(self.dtype)
            z, hidden, _ = m.next(z_traj[t], actions[t], hidden)
            zs_pred = m.pred_z(z)
            zs_pred = F.normalize(zs_pred.unsqueeze(0), dim=-1, p=2)
            target = F.normalize(zs_target[t:t + 1], dim=-1, p=2)
            unc[t][t:t + 1] = 2.0 - 2.0 * (zs_pred * target).sum(dim=-1, keepdim=True)
        raw = torch.sum(unc, dim=0).numpy()
        self.raw_uncertainty = raw.copy()
        bm, bs = np.mean(raw), np.std(raw)
        self.rms = rms_update_from_moments(self.rms, np.float64(bm), np.float64(bs ** 2))
        sd = np.sqrt(self.rms[1])
        x = (raw.astype(np.float64) / sd).astype(raw.dtype)
        x = np.maximum(x.astype(np.float64) - self.rms[0] / sd, 0)
        return torch.from_numpy(x).to(self.dtype)

    def update(self, b, step, noise):
        """:445-553 on the batch b -> dict(metrics [9] (METRICS), prio, intrinsic, rms, grads, tie). noise: the 2H + 1
        TruncatedNormal draws in the reference's order (H value targets, H + 1 update_pi)."""
        cfg, m, mt, dt = self.cfg, self.model, self.model_target, self.dtype
        H = cfg.horizon
        obs, next_obses, action, reward = (t.to(dt) for t in b[:4])
        weights = b[5].to(dt)
        noise = [n.to(dt) for n in noise]
        m.train()
        self.optim.zero_grad(set_to_none=True)
        z = m.h(obs)
        next_zs = mt.h(next_obses)
        online_next_zs = m.h(next_obses)
        zs = [z.detach()]
        explore_coef = linear_schedule(cfg.explore_schedule, step)
        intrinsic = self.intrinsic_rewards(obs, next_obses, action)
        reward_pi = explore_coef * intrinsic + reward

        similarity_loss, reward_loss, value_loss, priority_loss = 0, 0, 0, 0
        hidden = m.init_hidden_state(z.shape[0], z.device).to(dt)
        zs_query, zs_key = [], []
        next_q_values, outputs = [], []
        rewards = reward_pi[:H]
        discounts = torch.ones_like(rewards) * cfg.discount
        for t, next_z in enumerate(online_next_zs[:H]):
            with torch.no_grad():
                next_q_value = torch.min(*mt.Q(next_z, self.pi(next_z, noise[t])))
            next_q_values.append(next_q_value)
        next_q_values = torch.stack(next_q_values, dim=0)
        last = next_q_values[-1]
        inputs = rewards + discounts * next_q_values * (1 - cfg.td_lambda)
        for index in reversed(range(next_q_values.shape[0])):
            last = inputs[index] + discounts[index] * last * cfg.td_lambda
            outputs.append(last)
        td_lambda_targets = torch.stack(list(reversed(outputs)), dim=0)

        for t in range(H):
            Q1, Q2 = m.Q(z, action[t])
            z, hidden, reward_pred = m.next(z, action[t], hidden)
            td_target = td_lambda_targets[t]
            reward_loss += F.mse_loss(reward_pred, reward[t], reduction="none")
            value_loss += (F.mse_loss(Q1, td_target, reduction="none") + F.mse_loss(Q2, td_target, reduction="none"))
            priority_loss += (F.l1_loss(Q1, td_target, reduction="none") + F.l1_loss(Q2, td_target, reduction="none"))
            zs_query.append(z)
            zs_key.append(next_zs[t].detach())
            zs.append(z.detach())
        queries = m.pred_z(torch.cat(zs_query, dim=0))
        keys = torch.cat(zs_key, dim=0)
        sim = 2.0 - 2.0 * (F.normalize(queries, dim=-1, p=2) * F.normalize(keys, dim=-1, p=2)).sum(dim=-1)
        similarity_loss += sim.reshape(H, cfg.batch_size, -1).sum(dim=0)

        model_loss = cfg.similarity_coef * similarity_loss.clamp(max=1e4) + \
            cfg.reward_coef * reward_loss.clamp(max=1e4)
        td_loss = cfg.value_coef * value_loss.clamp(max=1e4)
        total_loss = model_loss + td_loss
        weighted_loss = (model_loss * weights).mean() + td_loss.mean()
        weighted_loss.register_hook(lambda grad: grad * (1 / H))
        weighted_loss.backward()
        grad_norm = torch.nn.utils.clip_grad_norm_(m.parameters(), cfg.grad_clip_norm, error_if_nonfinite=False)
        self.optim.step()
        prio = priority_loss.clamp(max=1e4).detach()

        pi_loss = self.update_pi(zs, noise[H:])
        if step % cfg.update_freq == 0:
            with torch.no_grad():
                for p, p_target in zip(m.parameters(), mt.parameters()):
                    p_target.data.lerp_(p.data, cfg.tau)
        m.eval()
        metrics = np.array([float(similarity_loss.mean().item()), float(reward_loss.mean().item()),
                            float(value_loss.mean().item()), pi_loss, float(total_loss.mean().item()),
                            float(weighted_loss.mean().item()), float(grad_norm), intrinsic.mean().item(),
                            explore_coef], dtype=np.float64)
        return dict(metrics=metrics, prio=prio.numpy().copy(), intrinsic=intrinsic.numpy().copy(),
                    rms=np.array([float(v) for v in self.rms]), grads=grads_of(m), tie=self.pi_tie)


def grads_of(model):
    return {k: None if p.grad is None else p.grad.detach().clone() for k, p in model.named_parameters()}


def record(out, k, r, model, model_target):
    """One update's results as the recording's arrays u{k}_*."""
    out[f"u{k}_metrics"], out[f"u{k}_prio"], out[f"u{k}_intrinsic"], out[f"u{k}_rms"] = \
        r["metrics"], r["prio"], r["intrinsic"], r["rms"]
    for tag, tensors in (("grad", r["grads"]), ("model", model.state_dict()), ("target", model_target.state_dict())):
        out[f"u{k}_{tag}_sum"], out[f"u{k}_{tag}_sumsq"], out[f"u{k}_{tag}_probe"] = summarize(tensors)


def run_case(name, dtype=torch.float32, noise=None):
    """The case's two consecutive updates -> (agent, [result per update], the recording's arrays). noise: per update
    the 2H + 1 draws (default: `draws` from the case's torch seed + update index)."""
    cfg = case_cfg(name)
    agent = RefAgent(cfg, name, dtype)
    b = batch(cfg, CASES[name][7])
    out, res = {}, []
    for k, step in enumerate(STEPS):
        nz = noise[k] if noise is not None else draws(cfg, 1000 + 10 * CASES[name][8] + k)
        r = agent.update(b, step, nz)
        record(out, k, r, agent.model, agent.model_target)
        res.append(r)
    return agent, res, out


def load(name):
    return np.load(os.path.join(GOLD_DIR, f"{name}.npz"))


def gold_noise(g, cfg):
    return [[torch.from_numpy(g[f"u{k}_noise"][i]) for i in range(2 * cfg.horizon + 1)] for k in range(len(STEPS))]


# ---------------------------------------------------------------------------------------------------------------------
# Comparing two runs of an update (tests/test_gpu_drnn_update.py; the float32 CPU run against float64 is the noise floor)
# ---------------------------------------------------------------------------------------------------------------------
ZERO_MEAN = {"_dynamics.prior_mlp.0.bias": "_dynamics.prior_mlp.0", "_predictor.0.bias": "_predictor.0"}
CLASSES = ("metrics", "prio", "intrinsic", "rms", "grad", "grad0", "stats", "param", "param_q", "param0", "target")


class PreBNScales:
    """As drnn_train_ref.PreBN for a whole update: the float64 gradients at the outputs of the two Linears that feed
    train-mode BatchNorms (calls under no_grad have none). Their biases' gradients are exactly zero in exact
    arithmetic; the scale of such a tensor is the largest column sum of |dL/d(pre-BatchNorm)|, the sum that cancels."""

    def __init__(self, model):
        self.outs = {k: [] for k in ZERO_MEAN}
        mods = dict(model.named_modules())
        self.hooks = [mods[m].register_forward_hook(self._hook(k)) for k, m in ZERO_MEAN.items()]

    def _hook(self, key):
        def keep(_module, _inputs, out):
            if out.requires_grad:
                out.retain_grad()
                self.outs[key].append(out)
        return keep

    def take(self):
        """The scales of the update that just ran (then forget its outputs)."""
        out = {}
        for k, os_ in self.outs.items():
            gs = [o.grad.abs().sum(0) for o in os_ if o.grad is not None]
            out[k] = float(torch.stack(gs).sum(0).max()) if gs else 0.0
            os_.clear()
        return out

    def close(self):
        for hk in self.hooks:
            hk.remove()


def _np64(t):
    return t.detach().double().cpu().numpy().copy()   # (a float64 CPU tensor would share its memory otherwise)


def snapshot(r, model, model_target):
    """One update's results by class, float64 numpy: r = dict(metrics [>= 8], prio, intrinsic, rms, grads)."""
    sd = model.state_dict()
    named = dict(model.named_parameters())
    zero = lambda k: np.zeros(tuple(named[k].shape))  # noqa: E731
    grads = {k: zero(k) if g is None else _np64(g) for k, g in r["grads"].items()}
    metrics = dict(zip(METRICS[:8], np.asarray(r["metrics"], np.float64)[:8]))
    # grad_norm is a backward quantity, the norm of the gradients: it is compared as one of them (DESIGN.md §7 f7 holds
    # forward values and gradients to separate bounds, and so does this)
    grads["grad_norm"] = np.float64(metrics.pop("grad_norm"))
    params = {k: _np64(v) for k, v in named.items()}
    return {
        "metrics": {n: np.float64(v) for n, v in metrics.items()},
        "prio": {"prio": np.asarray(r["prio"], np.float64)},
        "intrinsic": {"intrinsic": np.asarray(r["intrinsic"], np.float64).reshape(-1)},
        "rms": {n: np.float64(v) for n, v in zip(("mean", "var", "count"), r["rms"])},
        "grad": {k: v for k, v in grads.items() if k not in ZERO_MEAN},
        "grad0": {k: v for k, v in grads.items() if k in ZERO_MEAN},
        "stats": {k: _np64(v) for k, v in sd.items() if k.endswith(("running_mean", "running_var"))},
        "param": {k: v for k, v in params.items() if k not in ZERO_MEAN},
        "param0": {k: v for k, v in params.items() if k in ZERO_MEAN},
        "target": {k: _np64(v) for k, v in model_target.named_parameters()},
    }


def figure(got, want, scale=None):
    """max |got - want| / max |want| (or / scale); a reference that is exactly zero asks for exact zeros."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    den = float(np.abs(want).max()) if scale is None else scale
    if den == 0.0:
        return 0.0 if not got.any() else float("inf")
    return float(np.abs(got - want).max()) / den


def figures(got, want, scales, lr, tau):
    """{class: (largest figure, its tensor)} of two snapshots; scales: PreBNScales.take() of the float64 run (grad0).

    Parameters after an Adam step are measured in units of the step size lr, not of the tensor: Adam's first step is
    -lr g / (|g| + 1e-8), about -lr sign(g), so an element whose gradient is within rounding of zero moves by up to lr
    in EITHER direction whatever the precision, and two correct runs differ there by up to 2 lr. `param` is the largest
    |difference| / lr of a tensor (such elements included), `param_q` its 99th percentile (the typical element; a
    missing or mis-scaled step shows here), `param0` the two zero-mean biases (ZERO_MEAN), whose every element is
    such an element. `target` (one EMA of the parameters, at the first update) likewise in units of tau lr."""
    out = {}
    for cls in CLASSES:
        worst = (0.0, "")
        src = "param" if cls == "param_q" else cls
        for k, w in want[src].items():
            if cls in ("param", "param_q", "param0", "target"):
                d = np.abs(np.asarray(got[src][k], np.float64) - w) / (lr * tau if cls == "target" else lr)
                f = float(d.max() if cls != "param_q" else np.quantile(d, 0.99))
            else:
                f = figure(got[cls][k], w, scales.get(k) if cls == "grad0" else None)
            if not f <= worst[0]:
                worst = (f, k)
        out[cls] = worst
    return out


def run_ref(name, dtype, noise=None, scales=False):
    """The case's two updates on the yardstick -> [snapshot per update] (and, float64 only, [scales per update])."""
    cfg = case_cfg(name)
    agent = RefAgent(cfg, name, dtype)
    pre = PreBNScales(agent.model) if scales else None
    b = batch(cfg, CASES[name][7])
    snaps, scs = [], []
    for k, step in enumerate(STEPS):
        nz = noise[k] if noise is not None else draws(cfg, 1000 + 10 * CASES[name][8] + k)
        r = agent.update(b, step, nz)
        snaps.append(snapshot(r, agent.model, agent.model_target))
        if pre:
            scs.append(pre.take())
    if pre:
        pre.close()
    return (snaps, scs) if scales else snaps


def bound(floors, cls, k):
    """The bound of class cls after update k (0, 1): 8 x the float32 CPU floor, never below 1e-6 -- but for the classes
    that Adam's step makes discontinuous, whose floor says whether an element with a gradient within rounding of zero
    exists and not how precise the run is, what Adam guarantees. A bias-corrected Adam step is at most lr at step 1
    and, by Cauchy-Schwarz on (0.09 g1 + 0.1 g2) / 0.19 against sqrt((0.000999 g1^2 + 0.001 g2^2) / 0.001999), at most
    1.0014 lr at step 2, so two correct runs differ by at most 2.01 lr per step taken (the target by tau times that of
    the one step before its EMA)."""
    if cls in ("param", "param0"):
        return 2.01 * (k + 1)
    if cls == "target":
        return 2.01
    return max(8 * floors[cls], 1e-6)


def case_noise(name):
    """The draws of the case's two updates: the recording's where there is one."""
    cfg = case_cfg(name)
    if name in RECORDED:
        return gold_noise(load(name), cfg)
    return [draws(cfg, 1000 + 10 * CASES[name][8] + k) for k in range(len(STEPS))]
