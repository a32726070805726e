"""GPU: the MPC DSSM agent's update (tdmpc_amd/drnn_learner.py::DssmSimLearner, the entry points of
include/tdmpc_drnn_learner.h's last section) against float64 (tests/drnn_sim_update_ref.py, which
tests/test_drnn_sim_update_cpu.py pins to the reference bit for bit).

  1  tdmpc_drnn_intrinsic_chain_fwd mode 0 with S = 4 == four tdmpc_drnn_next_fwd calls with the hidden state handed on
     + tdmpc_drnn_simloss_fwd on the segments >= warm, bitwise: losses, h_out, both BatchNorms' running statistics;
     shapes (L, Hd, A) = (8, 32, 1) and (50, 128, 6); B = 33 and 130; warm = 0, 1, 3.
  2  mode 1 (the recurrence in one launch) against the float64 CPU modules: every segment's hidden state and the
     losses; shapes (8, 32, 1), (50, 128, 6), (129, 224, 21), (256, 256, 38); B = 2, 33, 130; S = 4, warm 1. Bound by
     DESIGN.md §7 f7's recipe: 8 x the figure (max |got - f64| / max |f64|) the float32 CPU modules show against
     float64 at the same case, never below 1e-6. Two runs bitwise equal; mode 0 is held to the same bound.
  3  tdmpc_drnn_sim_loss_forward / _backward against float64 autograd of the reference's expressions at (H, W) =
     (3, 1), (3, 2), (5, 2); rows past the 1e4 clamps.
  4  two consecutive whole updates of tiny, cheetah and wide against the float64 yardstick.
  5  graph replay against eager from the same state; two eager runs bitwise.
  6  TdMpcDrnn.update, then plan() on repacked weights.

Bounds of 4 and 5 as tests/test_gpu_drnn_update.py: per class of results the figure (drnn_update_ref.figures) that the
float32 CPU run of the same yardstick shows against float64 is the noise floor (FLOORS below;
tests/test_drnn_sim_update_cpu.py::test_fp32_floors_the_gpu_bounds_are_derived_from recomputes them and holds the
float32 run to the bounds), the bound is 8 x that floor, never below 1e-6 (drnn_update_ref.bound), per update and with
B = 2 on its own; `param`, `param0` and `target` are bounded by what Adam guarantees.

Floors (float32 CPU against float64): the largest figure over the cases of a group (rest: cheetah, wide; B = 2:
tiny) and over float32 runs with 1, 2, 4 and 8 CPU threads (THREADS). The thread count moves the summation order of
the CPU's products, and with it which near-zero gradient elements Adam's first step sends the other way; what the
second update computes from those parameters moves by far more than one rounding: wide's pi_loss at update 1 shows
7.8e-06 (5 threads), 9.4e-06 (8), 4.5e-05 (2), 5.9e-05 (3) and 1.2e-04 (1) against float64. One thread count is one
draw of that noise, not its size; a first version of this file took the 8-thread draw alone, and the MI355X's 8.3e-05
lay above 8 x it and inside the CPU's own spread.
                  metrics   prio      intrinsic rms       grad      grad0     stats     param_q
  rest, update 0  5.40e-07  4.20e-07  8.51e-07  1.57e-07  2.64e-06  1.21e-07  3.88e-07  5.95e-05
  rest, update 1  1.19e-04  6.59e-06  6.23e-06  1.36e-07  3.45e-04  1.20e-07  5.62e-04  1.43e-03
  B = 2, update 0 2.17e-04  1.47e-08  1.08e-05  2.75e-06  1.39e-04  2.65e-07  1.44e-06  2.50e-03
  B = 2, update 1 3.82e-04  8.96e-06  1.22e-04  1.44e-05  1.69e-03  1.11e-06  8.38e-04  4.05e-03
  (param / param0 / target, in lr or tau lr: 0.13 / 0.48 / 0.30 on the rest, 0.24 / 1.82 / 1.00 at B = 2)
With one shoot step (tiny, wide) `_dynamics.prior_mlp.3.bias` is a zero-mean tensor and is compared as one
(drnn_sim_update_ref.zero_mean). GPU figures measured on an MI355X: DESIGN.md §7 f9.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import drnn_sim_update_ref as U
import drnn_train_ref as R
from update_gpu import gpu_learner, hold, same, snap, yardstick

pytestmark = pytest.mark.gpu

THREADS = (1, 2, 4, 8)
FLOORS = {
    ("rest", 0): dict(metrics=5.402e-07, prio=4.200e-07, intrinsic=8.506e-07, rms=1.567e-07, grad=2.642e-06,
                      grad0=1.209e-07, stats=3.884e-07, param_q=5.952e-05),
    ("rest", 1): dict(metrics=1.186e-04, prio=6.588e-06, intrinsic=6.232e-06, rms=1.360e-07, grad=3.453e-04,
                      grad0=1.199e-07, stats=5.623e-04, param_q=1.430e-03),
    ("b2", 0): dict(metrics=2.165e-04, prio=1.472e-08, intrinsic=1.077e-05, rms=2.753e-06, grad=1.385e-04,
                    grad0=2.654e-07, stats=1.442e-06, param_q=2.501e-03),
    ("b2", 1): dict(metrics=3.823e-04, prio=8.956e-06, intrinsic=1.220e-04, rms=1.444e-05, grad=1.692e-03,
                    grad0=1.110e-06, stats=8.381e-04, param_q=4.051e-03),
}


def group(name):
    return "b2" if U.CASES[name][5] == 2 else "rest"


# ---------------------------------------------------------------------------------------------------------------- 1, 2
SHAPES = {(8, 32, 1): "cartpole", (50, 128, 6): "cheetah", (129, 224, 21): "humanoid", (256, 256, 38): "dog"}
S = 4


def _train_step(shape, rows, **kw):
    from tdmpc_amd.dssm_train import DssmTrainStep
    L, Hd, A = shape
    cfg = R.cfg_for(SHAPES[shape], L, Hd)
    assert cfg.action_dim == A
    model = R.make_model(cfg, torch.float32, device="cuda")
    return cfg, model, DssmTrainStep(model, max_rows=rows, max_steps=1, max_loss_rows=rows, max_losses=1, **kw)


def _stats(model):
    return {k: v.clone() for k, v in model.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


@pytest.mark.parametrize("warm", [0, 1, 3])
@pytest.mark.parametrize("B", [33, 130])
@pytest.mark.parametrize("shape", [(8, 32, 1), (50, 128, 6)], ids=lambda s: "-".join(map(str, s)))
def test_launch_chain_equals_separate_calls_bitwise(shape, B, warm):
    cfg, chain_model, chain_step = _train_step(shape, B)
    _, sep_model, sep_step = _train_step(shape, B)
    z, a, keys = (t.cuda() for t in U.chain_inputs(cfg, S, B, 100 + B))
    loss, h_out, hs = chain_step.intrinsic_chain_loss(z, a, keys, S, warm, mode=0, hidden=True)
    want, hid = [], torch.zeros(B, cfg.hidden_dim, device="cuda")
    with torch.no_grad():
        for s in range(S):
            rows = slice(s * B, (s + 1) * B)
            zo, hid, _ = sep_step.next(z[rows], a[rows], hid)
            assert torch.equal(hs[s], hid), s
            want.append(sep_step.similarity_loss(zo, keys[rows]) if s >= warm else torch.zeros(B, device="cuda"))
    want = torch.cat(want)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and float(loss[warm * B:].abs().min()) > 0 and not loss[:warm * B].any()
    assert torch.equal(loss, want), float((loss - want).abs().max())
    assert torch.equal(h_out, hid)
    sa, sb = _stats(chain_model), _stats(sep_model)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert int(sa["_dynamics.prior_mlp.1.num_batches_tracked"]) == 1000 + S
    assert int(sa["_predictor.1.num_batches_tracked"]) == 1000 + S - warm
    assert not torch.equal(sa["_predictor.1.running_mean"],
                           U.synthetic_dssm_state_dict(cfg, R.WSEED)["_predictor.1.running_mean"].cuda())


_CHAIN = {}


def _chain_ref(shape, B, warm):
    """Per case, once: the inputs, the float64 CPU modules' result and the float32 CPU modules' figures against it."""
    key = (shape, B, warm)
    if key not in _CHAIN:
        L, Hd, _ = shape
        cfg = R.cfg_for(SHAPES[shape], L, Hd)
        d = U.chain_inputs(cfg, S, B, 200 + B)
        want = U.chain_ref(R.make_model(cfg, torch.float64), *d, S, warm)
        cpu = U.chain_ref(R.make_model(cfg, torch.float32), *d, S, warm)
        _CHAIN[key] = (d, want, tuple(R.figure(c, w) for c, w in zip(cpu, want)))
    return _CHAIN[key]


@pytest.mark.parametrize("B", [2, 33, 130])
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "-".join(map(str, s)))
def test_one_launch_recurrence_matches_float64(shape, B):
    warm = 1
    d, (want_h, want_l), floors = _chain_ref(shape, B, warm)
    z, a, keys = (t.cuda() for t in d)
    runs = {}
    for tag, mode in (("mode 1", 1), ("mode 1 again", 1), ("mode 0", 0)):
        _, model, step = _train_step(shape, B)
        loss, h_out, hs = step.intrinsic_chain_loss(z, a, keys, S, warm, mode=mode, hidden=True)
        torch.cuda.synchronize()
        runs[tag] = (hs.clone(), loss, h_out, _stats(model))
        assert torch.equal(h_out, hs[S - 1]) and not loss[:warm * B].any()
    for x, y in zip(runs["mode 1"][:3], runs["mode 1 again"][:3]):
        assert torch.equal(x, y)
    for k, v in runs["mode 1"][3].items():
        assert torch.equal(v, runs["mode 1 again"][3][k]), k
    for tag in ("mode 1", "mode 0"):
        hs, loss = runs[tag][:2]
        for what, got, want, floor in (("hidden", hs, want_h, floors[0]), ("loss", loss, want_l, floors[1])):
            f, bound = R.figure(got.double().cpu().numpy(), want), max(8 * floor, 1e-6)
            print(f"chain {shape} B {B} {tag} {what}: gpu {f:.3e}, fp32cpu {floor:.3e} (bound {bound:.2e})")
            assert f <= bound, (tag, what, f, bound)


# ---------------------------------------------------------------------------------------------------------------- 3
def _loss_ref(sim, q1, q2, rp, rw, rwpi, nq, w, coefs, W):
    """The reference's expressions (tdmpc_similarity_drnn.py:423, :447-471); sim [H, B, 1], the rest [H - W, B, 1]."""
    sc, rc, vc, disc = coefs
    N = q1.shape[0]
    reward_loss, value_loss, priority_loss = 0, 0, 0
    tds = []
    for i in range(N):
        rho = 0.5 ** 0
        td = rwpi[i] + disc * nq[i]
        tds.append(td)
        reward_loss = reward_loss + (rp[i] - rw[i]) ** 2 * rho
        value_loss = value_loss + ((q1[i] - td) ** 2 + (q2[i] - td) ** 2) * rho
        priority_loss = priority_loss + ((q1[i] - td).abs() + (q2[i] - td).abs()) * rho
    similarity_loss = sim[:W].sum(dim=0) + sim[W:].sum(dim=0)
    total = sc * similarity_loss.clamp(max=1e4) + rc * reward_loss.clamp(max=1e4) + vc * value_loss.clamp(max=1e4)
    weighted = (total * w).mean()   # [B, 1] * [B]: the [B, B] broadcast
    return dict(td=torch.stack(tds), sim=similarity_loss, rew=reward_loss, val=value_loss,
                prio=priority_loss.clamp(max=1e4), total=total, weighted=weighted)


@pytest.mark.parametrize("H,W", [(3, 1), (3, 2), (5, 2)])
def test_fused_sim_loss_matches_float64_autograd(H, W):
    """B = 600 (three workgroups of the row kernel, two strides of the means kernel). A fifth of the rows carry
    similarity, reward or value sums past 1e4: their clamps are active and their gradients zero. fp32 sums of at most
    5 terms per row and 600 rows per mean: rtol 1e-5 (atol 1e-6 of the tensor's largest entry), as the iCEM loss's test."""
    from tdmpc_amd.dssm_train import _DssmSimFusedLoss
    B, N = 600, H - W
    rs = np.random.RandomState(10 * H + W)
    sim = np.abs(rs.standard_normal((H, B)))
    q1, q2, rp, rw, rwpi, nq = (rs.standard_normal((N, B)) for _ in range(6))
    sim[:, 0:40] *= 1e4        # similarity past the clamp
    rp[:, 40:80] *= 200        # reward loss past the clamp
    q1[:, 80:120] *= 200       # value loss (the priority's sum of absolute values stays below 1e4)
    q2[:, 120:140] *= 1e4      # priority past its clamp as well
    w = rs.uniform(0.5, 1.0, B)
    coefs = (1.0, 0.5, 0.1, 0.99)
    ops = (sim, q1, q2, rp, rw, rwpi, nq)
    t64 = [torch.from_numpy(x).unsqueeze(2).requires_grad_(i < 4) for i, x in enumerate(ops)]
    want = _loss_ref(*t64, torch.from_numpy(w), coefs, W)
    up = 0.7
    (want["weighted"] * up).backward()
    assert (want["sim"] > 1e4).any() and (want["rew"] > 1e4).any() and (want["val"] > 1e4).any()
    assert (want["prio"] == 1e4).any() and (want["sim"] < 1e4).any()
    t32 = [torch.from_numpy(x.astype(np.float32)).cuda().requires_grad_(i < 4) for i, x in enumerate(ops)]
    scal, rows, td = _DssmSimFusedLoss.apply(*t32, torch.from_numpy(w.astype(np.float32)).cuda(), coefs)
    (scal[4] * up).backward()
    torch.cuda.synchronize()
    assert tuple(td.shape) == (N, B) and tuple(rows.shape) == (5, B) and tuple(scal.shape) == (6,)

    same("td", td, want["td"])
    for i, k in enumerate(("sim", "rew", "val", "prio", "total")):
        same(k, rows[i], want[k])
    same("scal", scal, torch.stack([want["sim"].mean(), want["rew"].mean(), want["val"].mean(), want["total"].mean(),
                                    want["weighted"], torch.tensor(float(np.mean(w)))]))
    for i, k in enumerate(("dsim", "dq1", "dq2", "drp")):
        assert t32[i].grad.shape == t32[i].shape
        same(k, t32[i].grad, t64[i].grad)
        assert (t32[i].grad == 0).any() and (t32[i].grad != 0).any(), k


# ---------------------------------------------------------------------------------------------------------------- 4, 5
def _gpu_learner(name, **kw):
    from tdmpc_amd.drnn_learner import DssmSimLearner
    return gpu_learner(U, DssmSimLearner, name, **kw)


def _nbt(model):
    return [int(model._dynamics.prior_mlp[1].num_batches_tracked), int(model._predictor[1].num_batches_tracked)]


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("name", ["cheetah", "tiny", "wide"])
def test_two_consecutive_updates_match_float64(name, mode):
    want, scales = yardstick(U, name)
    cfg, agent, learner, buf = _gpu_learner(name)
    learner.train_step.chain_mode = mode
    noise = [([n.cuda() for n in eps], [n.cuda() for n in aug]) for eps, aug in U.case_noise(name)]
    H, W = cfg.horizon, cfg.warmup_len
    for k, step in enumerate(U.STEPS):
        m, coef = learner.update(buf, step, noise[k])
        assert not agent.model.training and coef > 0
        hold(U, f"{name} mode {mode} update {k}", snap(U, agent, learner, buf, m.tolist(), cfg), want[k], scales[k],
             cfg, FLOORS[(group(name), k)], k)
        assert _nbt(agent.model) == [1000 + (k + 1) * (2 * H + 1), 1000 + (k + 1) * (H + 3 - W)]
        assert not learner.last["intrinsic"][:W].any()
    assert len(learner.train_step._next_pool.free) == H and len(learner.train_step._loss_pool.free) == 2


def test_graph_replay_matches_eager_and_eager_is_reproducible():
    """cheetah with min_std = 0 and the augmentation scaled by 0 (no draw changes a value, so the eager and the captured
    update do the same arithmetic whatever the generator's state). Two graph-mode learners (the same optimiser
    arithmetic) run the first update eagerly from the same state: every class bitwise equal. Then A runs the second
    update eagerly -- explicit draws keep a call eager -- and B captures and replays it: again every class (metrics,
    priorities, intrinsic rewards, RunningMeanStd, gradients, running statistics, parameters, target) bitwise equal."""
    runs = []
    for replay in (False, True):
        cfg, agent, learner, buf = _gpu_learner("cheetah", graph=True, warmup=1, min_std=0.0)
        learner.AUG_SCALE = 0.0
        n = 2 * (cfg.horizon - cfg.warmup_len) + 1
        eager = ([torch.zeros(cfg.batch_size, cfg.action_dim, device="cuda") for _ in range(n)],
                 [torch.zeros(cfg.batch_size, cfg.latent_dim, device="cuda") for _ in range(cfg.horizon)])
        snaps = []
        for k, step in enumerate(U.STEPS):
            m, _ = learner.update(buf, step, eager if k and not replay else None)
            snaps.append(snap(U, agent, learner, buf, m.tolist(), cfg))
        runs.append((snaps, learner))
    (a, la), (b, lb) = runs
    assert lb._graphs and not la._graphs, "the second update was not captured"
    for cls in a[0]:
        for k in a[0][cls]:
            assert np.array_equal(a[0][cls][k], b[0][cls][k]), ("eager twice", cls, k)
    for cls in a[1]:
        for k in a[1][cls]:
            assert np.array_equal(a[1][cls][k], b[1][cls][k]), ("replay", cls, k)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_agent_update_returns_reference_metrics_and_plan_repacks():
    from tdmpc_amd.drnn import TdMpcDrnn
    from tdmpc_amd.drnn_learner import DssmSimLearner
    from tdmpc_amd.replay import ReplayBuffer
    cfg = U.case_cfg("cheetah")
    for k, v in dict(num_samples=32, num_elites=8, iterations=2, train_steps=500, episode_length=50,
                     max_buffer_size=10**6, env_horizon=cfg.horizon).items():
        setattr(cfg, k, v)
    rs = np.random.RandomState(5)
    agent = TdMpcDrnn(cfg, graph=True)
    agent.model.load_state_dict(U.synthetic_dssm_state_dict(cfg, 51))
    agent.model_target.load_state_dict(U.synthetic_dssm_state_dict(cfg, 52))
    buf = ReplayBuffer(cfg, latent_plan=True)
    O, A = cfg.obs_shape[0], cfg.action_dim
    for _ in range(3):
        buf.add(SimpleNamespace(obs=torch.from_numpy(rs.standard_normal((51, O)).astype(np.float32)),
                                action=torch.from_numpy(rs.uniform(-1, 1, (50, A)).astype(np.float32)),
                                reward=torch.from_numpy(rs.standard_normal(50).astype(np.float32))))
    obs = rs.standard_normal(O).astype(np.float32)
    hidden = np.zeros((1, cfg.hidden_dim), np.float32)

    def plan(ag):
        torch.manual_seed(11)
        np.random.seed(12)
        return ag.plan(obs, hidden, step=30000, t0=True)[0]
    a0 = plan(agent)
    assert agent._learner is None
    for k in range(5):
        m = agent.update(buf, 20000 + k)
        assert not agent.model.training
    assert set(m) == {"consistency_loss", "reward_loss", "value_loss", "pi_loss", "total_loss", "weighted_loss",
                      "grad_norm", "mixture_coef", "intrinsic_batch_reward_mean"}
    assert all(isinstance(v, float) and np.isfinite(v) for v in m.values())
    assert isinstance(agent.learner, DssmSimLearner) and agent.learner.hip
    assert agent.learner._graphs, "the learner never replayed its captured graph"
    assert agent.reward_rms.count == pytest.approx(5 + 1e-4) and isinstance(agent.optim, torch.optim.Adam)
    t = agent.update(buf, 20005, sync_metrics=False)
    assert torch.is_tensor(t["total_loss"]) and t["total_loss"].is_cuda
    w_pi = agent.model._pi[0].weight.detach().clone()
    zs = [torch.from_numpy(rs.standard_normal((cfg.batch_size, cfg.latent_dim)).astype(np.float32)).cuda()
          for _ in range(cfg.horizon - cfg.warmup_len + 1)]
    assert np.isfinite(agent.update_pi(zs)) and not torch.equal(w_pi, agent.model._pi[0].weight)
    agent._memories[0].clear()
    a1 = plan(agent)
    fresh = TdMpcDrnn(cfg, graph=False)
    fresh.model.load_state_dict(agent.model.state_dict())
    fresh.std = agent.std
    a2 = plan(fresh)
    assert torch.equal(a1, a2), (a1, a2)            # the plan after the updates ran on the updated weights
    assert not torch.equal(a0, a1)
