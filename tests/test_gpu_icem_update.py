"""GPU: the MLP iCEM agent's update (tdmpc_amd/icem_learner.py, include/tdmpc_icem_learner.h) against
float64 (tests/icem_update_ref.py, which tests/test_icem_update_cpu.py pins to the reference bit for bit).

  1  tdmpc_icem_intrinsic_fwd against the float64 CPU modules: (L, A) = (8, 1), (50, 6), (256, 38), S = 4, B = 2 (the
     two-row BatchNorm), 33 (one partial 128-row chunk), 130 (two chunks, later segments off the 128-row grid), and
     (8, 1), S = 2, B = 2048 (the other GEMM tile, at the row cap). The segmented call == S one-segment calls bitwise,
     losses and running statistics; two runs give the same bits.
  2  tdmpc_icem_loss_forward / _backward against float64 autograd of the reference's expressions: H = 1, 3; B = 2, 130;
     rho = 1, 0.5; one row past every 1e4 clamp.
  3  two consecutive whole updates on the recorded cases and B = 130 against the float64 yardstick.
  4  graph replay against the eager update from the same state, bitwise.
  5  TdIcemMlp.update, then plan() on repacked weights; num_batches_tracked moves by H + 2.

Bounds of 1: per case, 8 x the figure (max |difference| / max |float64 value|) that the SAME modules show in float32 on
the CPU against float64 on the same inputs, never below 1e-6 (the recipe of 3, measured in the test itself since the
inputs are the test's own).

Bounds of 3, by this project's recipe (tests/test_gpu_drnn_update.py): per class of results and
per update the figure (drnn_update_ref.figures) that the float32 CPU run of the yardstick shows against float64 is the
noise floor -- the largest over 1, 2, 4 and 8 CPU threads, whose summation orders differ -- and the
bound is 8 x that floor, never below 1e-6; B = 2 has its own. `param`, `param0` and `target` are bounded by what Adam
guarantees, 2.01 lr per step taken (drnn_update_ref.bound). grad_norm is compared with the gradients.

Floors (float32 CPU against float64, the largest over 1, 2, 4, 8 threads and over the cases of a group):
                  metrics   prio      intrinsic rms       grad      grad0     stats     param_q
  rest, update 0  6.86e-07  3.69e-07  1.01e-06  1.98e-07  4.27e-06  2.29e-07  2.98e-07  5.94e-05
  rest, update 1  5.62e-06  7.50e-06  1.56e-05  1.68e-06  2.37e-04  2.25e-07  6.01e-04  1.17e-04
  B = 2, update 0 1.46e-06  9.48e-07  7.33e-06  8.25e-06  7.04e-06  2.26e-08  2.42e-07  1.98e-04
  B = 2, update 1 5.48e-07  4.51e-07  1.32e-06  7.65e-07  1.21e-05  8.06e-08  1.56e-04  3.77e-04
  (param / param0 / target, in lr or tau lr: 1.20 / 0.79 / 1.20 on the rest, 0.08 / 1.38 / 0.84 at B = 2)
GPU figures measured on an MI355X: see DESIGN.md §7 f10 (every comparison prints its figure beside the bound).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import icem_update_ref as U
from tdmpc_amd.config import make_cfg
from update_gpu import gpu_learner, hold, same, snap, yardstick

pytestmark = pytest.mark.gpu

FLOORS = {
    ("rest", 0): dict(metrics=6.863e-07, prio=3.687e-07, intrinsic=1.006e-06, rms=1.978e-07, grad=4.273e-06,
                      grad0=2.286e-07, stats=2.980e-07, param_q=5.937e-05),
    ("rest", 1): dict(metrics=5.617e-06, prio=7.502e-06, intrinsic=1.559e-05, rms=1.676e-06, grad=2.368e-04,
                      grad0=2.246e-07, stats=6.014e-04, param_q=1.174e-04),
    ("b2", 0): dict(metrics=1.462e-06, prio=9.478e-07, intrinsic=7.325e-06, rms=8.252e-06, grad=7.040e-06,
                    grad0=2.258e-08, stats=2.421e-07, param_q=1.979e-04),
    ("b2", 1): dict(metrics=5.480e-07, prio=4.511e-07, intrinsic=1.322e-06, rms=7.648e-07, grad=1.210e-05,
                    grad0=8.061e-08, stats=1.563e-04, param_q=3.769e-04),
}


def group(name):
    return "b2" if U.CASES[name][3] == 2 else "rest"


# ---------------------------------------------------------------------------------------------------------------- 1
SHAPES = {(8, 1): "cartpole", (50, 6): "cheetah", (256, 38): "dog"}


def _shape_model(L, A, seed=7):
    from tdmpc_amd.icem_mlp import IcemMlpModel, synthetic_icem_mlp_state_dict
    cfg = make_cfg(SHAPES[(L, A)], latent_dim=L)
    assert cfg.action_dim == A
    model = IcemMlpModel(cfg, init="none")
    model.load_state_dict(synthetic_icem_mlp_state_dict(cfg, seed))
    return cfg, model


def _modules_loss(model, z, a, keys, S):
    """The reference's H + 1 passes (:328-334) on the eager modules in the model's precision -> loss [S B]; moves
    `_predictor.1`'s running statistics S times."""
    B = z.shape[0] // S
    out = []
    model.train()
    with torch.no_grad():
        for s in range(S):
            r = slice(s * B, (s + 1) * B)
            zl, _ = model.next(z[r], a[r])
            pred = F.normalize(model.pred_z(zl), dim=-1, p=2)
            out.append(2.0 - 2.0 * (pred * F.normalize(keys[r], dim=-1, p=2)).sum(dim=-1))
    return torch.cat(out)


def _stats(model):
    return torch.cat([model._predictor[1].running_mean, model._predictor[1].running_var]).detach().double().cpu().numpy()


@pytest.mark.parametrize("L,A,S,B", [(L, A, 4, B) for (L, A) in SHAPES for B in (2, 33, 130)] + [(8, 1, 2, 2048)])
def test_intrinsic_pass_matches_float64_modules_and_its_one_segment_calls_bitwise(L, A, S, B):
    from tdmpc_amd.icem_learner import IcemTrainStep
    rs = np.random.RandomState(1000 * L + B)
    z = rs.standard_normal((S * B, L)).astype(np.float32)
    keys = rs.standard_normal((S * B, L)).astype(np.float32)
    a = rs.uniform(-1, 1, (S * B, A)).astype(np.float32)
    t = lambda x, dt: torch.from_numpy(x).to(dt)  # noqa: E731
    cfg, m64 = _shape_model(L, A)
    want = _modules_loss(m64.double(), t(z, torch.float64), t(a, torch.float64), t(keys, torch.float64), S).numpy()
    _, m32 = _shape_model(L, A)
    cpu = _modules_loss(m32, t(z, torch.float32), t(a, torch.float32), t(keys, torch.float32), S).numpy()
    floor_loss, floor_stats = U.figure(cpu, want), U.figure(_stats(m32), _stats(m64))

    runs = []
    for segmented in (True, True, False):
        _, model = _shape_model(L, A)
        model = model.cuda().train()
        step = IcemTrainStep(model, max_loss_rows=B)
        zc, ac, kc = (torch.from_numpy(x).cuda() for x in (z, a, keys))
        if segmented:
            loss = step.intrinsic_loss(zc, ac, kc, S)
        else:
            loss = torch.cat([step.intrinsic_loss(zc[s * B:(s + 1) * B], ac[s * B:(s + 1) * B], kc[s * B:(s + 1) * B], 1)
                              for s in range(S)])
        torch.cuda.synchronize()
        assert int(model._predictor[1].num_batches_tracked) == 1000 + S
        runs.append((loss.cpu(), model._predictor[1].running_mean.cpu(), model._predictor[1].running_var.cpu(), model))
    first, again, separate = runs
    assert torch.isfinite(first[0]).all() and float(first[0].abs().max()) > 0
    for k, what in enumerate(("loss", "running_mean", "running_var")):
        assert torch.equal(first[k], again[k]), f"two runs differ in {what}"
        assert torch.equal(first[k], separate[k]), (f"segmented and one-segment calls differ in {what}",
                                                    float((first[k] - separate[k]).abs().max()))
    f_loss, f_stats = U.figure(first[0].double().numpy(), want), U.figure(_stats(first[3]), _stats(m64))
    b_loss, b_stats = max(8 * floor_loss, 1e-6), max(8 * floor_stats, 1e-6)
    print(f"intrinsic L {L} A {A} S {S} B {B}: loss gpu {f_loss:.3e} (cpu fp32 {floor_loss:.3e}, bound {b_loss:.2e}); "
          f"stats gpu {f_stats:.3e} (cpu fp32 {floor_stats:.3e}, bound {b_stats:.2e})")
    assert f_loss <= b_loss and f_stats <= b_stats
    sd0 = _shape_model(L, A)[1].state_dict()
    assert not torch.equal(first[1], sd0["_predictor.1.running_mean"])


# ---------------------------------------------------------------------------------------------------------------- 2
def _loss_ref(sim, q1, q2, rp, rw, rwpi, nq, w, coefs):
    """The reference's expressions (:384-406), [H, B, 1] operands and w [B]."""
    sc, rc, vc, disc, rho_ = coefs
    H = sim.shape[0]
    reward_loss, value_loss, priority_loss = 0, 0, 0
    tds = []
    for t in range(H):
        rho = rho_ ** t
        td = rwpi[t] + disc * nq[t]
        tds.append(td)
        reward_loss += F.mse_loss(rp[t], rw[t], reduction="none") * rho
        value_loss += (F.mse_loss(q1[t], td, reduction="none") + F.mse_loss(q2[t], td, reduction="none")) * rho
        priority_loss += (F.l1_loss(q1[t], td, reduction="none") + F.l1_loss(q2[t], td, reduction="none")) * rho
    similarity_loss = sim.sum(dim=0)
    total = sc * similarity_loss.clamp(max=1e4) + rc * reward_loss.clamp(max=1e4) + vc * value_loss.clamp(max=1e4)
    weighted = (total * w).mean()                             # [B, 1] * [B]: the [B, B] broadcast
    weighted.register_hook(lambda grad: grad * (1 / H))
    return dict(td=torch.stack(tds), sim=similarity_loss, rew=reward_loss, val=value_loss,
                prio=priority_loss.clamp(max=1e4), total=total, weighted=weighted)


@pytest.mark.parametrize("rho", [1.0, 0.5])
@pytest.mark.parametrize("B", [2, 130])
@pytest.mark.parametrize("H", [1, 3])
def test_fused_loss_matches_float64_autograd(H, B, rho):
    """Row 0 carries similarity, reward, value and priority sums past 1e4: its clamps are active and its gradients zero;
    row 1 does not. fp32 sums of at most 3 terms per row and 130 rows per mean: rtol 1e-5 (atol 1e-6 of the tensor's
    largest entry)."""
    from tdmpc_amd.icem_learner import _IcemFusedLoss
    rs = np.random.RandomState(100 * H + B + int(10 * rho))
    sim, q1, q2, rp, rw, rwpi, nq = (rs.standard_normal((H, B)) for _ in range(7))
    sim = np.abs(sim)
    sim[:, 0] = 2e4
    rp[:, 0] = 300.0 * (1 + np.arange(H))
    q1[:, 0] = 2e4
    w = rs.uniform(0.5, 1.0, B)
    coefs = (1.0, 0.5, 0.1, 0.99, rho)
    ops = (sim, q1, q2, rp, rw, rwpi, nq)
    t64 = [torch.from_numpy(x).unsqueeze(2).requires_grad_(i < 4) for i, x in enumerate(ops)]
    want = _loss_ref(*t64, torch.from_numpy(w), coefs)
    up = 0.7
    (want["weighted"] * up).backward()
    for k in ("sim", "rew", "val"):
        assert float(want[k][0].detach()) > 1e4 and float(want[k][1].detach()) < 1e4, k
    assert float(want["prio"][0].detach()) == 1e4 and float(want["prio"][1].detach()) < 1e4
    t32 = [torch.from_numpy(x.astype(np.float32)).cuda().requires_grad_(i < 4) for i, x in enumerate(ops)]
    scal, rows, td = _IcemFusedLoss.apply(*t32, torch.from_numpy(w.astype(np.float32)).cuda(), coefs)
    (scal[4] * up).backward()
    torch.cuda.synchronize()

    same("td", td, want["td"])
    for i, k in enumerate(("sim", "rew", "val", "prio", "total")):
        same(k, rows[i], want[k])
    same("scal", scal, torch.stack([want["sim"].mean(), want["rew"].mean(), want["val"].mean(), want["total"].mean(),
                                    want["weighted"], torch.tensor(float(np.mean(w)))]))
    for i, k in enumerate(("dsim", "dq1", "dq2", "drp")):
        same(k, t32[i].grad, t64[i].grad)
        assert not t32[i].grad[:, 0].any() and t32[i].grad[:, 1].all(), k


# ---------------------------------------------------------------------------------------------------------------- 3, 4
def _gpu_learner(name, **kw):
    from tdmpc_amd.icem_learner import IcemMlpLearner
    return gpu_learner(U, IcemMlpLearner, name, **kw)


@pytest.mark.parametrize("name", ["cheetah", "tiny", "wide"])
def test_two_consecutive_updates_match_float64(name):
    want, scales = yardstick(U, name)
    cfg, agent, learner, buf = _gpu_learner(name)
    noise = [[n.cuda() for n in nz] for nz in U.case_noise(name)]
    H = cfg.horizon
    for k, step in enumerate(U.STEPS):
        m, coef = learner.update(buf, step, noise[k])
        assert not agent.model.training
        hold(U, f"{name} update {k}", snap(U, agent, learner, buf, m.tolist() + [coef]), want[k], scales[k],
             cfg, FLOORS[(group(name), k)], k)
        assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + (k + 1) * (H + 2)
    assert len(learner.train_step._loss_pool.free) == 1


def test_graph_replay_equals_the_eager_update_from_the_same_state_bitwise():
    """cheetah with min_std = 0 (no TruncatedNormal draws, so the eager and the captured update consume no generator
    state). Two graph-mode learners (the same optimiser arithmetic: torch's capturable Adam) run the first update
    eagerly from the same state. Then A runs the second update eagerly -- explicit draws, which min_std = 0 ignores,
    keep a call eager -- and B captures and replays it: every class of result is bitwise equal."""
    runs = []
    for replay in (False, True):
        cfg, agent, learner, buf = _gpu_learner("cheetah", graph=True, warmup=1, min_std=0.0)
        eager = [torch.zeros(cfg.batch_size, cfg.action_dim, device="cuda") for _ in range(2 * cfg.horizon + 1)]
        snaps = []
        for k, step in enumerate(U.STEPS):
            m, coef = learner.update(buf, step, eager if k and not replay else None)
            snaps.append(snap(U, agent, learner, buf, m.tolist() + [coef]))
        runs.append((snaps, learner))
    (a, la), (b, lb) = runs
    assert lb._graphs and not la._graphs, "the second update was not captured"
    differ = []
    for u in range(2):
        for cls in a[u]:
            for k in a[u][cls]:
                if not np.array_equal(a[u][cls][k], b[u][cls][k]):
                    differ.append((u, cls, k, float(np.abs(a[u][cls][k] - b[u][cls][k]).max())))
    print("graph replay against eager:", differ or "bitwise equal")
    assert not differ, differ


# ---------------------------------------------------------------------------------------------------------------- 5
def test_agent_update_returns_reference_metrics_and_plan_repacks():
    from tdmpc_amd import TdIcemMlp
    from tdmpc_amd.icem_mlp import synthetic_icem_mlp_state_dict
    from tdmpc_amd.replay import ReplayBuffer
    cfg = U.case_cfg("cheetah")
    for k, v in dict(num_samples=32, num_elites=8, iterations=2, train_steps=500, episode_length=50,
                     max_buffer_size=10**6, env_horizon=cfg.horizon).items():
        setattr(cfg, k, v)
    H = cfg.horizon
    rs = np.random.RandomState(5)
    agent = TdIcemMlp(cfg, graph=True)
    agent.model.load_state_dict(synthetic_icem_mlp_state_dict(cfg, 51))
    agent.model_target.load_state_dict(synthetic_icem_mlp_state_dict(cfg, 52))
    assert agent._learner is None
    buf = ReplayBuffer(cfg, latent_plan=True)
    O, A = cfg.obs_shape[0], cfg.action_dim
    for _ in range(3):
        buf.add(SimpleNamespace(obs=torch.from_numpy(rs.standard_normal((51, O)).astype(np.float32)),
                                action=torch.from_numpy(rs.uniform(-1, 1, (50, A)).astype(np.float32)),
                                reward=torch.from_numpy(rs.standard_normal(50).astype(np.float32))))
    obs = rs.standard_normal(O).astype(np.float32)

    def plan(ag):
        torch.manual_seed(11)
        np.random.seed(12)
        return ag.plan(obs, step=30000, t0=True)[0]
    a0 = plan(agent)
    assert agent._learner is None and agent.explore_coef == 0            # planning built no learner
    for k in range(5):
        m = agent.update(buf, 20000 + k)
        assert not agent.model.training
        assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + (k + 1) * (H + 2)
    assert set(m) == {"consistency_loss", "reward_loss", "value_loss", "pi_loss", "total_loss", "weighted_loss",
                      "grad_norm", "intrinsic_batch_reward_mean", "current_explore_coef", "mixture_coef"}
    assert all(isinstance(v, float) and np.isfinite(v) for v in m.values())
    assert m["current_explore_coef"] == agent.explore_coef > 0
    assert agent.learner._graphs, "the learner never replayed its captured graph"
    assert agent.reward_rms.count == pytest.approx(5 + 1e-4) and isinstance(agent.optim, torch.optim.Adam)
    t = agent.update(buf, 20005, sync_metrics=False)
    assert torch.is_tensor(t["total_loss"]) and t["total_loss"].is_cuda
    w_pi = agent.model._pi[0].weight.detach().clone()
    zs = [torch.from_numpy(rs.standard_normal((cfg.batch_size, cfg.latent_dim)).astype(np.float32)).cuda()
          for _ in range(H + 1)]
    assert np.isfinite(agent.update_pi(zs)) and not torch.equal(w_pi, agent.model._pi[0].weight)
    a1 = plan(agent)
    # The MLP agent re-evaluates the previous plan's elites at an episode start too (:204), so a second agent repeats
    # the first plan on the first weights before it takes the updated ones. TdICEM, whose model has no predictor, packs
    # the same TOLD tensors: the planner selects them by name.
    from tdmpc_amd import TdICEM
    told = lambda sd: {k: v for k, v in sd.items() if not k.startswith("_predictor")}  # noqa: E731
    for other, pick in ((TdIcemMlp(cfg, graph=False), dict), (TdICEM(cfg), told)):
        other.model.load_state_dict(pick(synthetic_icem_mlp_state_dict(cfg, 51)))
        assert torch.equal(plan(other), a0)
        other.model.load_state_dict(pick(agent.model.state_dict()))
        other.std = agent.std
        a2 = plan(other)
        assert torch.equal(a1, a2), (type(other).__name__, a1, a2)   # the plan after the updates ran on the updated weights
    assert not torch.equal(a0, a1)
