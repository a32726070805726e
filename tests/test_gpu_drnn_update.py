"""GPU: the DSSM update (tdmpc_amd/drnn_learner.py, the new entry points of include/tdmpc_drnn_learner.h; DESIGN.md
§7 f8) against float64 (tests/drnn_update_ref.py, which tests/test_drnn_update_cpu.py pins to the reference bit for bit).

  1  tdmpc_drnn_intrinsic_fwd with S = 4 == four tdmpc_drnn_next_fwd (h = zeros) + tdmpc_drnn_simloss_fwd calls,
     bitwise: losses and both BatchNorms' running statistics; B = 33 (one short chunk) and B = 130 (two chunks, the
     second short, every later segment off the 128-row grid); shapes (L, Hd, A) = (50, 128, 6) and (8, 32, 1).
  2  tdmpc_drnn_intrinsic_finish over three consecutive calls against float64 numpy.
  3  tdmpc_drnn_loss_forward / _backward against float64 autograd of the reference's expressions; td_lambda 0, 0.4, 1;
     rows past the 1e4 clamps.
  4  two consecutive whole updates on the recorded cases and B = 130 against the float64 yardstick.
  5  graph replay against eager from the same state; two eager runs bitwise.
  6  TdIcemDrnn.update, then plan() on repacked weights.

Bounds of 4 and 5, by this project's recipe (tests/test_gpu_drnn_train.py): per class of results the
figure (drnn_update_ref.figures) that the float32 CPU run of the same yardstick shows against float64 is the noise floor
(FLOORS below; tests/test_drnn_update_cpu.py::test_fp32_floors_the_gpu_bounds_are_derived_from recomputes them), and the
bound is 8 x that floor, never below 1e-6 (drnn_update_ref.bound). The floors are kept per update, because the second
update starts from parameters that already carry the first Adam step's sign noise (below) and its floor is one to two
orders of magnitude above the first's, and B = 2 has its own, as §7 f7 found for a two-row BatchNorm. Three classes
are bounded by what Adam guarantees instead (drnn_update_ref.bound): `param`, `param0` and `target` are largest
differences in units of the step size, which a gradient element within rounding of zero moves by up to 2 lr whatever
the precision; `param_q`, the 99th percentile, carries the floor-derived bound for the typical element.

Floors (float32 CPU against float64), largest figure over the cases of a group:
                 metrics   prio      intrinsic rms       grad      grad0     stats     param_q
  rest, update 0 9.19e-07  2.81e-07  8.72e-07  2.02e-07  1.96e-06  6.92e-08  3.45e-07  5.94e-05
  rest, update 1 4.84e-07  1.27e-06  2.18e-06  9.56e-08  8.31e-05  5.64e-08  5.79e-04  1.17e-04
  B = 2, update 0 8.42e-06 8.41e-06  3.66e-05  2.22e-05  7.85e-05  3.02e-08  1.02e-06  2.60e-03
  B = 2, update 1 3.51e-04 3.75e-05  1.49e-04  8.27e-05  2.19e-02  5.58e-08  2.90e-04  3.92e-02
  (param / param0 / target, in lr or tau lr: 0.21 / 0.47 / 0.28 on the rest, 1.70 / 1.90 / 1.71 at B = 2)
`metrics` holds the forward quantities (the loss means, pi_loss, the intrinsic mean); grad_norm, the norm of the
gradients, is compared in the `grad` class as §7 f7 separates forward values from gradients. (A first version of this
file had it under `metrics`; at B = 2, update 0, the GPU's grad_norm is 2.31e-04 off, the float32 CPU's 1.59e-05, the
largest gradient tensor's 2.84e-04 and 7.85e-05: the norm follows the gradients, whose floor it now shares.)
GPU figures measured on an MI355X: see DESIGN.md §7 f8 (every comparison prints its figure beside the bound).
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import drnn_update_ref as U
from update_gpu import gpu_learner, hold, same, snap, yardstick

pytestmark = pytest.mark.gpu

FLOORS = {
    ("rest", 0): dict(metrics=9.192e-07, prio=2.808e-07, intrinsic=8.717e-07, rms=2.019e-07, grad=1.962e-06,
                      grad0=6.920e-08, stats=3.446e-07, param_q=5.944e-05),
    ("rest", 1): dict(metrics=4.836e-07, prio=1.271e-06, intrinsic=2.179e-06, rms=9.562e-08, grad=8.308e-05,
                      grad0=5.643e-08, stats=5.789e-04, param_q=1.165e-04),
    ("b2", 0): dict(metrics=8.423e-06, prio=8.410e-06, intrinsic=3.662e-05, rms=2.218e-05, grad=7.847e-05,
                    grad0=3.022e-08, stats=1.015e-06, param_q=2.597e-03),
    ("b2", 1): dict(metrics=3.509e-04, prio=3.749e-05, intrinsic=1.492e-04, rms=8.272e-05, grad=2.185e-02,
                    grad0=5.575e-08, stats=2.897e-04, param_q=3.915e-02),
}


def group(name):
    return "b2" if U.CASES[name][4] == 2 else "rest"


# ---------------------------------------------------------------------------------------------------------------- 1
def _train_step(task, L, Hd, rows, seed=7):
    import drnn_train_ref as R
    from tdmpc_amd.dssm_train import DssmTrainStep
    cfg = R.cfg_for(task, L, Hd)
    model = R.make_model(cfg, torch.float32, seed=seed, device="cuda")
    return cfg, model, DssmTrainStep(model, max_rows=rows, max_steps=1, max_loss_rows=rows, max_losses=1)


@pytest.mark.parametrize("B", [33, 130])
@pytest.mark.parametrize("shape", [("cheetah", 50, 128), ("cartpole", 8, 32)], ids=lambda s: "-".join(map(str, s)))
def test_segmented_pass_equals_separate_passes_bitwise(shape, B):
    S = 4
    cfg, seg_model, seg_step = _train_step(*shape, rows=B)
    _, sep_model, sep_step = _train_step(*shape, rows=B)
    rs = np.random.RandomState(100 + B)
    f = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32)).cuda()  # noqa: E731
    z, keys = f(S * B, cfg.latent_dim), f(S * B, cfg.latent_dim)
    a = torch.from_numpy(rs.uniform(-1, 1, (S * B, cfg.action_dim)).astype(np.float32)).cuda()
    got = seg_step.intrinsic_loss(z, a, keys, S)
    want = []
    with torch.no_grad():
        h0 = torch.zeros(B, cfg.hidden_dim, device="cuda")
        for s in range(S):
            rows = slice(s * B, (s + 1) * B)
            zo, _, _ = sep_step.next(z[rows], a[rows], h0)
            want.append(sep_step.similarity_loss(zo, keys[rows]))
    want = torch.cat(want)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and float(got.abs().max()) > 0
    assert torch.equal(got, want), float((got - want).abs().max())
    sd_a, sd_b = seg_model.state_dict(), sep_model.state_dict()
    for k in sd_a:
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            assert torch.equal(sd_a[k], sd_b[k]), k
    assert int(sd_a["_dynamics.prior_mlp.1.num_batches_tracked"]) == 1000 + S
    assert int(sd_a["_predictor.1.num_batches_tracked"]) == 1000 + S
    assert not torch.equal(sd_a["_predictor.1.running_mean"],
                           U.synthetic_dssm_state_dict(cfg, 7)["_predictor.1.running_mean"].cuda())


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("n", [132, 4096])
def test_intrinsic_finish_matches_float64_numpy_over_three_calls(n):
    """The RunningMeanStd state to float64 rounding (the sums of n <= 4096 float64 terms run in another order than
    numpy's: at most n eps = 4.5e-13 relative; bound 1e-12), the rewards to the `intrinsic` bound of the whole update."""
    from tdmpc_amd.dssm_train import intrinsic_finish, new_rms_state
    rs = np.random.RandomState(n)
    rms = new_rms_state("cuda")
    ref = [np.float64(0.0), np.float64(1.0), np.float64(1e-4)]
    coef = torch.zeros(1, device="cuda")
    tol = U.bound(FLOORS[("rest", 0)], "intrinsic", 0)
    for call, c in enumerate((0.0, 0.3, 0.5)):
        loss = (rs.uniform(0, 2, n) ** 2).astype(np.float32) * (call + 1)
        reward = rs.standard_normal(n).astype(np.float32)
        coef.fill_(c)
        got_i, got_r = intrinsic_finish(torch.from_numpy(loss).cuda(), rms, coef, torch.from_numpy(reward).cuda())
        x = loss.astype(np.float64)
        ref = U.rms_update_from_moments(ref, x.mean(), x.var())
        sd = np.sqrt(ref[1])
        want_i = np.maximum(x / sd - ref[0] / sd, 0)
        want_r = np.float64(np.float32(c)) * want_i + reward
        np.testing.assert_allclose(rms.cpu().numpy(), np.array(ref, np.float64), rtol=1e-12, atol=0)
        fi, fr = U.figure(got_i.cpu().numpy(), want_i), U.figure(got_r.cpu().numpy(), want_r)
        print(f"intrinsic_finish n {n} call {call}: intrinsic {fi:.3e}, reward_pi {fr:.3e} (bound {tol:.2e})")
        assert fi <= tol and fr <= tol
        assert (want_i == 0).any() and (want_i > 0).any()   # the threshold is active


# ---------------------------------------------------------------------------------------------------------------- 3
def _loss_ref(sim, q1, q2, rp, rw, rwpi, nq, w, coefs):
    """The reference's expressions (tdmpc_icem_similarity_drnn.py:471-485, :497-499, :522-530), [H, B, 1] operands."""
    sc, rc, vc, disc, lam = coefs
    H = sim.shape[0]
    discounts = torch.ones_like(rwpi) * disc
    last = nq[-1]
    inputs = rwpi + discounts * nq * (1 - lam)
    outputs = []
    for index in reversed(range(H)):
        last = inputs[index] + discounts[index] * last * lam
        outputs.append(last)
    td = torch.stack(list(reversed(outputs)), dim=0)
    mse = lambda x, y: (x - y) ** 2  # noqa: E731
    reward_loss = sum(mse(rp[t], rw[t]) for t in range(H))
    value_loss = sum(mse(q1[t], td[t]) + mse(q2[t], td[t]) for t in range(H))
    priority_loss = sum((q1[t] - td[t]).abs() + (q2[t] - td[t]).abs() for t in range(H))
    similarity_loss = sim.sum(dim=0)
    model_loss = sc * similarity_loss.clamp(max=1e4) + rc * reward_loss.clamp(max=1e4)
    td_loss = vc * value_loss.clamp(max=1e4)
    weighted = (model_loss * w).mean() + td_loss.mean()   # [B, 1] * [B]: the [B, B] broadcast
    return dict(td=td, sim=similarity_loss, rew=reward_loss, val=value_loss, prio=priority_loss.clamp(max=1e4),
                model=model_loss, tdl=td_loss, weighted=weighted, total=(model_loss + td_loss).mean())


@pytest.mark.parametrize("lam", [0.0, 0.4, 1.0])
def test_fused_loss_matches_float64_autograd(lam):
    """H = 3, B = 600 (three workgroups of the row kernel, two strides of the means kernel). A fifth of the rows carry
    similarity, reward or value sums past 1e4: their clamps are active and their gradients zero. fp32 sums of at most
    3 terms per row and 600 rows per mean: rtol 1e-5 (atol 1e-6 of the tensor's largest entry)."""
    from tdmpc_amd.dssm_train import _DssmFusedLoss
    H, B = 3, 600
    rs = np.random.RandomState(int(lam * 10))
    f = lambda *s: rs.standard_normal(s)  # noqa: E731
    sim, q1, q2, rp, rw, rwpi, nq = (f(H, B) for _ in range(7))
    sim = np.abs(sim)
    sim[:, 0:40] *= 1e4        # similarity past the clamp
    rp[:, 40:80] *= 200        # reward loss past the clamp
    q1[:, 80:120] *= 200       # value loss (and the priority's sum of absolute values stays below 1e4)
    q2[:, 120:140] *= 1e4      # priority past its clamp as well
    w = rs.uniform(0.5, 1.0, B)
    coefs = (1.0, 0.5, 0.1, 0.99, lam)
    t64 = [torch.from_numpy(x).unsqueeze(2).requires_grad_(i < 4) for i, x in enumerate((sim, q1, q2, rp, rw, rwpi, nq))]
    want = _loss_ref(*t64, torch.from_numpy(w), coefs)
    up = 0.7
    (want["weighted"] * up).backward()
    assert (want["sim"] > 1e4).any() and (want["rew"] > 1e4).any() and (want["val"] > 1e4).any()
    assert (want["prio"] == 1e4).any() and (want["sim"] < 1e4).any()
    t32 = [torch.from_numpy(x.astype(np.float32)).cuda().requires_grad_(i < 4)
           for i, x in enumerate((sim, q1, q2, rp, rw, rwpi, nq))]
    scal, rows, td = _DssmFusedLoss.apply(*t32, torch.from_numpy(w.astype(np.float32)).cuda(), coefs)
    (scal[4] * up).backward()
    torch.cuda.synchronize()

    same("td", td, want["td"])
    for i, k in enumerate(("sim", "rew", "val", "prio", "model", "tdl")):
        same(k, rows[i], want[k])
    wmean = float(np.mean(w))
    same("scal", scal, torch.stack([want["sim"].mean(), want["rew"].mean(), want["val"].mean(), want["total"],
                                    want["weighted"], torch.tensor(wmean), want["model"].mean(), want["tdl"].mean()]))
    for i, k in enumerate(("dsim", "dq1", "dq2", "drp")):
        same(k, t32[i].grad, t64[i].grad)
        assert (t32[i].grad == 0).any() and (t32[i].grad != 0).any(), k


# ---------------------------------------------------------------------------------------------------------------- 4, 5
def _gpu_learner(name, **kw):
    from tdmpc_amd.drnn_learner import DssmLearner
    return gpu_learner(U, DssmLearner, name, **kw)


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
        assert int(agent.model._dynamics.prior_mlp[1].num_batches_tracked) == 1000 + (k + 1) * (2 * H + 1)
        assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + (k + 1) * (H + 2)
    assert len(learner.train_step._next_pool.free) == H and len(learner.train_step._loss_pool.free) == 1


def test_graph_replay_matches_eager_and_eager_is_reproducible():
    """cheetah with min_std = 0 (no TruncatedNormal draws, so the eager and the captured update consume no generator
    state). Two graph-mode learners (the same optimiser arithmetic: torch's capturable Adam takes its bias corrections
    in float32) run the first update eagerly from the same state: everything the new kernels write (the intrinsic
    rewards, the priorities, the loss means) is bitwise equal. Then A runs the second update eagerly -- explicit draws,
    which min_std = 0 ignores, keep a call eager -- and B captures and replays it: within the bound of a second update,
    A as the reference."""
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
    for cls in ("intrinsic", "prio", "rms"):
        for k in a[0][cls]:
            assert np.array_equal(a[0][cls][k], b[0][cls][k]), (cls, k)
    for k in ("consistency_loss", "reward_loss", "value_loss", "total_loss", "weighted_loss"):
        assert a[0]["metrics"][k] == b[0]["metrics"][k], k
    zero = {k: 1.0 for k in U.ZERO_MEAN}   # (grad0 against a float32 reference: absolute, the bound is 1e-6)
    hold(U, "graph replay against eager, update 1", b[1], a[1], zero, U.case_cfg("cheetah"), FLOORS[("rest", 1)], 1)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_agent_update_returns_reference_metrics_and_plan_repacks():
    from tdmpc_amd.drnn_icem import TdIcemDrnn
    from tdmpc_amd.replay import ReplayBuffer
    cfg = U.case_cfg("cheetah")
    for k, v in dict(num_samples=32, num_elites=8, iterations=2, train_steps=500, episode_length=50,
                     max_buffer_size=10**6, env_horizon=cfg.horizon, noise_beta=0.0).items():
        setattr(cfg, k, v)
    rs = np.random.RandomState(5)
    agent = TdIcemDrnn(cfg, graph=True)
    agent.model.load_state_dict(U.synthetic_dssm_state_dict(cfg, 31))
    agent.model_target.load_state_dict(U.synthetic_dssm_state_dict(cfg, 32))
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
    assert agent.explore_coef == 0
    for k in range(5):
        m = agent.update(buf, 20000 + k)
        assert not agent.model.training
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
          for _ in range(cfg.horizon + 1)]
    assert np.isfinite(agent.update_pi(zs)) and not torch.equal(w_pi, agent.model._pi[0].weight)
    a1 = plan(agent)
    fresh = TdIcemDrnn(cfg, graph=False)
    fresh.model.load_state_dict(agent.model.state_dict())
    fresh.std = agent.std
    a2 = plan(fresh)
    assert torch.equal(a1, a2), (a1, a2)            # the plan after the updates ran on the updated weights
    assert not torch.equal(a0, a1)
