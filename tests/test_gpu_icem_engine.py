"""GPU: the MLP iCEM agent's update on the learner engine (tdmpc_amd/icem_engine.py) against float64
(tests/icem_update_ref.py, which tests/test_icem_update_cpu.py pins to the reference bit for bit and which knows nothing
of the engine).

  1  two consecutive engine updates on the recorded cases cheetah and tiny (B = 2, the two-row BatchNorm) and on wide
     (B = 130) against the float64 yardstick, every class tests/test_gpu_icem_update.py compares.
  2  the order of the BatchNorm's two writers (the intrinsic pass's H + 1 segments, then the similarity head): the
     running statistics after one update against the yardstick's, on the recorded batch and on one with the observations
     scaled by 10; for both the test computes in float64 on the CPU by how much the other order would differ.
  3  graph replay against the eager update from the same state, bitwise, across a buffer-fill change (a second capture).
  4  two runs from the same state: the same bits.
  5  TdIcemMlp(cfg, graph=True, engine=True): plan, updates, the live repack, update_pi, load_state_dict.
  6  TDMPC_ICEM_LEARNER_ENGINE=1 alone selects the engine; nothing set, the autograd learner as before.

Bounds of 1 and 2, by this project's recipe (tests/test_gpu_icem_update.py): per class of results
and per update the figure (icem_update_ref.figures) that the float32 CPU run of the yardstick shows against float64 is
the noise floor -- the largest over 1, 2, 4 and 8 CPU threads, whose summation orders differ, and over the cases of a
group -- and the bound is 8 x that floor, never below 1e-6; B = 2 has its own. `param`, `param0` and `target` are
bounded by what Adam guarantees, 2.01 lr per step taken (drnn_update_ref.bound). grad_norm is compared with the
gradients. The floors are properties of the yardstick, not of the path under test: FLOORS restates
tests/test_gpu_icem_update.py's table (measured there by tests/test_icem_update_cpu.py::
test_fp32_floors_the_gpu_bounds_are_derived_from's run of the float32 yardstick), not re-measured against the engine.

Floors (float32 CPU against float64, the largest over 1, 2, 4, 8 threads and over the cases of a group):
                  metrics   prio      intrinsic rms       grad      grad0     stats     param_q
  rest, update 0  6.86e-07  3.69e-07  1.01e-06  1.98e-07  4.27e-06  2.29e-07  2.98e-07  5.94e-05
  rest, update 1  5.62e-06  7.50e-06  1.56e-05  1.68e-06  2.37e-04  2.25e-07  6.01e-04  1.17e-04
  B = 2, update 0 1.46e-06  9.48e-07  7.33e-06  8.25e-06  7.04e-06  2.26e-08  2.42e-07  1.98e-04
  B = 2, update 1 5.48e-07  4.51e-07  1.32e-06  7.65e-07  1.21e-05  8.06e-08  1.56e-04  3.77e-04
Every comparison prints its figure beside the bound; the figures measured on an MI355X are in DESIGN.md §7 f13.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import icem_update_ref as U
from update_gpu import hold, yardstick

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
STAT_KEYS = ("_predictor.1.running_mean", "_predictor.1.running_var")


def group(name):
    return "b2" if U.CASES[name][3] == 2 else "rest"


def _gpu_learner(name, graph=False, warmup=3, batch=None, **cfg_over):
    """-> (cfg, agent, learner, buffer): IcemEngineLearner over the case's models and batch (or `batch`)."""
    from tdmpc_amd.icem_engine import IcemEngineLearner
    cfg = U.case_cfg(name)
    for k, v in cfg_over.items():
        setattr(cfg, k, v)
    model, target = U.make_models(cfg, name, device="cuda")
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cuda"), planner=None)
    learner = IcemEngineLearner(agent, graph=graph, warmup=warmup)
    assert learner.path == "engine" and learner.engine is not None
    buf = U.FakeBuffer(tuple(t.cuda() for t in (batch or U.case_batch(name))))
    return cfg, agent, learner, buf


def _snap(agent, learner, buf, m, coef):
    """One update's results by class (U.snapshot). The gradients are read from the engine's flat G by name (what
    tdmpc_lg_adam leaves there: the clipped gradient, as clip_grad_norm_ leaves it in .grad)."""
    torch.cuda.synchronize()
    eng = learner.engine
    grads = {}
    for k, (o, shape) in eng.off.items():
        n = int(np.prod(shape)) if len(shape) else 1
        grads[k] = eng.G[o:o + n].view(shape).clone()
    assert set(grads) == {k for k, _ in agent.model.named_parameters()}
    r = dict(metrics=np.array(m.tolist() + [coef]), prio=buf.prios[-1].cpu().numpy(),
             intrinsic=learner.last["intrinsic"].cpu().numpy(), rms=learner.rms.cpu().numpy(), grads=grads)
    return U.snapshot(r, agent.model, agent.model_target)


def _differences(a, b):
    differ = []
    for u in range(len(a)):
        for cls in a[u]:
            for k in a[u][cls]:
                if not np.array_equal(a[u][cls][k], b[u][cls][k]):
                    differ.append((u, cls, k, float(np.abs(a[u][cls][k] - b[u][cls][k]).max())))
    return differ


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", ["cheetah", "tiny", "wide"])
def test_two_consecutive_engine_updates_match_float64(name):
    want, scales = yardstick(U, name)
    cfg, agent, learner, buf = _gpu_learner(name)
    eng = learner.engine
    noise = [[n.cuda() for n in nz] for nz in U.case_noise(name)]
    H = cfg.horizon
    for k, step in enumerate(U.STEPS):
        m, coef = learner.update(buf, step, noise[k])
        assert not agent.model.training and m.is_cuda and m.shape == (8,)
        hold(U, f"{name} engine update {k}", _snap(agent, learner, buf, m, coef), want[k], scales[k], cfg,
             FLOORS[(group(name), k)], k)
        assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + (k + 1) * (H + 2)
    assert learner.path == "engine" and agent.optim is eng.opt_main and agent.pi_optim is eng.opt_pi
    # the policy optimiser's learning rate is IcemMlpLearner's (learner.make_optimizer(pi_params, cfg, cfg.pi_lr))
    from tdmpc_amd.icem_learner import IcemMlpLearner
    cfg2 = U.case_cfg(name)
    m2, t2 = U.make_models(cfg2, name, device="cuda")
    stock = IcemMlpLearner(SimpleNamespace(cfg=cfg2, model=m2, model_target=t2, device=torch.device("cuda"),
                                           planner=None), graph=False)
    assert eng.opt_pi.lr == stock.agent.pi_optim.param_groups[0]["lr"] == float(cfg.pi_lr)
    assert eng.opt_main.lr == stock.agent.optim.param_groups[0]["lr"] == float(cfg.lr)
    # the flat layout is SimEngine's: `_predictor` in the main range, the BatchNorm's buffers outside P
    lo, hi = eng.P.data_ptr(), eng.P.data_ptr() + 4 * eng.P.numel()
    bn = agent.model._predictor[1]
    for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked):
        assert not lo <= t.data_ptr() < hi
    assert eng.off["_predictor.3.bias"][0] < eng.n_main == eng.off["_pi.0.weight"][0]
    assert not (eng.rho != 1).any()


# ---------------------------------------------------------------------------------------------------------------- 2
def _bn_orders(name, batch, noise):
    """One float64 yardstick update on `batch` -> (its running statistics, by how much the statistics of the OTHER order
    of the BatchNorm's writers -- the similarity head's batch first, then the intrinsic pass's H + 1 segments -- differ
    from them, as icem_update_ref.figure). A train-mode BatchNorm's outputs do not depend on its running statistics, so
    both orders see the same H + 2 batches; the recurrence 0.9 x + 0.1 m over them is replayed in both orders and the
    reference's order is checked against the module."""
    cfg = U.case_cfg(name)
    ref = U.RefAgent(cfg, name, torch.float64)
    bn = ref.model._predictor[1]
    m0, v0 = bn.running_mean.clone(), bn.running_var.clone()
    seen = []
    hook = bn.register_forward_hook(lambda _m, inp, _out: seen.append(inp[0].detach().clone()))
    ref.update(batch, U.STEPS[0], noise)
    hook.remove()
    assert len(seen) == cfg.horizon + 2 and seen[-1].shape[0] == cfg.horizon * cfg.batch_size

    def run(batches):
        m, v = m0.clone(), v0.clone()
        for x in batches:
            m = 0.9 * m + 0.1 * x.mean(0)
            v = 0.9 * v + 0.1 * x.var(0, unbiased=True)
        return m, v
    ours = run(seen)
    torch.testing.assert_close(ours[0], bn.running_mean, rtol=0, atol=1e-12)
    torch.testing.assert_close(ours[1], bn.running_var, rtol=0, atol=1e-12)
    other = run(seen[-1:] + seen[:-1])
    want = {k: v.numpy().copy() for k, v in zip(STAT_KEYS, (bn.running_mean, bn.running_var))}
    swapped = max(U.figure(o.numpy(), want[k]) for k, o in zip(STAT_KEYS, other))
    return want, swapped


@pytest.mark.parametrize("scale", [1.0, 10.0])
def test_the_intrinsic_pass_moves_the_running_statistics_before_the_similarity_head(scale):
    """The other order of the two writers differs from the reference's, in float64 on the CPU, by 3.69e-2 of the largest
    statistic on the recorded cheetah batch and by 3.64e-2 with the observations scaled by 10 (the encoder's LayerNorm
    takes most of the scale out again; the similarity head's batch of rolled-out latents is what differs from the
    intrinsic pass's one-step batches): both 1.5e4 times the `stats` bound of 2.38e-6 (figures of this test's own
    `_bn_orders`, computed again and printed at every run). The test requires at least 100 times the bound."""
    name = "cheetah"
    b = U.case_batch(name)
    b = (b[0] * scale, b[1] * scale) + tuple(b[2:])
    noise = U.case_noise(name)[0]
    want, swapped = _bn_orders(name, b, noise)
    bound = U.bound(FLOORS[("rest", 0)], "stats", 0)
    print(f"BatchNorm writers, observations x {scale:g}: the other order differs by {swapped:.3e} in float64 "
          f"({swapped / bound:.1e} x the bound {bound:.2e})")
    assert swapped >= 100 * bound, "the case does not tell the two orders apart"
    cfg, agent, learner, buf = _gpu_learner(name, batch=b)
    learner.update(buf, U.STEPS[0], [n.cuda() for n in noise])
    torch.cuda.synchronize()
    sd = agent.model.state_dict()
    for k in STAT_KEYS:
        f = U.figure(sd[k].double().cpu().numpy(), want[k])
        print(f"BatchNorm writers, observations x {scale:g} {k}: gpu {f:.3e}, bound {bound:.2e}")
        assert f <= bound, (k, f, bound)
    assert int(sd["_predictor.1.num_batches_tracked"]) == 1000 + cfg.horizon + 2


# ---------------------------------------------------------------------------------------------------------------- 3, 4
def test_graph_replay_equals_the_eager_update_from_the_same_state_bitwise():
    """wide with min_std = 0 (the TruncatedNormal draws are multiplied by zero, so the eager and the captured update
    compute the same whatever the generator gives). Two graph-mode learners run the first update eagerly from the same
    state (warmup = 1). Then A runs two more updates eagerly -- explicit draws, which min_std = 0 ignores, keep a call
    eager -- and B captures and replays them, the third at another buffer fill, which takes a second capture: every
    class of result is bitwise equal after every update."""
    steps = U.STEPS + (U.STEPS[-1] + 1,)
    runs = []
    for replay in (False, True):
        cfg, agent, learner, buf = _gpu_learner("wide", graph=True, warmup=1, min_std=0.0)
        eager = [torch.zeros(cfg.batch_size, cfg.action_dim, device="cuda") for _ in range(2 * cfg.horizon + 1)]
        snaps = []
        for k, step in enumerate(steps):
            if k == 2:
                buf.idx = 1                                                # the buffer grew: another graph key
            m, coef = learner.update(buf, step, eager if k and not replay else None)
            snaps.append(_snap(agent, learner, buf, m, coef))
            assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + (k + 1) * (cfg.horizon + 2)
        runs.append((snaps, learner))
    (a, la), (b, lb) = runs
    assert len(lb._graphs) == 2 and not la._graphs, "the second and third updates were not captured"
    differ = _differences(a, b)
    print("graph replay against eager:", differ or "bitwise equal")
    assert not differ, differ


@pytest.mark.parametrize("name", ["cheetah", "wide"])
def test_two_runs_from_the_same_state_agree_bitwise(name):
    runs = []
    for _ in range(2):
        cfg, agent, learner, buf = _gpu_learner(name)
        noise = [[n.cuda() for n in nz] for nz in U.case_noise(name)]
        runs.append([_snap(agent, learner, buf, *learner.update(buf, step, noise[k])) for k, step in enumerate(U.STEPS)])
    differ = _differences(*runs)
    assert not differ, differ


# ---------------------------------------------------------------------------------------------------------------- 5, 6
def _small_planner_cfg():
    cfg = U.case_cfg("cheetah")
    for k, v in dict(num_samples=32, num_elites=8, iterations=2, train_steps=500, episode_length=50,
                     max_buffer_size=10**6, env_horizon=cfg.horizon).items():
        setattr(cfg, k, v)
    return cfg


def _filled_buffer(cfg, rs):
    from tdmpc_amd.replay import ReplayBuffer
    buf = ReplayBuffer(cfg, latent_plan=True)
    O, A = cfg.obs_shape[0], cfg.action_dim
    for _ in range(3):
        buf.add(SimpleNamespace(obs=torch.from_numpy(rs.standard_normal((51, O)).astype(np.float32)),
                                action=torch.from_numpy(rs.uniform(-1, 1, (50, A)).astype(np.float32)),
                                reward=torch.from_numpy(rs.standard_normal(50).astype(np.float32))))
    return buf


def test_agent_on_the_engine_updates_plans_on_the_live_repack_and_sees_loaded_weights(monkeypatch):
    from tdmpc_amd import TdIcemMlp
    from tdmpc_amd.icem_engine import IcemEngineLearner
    from tdmpc_amd.icem_mlp import synthetic_icem_mlp_state_dict
    monkeypatch.delenv("TDMPC_ICEM_LEARNER_ENGINE", raising=False)
    cfg = _small_planner_cfg()
    H = cfg.horizon
    rs = np.random.RandomState(5)
    agent = TdIcemMlp(cfg, graph=True, engine=True)
    agent.model.load_state_dict(synthetic_icem_mlp_state_dict(cfg, 51))
    agent.model_target.load_state_dict(synthetic_icem_mlp_state_dict(cfg, 52))
    assert agent._learner is None
    buf = _filled_buffer(cfg, rs)
    obs = rs.standard_normal(cfg.obs_shape[0]).astype(np.float32)

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
    assert all(isinstance(v, float) and np.isfinite(v) for v in m.values()), m
    assert m["current_explore_coef"] == agent.explore_coef > 0
    learner = agent.learner
    eng = learner.engine
    assert isinstance(learner, IcemEngineLearner) and learner.path == "engine"
    assert learner._graphs, "the learner never replayed its captured graph"
    assert agent.reward_rms.count == pytest.approx(5 + 1e-4)
    assert agent.optim is eng.opt_main and agent.pi_optim is eng.opt_pi
    # the captured update repacked the planner from the flat buffer: a fresh agent on the state_dict plans the same
    a1 = plan(agent)
    assert not torch.equal(a0, a1)
    other = TdIcemMlp(cfg, graph=False)
    other.model.load_state_dict(synthetic_icem_mlp_state_dict(cfg, 51))
    assert torch.equal(plan(other), a0)          # (the next plan re-evaluates this one's elites, as `agent`'s did)
    other.model.load_state_dict(agent.model.state_dict())
    other.std = agent.std
    a2 = plan(other)
    assert torch.equal(a1, a2), (a1, a2)
    assert other._learner is None
    t = agent.update(buf, 20005, sync_metrics=False)
    assert torch.is_tensor(t["total_loss"]) and t["total_loss"].is_cuda and t["total_loss"].dim() == 0
    # update_pi changes `_pi` alone
    before = {k: v.detach().clone() for k, v in agent.model.state_dict().items()}
    zs = [torch.from_numpy(rs.standard_normal((cfg.batch_size, cfg.latent_dim)).astype(np.float32)).cuda()
          for _ in range(H + 1)]
    assert np.isfinite(agent.update_pi(zs))
    for k, v in agent.model.state_dict().items():
        assert torch.equal(v, before[k]) == (not k.startswith("_pi.")), k
    # load_state_dict after the engine exists lands in the flat buffer, and the next update starts from it: seed 77's
    # weights differ from the trained ones by ~0.1 an element (lr = 1e-3), one Adam step on kept moments moves an
    # element by a few lr at the most
    sd = synthetic_icem_mlp_state_dict(cfg, 77)
    agent.model.load_state_dict(sd)
    lo, hi = eng.P.data_ptr(), eng.P.data_ptr() + 4 * eng.P.numel()
    for k, p in agent.model.named_parameters():
        assert lo <= p.data_ptr() < hi and torch.equal(eng.wv(k), sd[k].cuda()), k
    agent.update(buf, 20006)
    for k in ("_dynamics.0.weight", "_encoder.0.weight", "_predictor.3.weight", "_Q1.0.weight"):
        d = float((agent.model.state_dict()[k] - sd[k].cuda()).abs().max())
        assert 0 < d <= 10 * cfg.lr < 0.1 * float(sd[k].abs().max()), (k, d)
    assert agent.state_dict()["model"]["_pi.0.weight"].data_ptr() == eng.wv("_pi.0.weight").data_ptr()


def test_the_environment_variable_alone_selects_the_engine(monkeypatch):
    from tdmpc_amd import TdIcemMlp
    from tdmpc_amd.icem_engine import IcemEngineLearner
    from tdmpc_amd.icem_learner import IcemMlpLearner
    cfg = _small_planner_cfg()
    monkeypatch.delenv("TDMPC_ICEM_LEARNER_ENGINE", raising=False)
    stock = TdIcemMlp(cfg, graph=False)
    assert type(stock.learner) is IcemMlpLearner and isinstance(stock.optim, torch.optim.Adam)
    monkeypatch.setenv("TDMPC_ICEM_LEARNER_ENGINE", "1")
    agent = TdIcemMlp(cfg, graph=False)
    assert agent._learner is None
    learner = agent.learner
    assert type(learner) is IcemEngineLearner and learner.path == "engine"
    assert agent.optim is learner.engine.opt_main and agent.pi_optim is learner.engine.opt_pi
    m = agent.update(_filled_buffer(cfg, np.random.RandomState(6)), 20000)
    assert np.isfinite(m["total_loss"]) and np.isfinite(m["intrinsic_batch_reward_mean"])
