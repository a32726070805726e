"""GPU: the DSSM iCEM agent's update on the learner engine (tdmpc_amd/dssm_engine.py) against float64
(tests/drnn_update_ref.py, which tests/test_drnn_update_cpu.py pins to the reference bit for bit and which knows nothing
of the engine).

  1  two consecutive engine updates on the recorded cases cheetah and tiny (B = 2, the two-row BatchNorm) and on wide
     (B = 130) against the float64 yardstick, every class tests/test_gpu_drnn_update.py compares.
  2  the order of the BatchNorms' writers: `_dynamics.prior_mlp.1` (the intrinsic pass's H + 1 segments, then the
     rollout's H steps) and `_predictor.1` (the H + 1 segments, then the similarity head): the running statistics after
     one update against the yardstick's; for both the test computes in float64 on the CPU by how much the other order
     would differ.
  3  graph replay against the eager update from the same state, bitwise, across a buffer-fill change (a second capture).
  4  two runs from the same state: the same bits (a stream race on the statistics would show here as well).
  5  TdIcemDrnn(cfg, graph=True, engine=True): plan, updates, plan on the new weights, load_state_dict.
  6  TDMPC_DSSM_LEARNER_ENGINE=1 alone selects the engine for TdIcemDrnn and leaves TdMpcDrnn on DssmSimLearner.

Bounds of 1 and 2: tests/test_gpu_drnn_update.py's FLOORS (float32 CPU against float64 on the same yardstick, per update
and per group of cases) x 8, never below 1e-6, and what Adam guarantees for `param`, `param0` and `target`
(drnn_update_ref.bound): properties of the yardstick, not of the path under test, values unchanged. Every comparison
prints its figure beside the bound; the figures measured on an MI355X are in DESIGN.md §7 f14.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import drnn_update_ref as U
from test_gpu_drnn_update import FLOORS, group
from update_gpu import hold, yardstick

pytestmark = pytest.mark.gpu

DYN_BN, PRED_BN = "_dynamics.prior_mlp.1", "_predictor.1"


def _gpu_learner(name, graph=False, warmup=3, batch=None, **cfg_over):
    """-> (cfg, agent, learner, buffer): DssmEngineLearner over the case's models and batch (or `batch`)."""
    from tdmpc_amd.dssm_engine import DssmEngineLearner
    cfg = U.case_cfg(name)
    for k, v in cfg_over.items():
        setattr(cfg, k, v)
    model, target = U.make_models(cfg, name, device="cuda")
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cuda"), planner=None)
    learner = DssmEngineLearner(agent, graph=graph, warmup=warmup)
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


def _nbt(model, H, updates):
    assert int(model._dynamics.prior_mlp[1].num_batches_tracked) == 1000 + updates * (2 * H + 1)
    assert int(model._predictor[1].num_batches_tracked) == 1000 + updates * (H + 2)


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
    for k, step in enumerate(U.STEPS):
        m, coef = learner.update(buf, step, noise[k])
        assert not agent.model.training and m.is_cuda and m.shape == (8,)
        hold(U, f"{name} engine update {k}", _snap(agent, learner, buf, m, coef), want[k], scales[k], cfg,
             FLOORS[(group(name), k)], k)
        _nbt(agent.model, cfg.horizon, k + 1)
    assert agent.optim is eng.opt_main and agent.pi_optim is eng.opt_pi
    assert eng.opt_pi.lr == float(cfg.pi_lr) and eng.opt_main.lr == float(cfg.lr)
    # the flat layout: both BatchNorms' buffers outside P, `_predictor` in the main range
    lo, hi = eng.P.data_ptr(), eng.P.data_ptr() + 4 * eng.P.numel()
    for bn in (agent.model._predictor[1], agent.model._dynamics.prior_mlp[1]):
        for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked):
            assert not lo <= t.data_ptr() < hi
    assert eng.off["_predictor.3.bias"][0] < eng.n_main == eng.off["_pi.0.weight"][0]
    assert not (eng.rho != 1).any()


# ---------------------------------------------------------------------------------------------------------------- 2
def _bn_orders(name, batch, noise):
    """One float64 yardstick update on `batch` -> {module: (its running statistics, by how much the statistics of the
    OTHER order of its writers differ from them, as drnn_update_ref.figure)}. A train-mode BatchNorm's outputs do not
    depend on its running statistics, so both orders see the same batches; the recurrence 0.9 x + 0.1 m over them is
    replayed in both orders and the reference's order is checked against the module. The other order: the rollout's H
    steps (prior_mlp.1) or the similarity head's batch (`_predictor.1`) BEFORE the intrinsic pass's H + 1 segments."""
    cfg = U.case_cfg(name)
    H = cfg.horizon
    ref = U.RefAgent(cfg, name, torch.float64)
    mods = {DYN_BN: ref.model._dynamics.prior_mlp[1], PRED_BN: ref.model._predictor[1]}
    start = {k: (bn.running_mean.clone(), bn.running_var.clone()) for k, bn in mods.items()}
    seen = {k: [] for k in mods}
    hooks = [bn.register_forward_hook(lambda _m, inp, _out, k=k: seen[k].append(inp[0].detach().clone()))
             for k, bn in mods.items()]
    ref.update(batch, U.STEPS[0], noise)
    for h in hooks:
        h.remove()
    assert len(seen[DYN_BN]) == 2 * H + 1 and len(seen[PRED_BN]) == H + 2
    assert seen[PRED_BN][-1].shape[0] == H * cfg.batch_size

    def run(k, batches):
        m, v = (t.clone() for t in start[k])
        for x in batches:
            m = 0.9 * m + 0.1 * x.mean(0)
            v = 0.9 * v + 0.1 * x.var(0, unbiased=True)
        return m, v
    out = {}
    for k, bn in mods.items():
        ours = run(k, seen[k])
        torch.testing.assert_close(ours[0], bn.running_mean, rtol=0, atol=1e-12)
        torch.testing.assert_close(ours[1], bn.running_var, rtol=0, atol=1e-12)
        other = run(k, seen[k][H + 1:] + seen[k][:H + 1])
        want = {k + ".running_mean": bn.running_mean.numpy().copy(), k + ".running_var": bn.running_var.numpy().copy()}
        out[k] = (want, max(U.figure(o.numpy(), w) for o, w in zip(other, want.values())))
    return out


def test_the_intrinsic_pass_moves_the_running_statistics_before_the_rollout_and_the_similarity_head():
    """For each BatchNorm the other order of its two writers must differ from the reference's, in float64 on the CPU, by
    at least 100 times the `stats` bound (printed at every run), so that the test tells the orders apart; the engine is
    held to the reference's order at that bound."""
    name = "cheetah"
    b, noise = U.case_batch(name), U.case_noise(name)[0]
    orders = _bn_orders(name, b, noise)
    bound = U.bound(FLOORS[("rest", 0)], "stats", 0)
    for k, (_, swapped) in orders.items():
        print(f"{k}: the other order of its writers differs by {swapped:.3e} in float64 "
              f"({swapped / bound:.1e} x the bound {bound:.2e})")
        assert swapped >= 100 * bound, (k, "the case does not tell the two orders apart")
    cfg, agent, learner, buf = _gpu_learner(name, batch=b)
    learner.update(buf, U.STEPS[0], [n.cuda() for n in noise])
    torch.cuda.synchronize()
    sd = agent.model.state_dict()
    for k, (want, _) in orders.items():
        for key, w in want.items():
            f = U.figure(sd[key].double().cpu().numpy(), w)
            print(f"{key}: gpu {f:.3e}, bound {bound:.2e}")
            assert f <= bound, (key, f, bound)
    _nbt(agent.model, cfg.horizon, 1)


# ---------------------------------------------------------------------------------------------------------------- 3, 4
def test_graph_replay_equals_the_eager_update_from_the_same_state_bitwise():
    """wide with min_std = 0 (the TruncatedNormal draws are multiplied by zero, so the eager and the captured update
    compute the same whatever the generator gives). Two graph-mode learners run the first update eagerly from the same
    state (warmup = 1). Then A runs two more updates eagerly -- explicit draws, which min_std = 0 ignores, keep a call
    eager -- and B captures and replays them, the third at another buffer fill, which takes a second capture: every
    class of result (parameters, running statistics, priorities, metrics, the gradients Adam left) is bitwise equal
    after every update, and so are the Adam moments at the end."""
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
            _nbt(agent.model, cfg.horizon, k + 1)
        runs.append((snaps, learner))
    (a, la), (b, lb) = runs
    assert len(lb._graphs) == 2 and not la._graphs, "the second and third updates were not captured"
    differ = _differences(a, b)
    print("graph replay against eager:", differ or "bitwise equal")
    assert not differ, differ
    for oa, ob in ((la.engine.opt_main, lb.engine.opt_main), (la.engine.opt_pi, lb.engine.opt_pi)):
        assert torch.equal(oa.exp_avg, ob.exp_avg) and torch.equal(oa.exp_avg_sq, ob.exp_avg_sq)
        assert int(oa.step_t) == int(ob.step_t) == 3


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
                     max_buffer_size=10**6, env_horizon=cfg.horizon, noise_beta=0.0).items():
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


def test_agent_on_the_engine_plans_before_and_after_updates_and_sees_loaded_weights(monkeypatch):
    from tdmpc_amd.drnn_icem import TdIcemDrnn
    from tdmpc_amd.dssm_engine import DssmEngineLearner
    monkeypatch.delenv("TDMPC_DSSM_LEARNER_ENGINE", raising=False)
    cfg = _small_planner_cfg()
    H = cfg.horizon
    rs = np.random.RandomState(5)
    agent = TdIcemDrnn(cfg, graph=True, engine=True)
    agent.model.load_state_dict(U.synthetic_dssm_state_dict(cfg, 31))
    agent.model_target.load_state_dict(U.synthetic_dssm_state_dict(cfg, 32))
    buf = _filled_buffer(cfg, rs)
    obs = rs.standard_normal(cfg.obs_shape[0]).astype(np.float32)
    hidden = np.zeros((1, cfg.hidden_dim), np.float32)

    def plan(ag):
        torch.manual_seed(11)
        np.random.seed(12)
        return ag.plan(obs, hidden, step=30000, t0=True)[0]
    a0 = plan(agent)                                                     # a pack made before the learner exists
    assert agent._learner is None and agent.explore_coef == 0            # planning built no learner
    for k in range(5):
        m = agent.update(buf, 20000 + k)
        assert not agent.model.training
        _nbt(agent.model, H, k + 1)
    assert set(m) == {"consistency_loss", "reward_loss", "value_loss", "pi_loss", "total_loss", "weighted_loss",
                      "grad_norm", "intrinsic_batch_reward_mean", "current_explore_coef", "mixture_coef"}
    assert all(isinstance(v, float) and np.isfinite(v) for v in m.values()), m
    assert m["current_explore_coef"] == agent.explore_coef > 0
    learner = agent.learner
    eng = learner.engine
    assert isinstance(learner, DssmEngineLearner) and learner.path == "engine"
    assert learner._graphs, "the learner never replayed its captured graph"
    assert agent.reward_rms.count == pytest.approx(5 + 1e-4)
    assert agent.optim is eng.opt_main and agent.pi_optim is eng.opt_pi
    # the plan after the updates runs on the new weights: a fresh agent on the state_dict plans the same
    a1 = plan(agent)
    assert not torch.equal(a0, a1)
    fresh = TdIcemDrnn(cfg, graph=False)
    fresh.model.load_state_dict(U.synthetic_dssm_state_dict(cfg, 31))
    assert torch.equal(plan(fresh), a0)
    fresh.model.load_state_dict(agent.model.state_dict())
    fresh.std = agent.std
    assert torch.equal(plan(fresh), a1)
    assert fresh._learner is None
    t = agent.update(buf, 20005, sync_metrics=False)
    assert torch.is_tensor(t["total_loss"]) and t["total_loss"].is_cuda and t["total_loss"].dim() == 0
    # load_state_dict after the engine exists lands in the flat buffer; the next update and plan start from it
    sd = U.synthetic_dssm_state_dict(cfg, 77)
    agent.model.load_state_dict(sd)
    lo, hi = eng.P.data_ptr(), eng.P.data_ptr() + 4 * eng.P.numel()
    for k, p in agent.model.named_parameters():
        assert lo <= p.data_ptr() < hi and torch.equal(eng.wv(k), sd[k].cuda()), k
    fresh.model.load_state_dict(sd)
    assert torch.equal(plan(agent), plan(fresh))
    agent.update(buf, 20006)
    for k in ("_dynamics.gru_cell.weight_hh.weight", "_dynamics.prior_mlp.0.weight", "_encoder.0.weight",
              "_predictor.3.weight", "_Q1.0.weight", "_reward.0.weight"):
        d = float((agent.model.state_dict()[k] - sd[k].cuda()).abs().max())
        assert 0 < d <= 10 * cfg.lr, (k, d)


def test_the_environment_variable_alone_selects_the_engine_for_the_icem_agent_only(monkeypatch):
    from tdmpc_amd.drnn import TdMpcDrnn
    from tdmpc_amd.drnn_icem import TdIcemDrnn
    from tdmpc_amd.drnn_learner import DssmLearner, DssmSimLearner
    from tdmpc_amd.dssm_engine import DssmEngineLearner
    cfg = _small_planner_cfg()
    monkeypatch.delenv("TDMPC_DSSM_LEARNER_ENGINE", raising=False)
    stock = TdIcemDrnn(cfg, graph=False)
    assert type(stock.learner) is DssmLearner and isinstance(stock.optim, torch.optim.Adam)
    monkeypatch.setenv("TDMPC_DSSM_LEARNER_ENGINE", "1")
    agent = TdIcemDrnn(cfg, graph=False)
    assert agent._learner is None
    learner = agent.learner
    assert type(learner) is DssmEngineLearner and learner.path == "engine"
    assert agent.optim is learner.engine.opt_main and agent.pi_optim is learner.engine.opt_pi
    m = agent.update(_filled_buffer(cfg, np.random.RandomState(6)), 20000)
    assert np.isfinite(m["total_loss"]) and np.isfinite(m["intrinsic_batch_reward_mean"])
    cfg2 = _small_planner_cfg()
    cfg2.warmup_len = 1
    mpc = TdMpcDrnn(cfg2, graph=False)
    assert type(mpc.learner) is DssmSimLearner and isinstance(mpc.optim, torch.optim.Adam)
