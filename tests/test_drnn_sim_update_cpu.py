"""CPU: the MPC DSSM agent's update -- the yardstick against the recorded reference run, `DssmSimLearner`'s PyTorch
path against the yardstick, both bit for bit; the refusals; the new ABI entry points without a device.

  * tests/drnn_sim_update_ref.py in float32 == tests/golden/drnn_sim_update/*.npz (the reference's
    `TdMpcSimDssm.update` run by tests/golden/make_drnn_sim_update_golden.py): metrics, priorities, intrinsic rewards,
    the RunningMeanStd state, every .grad and every tensor of model and target after each of two consecutive updates,
    as exact equality of the recording's arrays (float64 sum, sum of squares and 64 fixed elements per tensor).
  * `tdmpc_amd.drnn_learner.DssmSimLearner` on a CPU model (its PyTorch path) == the yardstick, to the same standard.
  * num_batches_tracked moves by 2H + 1 (prior_mlp) and H + 3 - W (_predictor) per update.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import drnn_sim_update_ref as U
from drnn_io import drnn_cfg
from tdmpc_amd import _lib

E_DIMS = -1
FAKE = 0x10000   # a non-null address that a refused call never reads

_RUN = {}


def _ref32(name):
    """The yardstick's float32 run on the recording's draws, once per case."""
    if name not in _RUN:
        g = U.load(name)
        _RUN[name] = (g,) + U.run_case(name, torch.float32, U.gold_noise(g, U.case_cfg(name)))
    return _RUN[name]


def _same(tag, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.array_equal(got, want), (tag, float(np.abs(got.astype(np.float64) - want).max()))


def _nbt(cfg, k):
    H, W = cfg.horizon, cfg.warmup_len
    return [1000 + (k + 1) * (2 * H + 1), 1000 + (k + 1) * (H + 3 - W)]


@pytest.mark.parametrize("name", U.RECORDED)
def test_restatement_equals_the_recorded_reference_update_bitwise(name):
    g, agent, res, out = _ref32(name)
    cfg = U.case_cfg(name)
    for k in range(len(U.STEPS)):
        keys = [key for key in sorted(out) if key.startswith(f"u{k}_")]
        assert len(keys) == 13
        for key in keys:
            _same((name, key), out[key], g[key])
        assert g[f"u{k}_nbt"].tolist() == _nbt(cfg, k)
        assert g[f"u{k}_noise"].shape[0] == 2 * (cfg.horizon - cfg.warmup_len) + 1
        assert g[f"u{k}_aug"].shape == (cfg.horizon, cfg.batch_size, cfg.latent_dim)
    assert [int(agent.model._dynamics.prior_mlp[1].num_batches_tracked),
            int(agent.model._predictor[1].num_batches_tracked)] == _nbt(cfg, 1)
    # the warm-up rows of the intrinsic rewards are the reference's zeros, and the rest is not
    W = cfg.warmup_len
    assert not g["u0_intrinsic"][:W].any() and g["u0_intrinsic"][W:].any()


@pytest.mark.parametrize("name", list(U.CASES))
def test_the_makers_tie_guard_holds_on_every_case(name):
    """Every row of both update_pi calls and of every TD target has |Q1 - Q2| > 1e-4 (1 + |min Q|)."""
    if name in U.RECORDED:
        res = _ref32(name)[2]
    else:
        res = U.run_case(name, torch.float32)[1]
    assert res[-1]["tie"] > U.TIE, res[-1]["tie"]


def test_fp32_floors_the_gpu_bounds_are_derived_from():
    """Prints, per case, update and CPU thread count (test_gpu_drnn_sim_update.THREADS: the summation order of the
    CPU's products moves with it), the figures (drnn_update_ref.figures) that the float32 CPU run of the yardstick shows
    against float64 -- the noise floors quoted in tests/test_gpu_drnn_sim_update.py (FLOORS) are their maxima, the
    bounds 8 x them -- and holds the float32 yardstick itself to those bounds."""
    from test_gpu_drnn_sim_update import FLOORS, THREADS, group
    threads = torch.get_num_threads()
    try:
        for name in U.CASES:
            cfg, nz = U.case_cfg(name), U.case_noise(name)
            want, scales = U.run_ref(name, torch.float64, nz, scales=True)
            for t in THREADS:
                torch.set_num_threads(t)
                got = U.run_ref(name, torch.float32, nz)
                for k in range(len(U.STEPS)):
                    figs = U.figures(got[k], want[k], scales[k], cfg.lr, cfg.tau)
                    print(name, "threads", t, "update", k, {c: f"{f:.3e} ({w})" for c, (f, w) in figs.items()})
                    over = {c: f for c, (f, _) in figs.items() if not f <= U.bound(FLOORS[(group(name), k)], c, k)}
                    assert not over, (name, t, k, over)
    finally:
        torch.set_num_threads(threads)


def _cpu_learner(name):
    from tdmpc_amd.drnn_learner import DssmSimLearner
    cfg = U.case_cfg(name)
    model, target = U.make_models(cfg, name)
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cpu"))
    return cfg, agent, DssmSimLearner(agent, graph=False)


@pytest.mark.parametrize("name", U.RECORDED)
def test_learner_pytorch_path_on_the_cpu_equals_the_restatement_bitwise(name):
    g, ref_agent, res, want = _ref32(name)
    cfg, agent, learner = _cpu_learner(name)
    assert not learner.hip and not learner.graph
    buf = U.FakeBuffer(U.case_batch(name))
    noise = U.gold_noise(g, cfg)
    got = {}
    for k, step in enumerate(U.STEPS):
        m, coef = learner.update(buf, step, noise[k])
        assert not agent.model.training
        r = dict(metrics=np.array(m.tolist(), dtype=np.float64), prio=buf.prios[-1].numpy(),
                 intrinsic=learner.last["intrinsic"].numpy(), rms=learner.rms.numpy().copy(),
                 grads=U.grads_of(agent.model))
        U.record(got, k, r, agent.model, agent.model_target)
        assert [int(agent.model._dynamics.prior_mlp[1].num_batches_tracked),
                int(agent.model._predictor[1].num_batches_tracked)] == _nbt(cfg, k)
    for key in sorted(want):
        _same((name, key), got[key], want[key])
    rms = learner.reward_rms
    assert (rms.mean, rms.var, rms.count) == tuple(res[-1]["rms"])


def test_learner_refusals_name_the_setting_and_need_no_device():
    from tdmpc_amd.drnn_learner import DssmSimLearner, check_sim_learner_cfg
    ok = dict(horizon=5, warmup_len=2)
    check_sim_learner_cfg(drnn_cfg("humanoid", **ok))                       # 6 * 512 = 3072 rows
    for W in (0, 5):
        with pytest.raises(ValueError, match=f"warmup_len={W} "):
            check_sim_learner_cfg(drnn_cfg("cheetah", horizon=5, warmup_len=W))
    with pytest.raises(NotImplementedError, match="similarity_horizon=2 "):
        check_sim_learner_cfg(drnn_cfg("cheetah", similarity_horizon=2, **ok))
    with pytest.raises(ValueError, match="batch_size"):
        check_sim_learner_cfg(drnn_cfg("dog", **ok))                         # batch_size 2048: 12288 rows
    with pytest.raises(ValueError, match="batch_size=1 "):
        check_sim_learner_cfg(drnn_cfg("cheetah", batch_size=1, **ok))
    for cfg, exc in ((drnn_cfg("dog", **ok), ValueError), (drnn_cfg("cheetah", horizon=5, warmup_len=0), ValueError),
                     (drnn_cfg("cheetah", similarity_horizon=2, **ok), NotImplementedError)):
        agent = SimpleNamespace(cfg=cfg, model=None, model_target=None, device=torch.device("cpu"))
        with pytest.raises(exc):
            DssmSimLearner(agent)                                            # before it looks at the model


def _dims(**kw):
    d = _lib.drnn_dims_from_cfg(drnn_cfg("humanoid"))
    for k, v in kw.items():
        setattr(d.base, k, v)
    return d


def _chain(d, S, B, warm, mode=0, z=FAKE, h_out=FAKE):
    t22, t8 = (C.c_void_p * 22)(*([FAKE] * 22)), (C.c_void_p * 8)(*([FAKE] * 8))
    return _lib.lib().tdmpc_drnn_intrinsic_chain_fwd(C.byref(d), t22, 22, t8, 8, z, FAKE, FAKE, S, B, warm, mode, FAKE,
                                                     h_out, FAKE, 1 << 40, None)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("what,S,B,warm", [
    ("warm = S", 4, 33, 4), ("warm > S", 4, 33, 7), ("warm < 0", 4, 33, -1), ("one row per segment", 4, 1, 1),
    ("4097 rows", 241, 17, 1)])
def test_chain_fwd_refuses_unsupported_calls_without_a_device(what, S, B, warm, mode):
    d, L = _dims(), _lib.lib()
    assert _chain(d, S, B, warm, mode) == E_DIMS and L.tdmpc_last_error(), what


def test_new_entry_points_refuse_null_pointers_without_a_device():
    d, L = _dims(), _lib.lib()
    n = C.c_size_t()
    assert L.tdmpc_drnn_intrinsic_chain_workspace_floats(C.byref(d), 6, 512, C.byref(n)) == 0 and n.value > 0
    assert L.tdmpc_drnn_intrinsic_chain_workspace_floats(C.byref(d), 6, 512, None) == E_DIMS
    assert L.tdmpc_drnn_intrinsic_chain_workspace_floats(C.byref(d), 241, 17, C.byref(n)) == E_DIMS
    assert L.tdmpc_drnn_intrinsic_chain_workspace_floats(C.byref(d), 4, 1, C.byref(n)) == E_DIMS
    assert _chain(d, 6, 512, 2, z=None) == E_DIMS and b"z is null" in L.tdmpc_last_error()
    assert _chain(d, 6, 512, 2, h_out=None) == E_DIMS and b"h_out is null" in L.tdmpc_last_error()
    assert _chain(d, 6, 512, 2, mode=2) == E_DIMS and b"mode" in L.tdmpc_last_error()
    assert _chain(_dims(mlp_dim=256), 6, 512, 2) == E_DIMS
    a = _lib.DrnnSimLossArgs()
    assert L.tdmpc_drnn_sim_loss_forward(C.byref(a), FAKE, FAKE, FAKE, None) == E_DIMS
    assert L.tdmpc_drnn_sim_loss_backward(C.byref(a), FAKE, FAKE, FAKE, FAKE, None, None, None, None, None) == E_DIMS
    for f in ("sim", "q1", "q2", "rp", "rw", "rwpi", "nq", "w"):
        setattr(a, f, FAKE)
    a.H, a.B = 3, 33
    for W in (0, 3):   # warmup_len outside [1, H - 1]
        a.W = W
        assert L.tdmpc_drnn_sim_loss_forward(C.byref(a), FAKE, FAKE, FAKE, None) == E_DIMS, W
    a.W = 1
    assert L.tdmpc_drnn_sim_loss_forward(C.byref(a), None, FAKE, FAKE, None) == E_DIMS
    assert L.tdmpc_drnn_sim_loss_backward(C.byref(a), FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE, None) == E_DIMS


def test_the_pinned_version_numbers_are_unchanged():
    L = _lib.lib()
    assert L.tdmpc_drnn_train_version() == 1 == _lib.DRNN_TRAIN_VERSION
    assert L.tdmpc_drnn_version() == 2 == _lib.DRNN_VERSION
    assert L.tdmpc_abi_version() == 8 == _lib.ABI_VERSION


class _StubPlanner:
    """What `TdMpcDrnn` asks of its planner when it only learns (the real one needs the GPU)."""
    _packed_key = "packed"

    def __init__(self, *a, **k):
        pass


def _cpu_agent(monkeypatch, **over):
    from tdmpc_amd import drnn
    monkeypatch.setattr(drnn, "DrnnPlanner", _StubPlanner)
    cfg = U.case_cfg("tiny")
    cfg.device = "cpu"
    for k, v in over.items():
        setattr(cfg, k, v)
    agent = drnn.TdMpcDrnn(cfg, graph=False)
    agent.model.load_state_dict(U.synthetic_dssm_state_dict(cfg, U.CASES["tiny"][6]))
    agent.model_target.load_state_dict(U.synthetic_dssm_state_dict(cfg, U.CASES["tiny"][7]))
    return cfg, agent


def test_agent_update_on_the_cpu_returns_the_reference_keys_and_values(monkeypatch):
    from tdmpc_amd.config import linear_schedule
    from tdmpc_amd.drnn_learner import DssmSimLearner
    g, _, res, _ = _ref32("tiny")
    cfg, agent = _cpu_agent(monkeypatch)
    assert agent._learner is None and "_optim" not in agent.__dict__     # a plan-only agent has built no learner
    buf = U.FakeBuffer(U.case_batch("tiny"))
    m = agent.update(buf, U.STEPS[0], noise=U.gold_noise(g, cfg)[0])
    assert isinstance(agent.learner, DssmSimLearner) and isinstance(agent.optim, torch.optim.Adam)
    assert set(m) == {"consistency_loss", "reward_loss", "value_loss", "pi_loss", "total_loss", "weighted_loss",
                      "grad_norm", "mixture_coef", "intrinsic_batch_reward_mean"}
    assert all(isinstance(v, float) for v in m.values())
    assert [m[k] for k in U.METRICS] == res[0]["metrics"].tolist()
    assert agent.std == linear_schedule(cfg.std_schedule, U.STEPS[0]) == float(g["u0_std"])
    assert agent.planner._packed_key is None and not agent.model.training
    assert agent.reward_rms.count == 1 + 1e-4
    zs = [torch.zeros(cfg.batch_size, cfg.latent_dim) for _ in range(2)]
    agent.planner._packed_key = "packed"
    assert np.isfinite(agent.update_pi(zs)) and agent.planner._packed_key is None


def test_an_agent_whose_cfg_the_learner_refuses_still_constructs(monkeypatch):
    cfg, agent = _cpu_agent(monkeypatch, warmup_len=0)     # cfgs/default.yaml's value
    assert agent._learner is None and len(agent._memories) == 1
    with pytest.raises(ValueError, match="warmup_len=0 "):
        agent.update(U.FakeBuffer(U.case_batch("tiny")), U.STEPS[0])
    with pytest.raises(ValueError, match="warmup_len=0 "):
        agent.optim
