"""CPU: the MLP iCEM agent's model and update.

  * `IcemMlpModel`'s state_dict == the reference model's recorded names, shapes and order
    (tests/golden/icem_mlp_layout.json); a synthetic state dict loads strictly; a `TdIcemMlp` checkpoint reloads bit for
    bit and a state dict without `_predictor.3.bias` is refused by name.
  * tests/icem_update_ref.py in float32 == tests/golden/icem_update/*.npz (the reference's `TdICemSimMlp.update` run by
    tests/golden/make_icem_update_golden.py): metrics, priorities, intrinsic rewards, the RunningMeanStd state, every
    .grad and every tensor of model and target after each of two consecutive updates, as exact equality of the
    recording's arrays.
  * `IcemMlpLearner` on a CPU model (its PyTorch path) and `TdIcemMlp.update` == the yardstick, to the same standard.
  * the learner's refusals name their setting, and a refused cfg still constructs an agent.
  * the new entry points refuse null pointers and inadmissible shapes without a device.
"""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import icem_update_ref as U
from tdmpc_amd import _lib
from tdmpc_amd.config import make_cfg

E_DIMS = -1
FAKE = 0x10000   # a non-null address that a refused call never reads
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

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


# ---------------------------------------------------------------------------------------------------------------------
# model, layout, checkpoint
# ---------------------------------------------------------------------------------------------------------------------
def test_model_layout_equals_the_recorded_reference_layout():
    from tdmpc_amd.icem_mlp import IcemMlpModel, synthetic_icem_mlp_state_dict
    lay = json.load(open(os.path.join(GOLD, "icem_mlp_layout.json")))
    cfg = make_cfg("humanoid")
    model = IcemMlpModel(cfg)
    assert [(k, list(v.shape)) for k, v in model.state_dict().items()] == list(lay.items())
    assert "_predictor.1.num_batches_tracked" in lay and lay["_predictor.3.bias"] == [cfg.latent_dim]
    sd = synthetic_icem_mlp_state_dict(cfg, 7)
    model.load_state_dict(sd)                                             # strict
    for k in ("_reward.4.weight", "_Q1.6.weight", "_Q2.6.weight"):       # the zero-initialised last layers
        assert float(sd[k].abs().max()) > 0
    assert float(sd["_predictor.1.running_mean"].abs().max()) > 0 and float(sd["_predictor.1.running_var"].min()) >= 0.5
    assert not torch.equal(sd["_predictor.1.running_var"], torch.ones_like(sd["_predictor.1.running_var"]))
    z = torch.randn(3, cfg.latent_dim)
    assert model.eval().pred_z(z).shape == (3, cfg.latent_dim)
    model.track_model_grad(False)
    assert not model._dynamics[0].weight.requires_grad and model._pi[0].weight.requires_grad


def test_seeded_reference_init_equals_the_recorded_reference_models():
    """The modules are built and initialised in the reference's order, so a seeded construction consumes torch's
    generator as the reference's does."""
    from tdmpc_amd.icem_mlp import IcemMlpModel
    g = np.load(os.path.join(U.GOLD_DIR, "init.npz"))
    torch.manual_seed(U.INIT_SEED)
    s, ss, pr = U.summarize(IcemMlpModel(U.case_cfg("tiny")).state_dict())
    _same("sum", s, g["sum"])
    _same("sumsq", ss, g["sumsq"])
    _same("probe", pr, g["probe"])


def test_reference_init_zeroes_the_last_layers_and_is_orthogonal():
    from tdmpc_amd.icem_mlp import IcemMlpModel
    torch.manual_seed(0)
    m = IcemMlpModel(make_cfg("cheetah"))
    for head in (m._reward, m._Q1, m._Q2):
        assert not head[-1].weight.any() and not head[-1].bias.any()
    w = m._predictor[0].weight.double()                                   # [512, 50]: orthonormal columns
    assert torch.allclose(w.T @ w, torch.eye(w.shape[1], dtype=torch.float64), atol=1e-5)
    assert not m._predictor[0].bias.any() and int(m._predictor[1].num_batches_tracked) == 0


class _StubPlanner:
    """What `TdIcemMlp` asks of its planner when it only learns (the real one needs the GPU)."""
    _packed_key = "packed"
    pmax, E_max, elites = 1, 0, None

    def __init__(self, *a, **k):
        pass


def _cpu_agent(monkeypatch, name="tiny", **over):
    from tdmpc_amd import icem_mlp
    monkeypatch.setattr(icem_mlp, "IcemMlpPlanner", _StubPlanner)
    cfg = U.case_cfg(name)
    cfg.device = "cpu"
    for k, v in over.items():
        setattr(cfg, k, v)
    agent = icem_mlp.TdIcemMlp(cfg, graph=False)
    if getattr(cfg, "normalize", True):
        agent.model.load_state_dict(icem_mlp.synthetic_icem_mlp_state_dict(cfg, U.CASES[name][4]))
        agent.model_target.load_state_dict(icem_mlp.synthetic_icem_mlp_state_dict(cfg, U.CASES[name][5]))
    return cfg, agent


def test_checkpoint_round_trip_and_a_predictorless_state_dict_is_refused(monkeypatch, tmp_path):
    cfg, agent = _cpu_agent(monkeypatch)
    fp = str(tmp_path / "agent.pt")
    agent.save(fp)
    _, other = _cpu_agent(monkeypatch)
    with torch.no_grad():
        for p in list(other.model.parameters()) + list(other.model_target.parameters()):
            p.add_(1.0)
    other.load(fp)
    for a, b in ((agent.model, other.model), (agent.model_target, other.model_target)):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        for k in sa:
            assert torch.equal(sa[k], sb[k]), k
    d = torch.load(fp, weights_only=True)
    assert set(d) == {"model", "model_target"}
    del d["model"]["_predictor.3.bias"]
    torch.save(d, fp)
    with pytest.raises(RuntimeError, match=r"_predictor\.3\.bias"):
        other.load(fp)
    # TdICEM keeps its predictor-less model: a TOLD state dict loads strictly there and not here
    from tdmpc_amd.told import synthetic_state_dict
    with pytest.raises(RuntimeError, match="_predictor"):
        agent.model.load_state_dict(synthetic_state_dict(cfg, 1, enc_norm=True))


# ---------------------------------------------------------------------------------------------------------------------
# the update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.RECORDED)
def test_restatement_equals_the_recorded_reference_update_bitwise(name):
    g, agent, res, out = _ref32(name)
    H = U.case_cfg(name).horizon
    for k in range(len(U.STEPS)):
        keys = [key for key in sorted(out) if key.startswith(f"u{k}_")]
        assert len(keys) == 13
        for key in keys:
            _same((name, key), out[key], g[key])
        assert g[f"u{k}_nbt"].tolist() == [1000 + (k + 1) * (H + 2)]
    assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + 2 * (H + 2)


@pytest.mark.parametrize("name", U.RECORDED)
def test_the_makers_tie_guard_holds_on_the_committed_cases(name):
    _, agent, res, _ = _ref32(name)
    assert res[-1]["tie"] > U.TIE, res[-1]["tie"]


def test_rho_shows_in_the_recorded_cases():
    """The cases run at rho = 0.5: with the default 1.0 a missing `rho ** t` would go unseen."""
    assert U.case_cfg("cheetah").rho == 0.5
    cfg = U.case_cfg("tiny")
    agent = U.RefAgent(cfg, "tiny")
    cfg.rho = 1.0
    r = agent.update(U.case_batch("tiny"), U.STEPS[0], U.gold_noise(U.load("tiny"), cfg)[0])
    assert r["metrics"][2] != U.load("tiny")["u0_metrics"][2]


def test_fp32_floors_the_gpu_bounds_are_derived_from():
    """Prints, per case and update, the figures that the float32 CPU run of the yardstick shows against float64 -- the
    noise floors quoted in tests/test_gpu_icem_update.py (FLOORS: the largest over 1, 2, 4 and 8 threads), whose bounds
    are 8 x them -- and holds this run of the float32 yardstick to those bounds."""
    from test_gpu_icem_update import FLOORS, group
    for name in U.CASES:
        cfg, nz = U.case_cfg(name), U.case_noise(name)
        want, scales = U.run_ref(name, torch.float64, nz, scales=True)
        got = U.run_ref(name, torch.float32, nz)
        for k in range(len(U.STEPS)):
            figs = U.figures(got[k], want[k], scales[k], cfg.lr, cfg.tau)
            print(name, "update", k, {c: f"{f:.3e} ({w})" for c, (f, w) in figs.items()})
            over = {c: f for c, (f, _) in figs.items() if not f <= U.bound(FLOORS[(group(name), k)], c, k)}
            assert not over, (name, k, over)


def _cpu_learner(name):
    from tdmpc_amd.icem_learner import IcemMlpLearner
    cfg = U.case_cfg(name)
    model, target = U.make_models(cfg, name)
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cpu"))
    return cfg, agent, IcemMlpLearner(agent, graph=False)


@pytest.mark.parametrize("name", U.RECORDED)
def test_learner_pytorch_path_on_the_cpu_equals_the_restatement_bitwise(name):
    g, ref_agent, res, want = _ref32(name)
    cfg, agent, learner = _cpu_learner(name)
    assert not learner.hip and not learner.graph and learner.train_step is None
    H = cfg.horizon
    buf = U.FakeBuffer(U.case_batch(name))
    noise = U.gold_noise(g, cfg)
    got = {}
    for k, step in enumerate(U.STEPS):
        m, coef = learner.update(buf, step, noise[k])
        assert not agent.model.training
        r = dict(metrics=np.array(m.tolist() + [coef], dtype=np.float64), prio=buf.prios[-1].numpy(),
                 intrinsic=learner.last["intrinsic"].numpy(), rms=learner.rms.numpy().copy(),
                 grads=U.grads_of(agent.model))
        U.record(got, k, r, agent.model, agent.model_target)
        assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + (k + 1) * (H + 2)
    for key in sorted(want):
        _same((name, key), got[key], want[key])
    rms = learner.reward_rms
    assert (rms.mean, rms.var, rms.count) == tuple(res[-1]["rms"])


def test_agent_update_on_the_cpu_equals_the_restatement_bitwise(monkeypatch):
    from tdmpc_amd.config import linear_schedule
    from tdmpc_amd.icem_learner import IcemMlpLearner
    g, _, res, want = _ref32("tiny")
    cfg, agent = _cpu_agent(monkeypatch)
    assert agent._learner is None and "_optim" not in agent.__dict__     # a plan-only agent has built no learner
    assert agent.explore_coef == 0
    buf = U.FakeBuffer(U.case_batch("tiny"))
    noise = U.gold_noise(g, cfg)
    got = {}
    for k, step in enumerate(U.STEPS):
        agent.planner._packed_key = "packed"
        m = agent.update(buf, step, noise=noise[k])
        assert set(m) == {"consistency_loss", "reward_loss", "value_loss", "pi_loss", "total_loss", "weighted_loss",
                          "grad_norm", "intrinsic_batch_reward_mean", "current_explore_coef", "mixture_coef"}
        assert all(isinstance(v, float) for v in m.values())
        assert m["mixture_coef"] == float(g[f"u{k}_mixture_coef"]) == agent.mixture_coef
        assert m["current_explore_coef"] == agent.explore_coef == linear_schedule(cfg.explore_schedule, step)
        assert agent.std == linear_schedule(cfg.std_schedule, step)
        assert agent.planner._packed_key is None and not agent.model.training
        r = dict(metrics=np.array([m[n] for n in U.METRICS]), prio=buf.prios[-1].numpy(),
                 intrinsic=agent.learner.last["intrinsic"].numpy(), rms=agent.learner.rms.numpy().copy(),
                 grads=U.grads_of(agent.model))
        U.record(got, k, r, agent.model, agent.model_target)
    for key in sorted(want):
        _same(key, got[key], want[key])
    assert isinstance(agent.learner, IcemMlpLearner) and isinstance(agent.optim, torch.optim.Adam)
    assert isinstance(agent.pi_optim, torch.optim.Adam) and agent.reward_rms.count == res[-1]["rms"][2]
    zs = [torch.zeros(cfg.batch_size, cfg.latent_dim) for _ in range(2)]
    agent.planner._packed_key = "packed"
    assert np.isfinite(agent.update_pi(zs)) and agent.planner._packed_key is None


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
REFUSED = [
    (dict(batch_size=2048, horizon=5), ValueError, r"batch_size=2048"),       # 12288 rows
    (dict(batch_size=1), ValueError, r"batch_size=1 "),
    (dict(latent_dim=257), ValueError, r"latent_dim=257"),
    (dict(mlp_dim=256), ValueError, r"mlp_dim=256"),
    (dict(modality="pixels"), NotImplementedError, r"modality='pixels'"),
    (dict(normalize=False), NotImplementedError, r"normalize=False"),
    (dict(norm_type="bn"), NotImplementedError, r"norm_type='bn'"),
    (dict(optim_id="sgd"), ValueError, r"optim_id='sgd'"),
]


@pytest.mark.parametrize("over,exc,match", REFUSED, ids=[next(iter(o)) + "=" + str(next(iter(o.values()))) for o, _, _ in REFUSED])
def test_learner_refusals_name_the_setting_and_need_no_device(over, exc, match):
    from tdmpc_amd.icem_learner import IcemMlpLearner, check_icem_learner_cfg
    cfg = make_cfg("cheetah", **over)
    with pytest.raises(exc, match=match):
        check_icem_learner_cfg(cfg)
    agent = SimpleNamespace(cfg=cfg, model=None, model_target=None, device=torch.device("cpu"))
    with pytest.raises(exc, match=match):
        IcemMlpLearner(agent)                                              # before it looks at the model


def test_the_reference_task_cfgs_are_admitted():
    from tdmpc_amd.icem_learner import check_icem_learner_cfg
    for task in ("cartpole", "cheetah", "humanoid"):
        check_icem_learner_cfg(make_cfg(task))                            # humanoid: 6 * 512 = 3072 rows
    check_icem_learner_cfg(make_cfg("humanoid", latent_dim=256, optim_id="adam"))


@pytest.mark.parametrize("over,match", [(dict(batch_size=2048, horizon=5), "4096"), (dict(normalize=False), "normalize"),
                                        (dict(optim_id="sgd"), "optim_id")])
def test_an_agent_whose_cfg_the_learner_refuses_still_constructs(monkeypatch, over, match):
    cfg, agent = _cpu_agent(monkeypatch, **over)
    assert agent._learner is None and agent.plan_horizon == 1
    assert ("_predictor.1.weight" in agent.model.state_dict()) == getattr(cfg, "normalize", True)
    with pytest.raises((ValueError, NotImplementedError), match=match):
        agent.update(U.FakeBuffer(U.case_batch("tiny")), U.STEPS[0])
    with pytest.raises((ValueError, NotImplementedError), match=match):
        agent.optim
    assert agent._learner is None


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
def _dims(**kw):
    d = _lib.dims_from_cfg(make_cfg("humanoid"), enc_norm=True)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _intrinsic(d, S, B, z=FAKE, n_dyn=6):
    t6, t8 = (C.c_void_p * 6)(*([FAKE] * 6)), (C.c_void_p * 8)(*([FAKE] * 8))
    return _lib.lib().tdmpc_icem_intrinsic_fwd(C.byref(d), t6, n_dyn, t8, 8, z, FAKE, FAKE, S, B, FAKE, FAKE, 1 << 40,
                                               None)


def _simloss(d, rows):
    L, t8 = _lib.lib(), (C.c_void_p * 8)(*([FAKE] * 8))
    return (L.tdmpc_icem_simloss_fwd(C.byref(d), t8, 8, FAKE, FAKE, rows, FAKE, FAKE, 1 << 40, FAKE, 1 << 40, None),
            L.tdmpc_icem_simloss_bwd(C.byref(d), t8, 8, FAKE, FAKE, rows, FAKE, 1 << 40, FAKE, FAKE, t8, FAKE, 1 << 40,
                                     None))


@pytest.mark.parametrize("what,dims,S,B", [
    ("one row per segment", {}, 4, 1), ("no segment", {}, 0, 33), ("4097 rows", {}, 241, 17),
    ("latent 257", dict(latent_dim=257), 4, 33), ("mlp_dim 256", dict(mlp_dim=256), 4, 33),
    ("pixels", dict(modality=1), 4, 33), ("no action", dict(action_dim=0), 4, 33)])
def test_new_entry_points_refuse_inadmissible_shapes_without_a_device(what, dims, S, B):
    d, L = _dims(**dims), _lib.lib()
    n = C.c_size_t(12345)
    assert L.tdmpc_icem_intrinsic_workspace_floats(C.byref(d), S, B, C.byref(n)) == E_DIMS and n.value == 12345, what
    assert _intrinsic(d, S, B) == E_DIMS and L.tdmpc_last_error(), what
    rows = S * B
    sz = _lib.IcemSimlossSizes()
    assert L.tdmpc_icem_simloss_sizes_for(C.byref(d), rows if dims or rows > 4096 else 1, C.byref(sz)) == E_DIMS, what
    assert _simloss(d, rows if dims or rows > 4096 else 1) == (E_DIMS, E_DIMS), what


def test_new_entry_points_refuse_null_pointers_without_a_device():
    d, L = _dims(), _lib.lib()
    n = C.c_size_t()
    assert L.tdmpc_icem_intrinsic_workspace_floats(C.byref(d), 6, 512, C.byref(n)) == 0 and n.value > 0
    assert L.tdmpc_icem_intrinsic_workspace_floats(None, 6, 512, C.byref(n)) == E_DIMS
    assert L.tdmpc_icem_intrinsic_workspace_floats(C.byref(d), 6, 512, None) == E_DIMS
    assert _intrinsic(d, 6, 512, z=None) == E_DIMS and b"z is null" in L.tdmpc_last_error()
    assert _intrinsic(d, 6, 512, n_dyn=5) == E_DIMS and b"dynamics tensors" in L.tdmpc_last_error()
    t6, t8 = (C.c_void_p * 6)(*([FAKE] * 5 + [None])), (C.c_void_p * 8)(*([FAKE] * 8))
    assert L.tdmpc_icem_intrinsic_fwd(C.byref(d), t6, 6, t8, 8, FAKE, FAKE, FAKE, 6, 512, FAKE, FAKE, 1 << 40,
                                      None) == E_DIMS
    sz = _lib.IcemSimlossSizes()
    assert L.tdmpc_icem_simloss_sizes_for(C.byref(d), 2560, C.byref(sz)) == 0
    ds = _lib.DrnnTrainSizes()                                            # the same internals as the DSSM entry points
    from drnn_io import drnn_cfg
    assert L.tdmpc_drnn_train_sizes_for(C.byref(_lib.drnn_dims_from_cfg(drnn_cfg("humanoid"))), 2560, C.byref(ds)) == 0
    assert sz.loss_saved_floats == ds.loss_saved_floats and 0 < sz.workspace_floats <= ds.workspace_floats
    assert L.tdmpc_icem_simloss_fwd(C.byref(d), t8, 8, None, FAKE, 64, FAKE, FAKE, 1 << 40, FAKE, 1 << 40,
                                    None) == E_DIMS and b"queries is null" in L.tdmpc_last_error()
    assert L.tdmpc_icem_simloss_bwd(C.byref(d), t8, 8, FAKE, FAKE, 64, FAKE, 1 << 40, None, FAKE, t8, FAKE, 1 << 40,
                                    None) == E_DIMS and b"dloss is null" in L.tdmpc_last_error()
    a = _lib.IcemLossArgs()
    assert L.tdmpc_icem_loss_forward(C.byref(a), FAKE, FAKE, FAKE, None) == E_DIMS
    assert L.tdmpc_icem_loss_backward(C.byref(a), FAKE, FAKE, FAKE, FAKE, None, None, None, None, None) == E_DIMS
    for f in ("sim", "q1", "q2", "rp", "rw", "rwpi", "nq", "w"):
        setattr(a, f, FAKE)
    a.H, a.B = 3, 0
    assert L.tdmpc_icem_loss_forward(C.byref(a), FAKE, FAKE, FAKE, None) == E_DIMS
    a.B = 33
    assert L.tdmpc_icem_loss_forward(C.byref(a), None, FAKE, FAKE, None) == E_DIMS
    assert L.tdmpc_icem_loss_backward(C.byref(a), FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE, None) == E_DIMS


def test_version_numbers():
    L = _lib.lib()
    assert L.tdmpc_icem_learner_version() == 1 == _lib.ICEM_LEARNER_VERSION
    assert L.tdmpc_drnn_train_version() == 1 == _lib.DRNN_TRAIN_VERSION
    assert L.tdmpc_drnn_version() == 2 == _lib.DRNN_VERSION
    assert L.tdmpc_abi_version() == 8 == _lib.ABI_VERSION
    assert _lib.ICEM_DYN_TENSORS == 6
