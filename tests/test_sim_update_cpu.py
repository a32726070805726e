"""CPU: the similarity TD-MPC agent's model and update (tdmpc_amd/tdmpc_sim.py, sim_learner.py).

  * `TdMpcSim`'s model state_dict == the reference `TDMPCSIM` model's recorded names, shapes and order
    (tests/golden/tdmpc_sim_layout.json); a reference-layout checkpoint (`{'model', 'model_target'}`) loads strictly;
    the planner's packed tensor list is exactly TOLD's.
  * tests/sim_update_ref.py in float32 == tests/golden/sim_update/*.npz (the reference's `TDMPCSIM.update` run by
    tests/golden/make_sim_update_golden.py): metrics, priorities, the BatchNorm's buffers, every .grad and every tensor of
    model and target after each of two consecutive updates, as exact equality of the recording's arrays.
  * `SimLearner`'s PyTorch path on a CPU model and `TdMpcSim.update` == the yardstick, to the same standard;
    num_batches_tracked moves by 1 per update.
  * refusals name their setting, and a refused cfg still constructs an agent.
  * the new entry points refuse null pointers and inadmissible shapes without a device.
"""
import ctypes as C
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import sim_update_ref as U
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


class _StubPlanner:
    """What `TdMpcSim` asks of its planner when it only learns (the real one needs the GPU)."""
    _packed_key = "packed"

    def __init__(self, *a, **k):
        pass


def _cpu_agent(monkeypatch, name="tiny", **over):
    from tdmpc_amd import tdmpc_sim
    from tdmpc_amd.icem_mlp import synthetic_icem_mlp_state_dict
    monkeypatch.setattr(tdmpc_sim, "SimPlanner", _StubPlanner)
    cfg = U.case_cfg(name)
    cfg.device = "cpu"
    for k, v in over.items():
        setattr(cfg, k, v)
    if cfg.modality == "pixels":
        cfg.obs_shape = (3 * cfg.frame_stack, cfg.img_size, cfg.img_size)
    agent = tdmpc_sim.TdMpcSim(cfg, graph=False)
    if getattr(cfg, "normalize", True) and cfg.modality == "state":
        agent.model.load_state_dict(synthetic_icem_mlp_state_dict(cfg, U.CASES[name][4]))
        agent.model_target.load_state_dict(synthetic_icem_mlp_state_dict(cfg, U.CASES[name][5]))
    return cfg, agent


# ---------------------------------------------------------------------------------------------------------------------
# model, layout, checkpoint, packing
# ---------------------------------------------------------------------------------------------------------------------
def test_model_layout_equals_the_recorded_reference_layout(monkeypatch):
    lay = json.load(open(os.path.join(GOLD, "tdmpc_sim_layout.json")))
    from tdmpc_amd import tdmpc_sim
    monkeypatch.setattr(tdmpc_sim, "SimPlanner", _StubPlanner)
    cfg = make_cfg("humanoid")
    cfg.device = "cpu"
    agent = tdmpc_sim.TdMpcSim(cfg, graph=False)
    for model in (agent.model, agent.model_target):
        assert [(k, list(v.shape)) for k, v in model.state_dict().items()] == list(lay.items())
    keys = list(lay)
    # the reference's TOLD of tdmpc_similarity.py: dynamics, reward, pi, Q1, Q2, encoder, _predictor
    first = [k.split(".")[0] for k in keys]
    assert [m for i, m in enumerate(first) if i == 0 or first[i - 1] != m] == \
        ["_dynamics", "_reward", "_pi", "_Q1", "_Q2", "_encoder", "_predictor"]
    assert lay["_encoder.1.weight"] == [cfg.enc_dim] and lay["_predictor.1.num_batches_tracked"] == []
    assert lay["_predictor.3.bias"] == [cfg.latent_dim]
    assert not agent.model.training and agent.mixture_coef == 0.05 and agent.plan_horizon == 1


def test_a_reference_layout_checkpoint_loads_strictly(monkeypatch, tmp_path):
    """The `{'model', 'model_target'}` dict that `TDMPCSIM.save` writes, built from the recorded layout's names and
    shapes: it loads under strict key matching, model and target, and a checkpoint without the predictor (TDMPC's) or
    with one tensor missing is refused by name."""
    lay = json.load(open(os.path.join(GOLD, "tdmpc_sim_layout.json")))
    from tdmpc_amd import tdmpc_sim
    monkeypatch.setattr(tdmpc_sim, "SimPlanner", _StubPlanner)
    cfg = make_cfg("humanoid")
    cfg.device = "cpu"
    rs = np.random.RandomState(3)

    def sd():
        return {k: (torch.tensor(7, dtype=torch.int64) if k.endswith("num_batches_tracked")
                    else torch.from_numpy(rs.standard_normal(shape).astype(np.float32))) for k, shape in lay.items()}
    ckpt = {"model": sd(), "model_target": sd()}
    fp = str(tmp_path / "ref.pt")
    torch.save(ckpt, fp)
    agent = tdmpc_sim.TdMpcSim(cfg, graph=False)
    agent.planner._packed_key = "packed"
    agent.load(fp)
    for part, model in (("model", agent.model), ("model_target", agent.model_target)):
        got = model.state_dict()
        assert list(got) == list(ckpt[part])
        for k in got:
            assert torch.equal(got[k], ckpt[part][k]), (part, k)
    out = str(tmp_path / "out.pt")
    agent.save(out)
    d = torch.load(out, weights_only=True)
    assert set(d) == {"model", "model_target"} and list(d["model"]) == list(lay)
    del d["model_target"]["_predictor.0.weight"]
    torch.save(d, out)
    with pytest.raises(RuntimeError, match=r"_predictor\.0\.weight"):
        agent.load(out)
    from tdmpc_amd.told import synthetic_state_dict
    with pytest.raises(RuntimeError, match="_predictor"):
        agent.model.load_state_dict(synthetic_state_dict(cfg, 1, enc_norm=True))


@pytest.mark.parametrize("normalize", [True, False])
def test_the_planner_packs_exactly_the_told_tensors(normalize):
    """`SimPlanner.pack_tensors` (no device needed): TOLD's names in TOLD's order, the model's own tensors, no
    `_predictor.*` and no integer tensor."""
    from tdmpc_amd.icem_mlp import IcemMlpModel
    from tdmpc_amd.tdmpc_sim import SimPlanner
    from tdmpc_amd.told import TOLD
    cfg = make_cfg("cheetah", normalize=normalize)
    pl = SimPlanner.__new__(SimPlanner)
    pl.cfg = cfg
    dims = pl._make_dims(cfg, 1)
    assert dims.enc_norm == int(normalize) and pl.enc_norm == normalize
    model = IcemMlpModel(cfg)
    told = TOLD(cfg, init="none", enc_norm=normalize).state_dict()
    assert pl.told_keys() == list(told)
    sd = model.state_dict()
    packed = pl.pack_tensors(model)
    assert len(packed) == len(told) == _lib.lib().tdmpc_num_param_tensors(C.byref(dims))
    for t, (k, v) in zip(packed, told.items()):
        assert t.data_ptr() == sd[k].data_ptr() and t.shape == v.shape and t.dtype == torch.float32, k
    ptrs = {t.data_ptr() for t in packed}
    for k, v in sd.items():
        if k.startswith("_predictor."):
            assert v.data_ptr() not in ptrs, k


# ---------------------------------------------------------------------------------------------------------------------
# the update
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.RECORDED)
def test_restatement_equals_the_recorded_reference_update_bitwise(name):
    g, agent, res, out = _ref32(name)
    for k in range(len(U.STEPS)):
        keys = [key for key in sorted(out) if key.startswith(f"u{k}_")]
        assert len(keys) == 14
        for key in keys:
            _same((name, key), out[key], g[key])
        assert g[f"u{k}_nbt"].tolist() == [1000 + (k + 1)]                 # one BatchNorm batch per update
    assert int(agent.model._predictor[1].num_batches_tracked) == 1002
    assert not np.array_equal(g["u0_bn_mean"], g["u1_bn_mean"])


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
    g = U.load("tiny")["u0_metrics"]
    assert r["metrics"][2] != g[2] and r["metrics"][3] != g[3]            # value_loss, pi_loss


def test_the_weighted_loss_is_the_mean_over_the_broadcast():
    """`(total_loss [B, 1] * weights [B]).mean()` is mean(total) mean(w), not the per-sample mean(total_b w_b): the
    recording decides (cheetah, B = 33, weights in [0.5, 1])."""
    g, _, res, _ = _ref32("cheetah")
    w = g["weights"].astype(np.float64)
    total, weighted = g["u0_metrics"][4], g["u0_metrics"][5]
    assert abs(weighted - total * w.mean()) <= 1e-5 * abs(weighted)   # float32 means of 33 and 33 x 33 terms
    assert abs(total * w.mean() - total) > 1e-2 * abs(total)              # the weights matter at this batch


def test_fp32_floors_the_gpu_bounds_are_derived_from():
    """Prints, per case and update, the figures that the float32 CPU run of the yardstick shows against float64 -- the
    noise floors quoted in tests/test_gpu_sim_update.py (FLOORS: the largest over 1, 2, 4 and 8 threads), whose bounds
    are 8 x them -- and holds this run of the float32 yardstick to those bounds."""
    from test_gpu_sim_update import FLOORS, group
    for name in ("cheetah", "tiny", "wide", "h1", "e512", "m256"):
        cfg, nz = U.case_cfg(name), U.case_noise(name)
        want, scales = U.run_ref(name, torch.float64, nz, scales=True)
        got = U.run_ref(name, torch.float32, nz)
        for k in range(len(U.STEPS)):
            figs = U.figures(got[k], want[k], scales[k], cfg.lr, cfg.tau)
            print(name, "update", k, {c: f"{f:.3e} ({w})" for c, (f, w) in figs.items()})
            over = {c: f for c, (f, _) in figs.items() if not f <= U.bound(FLOORS[(group(name), k)], c, k)}
            assert not over, (name, k, over)


def _cpu_learner(name):
    from tdmpc_amd.sim_learner import SimLearner
    cfg = U.case_cfg(name)
    model, target = U.make_models(cfg, name)
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cpu"))
    return cfg, agent, SimLearner(agent, graph=False)


@pytest.mark.parametrize("name", U.RECORDED)
def test_learner_pytorch_path_on_the_cpu_equals_the_restatement_bitwise(name):
    g, ref_agent, res, want = _ref32(name)
    cfg, agent, learner = _cpu_learner(name)
    assert learner.path == "torch" and learner.engine is None and not learner.graph
    assert isinstance(agent.optim, torch.optim.Adam) and agent.pi_optim.param_groups[0]["lr"] == cfg.pi_lr
    buf = U.FakeBuffer(U.case_batch(name))
    noise = U.gold_noise(g, cfg)
    got = {}
    for k, step in enumerate(U.STEPS):
        m = learner.update(buf, step, noise[k])
        assert not agent.model.training
        r = dict(metrics=np.array(m.tolist() + [ref_agent.mixture_coef], dtype=np.float64), prio=buf.prios[-1].numpy(),
                 grads=U.grads_of(agent.model))
        U.record(got, k, r, agent.model, agent.model_target)
        assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + (k + 1)
    for key in sorted(want):
        _same((name, key), got[key], want[key])


def test_agent_update_on_the_cpu_equals_the_restatement_bitwise(monkeypatch):
    from tdmpc_amd.config import linear_schedule
    from tdmpc_amd.sim_learner import SimLearner
    g, _, res, want = _ref32("tiny")
    cfg, agent = _cpu_agent(monkeypatch)
    assert agent._learner is None and "_optim" not in agent.__dict__     # a plan-only agent has built no learner
    buf = U.FakeBuffer(U.case_batch("tiny"))
    noise = U.gold_noise(g, cfg)
    got = {}
    for k, step in enumerate(U.STEPS):
        agent.planner._packed_key = "packed"
        m = agent.update(buf, step, noise=noise[k])
        assert list(m) == list(U.METRICS)                                  # the reference's dict, its keys in order
        assert all(isinstance(v, float) for v in m.values())
        assert m["mixture_coef"] == float(g[f"u{k}_metrics"][7]) == agent.mixture_coef
        assert agent.std == linear_schedule(cfg.std_schedule, step)
        assert agent.planner._packed_key is None and not agent.model.training
        r = dict(metrics=np.array([m[n] for n in U.METRICS]), prio=buf.prios[-1].numpy(), grads=U.grads_of(agent.model))
        U.record(got, k, r, agent.model, agent.model_target)
    for key in sorted(want):
        _same(key, got[key], want[key])
    assert isinstance(agent.learner, SimLearner) and isinstance(agent.optim, torch.optim.Adam)
    assert isinstance(agent.pi_optim, torch.optim.Adam)
    t = agent.update(buf, U.STEPS[1], sync_metrics=False)
    assert torch.is_tensor(t["total_loss"]) and t["total_loss"].dim() == 0 and t["mixture_coef"] == agent.mixture_coef
    zs = [torch.zeros(cfg.batch_size, cfg.latent_dim) for _ in range(2)]
    agent.planner._packed_key = "packed"
    assert np.isfinite(agent.update_pi(zs)) and agent.planner._packed_key is None
    assert set(agent.state_dict()) == {"model", "model_target"}


# ---------------------------------------------------------------------------------------------------------------------
# refusals and admission
# ---------------------------------------------------------------------------------------------------------------------
REFUSED = [
    (dict(modality="pixels"), NotImplementedError, r"modality='pixels'"),
    (dict(normalize=False), NotImplementedError, r"normalize=False"),
    (dict(batch_size=1), ValueError, r"batch_size=1 "),
    (dict(optim_id="sgd"), ValueError, r"optim_id='sgd'"),
]


@pytest.mark.parametrize("over,exc,match", REFUSED, ids=[next(iter(o)) + "=" + str(next(iter(o.values()))) for o, _, _ in REFUSED])
def test_learner_refusals_name_the_setting_and_need_no_device(over, exc, match):
    from tdmpc_amd.sim_learner import SimLearner, check_sim_learner_cfg
    cfg = make_cfg("cheetah", **over)
    with pytest.raises(exc, match=match):
        check_sim_learner_cfg(cfg)
    agent = SimpleNamespace(cfg=cfg, model=None, model_target=None, device=torch.device("cpu"))
    with pytest.raises(exc, match=match):
        SimLearner(agent)                                                  # before it looks at the model


@pytest.mark.parametrize("over,match", [(dict(normalize=False), "normalize=False"),
                                        (dict(modality="pixels"), "modality='pixels'")])
def test_an_agent_whose_cfg_the_learner_refuses_still_constructs(monkeypatch, over, match):
    cfg, agent = _cpu_agent(monkeypatch, **over)
    assert agent._learner is None and agent.plan_horizon == 1
    if not getattr(cfg, "normalize", True):
        sd = agent.model.state_dict()
        assert "_predictor.1.weight" not in sd and "_predictor.4.weight" in sd and "_encoder.2.weight" in sd
    with pytest.raises(NotImplementedError, match=match):
        agent.update(U.FakeBuffer(U.case_batch("tiny")), U.STEPS[0])
    with pytest.raises(NotImplementedError, match=match):
        agent.optim
    assert agent._learner is None


def test_norm_type_bn_is_refused_at_construction(monkeypatch):
    from tdmpc_amd import tdmpc_sim
    monkeypatch.setattr(tdmpc_sim, "SimPlanner", _StubPlanner)
    cfg = make_cfg("cheetah", norm_type="bn")
    cfg.device = "cpu"
    with pytest.raises(NotImplementedError, match=r"norm_type='bn'"):
        tdmpc_sim.TdMpcSim(cfg)


def test_what_the_engine_admits():
    from tdmpc_amd.sim_engine import supported
    for task in ("cartpole", "cheetah", "humanoid"):
        assert supported(make_cfg(task)), task                            # humanoid: 5 * 512 = 2560 rows
    for E in (256, 512, 1024):
        assert supported(make_cfg("cheetah", enc_dim=E))
    assert supported(make_cfg("cheetah", latent_dim=256, optim_id="adam"))
    assert supported(make_cfg("cartpole", horizon=2, batch_size=2048))    # 4096 rows, the cap
    for over in (dict(mlp_dim=256), dict(mlp_dim=1024), dict(enc_dim=128), dict(latent_dim=257), dict(batch_size=1),
                 dict(horizon=2, batch_size=2049), dict(optim_id="sgd"), dict(weight_decay=0.01),
                 dict(normalize=False), dict(norm_type="bn"), dict(modality="pixels")):
        assert not supported(make_cfg("cheetah", **over)), over
    assert not supported(make_cfg("dog"))                                 # 2048 x 5 rows: the PyTorch path


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI without a device
# ---------------------------------------------------------------------------------------------------------------------
def _loss_args(**kw):
    a = _lib.SimLossArgs()
    for f in ("sim", "q1", "q2", "rp", "rw", "td", "w"):
        setattr(a, f, FAKE)
    a.H, a.B, a.rho = 3, 33, 0.5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_loss_entry_points_refuse_null_pointers_and_empty_shapes_without_a_device():
    L = _lib.lib()
    fwd = lambda a, rows=FAKE, scal=FAKE: L.tdmpc_sim_loss_forward(C.byref(a), rows, scal, None)  # noqa: E731
    bwd = lambda a, rows=FAKE, scal=FAKE, gw=FAKE: L.tdmpc_sim_loss_backward(  # noqa: E731
        C.byref(a), rows, scal, gw, None, None, None, None, None)
    assert L.tdmpc_sim_loss_forward(None, FAKE, FAKE, None) == E_DIMS
    assert L.tdmpc_sim_loss_backward(None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None) == E_DIMS
    assert fwd(_lib.SimLossArgs()) == E_DIMS and b"loss_forward" in L.tdmpc_last_error()
    for f in ("sim", "q1", "q2", "rp", "rw", "td", "w"):
        assert fwd(_loss_args(**{f: None})) == E_DIMS and bwd(_loss_args(**{f: None})) == E_DIMS, f
    for kw in (dict(H=0), dict(B=0), dict(H=-1)):
        assert fwd(_loss_args(**kw)) == E_DIMS and bwd(_loss_args(**kw)) == E_DIMS, kw
    assert fwd(_loss_args(), rows=None) == E_DIMS and fwd(_loss_args(), scal=None) == E_DIMS
    assert bwd(_loss_args(), rows=None) == E_DIMS and bwd(_loss_args(), scal=None) == E_DIMS
    assert bwd(_loss_args(), gw=None) == E_DIMS and b"loss_backward" in L.tdmpc_last_error()


def _bn_fwd(rows, **null):
    names = ("x", "g", "b", "rmean", "rvar", "xhat", "rstd", "e", "part")
    return _lib.lib().tdmpc_sim_bn_fwd(*[None if n in null else FAKE for n in names], rows, None)


def _bn_bwd(rows, **null):
    names = ("de", "g", "xhat", "rstd", "e", "part", "dx", "dg", "db")
    return _lib.lib().tdmpc_sim_bn_bwd(*[None if n in null else FAKE for n in names], rows, None)


@pytest.mark.parametrize("rows", [1, 0, -3, 4097])
def test_batchnorm_entry_points_refuse_inadmissible_rows_without_a_device(rows):
    L = _lib.lib()
    n = C.c_size_t(12345)
    assert L.tdmpc_sim_bn_part_floats(rows, C.byref(n)) == E_DIMS and n.value == 12345
    assert _bn_fwd(rows) == E_DIMS and b"rows" in L.tdmpc_last_error()
    assert _bn_bwd(rows) == E_DIMS and b"rows" in L.tdmpc_last_error()


def test_predictor_piece_entry_points_refuse_null_pointers_without_a_device():
    L = _lib.lib()
    n = C.c_size_t()
    assert L.tdmpc_sim_bn_part_floats(130, C.byref(n)) == 0 and n.value == 2 * 2 * 512       # two 128-row chunks
    assert L.tdmpc_sim_bn_part_floats(4096, C.byref(n)) == 0 and n.value == 32 * 2 * 512
    assert L.tdmpc_sim_bn_part_floats(130, None) == E_DIMS
    for name in ("x", "g", "b", "rmean", "rvar", "xhat", "rstd", "e", "part"):
        assert _bn_fwd(130, **{name: 1}) == E_DIMS and f"{name} is null".encode() in L.tdmpc_last_error(), name
    for name in ("de", "g", "xhat", "rstd", "e", "part", "dx", "dg", "db"):
        assert _bn_bwd(130, **{name: 1}) == E_DIMS and f"{name} is null".encode() in L.tdmpc_last_error(), name
    for rows, lat in ((0, 50), (4097, 50), (33, 0), (33, 257)):
        assert L.tdmpc_sim_cos_fwd(FAKE, FAKE, FAKE, rows, lat, None) == E_DIMS, (rows, lat)
        assert L.tdmpc_sim_cos_bwd(FAKE, FAKE, FAKE, FAKE, rows, lat, None) == E_DIMS, (rows, lat)
    for i in range(3):
        ptrs = [FAKE] * 3
        ptrs[i] = None
        assert L.tdmpc_sim_cos_fwd(*ptrs, 33, 50, None) == E_DIMS and b"is null" in L.tdmpc_last_error()
    for i in range(4):
        ptrs = [FAKE] * 4
        ptrs[i] = None
        assert L.tdmpc_sim_cos_bwd(*ptrs, 33, 50, None) == E_DIMS and b"is null" in L.tdmpc_last_error()


def test_version_numbers():
    L = _lib.lib()
    assert L.tdmpc_sim_learner_version() == 1 == _lib.SIM_LEARNER_VERSION
    assert L.tdmpc_abi_version() == _lib.ABI_VERSION                      # the existing ABI is unchanged
