"""CPU: the DSSM update's yardstick against the recorded reference run, and `DssmLearner`'s PyTorch path against the
yardstick, both bit for bit; the ABI refusals of the new entry points without a device.

  * tests/drnn_update_ref.py in float32 == tests/golden/drnn_update/*.npz (the reference's `TdICemSimDssm.update` run by
    tests/golden/make_drnn_update_golden.py): metrics, priorities, intrinsic rewards, the RunningMeanStd state, every
    .grad and every tensor of model and target after each of two consecutive updates, as exact equality of the
    recording's arrays (float64 sum, sum of squares and 64 fixed elements per tensor).
  * `tdmpc_amd.drnn_learner.DssmLearner` on a CPU model (its PyTorch path) == the yardstick, to the same standard.
  * num_batches_tracked moves by 2H + 1 (prior_mlp) and H + 2 (_predictor) per update.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import drnn_update_ref as U
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


@pytest.mark.parametrize("name", U.RECORDED)
def test_restatement_equals_the_recorded_reference_update_bitwise(name):
    g, agent, res, out = _ref32(name)
    H = U.case_cfg(name).horizon
    for k in range(len(U.STEPS)):
        for key in sorted(out):
            if key.startswith(f"u{k}_"):
                _same((name, key), out[key], g[key])
        nbt = 1000 + (k + 1) * np.array([2 * H + 1, H + 2])
        assert g[f"u{k}_nbt"].tolist() == nbt.tolist()
    assert int(agent.model._dynamics.prior_mlp[1].num_batches_tracked) == 1000 + 2 * (2 * H + 1)
    assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + 2 * (H + 2)


@pytest.mark.parametrize("name", U.RECORDED)
def test_the_makers_tie_guard_holds_on_the_committed_cases(name):
    """Every row of both update_pi calls has |Q1 - Q2| > 1e-4 (1 + |min Q|) (the float32 run is the reference's)."""
    _, agent, res, _ = _ref32(name)
    assert res[-1]["tie"] > U.TIE, res[-1]["tie"]


def test_fp32_floors_the_gpu_bounds_are_derived_from():
    """Prints, per case and update, the figures (drnn_update_ref.figures) that the float32 CPU run of the yardstick
    shows against float64 -- the noise floors quoted in tests/test_gpu_drnn_update.py (FLOORS), whose bounds are 8 x
    them -- and holds the float32 yardstick itself to those bounds, so a change of the yardstick or of the cases that
    moves a floor by a large factor shows up here."""
    from test_gpu_drnn_update import FLOORS, group
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
    from tdmpc_amd.drnn_learner import DssmLearner
    cfg = U.case_cfg(name)
    model, target = U.make_models(cfg, name)
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cpu"))
    return cfg, agent, DssmLearner(agent, graph=False)


@pytest.mark.parametrize("name", U.RECORDED)
def test_learner_pytorch_path_on_the_cpu_equals_the_restatement_bitwise(name):
    g, ref_agent, res, want = _ref32(name)
    cfg, agent, learner = _cpu_learner(name)
    assert not learner.hip and not learner.graph
    H = cfg.horizon
    buf = U.FakeBuffer(U.batch(cfg, U.CASES[name][7]))
    noise = U.gold_noise(g, cfg)
    got = {}
    for k, step in enumerate(U.STEPS):
        m, coef = learner.update(buf, step, noise[k])
        assert not agent.model.training
        r = dict(metrics=np.array(m.tolist() + [coef], dtype=np.float64), prio=buf.prios[-1].numpy(),
                 intrinsic=learner.last["intrinsic"].numpy(), rms=learner.rms.numpy().copy(),
                 grads=U.grads_of(agent.model))
        U.record(got, k, r, agent.model, agent.model_target)
        assert int(agent.model._dynamics.prior_mlp[1].num_batches_tracked) == 1000 + (k + 1) * (2 * H + 1)
        assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + (k + 1) * (H + 2)
    for key in sorted(want):
        _same((name, key), got[key], want[key])
    rms = learner.reward_rms
    assert (rms.mean, rms.var, rms.count) == tuple(res[-1]["rms"])


def test_learner_refusals_name_the_setting_and_need_no_device():
    from tdmpc_amd.drnn_learner import DssmLearner, check_learner_cfg
    from drnn_io import drnn_cfg
    dog = drnn_cfg("dog")                                      # batch_size 2048, horizon 5: 12288 rows
    with pytest.raises(ValueError, match="batch_size"):
        check_learner_cfg(dog)
    with pytest.raises(ValueError, match="batch_size=1 "):
        check_learner_cfg(drnn_cfg("cheetah", batch_size=1))
    with pytest.raises(NotImplementedError, match="norm_cell"):
        check_learner_cfg(drnn_cfg("cheetah", norm_cell=False))
    with pytest.raises(ValueError, match="optim_id"):
        check_learner_cfg(drnn_cfg("cheetah", optim_id="sgd"))
    check_learner_cfg(drnn_cfg("humanoid"))                    # 6 * 512 = 3072 rows
    agent = SimpleNamespace(cfg=dog, model=None, model_target=None, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="4096"):
        DssmLearner(agent)                                     # before it looks at the model


def _dims(**kw):
    from drnn_io import drnn_cfg
    d = _lib.drnn_dims_from_cfg(drnn_cfg("humanoid"))
    for k, v in kw.items():
        setattr(d.base, k, v)
    return d


def _intrinsic(d, S, B, z=FAKE):
    t22, t8 = (C.c_void_p * 22)(*([FAKE] * 22)), (C.c_void_p * 8)(*([FAKE] * 8))
    return _lib.lib().tdmpc_drnn_intrinsic_fwd(C.byref(d), t22, 22, t8, 8, z, FAKE, FAKE, S, B, FAKE, FAKE, 1 << 40,
                                               None)


@pytest.mark.parametrize("what,dims,S,B", [
    ("one row per segment", {}, 4, 1), ("no segment", {}, 0, 33), ("4097 rows", {}, 241, 17),
    ("mlp_dim 256", dict(mlp_dim=256), 4, 33)])
def test_intrinsic_fwd_refuses_unsupported_shapes_without_a_device(what, dims, S, B):
    d, L = _dims(**dims), _lib.lib()
    n = C.c_size_t()
    assert L.tdmpc_drnn_intrinsic_workspace_floats(C.byref(d), S, B, C.byref(n)) == E_DIMS, what
    assert _intrinsic(d, S, B) == E_DIMS and L.tdmpc_last_error(), what


def test_new_entry_points_refuse_null_pointers_without_a_device():
    d, L = _dims(), _lib.lib()
    n = C.c_size_t()
    assert L.tdmpc_drnn_intrinsic_workspace_floats(C.byref(d), 6, 512, C.byref(n)) == 0 and n.value > 0
    assert _intrinsic(d, 6, 512, z=None) == E_DIMS and b"z is null" in L.tdmpc_last_error()
    assert L.tdmpc_drnn_intrinsic_finish(FAKE, 4097, FAKE, FAKE, FAKE, FAKE, FAKE, None) == E_DIMS
    assert L.tdmpc_drnn_intrinsic_finish(FAKE, 0, FAKE, FAKE, FAKE, FAKE, FAKE, None) == E_DIMS
    assert L.tdmpc_drnn_intrinsic_finish(FAKE, 64, None, FAKE, FAKE, FAKE, FAKE, None) == E_DIMS
    assert L.tdmpc_drnn_intrinsic_finish(FAKE, 64, FAKE, None, FAKE, FAKE, FAKE, None) == E_DIMS   # reward_pi, no coef
    a = _lib.DrnnLossArgs()
    assert L.tdmpc_drnn_loss_forward(C.byref(a), FAKE, FAKE, FAKE, None) == E_DIMS
    assert L.tdmpc_drnn_loss_backward(C.byref(a), FAKE, FAKE, FAKE, FAKE, None, None, None, None, None) == E_DIMS
