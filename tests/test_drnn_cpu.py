"""CPU checks of the recurrent-latent (DSSM) planner: the module's layout, the restatement against the reference's
recorded outputs (bit for bit), and the C ABI's argument checks (no GPU needed)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import drnn_ref
from drnn_io import case_inputs, cases, drnn_cfg
from tdmpc_amd import _lib
from tdmpc_amd.dssm import DSSM, float_tensors, synthetic_dssm_state_dict

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_dssm_state_dict_matches_reference_layout():
    cfg = cases()["humanoid"][0]
    lay = json.load(open(os.path.join(GOLD, "dssm_layout.json")))
    sd = DSSM(cfg).state_dict()
    assert list(sd.keys()) == list(lay.keys())
    for k, v in sd.items():
        assert list(v.shape) == lay[k], k
    syn = synthetic_dssm_state_dict(cfg, 3)
    assert list(syn.keys()) == list(lay.keys())
    DSSM(cfg).load_state_dict(syn)
    # the zero-initialised last layers and the BatchNorm statistics are not degenerate
    for k in ("_reward.4.weight", "_Q1.6.weight", "_Q2.6.weight"):
        assert syn[k].abs().max() > 0
    rv = syn["_dynamics.prior_mlp.1.running_var"]
    assert 0.5 <= rv.min() and rv.max() <= 1.5 and rv.std() > 0.1
    assert syn["_dynamics.prior_mlp.1.running_mean"].abs().max() > 0


@pytest.mark.parametrize("ov,word", [(dict(modality="pixels"), "modality"), (dict(norm_cell=False), "norm_cell"),
                                      (dict(plan2expl=True), "plan2expl")])
def test_dssm_unsupported_settings_raise(ov, word):
    with pytest.raises(NotImplementedError, match=word):
        DSSM(drnn_cfg("cheetah", **ov))


@pytest.mark.parametrize("name", ["humanoid", "cheetah", "horizon"])
def test_restatement_matches_reference_bitwise(name):
    cfg, wseed, iseed, calls = cases()[name]
    G = np.load(os.path.join(GOLD, "drnn", f"drnn_{name}.npz"))
    model = drnn_ref.RefDSSM(synthetic_dssm_state_dict(cfg, wseed), cfg)
    st = drnn_ref.DrnnState(0.05, cfg.warmup_len)
    obs, hidden = case_inputs(cfg, iseed, len(calls))
    assert np.array_equal(hidden, G["hidden"])
    for ci, (step, t0, ev) in enumerate(calls):
        torch.manual_seed(300 + ci)
        np.random.seed(400 + ci)
        nz = drnn_ref.draw_drnn_noise(cfg, st, step, t0, ev)
        tr = {}
        a, m = drnn_ref.plan(model, cfg, st, obs[ci], hidden, nz, eval_mode=ev, step=step, t0=t0, trace=tr)
        assert st.plan_horizon == int(G[f"c{ci}_horizon"])
        vals = torch.stack([v.squeeze(1) for v in tr["value"]]).numpy()
        assert np.array_equal(vals, G[f"c{ci}_values"]), ci
        assert np.array_equal(a.numpy(), G[f"c{ci}_action"]), ci
        assert np.array_equal(np.array([m["intrinsic_reward_mean"], m["external_reward_mean"], m["current_std"]],
                                       dtype=np.float64), G[f"c{ci}_metrics"]), ci
        assert np.array_equal(st.prev_mean.numpy(), G[f"c{ci}_prev_mean"]), ci
    if name == "horizon":
        assert int(G["c1_horizon"]) == 3   # the schedule says 4 at step 17000; inside the episode it stays 3
    if name == "cheetah":
        assert len(st.memory) == cfg.warmup_len


def test_eager_next_equals_restatement():
    """The module's own forward (NormGRUCell, DGruDyna, DSSM.next in eval mode) is the restatement's, bit for bit."""
    cfg = cases()["cheetah"][0]
    sd = synthetic_dssm_state_dict(cfg, 5)
    model = DSSM(cfg, init="none")
    model.load_state_dict(sd)
    model.eval()
    ref = drnn_ref.RefDSSM(sd, cfg)
    rs = np.random.RandomState(2)
    z = torch.from_numpy(rs.standard_normal((7, cfg.latent_dim)).astype(np.float32))
    a = torch.from_numpy(rs.uniform(-1, 1, (7, cfg.action_dim)).astype(np.float32))
    h = torch.from_numpy(rs.uniform(-1, 1, (7, cfg.hidden_dim)).astype(np.float32))
    with torch.no_grad():
        got = model.next(z, a, h)
        obs = torch.from_numpy(rs.standard_normal((3, cfg.obs_shape[0])).astype(np.float32))
        assert torch.equal(model.h(obs), ref.h(obs))
    for g, r in zip(got, ref.next(z, a, h)):
        assert torch.equal(g, r)
    assert model.init_hidden_state(4, "cpu").shape == (4, cfg.hidden_dim)


def test_default_cfg_carries_the_dssm_settings():
    """make_cfg ships the reference's DSSM defaults (hidden_dim 128, norm_cell, warmup_len 0), so the agent builds from a
    plain task cfg; a cfg without hidden_dim is refused with the setting named."""
    from tdmpc_amd.config import make_cfg
    from tdmpc_amd.drnn import TdMpcDrnn
    cfg = make_cfg("cheetah", num_samples=32, num_elites=8)
    cfg.device = "cpu"
    assert (cfg.hidden_dim, cfg.norm_cell, cfg.warmup_len, cfg.plan2expl) == (128, True, 0, False)
    agent = TdMpcDrnn(cfg)
    assert agent.planner.hidden_dim == 128 and agent.memory_latents.maxlen == 0
    del cfg.hidden_dim
    with pytest.raises(AttributeError, match="hidden_dim"):
        DSSM(cfg)


def _dims(cfg, **ov):
    d = _lib.drnn_dims_from_cfg(cfg)
    for k, v in ov.items():
        if k == "hidden_dim":
            d.hidden_dim = v
        else:
            setattr(d.base, k, v)
    return d


def test_drnn_sizes_and_tensor_count():
    L = _lib.lib()
    assert L.tdmpc_drnn_version() == _lib.DRNN_VERSION
    for name in ("humanoid", "cheetah"):
        cfg = cases()[name][0]
        d = _dims(cfg)
        s, s0 = _lib.Sizes(), _lib.Sizes()
        assert L.tdmpc_drnn_sizes_for(C.byref(d), C.byref(s)) == 0
        assert L.tdmpc_sizes_for(C.byref(d.base), C.byref(s0)) == 0
        # the shared planner layout plus the GRU / prior / reward regions and two hidden-state buffers
        assert s.packed_weight_bytes > s0.packed_weight_bytes and s.workspace_bytes > s0.workspace_bytes
        assert s.noise_floats_per_env == s0.noise_floats_per_env
        n = L.tdmpc_drnn_num_param_tensors(C.byref(d))
        assert n == len(float_tensors(synthetic_dssm_state_dict(cfg, 0))) == 62
        # a smaller hidden state needs less of both
        s1 = _lib.Sizes()
        assert L.tdmpc_drnn_sizes_for(C.byref(_dims(cfg, hidden_dim=64)), C.byref(s1)) == 0
        assert s1.packed_weight_bytes < s.packed_weight_bytes and s1.workspace_bytes < s.workspace_bytes


@pytest.mark.parametrize("ov", [dict(hidden_dim=100), dict(hidden_dim=288), dict(modality=1), dict(mlp_dim=500),
                                dict(mlp_dim=256), dict(enc_norm=0)])
def test_drnn_bad_dims_rejected(ov):
    L = _lib.lib()
    d = _dims(cases()["humanoid"][0], **ov)
    s = _lib.Sizes()
    assert L.tdmpc_drnn_sizes_for(C.byref(d), C.byref(s)) == -1
    assert L.tdmpc_last_error()
    one = C.c_void_p(64)   # never dereferenced: the dims check comes first
    arr = (C.c_void_p * 62)(*[64] * 62)
    prm = _lib.PlanParams()
    prm.horizon, prm.iterations, prm.batch = 5, 3, 1
    assert L.tdmpc_drnn_pack_weights(C.byref(d), arr, 62, one, 1 << 30, None) == -1
    assert L.tdmpc_drnn_next(C.byref(d), one, one, one, one, 4, one, one, one, one, 1 << 30, None) == -1
    assert L.tdmpc_drnn_estimate_value(C.byref(d), C.byref(prm), one, one, one, one, one, 96, one, one, one, 1 << 30,
                                       None) == -1
    assert L.tdmpc_drnn_pi_rollout(C.byref(d), C.byref(prm), one, one, one, one, one, one, 1 << 30, None) == -1
    assert L.tdmpc_drnn_plan(C.byref(d), C.byref(prm), one, one, one, one, one, one, one, one, None, None, None, None,
                             None, None, one, 1 << 30, None) == -1


def test_drnn_null_arguments_rejected():
    L = _lib.lib()
    d = _dims(cases()["humanoid"][0])
    s = _lib.Sizes()
    prm = _lib.PlanParams()
    prm.horizon, prm.iterations, prm.batch = 5, 3, 1
    one = C.c_void_p(64)
    arr = (C.c_void_p * 62)(*[64] * 62)
    assert L.tdmpc_drnn_sizes_for(None, C.byref(s)) == -3
    assert L.tdmpc_drnn_sizes_for(C.byref(d), None) == -3
    assert L.tdmpc_drnn_num_param_tensors(None) == -3
    assert L.tdmpc_drnn_pack_weights(C.byref(d), None, 62, one, 1 << 30, None) == -3
    assert L.tdmpc_drnn_pack_weights(C.byref(d), arr, 62, None, 1 << 30, None) == -3
    assert L.tdmpc_drnn_next(C.byref(d), one, one, one, None, 4, one, one, one, one, 1 << 30, None) == -3
    assert L.tdmpc_drnn_next(C.byref(d), one, one, one, one, 4, one, one, None, one, 1 << 30, None) == -3
    assert L.tdmpc_drnn_estimate_value(C.byref(d), C.byref(prm), one, one, None, one, one, 96, one, one, one, 1 << 30,
                                       None) == -3
    assert L.tdmpc_drnn_pi_rollout(C.byref(d), C.byref(prm), one, one, None, one, one, one, 1 << 30, None) == -3
    assert L.tdmpc_drnn_plan(C.byref(d), C.byref(prm), one, one, None, one, one, one, one, one, None, None, None, None,
                             None, None, one, 1 << 30, None) == -3
    assert L.tdmpc_drnn_plan(C.byref(d), None, one, one, one, one, one, one, one, one, None, None, None, None, None,
                             None, one, 1 << 30, None) == -3
    # a tensor count other than the state_dict's
    assert L.tdmpc_drnn_pack_weights(C.byref(d), arr, 61, one, 1 << 30, None) == -1


def test_seed_step_branch_needs_no_model():
    """plan() below seed_steps returns a uniform action and the zero metrics without touching the device planner."""
    from tdmpc_amd.drnn import TdMpcDrnn
    cfg = cases()["horizon"][0]
    cfg.device = "cpu"
    agent = TdMpcDrnn(cfg)
    torch.manual_seed(1)
    a, m = agent.plan(np.zeros(cfg.obs_shape, np.float32), np.zeros((1, cfg.hidden_dim), np.float32), step=10, t0=True)
    torch.manual_seed(1)
    assert torch.equal(a, torch.empty(cfg.action_dim).uniform_(-1, 1))
    assert m == {"intrinsic_reward_mean": 0.0, "external_reward_mean": 0.0, "current_std": 0.0}
    assert len(agent.memory_latents) == 0
