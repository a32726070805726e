"""CPU checks of the recurrent-latent iCEM planner: the restatement against the reference's recorded outputs (bit for
bit), the agent's per-iteration counts and noise-stream layout against the restatement's, and the C ABI's argument
checks (no GPU needed)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import drnn_icem_ref as ref
import drnn_ref
from drnn_icem_io import case_inputs, cases, load
from tdmpc_amd import _lib
from tdmpc_amd.config import linear_schedule
from tdmpc_amd.dssm import synthetic_dssm_state_dict


@pytest.mark.parametrize("name", ["humanoid", "cheetah"])
def test_restatement_matches_reference_bitwise(name):
    cfg, wseed, iseed, base, calls = cases()[name]
    G = load(name)
    model = drnn_ref.RefDSSM(synthetic_dssm_state_dict(cfg, wseed), cfg)
    st = ref.IcemDrnnState(0.05)
    obs, hidden = case_inputs(cfg, iseed, len(calls))
    assert np.array_equal(hidden, G["hidden"])
    for ci, (step, t0, ev) in enumerate(calls):
        torch.manual_seed(base + ci)
        np.random.seed(base + 100 + ci)
        nz = ref.draw_noise(cfg, st, step, t0, ev)
        tr = {}
        a, h, m = ref.plan(model, cfg, st, obs[ci], hidden, nz, eval_mode=ev, step=step, t0=t0, trace=tr)
        assert st.plan_horizon == int(G[f"c{ci}_horizon"])
        assert np.array_equal(np.array([len(v) for v in tr["value"]]), G[f"c{ci}_nvals"]), ci
        vals = torch.cat([v.squeeze(1) for v in tr["value"]]).numpy()
        assert np.array_equal(vals, G[f"c{ci}_values"]), ci
        assert np.array_equal(a.numpy(), G[f"c{ci}_action"]), ci
        assert np.array_equal(h.numpy(), G[f"c{ci}_hidden"]), ci
        assert np.array_equal(np.array([m["external_reward_mean"], m["current_std"]], dtype=np.float64),
                              G[f"c{ci}_metrics"]), ci
        assert np.array_equal(st.prev_mean.numpy(), G[f"c{ci}_prev_mean"]), ci
        assert np.array_equal(st.elite_actions.numpy(), G[f"c{ci}_elites"]), ci
    if name == "humanoid":
        assert G["c0_nvals"].tolist() == [96, 76, 60] and G["c1_nvals"].tolist() == [100, 80, 64]
    else:
        # the second episode start: the horizon grows and an agent with elites reuses none
        assert [int(G[f"c{ci}_horizon"]) for ci in range(3)] == [3, 3, 4]
        assert G["c1_nvals"].tolist() == [50, 39] and G["c2_nvals"].tolist() == [48, 37]


@pytest.mark.parametrize("name", ["humanoid", "cheetah"])
def test_agent_counts_and_layout_equal_restatement(name):
    from tdmpc_amd.drnn_icem import TdIcemDrnn
    cfg = SimpleNamespace(**vars(cases()[name][0]))
    cfg.device = "cpu"
    agent = TdIcemDrnn(cfg)
    step = cases()[name][4][0][0]
    mix = linear_schedule(cfg.regularization_schedule, step)
    H = int(min(cfg.horizon, linear_schedule(cfg.horizon_schedule, step)))
    for t0 in (True, False):
        for has in (False, True):
            st = ref.IcemDrnnState(0.05)
            st.elite_actions = torch.zeros(H, cfg.num_elites, cfg.action_dim) if has else None
            want = ref.counts(cfg, mix, has, t0)
            got = agent.counts(mix, has, t0)
            assert got == want, (t0, has)
            reuse = ref.reuses(cfg, st, t0)
            assert reuse == (got[0][2] > 0)
            assert agent.layout(H, got, reuse) == ref.layout(cfg, H, want, reuse), (t0, has)
            if t0:
                assert all(e == 0 for _, _, e in got)
            else:
                assert [e for _, _, e in got][1:] == [int(cfg.fraction_elites_reused * cfg.num_elites)] * (
                    cfg.iterations - 1)
    # the stream the draws fill is the layout: sizes of an explicit draw add up to its total
    st = ref.IcemDrnnState(0.05)
    st.plan_horizon = H
    st.elite_actions = torch.zeros(H, cfg.num_elites, cfg.action_dim)
    nz = ref.draw_noise(cfg, st, step, False, False)
    cts = agent.counts(mix, True, False)
    n = nz.eps_pi.numel() + sum(s.numel() for s in nz.samp) + nz.reuse.numel() + sum(t.numel() for t in nz.term) + \
        nz.eps_act.numel()
    assert n == agent.layout(H, cts, True)["total"]


def test_agent_refuses_what_the_reference_cannot_run():
    from tdmpc_amd.drnn_icem import TdIcemDrnn
    base = vars(cases()["cheetah"][0])
    hidden = np.zeros((1, 128), np.float32)
    obs = np.zeros(17, np.float32)
    for ov, exc, word in ((dict(keep_previous_elites=False), NotImplementedError, "keep_previous_elites"),
                          (dict(noise_beta=2.5, horizon_schedule="1"), ValueError, "noise_beta")):
        cfg = SimpleNamespace(**{**base, **ov, "device": "cpu"})
        agent = TdIcemDrnn(cfg)
        with pytest.raises(exc, match=word):
            agent.plan(obs, hidden, step=10**6, t0=False)
    cfg = SimpleNamespace(**{**base, "shift_elites_over_time": False, "device": "cpu"})
    agent = TdIcemDrnn(cfg)
    agent._has_elites = True
    with pytest.raises(NotImplementedError, match="shift_elites_over_time"):
        agent.plan(obs, hidden, step=10**6, t0=False)
    a, h, m = TdIcemDrnn(SimpleNamespace(**{**base, "device": "cpu"})).plan(obs, hidden, step=10, t0=True)
    assert a.shape == (6,) and h is None and m == {"external_reward_mean": 0.0, "current_std": 0.0}


def test_icem_sizes_and_null_checks():
    L = _lib.lib()
    for name in ("humanoid", "cheetah"):
        cfg = cases()[name][0]
        d = _lib.drnn_dims_from_cfg(cfg, max_batch=3)
        s, s0 = _lib.Sizes(), _lib.Sizes()
        assert L.tdmpc_drnn_icem_sizes_for(C.byref(d), C.byref(s)) == 0
        assert L.tdmpc_drnn_sizes_for(C.byref(d), C.byref(s0)) == 0
        assert s.packed_weight_bytes == s0.packed_weight_bytes
        assert s.workspace_bytes >= s0.workspace_bytes         # (one workspace serves both sets of entry points)
        assert s.noise_floats_per_env >= s0.noise_floats_per_env
    assert L.tdmpc_drnn_icem_sizes_for(None, C.byref(s)) == -3
    assert L.tdmpc_drnn_icem_sizes_for(C.byref(d), None) == -3
    d.base.num_pi = 0
    assert L.tdmpc_drnn_icem_sizes_for(C.byref(d), C.byref(s)) == -1
    assert b"num_pi" in L.tdmpc_last_error()
    # TDMPC_E_NULL for each missing required pointer, before anything touches the device (fake non-null addresses)
    d = _lib.drnn_dims_from_cfg(cfg)
    prm = _lib.IcemParams()
    req = [C.byref(d), C.byref(prm)] + [C.c_void_p(4096)] * 10 + [None, None, None, None, C.c_void_p(4096)]
    # (dims, params, packed, obs, hidden, noise, u, prev_mean, elites, action, metrics, hidden_out | z_out, value_out,
    #  mean_out, std_out | workspace)
    required = list(range(12)) + [16]
    for k in required:
        args = list(req)
        args[k] = None
        assert L.tdmpc_drnn_plan_icem(*args, 1 << 30, None) == -3, k
    cp = _lib.ColoredNoiseParams()
    assert L.tdmpc_drnn_colored_noise(None, C.c_void_p(4096), 16, C.c_void_p(4096), 16, None) == -3
    assert L.tdmpc_drnn_colored_noise(C.byref(cp), None, 16, C.c_void_p(4096), 16, None) == -3
    assert L.tdmpc_drnn_colored_noise(C.byref(cp), C.c_void_p(4096), 16, None, 16, None) == -3
    # ... and the domain / bounds checks reject a job before any launch
    assert L.tdmpc_drnn_colored_noise(C.byref(cp), C.c_void_p(4096), 16, C.c_void_p(4096), 16, None) == -1   # L = 0
    from tdmpc_amd.drnn_icem import colored_noise_params
    with pytest.raises(ValueError, match="2..16"):
        colored_noise_params(1, 6, 1, 100, 100, [(0, 1, 1, 0, 0, 0)], [2.5])
    # one job of 4 sequences x A = 6 over L = 5: 120 stream floats, 2 * 3 * 24 = 144 normals
    ok = colored_noise_params(5, 6, 1, 120, 144, [(0, 4, 4, 0, 0, 0)], [2.5])
    assert L.tdmpc_drnn_colored_noise(C.byref(ok), C.c_void_p(4096), 143, C.c_void_p(4096), 120, None) == -4
    assert L.tdmpc_drnn_colored_noise(C.byref(ok), C.c_void_p(4096), 144, C.c_void_p(4096), 119, None) == -4
    short = colored_noise_params(5, 6, 1, 119, 144, [(0, 4, 4, 0, 0, 0)], [2.5])
    assert L.tdmpc_drnn_colored_noise(C.byref(short), C.c_void_p(4096), 144, C.c_void_p(4096), 120, None) == -4
    wide = colored_noise_params(5, 6, 1, 120, 144, [(0, 4, 4, 1, 0, 0)], [2.5])   # c0 + n > rows
    assert L.tdmpc_drnn_colored_noise(C.byref(wide), C.c_void_p(4096), 144, C.c_void_p(4096), 120, None) == -1


def test_drnn_abi_version_is_2():
    assert _lib.lib().tdmpc_drnn_version() == 2 == _lib.DRNN_VERSION
