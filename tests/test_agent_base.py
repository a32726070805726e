"""What the four planning agents share (tdmpc_amd.tdmpc.Agent, HipPlanner's read-back and graph cache, _lib.call):
the ABI call helper and the seed-step returns without a GPU; on the GPU the one status / metrics read-back of every
agent and the graph cache's cap. Shapes: tools/lib_equal.py's SMALL, humanoid dims for TOLD, cheetah dims with
hidden_dim 128 for the DSSM, B = 1 and B = 3."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tdmpc_amd import TDMPC, TdICEM, TdIcemDrnn, TdMpcDrnn, _lib, make_cfg
from tdmpc_amd.dssm import synthetic_dssm_state_dict
from tdmpc_amd.told import synthetic_state_dict

SMALL = dict(num_samples=64, num_elites=16, iterations=3, horizon=5)
STEP = 10**6   # past every schedule
M2 = {"external_reward_mean": 0.0, "current_std": 0.0}
M3 = {"intrinsic_reward_mean": 0.0, **M2}


def told_cfg(device, **kw):
    cfg = make_cfg("humanoid", **SMALL, **kw)
    cfg.device = device
    return cfg


def dssm_cfg(device, **kw):
    kw.setdefault("regularization_schedule", "0.5")
    cfg = make_cfg("cheetah", hidden_dim=128, norm_cell=True, plan2expl=False, warmup_len=0, **SMALL, **kw)
    cfg.device = device
    return cfg


# name -> (class, cfg, weights, plan takes a GRU state)
AGENTS = {"TDMPC": (TDMPC, told_cfg, lambda c: synthetic_state_dict(c, 7), False),
          "TdICEM": (TdICEM, told_cfg, lambda c: synthetic_state_dict(c, 31, enc_norm=True), False),
          "TdMpcDrnn": (TdMpcDrnn, dssm_cfg, lambda c: synthetic_dssm_state_dict(c, 7), True),
          "TdIcemDrnn": (TdIcemDrnn, dssm_cfg, lambda c: synthetic_dssm_state_dict(c, 7), True)}


def _inputs(cfg):
    g = torch.Generator().manual_seed(1)
    return torch.randn(3, cfg.obs_shape[0], generator=g), torch.rand(3, 128, generator=g) * 2 - 1


def _plan(agent, rec, obs, hidden, B, **kw):
    """plan() for one env, plan_batch() for B > 1 -> the whole return."""
    if B == 1:
        return agent.plan(obs[0].numpy(), *((hidden[:1],) if rec else ()), **kw)
    return agent.plan_batch(obs[:B], *((hidden[:B],) if rec else ()), **kw)


# ---------------------------------------------------------------------------------------------------- no GPU
def test_call_converts_arguments_and_raises_with_the_entry_point(monkeypatch):
    seen = []
    fake = SimpleNamespace(tdmpc_fake=lambda *a: seen.append(a) or 0)
    t, d = torch.zeros(4), _lib.Dims()
    with monkeypatch.context() as mp:
        mp.setattr(_lib, "_LIB", fake)
        _lib.call("tdmpc_fake", t[1:], None, d, 7)
    (a,) = seen
    assert a[0] == t.data_ptr() + 4 and a[1] is None and a[3] == 7   # (None: ctypes' null pointer, 0 at the ABI)
    assert C.addressof(a[2]._obj) == C.addressof(d)                  # the structure itself, by reference
    # through the library: structures filled through their reference, None arriving as a null pointer
    dd, sz = _lib.drnn_dims_from_cfg(dssm_cfg("cpu"), max_batch=3), _lib.Sizes()
    _lib.call("tdmpc_drnn_icem_sizes_for", dd, sz)
    assert sz.packed_weight_bytes > 0 and sz.workspace_bytes > 0
    cp = _lib.ColoredNoiseParams()
    for args in ((None, 4096, 16, 4096, 16, None), (cp, None, 16, 4096, 16, None), (cp, 4096, 16, None, 16, None)):
        with pytest.raises(RuntimeError, match="tdmpc_drnn_colored_noise failed with code -3"):
            _lib.call("tdmpc_drnn_colored_noise", *args)
    with pytest.raises(RuntimeError, match="tdmpc_drnn_icem_sizes_for failed with code -3"):
        _lib.call("tdmpc_drnn_icem_sizes_for", dd, None)


@pytest.mark.parametrize("name", AGENTS)
def test_seed_step_returns(name):
    cls, mk, _, rec = AGENTS[name]
    cfg = mk("cpu")
    agent = cls(cfg, max_batch=3)
    obs, hidden = _inputs(cfg)
    A, m0 = cfg.action_dim, M3 if name == "TdMpcDrnn" else M2
    out = _plan(agent, rec, obs, hidden, 1, step=0, t0=True)
    assert len(out) == (3 if name == "TdIcemDrnn" else 2)
    assert out[0].shape == (A,) and out[0].dtype == torch.float32 and bool((out[0].abs() <= 1).all())
    assert out[-1] == m0 and list(out[-1]) == list(m0)
    if name == "TdICEM":
        with pytest.raises(ValueError, match="seed steps"):
            agent.plan_batch(obs, step=0, t0=True)
        return
    out = _plan(agent, rec, obs, hidden, 3, step=0, t0=True)
    assert len(out) == (3 if name == "TdIcemDrnn" else 2)
    assert out[0].shape == (3, A) and bool((out[0].abs() <= 1).all())
    assert out[-1] == [m0] * 3 and all(list(m) == list(m0) for m in out[-1])
    if name == "TdIcemDrnn":
        assert out[1] is None and _plan(agent, rec, obs, hidden, 1, step=0, t0=True)[1] is None
    if name == "TDMPC":
        a, m = agent.plan_batch(obs, step=0, t0=True, sync_metrics=False)
        assert a.shape == (3, A) and torch.is_tensor(m) and m.shape == (3, 2) and not m.any()
    # an evaluation call is planned even at a seed step: it reaches the argument checks
    with pytest.raises(ValueError, match="max_batch"):
        agent.plan_batch(torch.zeros(4, cfg.obs_shape[0]), *((torch.zeros(4, 128),) if rec else ()), step=0,
                         eval_mode=True)


# ---------------------------------------------------------------------------------------------------- GPU
def _gpu_agent(name, **kw):
    cls, mk, weights, rec = AGENTS[name]
    cfg = mk("cuda", **kw.pop("cfg", {}))
    agent = cls(cfg, max_batch=3, **kw)
    agent.model.load_state_dict(weights(cfg))
    agent.std = 0.05
    return agent, cfg, rec


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("name", AGENTS)
def test_status_word_raises_once_at_the_read_back(name, B):
    agent, cfg, rec = _gpu_agent(name)
    obs, hidden = _inputs(cfg)
    pl = agent.planner
    pl.status.fill_(_lib.STATUS_PACK_STALE)
    with pytest.raises(RuntimeError, match="job table"):
        _plan(agent, rec, obs, hidden, B, step=STEP, t0=True)
    assert int(pl.status.item()) == 0
    a = _plan(agent, rec, obs, hidden, B, step=STEP, t0=True)[0]
    assert a.shape == ((cfg.action_dim,) if B == 1 else (B, cfg.action_dim)) and bool(torch.isfinite(a).all())


@pytest.mark.gpu
def test_graph_cache_cap_and_recapture():
    """Ten values of num_pi over a ramping regularization_schedule: TdMpcDrnn keeps MAX_GRAPHS captured plans, and a
    plan evicted and captured again equals, bitwise, the eager agent's on the same seeds. TDMPC keeps every graph."""
    ramp = dict(cfg=dict(regularization_schedule="linear(0.0, 0.5, 32000, 0)"))   # P = int(step / 1000)
    ga, cfg, _ = _gpu_agent("TdMpcDrnn", graph=True, **ramp)
    ea, _, _ = _gpu_agent("TdMpcDrnn", graph=False, **ramp)
    obs, hidden = _inputs(cfg)
    pl = ga.planner
    for k, P in enumerate(list(range(5, 15)) + [5, 6]):   # (5 and 6 were evicted by 13 and 14)
        acts = []
        for agent in (ga, ea):
            torch.manual_seed(100 + k)
            np.random.seed(200 + k)
            acts.append(agent.plan(obs[0].numpy(), hidden[:1], step=1000 * P + 500, t0=k == 0)[0])
            assert agent.planner.P == P
        assert torch.equal(*acts), (k, P)
        assert len(pl._graphs) == min(k + 1, TdMpcDrnn.MAX_GRAPHS) and not ea.planner._graphs
    assert [key[3] for key in pl._graphs] == [9, 10, 11, 12, 13, 14, 5, 6]
    agent, cfg, _ = _gpu_agent("TDMPC", rng="fused")
    obs, _ = _inputs(cfg)
    n = 0
    for B in (1, 2, 3):
        for ev in (False, True):
            for sync in (True, False):
                a, _ = agent.plan_batch(obs[:B], eval_mode=ev, step=STEP, t0=True, sync_metrics=sync)
                n += 1
                assert len(agent.planner._graphs) == n and bool(torch.isfinite(a).all())
    agent.planner.check_status()
    assert n > TdMpcDrnn.MAX_GRAPHS
