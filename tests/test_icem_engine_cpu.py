"""CPU: what tdmpc_amd/icem_engine.py (the MLP iCEM agent's update on the learner engine) decides
without a device -- which cfgs the engine admits and how it names the ones it does not, and that `TdIcemMlp(engine=True)`
whose cfg or device the engine refuses still constructs and plans. The update itself: tests/test_gpu_icem_engine.py.

The engine adds no C entry point (the encoders' second copy of the latents is tdmpc_lg_job.c2), so there is no new
null-pointer or shape refusal to pin here.
"""
from types import SimpleNamespace

import pytest
import torch

import icem_update_ref as U
from tdmpc_amd import icem_engine, sim_engine
from tdmpc_amd.config import make_cfg

ADMITTED = [("cartpole", {}), ("cheetah", {}), ("humanoid", {}), ("cheetah", dict(enc_dim=256)),
            ("cheetah", dict(enc_dim=1024)), ("humanoid", dict(latent_dim=256, optim_id="adam")),
            ("cheetah", dict(horizon=7, batch_size=512)),          # (7 + 1) * 512 = 4096 rows exactly
            ("cheetah", dict(horizon=1, batch_size=2))]

# 4097 = 17 * 241: horizon 16, batch 241 is one row past the cap, while horizon * batch_size = 3856 passes SimEngine's
REFUSED = [
    (dict(mlp_dim=256), r"mlp_dim=256"),
    (dict(batch_size=2048, horizon=5), r"batch_size=2048"),        # 12288 rows
    (dict(horizon=16, batch_size=241), r"4097 rows exceed 4096 \(horizon=16, batch_size=241\)"),
    (dict(weight_decay=0.01), r"weight_decay=0.01"),
    (dict(normalize=False), r"normalize=False"),
    (dict(modality="pixels"), r"modality='pixels'"),
    (dict(optim_id="sgd"), r"optim_id='sgd'"),
    (dict(batch_size=1), r"batch_size=1 "),
    (dict(latent_dim=257), r"latent_dim=257"),
    (dict(norm_type="bn"), r"norm_type='bn'"),
    (dict(enc_dim=300), r"enc_dim=300"),
]
_ids = [",".join(f"{k}={v}" for k, v in o.items()) for o, _ in REFUSED]


@pytest.mark.parametrize("task,over", ADMITTED)
def test_admitted_cfgs(task, over):
    cfg = make_cfg(task, **over)
    assert icem_engine.supported(cfg) and icem_engine.reason(cfg) is None and sim_engine.supported(cfg)


@pytest.mark.parametrize("over,match", REFUSED, ids=_ids)
def test_refusals_name_the_setting_and_need_no_device(over, match):
    import re
    cfg = make_cfg("cheetah", **over)
    why = icem_engine.reason(cfg)
    assert not icem_engine.supported(cfg) and why is not None
    assert why.startswith("IcemEngineLearner: ") and re.search(match, why), why
    agent = SimpleNamespace(cfg=cfg, model=None, model_target=None, device=torch.device("cpu"))
    with pytest.raises(ValueError, match=match):
        icem_engine.IcemEngineLearner(agent)                               # before it looks at the model
    with pytest.raises(ValueError, match=match):
        icem_engine.IcemEngine(agent)


def test_the_row_cap_is_the_intrinsic_pass_s():
    """SimEngine admits horizon * batch_size <= 4096; the intrinsic pass takes one more block of rows."""
    cfg = make_cfg("cheetah", horizon=16, batch_size=241)
    assert sim_engine.supported(cfg) and not icem_engine.supported(cfg)
    cfg = make_cfg("cheetah", horizon=7, batch_size=513)
    assert sim_engine.supported(cfg) and not icem_engine.supported(cfg)


class _StubPlanner:
    """What `TdIcemMlp` asks of its planner when it only learns (the real one needs the GPU)."""
    _packed_key = "packed"
    pmax, E_max, elites = 1, 0, None

    def __init__(self, *a, **k):
        pass


def _cpu_agent(monkeypatch, engine, **over):
    from tdmpc_amd import icem_mlp
    monkeypatch.setattr(icem_mlp, "IcemMlpPlanner", _StubPlanner)
    cfg = U.case_cfg("tiny")
    cfg.device = "cpu"
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg, icem_mlp.TdIcemMlp(cfg, graph=False, engine=engine)


@pytest.mark.parametrize("over,match", [(dict(batch_size=2048, horizon=5), "4096"), (dict(normalize=False), "normalize"),
                                        (dict(weight_decay=0.01), "weight_decay"), (dict(mlp_dim=256), "mlp_dim=256"),
                                        ({}, "CPU")])
@pytest.mark.parametrize("by_env", [False, True])
def test_an_agent_the_engine_refuses_still_constructs_and_names_the_reason(monkeypatch, over, match, by_env):
    if by_env:
        monkeypatch.setenv("TDMPC_ICEM_LEARNER_ENGINE", "1")
    else:
        monkeypatch.delenv("TDMPC_ICEM_LEARNER_ENGINE", raising=False)
    cfg, agent = _cpu_agent(monkeypatch, engine=not by_env, **over)
    assert agent._learner is None and agent.plan_horizon == 1 and isinstance(agent.planner, _StubPlanner)
    assert ("_predictor.1.weight" in agent.model.state_dict()) == getattr(cfg, "normalize", True)
    with pytest.raises(ValueError, match=match) as e:
        agent.update(U.FakeBuffer(U.case_batch("tiny")), U.STEPS[0])
    assert "IcemEngineLearner" in str(e.value)
    with pytest.raises(ValueError, match=match):
        agent.optim
    with pytest.raises(ValueError, match=match):
        agent.reward_rms
    assert agent._learner is None


def test_without_the_argument_and_the_variable_the_learner_is_the_autograd_one(monkeypatch):
    from tdmpc_amd.icem_learner import IcemMlpLearner
    monkeypatch.delenv("TDMPC_ICEM_LEARNER_ENGINE", raising=False)
    cfg, agent = _cpu_agent(monkeypatch, engine=False)
    assert isinstance(agent.learner, IcemMlpLearner) and agent.LEARNER == "IcemMlpLearner"
    monkeypatch.setenv("TDMPC_ICEM_LEARNER_ENGINE", "0")
    cfg, agent = _cpu_agent(monkeypatch, engine=False)
    assert isinstance(agent.learner, IcemMlpLearner)
