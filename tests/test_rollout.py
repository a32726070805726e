"""`RolloutBuffer` (the reference's variable-length-episode buffer, helper.py:537-636).

* `RefRollout` (tests/rollout_ref.py) reproduces the reference class's recorded samples and priorities
  (tests/golden/rollout/*.npz from make_rollout_golden.py) with max abs diff 0.
* The device buffer (tdmpc_amd.replay.RolloutBuffer) against `RefRollout` on the same schedules and uniforms: indices,
  windows and priorities bitwise, `idx` / `_full` after every step; weights to the 2e-6 relative that
  tests/test_replay.py::test_gpu_replay_matches_reference uses (the device's fp32 sum of p**alpha has its own order).
* A TDMPC learner on the new buffer: graph replay equals eager, bitwise.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from rollout_ref import SCHEDULES, Ep, RefRollout, case_cfg, episode, run_schedule, uniforms

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "rollout")
WEIGHT_RTOL = 2e-6   # tests/test_replay.py::test_gpu_replay_matches_reference


def _buffer_cfg(c, device, **over):
    return SimpleNamespace(**{**vars(c), "device": device, "train_steps": c.capacity, "max_buffer_size": 10**9, **over})


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_ref_rollout_matches_reference(name):
    c = case_cfg()
    g = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    ref = RefRollout(c)
    seen = []

    def sample(k, seed):
        obs, next_obs, action, reward, idxs, weights, _ = ref.sample(uniforms(c, seed))
        assert np.array_equal(idxs.numpy(), g[f"s{k}_idxs"]), k
        for key, v in dict(obs=obs, next_obs=next_obs, action=action, reward=reward, weights=weights).items():
            assert np.array_equal(v.numpy(), g[f"s{k}_{key}"]), (k, key)
        seen.append(k)
        return idxs

    for step, op in run_schedule(name, ref, sample, c):
        assert np.array_equal(ref._priorities.numpy(), g[f"t{step}_priorities"]), (step, op)
        assert [ref.idx, int(ref._full)] == g[f"t{step}_idx_full"].tolist(), (step, op)
    assert len(seen) == int(g["nsamples"]) == 3


def test_schedules_cover_the_cases():
    """What the schedules are there for, checked on the restatement: a sample while not full; idx reaching 0 by an
    exact fit (`add` sets _full) in one and by a dropped episode (tail zeroed, nothing stored) in the other; two adds
    of different lengths while full."""
    c = case_cfg()
    for name in SCHEDULES:
        ref = RefRollout(c)
        full_at_sample, dropped, adds_while_full = [], [], []

        def sample(k, seed):
            full_at_sample.append(ref._full)
            return ref.sample(uniforms(c, seed))[4]

        stored, was_full = 0, False
        for step, op in run_schedule(name, ref, sample, c):
            if op[0] == "add":
                if len(ref._last_obs) == stored:   # not stored
                    dropped.append(op[2])
                    tail = sum(n for o, _, n in (q for q in SCHEDULES[name][:step] if q[0] == "add"))
                    assert ref.idx == 0 and ref._full and (ref._priorities[tail:] == 0).all()
                elif was_full:
                    adds_while_full.append(op[2])
                stored = len(ref._last_obs)
            was_full = ref._full
        assert full_at_sample == [False, True, True]
        assert dropped == ([10] if name == "drop" else []) and adds_while_full == [10, 5]
    lens = [op[2] for op in SCHEDULES["wrap"] if op[0] == "add"]
    assert lens[:4] == [7, c.horizon + 1, c.horizon, 20] and sum(lens[:5]) == c.capacity


def test_rollout_refuses_pixels():
    from tdmpc_amd.replay import RolloutBuffer
    with pytest.raises(NotImplementedError, match="modality"):
        RolloutBuffer(_buffer_cfg(case_cfg(), "cpu", modality="pixels"))


def test_rollout_add_refuses_an_episode_that_does_not_fit():
    """`add` called directly (not `+=`, which drops such an episode): the reference fails on a shape mismatch."""
    from tdmpc_amd.replay import RolloutBuffer
    c = case_cfg()
    buf = RolloutBuffer(_buffer_cfg(c, "cpu"))
    assert buf.capacity == 64 and buf._obs.shape == (65, 5) and buf._last_obs == [] and buf.graph_safe
    assert (buf._obs == 0).all()
    buf.idx = 60   # as after 60 stored transitions
    with pytest.raises(ValueError, match=r"7 .* 4 "):
        buf.add(episode(c, 1, 7))
    assert buf.idx == 60 and not buf._full and buf._last_obs == []


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_gpu_rollout_matches_ref(name):
    from tdmpc_amd.replay import RolloutBuffer
    c = case_cfg()
    buf, ref = RolloutBuffer(_buffer_cfg(c, "cuda")), RefRollout(c)
    want = {}

    def ref_sample(k, seed):
        want[k] = ref.sample(uniforms(c, seed))
        return want[k][4]

    ref_state = [(ref._priorities.clone(), ref.idx, ref._full) for _ in run_schedule(name, ref, ref_sample, c)]

    def sample(k, seed):
        obs, next_obs, action, reward, idxs, weights = buf.sample(u=uniforms(c, seed))
        w_obs, w_next, w_action, w_reward, w_idxs, w_weights, w_used = want[k]
        assert np.array_equal(idxs.cpu().numpy(), w_idxs.numpy()), k
        for key, v, w in (("obs", obs, w_obs), ("next_obs", next_obs, w_next), ("action", action, w_action),
                          ("reward", reward, w_reward)):
            assert v.shape == w.shape and torch.equal(v.cpu(), w), (k, key)
        np.testing.assert_allclose(weights.cpu().numpy(), w_weights.numpy(), rtol=WEIGHT_RTOL, atol=0)
        assert buf.uniforms_used == w_used
        return idxs.clone()

    for step, op in run_schedule(name, buf, sample, c):
        prio, idx, full = ref_state[step]
        assert (buf.idx, buf._full) == (idx, full), (step, op)
        assert torch.equal(buf._priorities.cpu(), prio), (step, op)
    assert len(want) == 3 and len(buf._last_obs) == len(ref._last_obs)


def _cheetah():
    from tdmpc_amd.config import make_cfg
    return make_cfg("cheetah", num_samples=64, num_elites=32, iterations=3, horizon=5, batch_size=52)


@pytest.mark.gpu
def test_gpu_learner_on_rollout_buffer_graph_equals_eager():
    """Twin TDMPC agents (the tests' small cheetah shape) update from twin RolloutBuffers, one by HIP-graph replay
    and one eagerly, across a fill change (a new graph key), a dropped episode (idx 0, _full) and an add while full:
    parameters, priorities and metrics bitwise equal after each update."""
    from tdmpc_amd.replay import RolloutBuffer
    from tdmpc_amd.tdmpc import TDMPC
    from tdmpc_amd.told import synthetic_state_dict
    cfg = _cheetah()
    rc = SimpleNamespace(**{**vars(cfg), "device": "cuda", "train_steps": 300, "max_buffer_size": 10**6,
                            "buffer_shape": tuple(cfg.obs_shape)})
    rs = np.random.RandomState(0)
    O, A = cfg.obs_shape[0], cfg.action_dim
    eps = [Ep(torch.from_numpy(rs.standard_normal((151, O)).astype(np.float32)),
              torch.from_numpy(rs.uniform(-1, 1, (150, A)).astype(np.float32)),
              torch.from_numpy(rs.standard_normal(150).astype(np.float32)), n) for n in (120, 100, 50, 60, 40)]
    runs = []
    for graph in (True, False):
        agent = TDMPC(cfg)
        agent.model.load_state_dict(synthetic_state_dict(cfg, 21))
        agent.model_target.load_state_dict(synthetic_state_dict(cfg, 22))
        agent.learner(graph=graph, warmup=2)
        buf = RolloutBuffer(rc)
        torch.manual_seed(7)
        todo, step, trail = list(eps), 0, []
        # episodes 120 + 100: idx 220; + 50: idx 270; 60 > the 30 left: dropped, idx 0, full; + 40: idx 40, full
        for k, want in ((2, (220, False)), (1, (270, False)), (1, (0, True)), (1, (40, True))):
            for _ in range(k):
                buf += todo.pop(0)
            assert (buf.idx, buf._full) == want
            for _ in range(2):
                step += 1
                m = agent.update(buf, step, sync_metrics=False).clone()
                params = [x.detach().clone() for x in list(agent.model.parameters()) +
                          list(agent.model_target.parameters())]
                trail.append((m, buf._priorities.clone(), params))
        assert len(buf._last_obs) == 4   # the 60-transition episode was not stored
        runs.append((agent, trail))
    (a1, t1), (a2, t2) = runs
    assert a1.learner()._graphs and not a2.learner()._graphs
    for step, ((m1, p1, w1), (m2, p2, w2)) in enumerate(zip(t1, t2)):
        assert torch.isfinite(m1).all(), step
        assert torch.equal(m1, m2), step
        assert torch.equal(p1, p2), step
        assert all(torch.equal(x, y) for x, y in zip(w1, w2)), step


@pytest.mark.gpu
def test_gpu_dog_shaped_rollout_buffer_builds_and_reads():
    """The dog task's batch of 2048 at cfgs/default.yaml's horizon, small observation and action widths: the buffer
    constructs, samples and gathers (with and without replacement)."""
    from tdmpc_amd.config import make_cfg
    from tdmpc_amd.replay import RolloutBuffer
    dog = make_cfg("dog")
    assert dog.batch_size == 2048
    H = make_cfg("cartpole").horizon
    c = SimpleNamespace(modality="state", buffer_shape=(7,), obs_shape=(7,), action_dim=3, batch_size=dog.batch_size,
                        horizon=H, per_alpha=dog.per_alpha, per_beta=dog.per_beta, device="cuda", train_steps=6000,
                        max_buffer_size=10**6)
    buf = RolloutBuffer(c)
    rs = np.random.RandomState(3)
    ep = Ep(torch.from_numpy(rs.standard_normal((1001, 7)).astype(np.float32)),
            torch.from_numpy(rs.uniform(-1, 1, (1000, 3)).astype(np.float32)),
            torch.from_numpy(rs.standard_normal(1000).astype(np.float32)), 1000)
    for full in (False, True):
        for _ in range(3):
            buf += ep
        assert buf._full == full and buf.idx == (0 if full else 3000)
        obs, next_obs, action, reward, idxs, weights = buf.sample()
        buf.check_sample()
        assert obs.shape == (2048, 7) and next_obs.shape == (H + 1, 2048, 7) and action.shape == (H + 1, 2048, 3)
        assert reward.shape == (H + 1, 2048, 1) and idxs.shape == weights.shape == (2048,)
        for v in (obs, next_obs, action, reward, weights):
            assert torch.isfinite(v).all()
        i = idxs.cpu()
        assert (i >= 0).all() and (i < (6000 if full else 3000)).all()
        assert len(set(i.tolist())) == 2048 or not full
        assert torch.equal(next_obs[H].cpu(), buf._obs.cpu()[i + H + 1])
