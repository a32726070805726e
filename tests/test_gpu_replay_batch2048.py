"""`ReplayBuffer` at batch sizes above 1024, up to the dog task's 2048 (include/tdmpc_replay.h): the two-items-per-thread
instance of the without-replacement kernel, and every other place that sizes by the batch.

Batches 1025 (one thread with two items), 1088 (one wave past 1024) and 2048 (the cap); capacities 4096 and 6144 (two
and three 2048-element scan blocks). The checker is numpy's choice algorithm (oracle.replay_ref.choice) on the device's
own float32 probabilities and the same uniforms, as in tests/test_replay.py::test_gpu_choice_large_buffer: indices equal
in numpy's output order, uniforms consumed equal.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.replay_ref import choice

L, H, OBS, A = 128, 5, 3, 2
ALPHA, BETA = 0.6, 0.4


class _Ep:
    def __init__(self, rs):
        self.obs = torch.from_numpy(rs.standard_normal((L + 1, OBS)).astype(np.float32))
        self.action = torch.from_numpy(rs.uniform(-1, 1, (L, A)).astype(np.float32))
        self.reward = torch.from_numpy(rs.standard_normal(L).astype(np.float32))


def _buffer(B, cap, full):
    from tdmpc_amd.replay import ReplayBuffer
    c = SimpleNamespace(modality="state", obs_shape=(OBS,), action_dim=A, episode_length=L, batch_size=B, horizon=H,
                        per_alpha=ALPHA, per_beta=BETA, frame_stack=1, device="cuda", train_steps=cap,
                        max_buffer_size=10**9, env_horizon=H)
    buf = ReplayBuffer(c, latent_plan=True)
    rs = np.random.RandomState(cap + B)
    for _ in range(cap // L if full else cap // L - 1):
        buf.add(_Ep(rs))
    return buf, rs


def _live(total):
    """Transitions whose window stays inside their episode (add() leaves the last H of each at priority 0)."""
    i = np.arange(total)
    return i[i % L < L - H]


def concentrated(total, rs):
    """Priorities for the without-replacement cases, chosen so that numpy's rounds number at least three and need
    fewer uniforms than the 8 x batch supplied, at every batch here: 64 hot transitions at 1e4, the other live ones
    in [1, 2). With alpha = 0.6 the probabilities span 1e4**0.6 ~ 250 in ratio (far inside the 2^29 exactness bound
    of replay_kernels.hip) and the hot 64 hold ~3/4 of the mass. Round 1 then finds the hot ones and a few hundred
    others; the later rounds draw the rest from a near-uniform remainder and keep colliding."""
    live = _live(total)
    p = rs.uniform(1.0, 2.0, size=live.size).astype(np.float32)
    p[rs.choice(live.size, 64, replace=False)] = 1e4
    return live, p


def rounds_at_least_three(probs, B, u, used):
    """On the oracle alone: round 1 draws B and finds n1 distinct, round 2 draws B - n1; a third round was taken
    exactly when more than B + (B - n1) uniforms were consumed."""
    cdf = np.cumsum(probs.astype(np.float64))
    cdf /= cdf[-1]
    n1 = np.unique(cdf.searchsorted(u[:B], side="right")).size
    return used > B + (B - n1)


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("cap", [4096, 6144])
@pytest.mark.parametrize("B", [1025, 1088, 2048])
def test_gpu_choice_batch_above_1024(B, cap, full):
    buf, rs = _buffer(B, cap, full)
    total = cap if full else buf.idx
    assert buf._full == full and total == (cap if full else cap - L)
    if full:
        idx, p = concentrated(total, rs)
    else:
        idx, p = _live(total), None
        p = rs.exponential(1.0, size=idx.size).astype(np.float32)
    buf.update_priorities(torch.from_numpy(idx), torch.from_numpy(p[:, None]))   # n > 1024: the three-launch path
    u = rs.random_sample(8 * B)
    obs, next_obs, action, reward, idxs, weights = buf.sample(u=u, keep_probs=True)
    probs = buf.last_probs.cpu().numpy()
    want, used = choice(probs, B, not full, u)
    if full:   # on the oracle alone, before comparing
        assert rounds_at_least_three(probs, B, u, used), (used, B)
        assert used <= u.size, (used, u.size)
        assert len(set(want.tolist())) == B
    got = idxs.cpu().numpy()
    assert np.array_equal(got, want)
    assert buf.uniforms_used == used
    w = (total * torch.from_numpy(probs)[torch.from_numpy(want)]) ** (-BETA)
    np.testing.assert_allclose(weights.cpu().numpy(), (w / w.max()).numpy(), rtol=2e-6)
    # the gathered windows are storage rows (live transitions: no episode end inside the first H steps)
    st, i = buf._obs.cpu(), idxs.cpu()
    assert torch.equal(obs.cpu(), st[i])
    assert torch.equal(next_obs[2].cpu(), st[i + 3])
    assert torch.equal(action[H].cpu(), buf._action.cpu()[i + H])
    assert torch.equal(reward[1, :, 0].cpu(), buf._reward.cpu()[i + 1])


@pytest.mark.gpu
def test_gpu_norepl_2048_fewer_nonzero_than_batch_raises():
    """Batch 2048 without replacement with 1500 non-zero priorities: the device flags it and check_sample() raises
    numpy's ValueError; the 1500 with mass are all found."""
    buf, _ = _buffer(2048, 4096, True)
    buf._priorities.zero_()
    hot = torch.arange(0, 1500, dtype=torch.int64) * 2 + 1
    buf.update_priorities(hot, torch.ones(1500, 1))
    *_, idxs, _ = buf.sample()
    with pytest.raises(ValueError, match="Fewer non-zero"):
        buf.check_sample()
    assert set(idxs.cpu().numpy().tolist()[:1500]) == set(hot.tolist())


@pytest.mark.gpu
def test_gpu_update_priorities_2048_last_writer_wins():
    """2048 indices with duplicates (above the one-workgroup path's 1024: three launches), twice: the last
    occurrence wins, as a sequential index_put_ on the CPU."""
    buf, rs = _buffer(2048, 4096, True)
    ref = buf._priorities.cpu().numpy().copy()
    for span in (300, 4096):
        idx = rs.randint(0, span, size=2048)
        v = rs.exponential(1.0, size=(2048, 1)).astype(np.float32)
        assert np.unique(idx).size < 2048
        buf.update_priorities(torch.from_numpy(idx), torch.from_numpy(v))
        for i, k in enumerate(idx):
            ref[k] = np.float32(v[i, 0] + np.float32(1e-6))
        assert np.array_equal(buf._priorities.cpu().numpy(), ref)
