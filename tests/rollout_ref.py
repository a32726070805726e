"""Shared by tests/golden/make_rollout_golden.py and tests/test_rollout.py: `RefRollout`, a CPU restatement of the
reference's `RolloutBuffer` (helper.py:537-636) with np.random.choice's uniforms taken from an explicit stream
(oracle.replay_ref.choice), and the golden schedules with their deterministic episode / priority data (regenerated
from seeds, so the fixtures under tests/golden/rollout/ hold only recorded outputs). Nothing here touches the GPU.

What the restatement keeps of the reference:
  * `+=`   helper.py:560-569  an episode that does not fit behind idx (idx != 0): `_priorities[idx:] = 0`, idx = 0,
                              `_full = True`, the episode is NOT stored; otherwise add()
  * add    helper.py:571-589  the first len(episode) rows; new priorities = the running max (1.0 for the first), the
                              last min(horizon, len) of them 0; idx = (idx + len) % capacity
  * sample helper.py:608-636  ReplayBuffer's probabilities, choice and weights; next_obs[t] = _obs[idxs + t + 1] with no
                              episode-end fix-up
The reference allocates its storage with torch.empty and never stores an episode's final observation, so the newest
episode's last window reads a row that was never written; here (and in the recording, which zeroes `_obs` right after
construction) that storage starts as zeros.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle.replay_ref import choice

# obs rows are buffer_shape wide (5), not obs_shape (3): a buffer built on the wrong one fails every comparison
CASE = dict(modality="state", buffer_shape=(5,), obs_shape=(3,), action_dim=2, capacity=64, batch_size=8, horizon=2,
            per_alpha=0.6, per_beta=0.4, max_len=40)
# operations: ("add", ep_seed, len) is `buffer += episode` | ("sample", np_seed) | ("prio", seed): update_priorities
# for the last sample's idxs with idxs[3] replaced by idxs[0] (a duplicate index)
_FILL = [("add", 1, 7), ("add", 2, 3), ("add", 3, 2), ("add", 4, 20), ("sample", 101)]   # lens: any, H + 1, H, any
_FULL = [("add", 7, 10), ("add", 8, 5), ("sample", 102), ("prio", 9), ("sample", 103)]   # 10 + 5 overwrite 7, 3, 2 | 20
SCHEDULES = {
    # the fifth episode ends exactly at the capacity: idx wraps to 0 and add() sets _full
    "wrap": _FILL + [("add", 5, 32)] + _FULL,
    # the sixth episode (10 > the 7 left at idx 57) does not fit: the tail is zeroed and the episode dropped
    "drop": _FILL + [("add", 5, 25), ("add", 6, 10)] + _FULL,
}


def case_cfg():
    return SimpleNamespace(**CASE)


class Ep:
    """An episode cut short after `n` transitions: obs [max_len + 1, *buffer_shape], action [max_len, A], reward
    [max_len] like the reference's `Episode`, of which the first n count."""

    def __init__(self, obs, action, reward, n):
        self.obs, self.action, self.reward, self._n = obs, action, reward, n

    def __len__(self):
        return self._n


def episode_arrays(cfg, seed):
    rs = np.random.RandomState(seed)
    obs = rs.standard_normal((cfg.max_len + 1,) + tuple(cfg.buffer_shape)).astype(np.float32)
    action = rs.uniform(-1, 1, size=(cfg.max_len, cfg.action_dim)).astype(np.float32)
    reward = rs.standard_normal(cfg.max_len).astype(np.float32)
    return obs, action, reward


def episode(cfg, seed, n):
    return Ep(*(torch.from_numpy(a) for a in episode_arrays(cfg, seed)), n)


def priorities(cfg, seed):
    return (np.random.RandomState(seed).rand(cfg.batch_size, 1) * 3).astype(np.float32)


def dup_idxs(idxs):
    idxs = idxs.clone()
    idxs[3] = idxs[0]
    return idxs


def uniforms(cfg, seed):
    """The stream np.random.choice reads after np.random.seed(seed) (4 x batch: enough for these cases' rounds)."""
    return np.random.RandomState(seed).random_sample(4 * cfg.batch_size)


def run_schedule(name, buf, sample, cfg=None):
    """Drive `buf` through SCHEDULES[name]. `sample(k, seed)` draws sample k and returns its idxs. Yields
    (step, op) after every operation, for the caller to compare state."""
    cfg = cfg or case_cfg()
    k, last = 0, None
    for step, op in enumerate(SCHEDULES[name]):
        if op[0] == "add":
            buf += episode(cfg, op[1], op[2])
        elif op[0] == "prio":
            buf.update_priorities(dup_idxs(last), torch.from_numpy(priorities(cfg, op[1])))
        else:
            last = sample(k, op[1])
            k += 1
        yield step, op


class RefRollout:
    def __init__(self, cfg):
        self.cfg = cfg
        self.capacity = int(cfg.capacity)
        self._obs = torch.zeros((self.capacity + 1, *cfg.buffer_shape), dtype=torch.float32)
        self._last_obs = []
        self._action = torch.zeros((self.capacity, cfg.action_dim), dtype=torch.float32)
        self._reward = torch.zeros((self.capacity,), dtype=torch.float32)
        self._priorities = torch.ones((self.capacity,), dtype=torch.float32)
        self._eps = 1e-6
        self._full = False
        self.idx = 0

    def __iadd__(self, ep):
        if len(ep) > self.capacity - self.idx and self.idx != 0:
            self._priorities[self.idx:] = 0
            self.idx = 0
            self._full = True
        else:
            self.add(ep)
        return self

    def add(self, ep):
        n, H = len(ep), int(self.cfg.horizon)
        self._obs[self.idx:self.idx + n] = ep.obs[:n]
        self._last_obs.append(ep.obs[-1])
        self._action[self.idx:self.idx + n] = ep.action[:n]
        self._reward[self.idx:self.idx + n] = ep.reward[:n]
        if self._full:
            max_priority = self._priorities.max().item()
        else:
            max_priority = 1.0 if self.idx == 0 else self._priorities[:self.idx].max().item()
        new = torch.full((n,), max_priority)
        new[torch.arange(n) >= n - H] = 0
        self._priorities[self.idx:self.idx + n] = new
        self.idx = (self.idx + n) % self.capacity
        self._full = self._full or self.idx == 0

    def update_priorities(self, idxs, priorities):
        self._priorities[torch.as_tensor(idxs)] = torch.as_tensor(priorities).reshape(-1) + self._eps

    def probs(self):
        pr = (self._priorities if self._full else self._priorities[:self.idx]) ** self.cfg.per_alpha
        return pr / pr.sum()

    def sample(self, u, probs=None):
        """u: float64 uniform stream (numpy order). probs: optional float32 probabilities to use instead of this
        restatement's own. -> (obs, next_obs, action, reward [H+1, B, 1], idxs, weights, uniforms used)."""
        cfg = self.cfg
        probs = torch.as_tensor(self.probs() if probs is None else probs, dtype=torch.float32)
        total = len(probs)
        idx_np, used = choice(probs.numpy(), int(cfg.batch_size), not self._full, np.asarray(u, dtype=np.float64))
        idxs = torch.from_numpy(idx_np)
        weights = (total * probs[idxs]) ** (-cfg.per_beta)
        weights /= weights.max()
        H = int(cfg.horizon)
        obs = self._obs[idxs]
        next_obs = torch.stack([self._obs[idxs + t + 1] for t in range(H + 1)])
        action = torch.stack([self._action[idxs + t] for t in range(H + 1)])
        reward = torch.stack([self._reward[idxs + t] for t in range(H + 1)])
        return obs, next_obs, action, reward.unsqueeze(2), idxs, weights, used
