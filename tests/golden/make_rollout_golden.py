"""Generate tests/golden/rollout/{wrap,drop}.npz by running the REFERENCE RolloutBuffer (helper.py:537-636).

Run once where the reference checkout exists:   python tests/golden/make_rollout_golden.py
The reference buffer runs on the CPU (cfg.device = 'cpu'; `torch.Tensor.cuda` made a no-op, as in
make_replay_golden.py: only placement changes, not the arithmetic). The reference is imported like make_golden.py
does. `buf._obs` is zeroed right after construction: the reference allocates it with torch.empty and reads a row it
never wrote (the newest episode's last window), which this makes deterministic. Each case follows
tests/rollout_ref.py's schedule with `buffer += episode`; every sample() runs right after np.random.seed(s), so
np.random.choice's uniforms are `RandomState(s).random_sample(...)`. The .npz holds each sample's outputs and, after
every step, `_priorities`, `idx` and `_full`.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_golden import import_reference  # noqa: E402
from rollout_ref import SCHEDULES, case_cfg, dup_idxs, episode_arrays, priorities  # noqa: E402


def ref_cfg(c):
    return types.SimpleNamespace(device="cpu", train_steps=c.capacity, max_buffer_size=10**9, modality=c.modality,
                                 obs_shape=c.obs_shape, buffer_shape=c.buffer_shape, episode_length=c.max_len,
                                 action_dim=c.action_dim, batch_size=c.batch_size, horizon=c.horizon,
                                 per_alpha=c.per_alpha, per_beta=c.per_beta)


def main():
    import_reference()
    import algorithm.helper as h
    torch.Tensor.cuda = lambda self, *a, **k: self
    os.makedirs(os.path.join(HERE, "rollout"), exist_ok=True)
    c = case_cfg()
    rc = ref_cfg(c)
    for name, schedule in SCHEDULES.items():
        buf = h.RolloutBuffer(rc)
        buf._obs.zero_()
        out, k, last = {}, 0, None
        for step, op in enumerate(schedule):
            if op[0] == "add":
                obs, act, rew = episode_arrays(c, op[1])
                ep = h.Episode(rc, obs[0])
                ep.obs[:] = torch.from_numpy(obs)
                ep.action[:] = torch.from_numpy(act)
                ep.reward[:] = torch.from_numpy(rew)
                ep._idx = op[2]
                buf += ep
            elif op[0] == "prio":
                buf.update_priorities(dup_idxs(last), torch.from_numpy(priorities(c, op[1])))
            else:
                np.random.seed(op[1])
                obs, next_obs, action, reward, idxs, weights = buf.sample()
                last = idxs
                for key, v in dict(obs=obs, next_obs=next_obs, action=action, reward=reward, idxs=idxs,
                                   weights=weights).items():
                    out[f"s{k}_{key}"] = v.numpy()
                k += 1
            out[f"t{step}_priorities"] = buf._priorities.numpy().copy()
            out[f"t{step}_idx_full"] = np.array([buf.idx, int(buf._full)])
        out["nsamples"] = np.array(k)
        path = os.path.join(HERE, "rollout", f"{name}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path}: {k} samples, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
