"""Device time of one replay `sample()` as the learners run it (captured in a HIP graph, replayed): `ReplayBuffer` at
batch 512 and 2048 and `RolloutBuffer` at batch 512, humanoid widths (obs 67, A 21), capacity 250k, H + 1 = 6-step
windows, random priorities on 50k transitions; not full (with replacement) and full (without). Prints one JSON line
(--out FILE also writes it). A tree that lacks a leg (no RolloutBuffer, a refused batch size) reports it as null, so the
same script times a tree from before those existed.

    python tools/replay_bench.py [--trials 5] [--replays 200] [--out FILE]

Each trial replays a graph of 20 samples `--replays` times between two synchronisations (4000 samples per trial);
the figure per leg is the median trial, with the fastest and slowest next to it."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tdmpc_amd import replay

L, CAP, H, OBS, A = 500, 250_000, 5, 67, 21
PER_GRAPH = 20


class Ep(SimpleNamespace):
    def __len__(self):
        return L


def build(kind, B, full, rs):
    """-> a filled buffer, or None where this tree cannot build it."""
    cls = getattr(replay, kind, None)
    if cls is None:
        return None
    rc = SimpleNamespace(device="cuda", modality="state", obs_shape=(OBS,), buffer_shape=(OBS,), action_dim=A,
                         episode_length=L, train_steps=CAP, max_buffer_size=10**6, batch_size=B, horizon=H,
                         env_horizon=H, per_alpha=0.6, per_beta=0.4, frame_stack=1)
    try:
        buf = cls(rc, latent_plan=True) if kind == "ReplayBuffer" else cls(rc)
    except ValueError:   # "unsupported replay buffer dims"
        return None
    ep = Ep(obs=torch.from_numpy(rs.standard_normal((L + 1, OBS)).astype(np.float32)),
            action=torch.from_numpy(rs.uniform(-1, 1, (L, A)).astype(np.float32)),
            reward=torch.from_numpy(rs.standard_normal(L).astype(np.float32)))
    for _ in range(CAP // L if full else CAP // L - 1):
        buf.add(ep)
    total = CAP if full else buf.idx
    r = rs.randint(0, total // L * (L - H), 50_000)   # outside the masked last H steps of each episode
    buf.update_priorities(torch.from_numpy((r // (L - H)) * L + r % (L - H)),
                          torch.from_numpy(rs.exponential(1.0, (50_000, 1)).astype(np.float32)))
    return buf


def time_sample(buf, trials, replays):
    for _ in range(5):
        buf.sample()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(PER_GRAPH):
            buf.sample()
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(trials):
        t = time.perf_counter()
        for _ in range(replays):
            g.replay()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t) / (replays * PER_GRAPH) * 1e6)
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "replay_bench needs a GPU"
    out = {"config": f"capacity {CAP}, window H+1={H + 1}, obs {OBS}, A {A}, alpha 0.6, beta 0.4; graph of "
                     f"{PER_GRAPH} samples x {a.replays} replays per trial, {a.trials} trials",
           "device": torch.cuda.get_device_name(0)}
    for kind, B in (("ReplayBuffer", 512), ("ReplayBuffer", 2048), ("RolloutBuffer", 512)):
        for full in (False, True):
            buf = build(kind, B, full, np.random.RandomState(0))
            key = f"{kind}_b{B}_{'full' if full else 'not_full'}"
            out[key] = None if buf is None else time_sample(buf, a.trials, a.replays)
            del buf
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
