"""Generate tests/golden/drnn_update/*.npz by running the REFERENCE `TdICemSimDssm.update` in this container.

Run once where the reference checkout exists (make_drnn_golden.import_drnn() names its place):
    python tests/golden/make_drnn_update_golden.py
Imports the reference's src/algorithm/tdmpc_icem_similarity_drnn.py as make_drnn_icem_golden.py does (rlpyt / gym /
colorednoise stubs, `Module.cuda` the identity, the agent on the CPU) and, for `update`, replaces in that module
  * `create_optimizer` by `torch.optim.Adam(model.parameters(), lr=lr)` (rlpyt's factory is not available),
  * `RunningMeanStd` by gym's class restated: mean 0, var 1, count 1e-4, `update_from_moments` as
    update_mean_var_count_from_moments (tests/drnn_update_ref.py::rms_update_from_moments, batch_count = 1),
  * `torch.Tensor.cuda` by the identity,
and hands `update` a fixed-batch buffer (tests/drnn_update_ref.py::batch) that keeps the priorities it is given.

One deliberate wrapper: `agent.intrinsic_rewards` returns `.float()`. With NumPy 2 the reference's
`intrinsic_reward - reward_threshold` (a float32 array minus a float64 scalar) promotes to float64, the tensor that
reaches `reward_pi` is float64 and `backward()` fails with a dtype error; the reference's pinned stack keeps float32
there. The wrapper restores that dtype and changes nothing else (tests/drnn_update_ref.py restates the same arithmetic).

Per case two consecutive updates at steps 20000 and 20001 (tests/drnn_update_ref.py::STEPS), so the second sees moved
BatchNorm running statistics, Adam moments and RunningMeanStd state. torch.manual_seed(case seed + update index) before
each update fixes the TruncatedNormal draws, which a wrapper around helper._standard_normal records. Per update the .npz
holds the draws, the metrics, the priorities, the intrinsic rewards, the RunningMeanStd state and, for every .grad and
every tensor of the model's and the target's state_dict, the float64 sum, sum of squares and 64 fixed elements (the
tensors themselves are megabytes); the inputs once.

Tie guard: on every row of every `update_pi`, |Q1 - Q2| > 1e-4 (1 + |min Q|), so that a float32 / float64 difference
cannot reroute torch.min's gradient in the GPU comparisons; the seeds in tests/drnn_update_ref.py::CASES were picked so
that this holds.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import ref_cfg  # noqa: E402
from make_drnn_icem_golden import import_icem_drnn  # noqa: E402
from tdmpc_amd.dssm import synthetic_dssm_state_dict  # noqa: E402
import drnn_update_ref as U  # noqa: E402


class RunningMeanStd:
    """gym.wrappers.normalize.RunningMeanStd (shape ())."""

    def __init__(self, epsilon=1e-4, shape=()):
        self.mean = np.zeros(shape, "float64")
        self.var = np.ones(shape, "float64")
        self.count = epsilon

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        assert batch_count == 1
        self.mean, self.var, self.count = U.rms_update_from_moments([self.mean, self.var, self.count], batch_mean,
                                                                    batch_var)


def run_case(ic, name):
    import src.algorithm.helper as h
    cfg = U.case_cfg(name)
    wseed, tseed, bseed, seed = U.CASES[name][5:9]
    ic.create_optimizer = lambda model, optim_id, lr: torch.optim.Adam(model.parameters(), lr=lr)
    ic.RunningMeanStd = RunningMeanStd
    torch.Tensor.cuda = lambda self, *a, **k: self
    agent = ic.TdICemSimDssm(ref_cfg(cfg))
    agent.device = torch.device("cpu")
    agent.model.load_state_dict(synthetic_dssm_state_dict(cfg, wseed))
    agent.model_target.load_state_dict(synthetic_dssm_state_dict(cfg, tseed))

    inner = agent.intrinsic_rewards
    kept = {}

    def intrinsic_rewards(*a):
        kept["intrinsic"] = inner(*a).float()
        return kept["intrinsic"]
    agent.intrinsic_rewards = intrinsic_rewards

    drawn = []
    std_normal = h._standard_normal

    def recording_normal(shape, dtype, device):
        drawn.append(std_normal(shape, dtype=dtype, device=device))
        return drawn[-1].clone()
    h._standard_normal = recording_normal

    tie = [np.inf]
    update_pi = agent.update_pi

    def guarded_update_pi(zs):
        Q = agent.model.Q

        def watched(z, a):
            q1, q2 = Q(z, a)
            with torch.no_grad():
                tie[0] = min(tie[0], float(((q1 - q2).abs() / (1 + torch.min(q1, q2).abs())).min()))
            return q1, q2
        agent.model.Q = watched
        try:
            return update_pi(zs)
        finally:
            del agent.model.Q
    agent.update_pi = guarded_update_pi

    b = U.batch(cfg, bseed)
    buf = U.FakeBuffer(b)
    out = {n: t.numpy() for n, t in zip(("obs", "next_obses", "action", "reward", "idxs", "weights"), b)}
    try:
        for k, step in enumerate(U.STEPS):
            torch.manual_seed(1000 + 10 * seed + k)
            drawn.clear()
            m = agent.update(buf, step)
            assert len(drawn) == 2 * cfg.horizon + 1
            r = dict(metrics=np.array([m[n] for n in U.METRICS], dtype=np.float64), prio=buf.prios[-1].numpy(),
                     intrinsic=kept["intrinsic"].numpy(),
                     rms=np.array([float(agent.reward_rms.mean), float(agent.reward_rms.var),
                                   float(agent.reward_rms.count)]),
                     grads=U.grads_of(agent.model))
            U.record(out, k, r, agent.model, agent.model_target)
            out[f"u{k}_noise"] = torch.stack(drawn).numpy()
            out[f"u{k}_nbt"] = np.array([int(agent.model._dynamics.prior_mlp[1].num_batches_tracked),
                                         int(agent.model._predictor[1].num_batches_tracked)])
    finally:
        h._standard_normal = std_normal
    return out, tie[0]


def main():
    ic = import_icem_drnn()
    os.makedirs(U.GOLD_DIR, exist_ok=True)
    for name in U.RECORDED:
        out, tie = run_case(ic, name)
        assert tie > U.TIE, f"{name}: an update_pi row has |Q1 - Q2| = {tie:.2e} (1 + |Q|): pick other seeds"
        path = os.path.join(U.GOLD_DIR, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes), update_pi tie margin {tie:.3e}; metrics "
              f"{np.round(out['u1_metrics'], 5).tolist()}, nbt {out['u1_nbt'].tolist()}")


if __name__ == "__main__":
    main()
