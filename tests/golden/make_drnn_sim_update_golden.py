"""Generate tests/golden/drnn_sim_update/*.npz by running the REFERENCE `TdMpcSimDssm.update` on the CPU.

Run once where the reference checkout exists (make_drnn_golden.import_drnn() names its place):
    python tests/golden/make_drnn_sim_update_golden.py
Imports the reference's src/algorithm/tdmpc_similarity_drnn.py as make_drnn_golden.py does (rlpyt / gym stubs,
`Module.cuda` the identity, the agent on the CPU) and, for `update`, replaces in that module
  * `create_optimizer` by `torch.optim.Adam(model.parameters(), lr=lr)` (rlpyt's factory is not available),
  * `RunningMeanStd` by gym's class restated (make_drnn_update_golden.RunningMeanStd),
  * `infer_leading_dims` / `restore_leading_dims` (rlpyt.utils.tensor, stubbed as None by import_drnn) by their
    meaning for the one way `intrinsic_rewards` calls them: a [T, B, L] tensor with one feature dimension,
  * `torch.Tensor.cuda` by the identity,
sets cfg.device = "cpu" (the augmentation's `.to(cfg.device)`; make_golden.ref_cfg) and hands `update` a fixed-batch
buffer (tests/drnn_update_ref.py::batch) that keeps the priorities it is given.

One deliberate wrapper, as in make_drnn_update_golden.py: `agent.intrinsic_rewards` returns `.float()` (with NumPy 2 the
reference's float32 array minus a float64 scalar promotes to float64 and `backward()` fails on the dtype; the
reference's pinned stack keeps float32 there).

Per case two consecutive updates at steps 20000 and 20001 (tests/drnn_sim_update_ref.py::STEPS). torch.manual_seed(case
seed + update index) before each update fixes the draws: a wrapper around helper._standard_normal records the
2 (H - W) + 1 TruncatedNormal draws (u{k}_noise), one around the augmentation's `noise_dist.sample` the H added noises
(u{k}_aug). Per update the .npz holds the draws, the metrics, the priorities, the intrinsic rewards, the
RunningMeanStd state, both BatchNorms' num_batches_tracked and, for every .grad and every tensor of the model's and
the target's state_dict, the float64 sum, sum of squares and 64 fixed elements; the inputs once.

Tie guard: on every row of every `update_pi` and every TD target, |Q1 - Q2| > 1e-4 (1 + |min Q|), so that a float32 /
float64 difference cannot flip torch.min in the GPU comparisons; the seeds in tests/drnn_sim_update_ref.py::CASES were
picked so that this holds.
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
from make_drnn_golden import import_drnn  # noqa: E402
from make_drnn_update_golden import RunningMeanStd  # noqa: E402
from tdmpc_amd.dssm import synthetic_dssm_state_dict  # noqa: E402
import drnn_sim_update_ref as U  # noqa: E402


def infer_leading_dims(tensor, dim):
    """rlpyt.utils.tensor.infer_leading_dims for a [T, B, *dim dims] tensor -> (lead_dim, T, B, shape)."""
    lead_dim = tensor.dim() - dim
    assert lead_dim == 2
    T, B = tensor.shape[:2]
    return lead_dim, T, B, tensor.shape[lead_dim:]


def restore_leading_dims(tensor, lead_dim, T=1, B=1):
    assert lead_dim == 2
    return tensor.view((T, B) + tensor.shape[1:])


def run_case(dr, name):
    import src.algorithm.helper as h
    cfg = U.case_cfg(name)
    wseed, tseed, bseed, seed = U.CASES[name][6:10]
    H, W = cfg.horizon, cfg.warmup_len
    dr.create_optimizer = lambda model, optim_id, lr: torch.optim.Adam(model.parameters(), lr=lr)
    dr.RunningMeanStd = RunningMeanStd
    dr.infer_leading_dims, dr.restore_leading_dims = infer_leading_dims, restore_leading_dims
    torch.Tensor.cuda = lambda self, *a, **k: self
    agent = dr.TdMpcSimDssm(ref_cfg(cfg))
    agent.device = torch.device("cpu")
    agent.model.load_state_dict(synthetic_dssm_state_dict(cfg, wseed))
    agent.model_target.load_state_dict(synthetic_dssm_state_dict(cfg, tseed))

    inner = agent.intrinsic_rewards
    kept = {}

    def intrinsic_rewards(*a):
        kept["intrinsic"] = inner(*a).float()
        return kept["intrinsic"]
    agent.intrinsic_rewards = intrinsic_rewards

    drawn, added = [], []
    std_normal = h._standard_normal

    def recording_normal(shape, dtype, device):
        drawn.append(std_normal(shape, dtype=dtype, device=device))
        return drawn[-1].clone()
    h._standard_normal = recording_normal

    dist = agent.dyna_aug.noise_dist

    class RecordingDist:
        def sample(self, shape):
            added.append(dist.sample(shape))
            return added[-1].clone()
    agent.dyna_aug.noise_dist = RecordingDist()

    # the tie guard: every torch.min(Q1, Q2) of the update (the TD targets on the target model, update_pi on the model)
    tie = [np.inf]

    def watch(model):
        Q = model.Q

        def watched(z, a):
            q1, q2 = Q(z, a)
            # (the update's own Q1 / Q2 on the model enter the losses one by one, not through torch.min: Q tracks grad)
            if model is agent.model_target or not next(model._Q1.parameters()).requires_grad:
                with torch.no_grad():
                    tie[0] = min(tie[0], float(((q1 - q2).abs() / (1 + torch.min(q1, q2).abs())).min()))
            return q1, q2
        model.Q = watched
    watch(agent.model)
    watch(agent.model_target)

    b = U.case_batch(name)
    buf = U.FakeBuffer(b)
    out = {n: t.numpy() for n, t in zip(("obs", "next_obses", "action", "reward", "idxs", "weights"), b)}
    try:
        for k, step in enumerate(U.STEPS):
            torch.manual_seed(1000 + 10 * seed + k)
            drawn.clear()
            added.clear()
            m = agent.update(buf, step)
            assert len(drawn) == 2 * (H - W) + 1 and len(added) == H, (len(drawn), len(added))
            assert set(m) == set(U.METRICS[:7]) | {"mixture_coef"}, sorted(m)
            r = dict(metrics=np.array([m[n] for n in U.METRICS[:7]] + [float(kept["intrinsic"].mean())],
                                      dtype=np.float64),
                     prio=buf.prios[-1].numpy(), intrinsic=kept["intrinsic"].numpy(),
                     rms=np.array([float(agent.reward_rms.mean), float(agent.reward_rms.var),
                                   float(agent.reward_rms.count)]),
                     grads=U.grads_of(agent.model))
            U.record(out, k, r, agent.model, agent.model_target)
            out[f"u{k}_noise"] = torch.stack(drawn).numpy()
            out[f"u{k}_aug"] = torch.stack(added).numpy()
            out[f"u{k}_nbt"] = np.array([int(agent.model._dynamics.prior_mlp[1].num_batches_tracked),
                                         int(agent.model._predictor[1].num_batches_tracked)])
            out[f"u{k}_std"] = np.array(agent.std)
    finally:
        h._standard_normal = std_normal
    return out, tie[0]


def main():
    dr = import_drnn()
    os.makedirs(U.GOLD_DIR, exist_ok=True)
    for name in U.RECORDED:
        out, tie = run_case(dr, name)
        assert tie > U.TIE, f"{name}: a row has |Q1 - Q2| = {tie:.2e} (1 + |Q|): pick other seeds"
        path = os.path.join(U.GOLD_DIR, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes), tie margin {tie:.3e}; metrics "
              f"{np.round(out['u1_metrics'], 5).tolist()}, nbt {out['u1_nbt'].tolist()}")


if __name__ == "__main__":
    main()
