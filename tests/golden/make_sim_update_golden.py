"""Generate tests/golden/sim_update/*.npz and tests/golden/tdmpc_sim_layout.json by running the REFERENCE
`TDMPCSIM.update` in this container.

Run once where the reference checkout exists (make_drnn_golden.import_drnn() names its place):
    python tests/golden/make_sim_update_golden.py
Imports the reference's src/algorithm/tdmpc_similarity.py as make_icem_update_golden.py imports the MLP iCEM agent's file
(rlpyt / gym stubs, `Module.cuda` the identity, the agent on the CPU) and, for `update`, replaces in that module
  * `create_optimizer` by `torch.optim.Adam(model.parameters(), lr=lr)` (rlpyt's factory is not available),
and hands `update` a fixed-batch buffer (tests/drnn_update_ref.py::batch) that keeps the priorities it is given.

Per case two consecutive updates at steps 20000 and 20001 (the first with the EMA), torch.manual_seed(case seed + update
index) before each; a wrapper around helper._standard_normal records the TruncatedNormal draws. Per update the .npz
holds the draws, the metrics, the priorities, `_predictor.1`'s num_batches_tracked and running statistics and, for every
.grad and every tensor of the model's and the target's state_dict, the float64 sum, sum of squares and 64 fixed elements;
the inputs once. Only data: no program text of the reference goes into the files.

Tie guard: on every row of every `update_pi`, |Q1 - Q2| > 1e-4 (1 + |min Q|); the seeds in
tests/sim_update_ref.py::CASES were picked so that this holds.

The layout file is the list of names and shapes of the reference model's state_dict at the humanoid sizes, in order.
"""
from __future__ import annotations

import json
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
from tdmpc_amd.config import make_cfg  # noqa: E402
from tdmpc_amd.icem_mlp import synthetic_icem_mlp_state_dict  # noqa: E402
import sim_update_ref as U  # noqa: E402


def import_sim():
    import_drnn()
    import src.algorithm.tdmpc_similarity as sim
    return sim


def make_agent(sim, cfg):
    sim.create_optimizer = lambda model, optim_id, lr: torch.optim.Adam(model.parameters(), lr=lr)
    torch.Tensor.cuda = lambda self, *a, **k: self
    agent = sim.TDMPCSIM(ref_cfg(cfg))
    agent.device = torch.device("cpu")
    return agent


def run_case(sim, name):
    import src.algorithm.helper as h
    cfg = U.case_cfg(name)
    wseed, tseed, bseed, seed = U.CASES[name][4:8]
    agent = make_agent(sim, cfg)
    agent.model.load_state_dict(synthetic_icem_mlp_state_dict(cfg, wseed))
    agent.model_target.load_state_dict(synthetic_icem_mlp_state_dict(cfg, tseed))

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

    b = U.case_batch(name)
    buf = U.FakeBuffer(b)
    out = {n: t.numpy() for n, t in zip(("obs", "next_obses", "action", "reward", "idxs", "weights"), b)}
    try:
        for k, step in enumerate(U.STEPS):
            torch.manual_seed(1000 + 10 * seed + k)
            drawn.clear()
            m = agent.update(buf, step)
            assert len(drawn) == 2 * cfg.horizon + 1
            r = dict(metrics=np.array([m[n] for n in U.METRICS], dtype=np.float64), prio=buf.prios[-1].numpy(),
                     grads=U.grads_of(agent.model))
            U.record(out, k, r, agent.model, agent.model_target)
            out[f"u{k}_noise"] = torch.stack(drawn).numpy()
    finally:
        h._standard_normal = std_normal
    return out, tie[0]


def write_layout(sim):
    agent = make_agent(sim, make_cfg("humanoid", optim_id="adam", train_steps=100000, episode_length=500))
    lay = {k: list(v.shape) for k, v in agent.model.state_dict().items()}
    path = os.path.join(HERE, "tdmpc_sim_layout.json")
    with open(path, "w") as f:
        json.dump(lay, f, indent=0)
    print(f"wrote {path} ({len(lay)} tensors)")


def main():
    sim = import_sim()
    write_layout(sim)
    os.makedirs(U.GOLD_DIR, exist_ok=True)
    for name in U.RECORDED:
        out, tie = run_case(sim, name)
        assert tie > U.TIE, f"{name}: an update_pi row has |Q1 - Q2| = {tie:.2e} (1 + |Q|): pick other seeds"
        path = os.path.join(U.GOLD_DIR, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes), update_pi tie margin {tie:.3e}; metrics "
              f"{np.round(out['u1_metrics'], 5).tolist()}, nbt {out['u1_nbt'].tolist()}")


if __name__ == "__main__":
    main()
