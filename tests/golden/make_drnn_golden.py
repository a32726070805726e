"""Generate tests/golden/drnn/drnn_*.npz and tests/golden/dssm_layout.json by running the REFERENCE DSSM planner in this container.

Run once in the build container (where /root/reference exists):   python tests/golden/make_drnn_golden.py
Imports /root/reference/src/algorithm/tdmpc_similarity_drnn.py (as `src.algorithm...`, the way it imports its own
models) with stub modules for its absent imports, like make_icem_golden.py: `rlpyt.utils.tensor`,
`rlpyt.ul.algos.utils.optim_factory` / `scheduler_factory` and `gym.wrappers.normalize.RunningMeanStd` (none used by
plan() on state observations). `Module.cuda` is the identity and the agent's `device` is set to the CPU after
construction (the class hard-codes 'cuda'). Each call runs after torch.manual_seed / np.random.seed; the .npz records
the inputs, actions, metrics, per-iteration values (from a wrapper around the reference's estimate_value) and
`_prev_mean` after each call.

Tie guard: for every iteration of every call the K-th and (K+1)-th values must differ by more than
1e-3 (1 + |cut|), ten times parity_util.near_tie's window, so that no GPU comparison on these inputs can leave through
the near-tie escape; the weight / input seeds in tests/drnn_io.py were picked so that this holds.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import import_reference, ref_cfg  # noqa: E402
from tdmpc_amd.dssm import synthetic_dssm_state_dict  # noqa: E402
from drnn_io import case_inputs, cases  # noqa: E402


def stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def import_drnn():
    import_reference()
    for n in ("rlpyt.utils", "rlpyt.ul.algos", "rlpyt.ul.algos.utils", "gym", "gym.wrappers"):
        sys.modules.setdefault(n, types.ModuleType(n))
    stub("rlpyt.utils.tensor", infer_leading_dims=None, restore_leading_dims=None)
    stub("rlpyt.ul.algos.utils.optim_factory", create_optimizer=lambda **k: None)
    stub("rlpyt.ul.algos.utils.scheduler_factory", create_scheduler=lambda **k: None)
    stub("gym.wrappers.normalize", RunningMeanStd=type("RunningMeanStd", (), {}))
    sys.path.insert(0, "/root/reference")
    import src.algorithm.tdmpc_similarity_drnn as dr
    return dr


def tie_margin(v, K):
    s = np.sort(np.asarray(v, np.float64))[::-1]
    return abs(s[K - 1] - s[K]) / (1 + abs(s[K - 1]))


def run_case(dr, name, cfg, wseed, iseed, calls, write=True):
    rc = ref_cfg(cfg)
    rc.train_steps, rc.episode_length, rc.optim_id, rc.pi_lr = 100000, 500, "adam", 1e-3
    agent = dr.TdMpcSimDssm(rc)
    agent.device = torch.device("cpu")
    sd = synthetic_dssm_state_dict(cfg, wseed)
    agent.model.load_state_dict(sd)
    agent.model.eval()
    agent.std = 0.05
    vals = []
    orig = agent.estimate_value

    def ev(z, actions, hidden):
        v, r = orig(z, actions, hidden)
        vals.append(v.squeeze(1).clone())
        return v, r
    agent.estimate_value = ev
    obs, hidden = case_inputs(cfg, iseed, len(calls))
    out = {"hidden": hidden}
    worst = 1.0
    for ci, (step, t0, eval_mode) in enumerate(calls):
        torch.manual_seed(300 + ci)
        np.random.seed(400 + ci)
        vals.clear()
        a, m = agent.plan(obs[ci], torch.from_numpy(hidden), eval_mode=eval_mode, step=step, t0=t0)
        for v in vals:
            worst = min(worst, tie_margin(v.numpy(), cfg.num_elites))
        out[f"c{ci}_obs"] = obs[ci]
        out[f"c{ci}_action"] = a.numpy().copy()
        out[f"c{ci}_metrics"] = np.array([m["intrinsic_reward_mean"], m["external_reward_mean"], m["current_std"]],
                                         dtype=np.float64)
        out[f"c{ci}_values"] = torch.stack(vals).numpy()
        out[f"c{ci}_prev_mean"] = agent._prev_mean.numpy().copy()
        out[f"c{ci}_horizon"] = np.array(agent.plan_horizon)
    if not write:
        return agent, worst
    assert worst > 1e-3, f"{name}: K-th / (K+1)-th values within {worst:.2e} (1 + |cut|): pick other seeds"
    # (a directory of their own: tests/golden_io.py takes every .npz directly under tests/golden/ that is not a
    # replay / learner / iCEM fixture for a TDMPC.plan case)
    os.makedirs(os.path.join(HERE, "drnn"), exist_ok=True)
    path = os.path.join(HERE, "drnn", f"drnn_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes), tie margin {worst:.3e}")
    return agent, worst


def main():
    dr = import_drnn()
    agent = None
    for name, (cfg, wseed, iseed, calls) in cases().items():
        agent, _ = run_case(dr, name, cfg, wseed, iseed, calls)
        if name == "humanoid":
            lay = {k: list(v.shape) for k, v in agent.model.state_dict().items()}
            with open(os.path.join(HERE, "dssm_layout.json"), "w") as f:
                json.dump(lay, f, indent=0)


if __name__ == "__main__":
    main()
