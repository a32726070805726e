"""Generate tests/golden/drnn_icem/*.npz by running the REFERENCE recurrent-latent iCEM planner in this container.

Run once where the reference checkout exists (make_drnn_golden.import_drnn() names its place):
    python tests/golden/make_drnn_icem_golden.py
Imports the reference's src/algorithm/tdmpc_icem_similarity_drnn.py (as `src.algorithm...`, the way it imports its own
models) with make_drnn_golden.import_drnn()'s stub modules plus a `colorednoise` stub whose `powerlaw_psd_gaussian` is
the restated generator of tdmpc_amd/colored_noise.py on numpy's global RandomState (the package is not installed; its
generator is an input, as in make_icem_golden.py). `Module.cuda` is the identity and the agent's `device` is set to
the CPU after construction (the class hard-codes 'cuda'). Each call runs after torch.manual_seed / np.random.seed
(tests/drnn_icem_io.py); the .npz records the inputs, action, returned hidden state, metrics, every iteration's values
(from a wrapper around the reference's estimate_value), `_prev_mean` and `_elite_actions` after each call.

Tie guard, as make_drnn_golden.py: for every iteration of every call the K-th and (K+1)-th values must differ by more
than 1e-3 (1 + |cut|), ten times parity_util.near_tie's window, so that the GPU comparisons on these inputs can
require equal elite sets outright; the call seed bases in tests/drnn_icem_io.py were picked so that this holds
(`--search name` prints the margin of a range of bases).
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
from make_drnn_golden import import_drnn, stub, tie_margin  # noqa: E402
from tdmpc_amd.colored_noise import powerlaw_psd_gaussian  # noqa: E402
from tdmpc_amd.dssm import synthetic_dssm_state_dict  # noqa: E402
from drnn_icem_io import GOLD_DIR, case_inputs, cases  # noqa: E402


def import_icem_drnn():
    import_drnn()
    stub("colorednoise", powerlaw_psd_gaussian=lambda beta, size: powerlaw_psd_gaussian(beta, size))
    import src.algorithm.tdmpc_icem_similarity_drnn as ic
    return ic


def run_case(ic, name, cfg, wseed, iseed, base, calls):
    rc = ref_cfg(cfg)
    rc.train_steps, rc.episode_length, rc.optim_id, rc.pi_lr = 100000, 500, "adam", 1e-3
    agent = ic.TdICemSimDssm(rc)
    agent.device = torch.device("cpu")
    agent.model.load_state_dict(synthetic_dssm_state_dict(cfg, wseed))
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
        torch.manual_seed(base + ci)
        np.random.seed(base + 100 + ci)
        vals.clear()
        a, h, m = agent.plan(obs[ci], torch.from_numpy(hidden), eval_mode=eval_mode, step=step, t0=t0)
        for v in vals:
            worst = min(worst, tie_margin(v.numpy(), cfg.num_elites))
        out[f"c{ci}_obs"] = obs[ci]
        out[f"c{ci}_action"] = a.numpy().copy()
        out[f"c{ci}_hidden"] = h.numpy().copy()
        out[f"c{ci}_metrics"] = np.array([m["external_reward_mean"], m["current_std"]], dtype=np.float64)
        out[f"c{ci}_nvals"] = np.array([len(v) for v in vals])
        out[f"c{ci}_values"] = torch.cat(vals).numpy()
        out[f"c{ci}_prev_mean"] = agent._prev_mean.numpy().copy()
        out[f"c{ci}_elites"] = agent._elite_actions.numpy().copy()
        out[f"c{ci}_horizon"] = np.array(agent.plan_horizon)
    return out, worst


def main():
    ic = import_icem_drnn()
    if len(sys.argv) > 2 and sys.argv[1] == "--search":
        cfg, wseed, iseed, _, calls = cases()[sys.argv[2]]
        for base in range(300, 400):   # (every few bases clear the guard on all of a case's iterations)
            print(base, f"{run_case(ic, sys.argv[2], cfg, wseed, iseed, base, calls)[1]:.3e}", flush=True)
        return
    os.makedirs(GOLD_DIR, exist_ok=True)
    for name, (cfg, wseed, iseed, base, calls) in cases().items():
        out, worst = run_case(ic, name, cfg, wseed, iseed, base, calls)
        assert worst > 1e-3, f"{name}: K-th / (K+1)-th values within {worst:.2e} (1 + |cut|): pick other seeds"
        path = os.path.join(GOLD_DIR, f"{name}.npz")
        np.savez_compressed(path, **out)
        print(f"wrote {path} ({os.path.getsize(path)} bytes), tie margin {worst:.3e}")


if __name__ == "__main__":
    main()
