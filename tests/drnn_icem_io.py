"""Shared by tests/golden/make_drnn_icem_golden.py and the iCEM DSSM tests: the recorded cases of the recurrent-latent
iCEM planner (tests/golden/drnn_icem/*.npz)."""
import os

import numpy as np

from drnn_io import case_inputs, drnn_cfg  # noqa: F401

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drnn_icem")


# name -> (cfg, weight seed, obs / hidden seed, call seed base, [(step, t0, eval_mode)]); call ci runs after
# torch.manual_seed(base + ci) and np.random.seed(base + 100 + ci)
#   humanoid: L100 A21 Hd128, coloured noise (beta 2.5); step 1e6: H = 5, mixture 0.5. Candidates per iteration
#             [96, 76, 60] at the episode start and [100, 80, 64] afterwards (N_i = 64, 51, 40; P_i = 32, 25, 20; E = 4):
#             N_i + E_i = 55 and 44 are no multiples of 32. An episode start, two warm calls with reuse, an eval call.
#   cheetah:  L50 A6, white noise (noise_beta 0); a t0 call at step 10000 (H = 3), a warm call, then a second t0 call at
#             step 17000 on an agent that has elites: the horizon grows to 4 and no iteration reuses anything.
def cases():
    return {
        "humanoid": (drnn_cfg("humanoid", num_samples=64, num_elites=16, iterations=3, horizon=5), 111, 21, SEEDS["humanoid"],
                     [(10**6, True, False), (10**6, False, False), (10**6, False, False), (10**6, False, True)]),
        "cheetah": (drnn_cfg("cheetah", num_samples=32, num_elites=8, iterations=2, horizon=5, noise_beta=0.0), 13, 23,
                    SEEDS["cheetah"], [(10000, True, False), (10000, False, False), (17000, True, False)]),
    }


# call seed bases picked so that the generator's tie guard holds (make_drnn_icem_golden.py)
SEEDS = {"humanoid": 317, "cheetah": 1100}


def load(name):
    return np.load(os.path.join(GOLD_DIR, f"{name}.npz"))
