"""Shared by tests/golden/make_drnn_golden.py and the DSSM tests: the recorded cases of the recurrent-latent planner."""
import numpy as np

from tdmpc_amd.config import make_cfg

DSSM_KEYS = dict(hidden_dim=128, norm_cell=True, plan2expl=False, warmup_len=0)


def drnn_cfg(task, **ov):
    d = dict(DSSM_KEYS)
    d.update(ov)
    return make_cfg(task, **d)


# name -> (cfg, weight seed, obs / hidden seed, [(step, t0, eval_mode)])
#   humanoid: L100 A21 Hd128; step 1e6: H = 5, mixture 0.5 (P = 32): an episode start, a warm start, an eval call
#   cheetah:  L50 A6, a two-step memory that fills and wraps over four calls, no policy rows (mixture 0 at every step)
#   horizon:  step 10000 gives H = 3 at the episode start; at step 17000 the schedule says 4, but a call inside the
#             episode (t0 False) keeps 3 (tdmpc_similarity_drnn.py:193-195)
def cases():
    return {
        "humanoid": (drnn_cfg("humanoid", num_samples=64, num_elites=16, iterations=3, horizon=5), 111, 21,
                     [(10**6, True, False), (10**6, False, False), (10**6, False, True)]),
        "cheetah": (drnn_cfg("cheetah", num_samples=32, num_elites=8, iterations=2, horizon=4, warmup_len=2,
                             mixture_coef=0.0, regularization_schedule="linear(0.0, 0.0, 1, 5000)"), 112, 22,
                    [(10**6, True, False), (10**6, False, False), (10**6, False, False), (10**6, False, True)]),
        "horizon": (drnn_cfg("cheetah", num_samples=32, num_elites=8, iterations=2, horizon=5), 13, 23,
                    [(10000, True, False), (17000, False, False)]),
    }


def case_inputs(cfg, seed, ncalls):
    """Observations [ncalls, obs] and the caller's hidden state [1, Hd] (non-zero, in [-1, 1])."""
    rs = np.random.RandomState(seed)
    obs = rs.standard_normal((ncalls, cfg.obs_shape[0])).astype(np.float32)
    hidden = rs.uniform(-1, 1, (1, cfg.hidden_dim)).astype(np.float32)
    return obs, hidden
