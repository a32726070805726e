"""GPU: the state learner's update at every hidden width the engine admits (256 / 512 / 1024), and at 384 on the
autograd learner, against the float64 oracle (oracle/learner_ref.py::RefLearner, dtype=float64, the same batch and
the same 2H + 1 TruncatedNormal draws per update).

After each of two updates (EMA on the second): the seven metrics, the priorities, every parameter's .grad per tensor
as it stands after the update (the main tensors' is what the main step left after clipping, the _pi.* tensors' what
update_pi left), and every parameter and target tensor. Parameters keep tests/test_learner.py::_params_close's
structure: at most 2 lr everywhere (what Adam guarantees) and a share of at least SHARE of each tensor inside
1e-6 + 1e-4 |f64|. Everything else is bounded by 8 x its float32 CPU floor, never below 1e-6;
gradient figure: max |got - f64| / max |f64| per tensor, the largest over the tensors.

FLOOR holds, per case and per class + update number, the largest figure float32 RefLearner on the CPU shows against
the float64 one over 1, 2, 4 and 8 threads; tests/test_learner_widths_cpu.py recomputes it and holds these constants
within 2 x. The second update has floors of its own: it starts from parameters that already differ by Adam's first
step on the elements whose gradient is ~0. The cases' floors differ by more than 4 x, so each case is its own group.
The MI355X figures in the comments are information, not bounds.
"""
import pytest
import torch

import learner_widths_ref as W
from lg_rows_ref import bound
from tdmpc_amd import learner_engine

# float32 CPU floors (learner_widths_ref.measure_floors). MI355X, largest per-tensor gradient figure at update 1 / 2:
# w256-ragged 3.6e-7 / 2.3e-6, w256-split 9.9e-7 / 2.7e-6, w512-ragged 1.1e-6 / 2.0e-5, w1024-ragged 8.4e-7 / 2.0e-4,
# w1024-split 5.8e-7 / 2.5e-5, w512-clipped 5.3e-7 / 7.0e-6, w384-autograd 3.9e-6 / 6.5e-5; golden-cartpole 7.2e-6,
# full-humanoid 4.1e-7, full-dog 3.9e-7, full-cheetah 6.4e-7; metrics at most 6.1e-6, priorities 1.8e-6; the smallest
# tight share 0.99994
FLOOR = {
    "w256-ragged": {"metrics1": 1.2e-07, "metrics2": 2.2e-07,
                    "prio1": 2.6e-07, "prio2": 3.3e-07, "grad1": 5.8e-07, "grad2": 2.1e-05},
    "w256-split": {"metrics1": 1.5e-07, "metrics2": 5.7e-07,
                   "prio1": 2.5e-07, "prio2": 1.8e-06, "grad1": 4.5e-06, "grad2": 0.00012},
    "w512-ragged": {"metrics1": 1.5e-06, "metrics2": 2.9e-06,
                    "prio1": 2.9e-07, "prio2": 2e-06, "grad1": 8.7e-07, "grad2": 2.5e-05},
    "w1024-ragged": {"metrics1": 1.3e-05, "metrics2": 1.1e-05,
                     "prio1": 4.8e-07, "prio2": 2.4e-06, "grad1": 7.9e-06, "grad2": 0.00034},
    "w1024-split": {"metrics1": 1.3e-05, "metrics2": 1.3e-05,
                    "prio1": 3.6e-07, "prio2": 1.9e-06, "grad1": 9.1e-06, "grad2": 3.5e-05},
    "w512-clipped": {"metrics1": 1.5e-06, "metrics2": 1.5e-06,
                     "prio1": 2.9e-07, "prio2": 2e-06, "grad1": 2.4e-06, "grad2": 1.3e-05},
    "w384-autograd": {"metrics1": 5.8e-07, "metrics2": 2.3e-06,
                      "prio1": 3.6e-07, "prio2": 1.5e-06, "grad1": 1.8e-06, "grad2": 6.7e-05},
    "golden-cartpole": {"metrics1": 1.2e-06, "prio1": 2.8e-07, "grad1": 3.9e-05},
    "full-humanoid": {"metrics1": 1.6e-06, "prio1": 2.7e-07, "grad1": 7.3e-07},
    "full-dog": {"metrics1": 1.4e-06, "prio1": 3.1e-07, "grad1": 1.2e-06},
    "full-cheetah": {"metrics1": 1.6e-06, "prio1": 3.2e-07, "grad1": 1.4e-06},
}
SHARE = {k: 0.999 for k in W.CASES}     # the float32 CPU run stays above it in every case


class _DeviceBatchBuffer:
    """Hands out one fixed batch (already on the device) and keeps the priorities it is given."""

    def __init__(self, b, device="cuda"):
        self.b = tuple(x.to(device) for x in b)
        self.prio = torch.zeros(self.b[0].shape[0], 1, device=device)

    def sample(self):
        return self.b

    def update_priorities(self, idxs, p):
        self.prio.copy_(p)


def gpu_snapshot(agent, buf, m):
    return W.snapshot(m, buf.prio, {k: p.grad for k, p in agent.model.named_parameters()},
                      agent.model.state_dict(), agent.model_target.state_dict())


def check_against_float64(name, k, got, classes=W.CLASSES):
    """One update's snapshot against the float64 oracle's, class by class; prints every figure before it asserts."""
    with torch.random.fork_rng(devices=[]):   # (building a case's model seeds torch's generator: keep the caller's)
        ref = W.oracle64(name, 2 if name in W.WIDTH_CASES else 1)[k]
    f, worst = W.figures(got, ref)
    for c in classes:
        b = bound(FLOOR[name][f"{c}{k + 1}"])
        print(f"{name} update {k + 1} {c}: {f[c]:.3g} (bound {b:.3g})" + (f" [{worst}]" if c == "grad" else ""))
    for c in classes:
        assert f[c] <= bound(FLOOR[name][f"{c}{k + 1}"]), (name, k + 1, c, f[c], worst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", W.WIDTH_CASES)
def test_gpu_update_matches_float64_at_every_width(name):
    from tdmpc_amd.tdmpc import TDMPC
    cfg, sd, sdt, b, noise = W.case_inputs(name)
    agent = TDMPC(cfg)
    agent.model.load_state_dict(sd)
    agent.model_target.load_state_dict(sdt)
    if cfg.mlp_dim == 384:      # off the row kernels' widths: refused by supported(), the learner runs on autograd
        assert not learner_engine.supported(cfg) and agent.learner().engine is None
    else:
        assert learner_engine.supported(cfg) and agent.learner().engine is not None
    buf = _DeviceBatchBuffer(b)
    for k in range(2):
        m = agent.update(buf, k + 1, noise=noise[k])
        got = gpu_snapshot(agent, buf, m)
        ref = W.oracle64(name)[k]
        if k == 0:
            assert (ref["metrics"][6] > cfg.grad_clip_norm) == (name == "w512-clipped")   # clipped only there
        check_against_float64(name, k, got)
        print(f"{name} update {k + 1} tight share: {W.tight_share(got, ref):.5f}")
        W.params_close(got, ref, cfg.lr, SHARE[name])
