"""What the GPU tests of the three similarity learners' updates share (tests/test_gpu_drnn_update.py,
test_gpu_drnn_sim_update.py, test_gpu_icem_update.py). `U` is the test's yardstick module (drnn_update_ref,
drnn_sim_update_ref or icem_update_ref)."""
from types import SimpleNamespace

import numpy as np
import torch

_WANT = {}


def yardstick(U, name):
    """The float64 yardstick's two updates (snapshots and zero-mean scales), once per yardstick and case."""
    if (U, name) not in _WANT:
        _WANT[(U, name)] = U.run_ref(name, torch.float64, U.case_noise(name), scales=True)
    return _WANT[(U, name)]


def gpu_learner(U, cls, name, graph=False, warmup=3, **cfg_over):
    """-> (cfg, agent, learner, buffer): learner class `cls` on the HIP path over the case's models and batch."""
    cfg = U.case_cfg(name)
    for k, v in cfg_over.items():
        setattr(cfg, k, v)
    model, target = U.make_models(cfg, name, device="cuda")
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cuda"), planner=None)
    learner = cls(agent, graph=graph, warmup=warmup)
    assert learner.hip
    buf = U.FakeBuffer(tuple(t.cuda() for t in U.case_batch(name)))
    return cfg, agent, learner, buf


def snap(U, agent, learner, buf, metrics, *cfg):
    """One update's results by class (U.snapshot; `metrics`: the values the yardstick records, `cfg` where its snapshot
    takes one)."""
    torch.cuda.synchronize()
    r = dict(metrics=np.array(metrics), prio=buf.prios[-1].cpu().numpy(),
             intrinsic=learner.last["intrinsic"].cpu().numpy(), rms=learner.rms.cpu().numpy(),
             grads=U.grads_of(agent.model))
    return U.snapshot(r, agent.model, agent.model_target, *cfg)


def hold(U, tag, got, want, scales, cfg, floors, k):
    figs = U.figures(got, want, scales, cfg.lr, cfg.tau)
    over = {}
    for cls, (f, where) in figs.items():
        b = U.bound(floors, cls, k)
        print(f"{tag} {cls}: gpu {f:.3e} ({where}), bound {b:.2e}")
        if not f <= b:
            over[cls] = (f, where, b)
    assert not over, (tag, over)


def same(tag, got, ref):
    """The fused-loss tests' comparison: rtol 1e-5, atol 1e-6 of the float64 tensor's largest entry."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().reshape(-1)
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6 * float(ref.abs().max()), msg=lambda m: f"{tag}: {m}")
