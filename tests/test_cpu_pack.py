"""The fused weight pack's job table (tdmpc_pack_weights, one launch) bounds-checked on the host for every model
family the packer serves: each job writes inside the packed layout and reads inside its source tensor
(tdmpc_debug_pack_check runs no HIP call, so this holds on the CPU-only driver)."""
import ctypes as C

import pytest

import plan_shapes_ref
from tdmpc_amd import _lib
from tdmpc_amd.config import make_cfg
from tdmpc_amd.told import TOLD


@pytest.mark.parametrize("task,kw", [("humanoid", {}), ("dog", {}), ("cheetah", {}), ("quadruped", {}),
                                     ("humanoid", {"latent_dim": 512}), ("cheetah", {"modality": "pixels"})] +
                         # tests/test_gpu_plan_shapes.py's twelve shapes (action_dim: set on the cfg after make_cfg)
                         [(t, {"action_dim": A, "latent_dim": L, "enc_dim": E})
                          for t, A, L, E in plan_shapes_ref.SHAPES.values()])
def test_pack_jobs_in_bounds(task, kw):
    kw = dict(kw)
    action_dim = kw.pop("action_dim", None)
    cfg = make_cfg(task, **kw)
    if action_dim is not None:
        cfg.action_dim = action_dim
    sd = TOLD(cfg).state_dict()
    L = _lib.lib()
    dims = _lib.dims_from_cfg(cfg, max_batch=1)
    n = len(sd)
    assert n == L.tdmpc_num_param_tensors(C.byref(dims))
    numel = (C.c_int64 * n)(*[v.numel() for v in sd.values()])
    rc = L.tdmpc_debug_pack_check(C.byref(dims), numel, n)
    assert rc > 0, L.tdmpc_last_error().decode()


# (task, latent_dim, hidden_dim): the shapes of tests/test_gpu_drnn_shapes.py (odd and padded k-groups of W_ih, every
# count of gate waves and of the prior's column blocks, the largest LDS footprint), then the two stock ones
DRNN_SHAPES = [("cartpole", 8, 32), ("cheetah", 64, 96), ("quadruped", 90, 160), ("dog", 100, 128),
               ("humanoid", 129, 224), ("humanoid", 200, 192), ("dog", 256, 256),
               ("humanoid", 100, 128), ("cheetah", 50, 128)]


@pytest.mark.parametrize("task,latent,hidden", DRNN_SHAPES)
def test_drnn_pack_jobs_in_bounds(task, latent, hidden):
    """tdmpc_drnn_pack_weights' job table (the shared heads' jobs, then the DSSM regions'): the head jobs write inside
    the planner layout, the DSSM jobs behind it, inside the packed size and into disjoint ranges (one launch runs them
    unordered), and every job reads inside its tensor."""
    from drnn_io import drnn_cfg
    from tdmpc_amd.dssm import DSSM, float_tensors
    cfg = drnn_cfg(task, latent_dim=latent, hidden_dim=hidden, num_samples=32, num_elites=8, iterations=1,
                   regularization_schedule="0.5")
    ts = float_tensors(DSSM(cfg).state_dict())
    L = _lib.lib()
    dims = _lib.drnn_dims_from_cfg(cfg, max_batch=2, num_pi=16)
    n = len(ts)
    assert n == L.tdmpc_drnn_num_param_tensors(C.byref(dims))
    numel = (C.c_int64 * n)(*[v.numel() for v in ts])
    rc = L.tdmpc_drnn_debug_pack_check(C.byref(dims), numel, n)
    assert rc > 0, L.tdmpc_last_error().decode()
    assert L.tdmpc_drnn_debug_pack_check(None, numel, n) == -3
    assert L.tdmpc_drnn_debug_pack_check(C.byref(dims), None, n) == -3
    assert L.tdmpc_drnn_debug_pack_check(C.byref(dims), numel, n - 1) == -1
    # one float short in any tensor the step kernel's regions read from is noticed (the check reads numel)
    for i in (7, 8, 15, 21):
        short = (C.c_int64 * n)(*[v.numel() - (j == i) for j, v in enumerate(ts)])
        assert L.tdmpc_drnn_debug_pack_check(C.byref(dims), short, n) < 0, i
