"""CPU: the DSSM learner ABI (include/tdmpc_drnn_learner.h) without a device -- its version, its sizes, its refusals --
and the yardstick tests/test_gpu_drnn_train.py compares against (tests/drnn_train_ref.py): fp32 against float64 autograd
over the eager `tdmpc_amd.dssm` modules in train() mode."""
import ctypes as C

import numpy as np
import pytest
import torch

import drnn_train_ref as R
from parity_util import close
from tdmpc_amd import _lib

E_DIMS = -1   # TDMPC_E_DIMS (include/tdmpc_hip.h)
FAKE = 0x10000   # a non-null address that a refused call never reads


def _dims(task="humanoid", L=100, Hd=128, **kw):
    d = _lib.drnn_dims_from_cfg(R.cfg_for(task, L, Hd))
    for k, v in kw.items():
        if k == "hidden_dim":
            d.hidden_dim = v
        else:
            setattr(d.base, k, v)
    return d


def _sizes(d, rows):
    s = _lib.DrnnTrainSizes()
    return _lib.lib().tdmpc_drnn_train_sizes_for(C.byref(d), rows, C.byref(s)), s


def _table(n):
    return (C.c_void_p * n)(*([FAKE] * n))


def _next_fwd(d, rows, z=FAKE):
    return _lib.lib().tdmpc_drnn_next_fwd(C.byref(d), _table(22), 22, z, FAKE, FAKE, rows, FAKE, FAKE, FAKE, FAKE,
                                          1 << 40, FAKE, 1 << 40, None)


def _loss_fwd(d, rows, keys=FAKE):
    return _lib.lib().tdmpc_drnn_simloss_fwd(C.byref(d), _table(8), 8, FAKE, keys, rows, FAKE, FAKE, 1 << 40, FAKE,
                                             1 << 40, None)


def test_version_and_pinned_versions():
    L = _lib.lib()
    assert L.tdmpc_drnn_train_version() == 1 == _lib.DRNN_TRAIN_VERSION
    assert L.tdmpc_drnn_version() == 2 and L.tdmpc_abi_version() == 8


def test_sizes_are_monotone_in_rows():
    for task, L, Hd in R.SHAPES + [R.STOCK[:3]]:
        d = _dims(task, L, Hd)
        prev = (0, 0, 0)
        for rows in (2, 3, 33, 128, 129, 130, 512, 2560, 4096):
            rc, s = _sizes(d, rows)
            assert rc == 0
            cur = (s.next_saved_floats, s.loss_saved_floats, s.workspace_floats)
            assert all(c >= p for c, p in zip(cur, prev)) and cur[0] > prev[0] and cur[1] > prev[1], (task, rows)
            prev = cur


@pytest.mark.parametrize("what,dims,rows", [
    ("one row", {}, 1), ("4097 rows", {}, 4097), ("Hd 48", dict(hidden_dim=48), 33),
    ("mlp_dim 256", dict(mlp_dim=256), 33)])
def test_unsupported_shapes_are_refused_without_a_device(what, dims, rows):
    d = _dims(**dims)
    L = _lib.lib()
    for rc in (_sizes(d, rows)[0], _next_fwd(d, rows), _loss_fwd(d, rows)):
        assert rc == E_DIMS, what
        assert L.tdmpc_last_error(), what


def test_null_input_pointer_is_refused_without_a_device():
    d = _dims()
    L = _lib.lib()
    assert _next_fwd(d, 33, z=None) == E_DIMS and b"z is null" in L.tdmpc_last_error()
    assert _loss_fwd(d, 33, keys=None) == E_DIMS and b"keys is null" in L.tdmpc_last_error()
    t = _table(22)
    t[8] = None
    assert L.tdmpc_drnn_next_fwd(C.byref(d), t, 22, FAKE, FAKE, FAKE, 33, FAKE, FAKE, FAKE, FAKE, 1 << 40, FAKE,
                                 1 << 40, None) == E_DIMS and L.tdmpc_last_error()


_YARD = {}


def _yardsticks(case):
    if case not in _YARD:
        cfg, d = R.case_data(*case)
        m64, m32 = R.make_model(cfg, torch.float64), R.make_model(cfg, torch.float32)
        names = [k for k, _ in m64.named_parameters() if k.startswith(("_dynamics", "_reward"))]
        lnames = [k for k, _ in m64.named_parameters() if k.startswith("_predictor")]
        pre = R.PreBN(m64)
        w = (R.run_next(m64, m64.next, d, names), R.run_loss(m64, lambda q, k: R.similarity_loss(m64, q, k), d, lnames))
        sc = pre.scales()
        g = (R.run_next(m32, m32.next, d, names), R.run_loss(m32, lambda q, k: R.similarity_loss(m32, q, k), d, lnames))
        _YARD[case] = (w, g, sc)
    return _YARD[case]


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "-".join(map(str, c)))
def test_fp32_yardstick_meets_the_forward_bound(case):
    """The float32 and the float64 eager modules agree on z', h', r, the similarity loss and the updated running
    statistics within parity_util.close (1e-5 + 1e-4 |ref|), so the GPU tests' forward bound is reachable in fp32
    (measured: at most 0.19 of the bound on these cases); num_batches_tracked moves by one."""
    want, got, _ = _yardsticks(case)
    for w, g in zip(want, got):
        assert w["nbt"] == g["nbt"] == 1
        for grp in ("out", "stats"):
            for k in w[grp]:
                assert close(g[grp][k], w[grp][k]).all(), (case, k, np.abs(g[grp][k] - w[grp][k]).max())


def test_fp32_gradient_error_the_gpu_bound_is_derived_from():
    """Prints, per case, the largest gradient figure (max |fp32 - f64| / max |f64| per tensor, drnn_train_ref.figure)
    that fp32 CPU autograd shows against float64 autograd. Measured when this test was written:

        rows 2 (BatchNorm over two rows: xhat = +-1, 1 / std up to ~300, every rounding error amplified):
            cartpole 2.4e-05, cheetah 3.9e-05 (_dynamics.gru_cell.ln_reset.weight), humanoid 2.5e-05, dog 1.6e-05
        rows 33, 130, 512: between 5.9e-07 and 1.01e-06 (dog rows 33, _dynamics.gru_cell.ln_reset.weight)
        three steps through time (cheetah, rows 33): 9.8e-07 (_dynamics.prior_mlp.0.weight)

    tests/test_gpu_drnn_train.py takes 8 x the largest of each group as its bounds (BOUND_ROWS2, BOUND_REST); this test
    holds the fp32 yardstick itself to those bounds, so a change of the yardstick or of the cases that moves the figures
    by a large factor shows up here."""
    from test_gpu_drnn_train import BOUND_REST, BOUND_ROWS2
    worst = {2: 0.0, 0: 0.0}
    for case in R.CASES:
        want, got, sc = _yardsticks(case)
        figs = R.grad_figures(got[0], want[0], sc)
        figs.update({"loss:" + k: v for k, v in R.grad_figures(got[1], want[1], sc).items()})
        k = max(figs, key=figs.get)
        print(f"{case}: largest fp32 CPU gradient figure {figs[k]:.3e} ({k})")
        grp = 2 if case[3] == 2 else 0
        worst[grp] = max(worst[grp], figs[k])
    cfg, d = R.bptt_data()
    m64, m32 = R.make_model(cfg, torch.float64), R.make_model(cfg, torch.float32)
    names = [k for k, _ in m64.named_parameters() if k.startswith(("_dynamics", "_reward", "_predictor"))]
    pre = R.PreBN(m64)
    w = R.run_bptt(m64, m64.next, lambda q, k: R.similarity_loss(m64, q, k), d, names)
    sc = pre.scales()
    g = R.run_bptt(m32, m32.next, lambda q, k: R.similarity_loss(m32, q, k), d, names)
    figs = R.grad_figures(g, w, sc)
    k = max(figs, key=figs.get)
    print(f"through time {R.BPTT}: largest fp32 CPU gradient figure {figs[k]:.3e} ({k})")
    worst[0] = max(worst[0], figs[k])
    assert worst[2] <= BOUND_ROWS2 and worst[0] <= BOUND_REST, worst
