"""The yardstick of the gate entry points (include/tdmpc_drnn_engine.h): `NormGRUCell.forward`'s expressions
(tdmpc_amd/dssm.py; models/rnns.py:19-29) applied to GIVEN gate products gi, gh and hidden state h, in a chosen dtype,
with autograd for the backward. float64 is the reference; float32 on the CPU gives the floors the GPU bounds are 8 x of
(tests/test_gpu_drnn_engine_kernels.py, recomputed by tests/test_dssm_engine_cpu.py).

  Hd 32              one block of 32 features: half a wave idle
  Hd 96, 224         not a multiple of 64: a ragged last feature group per lane
  Hd 256             the widest, four features per lane
  rows 2             the smallest admitted
  rows 33            two 32-row LayerNorm-affine partials, the second of one row
  rows 130           five partials, the last short (and two BatchNorm chunks for the engine's next pass)
"""
import numpy as np
import torch
import torch.nn.functional as F

HDS = (32, 96, 224, 256)
ROWS = (2, 33, 130)
CASES = [(Hd, rows) for Hd in HDS for rows in ROWS]
LN_EPS = 1e-3
PART_ROWS = 32
FWD = ("gate", "lnx", "lnr", "hn")
LN_NAMES = ("ln_reset.weight", "ln_reset.bias", "ln_update.weight", "ln_update.bias", "ln_newval.weight",
            "ln_newval.bias")


def data(Hd, rows, seed=11):
    """float32 CPU tensors: gi, gh [rows, 3Hd] at the scale of a product over ~100 inputs, h and dhn [rows, Hd], the
    six LayerNorm-affine vectors (gains around 1, shifts around 0)."""
    g = torch.Generator().manual_seed(seed + 1000 * Hd + rows)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d = dict(gi=1.5 * r(rows, 3 * Hd), gh=1.5 * r(rows, 3 * Hd), h=torch.tanh(r(rows, Hd)), dhn=r(rows, Hd))
    d["ln"] = [(1.0 + 0.2 * r(Hd)) if i % 2 == 0 else 0.2 * r(Hd) for i in range(6)]
    return d


def gate(d, dtype, zero_hidden=False):
    """-> {"gate", "lnx", "lnr", "hn", "dgi", "dgh", "dhd", the six LN_NAMES gradients}: numpy arrays in `dtype`.
    zero_hidden: gh and h are explicit zeros (what a null hidden state must equal). dgh is the gradient with respect
    to gh and dhd with respect to h with gh held fixed: dhn (1 - update), the direct path."""
    t = lambda x: x.to(dtype).clone().requires_grad_(True)  # noqa: E731
    gi, dhn = t(d["gi"]), d["dhn"].to(dtype)
    gh = t(torch.zeros_like(d["gh"]) if zero_hidden else d["gh"])
    h = t(torch.zeros_like(d["h"]) if zero_hidden else d["h"])
    ln = [t(x) for x in d["ln"]]
    Hd = h.shape[1]
    ri, ui, ni = gi.chunk(3, 1)
    rh, uh, nh = gh.chunk(3, 1)
    pre_r, pre_u = ri + rh, ui + uh
    reset = torch.sigmoid(F.layer_norm(pre_r, (Hd,), ln[0], ln[1], LN_EPS))
    update = torch.sigmoid(F.layer_norm(pre_u, (Hd,), ln[2], ln[3], LN_EPS))
    pre_n = ni + reset * nh
    newval = torch.tanh(F.layer_norm(pre_n, (Hd,), ln[4], ln[5], LN_EPS))
    hn = update * newval + (1 - update) * h
    grads = torch.autograd.grad(hn, [gi, gh, h] + ln, dhn)
    with torch.no_grad():
        xs, rs = [], []
        for p in (pre_r, pre_u, pre_n):
            mu, var = p.mean(1, keepdim=True), p.var(1, unbiased=False, keepdim=True)
            rstd = 1.0 / torch.sqrt(var + LN_EPS)
            xs.append((p - mu) * rstd)
            rs.append(rstd)
        out = dict(gate=torch.cat([reset, update, newval], 1), lnx=torch.cat(xs, 1), lnr=torch.cat(rs, 1), hn=hn,
                   dgi=grads[0], dgh=grads[1], dhd=grads[2])
        out.update(zip(LN_NAMES, grads[3:]))
    return {k: v.detach().numpy() for k, v in out.items()}


def figure(got, want):
    """max |got - want| / max |want|. A reference that is exactly zero (the reset gate's gradients from a zero hidden
    state) admits only exact zeros: 0.0 then, else inf."""
    got, want = np.asarray(got, np.float64).reshape(want.shape), np.asarray(want, np.float64)
    diff, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    if scale == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / scale


def figures(got, want, keys=None):
    return {k: figure(got[k], want[k]) for k in (keys or want) if k in got}


def nparts(rows):
    return -(-rows // PART_ROWS)
