"""Shared by tests/test_gpu_lg_rows.py and tests/test_learner_widths_cpu.py: inputs and plain torch references of the
learner engine's small kernels (include/tdmpc_learner.h: tdmpc_lg_rows_fwd / _bwd, tdmpc_lg_finalize, tdmpc_lg_pi_loss,
tdmpc_lg_lerp, tdmpc_lg_act), on the CPU in a dtype the caller names. float64 is the yardstick; the same functions in
float32 give the noise floor the GPU bounds are derived from (bound = 8 x floor, never below 1e-6).

Nothing here touches the GPU or the HIP library."""
import functools

import torch
import torch.nn.functional as F

WIDTHS = (256, 512, 1024)
GAMMA = 0.99
FACTOR, MIN_BOUND = 8.0, 1e-6


def bound(floor):
    return max(FACTOR * floor, MIN_BOUND)


def fig(got, ref):
    """max |got - ref| / max |ref| of one tensor, in float64."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


# ------------------------------------------------------------------------------------------------ row kernels
# head sets as learner_engine.py issues them: (ln, act, tail) per head; act 0 none, 1 tanh, 2 elu
FWD_SETS = {
    "a_tanh_y": [(1, 1, 0)] * 2,            # _td_steps / q_forward: y written, nothing saved
    "b_elu_tail_td": [(1, 2, 1)] * 2,       # _td_steps: out and td only
    "c_tanh_saved": [(1, 1, 0)] * 2,        # _fwd_steps: xhat / rstd saved
    "d_q_q_reward": [(1, 2, 1), (1, 2, 1), (0, 2, 1)],   # _fwd_steps: Q1, Q2 and the reward head's output layers
    "act0": [(1, 0, 0)],                    # the ABI beyond the engine: no activation
    "strided": [(1, 1, 0), (1, 2, 1)],      # ldx = m + 4, ldy = m + 8
}
BWD_SETS = {
    "a_q_q_reward": [(1, 2, 1), (1, 2, 1), (0, 2, 1)],   # update: dq given, partials
    "b_tanh_part": [(1, 1, 0)] * 2,                      # update: dA given, partials
    "c_pi": [(1, 2, 1)] * 2,                             # _update_pi: dq from q1 / q2 / rho, no partials
    "d_tanh_nopart": [(1, 1, 0)] * 2,                    # _update_pi: dA given, no partials
}


def _seed(*key):
    return sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))


def row_inputs(m, rows, nh, seed):
    """float32 inputs of `nh` heads over [rows][m]: every row of x has its own offset (up to +-30) and scale (1e-2 to
    1e2), so the mean and the variance passes both matter; g has negative entries."""
    g = torch.Generator().manual_seed(seed)
    heads = []
    for _ in range(nh):
        scale = 10.0 ** (torch.rand(rows, 1, generator=g) * 4 - 2)
        off = (torch.rand(rows, 1, generator=g) * 2 - 1) * 30
        heads.append({
            "x": torch.randn(rows, m, generator=g) * scale + off,
            "g": torch.randn(m, generator=g),
            "beta": torch.randn(m, generator=g) * 0.5,
            "w3": torch.randn(m, generator=g) / m ** 0.5,
            "b3": torch.randn(1, generator=g) * 0.1,
            "dq": torch.randn(rows, generator=g),
            "dA": torch.randn(rows, m, generator=g),
        })
        assert (heads[-1]["g"] < 0).any()
    reward = torch.randn(rows, generator=g)
    return heads, reward


def head_forward(h, spec, dtype, x=None):
    """One head in `dtype`: dict(xhat, rstd, y, out) (those that exist for spec = (ln, act, tail))."""
    ln, act, tail = spec
    m = h["x"].shape[1]
    v = h["x"].to(dtype) if x is None else x
    o = {}
    if ln:
        o["rstd"] = 1.0 / torch.sqrt(v.var(dim=1, unbiased=False) + 1e-5)
        o["xhat"] = F.layer_norm(v, (m,), None, None, 1e-5)
        v = o["xhat"] * h["g"].to(dtype) + h["beta"].to(dtype)
    o["y"] = torch.tanh(v) if act == 1 else F.elu(v) if act == 2 else v
    if tail:
        o["out"] = o["y"] @ h["w3"].to(dtype) + h["b3"].to(dtype)
    return o


@functools.lru_cache(maxsize=None)
def fwd_case(m, rows, name, dtype=torch.float64):
    specs = FWD_SETS[name]
    heads, reward = row_inputs(m, rows, len(specs), _seed(1, m, rows, sorted(FWD_SETS).index(name)))
    outs = [head_forward(h, s, dtype) for h, s in zip(heads, specs)]
    td = None
    if name == "b_elu_tail_td":
        td = reward.to(dtype) + GAMMA * torch.minimum(outs[0]["out"], outs[1]["out"])
    return heads, reward, outs, td


def pi_q(nt, bsz, seed):
    """q1, q2 [nt * bsz] float32 with about an eighth of exact ties and the rest split between q1 < q2 and q1 > q2;
    rho [nt] distinct."""
    g = torch.Generator().manual_seed(seed)
    n = nt * bsz
    q1 = torch.randn(n, generator=g)
    q2 = q1 + torch.randn(n, generator=g)
    tie = torch.rand(n, generator=g) < 0.125
    if n >= 3:
        tie[0], tie[1], tie[2] = True, False, False
        q2[1], q2[2] = q1[1] + 0.5, q1[2] - 0.5
    q2 = torch.where(tie, q1, q2)
    rho = torch.tensor([0.9 ** t + 0.01 * t for t in range(nt)], dtype=torch.float32)
    assert len(set(rho.tolist())) == nt
    return q1, q2, rho


def pi_loss_ref(q1, q2, rho, nt, bsz, dtype):
    q1, q2, rho = q1.to(dtype), q2.to(dtype), rho.to(dtype)
    return -(rho * torch.minimum(q1, q2).view(nt, bsz).mean(dim=1)).sum()


@functools.lru_cache(maxsize=None)
def bwd_case(m, rows, name, dtype=torch.float64, bsz=0):
    """-> heads (float32 inputs, with the saved activations yact / xhat / rstd of a float64 forward cast to float32),
    per head dict(dP, and dg / dbeta / dW3 / db3 where the head has them) from autograd in `dtype`, and for the pi
    mode (q1, q2, rho)."""
    specs = BWD_SETS[name]
    heads, _ = row_inputs(m, rows, len(specs), _seed(2, m, rows, sorted(BWD_SETS).index(name)))
    pi = None
    if name == "c_pi":
        nt = rows // bsz
        q1, q2, rho = pi_q(nt, bsz, _seed(3, m, rows))
        l1, l2 = q1.to(dtype).requires_grad_(), q2.to(dtype).requires_grad_()
        pi_loss_ref(l1, l2, rho, nt, bsz, dtype).backward()
        heads[0]["dq"], heads[1]["dq"] = l1.grad.float(), l2.grad.float()
        dq_exact = (l1.grad, l2.grad)
        pi = (q1, q2, rho)
    grads = []
    for i, (h, s) in enumerate(zip(heads, specs)):
        ln, act, tail = s
        saved = head_forward(h, s, torch.float64)
        h["yact"] = saved["y"].float()
        if ln:
            h["xhat"], h["rstd"] = saved["xhat"].float(), saved["rstd"].float()
        leaves = {k: h[k].to(dtype).requires_grad_() for k in ("x", "g", "beta", "w3", "b3")}
        o = head_forward({**h, **leaves}, s, dtype, x=leaves["x"])
        if tail:
            dq = dq_exact[i] if pi is not None else h["dq"].to(dtype)
            (o["out"] * dq).sum().backward()
        else:
            (o["y"] * h["dA"].to(dtype)).sum().backward()
        r = {"dP": leaves["x"].grad}
        if ln:
            r["dg"], r["dbeta"] = leaves["g"].grad, leaves["beta"].grad
        if tail:
            r["dW3"], r["db3"] = leaves["w3"].grad, leaves["b3"].grad
        grads.append(r)
    return heads, grads, pi


def part_width(spec, m):
    ln, _, tail = spec
    return (2 * m if ln else 0) + (m + 1 if tail else 0)


def split_part(spec, m, colsum):
    """The header's layout of one head's partial sums: dg | dbeta if ln, then dW3 | db3 if tail."""
    ln, _, tail = spec
    r, o = {}, 0
    if ln:
        r["dg"], r["dbeta"], o = colsum[:m], colsum[m:2 * m], 2 * m
    if tail:
        r["dW3"], r["db3"] = colsum[o:o + m], colsum[o + m:o + m + 1]
    return r


FWD_ROWS = (1, 5, 70)
BWD_SHAPES = ((5, 256), (70, 1), (70, 3), (1100, 2))     # (rows, nwg)
PI_SHAPES = ((1, 5, 256), (6, 35, 1), (6, 35, 3))         # (nt, bsz, nwg)
FWD_CLASSES = ("xhat", "rstd", "y", "out", "td")
BWD_CLASSES = ("dP", "dg", "dbeta", "dW3", "db3")


def rows_fp32_floors():
    """{class: the largest figure float32 torch on the CPU shows against float64 over all the row cases}."""
    fl = {c: 0.0 for c in FWD_CLASSES + BWD_CLASSES}
    for m in WIDTHS:
        for rows in FWD_ROWS:
            for name in FWD_SETS:
                _, _, o64, td64 = fwd_case(m, rows, name)
                _, _, o32, td32 = fwd_case(m, rows, name, torch.float32)
                for a, b in zip(o32, o64):
                    for k in b:
                        fl[k] = max(fl[k], fig(a[k], b[k]))
                if td64 is not None:
                    fl["td"] = max(fl["td"], fig(td32, td64))
        cases = [(rows, name, 0) for rows, _ in BWD_SHAPES for name in BWD_SETS if name != "c_pi"]
        cases += [(nt * bsz, "c_pi", bsz) for nt, bsz, _ in PI_SHAPES]
        for rows, name, bsz in set(cases):
            _, g64, _ = bwd_case(m, rows, name, torch.float64, bsz)
            _, g32, _ = bwd_case(m, rows, name, torch.float32, bsz)
            for a, b in zip(g32, g64):
                for k in b:
                    fl[k] = max(fl[k], fig(a[k], b[k]))
    return fl


# ------------------------------------------------------------------------------------------------ finalize
FIN_NSLICES = (1, 4, 31, 32, 33, 37, 60, 64, 65, 256)
FIN_SIZES = {1: (1, 1), 63: (9, 7), 64: (8, 8), 65: (5, 13), 2047: (23, 89), 2048: (32, 64), 2049: (3, 683),
             5000: (8, 625)}
FIN_MANY, FIN_PER = 32, 2048     # lg_finalize: from 32 slices a workgroup takes 64 elements, below that 2048


def finalize_layout(combos):
    """[(nslices, size)] -> tensors [(rows, cols, ld, nslices, sstride, dst, src_off)], total g length, source length,
    workgroup count. Odd tensors are [rows][cols] with ld = cols + 1 (the weight-with-bias-column layout), even ones
    one row; sstride exceeds the tensor by 0 / 5 / 10 elements; dst leaves gaps of 0 / 3 / 6 elements."""
    ts, dst, src, blocks = [], 0, 0, 0
    for i, (ns, size) in enumerate(combos):
        rows, cols = FIN_SIZES[size] if i % 2 else (1, size)
        ld = cols + 1 if i % 2 else cols
        sstride = rows * ld + 5 * (i % 3)
        dst += 3 * (i % 3)
        ts.append((rows, cols, ld, ns, sstride, dst, src))
        dst += rows * cols
        src += ns * sstride
        per = FIN_PER if ns < FIN_MANY else 64
        blocks += -(-rows * cols // per)
    return ts, dst + 64, src, blocks


def finalize_ref(ts, src, dtype=torch.float64):
    """-> per tensor the slice sum [rows * cols] in `dtype`, and the per-workgroup sums of squares (in tensor order)."""
    gs, sq = [], []
    for rows, cols, ld, ns, sstride, dst, off in ts:
        s = src[off:off + ns * sstride].to(dtype).view(ns, sstride)[:, :rows * ld].reshape(ns, rows, ld)[:, :, :cols]
        v = s.sum(0).reshape(-1)
        gs.append(v)
        per = FIN_PER if ns < FIN_MANY else 64
        sq += [(c ** 2).sum() for c in v.split(per)]
    return gs, torch.stack(sq)


# ------------------------------------------------------------------------------------------------ elementwise
def act_inputs(n, seed):
    """x straddles 0 and holds x < -20; y (a saved ELU output) holds exact zeros."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * 3
    x[::7] *= 10
    x[0], x[1], x[2], x[3] = -25.0, 0.0, -1e-4, 30.0
    y = F.elu(torch.randn(n, generator=g) * 2)
    y[::5] = 0.0
    return x, y


def elu_fig(got, ref):
    """ELU's figure: max |got - ref| / max(|ref|, 1) elementwise (its negative branch lives in (-1, 0))."""
    got, ref = got.double().cpu(), ref.double()
    return float(((got - ref).abs() / ref.abs().clamp(min=1.0)).max())
