"""GPU: the learner engine's small kernels, one by one, against float64 torch on the CPU (include/tdmpc_learner.h:
tdmpc_lg_rows_fwd / _bwd at every admitted width 256 / 512 / 1024, tdmpc_lg_finalize, tdmpc_lg_pi_loss,
tdmpc_lg_lerp, tdmpc_lg_act). Inside whole updates these are seen only through Adam, which hides a lost partial or a
constant factor; here every output is compared on its own.

Conventions: every output buffer is prefilled with a sentinel and followed by a guard (8 rows behind row tensors, 64
elements behind flat ones) that must keep it; everything meant to be written must be finite; a refused call
(TDMPC_E_DIMS / TDMPC_E_NULL, checked on the host before any launch) leaves its outputs at the sentinel.

Bounds: where no analytic bound is stated the figure is max |got - f64| / max |f64| per tensor and
the bound is 8 x the largest figure float32 torch on the CPU shows against the same float64 result on the same inputs,
never below 1e-6. The floors below are recomputed, and held within 2 x, by
tests/test_learner_widths_cpu.py::test_fp32_floors_the_gpu_bounds_are_derived_from. They are large because the inputs
are meant to hurt: a row of x with offset 30 and scale 1e-2 loses ~1e-4 of its normalised value to the rounding of
its mean in any float32 LayerNorm. Figures measured on the MI355X are quoted beside them as information only.
"""
import ctypes as C

import pytest
import torch

import lg_rows_ref as R
from tdmpc_amd import _lib

pytestmark = pytest.mark.gpu

E_DIMS, E_NULL = -1, -3
S = -12345.0            # the sentinel
U24 = 2.0 ** -24

# float32-CPU floors over all the row cases (lg_rows_ref.rows_fp32_floors); MI355X figures in the comments
ROWS_FLOOR = {
    "xhat": 8.2e-5, "rstd": 1.1e-7, "y": 7.0e-4, "out": 9.9e-5, "td": 4.8e-5,     # MI355X: 5.2e-5 9.0e-8 4.4e-4 9.6e-5 3.2e-5
    # (the backward reads the saved float64 activations, where float32 autograd recomputes its LayerNorm)
    "dP": 3.7e-4, "dg": 6.2e-5, "dbeta": 7.4e-5, "dW3": 3.0e-5, "db3": 1.5e-6,    # MI355X: 1.7e-7 3.0e-7 4.3e-7 5.3e-7 1.5e-6
}
FIN_FLOOR = {"g": 1.4e-7, "normp": 1.6e-7}     # the random-valued finalize case; MI355X: 1.6e-7, 2.4e-7
PI_LOSS_FLOOR = 2.7e-8                          # MI355X: 2.2e-8 (the bound is the 1e-6 minimum)
ELU_FLOOR = 6.0e-8                              # MI355X: 4.2e-8 (the 1e-6 minimum)


def _dev(t):
    return t.contiguous().cuda()


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rowbuf(rows, ld, guard=8):
    return torch.full((rows + guard, ld), S, device="cuda")


def _flat(n, guard=64):
    return torch.full((n + guard,), S, device="cuda")


def _strided(x, ld):
    """x [rows][m] on the device with row stride ld."""
    b = torch.full((x.shape[0], ld), 7.0, device="cuda")
    b[:, :x.shape[1]] = x.cuda()
    return b


def _check_rowbuf(buf, rows, m, ref, key, what):
    """buf [rows + guard][ld]: [:rows, :m] finite and within the class bound of ref; the rest keeps the sentinel."""
    b = buf.cpu()
    assert (b[rows:] == S).all(), (what, key, "guard rows written")
    assert (b[:rows, m:] == S).all(), (what, key, "row padding written")
    got = b[:rows, :m].reshape(ref.shape)
    assert torch.isfinite(got).all(), (what, key)
    f = R.fig(got, ref)
    print(f"{what} {key}: {f:.3g} (bound {R.bound(ROWS_FLOOR[key]):.3g})")
    assert f <= R.bound(ROWS_FLOOR[key]), (what, key, f)


def _untouched(bufs):
    torch.cuda.synchronize()
    for b in bufs:
        assert (b == S).all()


def _last_error():
    return _lib.lib().tdmpc_last_error().decode(errors="replace")


# ------------------------------------------------------------------------------------------------ rows_fwd
FWD_WANT = {"a_tanh_y": ("y",), "b_elu_tail_td": ("out",), "c_tanh_saved": ("y", "xhat", "rstd"),
            "d_q_q_reward": ("y", "xhat", "rstd", "out"), "act0": ("y",), "strided": ("y", "xhat", "rstd", "out")}


def _fwd_args(m, rows, name):
    """-> (LgRows, per head {key: buffer}, td buffer or None, ldy, keepalive) for one forward head set."""
    specs = R.FWD_SETS[name]
    heads, reward, _, _ = R.fwd_case(m, rows, name)
    ldx, ldy = (m + 4, m + 8) if name == "strided" else (m, m)
    a, bufs, keep = _lib.LgRows(), [], []
    for i, (h, (ln, act, tail)) in enumerate(zip(heads, specs)):
        H = a.hd[i]
        d = {k: _dev(h[k]) for k in ("g", "beta", "w3", "b3")}
        d["x"] = _strided(h["x"], ldx)
        keep.append(d)
        o = {}
        for k in FWD_WANT[name]:
            if k in ("xhat", "rstd") and not ln or k == "out" and not tail:
                continue
            o[k] = _rowbuf(rows, {"y": ldy, "xhat": m}.get(k, 1))
        bufs.append(o)
        H.x, H.ldx, H.ldy, H.ln, H.act, H.tail = d["x"].data_ptr(), ldx, ldy, ln, act, tail
        if ln:
            H.g, H.beta = d["g"].data_ptr(), d["beta"].data_ptr()
        if tail:
            H.w3, H.b3 = d["w3"].data_ptr(), d["b3"].data_ptr()
        for k, b in o.items():
            setattr(H, k, b.data_ptr())
    a.nh, a.rows, a.m, a.bsz = len(specs), rows, m, 1
    td = None
    if name == "b_elu_tail_td":
        td, rw = _rowbuf(rows, 1), _dev(reward)
        keep.append(rw)
        a.reward, a.td, a.gamma = rw.data_ptr(), td.data_ptr(), R.GAMMA
    return a, bufs, td, ldy, keep


@pytest.mark.parametrize("rows", R.FWD_ROWS)
@pytest.mark.parametrize("m", R.WIDTHS)
def test_rows_fwd_matches_float64(m, rows):
    """Every head set the engine issues (and act 0, and padded row strides) at every width; 5 and 70 rows leave idle
    waves in the last workgroup of 4, which the guard rows behind every output watch."""
    L = _lib.lib()
    for name in R.FWD_SETS:
        a, bufs, td, ldy, keep = _fwd_args(m, rows, name)
        _lib.check(L.tdmpc_lg_rows_fwd(C.byref(a), _st()), "tdmpc_lg_rows_fwd")
        torch.cuda.synchronize()
        _, _, ref, td_ref = R.fwd_case(m, rows, name)
        for i, o in enumerate(bufs):
            for k, b in o.items():
                _check_rowbuf(b, rows, m if k in ("y", "xhat") else 1, ref[i][k], k, f"fwd m{m} r{rows} {name} h{i}")
        if td is not None:
            if rows >= 5:   # min() takes both sides
                assert (ref[0]["out"] < ref[1]["out"]).any() and (ref[0]["out"] > ref[1]["out"]).any()
            _check_rowbuf(td, rows, 1, td_ref, "td", f"fwd m{m} r{rows} {name}")


# ------------------------------------------------------------------------------------------------ rows_bwd
def _bwd_args(m, rows, name, nwg, bsz=0):
    specs = R.BWD_SETS[name]
    heads, _, pi = R.bwd_case(m, rows, name, torch.float64, bsz)
    with_part = name in ("a_q_q_reward", "b_tanh_part")
    a, bufs, keep = _lib.LgRows(), [], []
    for i, (h, (ln, act, tail)) in enumerate(zip(heads, specs)):
        H = a.hd[i]
        d = {k: _dev(h[k]) for k in ("g", "w3", "yact", "dq", "dA") + (("xhat", "rstd") if ln else ())}
        keep.append(d)
        o = {"y": _rowbuf(rows, m)}
        if with_part:
            o["part"] = _flat(nwg * R.part_width(specs[i], m))
        bufs.append(o)
        H.y, H.ldx, H.ldy, H.ln, H.act, H.tail = o["y"].data_ptr(), m, m, ln, act, tail
        H.yact = d["yact"].data_ptr()
        if ln:
            H.xhat, H.rstd, H.g = d["xhat"].data_ptr(), d["rstd"].data_ptr(), d["g"].data_ptr()
        if tail:
            H.w3 = d["w3"].data_ptr()
            if pi is None:
                H.dq = d["dq"].data_ptr()
        else:
            H.x = d["dA"].data_ptr()
        if with_part:
            H.part = o["part"].data_ptr()
    a.nh, a.rows, a.m, a.bsz = len(specs), rows, m, max(bsz, 1)
    if pi is not None:
        q = [_dev(t) for t in pi]
        keep.append(q)
        a.q1, a.q2, a.rho = (t.data_ptr() for t in q)
    return a, bufs, keep


def _check_bwd(m, rows, name, nwg, bsz=0):
    L = _lib.lib()
    specs = R.BWD_SETS[name]
    a, bufs, keep = _bwd_args(m, rows, name, nwg, bsz)
    _lib.check(L.tdmpc_lg_rows_bwd(C.byref(a), nwg, _st()), "tdmpc_lg_rows_bwd")
    torch.cuda.synchronize()
    _, ref, _ = R.bwd_case(m, rows, name, torch.float64, bsz)
    what = f"bwd m{m} r{rows} nwg{nwg} {name}"
    nw = 4 if m == 1024 else 16      # rows per workgroup and stride step
    for i, o in enumerate(bufs):
        _check_rowbuf(o["y"], rows, m, ref[i]["dP"], "dP", f"{what} h{i}")
        if "part" not in o:
            continue
        pw = R.part_width(specs[i], m)
        p = o["part"].cpu()
        assert (p[nwg * pw:] == S).all(), (what, i, "guard behind part written")
        p = p[:nwg * pw].view(nwg, pw)
        assert torch.isfinite(p).all() and not (p == S).any(), (what, i, "a workgroup wrote no partials")
        for wg in range(nwg):        # a workgroup that owns no row writes zeros: lg_finalize sums all nwg slices
            if wg * nw >= rows:
                assert (p[wg] == 0).all(), (what, i, wg)
        for k, v in R.split_part(specs[i], m, p.double().sum(0)).items():
            f = R.fig(v, ref[i][k])
            print(f"{what} h{i} {k}: {f:.3g} (bound {R.bound(ROWS_FLOOR[k]):.3g})")
            assert f <= R.bound(ROWS_FLOOR[k]), (what, i, k, f)


@pytest.mark.parametrize("rows,nwg", R.BWD_SHAPES)
@pytest.mark.parametrize("m", R.WIDTHS)
def test_rows_bwd_matches_float64_autograd(m, rows, nwg):
    """update's and _update_pi's head sets with given upstream gradients: workgroups without rows (5, 256), one
    workgroup looping over everything (70, 1), a ragged stride (70, 3) and several strides at 16 and at 4 waves per
    workgroup (1100, 2)."""
    for name in ("a_q_q_reward", "b_tanh_part", "d_tanh_nopart"):
        _check_bwd(m, rows, name, nwg)


@pytest.mark.parametrize("nt,bsz,nwg", R.PI_SHAPES)
@pytest.mark.parametrize("m", R.WIDTHS)
def test_rows_bwd_pi_mode_matches_float64_autograd(m, nt, bsz, nwg):
    """dq of head h = d(-sum_t rho_t mean_b min(q1, q2)) / dq_h from q1 / q2 / rho[r / bsz]: an eighth of exact ties
    (split in half, as torch.minimum's backward), the rest on both sides, distinct rho."""
    q1, q2, rho = R.pi_q(nt, bsz, R._seed(3, m, nt * bsz))
    assert (q1 == q2).any() and (q1 < q2).any() and (q1 > q2).any()
    _check_bwd(m, nt * bsz, "c_pi", nwg, bsz)


def _refuse_fwd(mutate, code, msg, name="d_q_q_reward"):
    a, bufs, td, _, keep = _fwd_args(256, 5, name)
    mutate(a)
    rc = _lib.lib().tdmpc_lg_rows_fwd(C.byref(a), _st())
    assert rc == code, rc
    if msg:
        assert msg in _last_error(), _last_error()
    _untouched([b for o in bufs for b in o.values()] + ([td] if td is not None else []))


def _refuse_bwd(mutate, nwg, code, msg):
    a, bufs, keep = _bwd_args(256, 5, "a_q_q_reward", 4)
    mutate(a)
    rc = _lib.lib().tdmpc_lg_rows_bwd(C.byref(a), nwg, _st())
    assert rc == code, rc
    if msg:
        assert msg in _last_error(), _last_error()
    _untouched([b for o in bufs for b in o.values()])


def _set(**kw):
    def f(a):
        for k, v in kw.items():
            setattr(a, k, v)
    return f


def _set_head(i, **kw):
    def f(a):
        for k, v in kw.items():
            setattr(a.hd[i], k, v(getattr(a.hd[i], k)) if callable(v) else v)
    return f


def test_rows_refusals_write_nothing():
    """What rows_ok and the wrappers refuse, on the host, with a message; the outputs keep their sentinel. (The
    pointer off by 4 bytes is an address inside the operand's own allocation.)"""
    for fn in (_refuse_fwd, lambda mu, c, s: _refuse_bwd(mu, 4, c, s)):
        fn(_set(m=384), E_DIMS, "nh / rows / m")
        fn(_set(nh=0), E_DIMS, "nh / rows / m")
        fn(_set(nh=4), E_DIMS, "nh / rows / m")
        fn(_set_head(1, w3=lambda p: p + 4), E_DIMS, "16-B aligned")
        fn(_set_head(0, y=lambda p: p + 4), E_DIMS, "16-B aligned")
    _refuse_fwd(_set_head(0, ldx=258), E_DIMS, "multiples of 4")
    _refuse_fwd(_set(nh=1), E_DIMS, "td needs two tail heads", name="b_elu_tail_td")
    _refuse_bwd(_set_head(0, ldy=258), 4, E_DIMS, "multiples of 4")
    _refuse_bwd(lambda a: None, 0, E_DIMS, "nwg")
    _refuse_bwd(lambda a: None, 4097, E_DIMS, "nwg")
    _refuse_bwd(_set_head(1, yact=None), 4, E_NULL, None)
    assert _lib.lib().tdmpc_lg_rows_fwd(None, _st()) == E_NULL


# ------------------------------------------------------------------------------------------------ finalize
def _gsrc(ts, src):
    arr = (_lib.LgGsrc * len(ts))()
    for t, (rows, cols, ld, ns, sstride, dst, off) in zip(arr, ts):
        t.src, t.dst, t.sstride = src.data_ptr() + 4 * off, dst, sstride
        t.rows, t.cols, t.ld, t.nslices = rows, cols, ld, ns
    return arr


def _finalize(ts, src, step=7, slack=5):
    glen, blocks = ts[-1][5] + ts[-1][0] * ts[-1][1] + 64, sum(
        -(-t[0] * t[1] // (R.FIN_PER if t[3] < R.FIN_MANY else 64)) for t in ts)
    g, normp = torch.full((glen,), S, device="cuda"), torch.full((blocks + slack,), S, device="cuda")
    st = torch.full((1,), step, dtype=torch.int32, device="cuda") if step is not None else None
    srcd = _dev(src)
    rc = _lib.lib().tdmpc_lg_finalize(_gsrc(ts, srcd), len(ts), g.data_ptr(), normp.data_ptr(), blocks + slack,
                                      st.data_ptr() if st is not None else None, _st())
    torch.cuda.synchronize()
    return rc, g.cpu(), normp.cpu(), blocks, (int(st.item()) if st is not None else None)


_COMBOS = [(ns, sz) for ns in R.FIN_NSLICES for sz in R.FIN_SIZES]     # 80 (nslices, rows * cols) pairs


@pytest.mark.parametrize("part", [0, 1])
def test_finalize_integer_sources_are_summed_exactly(part):
    """Sources of small integers: every slice sum (<= 256 * 8) and every workgroup's sum of squares (asserted below
    2^24) is exact in float32 in any order, so g and normp must equal the float64 sums bit for bit. nslices spans
    both code paths (>= 32: 64 elements per workgroup, four thread groups, an unrolled-by-8 body and its tail) and
    every tail length; rows * cols put chunk boundaries on both paths; ld > cols, sstride beyond the tensor, gaps in
    dst. The first launch holds 48 tensors (the most a launch takes), the second the other 32 with a null step."""
    combos = _COMBOS[:48] if part == 0 else _COMBOS[48:]
    ts, glen, slen, blocks = R.finalize_layout(combos)
    src = torch.randint(-8, 9, (slen,), generator=torch.Generator().manual_seed(11 + part)).float()
    gs, sq = R.finalize_ref(ts, src)
    assert float(sq.max()) < 2 ** 24
    rc, g, normp, nb, step = _finalize(ts, src, step=7 if part == 0 else None)
    _lib.check(rc, "tdmpc_lg_finalize")
    assert nb == blocks and len(sq) == blocks
    written = torch.zeros(len(g), dtype=torch.bool)
    for (rows, cols, ld, ns, sstride, dst, off), v in zip(ts, gs):
        assert torch.equal(g[dst:dst + rows * cols].double(), v), (rows, cols, ld, ns)
        written[dst:dst + rows * cols] = True
    assert (g[~written] == S).all() and int((~written).sum()) > 64      # the gaps and the guard
    assert torch.equal(normp[:blocks].double(), sq)
    assert (normp[blocks:] == S).all()
    assert step == (8 if part == 0 else None)


def test_finalize_random_sources_within_float32_of_float64():
    """The float path: random sources, a few tensors on both code paths."""
    combos = [(4, 5000), (31, 2049), (32, 2047), (65, 5000), (256, 2048), (37, 63)]
    ts, glen, slen, blocks = R.finalize_layout(combos)
    src = torch.randn(slen, generator=torch.Generator().manual_seed(13))
    gs, sq = R.finalize_ref(ts, src)
    rc, g, normp, _, step = _finalize(ts, src)
    _lib.check(rc, "tdmpc_lg_finalize")
    assert step == 8
    for (rows, cols, ld, ns, sstride, dst, off), v in zip(ts, gs):
        f = R.fig(g[dst:dst + rows * cols], v)
        print(f"finalize ns{ns} n{rows * cols}: {f:.3g}")
        assert f <= R.bound(FIN_FLOOR["g"]), (ns, rows * cols, f)
    f = float(((normp[:blocks].double() - sq).abs() / sq).max())
    print(f"finalize normp: {f:.3g}")
    assert f <= R.bound(FIN_FLOOR["normp"]), f
    assert (normp[blocks:] == S).all()


def test_finalize_refusals_write_nothing():
    src = torch.ones(4096)
    base = R.finalize_layout([(4, 63), (33, 65), (1, 64)])[0]

    def refused(ts, slack=5, msg="in order without overlap"):
        rc, g, normp, _, step = _finalize(ts, src, slack=slack)
        assert rc == E_DIMS and msg in _last_error(), (rc, _last_error())
        assert (g == S).all() and (normp == S).all() and step == 7

    t = [list(x) for x in base]
    refused([tuple(x) for x in [t[1], t[0], t[2]]])                         # dst out of order
    t[1][5] = t[0][5] + t[0][0] * t[0][1] - 1
    refused([tuple(x) for x in t])                                          # overlapping by one element
    t = [list(x) for x in base]
    t[1][2] = t[1][1] - 1
    refused([tuple(x) for x in t])                                          # ld < cols
    t = [list(x) for x in base]
    t[2][3] = 0
    refused([tuple(x) for x in t])                                          # nslices = 0
    refused(base, slack=-1, msg="fewer entries than workgroups")             # nblk below the workgroup count
    many = R.finalize_layout([(1, 1)] * 49)[0]
    refused(many, msg="nt / nblk")                                          # 49 tensors


# ------------------------------------------------------------------------------------------------ pi_loss
@pytest.mark.parametrize("bsz", [1, 255, 256, 257, 600])
@pytest.mark.parametrize("nt", [1, 6])
def test_pi_loss_matches_float64(nt, bsz):
    q1, q2, rho = R.pi_q(nt, bsz, 100 * nt + bsz)
    if nt * bsz >= 3:
        assert (q1 == q2).any()
    ref = R.pi_loss_ref(q1, q2, rho, nt, bsz, torch.float64)
    scale = float((rho.double() * torch.minimum(q1, q2).double().abs().view(nt, bsz).mean(1)).sum())
    out = _flat(1)
    d = [_dev(q1), _dev(q2), _dev(rho)]
    _lib.check(_lib.lib().tdmpc_lg_pi_loss(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), nt, bsz,
                                           out.data_ptr(), _st()), "tdmpc_lg_pi_loss")
    o = out.cpu()
    assert (o[1:] == S).all() and torch.isfinite(o[0])
    f = abs(float(o[0]) - float(ref)) / scale
    print(f"pi_loss nt{nt} bsz{bsz}: {f:.3g}")
    assert f <= R.bound(PI_LOSS_FLOOR), f


# ------------------------------------------------------------------------------------------------ lerp / act
@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 3])
def test_lerp_matches_float64(n):
    """t <- lerp(t, p, w): w = 0 returns t and w = 1 returns p exactly (both formula branches, which switch at 0.5);
    otherwise three float32 roundings of terms no larger than |t| + |p|, one spare. 2048 * 256 + 3 elements run the
    grid-stride loop twice. (Not bitwise against CPU float32: the device contracts to fma.)"""
    g = torch.Generator().manual_seed(n)
    t0, p = torch.randn(n, generator=g) * 3, torch.randn(n, generator=g) * 3
    pd = _dev(p)
    for w in (0.0, 0.01, 0.49999, 0.5, 0.99, 1.0):
        buf = _flat(n)
        buf[:n] = t0.cuda()
        _lib.check(_lib.lib().tdmpc_lg_lerp(buf.data_ptr(), pd.data_ptr(), n, w, _st()), "tdmpc_lg_lerp")
        got = buf.cpu()
        assert (got[n:] == S).all(), w
        got = got[:n]
        if w == 0.0:
            assert torch.equal(got, t0)
        elif w == 1.0:
            assert torch.equal(got, p)
        else:
            wf = float(torch.tensor(w, dtype=torch.float32))      # the float the kernel receives
            ref = t0.double() + wf * (p.double() - t0.double())
            assert ((got.double() - ref).abs() <= 4 * U24 * (t0.double().abs() + p.double().abs())).all(), w
    assert torch.equal(pd.cpu(), p)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [4, 1028, 4 * 2048 * 256 + 4])
def test_act_matches_float64(n, mode):
    """In place: mode 0 ELU (bounded from the float32 CPU floor), mode 1 x * ELU'(y) with y the saved ELU output (two
    roundings). x straddles 0 and reaches below -20; y holds exact zeros (ELU' = y + 1 = 1 there)."""
    x, y = R.act_inputs(n, n + mode)
    buf = _flat(n)
    buf[:n] = x.cuda()
    yd = _dev(y)
    _lib.check(_lib.lib().tdmpc_lg_act(buf.data_ptr(), yd.data_ptr() if mode else None, n, mode, _st()),
               "tdmpc_lg_act")
    got = buf.cpu()
    assert (got[n:] == S).all() and torch.isfinite(got[:n]).all()
    got = got[:n]
    if mode == 0:
        f = R.elu_fig(got, torch.nn.functional.elu(x.double()))
        print(f"act elu n{n}: {f:.3g}")
        assert f <= R.bound(ELU_FLOOR), f
    else:
        assert (y == 0).any() and (y < 0).any() and (y > 0).any()
        y64 = y.double()
        ref = x.double() * torch.where(y64 > 0, torch.ones_like(y64), y64 + 1)
        assert ((got.double() - ref).abs() <= 2 * U24 * ref.abs()).all()
        assert torch.equal(yd.cpu(), y)


def test_act_refusals_write_nothing():
    L = _lib.lib()
    buf, y = _flat(16), torch.zeros(16, device="cuda")
    for args, code in (((buf.data_ptr(), None, 6, 0), E_DIMS), ((buf.data_ptr() + 4, None, 8, 0), E_DIMS),
                       ((buf.data_ptr(), y.data_ptr(), 8, 2), E_DIMS), ((buf.data_ptr(), None, 8, 1), E_NULL)):
        assert L.tdmpc_lg_act(*args, _st()) == code, args
        if code == E_DIMS:
            assert "tdmpc_lg_act" in _last_error()
    _untouched([buf])
