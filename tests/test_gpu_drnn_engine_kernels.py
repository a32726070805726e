"""GPU: the gate entry points of include/tdmpc_drnn_engine.h (csrc/drnn_engine.inc) against float64 PyTorch: the
`NormGRUCell` expressions of tdmpc_amd/dssm.py applied to given gi, gh, h, with autograd for the backward
(tests/drnn_gate_ref.py, which lists what each shape exercises).

Every tensor is held to max |gpu - f64| / max |f64| <= 8 x the largest such figure float32 CPU PyTorch shows against
float64 on the same inputs, never below 1e-6 (the project's recipe, DESIGN.md §7 f7: another but fixed summation order
moves float32 results by a small multiple of what the CPU's order does). The float32 CPU figures are the constants
below, one for the forward's saved regions and h', one for the gradients; tests/test_dssm_engine_cpu.py
recomputes them. A reference that is exactly zero (the reset gate's gradients from a zero hidden state) admits only
exact zeros. Every comparison prints the GPU figure beside the float32 CPU one.
"""
import ctypes as C

import pytest
import torch

import drnn_gate_ref as R

pytestmark = pytest.mark.gpu

# float32 CPU PyTorch against float64, largest figure over drnn_gate_ref.CASES x (a hidden state, explicit zeros)
FP32_CPU_FWD = 2.912e-07   # Hd 96 rows 130, gate
FP32_CPU_BWD = 3.695e-07   # Hd 224 rows 2, ln_reset.weight
BOUND_FWD = max(8 * FP32_CPU_FWD, 1e-6)
BOUND_BWD = max(8 * FP32_CPU_BWD, 1e-6)
E_DIMS = -1   # TDMPC_E_DIMS (include/tdmpc_hip.h)
SENTINEL = 12345.0

_REF = {}


def _reference(case, zero_hidden):
    """Per (case, hidden state), computed once and left unchanged: the data, the float64 and the float32 CPU results."""
    key = (case, zero_hidden)
    if key not in _REF:
        d = R.data(*case)
        _REF[key] = (d, R.gate(d, torch.float64, zero_hidden), R.gate(d, torch.float32, zero_hidden))
    return _REF[key]


def _lib():
    from tdmpc_amd import _lib
    return _lib


def _table(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _part_floats(rows, Hd):
    n = C.c_size_t()
    _lib().call("tdmpc_drnn_gate_part_floats", rows, Hd, C.byref(n))
    return n.value


def _run(d, Hd, rows, null_hidden):
    """The forward, then the backward over the regions the forward saved -> numpy results keyed as drnn_gate_ref.gate's
    (without dgh / dhd when null_hidden), `part` summed in slice order."""
    lib = _lib()
    dev = "cuda"
    gi, dhn = d["gi"].to(dev), d["dhn"].to(dev)
    gh, h = (None, None) if null_hidden else (d["gh"].to(dev), d["h"].to(dev))
    ln = [x.to(dev) for x in d["ln"]]
    tab = _table(ln)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)  # noqa: E731
    gate, lnx, lnr, hn = nan(rows, 3 * Hd), nan(rows, 3 * Hd), nan(rows, 4), nan(rows, Hd)
    lib.call("tdmpc_drnn_gate_fwd", gi, gh, h, tab, gate, lnx, lnr, hn, rows, Hd, _stream())
    n = _part_floats(rows, Hd)
    assert n == R.nparts(rows) * 6 * Hd
    dgi, part = nan(rows, 3 * Hd), nan(n)
    dgh, dhd = (None, None) if null_hidden else (nan(rows, 3 * Hd), nan(rows, Hd))
    lib.call("tdmpc_drnn_gate_bwd", dhn, gh, h, tab, gate, lnx, lnr, dgi, dgh, dhd, part, rows, Hd, _stream())
    torch.cuda.synchronize()
    assert bool((lnr[:, 3] == 0).all())
    out = dict(gate=gate, lnx=lnx, lnr=lnr[:, :3], hn=hn, dgi=dgi)
    if not null_hidden:
        out.update(dgh=dgh, dhd=dhd)
    slices = part.view(R.nparts(rows), 6, Hd)
    total = slices[0].clone()
    for p in range(1, slices.shape[0]):   # (slice order: what tdmpc_lg_finalize does with this source)
        total += slices[p]
    out.update(zip(R.LN_NAMES, total))
    for k, v in out.items():
        assert bool(torch.isfinite(v).all()), (k, "a value was not written")
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check(tag, got, want, cpu):
    gf, cf = R.figures(got, want), R.figures(cpu, want)
    over = {}
    for k, v in gf.items():
        bound = BOUND_FWD if k in R.FWD else BOUND_BWD
        print(f"{tag} {k}: gpu {v:.3e}, fp32cpu {cf[k]:.3e} (bound {bound:.2e})")
        if not v <= bound:
            over[k] = v
    assert not over, (tag, over)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "Hd%d-rows%d" % c)
def test_gate_with_a_hidden_state_matches_float64(case):
    """gate, lnx, lnr, h'; dgi, dgh, the direct path dhd; the six LayerNorm-affine gradients as the slice-order sum of
    ceil(rows / 32) partials, every float of which the kernel has written."""
    d, want, cpu = _reference(case, False)
    got = _run(d, *case, null_hidden=False)
    assert set(got) == set(want)
    _check("Hd %d rows %d" % case, got, want, cpu)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "Hd%d-rows%d" % c)
def test_gate_with_a_null_hidden_state_matches_explicit_zeros(case):
    """gh = h = null against float64 on explicit zeros, and equal to the entry points' own result on explicit zeros
    (dgi's reset third and ln_reset's partials exactly zero); dgh and dhd are not asked for."""
    d, want, cpu = _reference(case, True)
    Hd, rows = case
    got = _run(d, Hd, rows, null_hidden=True)
    assert set(got) == set(want) - {"dgh", "dhd"}
    _check("Hd %d rows %d null" % case, got, want, cpu)
    assert not got["dgi"][:, :Hd].any() and not got["ln_reset.weight"].any() and not got["ln_reset.bias"].any()
    zeros = dict(d, gh=torch.zeros_like(d["gh"]), h=torch.zeros_like(d["h"]))
    explicit = _run(zeros, Hd, rows, null_hidden=False)
    for k, v in got.items():
        assert (v == explicit[k]).all(), k
    assert (explicit["dhd"] == d["dhn"].numpy() * (1 - got["gate"][:, Hd:2 * Hd])).all()


def test_h_steps_of_partials_are_one_finalize_source():
    """Two steps' `part` buffers laid end to end (tdmpc_drnn_gate_part_floats each) go through tdmpc_lg_finalize as
    one source of 2 ceil(rows / 32) slices per tensor: the six gradients it writes are the two steps' sums."""
    from tdmpc_amd._lib import LgGsrc
    lib, Hd, rows = _lib(), 96, 33
    n = _part_floats(rows, Hd)
    steps = [R.data(Hd, rows, seed=s) for s in (11, 12)]
    ln = [x.cuda() for x in steps[0]["ln"]]
    tab = _table(ln)
    part = torch.full((2 * n,), float("nan"), device="cuda")
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    for t, d in enumerate(steps):
        gate, lnx, lnr, hn, dgi = z(rows, 3 * Hd), z(rows, 3 * Hd), z(rows, 4), z(rows, Hd), z(rows, 3 * Hd)
        gi, dhn = d["gi"].cuda(), d["dhn"].cuda()
        lib.call("tdmpc_drnn_gate_fwd", gi, None, None, tab, gate, lnx, lnr, hn, rows, Hd, _stream())
        lib.call("tdmpc_drnn_gate_bwd", dhn, None, None, tab, gate, lnx, lnr, dgi, None, None, part[t * n:], rows, Hd,
                 _stream())
    nsl = 2 * R.nparts(rows)
    src = (LgGsrc * 6)()
    for k in range(6):
        src[k].src, src[k].dst, src[k].sstride = part.data_ptr() + 4 * k * Hd, k * Hd, 6 * Hd
        src[k].rows, src[k].cols, src[k].ld, src[k].nslices = 1, Hd, Hd, nsl
    g, normp, step = z(6 * Hd), z(2048), torch.zeros(1, dtype=torch.int32, device="cuda")
    lib.call("tdmpc_lg_finalize", src, 6, g, normp, 2048, step, _stream())
    torch.cuda.synchronize()
    refs = [R.gate(dict(d, ln=steps[0]["ln"]), torch.float64, True) for d in steps]
    sums = {k: refs[0][k] + refs[1][k] for k in R.LN_NAMES}
    got = dict(zip(R.LN_NAMES, g.view(6, Hd).cpu().numpy()))
    for k in R.LN_NAMES:
        f = R.figure(got[k], sums[k])
        print(f"two steps {k}: gpu {f:.3e} (bound {BOUND_BWD:.2e})")
        assert f <= BOUND_BWD, (k, f)


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    """Forward + backward at Hd 224, rows 130 (ragged feature groups, a short last partial): run twice, then captured
    and replayed; every output is bitwise equal."""
    lib, Hd, rows = _lib(), 224, 130
    d = R.data(Hd, rows)
    gi, gh, h, dhn = (d[k].cuda() for k in ("gi", "gh", "h", "dhn"))
    ln = [x.cuda() for x in d["ln"]]
    tab = _table(ln)
    n = _part_floats(rows, Hd)
    shapes = ((rows, 3 * Hd), (rows, 3 * Hd), (rows, 4), (rows, Hd), (rows, 3 * Hd), (rows, 3 * Hd), (rows, Hd), (n,))

    def run(o):
        gate, lnx, lnr, hn, dgi, dgh, dhd, part = o
        lib.call("tdmpc_drnn_gate_fwd", gi, gh, h, tab, gate, lnx, lnr, hn, rows, Hd, _stream())
        lib.call("tdmpc_drnn_gate_bwd", dhn, gh, h, tab, gate, lnx, lnr, dgi, dgh, dhd, part, rows, Hd, _stream())

    outs = [[torch.zeros(*s, device="cuda") for s in shapes] for _ in range(3)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(outs[0])
        run(outs[1])
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        run(outs[2])
    for t in outs[2]:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for x, y, w in zip(*outs):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y) and torch.equal(x, w)


@pytest.mark.parametrize("what,rows,Hd,null,match", [
    ("one row", 1, 96, None, b"rows 1"), ("4097 rows", 4097, 96, None, b"rows 4097"),
    ("Hd 48", 33, 48, None, b"hidden_dim 48"), ("Hd 288", 33, 288, None, b"hidden_dim 288"),
    ("null gi / dhn", 33, 96, "first", b"is null"), ("null h alone", 33, 96, "h", b"h is null"),
    ("null ln entry", 33, 96, "ln", b"ln[4] is null"), ("null part / hn", 33, 96, "last", b"is null")])
def test_refusals_write_nothing(what, rows, Hd, null, match):
    """An inadmissible shape or a null required pointer: TDMPC_E_DIMS with its message, and every output buffer keeps
    its sentinel value."""
    lib = _lib().lib()
    vp = C.c_void_p
    r = max(rows, 2) if rows <= 4096 else 8
    w = min(max(Hd, 32), 256)
    full = lambda *s: torch.full(s, SENTINEL, device="cuda")  # noqa: E731
    gi, gh, h, dhn = full(r, 3 * w), full(r, 3 * w), full(r, w), full(r, w)
    ln = [full(w) for _ in range(6)]
    outs = [full(r, 3 * w), full(r, 3 * w), full(r, 4), full(r, w), full(r, 3 * w), full(r, 3 * w), full(r, w),
            full(8 * 6 * w)]
    gate, lnx, lnr, hn, dgi, dgh, dhd, part = outs
    tab = _table(ln)
    if null == "ln":
        tab[4] = None
    p = lambda t: vp(t.data_ptr())  # noqa: E731
    st = _stream()
    rc = lib.tdmpc_drnn_gate_fwd(None if null == "first" else p(gi), p(gh), None if null == "h" else p(h), tab, p(gate),
                                 p(lnx), p(lnr), None if null == "last" else p(hn), rows, Hd, st)
    assert rc == E_DIMS and match in lib.tdmpc_last_error(), (what, lib.tdmpc_last_error())
    rc = lib.tdmpc_drnn_gate_bwd(None if null == "first" else p(dhn), p(gh), None if null == "h" else p(h), tab,
                                 p(gate), p(lnx), p(lnr), p(dgi), p(dgh), p(dhd), None if null == "last" else p(part),
                                 rows, Hd, st)
    assert rc == E_DIMS and match in lib.tdmpc_last_error(), (what, lib.tdmpc_last_error())
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in outs), what
    # with a hidden state, its two gradients are required
    if null is None and rows == 33 and Hd == 48:
        rc = lib.tdmpc_drnn_gate_bwd(p(dhn), p(gh), p(h), tab, p(gate), p(lnx), p(lnr), p(dgi), None, p(dhd), p(part),
                                     33, 32, st)
        assert rc == E_DIMS and b"dgh is null" in lib.tdmpc_last_error()
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in outs), what
