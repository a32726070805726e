"""GPU: the DSSM learner kernels (csrc/drnn_learner.hip behind tdmpc_amd.dssm_train.DssmTrainStep) against float64
autograd over the eager `tdmpc_amd.dssm` modules in train() mode (tests/drnn_train_ref.py; weights
synthetic_dssm_state_dict seed 7, inputs as tests/test_gpu_drnn_shapes.py::_inputs).

  shape (task, L, Hd)       exercises
  (cartpole, 8, 32)         one gate block; the one-wide action as a K segment
  (cheetah, 64, 96)         Hd not a multiple of 64
  (humanoid, 129, 224)      ragged latent width, 7 gate blocks
  (dog, 256, 256)           the widest
  rows 2                    the smallest legal batch: variance over two rows, R / (R - 1) = 2
  rows 33                   ragged row block
  rows 130                  more than one partial per column reduction, a ragged tail
  rows 512, once, at the stock (humanoid, 100, 128): the learner's batch size

Forward (z', h', r, the similarity loss, the updated running statistics): parity_util.close, 1e-5 + 1e-4 |ref|.

Gradients: per tensor max |got - f64| / max |f64| (drnn_train_ref.figure, with its two documented special scales),
bounded by 8 x the largest such figure fp32 CPU autograd itself shows against float64 on these cases (measured by
tests/test_drnn_train_cpu.py::test_fp32_gradient_error_the_gpu_bound_is_derived_from and quoted below), never below
1e-6. Why 8: K runs up to 512 and the row sums up to 512 terms; a different but fixed summation order moves fp32
results by a small multiple of what the CPU's order does. The rows-2 cases carry their own constant: a BatchNorm over two
rows has xhat = +-1 and 1 / std up to ~300, which amplifies every rounding error -- in fp32 CPU autograd as well
(3.9e-05 there against 1.0e-06 on the other cases) -- and one constant for all would leave the well-conditioned cases
forty times the room they need. Every comparison prints the GPU figure beside the fp32 CPU figure.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import drnn_train_ref as R
from parity_util import close

pytestmark = pytest.mark.gpu

# fp32 CPU autograd against float64 autograd, largest gradient figure over the cases of each group
FP32_CPU_ROWS2 = 3.915e-05   # (cheetah, 64, 96) rows 2, _dynamics.gru_cell.ln_reset.weight
FP32_CPU_REST = 1.010e-06    # (dog, 256, 256) rows 33, _dynamics.gru_cell.ln_reset.weight; through time: 9.8e-07
BOUND_ROWS2 = max(8 * FP32_CPU_ROWS2, 1e-6)
BOUND_REST = max(8 * FP32_CPU_REST, 1e-6)
E_DIMS = -1   # TDMPC_E_DIMS (include/tdmpc_hip.h)


def _names(model, prefixes):
    return [k for k, _ in model.named_parameters() if k.startswith(prefixes)]


_REF = {}


def _reference(case):
    """Per case, computed once and left unchanged: the data, float64 and fp32 CPU results of next and of the loss."""
    if case not in _REF:
        cfg, d = R.case_data(*case)
        m64, m32 = R.make_model(cfg, torch.float64), R.make_model(cfg, torch.float32)
        nn_, ln = _names(m64, ("_dynamics", "_reward")), _names(m64, ("_predictor",))
        pre = R.PreBN(m64)
        want = (R.run_next(m64, m64.next, d, nn_), R.run_loss(m64, lambda q, k: R.similarity_loss(m64, q, k), d, ln))
        sc = pre.scales()
        cpu = (R.run_next(m32, m32.next, d, nn_), R.run_loss(m32, lambda q, k: R.similarity_loss(m32, q, k), d, ln))
        _REF[case] = (cfg, d, want, cpu, sc, nn_, ln)
    return _REF[case]


def _gpu_step(cfg, rows, **kw):
    from tdmpc_amd.dssm_train import DssmTrainStep
    model = R.make_model(cfg, torch.float32, device="cuda")
    return model, DssmTrainStep(model, max_rows=rows, **kw)


def _check_forward(tag, got, want, cpu):
    for grp in ("out", "stats"):
        for k, w in want[grp].items():
            g, c = got[grp][k].reshape(w.shape), cpu[grp][k]
            print(f"{tag} {k}: max |gpu - f64| {np.abs(g - w).max():.3e}, max |fp32cpu - f64| {np.abs(c - w).max():.3e}")
            bad = ~close(g, w)
            assert not bad.any(), (tag, k, np.abs(g - w).max(), np.argwhere(bad)[:4].tolist())


def _check_grads(tag, got, want, cpu, scales, bound):
    gf, cf = R.grad_figures(got, want, scales), R.grad_figures(cpu, want, scales)
    for k in gf:
        print(f"{tag} grad {k}: gpu {gf[k]:.3e}, fp32cpu {cf[k]:.3e} (bound {bound:.2e})")
    over = {k: v for k, v in gf.items() if not v <= bound}
    assert not over, (tag, over)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "-".join(map(str, c)))
def test_next_and_similarity_loss_match_float64(case):
    """One `next` and one `similarity_loss`, forward and backward, per (shape, rows): outputs and running statistics
    within `close`, num_batches_tracked + 1, every input and parameter gradient within the bound of its group. Three of
    the rows-33 cases leave dz', dh' or dr out (drnn_train_ref.ABSENT)."""
    cfg, d, want, cpu, sc, nn_, ln = _reference(case)
    rows = case[3]
    model, step = _gpu_step(cfg, rows)
    bound = BOUND_ROWS2 if rows == 2 else BOUND_REST
    tag = "%s L %d Hd %d rows %d" % case
    got = R.run_next(model, step.next, d, nn_)
    assert got["nbt"] == 1
    _check_forward(tag, got, want[0], cpu[0])
    _check_grads(tag, got, want[0], cpu[0], sc, bound)
    got = R.run_loss(model, step.similarity_loss, d, ln)
    assert got["nbt"] == 1
    _check_forward(tag + " loss", got, want[1], cpu[1])
    _check_grads(tag + " loss", got, want[1], cpu[1], sc, bound)


def test_three_steps_through_time_match_float64():
    """T = 3 steps of `next` chained by autograd at (cheetah, 64, 96), rows 33, each predicted latent feeding the next
    step; loss = mean similarity loss of the three predictions (passed as a list) against fixed keys + the sum of the
    rewards. Parameter gradients (prior_mlp's BatchNorm affine is hit three times) within BOUND_REST, the running
    statistics after three updates within `close`, and no saved buffer is left taken."""
    cfg, d = R.bptt_data()
    m64, m32 = R.make_model(cfg, torch.float64), R.make_model(cfg, torch.float32)
    names = _names(m64, ("_dynamics", "_reward", "_predictor"))
    pre = R.PreBN(m64)
    want = R.run_bptt(m64, m64.next, lambda q, k: R.similarity_loss(m64, q, k), d, names)
    sc = pre.scales()
    cpu = R.run_bptt(m32, m32.next, lambda q, k: R.similarity_loss(m32, q, k), d, names)
    model, step = _gpu_step(cfg, R.BPTT[3], max_steps=3)
    got = R.run_bptt(model, step.next, step.similarity_loss, d, names)
    _check_forward("through time", got, want, cpu)
    _check_grads("through time", got, want, cpu, sc, BOUND_REST)
    assert int(model._dynamics.prior_mlp[1].num_batches_tracked) == 1003
    assert int(model._predictor[1].num_batches_tracked) == 1001
    assert len(step._next_pool.free) == 3 and len(step._loss_pool.free) == 2


def test_more_live_calls_than_saved_buffers_raise():
    cfg, d = R.bptt_data()
    model, step = _gpu_step(cfg, R.BPTT[3], max_steps=2)
    z, h, a = d["z"].cuda(), d["h"].cuda(), d["acts"][0].cuda()
    live = [step.next(z, a, h), step.next(z, a, h)]
    with pytest.raises(RuntimeError, match="max_steps"):
        step.next(z, a, h)
    del live
    with torch.no_grad():   # no graph: nothing stays taken, and the train-mode forward still runs
        for _ in range(3):
            out = step.next(z, a, h)
    assert all(o.grad_fn is None and not o.requires_grad for o in out)
    assert len(step._next_pool.free) == 2


def _fwd_bwd(step, params, z, a, h, q, k, up, dl):
    """Outputs and gradients, detached: no autograd node (and so no gradient accumulator of a leaf, which remembers
    the stream it was created on) outlives the call."""
    zo, ho, r = step.next(z, a, h)
    loss = step.similarity_loss(q, k)
    total = (zo * up[0]).sum() + (ho * up[1]).sum() + (r * up[2]).sum() + (loss * dl).sum()
    grads = torch.autograd.grad(total, [z, a, h, q] + params)
    return [t.detach() for t in [zo, ho, r, loss] + list(grads)]


def test_two_runs_and_a_graph_replay_give_the_same_bits():
    """The same forward + backward of `next` and the loss at (humanoid, 129, 224), rows 130 (two partials per column,
    ragged everything): run twice, then captured in a graph and replayed; every output and gradient is bitwise equal.
    The eager runs and the capture share one side stream, as torch's whole-network capture asks: a backward captured
    while a leaf's gradient accumulator from a run on another stream is alive makes that stream wait on the capturing
    one, a cross-stream dependency that is never joined."""
    case = ("humanoid", 129, 224, 130)
    cfg, d = R.case_data(*case)
    model, step = _gpu_step(cfg, case[3])
    params = [p for k, p in model.named_parameters() if k.startswith(("_dynamics", "_reward", "_predictor"))]
    z, a, h, q = (d[n].cuda().requires_grad_(True) for n in ("z", "a", "h", "q"))
    k, dl = d["k"].cuda(), d["dl"].cuda()
    up = [u.cuda() for u in d["up"]]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        first = [t.clone() for t in _fwd_bwd(step, params, z, a, h, q, k, up, dl)]
        second = [t.clone() for t in _fwd_bwd(step, params, z, a, h, q, k, up, dl)]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for x, y in zip(first, second):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        static = _fwd_bwd(step, params, z, a, h, q, k, up, dl)
    for t in static:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for x, y in zip(first, static):
        assert torch.equal(x, y)


def test_refusals_on_the_device():
    """A refused call (one row) leaves its output buffers at their sentinel value and launches nothing; calling with
    the model in eval() raises and points to the planner's next."""
    cfg = R.cfg_for("cheetah", 64, 96)
    model, step = _gpu_step(cfg, 33)
    z, a, h = (t.cuda() for t in R.inputs(np.random.RandomState(1), 1, cfg))
    S = 12345.0
    zo, ho, ro, lo = (torch.full(s, S, device="cuda") for s in ((1, 64), (1, 96), (1,), (1,)))
    from tdmpc_amd import _lib, dssm_train
    vp = C.c_void_p
    tab, n = dssm_train._table(step._next_params, step._next_stats)
    slot = step._next_pool.bufs[0]
    st = vp(torch.cuda.current_stream().cuda_stream)
    L = _lib.lib()
    rc = L.tdmpc_drnn_next_fwd(C.byref(step.dims), tab, n, vp(z.data_ptr()), vp(a.data_ptr()), vp(h.data_ptr()), 1,
                               vp(zo.data_ptr()), vp(ho.data_ptr()), vp(ro.data_ptr()), vp(slot.data_ptr()),
                               slot.numel(), vp(step._ws.data_ptr()), step._ws.numel(), st)
    assert rc == E_DIMS and L.tdmpc_last_error()
    ltab, ln = dssm_train._table(step._loss_params, step._loss_stats)
    lslot = step._loss_pool.bufs[0]
    rc = L.tdmpc_drnn_simloss_fwd(C.byref(step.dims), ltab, ln, vp(z.data_ptr()), vp(z.data_ptr()), 1,
                                  vp(lo.data_ptr()), vp(lslot.data_ptr()), lslot.numel(), vp(step._ws.data_ptr()),
                                  step._ws.numel(), st)
    assert rc == E_DIMS and L.tdmpc_last_error()
    torch.cuda.synchronize()
    assert all(bool((t == S).all()) for t in (zo, ho, ro, lo)), "a refused call wrote its outputs"
    with pytest.raises(RuntimeError, match="rows 1"):
        step.next(z, a, h)
    z, a, h = (t.cuda() for t in R.inputs(np.random.RandomState(1), 33, cfg))
    model.eval()
    with pytest.raises(RuntimeError, match="DrnnPlanner.next"):
        step.next(z, a, h)
    with pytest.raises(RuntimeError, match="eval"):
        step.similarity_loss(z, z)
    assert int(model._dynamics.prior_mlp[1].num_batches_tracked) == 1000
    model.train()
    assert torch.isfinite(step.next(z, a, h)[0]).all()
