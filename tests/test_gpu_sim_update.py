"""GPU: the similarity TD-MPC agent's update (tdmpc_amd/sim_learner.py, sim_engine.py, include/tdmpc_sim_learner.h;
DESIGN.md §7 f11) against float64 (tests/sim_update_ref.py, which tests/test_sim_update_cpu.py pins to the reference bit
for bit).

  1  tdmpc_sim_loss_forward / _backward against float64 autograd of the reference's expressions: H = 1, 3; B = 2, 130;
     rho = 1, 0.5; one row past every 1e4 clamp.
  2  the predictor pieces (tdmpc_sim_bn_* / tdmpc_sim_cos_* around the caller's own products) against the float64
     modules, forward and backward: L = 8, 50, 256; rows = 2 (the two-row BatchNorm), 33 (one partial 128-row chunk),
     130 (two chunks, a ragged last one), 4096 (the cap, the other GEMM tile). Loss, running statistics, the queries'
     gradient and every parameter gradient are bitwise those of tdmpc_icem_simloss_fwd / _bwd, which run the same
     kernels around the same products.
  3  two consecutive whole updates on the engine path against the float64 yardstick: (L, A, H, B) = (8, 1, 2, 2),
     (50, 6, 3, 33), (50, 6, 3, 130), (50, 6, 1, 33), (8, 1, 2, 2048) at enc_dim 256, (50, 6, 3, 33) at enc_dim 512.
  4  graph replay against the eager update from the same state, and two runs from the same state: bitwise.
  5  mlp_dim 256 and horizon * batch_size = 4098 take the PyTorch path and meet the same bounds.
  6  TdMpcSim.plan / plan_batch == TDMPC's planner on the same TOLD weights, bitwise; after an update the planner sees
     the new weights.

Bounds of 2: per case, 8 x the figure (max |difference| / max |float64 value|) that the SAME modules show in float32 on
the CPU against float64 on the same inputs, never below 1e-6 (measured in the test itself since the inputs are the
test's own).

Bounds of 3 and 5, by this project's recipe (tests/test_gpu_icem_update.py): per class of results
and per update the figure (sim_update_ref.figures) that the float32 CPU run of the yardstick shows against float64 is
the noise floor -- the largest over 1, 2, 4 and 8 CPU threads, whose summation orders differ, and over the cases of a
group -- and the bound is 8 x that floor, never below 1e-6; B = 2 has its own. `param`, `param0` and `target` are
bounded by what Adam guarantees, 2.01 lr per step taken (drnn_update_ref.bound). grad_norm is compared with the
gradients. At horizon 1 `_dynamics.4.bias` joins `_predictor.0.bias` among the tensors whose gradient is a column sum
that cancels (sim_update_ref.zero_mean).

Floors (float32 CPU against float64, the largest over 1, 2, 4, 8 threads and over the cases of a group):
                  metrics   prio      grad      grad0     stats     param_q
  rest, update 0  6.26e-07  3.85e-07  1.25e-05  3.22e-07  2.08e-07  9.13e-03
  rest, update 1  3.55e-04  7.04e-06  8.46e-04  5.74e-07  3.99e-04  9.14e-03
  B = 2, update 0 4.62e-07  9.90e-08  5.19e-06  3.52e-08  1.28e-07  1.98e-04
  B = 2, update 1 1.32e-06  9.73e-07  4.48e-06  2.33e-07  9.10e-05  3.72e-04
  (param / param0 / target, in lr or tau lr: 0.60 / 1.70 / 0.91 on the rest, 0.04 / 1.47 / 0.89 at B = 2)
GPU figures measured on an MI355X: see DESIGN.md §7 f11 (every comparison prints its figure beside the bound).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sim_update_ref as U
from tdmpc_amd import _lib
from tdmpc_amd.config import make_cfg
from update_gpu import hold, same, yardstick

pytestmark = pytest.mark.gpu

FLOORS = {
    ("rest", 0): dict(metrics=6.263e-07, prio=3.854e-07, grad=1.249e-05, grad0=3.222e-07, stats=2.079e-07, param_q=9.134e-03),
    ("rest", 1): dict(metrics=3.554e-04, prio=7.035e-06, grad=8.462e-04, grad0=5.744e-07, stats=3.992e-04, param_q=9.140e-03),
    ("b2", 0): dict(metrics=4.622e-07, prio=9.899e-08, grad=5.186e-06, grad0=3.521e-08, stats=1.280e-07, param_q=1.976e-04),
    ("b2", 1): dict(metrics=1.319e-06, prio=9.731e-07, grad=4.483e-06, grad0=2.331e-07, stats=9.099e-05, param_q=3.717e-04),
}


def group(name):
    return "b2" if U.CASES[name][3] == 2 else "rest"


def _p(t, off=0):
    return t.data_ptr() + 4 * off


# ---------------------------------------------------------------------------------------------------------------- 1
def _loss_ref(sim, q1, q2, rp, rw, td, w, coefs):
    """The reference's expressions (tdmpc_similarity.py:336-353), [H, B, 1] operands and w [B]."""
    sc, rc, vc, rho_ = coefs
    H = sim.shape[0]
    reward_loss, value_loss, priority_loss = 0, 0, 0
    for t in range(H):
        rho = rho_ ** t
        reward_loss += rho * F.mse_loss(rp[t], rw[t], reduction="none")
        value_loss += rho * (F.mse_loss(q1[t], td[t], reduction="none") + F.mse_loss(q2[t], td[t], reduction="none"))
        priority_loss += rho * (F.l1_loss(q1[t], td[t], reduction="none") + F.l1_loss(q2[t], td[t], reduction="none"))
    similarity_loss = sim.sum(dim=0)
    total = sc * similarity_loss.clamp(max=1e4) + rc * reward_loss.clamp(max=1e4) + vc * value_loss.clamp(max=1e4)
    weighted = (total * w).mean()                             # [B, 1] * [B]: the [B, B] broadcast
    weighted.register_hook(lambda grad: grad * (1 / H))
    return dict(sim=similarity_loss, rew=reward_loss, val=value_loss, prio=priority_loss.clamp(max=1e4), total=total,
                weighted=weighted)


@pytest.mark.parametrize("rho", [1.0, 0.5])
@pytest.mark.parametrize("B", [2, 130])
@pytest.mark.parametrize("H", [1, 3])
def test_sim_loss_kernels_match_float64_autograd(H, B, rho):
    """Row 0 carries similarity, reward, value and priority sums past 1e4: its clamps are active and its gradients zero;
    row 1 does not. fp32 sums of at most 3 terms per row and 130 rows per mean: rtol 1e-5 (atol 1e-6 of the tensor's
    largest entry), update_gpu.same."""
    rs = np.random.RandomState(100 * H + B + int(10 * rho))
    sim, q1, q2, rp, rw, td = (rs.standard_normal((H, B)) for _ in range(6))
    sim = np.abs(sim)
    sim[:, 0] = 2e4
    rp[:, 0] = 300.0 * (1 + np.arange(H))
    q1[:, 0] = 2e4
    w = rs.uniform(0.5, 1.0, B)
    coefs = (1.0, 0.5, 0.1, rho)
    ops = (sim, q1, q2, rp, rw, td)
    t64 = [torch.from_numpy(x).unsqueeze(2).requires_grad_(i < 4) for i, x in enumerate(ops)]
    want = _loss_ref(*t64, torch.from_numpy(w), coefs)
    up = 0.7
    (want["weighted"] * up).backward()
    for k in ("sim", "rew", "val"):
        assert float(want[k][0].detach()) > 1e4 and float(want[k][1].detach()) < 1e4, k
    assert float(want["prio"][0].detach()) == 1e4 and float(want["prio"][1].detach()) < 1e4

    t32 = [torch.from_numpy(x.astype(np.float32)).cuda() for x in ops]
    w32 = torch.from_numpy(w.astype(np.float32)).cuda()
    td0 = t32[5].clone()
    rows, scal = torch.zeros(5, B, device="cuda"), torch.zeros(6, device="cuda")
    grads = [torch.zeros(H, B, device="cuda") for _ in range(4)]
    gw = torch.full((1,), up, device="cuda")
    a = _lib.SimLossArgs(*[_p(t) for t in t32], _p(w32), H, B, *coefs[:3], rho)
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.tdmpc_sim_loss_forward(C.byref(a), _p(rows), _p(scal), st), "tdmpc_sim_loss_forward")
    _lib.check(L.tdmpc_sim_loss_backward(C.byref(a), _p(rows), _p(scal), _p(gw), *[_p(g) for g in grads], st),
               "tdmpc_sim_loss_backward")
    torch.cuda.synchronize()
    assert torch.equal(t32[5], td0), "the TD targets are an input"
    for i, k in enumerate(("sim", "rew", "val", "prio", "total")):
        same(k, rows[i], want[k])
    same("scal", scal, torch.stack([want["sim"].mean(), want["rew"].mean(), want["val"].mean(), want["total"].mean(),
                                    want["weighted"], torch.tensor(float(np.mean(w)))]))
    for i, k in enumerate(("dsim", "dq1", "dq2", "drp")):
        same(k, grads[i], t64[i].grad)
        assert not grads[i][:, 0].any() and grads[i][:, 1].all(), k
    # each output of the backward is optional
    only = torch.zeros(H, B, device="cuda")
    _lib.check(L.tdmpc_sim_loss_backward(C.byref(a), _p(rows), _p(scal), _p(gw), None, None, _p(only), None, st),
               "tdmpc_sim_loss_backward")
    torch.cuda.synchronize()
    assert torch.equal(only, grads[2])


# ---------------------------------------------------------------------------------------------------------------- 2
SHAPES = {8: "cartpole", 50: "cheetah", 256: "dog"}
M = 512
EXACT = 0x100


def _shape_model(L, seed=7):
    from tdmpc_amd.icem_mlp import IcemMlpModel, synthetic_icem_mlp_state_dict
    cfg = make_cfg(SHAPES[L], latent_dim=L)
    model = IcemMlpModel(cfg, init="none")
    model.load_state_dict(synthetic_icem_mlp_state_dict(cfg, seed))
    return cfg, model


def _job(m, n, c, ldc, a, lda, b, ldb, k, amode=0, bmode=0, ones=-1, bias=None):
    return dict(m=m, n=n, c=c, ldc=ldc, seg=(a, b, lda, ldb, k, amode, bmode, ones), bias=bias)


def _gemm(jobs, like=None):
    """One grouped tdmpc_lg_gemm launch on the exact f32 MFMA with the tile the similarity loss's own launches take:
    64 x 64 tiles once the largest job (of `like`, the (m, n) of the jobs that share the launch there) fills the chip."""
    big = max(-(-m // 64) * -(-n // 64) for m, n in (like or [(j["m"], j["n"]) for j in jobs]))
    arr = (_lib.LgJob * len(jobs))()
    for J, j in zip(arr, jobs):
        s = J.seg[0]
        s.a, s.b, s.lda, s.ldb, s.k, s.amode, s.bmode, s.ones_col = j["seg"]
        J.nseg, J.m, J.n, J.epi, J.c, J.ldc, J.bias, J.splits = 1, j["m"], j["n"], 0, j["c"], j["ldc"], j["bias"], 1
    _lib.check(_lib.lib().tdmpc_lg_gemm(arr, len(jobs), (2 if big >= 256 else 1) | EXACT,
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tdmpc_lg_gemm")


def _modules(model, x, keys, dloss):
    """`_predictor` in train mode + the cosine loss on the eager modules in the model's precision -> loss, the queries'
    gradient under dloss, the parameter gradients, the running statistics."""
    model.train()
    x = x.clone().requires_grad_(True)
    pred = F.normalize(model.pred_z(x), dim=-1, p=2)
    loss = 2.0 - 2.0 * (pred * F.normalize(keys, dim=-1, p=2)).sum(dim=-1)
    model.zero_grad()
    loss.backward(dloss)
    p = model._predictor
    return dict(loss=loss.detach(), dq=x.grad, stats=torch.cat([p[1].running_mean, p[1].running_var]).detach(),
                **{f"d{k}": v.grad for k, v in p.named_parameters()})


@pytest.mark.parametrize("R", [2, 33, 130, 4096])
@pytest.mark.parametrize("L", [8, 50, 256])
def test_predictor_pieces_match_float64_modules_and_the_similarity_loss_bitwise(L, R):
    from tdmpc_amd.icem_learner import IcemTrainStep
    rs = np.random.RandomState(1000 * L + R)
    x, keys = (rs.standard_normal((R, L)).astype(np.float32) for _ in range(2))
    dloss = rs.uniform(0.5, 1.5, R).astype(np.float32)
    t = lambda a, dt: torch.from_numpy(a).to(dt)  # noqa: E731
    want = _modules(_shape_model(L)[1].double(), t(x, torch.float64), t(keys, torch.float64), t(dloss, torch.float64))
    cpu = _modules(_shape_model(L)[1], t(x, torch.float32), t(keys, torch.float32), t(dloss, torch.float32))

    # the similarity loss's own entry points (tdmpc_icem_simloss_fwd / _bwd through their autograd wrapper)
    _, ma = _shape_model(L)
    ma = ma.cuda().train()
    step = IcemTrainStep(ma, max_loss_rows=R)
    xa = torch.from_numpy(x).cuda().requires_grad_(True)
    la = step.similarity_loss(xa, torch.from_numpy(keys).cuda())
    la.backward(torch.from_numpy(dloss).cuda())
    pa = ma._predictor

    # the pieces around the test's own products
    _, mb = _shape_model(L)
    mb = mb.cuda().train()
    pb = mb._predictor
    lib = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    xg, kg, dl = (torch.from_numpy(v).cuda() for v in (x, keys, dloss))
    n = C.c_size_t()
    _lib.call("tdmpc_sim_bn_part_floats", R, C.byref(n))
    assert n.value == -(-R // 128) * 2 * M
    p1, xhat, rstd, e, pred, loss, part = z(R, M), z(R, M), z(M), z(R, M), z(R, L), z(R), z(n.value)
    w0, b0, w3, b3 = pb[0].weight, pb[0].bias, pb[3].weight, pb[3].bias
    _gemm([_job(R, M, _p(p1), M, _p(xg), L, _p(w0), L, L, bias=_p(b0))])
    _lib.check(lib.tdmpc_sim_bn_fwd(_p(p1), _p(pb[1].weight), _p(pb[1].bias), _p(pb[1].running_mean),
                                    _p(pb[1].running_var), _p(xhat), _p(rstd), _p(e), _p(part), R, st), "bn_fwd")
    _gemm([_job(R, L, _p(pred), L, _p(e), M, _p(w3), M, M, bias=_p(b3))])
    _lib.check(lib.tdmpc_sim_cos_fwd(_p(pred), _p(kg), _p(loss), R, L, st), "cos_fwd")
    dpred, de, dg, db, dq = z(R, L), z(R, M), z(M), z(M), z(R, L)
    dw3, dw0 = z(L, M + 1), z(M, L + 1)
    _lib.check(lib.tdmpc_sim_cos_bwd(_p(pred), _p(kg), _p(dl), _p(dpred), R, L, st), "cos_bwd")
    _gemm([_job(R, M, _p(de), M, _p(dpred), L, _p(w3), M, L, bmode=1)])
    _lib.check(lib.tdmpc_sim_bn_bwd(_p(de), _p(pb[1].weight), _p(xhat), _p(rstd), _p(e), _p(part), _p(de), _p(dg),
                                    _p(db), R, st), "bn_bwd")
    _gemm([_job(R, L, _p(dq), L, _p(de), M, _p(w0), L, M, bmode=1),
           _job(L, M + 1, _p(dw3), M + 1, _p(dpred), L, _p(e), M, R, amode=1, bmode=1, ones=M),
           _job(M, L + 1, _p(dw0), L + 1, _p(de), M, _p(xg), L, R, amode=1, bmode=1, ones=L)])
    torch.cuda.synchronize()
    got = {"loss": loss, "dq": dq, "stats": torch.cat([pb[1].running_mean, pb[1].running_var]), "d0.weight": dw0[:, :L],
           "d0.bias": dw0[:, L], "d1.weight": dg, "d1.bias": db, "d3.weight": dw3[:, :M], "d3.bias": dw3[:, M]}
    ref = {"loss": la.detach(), "dq": xa.grad, "stats": torch.cat([pa[1].running_mean, pa[1].running_var]).detach(),
           **{f"d{k}": v.grad for k, v in pa.named_parameters()}}
    assert not torch.equal(got["stats"], torch.cat([_shape_model(L)[1]._predictor[1].running_mean,
                                                    _shape_model(L)[1]._predictor[1].running_var]).cuda())
    # d0.bias is the column sum that the BatchNorm cancels: measured against the sum of |dL / d(pre-BatchNorm)|
    cancel = float(de.abs().sum(0).max())
    over = {}
    for k, v in got.items():
        assert torch.equal(v, ref[k]), (f"{k}: the pieces and tdmpc_icem_simloss_* differ",
                                        float((v - ref[k]).abs().max()))
        scale = cancel if k == "d0.bias" else None
        f = U.figure(v.double().cpu().numpy(), want[k].numpy(), scale)
        floor = U.figure(cpu[k].double().numpy(), want[k].numpy(), scale)
        b = max(8 * floor, 1e-6)
        print(f"predictor pieces L {L} rows {R} {k}: gpu {f:.3e} (cpu fp32 {floor:.3e}, bound {b:.2e})")
        if not f <= b:
            over[k] = (f, b)
    assert not over, over


# ---------------------------------------------------------------------------------------------------------------- 3, 4, 5
def _gpu_learner(name, graph=False, warmup=3, **cfg_over):
    from tdmpc_amd.sim_learner import SimLearner
    cfg = U.case_cfg(name)
    for k, v in cfg_over.items():
        setattr(cfg, k, v)
    model, target = U.make_models(cfg, name, device="cuda")
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cuda"), planner=None)
    learner = SimLearner(agent, graph=graph, warmup=warmup)
    buf = U.FakeBuffer(tuple(t.cuda() for t in U.case_batch(name)))
    return cfg, agent, learner, buf


def _snap(agent, buf, m):
    torch.cuda.synchronize()
    r = dict(metrics=np.array(m.tolist() + [0.0]), prio=buf.prios[-1].cpu().numpy(), grads=U.grads_of(agent.model))
    return U.snapshot(r, agent.model, agent.model_target)


def _two_updates(name, path):
    want, scales = yardstick(U, name)
    cfg, agent, learner, buf = _gpu_learner(name)
    assert learner.path == path and (learner.engine is not None) == (path == "engine")
    noise = [[n.cuda() for n in nz] for nz in U.case_noise(name)]
    for k, step in enumerate(U.STEPS):
        m = learner.update(buf, step, noise[k])
        assert not agent.model.training and m.is_cuda and m.shape == (7,)
        hold(U, f"{name} update {k}", _snap(agent, buf, m), want[k], scales[k], cfg, FLOORS[(group(name), k)], k)
        assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + (k + 1)
    return agent, learner


@pytest.mark.parametrize("name", ["tiny", "cheetah", "wide", "h1", "cap", "e512"])
def test_two_consecutive_engine_updates_match_float64(name):
    agent, learner = _two_updates(name, "engine")
    eng = learner.engine
    # the BatchNorm's buffers are the module's own tensors, outside the flat parameter / gradient / Adam buffers
    lo, hi = eng.P.data_ptr(), eng.P.data_ptr() + 4 * eng.P.numel()
    bn = agent.model._predictor[1]
    for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked):
        assert not lo <= t.data_ptr() < hi
    for k, p in agent.model.named_parameters():
        assert lo <= p.data_ptr() < hi and p.data_ptr() % 16 == 0, k
    assert agent.optim is eng.opt_main and agent.pi_optim is eng.opt_pi
    assert eng.opt_pi.lr == float(learner.cfg.pi_lr) and eng.opt_main.lr == float(learner.cfg.lr)


@pytest.mark.parametrize("name", ["m256", "over"])
def test_what_the_engine_does_not_admit_takes_the_pytorch_path_and_meets_the_same_bounds(name):
    agent, learner = _two_updates(name, "torch")
    assert isinstance(agent.optim, torch.optim.Adam)


def _differences(a, b):
    differ = []
    for u in range(len(a)):
        for cls in a[u]:
            for k in a[u][cls]:
                if not np.array_equal(a[u][cls][k], b[u][cls][k]):
                    differ.append((u, cls, k, float(np.abs(a[u][cls][k] - b[u][cls][k]).max())))
    return differ


def test_graph_replay_equals_the_eager_update_from_the_same_state_bitwise():
    """wide (four BatchNorm chunks) with min_std = 0 (the TruncatedNormal draws are multiplied by zero, so the eager and
    the captured update compute the same whatever the generator gives). Two graph-mode learners run the first update
    eagerly from the same state. Then A runs the second update eagerly -- explicit draws, which min_std = 0 ignores,
    keep a call eager -- and B captures and replays it: every class of result is bitwise equal."""
    runs = []
    for replay in (False, True):
        cfg, agent, learner, buf = _gpu_learner("wide", graph=True, warmup=1, min_std=0.0)
        assert learner.path == "engine"
        eager = [torch.zeros(cfg.batch_size, cfg.action_dim, device="cuda") for _ in range(2 * cfg.horizon + 1)]
        snaps = []
        for k, step in enumerate(U.STEPS):
            m = learner.update(buf, step, eager if k and not replay else None)
            snaps.append(_snap(agent, buf, m))
            assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + (k + 1)
        runs.append((snaps, learner))
    (a, la), (b, lb) = runs
    assert lb._graphs and not la._graphs, "the second update was not captured"
    differ = _differences(a, b)
    print("graph replay against eager:", differ or "bitwise equal")
    assert not differ, differ


@pytest.mark.parametrize("name", ["cheetah", "wide"])
def test_two_runs_from_the_same_state_agree_bitwise(name):
    runs = []
    for _ in range(2):
        cfg, agent, learner, buf = _gpu_learner(name)
        noise = [[n.cuda() for n in nz] for nz in U.case_noise(name)]
        runs.append([_snap(agent, buf, learner.update(buf, step, noise[k])) for k, step in enumerate(U.STEPS)])
    differ = _differences(*runs)
    assert not differ, differ


def test_update_pi_on_the_engine_steps_the_policy_alone_at_pi_lr():
    cfg, agent, learner, buf = _gpu_learner("cheetah", pi_lr=2e-3)
    assert learner.path == "engine" and learner.engine.opt_pi.lr == 2e-3 and learner.engine.opt_main.lr == cfg.lr
    before = {k: v.detach().clone() for k, v in agent.model.state_dict().items()}
    rs = np.random.RandomState(9)
    zs = [torch.from_numpy(rs.standard_normal((cfg.batch_size, cfg.latent_dim)).astype(np.float32)).cuda()
          for _ in range(cfg.horizon + 1)]
    loss = learner.update_pi(zs)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    for k, v in agent.model.state_dict().items():
        assert torch.equal(v, before[k]) == (not k.startswith("_pi.")), k
    # Adam's first step is lr sign(g) wherever |g| >> eps: the step size shows which learning rate was used
    d = (agent.model._pi[0].weight - before["_pi.0.weight"]).abs().max()
    assert 1.9e-3 < float(d) <= 2e-3 * (1 + 1e-5)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_plan_is_tdmpcs_planner_on_the_told_tensors_and_sees_the_updated_weights():
    from tdmpc_amd import TDMPC, TOLD, TdMpcSim
    from tdmpc_amd.icem_mlp import synthetic_icem_mlp_state_dict
    from tdmpc_amd.replay import ReplayBuffer
    from tdmpc_amd.tdmpc_sim import SimPlanner
    cfg = U.case_cfg("cheetah")
    for k, v in dict(num_samples=32, num_elites=8, iterations=2, train_steps=500, episode_length=50,
                     max_buffer_size=10**6, env_horizon=cfg.horizon).items():
        setattr(cfg, k, v)
    rs = np.random.RandomState(5)
    sd = synthetic_icem_mlp_state_dict(cfg, 71)
    agent = TdMpcSim(cfg, max_batch=3, graph=True)
    agent.model.load_state_dict(sd)
    agent.model_target.load_state_dict(synthetic_icem_mlp_state_dict(cfg, 72))
    assert agent._learner is None

    def told_agent(weights):
        """TDMPC over a TOLD with the LayerNorm encoder and the same planner class: the same packed tensors."""
        t = TDMPC(cfg, max_batch=3)
        t.model = TOLD(cfg, init="none", enc_norm=True).to(t.device).eval()
        t.model.load_state_dict({k: v for k, v in weights.items() if not k.startswith("_predictor")})
        t.planner = SimPlanner(cfg, max_batch=3, device=t.device)
        return t
    told = told_agent(sd)
    # (update() sets std from std_schedule: plan at that value before and after, so that only the weights differ)
    from tdmpc_amd.config import linear_schedule
    agent.std = told.std = linear_schedule(cfg.std_schedule, 20005)
    O = cfg.obs_shape[0]
    obs = rs.standard_normal((3, O)).astype(np.float32)

    def plan(ag, batch):
        torch.manual_seed(11)
        np.random.seed(12)
        if batch == 1:
            return ag.plan(obs[0], step=30000, t0=True)[0]
        return ag.plan_batch(obs[:batch], step=30000, t0=True)[0].clone()
    a1, a3 = plan(agent, 1), plan(agent, 3)
    # the encoder the planner packed is the model's, LayerNorm included (the x6 products: fp32-accurate)
    og = torch.from_numpy(obs).cuda()
    torch.testing.assert_close(agent.planner.encode(og), agent.model.h(og).detach(), rtol=1e-4, atol=1e-4)
    assert torch.equal(a1, plan(told, 1)) and torch.equal(a3, plan(told, 3))
    assert agent._learner is None                                         # planning built no learner
    assert a1.shape == (cfg.action_dim,) and a3.shape == (3, cfg.action_dim) and torch.isfinite(a3).all()

    buf = ReplayBuffer(cfg, latent_plan=True)
    A = cfg.action_dim
    for _ in range(3):
        buf.add(SimpleNamespace(obs=torch.from_numpy(rs.standard_normal((51, O)).astype(np.float32)),
                                action=torch.from_numpy(rs.uniform(-1, 1, (50, A)).astype(np.float32)),
                                reward=torch.from_numpy(rs.standard_normal(50).astype(np.float32))))
    for k in range(5):
        m = agent.update(buf, 20000 + k)
        assert not agent.model.training
        assert int(agent.model._predictor[1].num_batches_tracked) == 1000 + (k + 1)
    assert list(m) == list(U.METRICS) and all(isinstance(v, float) and np.isfinite(v) for v in m.values())
    assert agent.learner.path == "engine" and agent.learner._graphs, "the learner never replayed its captured graph"
    t = agent.update(buf, 20005, sync_metrics=False)
    assert torch.is_tensor(t["total_loss"]) and t["total_loss"].is_cuda and t["total_loss"].dim() == 0
    b1, b3 = plan(agent, 1), plan(agent, 3)
    assert not torch.equal(a1, b1) and not torch.equal(a3, b3)            # the planner saw the new weights
    fresh = TdMpcSim(cfg, max_batch=3, graph=False)
    fresh.model.load_state_dict(agent.model.state_dict())
    fresh.std = agent.std
    assert torch.equal(plan(fresh, 1), b1) and torch.equal(plan(fresh, 3), b3)
    other = told_agent(agent.model.state_dict())
    other.std = agent.std
    assert torch.equal(plan(other, 1), b1)
    w_pi = agent.model._pi[0].weight.detach().clone()
    zs = [torch.from_numpy(rs.standard_normal((cfg.batch_size, cfg.latent_dim)).astype(np.float32)).cuda()
          for _ in range(cfg.horizon + 1)]
    assert np.isfinite(agent.update_pi(zs)) and not torch.equal(w_pi, agent.model._pi[0].weight)
    assert not torch.equal(plan(agent, 1), b1)
