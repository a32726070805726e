"""Throughput of the recurrent-latent iCEM planner (TdIcemDrnn) on one MI355X, with the neighbours it was built from.

    python tools/drnn_icem_bench.py [--out profiles/r08/drnn_icem_bench.json] [--envs 1,32] [--reps 7] [--calls 20]

Shape: humanoid (L 100, A 21, Hd 128), N = 512 shrinking by 1.25 over 6 iterations, K = 64 (16 reused), H = 5,
mixture 0.5, noise_beta 2.5. Per batch size, from one run:
  * `icem_drnn_plan`: TdIcemDrnn.plan_batch, rng "device", graph replay, warm calls with elite reuse; `reps` timed
    batches of `calls` calls between HIP events after a warm-up, the median is the figure;
  * `drnn_plan` / `icem_plan`: TdMpcDrnn (rng "fused") and TdICEM (rng "device") at the same shape, timed the same way;
  * `drnn_step_kernel`: the step kernel's launches of eager plans, per iCEM row count B * (N_i + E_i) and for the
    policy pre-rollout's B * P0, through tdmpc_drnn_profile_begin / _end;
  * `noise_new`: this agent's device draw per call (two normal_, one tdmpc_drnn_colored_noise launch, the uniforms),
    eager between HIP events; `noise_parent`: the parent's construction of the same blocks (the stream's normal_,
    BatchedColoredNoise.draw, the indexed store through precomputed positions, the uniforms), as TdICEM._draw_device.
The CPU figure is the float32 restatement (tests/drnn_icem_ref.py) on 16 host threads, one env. No GPU: it fails.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tdmpc_amd import _lib  # noqa: E402
from tdmpc_amd.colored_noise import BatchedColoredNoise  # noqa: E402
from tdmpc_amd.config import make_cfg  # noqa: E402
from drnn_bench import summary, timed_batches  # noqa: E402


def bench_cfg():
    return make_cfg("humanoid", num_samples=512, num_elites=64, iterations=6, horizon=5, hidden_dim=128,
                    norm_cell=True, plan2expl=False, warmup_len=0, regularization_schedule="0.5")


def parent_noise(agent, B, H, cts, off, reuse):
    """The same coloured blocks built as TdICEM._draw_device builds its own: one BatchedColoredNoise over the blocks
    of B envs and the int64 stream position of every float."""
    cfg, pl = agent.cfg, agent.planner
    A, S = cfg.action_dim, off["total"]
    specs, pos = [], []
    t = np.arange(H)[None, None, :]
    a = np.arange(A)[None, :, None]
    for n, dst in agent._colored_blocks(H, cts, off, reuse):
        r = np.arange(n)[:, None, None]
        p = dst + t * n * A + r * A + a                      # [n, A, H]
        for e in range(B):
            specs.append((cfg.noise_beta, n))
            pos.append(p.reshape(n * A, H) + e * S)
    gen = BatchedColoredNoise(specs, A, H, H, agent.device)
    posd = torch.as_tensor(np.concatenate(pos), dtype=torch.int64, device=agent.device)

    def draw():
        pl.noise_flat[:B * S].normal_()
        pl.noise_flat[posd] = gen.draw()
        pl.u[:B].uniform_()
    return draw, posd.numel()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--envs", default="1,32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--cpu-calls", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("drnn_icem_bench needs a GPU: nothing is measured without one")
    from tdmpc_amd.drnn import TdMpcDrnn
    from tdmpc_amd.drnn_icem import TdIcemDrnn
    from tdmpc_amd.dssm import synthetic_dssm_state_dict
    from tdmpc_amd.icem import TdICEM
    from tdmpc_amd.told import synthetic_state_dict
    cfg = bench_cfg()
    sd = synthetic_dssm_state_dict(cfg, 0)
    out = {"shape": "humanoid L100 A21 Hd128 M512, N=512/1.25 K=64 E=16 H=5 I=6, noise_beta 2.5",
           "device": torch.cuda.get_device_name(0), "envs": {}}
    step = 10**6
    for B in [int(x) for x in args.envs.split(",") if x]:
        rs = np.random.RandomState(B)
        obs = rs.standard_normal((B, cfg.obs_shape[0])).astype(np.float32)
        hidden = rs.uniform(-1, 1, (B, cfg.hidden_dim)).astype(np.float32)
        agent = TdIcemDrnn(cfg, max_batch=B, rng="device")
        agent.model.load_state_dict(sd)
        agent.std = 0.05
        agent.plan_batch(obs, hidden, step=step, t0=True)
        ms = timed_batches(lambda: agent.plan_batch(obs, hidden, step=step, t0=False), args.reps, args.calls)
        leg = {"icem_drnn_plan": summary(ms, B)}
        cts = agent.counts(agent.mixture_coef, True, False)
        H = agent.plan_horizon
        off = agent.layout(H, cts, True)
        leg["counts_N_P_E"] = cts
        leg["stream_floats_per_env"] = off["total"]
        # the step kernel per row count (eager launches between HIP events)
        agent.graph = False
        agent.plan_batch(obs, hidden, step=step, t0=False)
        torch.cuda.synchronize()
        steps = {}
        for rows in sorted({B * (n + e) for n, _, e in cts} | {B * cts[0][1]}):
            _lib.call("tdmpc_drnn_profile_begin", rows, 4096)
            for _ in range(4):
                agent.plan_batch(obs, hidden, step=step, t0=False)
            n, tms, fl = C.c_int32(), C.c_double(), C.c_double()
            _lib.call("tdmpc_drnn_profile_end", C.byref(n), C.byref(tms), C.byref(fl))
            if n.value:
                steps[str(rows)] = {"launches_per_plan": n.value // 4, "us_per_launch": round(tms.value / n.value * 1e3, 2),
                                    "tflops_algorithmic": round(fl.value / tms.value / 1e9, 2)}
        leg["drnn_step_kernel"] = steps
        leg["drnn_step_kernel_ms_per_plan"] = round(sum(v["launches_per_plan"] * v["us_per_launch"]
                                                        for v in steps.values()) / 1e3, 4)
        # the noise: this agent's draw and the parent's construction of the same blocks
        ms = timed_batches(lambda: agent._draw_device(B, H, cts, off, True), args.reps, args.calls)
        leg["noise_new"] = summary(ms, B)
        draw, npos = parent_noise(agent, B, H, cts, off, True)
        ms = timed_batches(draw, args.reps, args.calls)
        leg["noise_parent"] = summary(ms, B)
        leg["noise_parent"]["index_positions"] = npos
        for k in ("noise_new", "noise_parent"):
            leg[k].pop("plan_steps_per_s")
        del agent, draw
        drnn = TdMpcDrnn(cfg, max_batch=B, rng="fused")
        drnn.model.load_state_dict(sd)
        drnn.std = 0.05
        drnn.plan_batch(obs, hidden, step=step, t0=True)
        ms = timed_batches(lambda: drnn.plan_batch(obs, hidden, step=step, t0=False), args.reps, args.calls)
        leg["drnn_plan"] = summary(ms, B)
        del drnn
        icem = TdICEM(cfg, max_batch=B, rng="device")
        icem.model.load_state_dict(synthetic_state_dict(cfg, 0, enc_norm=True), strict=False)
        icem.std = 0.05
        icem.plan_batch(obs, step=step, t0=True, sync_metrics=False)
        ms = timed_batches(lambda: icem.plan_batch(obs, step=step, t0=False, sync_metrics=False), args.reps, args.calls)
        leg["icem_plan"] = summary(ms, B)
        del icem
        out["envs"][str(B)] = leg
        print(json.dumps({str(B): leg}), flush=True)
    # the CPU figure: the float32 restatement on 16 threads, one env
    import drnn_icem_ref as ref
    import drnn_ref
    torch.set_num_threads(16)
    model = drnn_ref.RefDSSM(sd, cfg)
    st = ref.IcemDrnnState(0.05)
    rs = np.random.RandomState(0)
    obs1 = rs.standard_normal(cfg.obs_shape).astype(np.float32)
    hid1 = rs.uniform(-1, 1, (1, cfg.hidden_dim)).astype(np.float32)
    ts = []
    for k in range(args.cpu_calls + 1):
        nz = ref.draw_noise(cfg, st, step, k == 0, False)
        t = time.perf_counter()
        ref.plan(model, cfg, st, obs1, hid1, nz, step=step, t0=k == 0)
        ts.append(time.perf_counter() - t)
    cpu = statistics.median(ts[1:])   # (the first call, an episode start, is the warm-up)
    out["cpu_restatement_fp32_16_threads"] = {"s_per_plan_median": round(cpu, 4), "s_per_plan_min": round(min(ts[1:]), 4),
                                              "s_per_plan_max": round(max(ts[1:]), 4), "calls": len(ts) - 1,
                                              "plan_steps_per_s": round(1 / cpu, 2)}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
