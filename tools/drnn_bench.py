"""Throughput of the recurrent-latent (DSSM) planner on one MI355X: plan-steps/s, the step kernel's time and its share
of the x6 roof, and the float32 CPU restatement as the CPU figure.

    python tools/drnn_bench.py [--out profiles/r07/drnn_bench.json] [--envs 1,32] [--reps 7] [--calls 20]

Shape: humanoid (L 100, A 21, Hd 128), N = 512, H = 5, 6 iterations, mixture 0.5 (P = 256), rng "fused" (one normal_
per call), graph replay. Per batch size: `reps` timed batches of `calls` plan_batch calls between HIP events after a
warm-up; the median is the figure, min / max the spread. drnn_step_kernel is timed per launch by the library's
HIP-event recorder (tdmpc_drnn_profile_begin, eager launches), over the launches of B * N rows (the sampled rows'
rollout: 5 steps x 5 iterations per plan); its rate is the algorithmic FLOPs (2 * rows * MACs per row at the real
widths) over that time, against the x6 roof 157.3 * 16 / 6 = 419.5 TFLOP/s of fp32 products, as bench.py's roofline.
The TOLD planner at the same shape and path selection ("auto") is timed beside it. The CPU figure is the median of
`--cpu-calls` warm restatement plans after one warm-up call, with min / max. No GPU: it fails.
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
from tdmpc_amd.config import make_cfg  # noqa: E402

X6_PEAK_TFLOPS = round(157.3 * 16 / 6, 1)


def bench_cfg():
    return make_cfg("humanoid", num_samples=512, num_elites=64, iterations=6, horizon=5, hidden_dim=128,
                    norm_cell=True, plan2expl=False, warmup_len=0, regularization_schedule="0.5")


def timed_batches(fn, reps, calls, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def summary(ms, B):
    med = statistics.median(ms)
    return {"ms_per_call_median": round(med, 4), "ms_per_call_min": round(min(ms), 4),
            "ms_per_call_max": round(max(ms), 4), "spread_frac": round((max(ms) - min(ms)) / med, 4),
            "plan_steps_per_s": round(B / med * 1e3, 1), "batches": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--envs", default="1,32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--cpu-calls", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("drnn_bench needs a GPU: nothing is measured without one")
    from tdmpc_amd.drnn import TdMpcDrnn
    from tdmpc_amd.dssm import synthetic_dssm_state_dict
    from tdmpc_amd.tdmpc import TDMPC
    from tdmpc_amd.told import synthetic_state_dict
    cfg = bench_cfg()
    L = _lib.lib()
    sd = synthetic_dssm_state_dict(cfg, 0)
    out = {"shape": "humanoid L100 A21 Hd128 M512, N=512 P=256 H=5 I=6", "x6_peak_tflops": X6_PEAK_TFLOPS,
           "device": torch.cuda.get_device_name(0), "envs": {}}
    step = 10**6
    for B in [int(x) for x in args.envs.split(",") if x]:
        rs = np.random.RandomState(B)
        obs = rs.standard_normal((B, cfg.obs_shape[0])).astype(np.float32)
        hidden = rs.uniform(-1, 1, (B, cfg.hidden_dim)).astype(np.float32)
        agent = TdMpcDrnn(cfg, max_batch=B, rng="fused")
        agent.model.load_state_dict(sd)
        agent.std = 0.05
        agent.plan_batch(obs, hidden, step=step, t0=True)
        ms = timed_batches(lambda: agent.plan_batch(obs, hidden, step=step, t0=False), args.reps, args.calls)
        leg = {"drnn_plan": summary(ms, B)}
        # the step kernel per launch (eager launches between HIP events), the sampled rows' rollout launches
        agent.graph = False
        agent.plan_batch(obs, hidden, step=step, t0=False)
        torch.cuda.synchronize()
        rows = B * cfg.num_samples
        _lib.check(L.tdmpc_drnn_profile_begin(rows, 4096), "profile_begin")
        for _ in range(8):
            agent.plan_batch(obs, hidden, step=step, t0=False)
        n, tms, fl = C.c_int32(), C.c_double(), C.c_double()
        _lib.check(L.tdmpc_drnn_profile_end(C.byref(n), C.byref(tms), C.byref(fl)), "profile_end")
        if n.value:
            tf = fl.value / tms.value / 1e9
            leg["drnn_step_kernel"] = {"rows": rows, "launches": n.value,
                                       "us_per_launch": round(tms.value / n.value * 1e3, 2),
                                       "tflops_algorithmic": round(tf, 2),
                                       "frac_of_x6_roof": round(tf / X6_PEAK_TFLOPS, 4),
                                       "flops_per_row": fl.value / n.value / rows}
        del agent
        # the TOLD planner at the same shape (its own path selection)
        told = TDMPC(cfg, max_batch=B, rng="fused")
        told.model.load_state_dict(synthetic_state_dict(cfg, 0))
        told.std = 0.05
        told.plan_batch(obs, step=step, t0=True)
        ms = timed_batches(lambda: told.plan_batch(obs, step=step, t0=False), args.reps, args.calls)
        leg["told_plan_same_shape"] = summary(ms, B)
        del told
        out["envs"][str(B)] = leg
        print(json.dumps({str(B): leg}), flush=True)
    # the CPU figure: the float32 restatement on 16 threads, one env
    import drnn_ref
    torch.set_num_threads(16)
    ref = drnn_ref.RefDSSM(sd, cfg)
    st = drnn_ref.DrnnState(0.05, 0)
    rs = np.random.RandomState(0)
    obs1 = rs.standard_normal(cfg.obs_shape).astype(np.float32)
    hid1 = rs.uniform(-1, 1, (1, cfg.hidden_dim)).astype(np.float32)
    ts = []
    for k in range(args.cpu_calls + 1):
        nz = drnn_ref.draw_drnn_noise(cfg, st, step, k == 0)
        t = time.perf_counter()
        drnn_ref.plan(ref, cfg, st, obs1, hid1, nz, step=step, t0=k == 0)
        ts.append(time.perf_counter() - t)
    cpu = statistics.median(ts[1:])   # (the first call, an episode start, is the warm-up)
    out["cpu_restatement_fp32_16_threads"] = {"s_per_plan_median": round(cpu, 4), "s_per_plan_min": round(min(ts[1:]), 4),
                                              "s_per_plan_max": round(max(ts[1:]), 4), "calls": len(ts) - 1,
                                              "spread_frac": round((max(ts[1:]) - min(ts[1:])) / cpu, 4),
                                              "plan_steps_per_s": round(1 / cpu, 2)}
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
