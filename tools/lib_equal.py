"""Do two builds of the library, or two trees of the Python layer, compute the same? A fixed, seeded list of small eager calls through every planning
entry point (TOLD on every kernel path, every instance family of the wide kernels, iCEM, the DSSM planners), once
per library in a fresh process; every output is compared bitwise. Needs a GPU.
    python -m tdmpc_amd.build --variant parent        # in a checkout of the other commit; copy the .so next to ours
    python tools/lib_equal.py tdmpc_amd/libtdmpc_hip_parent.so tdmpc_amd/libtdmpc_hip.so [OUT_DIR]
Or two source trees on one library: in each tree, `python tools/lib_equal.py --child OUT.npz` (with TDMPC_LIB_PATH set
to the one library), then
    python tools/lib_equal.py --compare A.npz B.npz [ARRAY_COUNT]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
TOLD_PATHS = ["layered", "chain16", "chain32", "split", "chain_x6", "split_x6", "chain", "persist", "wide"]
SMALL = dict(num_samples=64, num_elites=16, iterations=3, horizon=5)
WIDE = dict(num_samples=128, num_elites=16, iterations=3, horizon=5)
STEP, H = 10**6, 5   # past every schedule: the full horizon, the final mixture


def child(out):
    import torch
    from tdmpc_amd import TDMPC, TdICEM, TdIcemDrnn, TdMpcDrnn, make_cfg
    from tdmpc_amd.dssm import synthetic_dssm_state_dict
    from tdmpc_amd.told import synthetic_state_dict
    res = {}

    def put(name, *vals):   # tensors, and lists of tensors, by position
        for i, v in enumerate(vals):
            for j, t in enumerate(v if isinstance(v, (list, tuple)) else [v]):
                if torch.is_tensor(t):
                    res[f"{name}/{i}.{j}"] = t.detach().cpu().numpy()
    def rand(seed, *shapes, uniform=False):
        g = torch.Generator().manual_seed(seed)
        return [torch.rand(*s, generator=g) * 2 - 1 if uniform else torch.randn(*s, generator=g) for s in shapes]
    def made(agent, sd):
        agent.model.load_state_dict(sd)
        agent.std = 0.05
        return agent

    for task in ("humanoid", "cheetah"):
        cfg = make_cfg(task, **SMALL)
        sd, (obs,) = synthetic_state_dict(cfg, 7), rand(1, (3, cfg.obs_shape[0]))
        for path in TOLD_PATHS:
            agent = made(TDMPC(cfg, max_batch=3, rng="fused", graph=False, path=path), sd)
            pl, tag = agent.planner, f"told/{task}/{path}"
            pl.pack(agent.model)
            N, P, T, A, L = pl.N, pl.P, pl.T, pl.A, cfg.latent_dim
            z0, eps, eps_pi, eps_cem = rand(2, (2, L), (2, T, A), (2, H, P, A), (2, H, N, A))
            (act,) = rand(3, (2, H, T, A), uniform=True)
            put(f"{tag}/estimate_value", *pl.estimate_value(z0, act, eps, H))
            pi = pl.pi_rollout(z0, eps_pi, H) if P > 0 else None
            mean, std = torch.zeros(2, H, A, device=pl.device), torch.full((2, H, A), 2.0, device=pl.device)
            put(f"{tag}/cem_iter", pi, *pl.cem_iter(z0, pi, eps_cem, eps, mean, std, H), mean, std)
            for B, t0 in ((1, True), (1, False), (3, True)):   # cold, warm, a batch
                torch.manual_seed(10 + B)
                tr = {}
                a, _ = agent._plan_envs(obs[:B], False, STEP, [t0] * B, trace=tr)
                put(f"{tag}/plan{B}{int(t0)}", a, pl.metrics[:B], pl.prev_mean_view(H, B), *tr.values())
    # the wide kernels, every instance family: N = 128 and P = 64 at STEP (N + P = T, multiples of 16; N a multiple of
    # 128: the t = 0 per-env-bias instances), path="wide" so that two envs reach them; max_batch 32 so that the pack
    # builds helper.q's statistics block. The profiler's kernel name proves that they ran.
    import ctypes as C
    from tdmpc_amd import _lib
    L = _lib.lib()

    def kernel_of(agent, obs, prof_cfg):   # as tests/test_gpu_configs.py::_kernel_of: 4 the step launches, 6 helper.q
        _lib.check(L.tdmpc_profile_begin(prof_cfg, -1, 0, 0, 256), "profile_begin")
        agent._plan_envs(obs, False, STEP, [False] * len(obs))
        n, ms, fl = C.c_int32(), C.c_double(), C.c_double()
        _lib.check(L.tdmpc_profile_end(C.byref(n), C.byref(ms), C.byref(fl)), "profile_end")
        return L.tdmpc_profile_kernel().decode() if n.value > 0 else ""
    for name, task, ov in (("humanoid", "humanoid", {}), ("dog", "dog", {}), ("cheetah", "cheetah", {}),
                           ("quadruped", "quadruped", {}), ("humanoid-l512", "humanoid", dict(latent_dim=512))):
        cfg = make_cfg(task, **dict(WIDE, **ov))
        sd, (obs,) = synthetic_state_dict(cfg, 7), rand(9, (2, cfg.obs_shape[0]))
        agent = made(TDMPC(cfg, max_batch=32, rng="fused", graph=False, path="wide"), sd)
        pl = agent.planner
        for B, t0 in ((1, True), (1, False), (2, True)):   # cold, warm, a batch
            torch.manual_seed(50 + B)
            tr = {}
            a, _ = agent._plan_envs(obs[:B], False, STEP, [t0] * B, trace=tr)
            put(f"wide/{name}/plan{B}{int(t0)}", a, pl.metrics[:B], pl.prev_mean_view(H, B), *tr.values())
        step_k, q_k = kernel_of(agent, obs, 4), kernel_of(agent, obs, 6)
        assert step_k.startswith("wide_step_kernel<17, 32" if ov else "wide_step_kernel"), (name, step_k)
        assert ov or q_k.startswith("wide_heads_kernel"), (name, q_k)   # (latent 512: no wide heads instance)
    cfg = make_cfg("humanoid", **dict(SMALL, num_elites=8))
    sd, (obs,) = synthetic_state_dict(cfg, 31, enc_norm=True), rand(4, (3, cfg.obs_shape[0]))
    for path in ("auto", "layered", "split", "chain_x6"):
        agent = made(TdICEM(cfg, max_batch=3, rng="device", path=path), sd)
        pl = agent.planner
        for k, (B, t0) in enumerate(((1, True), (1, False), (3, False))):   # cold, warm with elite reuse, a batch
            torch.manual_seed(20 + k)
            tr = {}
            a, _ = agent._plan_envs(obs[:B], False, STEP, t0, None, tr)
            put(f"icem/{path}/{k}", a, pl.metrics[:B], pl.elites, pl.prev_mean_flat, *tr.values())
    for task in ("humanoid", "cheetah"):
        cfg = make_cfg(task, hidden_dim=128, norm_cell=True, plan2expl=False, warmup_len=0,
                       regularization_schedule="0.5", **SMALL)
        sd = synthetic_dssm_state_dict(cfg, 7)
        agent = made(TdMpcDrnn(cfg, max_batch=3, rng="fused", graph=False), sd)
        pl, tag = agent.planner, f"dssm/{task}"
        pl.pack(agent.model)
        T, P, A, L = pl.T, pl.P, pl.A, cfg.latent_dim
        obs, z0, eps, eps_pi = rand(5, (3, cfg.obs_shape[0]), (3, L), (3, T, A), (3, H, P, A))
        h0, act, a70 = rand(6, (3, 128), (3, H, T, A), (70, A), uniform=True)
        put(f"{tag}/next", *pl.next(rand(7, (70, L))[0], a70, rand(8, (70, 128), uniform=True)[0]))
        for B in (1, 3):
            put(f"{tag}/estimate_value{B}", *pl.estimate_value(z0[:B], h0[:B], act[:B], eps[:B], H))
            put(f"{tag}/pi_rollout{B}", pl.pi_rollout(z0[:B], h0[:B], eps_pi[:B], H))
        for B, t0 in ((1, True), (1, False), (3, True)):   # cold, warm, a batch
            torch.manual_seed(30 + B)
            tr = {}
            a, _ = agent.plan_batch(obs[:B], h0[:B], step=STEP, t0=t0, trace=tr)
            put(f"{tag}/plan{B}{int(t0)}", a, pl.z_in[:B], pl.prev_mean_view(H, B), *tr.values())
        icem = made(TdIcemDrnn(cfg, max_batch=3, rng="device", graph=False), sd)
        for k, (B, t0) in enumerate(((3, True), (3, False), (1, False))):   # cold, warm with elite reuse, one env
            torch.manual_seed(40 + k)
            tr = {}
            a, h, _ = icem.plan_batch(obs[:B], h0[:B], step=STEP, t0=t0, trace=tr)
            put(f"{tag}/icem{k}", a, h, icem.planner.elites, icem.planner.prev_mean_flat, *tr.values())
    torch.cuda.synchronize()
    np.savez(out, **res)


def compare(fa, fb, count=None):
    """Exit status 0 when the two dumps hold the same arrays (and `count` of them, when given), bitwise."""
    a, b = np.load(fa), np.load(fb)
    bad = sorted(set(a.files) ^ set(b.files)) + [   # bitwise: equal shapes and bytes (so NaN equals the same NaN)
        k for k in a.files if k in b.files and (a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes())]
    if count is not None and len(a.files) != count:
        bad.append(f"{len(a.files)} arrays, not {count}")
    print(f"{len(a.files)} arrays, differing: {bad}" if bad else f"{len(a.files)} arrays equal")
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        sys.exit(child(sys.argv[2]))
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else None))
    out = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="lib_equal_")
    os.makedirs(out, exist_ok=True)
    files = [os.path.join(out, f"lib{i}.npz") for i in (0, 1)]
    for lib, f in zip(sys.argv[1:3], files):   # one fresh process per library; the first failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", f],
                            env=dict(os.environ, TDMPC_LIB_PATH=os.path.abspath(lib)), cwd=REPO).returncode
        if rc:
            sys.exit(f"{lib}: exit status {rc}")
    sys.exit(compare(*files))
