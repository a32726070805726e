"""CPU: the DSSM update's engine without a device (tdmpc_amd/dssm_engine.py, include/tdmpc_drnn_engine.h; DESIGN.md §7
f14): what `dssm_engine.reason` refuses and admits, the CPU model's refusal, the default learner, the gate entry points'
ABI -- version, sizes, refusals -- and the float32 floors tests/test_gpu_drnn_engine_kernels.py derives its bounds from,
recomputed."""
import ctypes as C
import os
import re

import pytest
import torch

import drnn_gate_ref as R
from tdmpc_amd import _lib

E_DIMS = -1   # TDMPC_E_DIMS (include/tdmpc_hip.h)
FAKE = 0x10000   # a non-null address that a refused call never reads
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(n=6, null=None):
    t = (C.c_void_p * n)(*([FAKE] * n))
    if null is not None:
        t[null] = None
    return t


def _fwd(rows, Hd, gi=FAKE, gh=FAKE, h=FAKE, ln=None, hn=FAKE):
    return _lib.lib().tdmpc_drnn_gate_fwd(gi, gh, h, ln or _table(), FAKE, FAKE, FAKE, hn, rows, Hd, None)


def _bwd(rows, Hd, dhn=FAKE, gh=FAKE, h=FAKE, ln=None, dgh=FAKE, dhd=FAKE, part=FAKE):
    return _lib.lib().tdmpc_drnn_gate_bwd(dhn, gh, h, ln or _table(), FAKE, FAKE, FAKE, FAKE, dgh, dhd, part, rows, Hd,
                                          None)


def test_version_matches_the_header_and_the_pinned_versions_stand():
    L = _lib.lib()
    text = open(os.path.join(REPO, "include", "tdmpc_drnn_engine.h")).read()
    v = int(re.search(r"#define TDMPC_DRNN_ENGINE_VERSION (\d+)", text).group(1))
    assert L.tdmpc_drnn_engine_version() == v == _lib.DRNN_ENGINE_VERSION
    rows = int(re.search(r"#define TDMPC_DRNN_GATE_PART_ROWS (\d+)", text).group(1))
    assert rows == _lib.DRNN_GATE_PART_ROWS == R.PART_ROWS
    assert L.tdmpc_drnn_train_version() == 1 == _lib.DRNN_TRAIN_VERSION
    assert L.tdmpc_sim_learner_version() == 1 and L.tdmpc_abi_version() == _lib.ABI_VERSION
    for name in ("tdmpc_drnn_engine_version", "tdmpc_drnn_gate_part_floats", "tdmpc_drnn_gate_fwd",
                 "tdmpc_drnn_gate_bwd"):
        assert name in _lib.EXPORTED


def test_part_floats_is_one_slice_of_six_vectors_per_32_rows():
    L = _lib.lib()
    for Hd in R.HDS:
        for rows, slices in ((2, 1), (32, 1), (33, 2), (130, 5), (2560, 80), (4096, 128)):
            n = C.c_size_t()
            assert L.tdmpc_drnn_gate_part_floats(rows, Hd, C.byref(n)) == 0
            assert n.value == slices * 6 * Hd == R.nparts(rows) * 6 * Hd
    assert L.tdmpc_drnn_gate_part_floats(33, 96, None) == E_DIMS and b"out is null" in L.tdmpc_last_error()


@pytest.mark.parametrize("what,rows,Hd,match", [
    ("one row", 1, 96, b"rows 1"), ("4097 rows", 4097, 96, b"rows 4097"), ("Hd 0", 33, 0, b"hidden_dim 0"),
    ("Hd 48", 33, 48, b"hidden_dim 48"), ("Hd 288", 33, 288, b"hidden_dim 288")])
def test_inadmissible_shapes_are_refused_without_a_device(what, rows, Hd, match):
    L = _lib.lib()
    n = C.c_size_t(7)
    for rc in (L.tdmpc_drnn_gate_part_floats(rows, Hd, C.byref(n)), _fwd(rows, Hd), _bwd(rows, Hd)):
        assert rc == E_DIMS and match in L.tdmpc_last_error(), (what, L.tdmpc_last_error())
    assert n.value == 7


def test_null_pointers_are_refused_by_name_without_a_device():
    L = _lib.lib()
    err = L.tdmpc_last_error
    assert _fwd(33, 96, gi=None) == E_DIMS and b"gi is null" in err()
    assert _fwd(33, 96, hn=None) == E_DIMS and b"hn is null" in err()
    assert _fwd(33, 96, h=None) == E_DIMS and b"h is null but gh is not" in err()
    assert _fwd(33, 96, gh=None) == E_DIMS and b"gh is null but h is not" in err()
    assert _fwd(33, 96, ln=_table(null=3)) == E_DIMS and b"ln[3] is null" in err()
    assert L.tdmpc_drnn_gate_fwd(FAKE, FAKE, FAKE, None, FAKE, FAKE, FAKE, FAKE, 33, 96, None) == E_DIMS and \
        b"ln is null" in err()
    assert _bwd(33, 96, dhn=None) == E_DIMS and b"dhn is null" in err()
    assert _bwd(33, 96, part=None) == E_DIMS and b"part is null" in err()
    assert _bwd(33, 96, gh=None) == E_DIMS and b"gh is null but h is not" in err()
    assert _bwd(33, 96, ln=_table(null=0)) == E_DIMS and b"ln[0] is null" in err()
    # a hidden state makes its two gradients required; a zero one (gh = h = null) does not ask for them
    assert _bwd(33, 96, dgh=None) == E_DIMS and b"dgh is null" in err()
    assert _bwd(33, 96, dhd=None) == E_DIMS and b"dhd is null" in err()
    assert _bwd(33, 96, gh=None, h=None, dgh=None, dhd=None, part=None) == E_DIMS and b"part is null" in err()


def test_fp32_figures_the_gpu_bounds_are_derived_from():
    """Prints, per case, the largest figure (drnn_gate_ref.figure: max |fp32 - f64| / max |f64| per tensor) that
    float32 CPU PyTorch shows against float64, for the forward's regions and for the gradients, with a hidden state and
    with explicit zeros. Measured when this test was written: forward between 8.5e-08 and 2.91e-07 (Hd 96 rows 130,
    gate), gradients between 1.4e-07 and 3.69e-07 (Hd 224 rows 2, ln_reset.weight).
    tests/test_gpu_drnn_engine_kernels.py takes 8 x the largest of each group; this test holds the constants there to
    what it measures (within a factor of two: another PyTorch build or CPU sums in another order) and the yardstick to
    the bounds, and checks that explicit zeros leave the reset gate exactly without gradient."""
    from test_gpu_drnn_engine_kernels import BOUND_BWD, BOUND_FWD, FP32_CPU_BWD, FP32_CPU_FWD
    worst = dict(fwd=0.0, bwd=0.0)
    for zero_hidden in (False, True):
        for case in R.CASES:
            d = R.data(*case)
            want, got = R.gate(d, torch.float64, zero_hidden), R.gate(d, torch.float32, zero_hidden)
            figs = R.figures(got, want)
            fw = {k: v for k, v in figs.items() if k in R.FWD}
            bw = {k: v for k, v in figs.items() if k not in R.FWD}
            kf, kb = max(fw, key=fw.get), max(bw, key=bw.get)
            print(f"{case} zero_hidden {zero_hidden}: forward {fw[kf]:.3e} ({kf}), gradients {bw[kb]:.3e} ({kb})")
            worst["fwd"], worst["bwd"] = max(worst["fwd"], fw[kf]), max(worst["bwd"], bw[kb])
            if zero_hidden:
                Hd = case[0]
                assert not want["dgi"][:, :Hd].any() and not want["ln_reset.weight"].any() and \
                    not want["ln_reset.bias"].any()
                assert (want["dhd"] == d["dhn"].double().numpy() * (1 - want["gate"][:, Hd:2 * Hd])).all()
    print(f"largest: forward {worst['fwd']:.3e}, gradients {worst['bwd']:.3e}")
    assert worst["fwd"] <= BOUND_FWD and worst["bwd"] <= BOUND_BWD, worst
    assert 0.5 * FP32_CPU_FWD <= worst["fwd"] <= 2 * FP32_CPU_FWD, worst
    assert 0.5 * FP32_CPU_BWD <= worst["bwd"] <= 2 * FP32_CPU_BWD, worst


# ---------------------------------------------------------------------------------------------------- the engine's switch
def _cfg(**over):
    import drnn_update_ref as U
    cfg = U.case_cfg("cheetah")
    for k, v in over.items():
        setattr(cfg, k, v)
    return cfg


def test_reason_admits_the_recorded_cases_and_names_each_refused_setting():
    import drnn_update_ref as U
    from tdmpc_amd.drnn_learner import check_learner_cfg
    from tdmpc_amd.dssm_engine import reason
    for name in U.CASES:
        assert reason(U.case_cfg(name)) is None, name
    # everything check_learner_cfg refuses, under the engine learner's name
    for over, word in ((dict(batch_size=1), "batch_size=1"), (dict(batch_size=2048), "rows exceed 4096"),
                       (dict(optim_id="sgd"), "optim_id='sgd'"), (dict(modality="pixels"), "modality='pixels'"),
                       (dict(norm_cell=False), "norm_cell=False"), (dict(plan2expl=True), "plan2expl=True"),
                       (dict(normalize=False), "normalize=False"), (dict(norm_type="bn"), "norm_type='bn'")):
        cfg = _cfg(**over)
        with pytest.raises((ValueError, NotImplementedError)):
            check_learner_cfg(cfg)
        why = reason(cfg)
        assert why and word in why and "DssmLearner" not in why, (over, why)
    # and what the engine's kernels add
    for over, word in ((dict(enc_dim=300), "enc_dim=300"), (dict(weight_decay=0.01), "weight_decay=0.01"),
                       (dict(hidden_dim=48), "hidden_dim=48"), (dict(hidden_dim=288), "hidden_dim=288"),
                       (dict(mlp_dim=256), "mlp_dim=256"), (dict(latent_dim=300), "latent_dim=300")):
        cfg = _cfg(**over)
        check_learner_cfg(cfg)
        why = reason(cfg)
        assert why and why.startswith("DssmEngineLearner: ") and word in why, (over, why)
    for E in (256, 512, 1024):
        assert reason(_cfg(enc_dim=E)) is None
    assert reason(_cfg(horizon=5, batch_size=682)) is None and "4098 rows" in reason(_cfg(horizon=5, batch_size=683))


def test_a_cpu_model_is_refused_by_name_and_the_default_is_the_stock_learner():
    """The learner classes on bare agents (the planner needs a GPU, the learners' refusals do not)."""
    from types import SimpleNamespace

    import drnn_update_ref as U
    from tdmpc_amd.drnn_learner import DssmLearner
    from tdmpc_amd.dssm_engine import DssmEngineLearner
    cfg = U.case_cfg("tiny")
    model, target = U.make_models(cfg, "tiny")
    agent = SimpleNamespace(cfg=cfg, model=model, model_target=target, device=torch.device("cpu"), planner=None)
    with pytest.raises(ValueError, match="DssmEngineLearner: the model is on the CPU"):
        DssmEngineLearner(agent, graph=False)
    with pytest.raises(ValueError, match="DssmEngineLearner: enc_dim=300"):
        DssmEngineLearner(SimpleNamespace(cfg=_cfg(enc_dim=300), model=None, model_target=None, device=None))
    assert type(DssmLearner(agent, graph=False)) is DssmLearner and isinstance(agent.optim, torch.optim.Adam)


def test_the_agents_name_their_learners():
    """`TdIcemDrnn` names `DssmLearner` until the argument or the variable selects the engine when the learner is first
    built; `TdMpcDrnn` has neither and keeps `DssmSimLearner`. Checked on the classes and on instances made without
    their constructors (the planners need a GPU)."""
    import inspect

    from tdmpc_amd import drnn, drnn_icem
    assert (drnn_icem.TdIcemDrnn.LEARNER, drnn_icem.TdIcemDrnn.LEARNER_MODULE) == ("DssmLearner", "drnn_learner")
    assert drnn.TdMpcDrnn.LEARNER == "DssmSimLearner" and drnn.TdMpcDrnn.LEARNER_MODULE == "drnn_learner"
    assert inspect.signature(drnn_icem.TdIcemDrnn.__init__).parameters["engine"].default is False
    assert "engine" not in inspect.signature(drnn.TdMpcDrnn.__init__).parameters
    assert "TDMPC_DSSM_LEARNER_ENGINE" not in inspect.getsource(drnn)
    assert drnn.TdMpcDrnn.learner is drnn.DssmLearning.learner          # (no override: the variable is never read)
    built = []

    class Probe(drnn_icem.TdIcemDrnn):
        def __init__(self, engine):
            self.use_engine, self._learner, self.graph = engine, None, False

    def fake_import(name, package):
        built.append(name)
        return type("M", (), {"DssmLearner": lambda a, graph: "stock", "DssmEngineLearner": lambda a, graph: "engine"})
    import importlib
    real = importlib.import_module
    importlib.import_module = fake_import
    old = os.environ.pop("TDMPC_DSSM_LEARNER_ENGINE", None)
    try:
        assert Probe(False).learner == "stock" and Probe(True).learner == "engine"
        os.environ["TDMPC_DSSM_LEARNER_ENGINE"] = "1"
        assert Probe(False).learner == "engine"
        os.environ["TDMPC_DSSM_LEARNER_ENGINE"] = "0"
        assert Probe(False).learner == "stock"
    finally:
        importlib.import_module = real
        os.environ.pop("TDMPC_DSSM_LEARNER_ENGINE", None)
        if old is not None:
            os.environ["TDMPC_DSSM_LEARNER_ENGINE"] = old
    assert built == [".drnn_learner", ".dssm_engine", ".dssm_engine", ".drnn_learner"]
