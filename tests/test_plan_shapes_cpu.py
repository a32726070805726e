"""CPU: the seeds of the planner's shape cases (tests/plan_shapes_ref.py) leave no near tie in the oracle's own trace,
so tests/test_gpu_plan_shapes.py cannot escape on one (tests/test_zz_parity_budget.py's budget is not touched); and
the padded widths its docstring and KERNELS table reason from are the ones the table of shapes gives."""
import pytest

import plan_shapes_ref as S


@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_committed_seeds_have_no_near_tie_in_the_oracle(shape):
    """For every committed seed and both call patterns an env slot can see: at every iteration of every call the gap
    between the num_elites-th and the next-best value exceeds 2 (1e-5 + 1e-4 max |v|)."""
    assert len(S.SEEDS[shape]) == max(S.BATCHES[shape]) == (32 if shape in "bd" else 3)
    for seed in S.SEEDS[shape]:
        for pattern in S.PATTERNS:
            r = S.min_gap_ratio(shape, seed, pattern)
            assert r > 1.0, (shape, seed, pattern, r)


def test_derived_widths():
    """(Lr, Kx) of every row, (Ap, Ar) where the row is about them: what the kernels' predicates switch on."""
    got = {s: (S.derived(s)["Lr"], S.derived(s)["Kx"]) for s in S.SHAPES}
    assert got == {"a": (32, 16), "b": (96, 104), "c": (128, 192), "d": (160, 160), "e": (224, 240), "f": (256, 296),
                   "g": (320, 328), "h": (448, 448), "i": (512, 536), "j": (64, 128), "k": (544, 544), "l": (1024, 1024)}
    assert (S.derived("c")["Ap"], S.derived("c")["Ar"]) == (64, 64)
    assert (S.derived("j")["Ap"], S.derived("j")["Ar"]) == (72, 96)
    assert S.derived("i")["Lp"] == 512 and S.derived("d")["Lp"] == 136
    for s in S.SHAPES:
        cfg = S.shape_cfg(s)
        assert (cfg.action_dim, cfg.latent_dim, cfg.enc_dim, cfg.mlp_dim) == S.SHAPES[s][1:] + (512,)
