"""CPU: the seeds of the planner's width cases (tests/plan_widths_ref.py) leave no near tie in the oracle's own trace,
so tests/test_gpu_plan_widths.py cannot escape on one (tests/test_zz_parity_budget.py's budget is not touched)."""
import pytest

import plan_widths_ref as P


@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_committed_seeds_have_no_near_tie_in_the_oracle(shape):
    """For every committed seed and both call patterns an env slot can see: at every iteration of every call the gap
    between the num_elites-th and the next-best value exceeds 2 (1e-5 + 1e-4 max |v|)."""
    for seed in P.SEEDS[shape]:
        for pattern in P.PATTERNS:
            r = P.min_gap_ratio(shape, seed, pattern)
            assert r > 1.0, (shape, seed, pattern, r)
