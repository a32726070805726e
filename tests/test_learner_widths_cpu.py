"""CPU: where the GPU bounds of tests/test_gpu_lg_rows.py and tests/test_gpu_learner_widths.py come from.

The yardstick of those tests is float64; the noise floor of a comparison is the figure float32 torch on the CPU shows
against the same float64 result on the same inputs, and the bound is 8 x that floor, never below 1e-6 (DESIGN.md §7
f7). This file recomputes every floor, requires the constants committed beside the GPU cases to lie within 2 x of
what it recomputes, and holds the float32 run itself to the bounds. No GPU output enters any of it."""
import pytest
import torch

import lg_rows_ref as R
import learner_widths_ref as W
import test_gpu_learner_widths as TW
import test_gpu_lg_rows as TR


def _within_2x(committed, measured, what):
    print(f"{what}: committed {committed:.3g} measured {measured:.3g}")
    if max(committed, measured) * R.FACTOR <= R.MIN_BOUND:
        return      # both below the 1e-6 minimum: the bound is the minimum either way
    assert measured / 2 <= committed <= measured * 2, (what, committed, measured)
    assert measured <= R.bound(committed), (what, measured)


def _small_kernel_floors():
    """The row kernels' classes over every case of test_gpu_lg_rows.py, the random finalize case, pi_loss and ELU."""
    for k, v in R.rows_fp32_floors().items():
        _within_2x(TR.ROWS_FLOOR[k], v, k)
    combos = [(4, 5000), (31, 2049), (32, 2047), (65, 5000), (256, 2048), (37, 63)]
    ts, _, slen, _ = R.finalize_layout(combos)
    src = torch.randn(slen, generator=torch.Generator().manual_seed(13))
    (g64, sq64), (g32, sq32) = R.finalize_ref(ts, src), R.finalize_ref(ts, src, torch.float32)
    _within_2x(TR.FIN_FLOOR["g"], max(R.fig(a, b) for a, b in zip(g32, g64)), "finalize g")
    _within_2x(TR.FIN_FLOOR["normp"], float(((sq32.double() - sq64).abs() / sq64).max()), "finalize normp")
    f = 0.0
    for nt in (1, 6):
        for bsz in (1, 255, 256, 257, 600):
            q1, q2, rho = R.pi_q(nt, bsz, 100 * nt + bsz)
            ref = R.pi_loss_ref(q1, q2, rho, nt, bsz, torch.float64)
            scale = float((rho.double() * torch.minimum(q1, q2).double().abs().view(nt, bsz).mean(1)).sum())
            f = max(f, abs(float(R.pi_loss_ref(q1, q2, rho, nt, bsz, torch.float32)) - float(ref)) / scale)
    _within_2x(TR.PI_LOSS_FLOOR, f, "pi_loss")
    f = 0.0
    for n in (4, 1028, 4 * 2048 * 256 + 4):
        x, _ = R.act_inputs(n, n)
        f = max(f, R.elu_fig(torch.nn.functional.elu(x), torch.nn.functional.elu(x.double())))
    _within_2x(TR.ELU_FLOOR, f, "elu")


def test_fp32_floors_the_gpu_bounds_are_derived_from():
    """The small kernels' floors, then whole updates: float32 RefLearner against float64 RefLearner on the cases of
    test_gpu_learner_widths.py, over 1, 2, 4 and 8 CPU threads (one thread count is one draw of the summation-order
    noise), per class and case group."""
    _small_kernel_floors()
    floors, shares = W.measure_floors(threads=(1, 2, 4, 8))
    for group, fl in floors.items():
        for cls, v in fl.items():
            _within_2x(TW.FLOOR[group][cls], v, f"{group} {cls}")
    for group, s in shares.items():
        print(f"{group}: share of parameters inside the tight bound {s:.5f}")
        assert s >= TW.SHARE[group], (group, s)
