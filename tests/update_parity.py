"""Forward parity stated on what the kernels compute.  Every drop-in model returns `x + update`, and in the suite's
batches the positions are 25 .. 65 times larger than the update: `scale_rel_err(out) <= 1e-5` therefore bounds the update
to about 5e-4 only, which lets a lost cross term of a split GEMM through (tests/test_update_metric.py shows it on the CPU).

`update_err(got, x, want64)`: per element e = |got - want64| and r = 2^-24 |fl32(want64)|, the result is
max(max(e - r, 0)) / max|want64 - x|.  r is derived, not measured: the kernel forms fl32(x + update32), one rounding of
at most half an ulp of the result, which says nothing about the update and is taken out.  (Half an ulp of a binade's
lower end is 2^-24 of it; the allowance is never larger than the rounding it stands for by more than that factor of two.)

`update_floor(want32, x, want64)` is the same quantity for the project's fp32 CPU restatement of the same inputs, the
reference every bar is taken against.  The bar is `update_err <= FACTOR * update_floor` with FACTOR = 4: the margin
tests/test_gpu_parity.py::test_inputs_at_extreme_magnitudes gives the kernels over the fp32 restatement, and what the
design gives away -- 22 against 24 significand bits per product of the split GEMMs (csrc/common.h) is 2^2.  A floor below
DEGENERATE (all errors of the restatement inside r) carries no information: such a case is given another seed.
"""
import torch

FACTOR = 4.0
DEGENERATE = 2e-8


def update_err(got_out_fp32, x, want_out_fp64):
    got, want = got_out_fp32.detach().cpu().double(), want_out_fp64.detach().cpu().double()
    x = x.detach().cpu().double()
    assert got.shape == want.shape == x.shape, (got.shape, want.shape, x.shape)
    assert torch.isfinite(got).all()
    e = (got - want).abs()
    r = 2.0 ** -24 * want.float().double().abs()
    upd = (want - x).abs().max()
    assert float(upd) > 0.0
    return float((e - r).clamp(min=0.0).max() / upd)


def update_floor(want32_out, x, want_out_fp64):
    return update_err(want32_out, x, want_out_fp64)


def check_update(what, got, want32, x, want64, factor=FACTOR):
    """Prints both figures (pytest -s shows them), then holds `got` to factor x the restatement's floor."""
    err, floor = update_err(got, x, want64), update_floor(want32, x, want64)
    print(f"update-parity {what}: err={err:.3e} floor={floor:.3e} ratio={err / max(floor, 1e-300):.2f}")
    assert floor >= DEGENERATE, (what, "degenerate floor: choose another seed", floor)
    assert err <= factor * floor, (what, err, floor, err / floor)
    return err, floor
