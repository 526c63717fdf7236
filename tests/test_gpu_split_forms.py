"""The range test and the fp16 split every split GEMM shares (csrc/common.h: split_scale_of / absmax4, split8 / split_pair),
bit for bit against numpy, run beside MFMAs.

aether_debug_split runs one workgroup of 12 waves, three per SIMD; wave w takes the tiles w and w + 12 of the 24 tiles of
tests/split_forms_cases.py -- random normal at 2^-30 .. 2^20, +-0, fp32 subnormals, values whose lo piece is an fp16
subnormal, fp16 rounding ties, |x| around 65,504 and 2^15, tile maxima just below and at 2^-6, an all-zero tile, +-inf and
a NaN in one lane, the special values in lanes 48-63 as well as in lanes 0-15 -- and writes the pieces, the SplitScale
decision and the product of gemm_split<4, 2> with a fixed weight image.

  hi = float16(s x),  lo = float16(float32(s x) - float32(hi)):  equal bit for bit (a NaN for a NaN);
  on, s: equal to the restated split_scale_of (a NaN lane is dropped from the maximum, an inf lane scales by 2^-40);
  y: equal bit for bit to tests/golden/split_forms_y.npy, which a build with -DAETHER_SPLIT_PARENT_FORMS (the forms of
     before: cvt / cvt / sub / cvt and the fmaxf tree) wrote from tests/golden/split_forms_x.npy.

The CPU test holds the restatement to itself on the NaN and inf tiles first."""
import os

import numpy as np
import pytest
import torch

import split_forms_cases as S
from conftest import GOLDEN


def _x():
    x = S.make_inputs()
    stored = np.load(os.path.join(GOLDEN, "split_forms_x.npy"))
    assert S.same_bits_or_both_nan(x, stored).all()              # the golden product belongs to these inputs
    return stored


def test_reference_is_self_consistent_on_nan_and_inf():
    x = S.make_inputs()
    assert x.shape == (S.N_TILES, 16, 64)
    hi, lo, on, scale = S.reference(x)
    # a NaN lane decides nothing: the decision is that of the tile without it
    for t in (22, 23):
        nan = np.isnan(x[t])
        assert nan.sum() == 1
        assert S.scale_decision(np.where(nan, np.float32(0), x[t])) == (bool(on[t]), scale[t])
        h, l = hi[t].view(np.float16), lo[t].view(np.float16)
        assert np.isnan(h[nan]).all() and np.isnan(l[nan]).all() and np.isfinite(h[~nan]).all() and np.isfinite(l[~nan]).all()
    assert (on[22], scale[22]) == (0, 1.0) and on[23] == 1
    # an inf lane is at or above 2^15: exponent 255 -> the shift clamps at -40; inf stays inf, its lo is inf - inf
    for t in (20, 21):
        inf = np.isinf(x[t])
        assert inf.sum() == 2 and on[t] == 1 and scale[t] == np.float32(2.0 ** -40)
        assert np.isinf(hi[t].view(np.float16)[inf]).all() and np.isnan(lo[t].view(np.float16)[inf]).all()
        assert (hi[t][~inf] & 0x7FFF == 0).all()                          # 2^-40 x is below half the smallest fp16 subnormal
    # the thresholds
    assert [int(v) for v in on[[11, 15, 16, 17, 18, 19]]] == [0, 0, 1, 1, 1, 0]
    assert on[12] == 1 and scale[12] == np.float32(2.0 ** 40)
    # finite tiles: the scaled maximum lies in [2^13, 2^14) and hi + lo restores s x to 2^-22 of it, or to half an fp16
    # subnormal step
    for t in range(S.N_TILES):
        if t in (11, 12, 20, 21, 22, 23):
            continue
        xs = x[t].astype(np.float64) * float(scale[t])
        m = np.abs(xs).max()
        if on[t] and scale[t] == np.float32(2.0 ** 40):           # (the shift is clamped: tile 0, maximum about 2^-28)
            assert 2.0 ** -6 <= m < 2.0 ** 14, (t, m)
        else:
            assert (2.0 ** 13 <= m < 2.0 ** 14) if on[t] else (2.0 ** -6 <= m < 2.0 ** 15), (t, m)
        rest = xs - hi[t].view(np.float16).astype(np.float64) - lo[t].view(np.float16).astype(np.float64)
        assert np.abs(rest).max() <= max(2.0 ** -22 * m, 2.0 ** -25), (t, np.abs(rest).max() / m)   # (2^-25: lo a subnormal)
    # special values sit in lanes 48-63 (features f % 16 >= 12) and in lanes 0-15 (f % 16 < 4)
    for t, pick in ((13, lambda a: a == np.float32(1 + 2.0 ** -11)), (17, lambda a: np.abs(a) == 65520), (20, np.isinf)):
        f = np.nonzero(pick(np.abs(x[t])))[1] % 16
        assert (f >= 12).any() and (f < 4).any(), (t, f)


@pytest.fixture(scope="module")
def run():
    from aether_amd import _lib
    lib = _lib.load()
    x = _x()
    dev = torch.device("cuda")
    xd = torch.from_numpy(x).to(dev)
    n = x.shape[0]
    hi = torch.zeros(x.shape, dtype=torch.int16, device=dev)
    lo = torch.zeros(x.shape, dtype=torch.int16, device=dev)
    on = torch.full((n,), -1, dtype=torch.int32, device=dev)
    scale = torch.zeros(n, dtype=torch.float32, device=dev)
    y = torch.zeros(x.shape, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    _lib.check(lib.aether_debug_split(xd.data_ptr(), n, hi.data_ptr(), lo.data_ptr(), on.data_ptr(), scale.data_ptr(),
                                      y.data_ptr()), "aether_debug_split")
    torch.cuda.synchronize()
    return dict(x=x, hi=hi.cpu().numpy().view(np.uint16), lo=lo.cpu().numpy().view(np.uint16), on=on.cpu().numpy(),
                scale=scale.cpu().numpy(), y=y.cpu().numpy(), ref=S.reference(x))


def _report(name, ok, x, got, want):
    bad = np.argwhere(~ok)
    print(f"{name}: {len(bad)} of {ok.size} differ")
    for t, i, f in bad[:8]:
        print(f"   tile {t} row {i} feature {f} (lane {16 * ((f % 16) // 4) + i}): x = {x[t, i, f]!r} "
              f"got {int(got[t, i, f]):#x} want {int(want[t, i, f]):#x}")
    return len(bad)


@pytest.mark.gpu
def test_decision_and_scale(run):
    _hi, _lo, on, scale = run["ref"]
    print("on   ", run["on"].tolist(), "\nwant ", on.tolist(), "\nscale", run["scale"].tolist())
    assert np.array_equal(run["on"], on)
    assert np.array_equal(run["scale"], scale)


@pytest.mark.gpu
def test_pieces_bit_for_bit(run):
    hi, lo, _on, _scale = run["ref"]
    bad_hi = _report("hi", S.same_bits_or_both_nan(run["hi"], hi), run["x"], run["hi"], hi)
    bad_lo = _report("lo", S.same_bits_or_both_nan(run["lo"], lo), run["x"], run["lo"], lo)
    assert bad_hi == 0 and bad_lo == 0


@pytest.mark.gpu
def test_product_equals_the_parent_forms(run):
    want = np.load(os.path.join(GOLDEN, "split_forms_y.npy"))
    got = run["y"]
    ok = S.same_bits_or_both_nan(got, want)
    bad = _report("y", ok, run["x"], got.view(np.uint32), want.view(np.uint32))
    assert bad == 0
    # (the golden is a product, not a table of NaNs: only the inf / NaN rows are non-finite)
    finite_rows = np.isfinite(run["x"]).all(axis=2)
    assert np.isfinite(want[finite_rows]).all() and finite_rows.sum() == S.N_TILES * 16 - 5
