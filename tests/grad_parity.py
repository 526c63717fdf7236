"""Gradient parity stated on what fp32 arithmetic gives, per tensor: the sibling of tests/update_parity.py.

The structural gradient tests hold `scale_rel_err(g, g64) <= GTOL = 5e-5`.  The arithmetic the backward kernels are meant
to do -- three-term products of fp16 pieces with fp32 results (csrc/common.h) -- sits at or under 1e-6 on every tensor,
so that bar lets a lost term of a weight-gradient product through (tests/test_grad_metric.py shows it on the CPU).

`grad_floors(g32, g64)`: per tensor k, floor_k = scale_rel_err of the project's fp32 CPU restatement's gradient against
the fp64 one on the same inputs, and the clamp Q, the upper quartile of those floors.  Two things make one evaluation's
floor a lucky draw, and both are handled on the reference side alone:
  * a tensor's floor is a maximum over few elements (a bias has 1 .. 64): over the cases of tests/grad_cases.py the
    smallest floor of a case is 5e-8 .. 1.3e-7 while the upper quartile is 2.3e-7 .. 1.2e-6 (steps), and the correct three-term
    arithmetic sits at up to 9 of the small floors.  Hence Q, a statement about fp32 on the whole case.
  * the gradients are sums over edges, and fp32 gives a different error for every order of the sum: with the edge list
    permuted (the same graph, the same exact gradient) the fp32 oracle's floor of one tensor moves by a factor 1.4 - 1.8
    (median over the tensors of a case) and by 3 - 8 on the ill-conditioned ones -- the field net's last bias at B2N5
    4e-7 .. 1.6e-6, the attention gate's first bias of DynamicFieldAether 2.6e-7 .. 2.1e-6 -- and the kernels sum in
    yet another fixed order.  `g32` is therefore the restatement's gradients under several orders of the edge list
    (tests/grad_cases.py: ORDERS = 8, the given one first) and floor_k the largest of them; a single dict is accepted too.

`check_grads(what, got, g32, g64)`: err_k = scale_rel_err(got_k, g64_k) <= FACTOR x max(floor_k, Q) for every tensor,
with update_parity's FACTOR = 4 for the same reason, 22 against 24 significand bits per product.  A case whose Q is below
DEGENERATE = 1e-7 carries no information and gets another seed: the smallest Q measured over all cases is 2.3e-7, the
smallest floors of single tensors 5e-8 .. 1.4e-7, and one rounding of a gradient to fp32 alone is up to 2^-24 = 6e-8 of
its maximum.

A tensor whose fp64 gradient is zero (at most ZERO = 1e-9 in magnitude: the softmax gate's last bias, a layer that does
not reach the output) has no scale: it is held to |got| <= ZERO, the structural tests' own rule, and takes no part in Q.
A tensor that has no gradient on the reference side (None) must have none on the other."""
import torch

from conftest import scale_rel_err
from update_parity import FACTOR

DEGENERATE = 1e-7
ZERO = 1e-9


def _is_zero(g):
    return float(g.detach().abs().max()) <= ZERO if g.numel() else True


def grad_floors(g32, g64):
    """({tensor: floor}, Q) from the two CPU references alone; `g32`: one dict, or one per order of evaluation."""
    runs = list(g32) if isinstance(g32, (list, tuple)) else [g32]
    floors = {k: max(scale_rel_err(r[k].detach(), g.detach()) for r in runs)
              for k, g in g64.items() if g is not None and not _is_zero(g)}
    assert floors, "no tensor with a gradient"
    q = float(torch.quantile(torch.tensor(list(floors.values()), dtype=torch.float64), 0.75))
    return floors, q


def grad_ratios(got, g32, g64, factor=FACTOR):
    """{tensor: (err, floor, err / bar)} for the tensors that have a scale."""
    floors, q = grad_floors(g32, g64)
    out = {}
    for k, floor in floors.items():
        err = scale_rel_err(got[k].detach().cpu(), g64[k].detach())
        out[k] = (err, floor, err / (factor * max(floor, q)))
    return out, q


def worst_ratio(got, g32, g64, factor=FACTOR):
    ratios, _ = grad_ratios(got, g32, g64, factor)
    return max(r[2] for r in ratios.values())


def check_grads(what, got, g32, g64, factor=FACTOR):
    """Prints err, floor and err / bar per tensor (pytest -s shows them), then holds every tensor of `got` to
    factor x max(its floor, Q).  Returns the largest err / bar."""
    assert set(g64) <= set(got), (what, sorted(set(g64) - set(got)))
    for k, want in g64.items():
        if want is None:
            assert got[k] is None, (what, k, "a gradient where the reference has none")
            continue
        assert got[k] is not None, (what, k, "no gradient")
        assert tuple(got[k].shape) == tuple(want.shape), (what, k, got[k].shape, want.shape)
        assert torch.isfinite(got[k]).all(), (what, k, "not finite")
    ratios, q = grad_ratios(got, g32, g64, factor)
    print(f"grad-parity {what}: Q={q:.2e} over {len(ratios)} tensors")
    for k, (err, floor, ratio) in ratios.items():
        print(f"grad-parity {what}: {k}: err={err:.2e} floor={floor:.2e} err/bar={ratio:.2f}")
    assert q >= DEGENERATE, (what, "degenerate Q: choose another seed", q)
    for k, want in g64.items():
        if want is not None and k not in ratios:
            m = float(got[k].detach().abs().max())
            print(f"grad-parity {what}: {k}: zero gradient, |got|={m:.1e}")
            assert m <= ZERO, (what, k, m)
    worst = max(ratios, key=lambda k: ratios[k][2])
    print(f"grad-parity {what}: worst err/bar={ratios[worst][2]:.2f} at {worst}")
    bad = {k: r for k, r in ratios.items() if r[2] > 1.0}
    assert not bad, (what, bad)
    return ratios[worst][2]
