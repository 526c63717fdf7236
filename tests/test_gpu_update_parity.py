"""Forward parity on the update.  Every drop-in returns `x + update`, and the positions of the suite's batches are 25 .. 65
times larger than the update, so the forward tests' `scale_rel_err(out) <= 1e-5` holds what the kernels compute to
about 5e-4 only.  Here the error of `out` beyond the one rounding of the sum is divided by max|update|
(tests/update_parity.py) and held to 4 x the same figure of the project's fp32 CPU restatement on the same inputs: one
lost cross term of one split GEMM sits 12 .. 690 floors up (tests/test_update_metric.py, on the CPU).

Cases, seeds and restatements: tests/update_cases.py and tests/update_s2s_cases.py; the fp64 expectation is the oracle's
or a restatement's from tests/, evaluated on the state_dict of the module under test.  Every test prints `err`, `floor`
and their ratio before it asserts (pytest -s)."""
import pytest
import torch

import update_cases as U
import update_s2s_cases as S2S
from aether_amd import _lib
from update_parity import check_update

pytestmark = pytest.mark.gpu
STREAMED = _lib.FLAG_FORCE_STREAMED


def _set_option(name, value):
    _lib.check(_lib.load().aether_set_option(name, value), "set_option")


def _forward(family_name, case, flags=0):
    family = U.FAMILIES[family_name]
    m = family.build(case, "cuda").eval()
    if flags:
        m.flags = flags
    x, want64, want32 = U.references_from(family, case, U.state_of(m))
    with torch.no_grad():
        got = family.call(m, U.to_cuda(family.inputs(case)), case)
    torch.cuda.synchronize()
    return got.cpu(), want32, x, want64


@pytest.mark.parametrize("flags", [0, STREAMED], ids=["default", "streamed"])
@pytest.mark.parametrize("case", U.AETHER_64 + U.AETHER_NARROW, ids=lambda c: U.case_id(("Aether", c)))
def test_aether_on_the_64_wide_kernels(case, flags):
    """Hidden 64 and the widths zero-padded to it, fused (k_fused: one and two node tiles, edge tiles across graph
    boundaries, the 12-wave instance) and streamed."""
    check_update(f"{U.case_id(('Aether', case))} flags={flags}", *_forward("Aether", case, flags))


@pytest.mark.parametrize("case", [c for c in U.AETHER_64 if c[2:4] == (2, 20)], ids=lambda c: U.case_id(("Aether", c)))
def test_aether_two_node_tiles_without_the_split_workgroup(case):
    """B2N20 with the `fused_split` option off: the instance of k_fused that keeps both node tiles in one workgroup."""
    try:
        _set_option(b"fused_split", 0)
        check_update(f"{U.case_id(('Aether', case))} fused_split=0", *_forward("Aether", case))
    finally:
        _set_option(b"fused_split", 1)


@pytest.mark.parametrize("case", U.AETHER_WIDE, ids=lambda c: U.case_id(("Aether", c)))
def test_aether_on_the_wide_path(case):
    """Hidden 128 and 192 (csrc/wide.h) and 70 (zero-padded to 128)."""
    check_update(U.case_id(("Aether", case)), *_forward("Aether", case))


@pytest.mark.parametrize("fc", [("LoCS", c) for c in U.LOCS_CASES] + [("DynamicFieldAether", c) for c in U.DYNFIELD_CASES] +
                         U.GNN_CASES, ids=U.case_id)
def test_the_other_state2state_models(fc):
    check_update(U.case_id(fc), *_forward(*fc))


@pytest.mark.parametrize("fc", U.ROLLOUT_CASES, ids=U.case_id)
def test_device_rollout_step_by_step(fc):
    """Five steps at B2N5.  Step t is held on its increment: traj[t] against the fp64 loop's traj64[t] with
    x = traj64[t - 1], and the bar is 4 x the fp32 loop's figure at the same step, so what the steps amplify is in the
    reference as well."""
    family_name, case = fc
    family = U.FAMILIES[family_name]
    m = family.build(case, "cuda").eval()
    x, want64, want32 = U.references_from(family, case, U.state_of(m), U.ROLLOUT_STEPS)
    with torch.no_grad():
        got = family.rollout(m, U.to_cuda(family.inputs(case)), case, U.ROLLOUT_STEPS)
    torch.cuda.synchronize()
    got = got.cpu()
    assert got.shape == want64.shape
    prev = torch.cat([x.double()[None], want64[:-1]])
    for t in range(U.ROLLOUT_STEPS):
        check_update(f"{U.case_id(fc)} rollout step {t}", got[t], want32[t], prev[t], want64[t])


@pytest.mark.parametrize("steps", [1, 3], ids=["one_step", "three_steps"])
@pytest.mark.parametrize("case", S2S.CASES, ids=S2S.case_id)
def test_seq2seq_and_variable_n_steps(case, steps):
    """N = 5, B = 3, D = 2 and 3: one fused step from a random state, and `predict_future` over one burn-in step and three
    predicted ones, with given uniform draws.  The metric is applied to "output state minus input state", per step as in
    the rollouts.  The hard Gumbel sample is discontinuous: the seeds keep every edge's two largest scores at least 1e-3
    apart in the fp64 loop (tests/update_s2s_cases.py), and the kernels have to draw the types that loop draws."""
    S2S.check(case, steps)
