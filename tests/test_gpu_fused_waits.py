"""k_fused after the memory waits of its prologue and tiles were removed (HISTORY R12): the LDS word `arrived` is an
LDS-typed pointer, the field wave's loads are unconditional on clamped indices with one wait, the node's nrange record
is requested during P1, and the node phase's weight fragments come by buffer loads.  None of the arithmetic changed;
the GPU tests hold the inference and the save-for-backward kernel to the fp64 oracle at the project's scale-relative
bars (1e-5 forward, 5e-5 gradients) on the graphs whose structure reaches every clamped load and select:

  n20_b2_d2 / _d3   split pairs (10 + 10 nodes): the partner wait on `arrived`, run boundary inside a tile
  n18_b130          2 * 130 > 256 workgroups: unsplit, two node tiles, 20 edge tiles (three per wave on waves 0-3)
  n5_b3             one tile per workgroup, padding rows, nodes slots beyond n (clamped nrange index)
  pairs_16          one-edge workgroups: every lane but one has no edge record (clamped ledge index, zero record)
  star_32           one receiver with 31 in-edges, its partner workgroup has m = 0 (descriptor read instead of records)
  isolated_n12      two 12-node graphs, every in-edge of node 3 dropped: a node without a tile (empty nrange runs)

Repeated calls must be bit-equal on both kernels (a race around `arrived` or the moved loads would show), a rollout of
three steps must equal three rollouts of one (the q_i q_j branch of the edge attributes), and one DynamicFieldAether
forward covers the external-field path.  The CPU tests assert that the fp32 oracle itself stays below a quarter of each
bar on every case."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_state_dict, scale_rel_err
from aether_amd.edges import prepare_edge_attr
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O
from fused_cases import KERNELS, fused_model, oracle_of, run_model, to_device

TOL = 1e-5
GTOL = 5e-5


def _with_edges(inp, send, recv):
    inp = dict(inp)
    inp["edges"] = [send, recv]
    inp["edge_attr"] = prepare_edge_attr(inp["x"], inp["edges"], inp["charges"][send] * inp["charges"][recv])
    return inp


def _star(seed):
    inp = make_batch(1, 32, 2, seed=seed)
    return _with_edges(inp, torch.arange(1, 32), torch.zeros(31, dtype=torch.long))


def _isolated(seed):
    inp = make_batch(2, 12, 2, seed=seed)
    send, recv = inp["edges"]
    keep = (recv % 12) != 3
    return _with_edges(inp, send[keep].clone(), recv[keep].clone())


CASES = {
    "n20_b2_d2": lambda: make_batch(2, 20, 2, seed=1201),
    "n20_b2_d3": lambda: make_batch(2, 20, 3, seed=1202),
    "n18_b130": lambda: make_batch(130, 18, 2, seed=1203),
    "n5_b3": lambda: make_batch(3, 5, 2, seed=1204),
    "pairs_16": lambda: make_batch(16, 2, 2, seed=1205),
    "star_32": lambda: _star(1206),
    "isolated_n12": lambda: _isolated(1207),
}
GRAD_CASES = ["n20_b2_d2", "n5_b3"]


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


def _dims(inp):
    return inp["x"].shape[1]


@functools.lru_cache(maxsize=None)
def _want64(name):
    inp = _case(name)
    return oracle_of(load_state_dict(_dims(inp)), inp)


@functools.lru_cache(maxsize=None)
def _oracle_grads(name, double):
    inp = _case(name)
    cast = (lambda t: t.double()) if double else (lambda t: t)
    sdg = {k: cast(v).clone().requires_grad_(True) for k, v in load_state_dict(_dims(inp)).items()}
    out = O.aether_forward(sdg, cast(inp["x"]), cast(inp["vel"]), inp["edges"], cast(inp["edge_attr"]), cast(inp["charges"]))
    torch.nn.functional.mse_loss(out, cast(inp["target"])).backward()
    return out.detach(), {k: v.grad for k, v in sdg.items()}


@functools.lru_cache(maxsize=None)
def _dynfield(double):
    """(state dict, inputs, oracle output) of the dynamic-field model at N = 20, B = 2."""
    d = np.load(os.path.join(GOLDEN, "dynfield_D2.npz"))
    sd = {str(k): torch.from_numpy(d["sd." + str(k)]) for k in d["keys"]}
    inp = make_batch(2, 20, 2, seed=1208)
    cast = (lambda t: t.double()) if double else (lambda t: t)
    with torch.no_grad():
        want = O.dynamic_field_aether_forward({k: cast(v) for k, v in sd.items()}, cast(inp["x"]), cast(inp["vel"]),
                                              inp["edges"], cast(inp["edge_attr"]), cast(inp["charges"]), 20)
    return sd, inp, want


# ------------------------------------------------------------------------------------------------------ on the CPU
def test_cases_have_the_structure_they_are_there_for():
    star, iso = _case("star_32"), _case("isolated_n12")
    assert star["edges"][1].unique().tolist() == [0] and star["edges"][0].numel() == 31
    indeg = torch.bincount(iso["edges"][1], minlength=24)
    assert indeg[3] == 0 and indeg[15] == 0 and (indeg[[0, 1, 2, 4]] == 11).all()
    assert _case("pairs_16")["edges"][0].numel() == 32 and _case("n18_b130")["edges"][0].numel() == 130 * 306


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_oracle_stays_below_a_quarter_of_the_forward_bar(name):
    inp = _case(name)
    with torch.no_grad():
        got = O.aether_forward(load_state_dict(_dims(inp)), inp["x"], inp["vel"], inp["edges"], inp["edge_attr"],
                               inp["charges"])
    err = scale_rel_err(got, _want64(name))
    print(f"{name}: fp32 oracle {err:.2e}")
    assert err <= TOL / 4, err


@pytest.mark.parametrize("name", GRAD_CASES)
def test_fp32_oracle_stays_below_a_quarter_of_the_gradient_bar(name):
    _, g64 = _oracle_grads(name, True)
    _, g32 = _oracle_grads(name, False)
    worst = max(scale_rel_err(g32[k], g64[k]) for k in g64)
    print(f"{name}: fp32 oracle gradients {worst:.2e}")
    assert worst <= GTOL / 4, worst


def test_fp32_oracle_of_the_dynamic_field_stays_below_a_quarter_of_the_forward_bar():
    err = scale_rel_err(_dynfield(False)[2], _dynfield(True)[2])
    print(f"dynamic field: fp32 oracle {err:.2e}")
    assert err <= TOL / 4, err


# ------------------------------------------------------------------------------------------------------ on the GPU


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["inference", "keep"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_the_fp64_oracle(name, kernel):
    inp = _case(name)
    m = fused_model(_dims(inp), KERNELS[kernel])
    out = run_model(m, to_device(inp))
    err = scale_rel_err(out.double(), _want64(name))
    print(f"{name} {kernel}: err={err:.2e}")
    assert torch.isfinite(out).all() and err <= TOL, err


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAD_CASES)
def test_training_forward_and_gradients(name):
    inp = _case(name)
    want, g64 = _oracle_grads(name, True)
    m = fused_model(_dims(inp), KERNELS["inference"])
    m.zero_grad(set_to_none=True)
    d = to_device(inp)
    out = m(d["h"], d["x"], d["edges"], d["vel"], d["edge_attr"], d["charges"])
    torch.nn.functional.mse_loss(out, d["target"]).backward()
    torch.cuda.synchronize()
    assert scale_rel_err(out.detach().cpu().double(), want) <= TOL
    for k, p in m.named_parameters():
        err = scale_rel_err(p.grad.detach().cpu(), g64[k])
        assert err <= GTOL, (k, err)


@pytest.mark.gpu
def test_twenty_calls_are_bit_equal():
    d = to_device(_case("n20_b2_d2"))
    for kernel, flags in KERNELS.items():
        m = fused_model(2, flags)
        first = run_model(m, d)
        for _ in range(19):
            assert torch.equal(run_model(m, d), first), kernel


@pytest.mark.gpu
def test_rollout_of_three_steps_equals_three_rollouts_of_one():
    d = to_device(_case("n20_b2_d2"))
    m = fused_model(2, KERNELS["inference"])
    whole = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    x, vel = d["x"], d["vel"]
    for t in range(3):
        nxt = m.rollout(x, vel, d["edges"], d["charges"], 1, 1.0)[0]
        assert torch.equal(nxt, whole[t]), t
        x, vel = nxt, (nxt - x) / 1.0          # the protocol's next velocity at dt = 1: one exact fp32 subtraction
    torch.cuda.synchronize()
    assert torch.isfinite(whole).all()


@pytest.mark.gpu
def test_dynamic_field_forward_matches_the_fp64_oracle():
    from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
    sd, inp, want = _dynfield(True)
    m = DynamicFieldAether(4, 64, 0.0, 2, device="cuda")
    m.load_state_dict(sd)
    d = to_device(inp)
    with torch.no_grad():
        out = m(None, d["x"], d["edges"], d["vel"], d["edge_attr"], d["charges"], 20)
    torch.cuda.synchronize()
    err = scale_rel_err(out.cpu().double(), want)
    print(f"dynamic field: err={err:.2e}")
    assert torch.isfinite(out).all() and err <= TOL, err
