"""k_fused, layers 2-4 of a split view: the first Linear of an edge tile runs under the wait for the partner workgroup's
P_s rows (HISTORY R17).  A partner-sender edge (local position >= na) starts its accumulator at
P_r[recv] alone and gets P_s[send] added behind the W_e e product, in front of the first SiLU; every other edge keeps
P_r + P_s as the start.  One rule in every kernel that runs workgroups of 9-16 tiles (12 waves, or 8 waves with two
tiles on some; the one-tile 8-wave kernels keep P_r + P_s in one rounding): the four dispatches `fused_waves12` {0, 1} x `fused_granules`
{0, 1} must give the same bits on one view, and each is held to the fp64 oracle at the project's scale-relative bars
(1e-5 forward, 5e-5 parameter gradients).

What can go wrong: a lane on the wrong side of na (a P_s row added twice, never, or read before it arrived), the wait or
the receive skipped on a wave without a tile or without a partner-sender tile (N = 17: wave 11 idle), a tile that
straddles na, a workgroup with no own-sender edge at all, a second receive sweep, and a non-finite row of the previous
layer read early and not selected away.
"""
import functools

import pytest
import torch

from conftest import load_state_dict, scale_rel_err
from aether_amd.edges import prepare_edge_attr
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O
from fused_cases import (TOL, call_model, check_four_ways, four_ways, fused_model, no_async_error, oracle_of, run_model,
                         set_option, tiles_of, to_device, uses_twelve_waves)
from fused_cases import options_restored  # noqa: F401  (autouse fixture: applies to the tests of this file)

pytestmark = pytest.mark.gpu
GTOL = 5e-5


@functools.lru_cache(maxsize=None)
def _inputs(D, N, B):
    return make_batch(B, N, D, seed=1700 + 10 * N + D)


@functools.lru_cache(maxsize=None)
def _oracle(D, N, B):
    return oracle_of(load_state_dict(D), _inputs(D, N, B))


# N = 20: na = 90 of 190 (tile 5 straddles it, tiles 6-11 are all partner senders); N = 17 / 18: na = 72 (tile 4 ends at
# 80), N = 17 has 9 tiles: waves 9-11 of the 12-wave kernel idle, the receiving wave among them; N = 16: na = 56, 8 tiles:
# the 8-wave kernel <D, 8, 1> whatever the option says
@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("D,N", [(2, 20), (3, 20), (2, 17), (2, 18), (2, 16)])
def test_four_dispatches_give_the_same_bits_and_match_the_oracle(D, N, B):
    d = to_device(_inputs(D, N, B))
    m = fused_model(D)
    info = m.prepare_graph(d["edges"], B * N)[1]
    assert info.n_groups == 2 * B and info.reserved & 1, (info.n_groups, info.reserved)
    assert uses_twelve_waves(info) == (N != 16), (info.max_group_nodes, info.max_group_edges)
    check_four_ways(m, d, _oracle(D, N, B), f"D={D} N={N} B={B} tiles={tiles_of(info)}")


def test_complete_bipartite_graph_has_no_own_sender():
    """K(12,12), the two parts being the two receiver ranges: every in-edge of a half comes from the partner (na = 0).
    144 in-edges = 9 tiles per half, all of them late; 12 partner rows, so the granule receive takes a second sweep."""
    D, P, B = 2, 12, 2
    N = 2 * P
    inp = make_batch(B, N, D, seed=1724)
    rows, cols = inp["edges"]
    keep = (rows // N == cols // N) & ((rows % N < P) != (cols % N < P))
    inp = dict(inp, edges=[rows[keep], cols[keep]], edge_attr=inp["edge_attr"][keep])
    d = to_device(inp)
    m = fused_model(D)
    info = m.prepare_graph(d["edges"], B * N)[1]
    assert info.n_groups == 2 * B and info.reserved & 1 and uses_twelve_waves(info), \
        (info.n_groups, info.reserved, info.max_group_nodes, info.max_group_edges)
    assert info.max_group_nodes == P and info.max_group_edges == P * P
    check_four_ways(m, d, oracle_of(load_state_dict(D), inp), "K(12,12)")


def test_ring_of_32_nodes_has_partner_senders_in_the_last_tile_only():
    """The sparse ring of tests/test_gpu_fused_granules.py (32 nodes, in-edges from the ten nodes behind a node), split
    16 + 16: of a half's 160 in-edges the last ones only come from the partner, and there are 16 partner rows."""
    D, N, B = 2, 32, 2
    inp = make_batch(B, N, D, seed=1732)
    rows, cols = inp["edges"]
    keep = ((cols - rows) % N >= 1) & ((cols - rows) % N <= 10) & (rows // N == cols // N)
    inp = dict(inp, edges=[rows[keep], cols[keep]], edge_attr=inp["edge_attr"][keep])
    d = to_device(inp)
    m = fused_model(D)
    info = m.prepare_graph(d["edges"], B * N)[1]
    assert info.n_groups == 2 * B and info.reserved & 1 and uses_twelve_waves(info) and info.max_group_nodes == 16, \
        (info.n_groups, info.reserved, info.max_group_nodes, info.max_group_edges)
    check_four_ways(m, d, oracle_of(load_state_dict(D), inp), "ring 32")


@pytest.mark.parametrize("N", [14, 12])
def test_unsplit_views_never_enter_the_late_block(N):
    D, B = 2, 2
    d = to_device(_inputs(D, N, B))
    m = fused_model(D)
    set_option(b"fused_split", 0)                       # read when the graph view is built
    info = m.prepare_graph(d["edges"], B * N)[1]
    set_option(b"fused_split", 1)
    assert info.n_groups == B and not info.reserved & 1, (info.n_groups, info.reserved)
    check_four_ways(m, d, _oracle(D, N, B), f"unsplit N={N}")


def test_inf_in_one_graph_stays_in_that_graph():
    """One coordinate of node 15 of graph 0 (owned by the graph's second workgroup) is inf.  Its P_s row is non-finite
    in every layer; the partner reads the previous layer's row of that slot early and must select it away, not multiply
    it by zero.  Graphs 1 and 2 do not notice, and graph 0 is non-finite in the same places in all four dispatches."""
    D, N, B = 2, 20, 3
    clean = _inputs(D, N, B)
    x = clean["x"].clone()
    x[15, 0] = float("inf")
    rows, cols = clean["edges"]
    bad = dict(clean, x=x, edge_attr=prepare_edge_attr(x, clean["edges"], clean["charges"][rows] * clean["charges"][cols]))
    assert torch.equal(bad["edge_attr"][rows >= N], clean["edge_attr"][rows >= N])     # the other graphs' inputs are the same
    m = fused_model(D)
    dc, db = to_device(clean), to_device(bad)
    info = m.prepare_graph(dc["edges"], B * N)[1]
    assert info.n_groups == 2 * B and info.reserved & 1
    want = four_ways(m, dc)
    got = four_ways(m, db)
    mask = torch.isnan(got[0]) | torch.isinf(got[0])
    assert mask[:N].any() and not mask[N:].any()
    for w, g in zip(want, got):
        assert torch.equal(w, want[0])
        assert torch.equal(g[N:], w[N:])
        assert torch.equal(torch.isnan(g) | torch.isinf(g), mask)
    again = four_ways(m, dc)                               # and nothing non-finite stays behind in the view
    for a in again:
        assert torch.equal(a, want[0])
    no_async_error()


def test_twenty_calls_on_one_view_are_bit_equal():
    D, N, B = 2, 20, 2
    m = fused_model(D)
    d = to_device(_inputs(D, N, B))
    first = run_model(m, d)
    assert scale_rel_err(first.double(), _oracle(D, N, B)) <= TOL
    outs = [call_model(m, d).clone() for _ in range(19)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert torch.equal(o.cpu(), first), k
    no_async_error()


def test_rollout_of_three_steps_equals_three_single_steps():
    D, N, B = 2, 20, 2
    d = to_device(_inputs(D, N, B))
    m = fused_model(D)
    assert uses_twelve_waves(m.prepare_graph(d["edges"], B * N)[1])
    whole = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    x, vel = d["x"], d["vel"]
    for t in range(3):
        nxt = m.rollout(x, vel, d["edges"], d["charges"], 1, 1.0)[0]
        assert torch.equal(nxt, whole[t]), t
        x, vel = nxt, (nxt - x) / 1.0          # the protocol's next velocity at dt = 1: one exact fp32 subtraction
    torch.cuda.synchronize()
    assert torch.isfinite(whole).all()
    no_async_error()


def test_ten_captured_steps_replayed_five_times_equal_eager():
    D, N, B = 2, 20, 3
    m = fused_model(D)
    d = to_device(_inputs(D, N, B))
    eager = run_model(m, d)
    assert scale_rel_err(eager.double(), _oracle(D, N, B)) <= TOL
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            call_model(m, d)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = [call_model(m, d) for _ in range(10)]
    for rep in range(5):
        for o in outs:
            o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            assert torch.equal(o.cpu(), eager), (rep, k)
    no_async_error()


def test_training_forward_and_all_parameter_gradients():
    """k_fused<2, 8, 2, true> at N = 20, B = 2.  Its output is bit-equal to the inference output of the 8-wave kernel
    (fused_waves12 = 0) on the same inputs: the parent of this change has that property (checked on the parent's
    library with these inputs), and the late add is the same expression in both.  The backward recomputes the
    pre-activation as P_s + P_r in one rounding; the 47 parameter gradients are held to the fp64 oracle's autograd."""
    D, N, B = 2, 20, 2
    inp = _inputs(D, N, B)
    sdg = {k: v.double().clone().requires_grad_(True) for k, v in load_state_dict(D).items()}
    want = O.aether_forward(sdg, inp["x"].double(), inp["vel"].double(), inp["edges"], inp["edge_attr"].double(),
                            inp["charges"].double())
    torch.nn.functional.mse_loss(want, inp["target"].double()).backward()
    d = to_device(inp)
    m = fused_model(D)
    set_option(b"fused_waves12", 0)
    inference = run_model(m, d)
    set_option(b"fused_waves12", 1)
    m.zero_grad(set_to_none=True)
    out = m(d["h"], d["x"], d["edges"], d["vel"], d["edge_attr"], d["charges"])
    torch.nn.functional.mse_loss(out, d["target"]).backward()
    torch.cuda.synchronize()
    assert torch.equal(out.detach().cpu(), inference)
    assert scale_rel_err(out.detach().cpu().double(), want.detach()) <= TOL
    params = list(m.named_parameters())
    assert len(params) == 47
    for k, p in params:
        err = scale_rel_err(p.grad.detach().cpu(), sdg[k].grad)
        assert err <= GTOL, (k, err)
    no_async_error()
