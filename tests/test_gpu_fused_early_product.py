"""k_fused, layers 2-4: the first Linear of an edge tile is g = W_e e from +0.0f accumulators, then g + (P_r + P_s), or
(g + P_r) + P_s on an edge whose sender the partner workgroup owns (HISTORY R18).  One rule in every kernel
that runs workgroups of 9-16 tiles; the 12-wave kernels compute g for layer l + 1 under layer l's node phase, in place in
the tile's registers, from the weight image that the LDS-DMA has just brought in.  The four dispatches `fused_waves12`
{0, 1} x `fused_granules` {0, 1} must give the same bits on one view, and each is held to the fp64 oracle at the project's
scale-relative bars (1e-5 forward, 5e-5 parameter gradients).

What the move can break: a wave without a tile that multiplies (or misses a barrier), a product that reads wA before the
next layer's image has landed or while it still holds this layer's, a tile that straddles na, a workgroup with no own
sender, a 12-wave launch without a partner, the operand-scale branch of the split GEMM with zero-start accumulators, and a
non-finite message that leaks out of its graph.
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
    return make_batch(B, N, D, seed=1800 + 10 * N + D)


@functools.lru_cache(maxsize=None)
def _oracle(D, N, B):
    return oracle_of(load_state_dict(D), _inputs(D, N, B))


# N = 20: 190 in-edges per half = 12 tiles, every wave multiplies, na = 90 (tile 5 straddles it).  N = 17: 9 tiles on 12
# waves -- waves 9-11 hold no tile, skip the product and reach every barrier; na = 72 >= 16, so wave 0 receives; the flag
# protocol's receiver (wave 11) is one of the idle three.
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("D,N", [(2, 20), (3, 20), (2, 17)])
def test_four_dispatches_give_the_same_bits_and_match_the_oracle(D, N, B):
    d = to_device(_inputs(D, N, B))
    m = fused_model(D)
    info = m.prepare_graph(d["edges"], B * N)[1]
    assert info.n_groups == 2 * B and info.reserved & 1, (info.n_groups, info.reserved)
    assert uses_twelve_waves(info), (info.max_group_nodes, info.max_group_edges)
    assert tiles_of(info) == (12 if N == 20 else 9)
    check_four_ways(m, d, _oracle(D, N, B), f"D={D} N={N} B={B} tiles={tiles_of(info)}")


def test_complete_bipartite_graph_has_no_own_sender():
    """K(12,12), the two parts being the two receiver ranges: na = 0, every edge adds its P_s late, the last wave
    receives (two sweeps for 12 partner rows) and every tile's g waits in registers for it."""
    D, P, B = 2, 12, 2
    N = 2 * P
    inp = make_batch(B, N, D, seed=1824)
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


@pytest.mark.parametrize("N", [14, 12])
def test_unsplit_views_run_twelve_waves_without_a_partner(N):
    """fused_split = 0: one workgroup per graph, 182 in-edges = 12 tiles (N = 14) or 132 = 9 tiles, the last one with four
    rows (N = 12).  No hand-off at all; every edge is g + (P_r + P_s)."""
    D, B = 2, 2
    d = to_device(_inputs(D, N, B))
    m = fused_model(D)
    set_option(b"fused_split", 0)                       # read when the graph view is built
    info = m.prepare_graph(d["edges"], B * N)[1]
    set_option(b"fused_split", 1)
    assert info.n_groups == B and not info.reserved & 1 and uses_twelve_waves(info), (info.n_groups, info.reserved)
    check_four_ways(m, d, _oracle(D, N, B), f"unsplit N={N}")


def test_two_models_alternate_on_one_view():
    """Two weight sets, called in turn on the same inputs, ten calls each.  A product that reads wA before the DMA of
    its own launch's next image has landed finds the other model's image of a neighbouring launch there (or the
    previous layer's): the output would differ from the model's first."""
    D, N, B = 2, 20, 2
    d = to_device(_inputs(D, N, B))
    sd_a = load_state_dict(D)
    g = torch.Generator().manual_seed(1841)
    sd_b = {k: v + 0.05 * v.abs().max() * torch.randn(v.shape, generator=g) for k, v in sd_a.items()}
    ma, mb = fused_model(D, sd=sd_a), fused_model(D, sd=sd_b)
    assert uses_twelve_waves(ma.prepare_graph(d["edges"], B * N)[1])
    first_a, first_b = run_model(ma, d), run_model(mb, d)
    assert scale_rel_err(first_a.double(), _oracle(D, N, B)) <= TOL
    assert scale_rel_err(first_b.double(), oracle_of(sd_b, _inputs(D, N, B))) <= TOL
    assert not torch.equal(first_a, first_b)
    outs = []
    for _ in range(10):
        outs.append(call_model(ma, d).clone())
        outs.append(call_model(mb, d).clone())
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert torch.equal(o.cpu(), first_b if k & 1 else first_a), k
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


# layer 1's message MLP with its first Linear (weight and bias) times 2^a and its second times 2^b: its messages, the
# operand of layer 2's g, scale with them.  (One factor of 2^18 on a weight matrix would leave the fp16 range of its image.)
@pytest.mark.parametrize("a,b", [(9, 9), (0, -10)])
def test_operand_scale_branch_with_zero_start_accumulators(a, b):
    """split_scale_of rescales a tile whose largest message is at or above 2^15, or below 2^-6, and the accumulators with
    it -- zeros now.  (9, 9): every edge's largest layer-1 message is above 5.6e4 (max 4.5e5) and the node state grows with
    it; (0, -10): the largest message of all is 7.4e-4.  The fp32 oracle's own error against fp64 on these inputs (N = 20,
    B = 2, measured on the CPU): 6.1e-7 at (9, 9), 4.0e-8 at (0, -10), both below a quarter of the bar."""
    D, N, B = 2, 20, 2
    k = a + b
    inp = _inputs(D, N, B)
    sd = {n: v.clone() for n, v in load_state_dict(D).items()}
    for lin, p2 in (("0", a), ("2", b)):
        sd[f"gnn.layer_1.message_fn.{lin}.weight"] *= 2.0 ** p2
        sd[f"gnn.layer_1.message_fn.{lin}.bias"] *= 2.0 ** p2
    res = oracle_of(sd, inp, return_all=True)
    rowmax = res["e1"].abs().max(dim=1).values
    assert (rowmax.min() >= 2.0 ** 15) if k > 0 else (0 < rowmax.max() < 2.0 ** -6), (rowmax.min(), rowmax.max())
    own = scale_rel_err(oracle_of(sd, inp, torch.float32), res["out"])
    print(f"2^{a} x 2^{b}: fp32 oracle against fp64 {own:.2e}")
    assert own <= TOL / 4
    check_four_ways(fused_model(D, sd=sd), to_device(inp), res["out"], f"scale 2^{a} x 2^{b}")


def test_inf_in_one_graph_stays_in_that_graph():
    """One coordinate of node 15 of graph 0 is inf: its tiles' messages, and the products computed early from them, are
    non-finite in every layer.  Graphs 1 and 2 do not notice, and graph 0 is non-finite in the same places in all four
    dispatches; nothing non-finite stays behind in registers, LDS or the view."""
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
    again = four_ways(m, dc)
    for a in again:
        assert torch.equal(a, want[0])
    no_async_error()


def test_training_forward_and_all_parameter_gradients():
    """k_fused<2, 8, 2, true> on the N = 20 split view, B = 2: its output is bit-equal to the inference output of the
    12-wave kernel (and so, by the four-dispatch tests, of all four), and the 47 parameter gradients are held to the fp64
    oracle's autograd."""
    D, N, B = 2, 20, 2
    inp = _inputs(D, N, B)
    sdg = {k: v.double().clone().requires_grad_(True) for k, v in load_state_dict(D).items()}
    want = O.aether_forward(sdg, inp["x"].double(), inp["vel"].double(), inp["edges"], inp["edge_attr"].double(),
                            inp["charges"].double())
    torch.nn.functional.mse_loss(want, inp["target"].double()).backward()
    d = to_device(inp)
    m = fused_model(D)
    assert uses_twelve_waves(m.prepare_graph(d["edges"], B * N)[1])
    inference = run_model(m, d)
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
        print(f"{k}: {err:.2e}")
        assert err <= GTOL, (k, err)
    no_async_error()
