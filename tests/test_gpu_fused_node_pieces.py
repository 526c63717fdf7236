"""k_fused<D, 12, 1, false>: the node phase's shared operands (n, u, x, the out MLP's o1) are split into fp16 pieces once,
by the waves that produce them, and the range decision of the split (common.h, split_scale_of) travels to the consumers
as one word per producing wave (HISTORY R21).  The pieces are the same function of the same fp32 values
and the scaled path is the code of before, so every case here asks for the bits of the 8-wave kernel (`fused_waves12`
0), which splits in the consumer, on the same view.

(a) shapes: every role layout of the twelve waves.  The smallest split view on twelve waves is N = 17 (halves of 9 and 8
    nodes, 144 in-edges = 9 tiles): the views that the default options build for N = 12 .. 16 have no workgroup of 9 - 12
    tiles and one node tile (a half of N = 16 has 8 tiles), so the dispatch rule keeps them on the 8-wave kernels (asserted
    below); the B = 3 case therefore runs at N = 17, and N = 12 runs as the unsplit view of 9 tiles.
(b) range words: operands at or above 2^15 in one node only (one producing wave's word decides), all operands below 2^-6,
    all operands zero.  The magnitudes are chosen and checked on the CPU (node_operands, an fp32 restatement of the
    oracle's layer); inputs alone cannot do it, a layer adds its biases, so the cases also change the weights:
      big   layer 1's second message Linear is zero (no message: n = res(rel_feat) of the node alone) and one node of
            graph 0 moves at 2^18
      tiny  the Linears that end in n, u, x or o1 are multiplied by 2^-12
      zero  the same Linears are zero
(c) a NaN in one node's velocity: the range words drop a NaN as fmaxf does in the consumer's test.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from conftest import load_state_dict
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O
from fused_cases import fused_model, run_model, set_option, tiles_of, to_device, uses_twelve_waves
from fused_cases import options_restored  # noqa: F401  (autouse fixture: applies to the tests of this file)

BIG, SMALL = 32768.0, 0.015625              # split_scale_of's thresholds: 2^15, 2^-6
# the Linears whose outputs are the node phase's operands
NODE_LINEARS = (["gnn.layer_1.res", "gnn.out_mlp.0"] +
                [f"gnn.layer_{k}.{name}" for k in range(1, 5) for name in ("message_fn.2", "update_fn.0", "update_fn.2")])


def node_operands(sd, inp):
    """fp32 n, u, x of the four layers and o1, [nodes, units] each: oracle.aether_oracle.gnn_layer / out_mlp with the
    intermediates kept."""
    D = inp["x"].shape[-1]
    send, recv = inp["edges"]
    lin = lambda name, v: O._linear(sd, name, v)
    with torch.no_grad():
        ext = torch.cat([inp["x"], inp["vel"], O.field_net(sd, inp["x"], inp["vel"], inp["charges"])], dim=-1)
        h, _ = O.canonical_nodes(ext, D)
        e = torch.cat([O.edge_features(ext, send, recv, D), h[recv], inp["edge_attr"]], -1)
        ops = {}
        for k in range(1, 5):
            p = f"gnn.layer_{k}"
            m = F.silu(lin(p + ".message_fn.0", e if k == 1 else torch.cat([h[send], h[recv], e], dim=-1)))
            m = F.silu(lin(p + ".message_fn.2", m))
            n = (lin(p + ".res", h) if k == 1 else h) + O.scatter_mean(m, recv, h.shape[0])
            u = F.silu(lin(p + ".update_fn.0", n))
            h, e = n + lin(p + ".update_fn.2", u), m
            ops[f"n{k}"], ops[f"u{k}"], ops[f"x{k}"] = n, u, h
        ops["o1"] = F.silu(lin("gnn.out_mlp.0", h))
    return ops


BIG_NODE = 3                                 # graph 0, first half of its split pair


@functools.lru_cache(maxsize=None)
def flag_case(kind):
    sd = {k: v.clone() for k, v in load_state_dict(2).items()}
    inp = make_batch(2, 20, 2, seed=2100)
    if kind == "big":
        for part in ("weight", "bias"):
            sd[f"gnn.layer_1.message_fn.2.{part}"].zero_()
        inp["vel"][BIG_NODE] *= 2.0 ** 19            # |vel| = 0.5 (make_batch) -> 2^18
        inp["h"] = inp["vel"].norm(dim=-1, keepdim=True)
    else:
        for name in NODE_LINEARS:
            for part in ("weight", "bias"):
                sd[f"{name}.{part}"].mul_(2.0 ** -12 if kind == "tiny" else 0.0)
    return sd, inp


def check_flag_case(kind):
    """The thresholds are crossed where the case intends, with a factor of two to spare for the kernel's own roundings."""
    sd, inp = flag_case(kind)
    ops = node_operands(sd, inp)
    assert all(torch.isfinite(v).all() for v in ops.values())
    if kind == "big":
        rows = ops["n1"].abs().max(dim=1).values
        others = torch.cat([rows[:BIG_NODE], rows[BIG_NODE + 1:]])
        print(f"big: n1 of node {BIG_NODE} reaches {float(rows[BIG_NODE]):.3e}, every other node stays at {float(others.max()):.3e}")
        assert rows[BIG_NODE] >= 2 * BIG and others.max() < BIG / 2 and others.min() >= 2 * SMALL
    elif kind == "tiny":
        for name, v in ops.items():
            # per workgroup (a half of 10 nodes) and, for u, per 64-unit half: each has a non-zero and none reaches 2^-6
            for blk in v.reshape(4, 10, -1, 64).permute(0, 2, 1, 3).reshape(-1, 640):
                assert 0.0 < blk.abs().max() < SMALL / 2, (name, float(blk.abs().max()))
        print("tiny: largest operand", max(float(v.abs().max()) for v in ops.values()))
    else:
        assert all(not v.any() for v in ops.values())


@pytest.mark.parametrize("kind", ["big", "tiny", "zero"])
def test_flag_cases_cross_the_intended_thresholds(kind):
    check_flag_case(kind)


def eight_and_twelve(m, d):
    set_option(b"fused_waves12", 0)
    eight = run_model(m, d)
    set_option(b"fused_waves12", 1)
    return eight, run_model(m, d)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# (D, N, B, fused_split, tiles)
SHAPES = [(2, 20, 2, 1, 12), (2, 17, 2, 1, 9), (2, 17, 3, 1, 9), (2, 12, 3, 0, 9), (3, 20, 1, 1, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,N,B,split,tiles", SHAPES)
def test_shapes_give_the_eight_wave_kernels_bits(D, N, B, split, tiles):
    inp = make_batch(B, N, D, seed=2100 + 10 * N + D)
    d = to_device(inp)
    m = fused_model(D)
    set_option(b"fused_split", split)                   # read when the graph view is built
    info = m.prepare_graph(d["edges"], B * N)[1]
    set_option(b"fused_split", 1)
    assert tiles_of(info) == tiles and bool(info.reserved & 1) == bool(split) and uses_twelve_waves(info)
    eight, twelve = eight_and_twelve(m, d)
    assert torch.isfinite(twelve).all() and same_bits(twelve, eight)


@pytest.mark.gpu
def test_no_split_view_below_seventeen_nodes_runs_on_twelve_waves():
    for N in range(12, 17):
        d = to_device(make_batch(3, N, 2, seed=2100 + N))
        info = fused_model(2).prepare_graph(d["edges"], 3 * N)[1]
        print(f"N={N}: split={info.reserved & 1} groups={info.n_groups} tiles={tiles_of(info)} nodes={info.max_group_nodes}")
        assert not uses_twelve_waves(info), N


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["big", "tiny", "zero"])
def test_range_words_give_the_eight_wave_kernels_bits(kind):
    check_flag_case(kind)
    sd, inp = flag_case(kind)
    d = to_device(inp)
    m = fused_model(2, sd=sd)
    info = m.prepare_graph(d["edges"], 40)[1]
    assert tiles_of(info) == 12 and info.reserved & 1 and uses_twelve_waves(info)
    eight, twelve = eight_and_twelve(m, d)
    assert torch.isfinite(twelve).all() and same_bits(twelve, eight)


@pytest.mark.gpu
def test_nan_velocity_gives_the_eight_wave_kernels_bits():
    inp = make_batch(2, 20, 2, seed=2100)
    inp["vel"][BIG_NODE, 0] = float("nan")
    d = to_device(inp)
    m = fused_model(2)
    assert uses_twelve_waves(m.prepare_graph(d["edges"], 40)[1])
    eight, twelve = eight_and_twelve(m, d)
    assert torch.isnan(twelve[:20]).any() and torch.isfinite(twelve[20:]).all()      # graph 0 has it, graph 1 does not
    assert same_bits(twelve, eight)
