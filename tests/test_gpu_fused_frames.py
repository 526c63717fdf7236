"""k_fused<D, 12, 1, false>: frames beside the field net, x0 behind the prologue's barrier (HISTORY R24).
The frame of a node (R, cv = R^T v) needs its velocity alone: wave 2 + t builds it for visible node tile t while the field
wave of that tile runs the field net, which stores the force alone; cf = R^T f is computed by whoever reads a record (the
feature build's receiver copy, the x0 waves); x0 is computed by waves 4-7 behind the barrier, on operands they load
themselves.  Who computes what changed, the operations did not: every GPU case asks for the bits of the 8-wave kernel
(`fused_waves12` 0) on the same view, compared as int32 so that NaNs count.

(a) CPU: the wave roles through the library's own constexprs (aether_debug_fused_wave_role) -- every visible node tile
    has one frame wave, every 16-row block of x0 one wave;
(b) shapes: N = 17 at B = 1 and 3 (9 / 8 tiles: waves without a tile, second halves whose own nodes straddle both visible
    node tiles), N = 20 at B = 2, N = 19 at B = 1, D = 3, and an unsplit view (N = 14: one visible node tile, off = 0);
(c) the frame's branches on velocities set by hand: v_y < 0, (-1, +0), (-1, -0), 0, a subnormal; D = 3: along +z and -z;
    a NaN velocity in one graph of three;
(d) nothing left over from the previous launch: two batches and two weight sets alternating on one view, ten captured
    steps replayed five times;
(e) the other entry paths: a 3-step device rollout against 3 x 1 step, the external field of DynamicFieldAether;
(f) layer 1's res Linear (the x0 waves' operands) changed in place; one shape against the fp64 oracle at 1e-5.
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_state_dict, scale_rel_err
from aether_amd import _lib
from aether_amd.synthetic import make_batch
from fused_cases import TOL, call_model, fused_model, no_async_error, oracle_of, run_model, set_option, tiles_of, to_device
from fused_cases import uses_twelve_waves
from fused_cases import options_restored  # noqa: F401  (autouse fixture: applies to the tests of this file)


def test_wave_roles_give_every_node_tile_and_row_block_one_owner():
    role = _lib.load().aether_debug_fused_wave_role
    waves = range(12)
    # frames: visible node tiles 0 and 1, one wave each, neither a field wave (waves 0, 1)
    frame = {w: role(0, w) for w in waves}
    assert sorted(t for t in frame.values() if t >= 0) == [0, 1]
    assert all(w >= 2 and t == w - 2 for w, t in frame.items() if t >= 0)
    # x0: the four 16-row blocks of the 64 rows, one wave each, none of them a feature-building wave (0-3)
    x0 = {w: role(1, w) for w in waves}
    assert sorted(b for b in x0.values() if b >= 0) == [0, 1, 2, 3]
    assert all(4 <= w < 8 and b == w - 4 for w, b in x0.items() if b >= 0)
    assert role(0, 12) == -1 and role(1, -1) == -1 and role(2, 4) == -1


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def eight_and_twelve(run):
    set_option(b"fused_waves12", 0)
    eight = run()
    set_option(b"fused_waves12", 1)
    return eight, run()


def twelve_wave_view(m, d, n_nodes, split=1):
    set_option(b"fused_split", split)                   # read when the graph view is built
    info = m.prepare_graph(d["edges"], n_nodes)[1]
    set_option(b"fused_split", 1)
    assert uses_twelve_waves(info) and bool(info.reserved & 1) == bool(split), (tiles_of(info), info.max_group_nodes)
    return info


# (D, N, B, fused_split, tiles of the largest workgroup)
SHAPES = [(2, 17, 1, 1, 9), (2, 17, 3, 1, 9), (2, 20, 2, 1, 12), (2, 19, 1, 1, 12), (3, 20, 1, 1, 12), (2, 14, 2, 0, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,N,B,split,tiles", SHAPES)
def test_shapes_give_the_eight_wave_kernels_bits(D, N, B, split, tiles):
    d = to_device(make_batch(B, N, D, seed=2400 + 10 * N + D + B))
    m = fused_model(D)
    info = twelve_wave_view(m, d, B * N, split)
    assert tiles_of(info) == tiles and info.n_groups == (2 * B if split else B)
    eight, twelve = eight_and_twelve(lambda: run_model(m, d))
    assert torch.isfinite(twelve).all() and same_bits(twelve, eight)
    no_async_error()


SUBNORMAL = 1e-40
BRANCHES = {
    2: [(0.3, -0.7), (-0.4, -1e-3), (-1.0, 0.0), (-1.0, -0.0), (0.0, 0.0), (-0.0, 0.0), (SUBNORMAL, -2 * SUBNORMAL),
        (-SUBNORMAL, 0.0), (0.0, -1.0), (1.0, 0.0)],
    3: [(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (0.0, 0.0, 0.0), (-1.0, -0.0, 0.5), (-1.0, 0.0, -0.5), (0.3, -0.7, 0.2),
        (SUBNORMAL, -SUBNORMAL, SUBNORMAL), (0.0, 0.0, SUBNORMAL), (-0.0, -0.0, -2.5), (1e-3, -1e-3, 3.0)],
}


@pytest.mark.gpu
@pytest.mark.parametrize("D,B", [(2, 2), (3, 1)])
def test_frame_branches_give_the_eight_wave_kernels_bits(D, B):
    N = 20
    inp = make_batch(B, N, D, seed=2410 + D)
    rows = torch.tensor(BRANCHES[D], dtype=torch.float32)
    assert (rows.abs().max(dim=1).values[6:8] < 1.1754944e-38).all()          # they are subnormals in fp32
    # both halves of a split graph (own nodes 0-9 and 10-19) meet every branch
    inp["vel"][0:len(rows)] = rows
    inp["vel"][N - len(rows):N] = rows.flip(0)
    d = to_device(inp)
    m = fused_model(D)
    twelve_wave_view(m, d, B * N)
    eight, twelve = eight_and_twelve(lambda: run_model(m, d))
    assert same_bits(twelve, eight)
    no_async_error()


@pytest.mark.gpu
def test_nan_velocity_stays_in_its_graph():
    N = 17
    inp = make_batch(3, N, 2, seed=2420)
    m = fused_model(2)
    clean = run_model(m, to_device(inp))
    inp["vel"][N + 5, 1] = float("nan")                      # graph 1
    d = to_device(inp)
    twelve_wave_view(m, d, 3 * N)
    eight, twelve = eight_and_twelve(lambda: run_model(m, d))
    assert torch.isnan(twelve[N:2 * N]).any() and same_bits(twelve, eight)
    assert torch.isfinite(clean).all() and same_bits(twelve[:N], clean[:N]) and same_bits(twelve[2 * N:], clean[2 * N:])
    no_async_error()


@pytest.mark.gpu
def test_two_batches_and_two_weight_sets_alternate_on_one_view():
    N, B = 20, 2
    batches = [make_batch(B, N, 2, seed=2430), make_batch(B, N, 2, seed=2431)]
    batches[1]["edges"] = batches[0]["edges"]
    batches[1]["vel"] = -1.5 * batches[1]["vel"]
    ds = [to_device(b) for b in batches]
    sd_a = load_state_dict(2)
    sd_b = {k: (v * 1.0625 if v.is_floating_point() else v) for k, v in sd_a.items()}
    m = fused_model(2)
    twelve_wave_view(m, ds[0], B * N)
    set_option(b"fused_waves12", 0)
    want = {}
    for w, sd in enumerate((sd_a, sd_b)):
        m.load_state_dict(sd)
        for b in range(2):
            want[(b, w)] = run_model(m, ds[b])
    assert len({tuple(v.view(torch.int32).flatten().tolist()) for v in want.values()}) == 4      # four different results
    set_option(b"fused_waves12", 1)
    for k in range(20):
        b, w = k % 2, (k // 2) % 2
        if k % 2 == 0:
            m.load_state_dict((sd_a, sd_b)[w])
        assert same_bits(run_model(m, ds[b]), want[(b, w)]), k
    no_async_error()


@pytest.mark.gpu
def test_ten_captured_steps_replayed_five_times_equal_the_eight_wave_kernel():
    N, B = 20, 2
    d = to_device(make_batch(B, N, 2, seed=2440))
    m = fused_model(2)
    twelve_wave_view(m, d, B * N)
    set_option(b"fused_waves12", 0)
    eight = run_model(m, d)
    set_option(b"fused_waves12", 1)
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
            assert same_bits(o.cpu(), eight), (rep, k)
    no_async_error()


@pytest.mark.gpu
def test_rollout_of_three_steps_equals_three_single_steps():
    N, B = 20, 2
    d = to_device(make_batch(B, N, 2, seed=2450))
    m = fused_model(2)
    twelve_wave_view(m, d, B * N)
    whole = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    x, vel = d["x"], d["vel"]
    for t in range(3):
        nxt = m.rollout(x, vel, d["edges"], d["charges"], 1, 1.0)[0]
        assert same_bits(nxt, whole[t]), t
        x, vel = nxt, (nxt - x) / 1.0          # the protocol's next velocity at dt = 1: one exact fp32 subtraction
    set_option(b"fused_waves12", 0)
    eight = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    torch.cuda.synchronize()
    assert torch.isfinite(whole).all() and same_bits(whole, eight)
    no_async_error()


@pytest.mark.gpu
def test_external_field_gives_the_eight_wave_kernels_bits():
    from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
    data = np.load(os.path.join(GOLDEN, "dynfield_D2.npz"))
    sd = {str(k): torch.from_numpy(data["sd." + str(k)]) for k in data["keys"]}
    m = DynamicFieldAether(4, 64, 0.0, 2, device="cuda")
    m.load_state_dict(sd)
    d = to_device(make_batch(2, 20, 2, seed=2460))

    def run():
        with torch.no_grad():
            out = m(None, d["x"], d["edges"], d["vel"], d["edge_attr"], d["charges"], 20)
        torch.cuda.synchronize()
        return out.cpu()

    eight, twelve = eight_and_twelve(run)
    assert torch.isfinite(twelve).all() and same_bits(twelve, eight)
    no_async_error()


@pytest.mark.gpu
def test_res_linear_changed_in_place_reaches_the_x0_waves():
    d = to_device(make_batch(2, 20, 2, seed=2470))
    m = fused_model(2)
    twelve_wave_view(m, d, 40)
    first = run_model(m, d)
    params = dict(m.named_parameters())
    with torch.no_grad():
        params["gnn.layer_1.res.weight"].add_(0.03125)
    second = run_model(m, d)
    with torch.no_grad():
        params["gnn.layer_1.res.bias"].sub_(0.0625)
    third = run_model(m, d)
    set_option(b"fused_waves12", 0)
    eight = run_model(m, d)
    assert torch.isfinite(third).all() and not same_bits(second, first) and not same_bits(third, second)
    assert same_bits(third, eight)
    no_async_error()


@functools.lru_cache(maxsize=None)
def _oracle_case():
    inp = make_batch(2, 20, 2, seed=2480)
    return inp, oracle_of(load_state_dict(2), inp)


@pytest.mark.gpu
def test_matches_the_fp64_oracle():
    inp, want = _oracle_case()
    d = to_device(inp)
    m = fused_model(2)
    twelve_wave_view(m, d, 40)
    got = run_model(m, d)
    err = scale_rel_err(got.double(), want)
    print(f"N=20 B=2: err={err:.2e}")
    assert torch.isfinite(got).all() and err <= TOL, err
    no_async_error()
