"""k_fused<D, 12, 1, false>: the prologue (HISTORY R23).  The layer-1 edge features of a workgroup's (at
most twelve) tiles are built by one wave per SIMD -- waves 0-3, lanes 0-47, edge 48 wave + lane of the local order -- and
written into the rows of the wave that owns the tile, behind one workgroup barrier, where every wave used to build its own
16 edges on a quarter of its lanes.  Who builds a row changed, `edge_features` and its inputs did not: every GPU case asks
for the bits of the 8-wave kernel (`fused_waves12` 0), which builds its rows per wave, on the same view.

(a) the packed mapping against the tile ownership, for every edge count m = 1 .. 192 (CPU: the library's own constexpr
    through aether_debug_fused_packed_edge);
(b) shapes: N = 20 (12 full tiles), N = 17, 18, 19 (workgroups of 9 / 8, 10, 12 / 11 tiles: waves without a tile, a partial
    last tile, builder lanes beyond m), D = 3;
(c) what else feeds the prologue: all three charge classes, the rollout's derived edge attributes (`qattr`), an external
    field (DynamicFieldAether), a NaN velocity in one graph;
(d) weights changed in place between two inference calls of one module (a field_net weight and layer 1's res Linear): the
    prepared weight data must follow.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from aether_amd import _lib
from aether_amd.synthetic import make_batch
from fused_cases import fused_model, run_model, set_option, tiles_of, to_device, uses_twelve_waves
from fused_cases import options_restored  # noqa: F401  (autouse fixture: applies to the tests of this file)

PACK_WAVES, PACK_LANES, MAX_TILES = 4, 48, 12


def test_packed_mapping_covers_every_row_of_the_owners_tiles():
    lib = _lib.load()
    edge = {(w, l): lib.aether_debug_fused_packed_edge(w, l) for w in range(12) for l in range(64)}
    builders = {}
    for (w, l), f in edge.items():
        if w >= PACK_WAVES or l >= PACK_LANES:
            assert f == -1, (w, l, f)                       # no other wave or lane builds a row
            continue
        assert f == 48 * w + l and f >> 4 == 3 * w + (l >> 4) and f & 15 == l & 15, (w, l, f)
        assert f not in builders, (w, l, f)                 # one builder per row
        builders[f] = (w, l)
    # every row of the twelve tiles is written (rows at or beyond m: zeros), by a lane of waves 0-3
    assert sorted(builders) == list(range(16 * MAX_TILES))
    for m in range(1, 16 * MAX_TILES + 1):
        n_tiles = (m + 15) >> 4
        for f in range(m):
            tile, row = f >> 4, f & 15
            w, l = builders[f]
            # the row's owner (wave `tile`, lane row `row` of its fragment reads) has that tile; its builder holds edge f
            assert tile < n_tiles and edge[(w, l)] == 16 * tile + row
        # builder lanes beyond m exist exactly for the rows that are not edges
        assert sum(1 for f in builders if f >= m) == 16 * MAX_TILES - m


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def eight_and_twelve(run):
    set_option(b"fused_waves12", 0)
    eight = run()
    set_option(b"fused_waves12", 1)
    return eight, run()


def check_view(m, d, n_nodes, tiles):
    info = m.prepare_graph(d["edges"], n_nodes)[1]
    assert tiles_of(info) == tiles and info.reserved & 1 and uses_twelve_waves(info), (tiles_of(info), info.max_group_nodes)


# (D, N, B, tiles of the largest workgroup)
SHAPES = [(2, 20, 2, 12), (2, 17, 2, 9), (2, 18, 2, 10), (2, 19, 2, 12), (3, 20, 1, 12)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,N,B,tiles", SHAPES)
def test_shapes_give_the_eight_wave_kernels_bits(D, N, B, tiles):
    d = to_device(make_batch(B, N, D, seed=2300 + 10 * N + D))
    m = fused_model(D)
    check_view(m, d, B * N, tiles)
    eight, twelve = eight_and_twelve(lambda: run_model(m, d))
    assert torch.isfinite(twelve).all() and same_bits(twelve, eight)


@pytest.mark.gpu
def test_three_charge_classes_give_the_eight_wave_kernels_bits():
    inp = make_batch(2, 20, 2, seed=2301)
    inp["charges"][1::3] = 0.0                               # -1, 0 and +1 in every workgroup
    assert {float(c) for c in inp["charges"].flatten()} == {-1.0, 0.0, 1.0}
    d = to_device(inp)
    m = fused_model(2)
    check_view(m, d, 40, 12)
    eight, twelve = eight_and_twelve(lambda: run_model(m, d))
    assert torch.isfinite(twelve).all() and same_bits(twelve, eight)


@pytest.mark.gpu
def test_two_step_rollout_gives_the_eight_wave_kernels_bits():
    d = to_device(make_batch(2, 20, 2, seed=2302))
    m = fused_model(2)
    check_view(m, d, 40, 12)

    def run():
        out = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 2, 1.0)
        torch.cuda.synchronize()
        return out.cpu()

    eight, twelve = eight_and_twelve(run)
    assert twelve.shape[0] == 2 and torch.isfinite(twelve).all() and same_bits(twelve, eight)


@pytest.mark.gpu
def test_external_field_gives_the_eight_wave_kernels_bits():
    from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
    data = np.load(os.path.join(GOLDEN, "dynfield_D2.npz"))
    sd = {str(k): torch.from_numpy(data["sd." + str(k)]) for k in data["keys"]}
    m = DynamicFieldAether(4, 64, 0.0, 2, device="cuda")
    m.load_state_dict(sd)
    d = to_device(make_batch(2, 20, 2, seed=2303))

    def run():
        with torch.no_grad():
            out = m(None, d["x"], d["edges"], d["vel"], d["edge_attr"], d["charges"], 20)
        torch.cuda.synchronize()
        return out.cpu()

    eight, twelve = eight_and_twelve(run)
    assert torch.isfinite(twelve).all() and same_bits(twelve, eight)


@pytest.mark.gpu
def test_nan_velocity_stays_in_its_graph():
    inp = make_batch(3, 20, 2, seed=2304)
    m = fused_model(2)
    clean = run_model(m, to_device(inp))
    inp["vel"][23, 0] = float("nan")                         # graph 1
    d = to_device(inp)
    check_view(m, d, 60, 12)
    eight, twelve = eight_and_twelve(lambda: run_model(m, d))
    assert torch.isnan(twelve[20:40]).any() and same_bits(twelve, eight)
    assert torch.isfinite(clean).all() and same_bits(twelve[:20], clean[:20]) and same_bits(twelve[40:], clean[40:])


@pytest.mark.gpu
def test_weights_changed_in_place_reach_the_next_call():
    d = to_device(make_batch(2, 20, 2, seed=2305))
    m = fused_model(2)
    check_view(m, d, 40, 12)
    first = run_model(m, d)
    assert same_bits(run_model(m, d), first)                 # the second call reuses the prepared weights
    params = dict(m.named_parameters())
    with torch.no_grad():
        params["field_net.net.2.weight"].mul_(1.25)
        params["gnn.layer_1.res.weight"].add_(0.03125)
    second = run_model(m, d)
    fresh = run_model(fused_model(2, sd={k: v.detach().cpu().clone() for k, v in m.state_dict().items()}), d)
    assert torch.isfinite(second).all() and same_bits(second, fresh) and not same_bits(second, first)
