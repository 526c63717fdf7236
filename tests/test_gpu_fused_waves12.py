"""k_fused<D, 12, 1, false>: twelve waves with one edge tile each, for inference on workgroups of 9-12 edge tiles and
one node tile (HISTORY R13).  The work moved between waves, the arithmetic did not: every shape is held
to the fp64 oracle at the project's scale-relative forward bar (1e-5) and must give the same bits with the option
`fused_waves12` off (the 8-wave kernels) and on.

Shapes, B = 2 throughout:
  (D 2 and 3, N 20)         split pairs, 10 + 10 nodes, 190 in-edges = 12 tiles: all twelve waves own a tile
  (2, 17), (2, 18)          split 9 + 8 / 9 + 9 nodes: 9 / 10 tiles, the last one partial; waves without a tile prefetch up front
  (2, 14), (2, 13) unsplit  182 / 156 in-edges = 12 / 10 tiles, n <= 16, no partner
  (2, 12) unsplit           132 in-edges = 9 tiles
  (2, 16)                   split 8 + 8 nodes, 120 in-edges = 8 tiles: stays on the 8-wave kernel (dispatch rule below)
"""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_state_dict, scale_rel_err
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O
from fused_cases import fused_model, oracle_of, run_model, set_option, tiles_of, to_device, uses_twelve_waves
from fused_cases import options_restored  # noqa: F401  (autouse fixture: applies to the tests of this file)

pytestmark = pytest.mark.gpu
TOL = 1e-5
B = 2
# (D, N, fused_split)
SHAPES = [(2, 20, 1), (3, 20, 1), (2, 17, 1), (2, 18, 1), (2, 14, 0), (2, 13, 0), (2, 12, 0), (2, 16, 1)]
TILES = {(20, 1): 12, (17, 1): 9, (18, 1): 10, (14, 0): 12, (13, 0): 10, (12, 0): 9, (16, 1): 8}


@functools.lru_cache(maxsize=None)
def _case(D, N):
    inp = make_batch(B, N, D, seed=1300 + 10 * N + D)
    return inp, oracle_of(load_state_dict(D), inp)


@pytest.mark.parametrize("D,N,split", SHAPES)
def test_matches_the_fp64_oracle_and_the_eight_wave_kernel(D, N, split):
    inp, want = _case(D, N)
    d = to_device(inp)
    m = fused_model(D)
    set_option(b"fused_split", split)                   # read when the graph view is built
    info = m.prepare_graph(d["edges"], B * N)[1]
    set_option(b"fused_split", 1)
    tiles = tiles_of(info)
    assert tiles == TILES[(N, split)] and info.max_group_nodes <= 16, (tiles, info.max_group_nodes)
    assert info.n_groups == (2 * B if split else B) and bool(info.reserved & 1) == bool(split)
    # 8 tiles stay on k_fused<D, 8, 1>; everything else here is in the 12-wave kernel's range
    assert uses_twelve_waves(info) == (N != 16), (tiles, info.max_group_nodes)
    set_option(b"fused_waves12", 0)
    eight = run_model(m, d)
    set_option(b"fused_waves12", 1)
    twelve = run_model(m, d)
    again = run_model(m, d)
    err = scale_rel_err(twelve.double(), want)
    print(f"D={D} N={N} split={split}: groups={info.n_groups} tiles={tiles} err={err:.2e}")
    assert torch.isfinite(twelve).all() and err <= TOL, err
    assert torch.equal(twelve, eight)
    assert torch.equal(again, twelve)                    # two calls on the same inputs


def test_rollout_of_three_steps_equals_three_single_steps():
    inp, _ = _case(2, 20)
    d = to_device(inp)
    m = fused_model(2)
    assert uses_twelve_waves(m.prepare_graph(d["edges"], B * 20)[1])
    whole = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    x, vel = d["x"], d["vel"]
    for t in range(3):
        nxt = m.rollout(x, vel, d["edges"], d["charges"], 1, 1.0)[0]
        assert torch.equal(nxt, whole[t]), t
        x, vel = nxt, (nxt - x) / 1.0          # the protocol's next velocity at dt = 1: one exact fp32 subtraction
    set_option(b"fused_waves12", 0)
    eight = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    torch.cuda.synchronize()
    assert torch.isfinite(whole).all() and torch.equal(whole, eight)


def test_dynamic_field_forward_matches_the_fp64_oracle():
    from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
    data = np.load(os.path.join(GOLDEN, "dynfield_D2.npz"))
    sd = {str(k): torch.from_numpy(data["sd." + str(k)]) for k in data["keys"]}
    inp = make_batch(B, 20, 2, seed=1208)
    with torch.no_grad():
        want = O.dynamic_field_aether_forward({k: v.double() for k, v in sd.items()}, inp["x"].double(), inp["vel"].double(),
                                              inp["edges"], inp["edge_attr"].double(), inp["charges"].double(), 20)
    m = DynamicFieldAether(4, 64, 0.0, 2, device="cuda")
    m.load_state_dict(sd)
    d = to_device(inp)

    def run():
        with torch.no_grad():
            out = m(None, d["x"], d["edges"], d["vel"], d["edge_attr"], d["charges"], 20)
        torch.cuda.synchronize()
        return out.cpu()

    twelve = run()
    set_option(b"fused_waves12", 0)
    eight = run()
    err = scale_rel_err(twelve.double(), want)
    print(f"dynamic field: err={err:.2e}")
    assert torch.isfinite(twelve).all() and err <= TOL, err
    assert torch.equal(twelve, eight)
