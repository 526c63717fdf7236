"""k_fused at the shapes where a workgroup's waves own different numbers of edge tiles (split groups, two-tile and
one-tile waves side by side, partial last tiles, absent second tiles) and where the node phase's step 3 runs on waves
4-7 (one node tile per workgroup).  Inference and save-for-backward kernels against the fp64 oracle at the project's
scale-relative bars: 1e-5 forward, 5e-5 gradients."""
import pytest
import torch

from conftest import load_state_dict, scale_rel_err
from aether_amd import _lib
from aether_amd.edges import prepare_edge_attr
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O
from fused_cases import KERNELS, fused_model, oracle_of, run_model, tiles_of, to_device

pytestmark = pytest.mark.gpu
TOL = 1e-5
GTOL = 5e-5


def _info(m, inp):
    return m.prepare_graph([e.to("cuda") for e in inp["edges"]], inp["x"].shape[0])[1]


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("D,N,B", [(2, 20, 2), (3, 20, 2), (2, 17, 2), (2, 18, 2), (2, 12, 2)])
def test_split_groups_match_oracle(D, N, B, kernel):
    inp = make_batch(B, N, D, seed=700 + N + D)
    m = fused_model(D, KERNELS[kernel])
    info = _info(m, inp)
    if N == 20:      # each graph over two workgroups of 10 nodes, 190 in-edges = 12 tiles: waves 0-3 own two, waves 4-7 one
        assert info.n_groups == 2 * B and tiles_of(info) == 12, (info.n_groups, info.max_group_edges)
    elif N in (17, 18):   # split 9 / 8 (9 / 9): 9 * (N - 1) in-edges, a partial last tile, two tiles on the first waves only
        assert info.n_groups == 2 * B and 8 < tiles_of(info) <= 16, (info.n_groups, info.max_group_edges)
    else:            # second tile absent on every wave or on some: one round only, or fewer than 16 tiles
        assert tiles_of(info) < 16, info.max_group_edges
    out = run_model(m, to_device(inp))
    err = scale_rel_err(out.double(), oracle_of(load_state_dict(D), inp))
    print(f"D={D} N={N} B={B} {kernel}: groups={info.n_groups} tiles={tiles_of(info)} err={err:.2e}")
    assert torch.isfinite(out).all() and err <= TOL, err


@pytest.mark.parametrize("N,B", [(5, 3), (18, 130), (32, 1)])
def test_one_and_three_round_kernels_unchanged_and_stable(N, B):
    """Unsplit groups: one round of tiles (N = 5), three rounds (N = 18 in a batch large enough that no graph is split:
    306 in-edges, 20 tiles); N = 32 has more edges than a fused group holds and goes wherever the dispatch sends it."""
    D = 2
    inp = make_batch(B, N, D, seed=720 + N)
    m = fused_model(D, KERNELS["inference"] if N < 32 else 0)
    info = _info(m, inp)
    if N == 5:
        assert tiles_of(info) <= 8, info.max_group_edges
    elif N == 18:
        assert info.n_groups == B and tiles_of(info) == 20, (info.n_groups, info.max_group_edges)
    a, b = run_model(m, to_device(inp)), run_model(m, to_device(inp))
    assert torch.equal(a, b)
    assert scale_rel_err(a.double(), oracle_of(load_state_dict(D), inp)) <= TOL


def test_tiles_of_one_wave_in_different_ranges():
    """Graph 0 scaled by 3e4, graph 1 by 1e-5, graph 2 as it is: the per-wave range decision of the split GEMMs differs from
    workgroup to workgroup, and inside a workgroup between a wave's tiles where their magnitudes differ."""
    D, N, B = 2, 20, 3
    inp = make_batch(B, N, D, seed=741)
    s = torch.ones(B * N, 1)
    s[:N] = 3e4
    s[N:2 * N] = 1e-5
    inp["x"] = inp["x"] * s
    inp["vel"] = inp["vel"] * s
    rows, cols = inp["edges"]
    inp["edge_attr"] = prepare_edge_attr(inp["x"], inp["edges"], inp["charges"][rows] * inp["charges"][cols])
    sd = load_state_dict(D)
    want = oracle_of(load_state_dict(D), inp)
    want32 = O.aether_forward(sd, inp["x"], inp["vel"], inp["edges"], inp["edge_attr"], inp["charges"])
    for kernel, flags in KERNELS.items():
        out = run_model(fused_model(D, flags), to_device(inp))
        assert torch.isfinite(out).all()
        for g in range(B):       # per graph: each has its own scale
            sl = slice(g * N, (g + 1) * N)
            err = scale_rel_err(out[sl].double(), want[sl])
            floor = scale_rel_err(want32[sl].double(), want[sl])
            assert err <= max(TOL, 4.0 * floor), (kernel, g, err, floor)


def test_twenty_calls_are_bit_equal():
    D = 2
    inp = make_batch(2, 20, D, seed=760)
    m = fused_model(D, KERNELS["inference"])
    first = run_model(m, to_device(inp))
    for _ in range(19):
        assert torch.equal(run_model(m, to_device(inp)), first)


def test_training_forward_and_gradients_split_groups():
    D = 2
    inp = make_batch(2, 20, D, seed=780)
    sdg = {k: v.clone().requires_grad_(True) for k, v in load_state_dict(D).items()}
    want = O.aether_forward(sdg, inp["x"], inp["vel"], inp["edges"], inp["edge_attr"], inp["charges"])
    torch.nn.functional.mse_loss(want, inp["target"]).backward()
    m = fused_model(D, _lib.FLAG_FORCE_FUSED)
    m.zero_grad(set_to_none=True)
    dev = "cuda"
    out = m(inp["h"].to(dev), inp["x"].to(dev), [e.to(dev) for e in inp["edges"]], inp["vel"].to(dev),
            inp["edge_attr"].to(dev), inp["charges"].to(dev))
    torch.nn.functional.mse_loss(out, inp["target"].to(dev)).backward()
    torch.cuda.synchronize()
    assert scale_rel_err(out.detach().cpu().double(), oracle_of(load_state_dict(D), inp)) <= TOL
    for k, p in m.named_parameters():
        assert scale_rel_err(p.grad.detach().cpu(), sdg[k].grad) <= GTOL, k
