"""k_fused reads every bias (and the last Linear's weights) from the per-layer constants block that k_prepare_weights
writes next to the weight images and that LDS-DMA delivers into one of two LDS slots with them.

Every test runs on the golden state dict with its 20 ``gnn.*.bias`` tensors replaced by ``0.5 * randn`` (generator seed
900 + D): with unit-scale, mutually distinct biases a block read from the wrong layer, slot or offset moves the output
by 0.15-0.3 of its scale.  Bars are the project's scale-relative ones against the fp64 oracle: 1e-5 forward, 5e-5
gradients.  Checked on the CPU at the shapes and seeds below: the fp32 oracle's forward stays <= 1.1e-7 from the fp64
oracle, and its gradients (the two gradient shapes) <= 7e-7, far inside a quarter of the gradient bar (1.25e-5), so the
amplitude 0.5 stands."""
import functools

import pytest
import torch

from conftest import load_state_dict, scale_rel_err
from aether_amd import _lib
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O
from fused_cases import KERNELS, fused_model, oracle_of, run_model, to_device

pytestmark = pytest.mark.gpu
TOL = 1e-5
GTOL = 5e-5
# (D, N, B): split pairs with one node tile, two rounds (2-D, 3-D); one round; three rounds with two node tiles, unsplit;
# split pairs with fewer than 16 tiles
SHAPES = [(2, 20, 2), (3, 20, 2), (2, 5, 3), (2, 18, 130), (2, 12, 2)]
STALE_KEYS = ("gnn.layer_3.update_fn.2.bias", "gnn.out_mlp.3.bias")


@functools.lru_cache(maxsize=None)
def _state_dict(D):
    sd = load_state_dict(D)
    gen = torch.Generator().manual_seed(900 + D)
    biases = sorted(k for k in sd if k.startswith("gnn.") and k.endswith(".bias"))
    assert len(biases) == 20, biases
    for k in biases:
        sd[k] = 0.5 * torch.randn(sd[k].shape, generator=gen)
    return sd


@functools.lru_cache(maxsize=None)
def _batch(D, N, B):
    return make_batch(B, N, D, seed=910 + N + D)


@functools.lru_cache(maxsize=None)
def _oracle64(D, N, B):
    return oracle_of(_state_dict(D), _batch(D, N, B))


def _model(D, flags):
    return fused_model(D, flags, _state_dict(D))


def _args(inp, dev="cuda"):
    return (inp["h"].to(dev), inp["x"].to(dev), [e.to(dev) for e in inp["edges"]], inp["vel"].to(dev),
            inp["edge_attr"].to(dev), inp["charges"].to(dev))


def _info(m, inp):
    return m.prepare_graph([e.to("cuda") for e in inp["edges"]], inp["x"].shape[0])[1]


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("D,N,B", SHAPES)
def test_forward_matches_oracle(D, N, B, kernel):
    inp = _batch(D, N, B)
    m = _model(D, KERNELS[kernel])
    info = _info(m, inp)
    tiles = (info.max_group_edges + 15) // 16
    if N == 20:
        assert info.n_groups == 2 * B and tiles == 12, (info.n_groups, info.max_group_edges)
    elif N == 5:         # the one-round kernel
        assert tiles <= 8, (info.n_groups, info.max_group_edges)
    elif N == 18:
        assert info.n_groups == B and tiles == 20, (info.n_groups, info.max_group_edges)
    else:
        assert info.n_groups == 2 * B and tiles < 16, (info.n_groups, info.max_group_edges)
    out = run_model(m, to_device(inp))
    err = scale_rel_err(out.double(), _oracle64(D, N, B))
    print(f"D={D} N={N} B={B} {kernel}: groups={info.n_groups} tiles={tiles} err={err:.2e}")
    assert torch.isfinite(out).all() and err <= TOL, err


@pytest.mark.parametrize("D,N,B", [(2, 20, 2), (2, 5, 3)])
def test_training_forward_and_gradients(D, N, B):
    inp = _batch(D, N, B)
    sdg = {k: v.clone().requires_grad_(True) for k, v in _state_dict(D).items()}
    want = O.aether_forward(sdg, inp["x"], inp["vel"], inp["edges"], inp["edge_attr"], inp["charges"])
    torch.nn.functional.mse_loss(want, inp["target"]).backward()
    m = _model(D, _lib.FLAG_FORCE_FUSED)
    m.zero_grad(set_to_none=True)
    out = m(*_args(inp))
    torch.nn.functional.mse_loss(out, inp["target"].to("cuda")).backward()
    torch.cuda.synchronize()
    err = scale_rel_err(out.detach().cpu().double(), _oracle64(D, N, B))
    print(f"D={D} N={N} B={B} training forward err={err:.2e}")
    assert err <= TOL, err
    worst = max((scale_rel_err(p.grad.detach().cpu(), sdg[k].grad), k) for k, p in m.named_parameters())
    print(f"D={D} N={N} B={B} worst gradient err={worst[0]:.2e} ({worst[1]})")
    for k, p in m.named_parameters():
        assert scale_rel_err(p.grad.detach().cpu(), sdg[k].grad) <= GTOL, k


@pytest.mark.parametrize("how", ["in_place", "load_state_dict"])
def test_changed_biases_reach_the_next_call(how):
    """The blocks belong to a weight version like the images: a second eval call on the same module, graph and workspace
    after two biases changed (layer 3's block; layer 4's block, which the out MLP reads) must not see the old blocks."""
    D, N, B = 2, 20, 2
    inp = _batch(D, N, B)
    m = _model(D, KERNELS["inference"]).eval()
    first = run_model(m, to_device(inp))
    assert scale_rel_err(first.double(), _oracle64(D, N, B)) <= TOL
    sd2 = {k: v.clone() for k, v in _state_dict(D).items()}
    for k in STALE_KEYS:
        sd2[k] += 0.3
    if how == "in_place":
        params = dict(m.named_parameters())
        with torch.no_grad():
            for k in STALE_KEYS:
                params[k].add_(0.3)
    else:
        m.load_state_dict(sd2)
    second = run_model(m, to_device(inp))
    want = oracle_of(sd2, inp)
    moved = scale_rel_err(want, _oracle64(D, N, B))
    err = scale_rel_err(second.double(), want)
    print(f"{how}: the new biases move the oracle by {moved:.2e}; err={err:.2e}")
    assert moved > 100 * TOL          # (the change is visible at all)
    assert err <= TOL, err


def test_rollout_redelivers_the_blocks_every_launch():
    """rollout(steps=3) prepares the blocks once and launches three times, each launch copying blocks 1-4 into the two
    slots again: bit for bit the three single calls -- rollout(steps=1), which derives the edge attributes in the kernel
    like every step of the long one (a module forward takes them from torch ops, a different rounding by design) --
    chained with the velocity of the protocol at dt = 1, (x' - x) / 1."""
    D, N, B = 2, 20, 2
    inp = make_batch(B, N, D, seed=930, device="cuda")
    m = _model(D, KERNELS["inference"]).eval()
    traj = m.rollout(inp["x"], inp["vel"], inp["edges"], inp["charges"], 3)
    x, vel = inp["x"], inp["vel"]
    for t in range(3):
        xn = m.rollout(x, vel, inp["edges"], inp["charges"], 1)[0]
        assert torch.equal(xn, traj[t]), t
        vel = (xn - x) / 1.0
        x = xn
    torch.cuda.synchronize()
    assert torch.isfinite(traj).all()


def test_twenty_calls_are_bit_equal():
    D, N, B = 2, 20, 2
    inp = _batch(D, N, B)
    m = _model(D, KERNELS["inference"])
    first = run_model(m, to_device(inp))
    assert scale_rel_err(first.double(), _oracle64(D, N, B)) <= TOL
    for _ in range(19):
        assert torch.equal(run_model(m, to_device(inp)), first)
