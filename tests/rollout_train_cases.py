"""Inputs and fp64 / fp32 reference gradients of the rollout-training tests (test helper, not a test module).

Reference: torch.autograd through ``oracle.aether_oracle.rollout``.  Model: ``torch.manual_seed(1); Aether(2D, 64, 0.0, D)``;
inputs ``make_batch(B, N, D, seed)``; targets = the fp64 oracle trajectory + 0.05 randn (generator seed ``seed + 100``);
loss = mean over the steps of the per-step MSE.  Every reference is computed once per process and shared.
"""
from __future__ import annotations

import functools

import torch

from aether_amd.nn.state2state.aether import Aether
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O

GTOL = 5e-5          # tests/test_gpu_backward.py
# (B, N, K, dt, seed)
SHAPES = [(3, 5, 4, 1.0, 3), (2, 20, 3, 0.5, 4), (2, 2, 4, 1.0, 5), (5, 7, 6, 1.0, 6)]


@functools.lru_cache(maxsize=None)
def state_dict(D):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        m = Aether(2 * D, 64, 0.0, D, device="cpu")
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def step_loss(traj, targets):
    """Mean over the steps of the per-step MSE."""
    return ((traj - targets) ** 2).mean(dim=(1, 2)).mean()


def rollout_grads(rollout_fn, sd, x, vel, edges, charges, targets, steps, dt, dtype):
    """Autograd through ``rollout_fn(sd, x, vel, edges, charges, steps, dt)`` in ``dtype`` ->
    ({parameter key | "x0" | "vel0": gradient}, trajectory)."""
    c = lambda t: t.detach().to(dtype)
    leaves = {k: c(v).requires_grad_(True) for k, v in sd.items()}
    x0, v0 = c(x).requires_grad_(True), c(vel).requires_grad_(True)
    traj = rollout_fn(leaves, x0, v0, edges, c(charges), steps, dt)
    step_loss(traj, c(targets)).backward()
    grads = {k: v.grad for k, v in leaves.items()}
    grads["x0"], grads["vel0"] = x0.grad, v0.grad
    return grads, traj.detach()


def reference(rollout_fn, sd, inp, K, dt, seed):
    """fp64 trajectory of ``rollout_fn``, targets = that + 0.05 randn (generator seed ``seed + 100``), and its autograd
    gradients in fp64 and fp32 -> dict(inp, targets, g64, g32, traj64, traj32)."""
    sd64 = {k: v.double() for k, v in sd.items()}
    with torch.no_grad():
        traj64 = rollout_fn(sd64, inp["x"].double(), inp["vel"].double(), inp["edges"], inp["charges"].double(), K, dt)
    g = torch.Generator().manual_seed(seed + 100)
    targets = traj64 + 0.05 * torch.randn(traj64.shape, generator=g, dtype=torch.float64)
    g64, _ = rollout_grads(rollout_fn, sd, inp["x"], inp["vel"], inp["edges"], inp["charges"], targets, K, dt, torch.float64)
    g32, traj32 = rollout_grads(rollout_fn, sd, inp["x"], inp["vel"], inp["edges"], inp["charges"], targets, K, dt, torch.float32)
    return dict(inp=inp, targets=targets, g64=g64, g32=g32, traj64=traj64, traj32=traj32)


def aether_margin(sd, inp, K, dt):
    """Smallest distance (radians) of any edge of any step of the fp64 oracle rollout from a branch cut of the feature map."""
    with torch.no_grad():
        _, margins = O.rollout({k: v.double() for k, v in sd.items()}, inp["x"].double(), inp["vel"].double(), inp["edges"],
                               inp["charges"].double(), K, dt, with_margin=True)
    return float(margins.min())


@functools.lru_cache(maxsize=None)
def case(D, B, N, K, dt, seed):
    """``reference`` of the oracle's rollout on ``make_batch(B, N, D, seed)`` + margin (``aether_margin``)."""
    sd = state_dict(D)
    inp = make_batch(B, N, D, seed=seed)
    return dict(reference(O.rollout, sd, inp, K, dt, seed), margin=aether_margin(sd, inp, K, dt))


# The further cases of tests/test_gpu_rollout_train.py (same model, same bound; tests/test_rollout_train_inputs.py holds
# their fp32 oracle error below GTOL as it does for SHAPES).
TWO_STEPS = (3, 5, 2, 0.5, 8)
# One shape per group layout of the fused kernels: one-node-tile workgroups; waves that own two edge tiles (156 edges per
# group; unsplit only above 128 groups, so the test builds this view with the fused_split option off instead of
# 130 graphs); groups split over two workgroups.  Seeds: the first tried whose fp64 reference keeps every edge 1e-4 rad
# from a branch cut (at 130 x 13 graphs, 40,000 edge-steps, hardly any seed does -- hence the small two-tile shape).
LAYOUT_SHAPES = {"one_node_tile": (130, 5, 2, 1.0, 203), "two_tile_waves": (3, 13, 2, 1.0, 220), "split": (16, 20, 2, 1.0, 212)}
MULTIGRAPH = (2, 1.0, 23)            # K, dt, seed


def multigraph_batch(seed, D):
    """The batch of test_gradients_on_random_multigraphs (components of 1..40 nodes, repeated edges, isolated nodes,
    nodes without in- or out-edges, unsorted) without its self loops: an edge whose end points coincide has no
    distance derivative -- undefined in the rollout protocol (include/aether_hip.h), NaN in the oracle's autograd."""
    from test_gpu_configs import _random_multigraph_batch
    inp = _random_multigraph_batch(seed, D)
    send, recv = inp["edges"]
    keep = send != recv
    assert int(keep.sum()) < send.numel()                        # (the generator did draw some)
    inp["edges"] = [send[keep].contiguous(), recv[keep].contiguous()]
    n = inp["x"].shape[0]
    deg_in = torch.bincount(inp["edges"][1], minlength=n)
    deg_out = torch.bincount(inp["edges"][0], minlength=n)
    assert int((deg_in == 0).sum()) and int((deg_out == 0).sum()) and int(((deg_in + deg_out) == 0).sum())
    pairs = inp["edges"][0] * n + inp["edges"][1]
    assert pairs.unique().numel() < pairs.numel()                # repeated edges
    return inp


@functools.lru_cache(maxsize=None)
def multigraph_case(D):
    K, dt, seed = MULTIGRAPH
    sd = state_dict(D)
    inp = multigraph_batch(seed, D)
    return dict(reference(O.rollout, sd, inp, K, dt, seed), margin=aether_margin(sd, inp, K, dt))


@functools.lru_cache(maxsize=None)
def locs_case(D, hidden):
    """LoCS(2D, hidden, 0.0, D) under torch.manual_seed(1) at SHAPES[0], against tests/locs_restatement.py::rollout
    -> (state_dict, ``reference``)."""
    import locs_restatement as LR
    from aether_amd.nn.state2state.locs import LoCS
    B, N, K, dt, seed = SHAPES[0]
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        m = LoCS(2 * D, hidden, 0.0, D, device="cpu")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return sd, reference(LR.rollout, sd, make_batch(B, N, D, seed=seed), K, dt, seed)
