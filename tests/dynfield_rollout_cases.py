"""Inputs and fp64 / fp32 reference gradients of the dynamic-field rollout-training tests (test helper, not a test module).

Reference: torch.autograd through ``rollout`` below, the protocol of ``oracle.aether_oracle.rollout`` restated over
``oracle.aether_oracle.dynamic_field_aether_forward`` (the latent field recomputed from the current state every step).
Model: ``torch.manual_seed(1); DynamicFieldAether(2D, H, 0.0, D)``; inputs ``make_batch(B, N, D, seed)``; targets, loss and
bound as in tests/rollout_train_cases.py (``reference``, ``step_loss``, ``GTOL``).  Every reference is computed once per
process and shared.
"""
from __future__ import annotations

import functools

import torch

from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O
from rollout_train_cases import GTOL, reference, step_loss  # noqa: F401  (re-exported)

# (H, B, N, K, dt, seed)
SHAPES = [(64, 3, 5, 4, 1.0, 3), (64, 2, 20, 3, 0.5, 4), (64, 2, 2, 4, 1.0, 5), (64, 5, 7, 6, 1.0, 6)]
TWO_STEPS = (64, 3, 5, 2, 0.5, 8)
# one shape per group layout of the fused kernels (tests/rollout_train_cases.py::LAYOUT_SHAPES)
LAYOUT_SHAPES = {"one_node_tile": (64, 130, 5, 2, 1.0, 203), "two_tile_waves": (64, 3, 13, 2, 1.0, 220),
                 "split": (64, 16, 20, 2, 1.0, 212)}
NARROW = [(20, 3, 5, 4, 1.0, 3), (32, 2, 5, 3, 1.0, 7)]
ALL_CASES = SHAPES + [TWO_STEPS] + list(LAYOUT_SHAPES.values()) + NARROW
# softmax is shift invariant: the gradient of the gate's last bias is exactly zero (tests/test_gpu_dynfield.py)
ZERO_GRAD = "field_net.summary_net.summary_net.gate_nn.2.bias"


@functools.lru_cache(maxsize=None)
def state_dict(D, H=64):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1)
        m = DynamicFieldAether(2 * D, H, 0.0, D, device="cpu")
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def rollout(sd, x, vel, edges, charges, steps, dt, num_nodes, with_margin=False):
    """x_{t+1} = DynamicFieldAether(x_t, v_t, ea_t), ea_t = [q_i q_j, |x_i - x_j|] from x_t, v_{t+1} = (x_{t+1} - x_t) / dt.
    ``with_margin``: also ``[steps, E]``, every edge's distance from a branch cut (``oracle.aether_oracle.cut_margin``)."""
    rows, cols = edges
    qprod = charges[rows] * charges[cols]
    D = x.shape[-1]
    traj, margins = [], []
    for _ in range(steps):
        dist = torch.sqrt(torch.sum((x[rows] - x[cols]) ** 2, 1)).unsqueeze(1)
        r = O.dynamic_field_aether_forward(sd, x, vel, edges, torch.cat([qprod, dist], 1), charges, num_nodes, return_all=True)
        if with_margin:
            margins.append(O.cut_margin(r["edge_attr_local"], D))
        xn = r["out"]
        vel = (xn - x) / dt
        x = xn
        traj.append(x)
    if with_margin:
        return torch.stack(traj), torch.stack(margins)
    return torch.stack(traj)


@functools.lru_cache(maxsize=None)
def case(D, H, B, N, K, dt, seed):
    """``rollout_train_cases.reference`` of ``rollout`` on ``make_batch(B, N, D, seed)`` + the smallest cut margin of the
    fp64 rollout + the model's state_dict."""
    sd = state_dict(D, H)
    inp = make_batch(B, N, D, seed=seed)
    fn = lambda sd_, x, v, e, q, steps, dt_: rollout(sd_, x, v, e, q, steps, dt_, N)
    with torch.no_grad():
        _, margins = rollout({k: v.double() for k, v in sd.items()}, inp["x"].double(), inp["vel"].double(), inp["edges"],
                             inp["charges"].double(), K, dt, N, with_margin=True)
    return dict(reference(fn, sd, inp, K, dt, seed), margin=float(margins.min()), sd=sd, num_nodes=N)
