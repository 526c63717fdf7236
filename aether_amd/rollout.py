"""Autoregressive rollout of the state2state step (metric 2).

The reference's state2state module predicts positions only and has no rollout of its own; the
protocol used for the "20-step rollout MSE" figure is the one SURVEY.md defines and the oracle
restates (oracle/aether_oracle.py::rollout): x_{t+1} = Aether(x_t, v_t), v_{t+1} = (x_{t+1} - x_t) / dt,
with ``edge_attr = [q_i q_j, |x_i - x_j|]`` rebuilt from the current positions every step
(experiments/lorentz/main.py:243-246).  Everything stays on the device; the edge index (and therefore
the receiver-sorted graph view) is reused across steps.  ``rollout`` runs the loop inside the library
(``aether_rollout``); ``rollout_stepwise`` is the loop of module calls it replaces; ``rollout_loss`` trains through it (``differentiable_rollout``:
the k-step loss and its backward through time on the device).  ``EGNN_vel_Aether`` and ``ClofNet*`` have
the same ``rollout`` (``aether_egnn_rollout`` / ``aether_clof_rollout``) under the runner's preparation for them --
``nodes = |vel|`` and the squared distance in ``edge_attr``; their loop of module calls is ``rollout_stepwise_gnn``.
"""
from __future__ import annotations

import inspect

import torch


def rollout(model, x, vel, edges, charges, steps: int, dt: float = 1.0):
    """Predicted positions ``[steps, n_nodes, D]``: the device rollout (``aether_rollout``, one kernel
    launch per step, edge attributes derived in the kernels)."""
    return model.rollout(x, vel, edges, charges, steps, dt)


@torch.no_grad()
def rollout_stepwise(model, x, vel, edges, charges, steps: int, dt: float = 1.0):
    """The same protocol as a loop of module calls with the runner's tensor ops in between (how a
    reference user would write it; kept as the cross-check of ``rollout``)."""
    rows, cols = edges
    qprod = charges[rows] * charges[cols]
    traj = []
    for _ in range(int(steps)):
        dist = torch.sqrt(torch.sum((x[rows] - x[cols]) ** 2, 1)).unsqueeze(1)
        ea = torch.cat([qprod, dist], 1)
        h = vel.norm(dim=-1, keepdim=True)            # `nodes` of the runner; ignored by the model
        xn = model(h, x, edges, vel, ea, charges)
        vel = (xn - x) / dt
        x = xn
        traj.append(x)
    return torch.stack(traj)


@torch.no_grad()
def rollout_stepwise_gnn(model, x, vel, edges, charges, steps: int, dt: float = 1.0, **fwd_kwargs):
    """``rollout_stepwise`` for the drop-ins the Lorentz runner feeds ``nodes = |vel|`` and the SQUARED distance
    (``EGNN_vel_Aether``, ``ClofNet*``; experiments/lorentz/main.py:254-271): the loop of module calls that their
    ``rollout`` replaces, kept as its cross-check.  ``fwd_kwargs`` go to every forward (ClofNet's ``n_nodes``)."""
    rows, cols = edges
    q = charges.reshape(-1, 1)
    qprod = q[rows] * q[cols]
    takes_charges = "charges" in inspect.signature(model.forward).parameters       # ClofNet's forward takes none
    traj = []
    for _ in range(int(steps)):
        dist2 = torch.sum((x[rows] - x[cols]) ** 2, 1).unsqueeze(1)
        ea = torch.cat([qprod, dist2], 1)
        h = torch.sqrt(torch.sum(vel ** 2, dim=1)).unsqueeze(1)
        args = (h, x, edges, vel, ea) + ((charges,) if takes_charges else ())
        xn = model(*args, **fwd_kwargs)
        vel = (xn - x) / dt
        x = xn
        traj.append(x)
    return torch.stack(traj) if traj else x.new_empty(0, *x.shape)


def rollout_mse(pred, truth):
    """Per-step MSE over (sample, particle, feature), experiments/electrostatic/evaluate.py:61-70."""
    return ((pred - truth) ** 2).mean(dim=(1, 2))


class _MseLoss(torch.autograd.Function):
    """``aether_mse_loss_grad`` behind torch.autograd: loss and d(loss)/d(pred) in one launch."""

    @staticmethod
    def forward(ctx, pred, target):
        from .optim import mse_loss_grad
        loss, grad = mse_loss_grad(pred, target)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        return ctx.saved_tensors[0] * g, None


def rollout_loss(model, x, vel, edges, charges, targets, dt: float = 1.0, **rollout_kwargs):
    """The k-step ("push-forward") training loss: mean over all steps and elements of the squared error between the
    device rollout ``model.differentiable_rollout(x, vel, edges, charges, steps = targets.shape[0], dt)`` and
    ``targets [steps, n_nodes, D]`` (the positions at t = 1 .. steps).  ``.backward()`` runs the backward through time
    on the device; where a runner computes ``loss_mse(model(...), target)`` for one step, it calls this instead.
    ``rollout_kwargs`` go to ``differentiable_rollout`` (``DynamicFieldAether``: ``num_nodes``, the objects per graph)."""
    if targets.dim() != 3:
        raise ValueError("targets must be [steps, n_nodes, D]")
    traj = model.differentiable_rollout(x, vel, edges, charges, targets.shape[0], dt, **rollout_kwargs)
    if traj.shape != targets.shape:
        raise ValueError(f"targets must be {tuple(traj.shape)}, got {tuple(targets.shape)}")
    return _MseLoss.apply(traj.reshape(-1), targets.reshape(-1))
