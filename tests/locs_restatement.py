"""fp64 CPU restatement of LoCS (nn/state2state/locs/locs.py) from a state_dict.

Test helper, not a test module: tests/test_locs.py holds it to the fixtures of tools/make_golden_locs.py,
tests/test_gpu_locs.py holds the HIP path to it.  Written from the reference's equations on the primitives of
oracle/aether_oracle.py (frames, local-frame edge features, GNN layer, out MLP), not imported from the reference:

  R = frame(vel); rel_feat = [0, R^T vel]                                              (locs.py:31-38)
  edge j -> i: [R_i^T (x_j - x_i), Euler(R_i^T R_j), |x_j - x_i|, angles, R_i^T v_j]   (locs.py:40-85)
  edge_attr = [those, rel_feat[i], edge_attr_orig]                                     (locs.py:87-92, 124)
  h = 4 GNN layers on (rel_feat, edge_attr); out = x + R out_mlp(h)                    (locs.py:126-135)

Aether's local-frame edge features are LoCS's followed by the rotated forces, so the first 3D + D(D-1)/2 columns of
``aether_oracle.edge_features`` (with any field) are LoCS's.
"""
from __future__ import annotations

import torch
import torch.nn.functional as Fn

from oracle import aether_oracle as O


def forward(sd, x, vel, edges, edge_attr_orig, dropout_masks=None, return_all=False):
    """LoCS.forward; ``dropout_masks``: the two scale masks [n_nodes, hidden] of a train()-mode step, or None."""
    D = x.shape[-1]
    n_local = 3 * D + D * (D - 1) // 2
    send, recv = edges
    R = O.frame_from_velocity(vel)
    cv = O.apply_rot(R.transpose(-1, -2), vel)
    rel_feat = torch.cat([torch.zeros_like(cv), cv], -1)
    ext = torch.cat([x, vel, torch.zeros_like(x)], -1)
    ea_local = O.edge_features(ext, send, recv, D)[:, :n_local]
    e = torch.cat([ea_local, rel_feat[recv], edge_attr_orig], -1)
    h = rel_feat
    res = {"rel_feat": rel_feat, "R": R, "edge_attr": e}
    for k in range(1, 5):
        h, e = O.gnn_layer(sd, f"gnn.layer_{k}", h, e, send, recv, first=(k == 1))
        res[f"x{k}"] = h
    out = x + O.apply_rot(R, O.out_mlp(sd, h, dropout_masks))
    res["out"] = out
    return res if return_all else out


def grads(sd, x, vel, edges, edge_attr_orig, target, dropout_masks=None, inputs=False):
    """({key: d MSELoss(out, target) / d param}, {"x", "vel", "edge_attr": d loss / d input} if ``inputs``, loss)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    ins = [t.detach().clone().requires_grad_(inputs) for t in (x, vel, edge_attr_orig)]
    out = forward(leaves, ins[0], ins[1], edges, ins[2], dropout_masks)
    loss = Fn.mse_loss(out, target)
    wrt = list(leaves.values()) + (ins if inputs else [])
    g = torch.autograd.grad(loss, wrt)
    pg = dict(zip(leaves, g[:len(leaves)]))
    ig = dict(zip(("x", "vel", "edge_attr"), g[len(leaves):])) if inputs else None
    return pg, ig, loss.detach()


def rollout(sd, x, vel, edges, charges, steps, dt=1.0):
    """The protocol of aether_amd.rollout: x_{t+1} = LoCS(x_t, v_t), v_{t+1} = (x_{t+1} - x_t) / dt, with
    edge_attr = [q_i q_j, |x_i - x_j|] from the current positions (experiments/lorentz/main.py:236-241)."""
    rows, cols = edges
    qprod = charges[rows] * charges[cols]
    traj = []
    for _ in range(int(steps)):
        dist = torch.sqrt(torch.sum((x[rows] - x[cols]) ** 2, 1)).unsqueeze(1)
        xn = forward(sd, x, vel, edges, torch.cat([qprod, dist], 1))
        vel = (xn - x) / dt
        x = xn
        traj.append(x)
    return torch.stack(traj)
