"""fp64 CPU restatement of the ClofNet models (nn/state2state/clof/clof.py with clof/gcl.py, clof/layers.py and
egnn/gcl.py) from a state_dict.

Test helper, not a test module: tests/test_clof.py holds it to the fixtures of tools/make_golden_clof.py,
tests/test_gpu_clof.py holds the HIP kernels to it.  Written from the equations, not imported from the reference:

  h = embedding_node(h); x = x - centroid of each block of n_nodes rows
  frame(x): d = x[row] - x[col], r = |d|^2, c = x[row] x x[col] (per edge); norm_diff: d /= sqrt(r) + 1, c /= |c| + 1;
            v = d x c
  prologue (frame with norm_diff for the _vel variants, the argument for ClofNet):
    ci = [d, c, v] . x[row], cj = [d, c, v] . x[col] (+ vi, vj from vel); cos = ci . cj / (|ci| + 1e-5) / (|cj| + 1e-5);
    sin = sqrt(1 - cos^2);  e = fuse_edge([edge_attr?, sin, cos, ci, cj, (vi, vj)])  (+ gaussian(type, dist) for _gbf)
  per layer, sums and means over row:
    m = SiLU-MLP3([h[row], h[col], r, e]); t = clamp(d k0 + c k1 + v k2, -100, 100), k = coord_mlp(m)
    x = (x + mean_row(t) coords_weight) + coord_mlp_vel(h) vel
    u = h + (h + node_mlp([h, sum_row m]))   (recurrent; h + node_mlp(...) otherwise);  h = LayerNorm(u)
  out = x + centroid
"""
from __future__ import annotations

import torch
import torch.nn.functional as Fn

from egnn_restatement import runner_batch  # noqa: F401  (the runner's inputs; re-exported for the tests)

VARIANTS = {"clof": 0, "clof_vel": 1, "clof_vel_gbf": 2}


def _lin(sd, key, v):
    return Fn.linear(v, sd[key + ".weight"], sd.get(key + ".bias"))


def _cross(a, b):
    return torch.linalg.cross(a, b, dim=1)


def frame(x, row, col, norm):
    d = x[row] - x[col]
    r = (d ** 2).sum(1, keepdim=True)
    c = _cross(x[row], x[col])
    if norm:
        d = d / (torch.sqrt(r) + 1)
        c = c / (torch.sqrt((c ** 2).sum(1, keepdim=True)) + 1)
    return r, d, c, _cross(d, c)


def edge_features(sd, variant, x, vel, row, col, edge_attr, norm):
    """edge_feat of the prologue (fuse_edge output, + the Gaussian embedding for ClofNet_vel_gbf)."""
    _, d, c, v = frame(x, row, col, norm)
    basis = torch.stack([d, c, v], 1)                       # [E, 3, 3]
    proj = lambda p: torch.einsum("ebk,ek->eb", basis, p)
    ci, cj = proj(x[row]), proj(x[col])
    cos = (ci * cj).sum(1, keepdim=True) / (ci.norm(dim=1, keepdim=True) + 1e-5) / (cj.norm(dim=1, keepdim=True) + 1e-5)
    sin = torch.sqrt(1 - cos ** 2)
    parts = [sin, cos, ci, cj]
    if variant != 0:
        parts += [proj(vel[row]), proj(vel[col])]
    if variant != 2:
        parts = [edge_attr] + parts
    z = torch.cat(parts, 1)
    e = Fn.silu(_lin(sd, "fuse_edge.2", Fn.silu(_lin(sd, "fuse_edge.0", z))))
    if variant == 2:
        t = (edge_attr[:, 0] * 0.5 + 0.5).long()
        xg = sd["gbf.mul.weight"][t] * edge_attr[:, 1:2] + sd["gbf.bias.weight"][t]
        # the reference evaluates the Gaussian in fp32 whatever the model's dtype (x.float(), layers.py:28-31)
        xg = xg.float()
        mean = sd["gbf.means.weight"].float().view(-1)
        std = sd["gbf.stds.weight"].float().view(-1).abs() + 1e-5
        g = torch.exp(-0.5 * (((xg - mean) / std) ** 2)) / ((2 * 3.14159) ** 0.5 * std)
        e = e + g.to(e.dtype)
    return e


def forward(sd, variant, h, x, edges, vel, edge_attr, n_layers, n_nodes, norm_diff=True, tanh=False, recurrent=True,
            coords_weight=1.0):
    """(out, [h_0 .. h_L], [x_0 .. x_L]) in the dtype of the state_dict's tensors; x_l are centred.  The caller's x is not
    modified."""
    row, col = edges
    n = x.shape[0]
    h = _lin(sd, "embedding_node", h)
    xb = x.reshape(-1, n_nodes, 3)
    centroid = xb.mean(1, keepdim=True)
    x = (xb - centroid).reshape(-1, 3)
    e = edge_features(sd, variant, x, vel, row, col, edge_attr, norm_diff if variant == 0 else True)
    hs, xs = [h], [x]
    cnt = torch.zeros(n, dtype=x.dtype, device=x.device).index_add_(0, row, torch.ones_like(row, dtype=x.dtype)).clamp(min=1)
    for l in range(n_layers):
        p = f"gcl_{l}."
        r, d, c, v = frame(x, row, col, norm_diff)
        z = torch.cat([h[row], h[col], r, e], 1)
        for k in (0, 2, 4):
            z = Fn.silu(_lin(sd, p + f"edge_mlp.{k}", z))
        m = z
        k = Fn.linear(Fn.silu(_lin(sd, p + "coord_mlp.0", m)), sd[p + "coord_mlp.2.weight"])
        if tanh:
            k = torch.tanh(k)
        t = torch.clamp(d * k[:, :1] + c * k[:, 1:2] + v * k[:, 2:3], min=-100, max=100)
        x = x + (torch.zeros_like(x).index_add_(0, row, t) / cnt[:, None]) * coords_weight
        x = x + _lin(sd, p + "coord_mlp_vel.2", Fn.silu(_lin(sd, p + "coord_mlp_vel.0", h))) * vel
        agg = torch.zeros(n, h.shape[1], dtype=h.dtype, device=h.device).index_add_(0, row, m)
        o = _lin(sd, p + "node_mlp.2", Fn.silu(_lin(sd, p + "node_mlp.0", torch.cat([h, agg], 1))))
        u = h + (h + o) if recurrent else h + o
        h = Fn.layer_norm(u, (u.shape[1],), sd[p + "layer_norm.weight"], sd[p + "layer_norm.bias"], 1e-5)
        hs.append(h)
        xs.append(x)
    out = (x.reshape(-1, n_nodes, 3) + centroid).reshape(-1, 3)
    return out, hs, xs


def grads(sd, variant, h, x, edges, vel, edge_attr, target, n_layers, n_nodes, **kw):
    """({key: d MSELoss(out, target) / d param or None where the parameter does not reach the output}, loss)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    out, _, _ = forward(leaves, variant, h, x, edges, vel, edge_attr, n_layers, n_nodes, **kw)
    loss = Fn.mse_loss(out, target)
    g = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return dict(zip(leaves, g)), loss.detach()
