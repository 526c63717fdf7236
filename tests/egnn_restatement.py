"""fp64 CPU restatement of EGNN_vel_Aether (nn/state2state/egnn_aether.py with gcl.py / egnn/gcl.py) from a state_dict.

Test helper, not a test module: tests/test_egnn_aether.py holds it to the fixtures of tools/make_golden_egnn_aether.py,
tests/test_gpu_egnn_aether.py holds the HIP kernels to it.  Written from the reference's equations, not imported from it:

  f = field_net(cat(x, vel), charges); h = embedding(h)
  per layer, row, col = edges, every sum / mean over row:
    d = x[row] - x[col]; r = |d|^2; norm_diff: d /= sqrt(r) + 1
    m = SiLU(W2 SiLU(W1 [h[row], h[col], r, edge_attr, f[row], f[col]] + b1) + b2)
    x = x + mean_row(clamp(d * phi(m), -100, 100)) + psi([h, f]) * vel      (psi on the layer's input h)
    h = h + node_mlp([h, sum_row(m)])
"""
from __future__ import annotations

import torch
import torch.nn.functional as Fn


def _lin(sd, key, v):
    b = sd.get(key + ".bias")
    return Fn.linear(v, sd[key + ".weight"], b)


def field(sd, x, vel, charges):
    emb = sd["field_net.class_embedding.weight"][(charges.reshape(-1) + 1).long()]
    z = torch.cat([x, vel, emb], -1)
    z = Fn.silu(_lin(sd, "field_net.net.0", z))
    z = Fn.silu(_lin(sd, "field_net.net.2", z))
    return _lin(sd, "field_net.net.4", z)


def forward(sd, h, x, edges, vel, edge_attr, charges, n_layers, norm_diff=False, tanh=False):
    """(out, [h_0 .. h_L], [x_0 .. x_L]) in the dtype of the state_dict's tensors.  The caller's x is not modified."""
    row, col = edges
    n = x.shape[0]
    f = field(sd, x, vel, charges)
    h = _lin(sd, "embedding", h)
    hs, xs = [h], [x]
    cnt = torch.zeros(n, dtype=x.dtype, device=x.device).index_add_(0, row, torch.ones_like(row, dtype=x.dtype)).clamp(min=1)
    for l in range(n_layers):
        p = f"gcl_{l}."
        d = x[row] - x[col]
        r = (d ** 2).sum(1, keepdim=True)
        if norm_diff:
            d = d / (torch.sqrt(r) + 1)
        e_in = torch.cat([h[row], h[col], r, edge_attr, f[row], f[col]], 1)
        m = Fn.silu(_lin(sd, p + "edge_mlp.2", Fn.silu(_lin(sd, p + "edge_mlp.0", e_in))))
        phi = Fn.linear(Fn.silu(_lin(sd, p + "coord_mlp.0", m)), sd[p + "coord_mlp.2.weight"])
        if tanh:
            phi = torch.tanh(phi)
        t = torch.clamp(d * phi, min=-100, max=100)
        x = x + torch.zeros_like(x).index_add_(0, row, t) / cnt[:, None]
        psi = _lin(sd, p + "coord_mlp_vel.2", Fn.silu(_lin(sd, p + "coord_mlp_vel.0", torch.cat([h, f], 1))))
        x = x + psi * vel
        agg = torch.zeros(n, h.shape[1], dtype=h.dtype, device=h.device).index_add_(0, row, m)
        h = h + _lin(sd, p + "node_mlp.2", Fn.silu(_lin(sd, p + "node_mlp.0", torch.cat([h, agg], 1))))
        hs.append(h)
        xs.append(x)
    return x, hs, xs


def grads(sd, h, x, edges, vel, edge_attr, charges, target, n_layers, norm_diff=False, tanh=False):
    """{key: d MSELoss(out, target) / d param} for every tensor of sd (the runner's loss, main.py:86,288)."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    out, _, _ = forward(leaves, h, x, edges, vel, edge_attr, charges, n_layers, norm_diff, tanh)
    loss = Fn.mse_loss(out, target)
    g = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    # the last layer's node_mlp does not reach the output: zeros, as the kernels write them
    return {k: (v if v is not None else torch.zeros_like(sd[k])) for k, v in zip(leaves, g)}, loss.detach()


def runner_batch(B, N, seed, pos_scale=1.0, dtype=torch.float32):
    """Inputs the way experiments/lorentz/main.py:204-259 builds them for --model egnn_aether: fully connected graphs
    without self loops (dataset get_edges: rows + N i), h = |vel|, edge_attr = [q_row q_col, |x_row - x_col|^2]."""
    g = torch.Generator().manual_seed(seed)
    loc = torch.randn(B * N, 3, generator=g, dtype=torch.float64) * pos_scale
    vel = torch.randn(B * N, 3, generator=g, dtype=torch.float64)
    charges = (torch.randint(0, 2, (B * N, 1), generator=g) * 2 - 1).to(torch.float64)
    loc_end = loc + 0.1 * torch.randn(B * N, 3, generator=g, dtype=torch.float64) * pos_scale
    r1 = [i for i in range(N) for j in range(N) if i != j]
    c1 = [j for i in range(N) for j in range(N) if i != j]
    rows = torch.cat([torch.tensor(r1, dtype=torch.int64) + N * b for b in range(B)])
    cols = torch.cat([torch.tensor(c1, dtype=torch.int64) + N * b for b in range(B)])
    loc, vel, charges, loc_end = (t.to(dtype) for t in (loc, vel, charges, loc_end))
    ea = charges[rows] * charges[cols]
    loc_dist = torch.sum((loc[rows] - loc[cols]) ** 2, 1).unsqueeze(1)
    edge_attr = torch.cat([ea, loc_dist], 1)
    h = torch.sqrt(torch.sum(vel ** 2, dim=1)).unsqueeze(1)
    return dict(h=h, x=loc, edges=[rows, cols], vel=vel, edge_attr=edge_attr, charges=charges, target=loc_end)
