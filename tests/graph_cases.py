"""Input sets on graphs the Lorentz runner never builds, for ClofNet and EGNN-Aether.

Test helper, not a test module: tools/make_golden_clof.py and tools/make_golden_egnn_aether.py build their multigraph and
in_node_nf = 3 fixtures from it, tests/test_gpu_clof_shapes.py and tests/test_gpu_egnn_aether_shapes.py their inputs.
Every function returns the dictionary of tests/egnn_restatement.py::runner_batch (h, x, edges, vel, edge_attr, charges,
target), edge_attr = [q_row q_col, |x_row - x_col|^2] as the runner computes it, in fp64 unless told otherwise.
"""
from __future__ import annotations

import torch


def _nodes(n, seed, pos_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, generator=g, dtype=torch.float64) * pos_scale
    vel = torch.randn(n, 3, generator=g, dtype=torch.float64)
    q = (torch.randint(0, 2, (n, 1), generator=g) * 2 - 1).to(torch.float64)
    target = x + 0.1 * torch.randn(n, 3, generator=g, dtype=torch.float64) * pos_scale
    return g, x, vel, q, target


def _batch(x, vel, q, target, row, col, in_nf=1, dtype=torch.float64):
    row, col = row.to(torch.int64), col.to(torch.int64)
    ea = torch.cat([q[row] * q[col], ((x[row] - x[col]) ** 2).sum(1, keepdim=True)], 1)
    h = wide_h(vel, q, x, in_nf)
    f = lambda t: t.to(dtype)
    return dict(h=f(h), x=f(x), edges=[row, col], vel=f(vel), edge_attr=f(ea), charges=f(q), target=f(target))


def wide_h(vel, q, x, in_nf):
    """Node features of width in_nf: |vel|, then the charge, |x|, and further columns cos(k |vel|) past three."""
    cols = [vel.norm(dim=1, keepdim=True), q.reshape(-1, 1).to(vel.dtype), x.norm(dim=1, keepdim=True)]
    cols += [torch.cos((k + 1) * cols[0]) for k in range(max(in_nf - 3, 0))]
    return torch.cat(cols[:in_nf], 1)


def with_wide_h(inp, in_nf):
    """The runner's batch with h = [|vel|, q, |x|, ...] in place of |vel|."""
    return dict(inp, h=wide_h(inp["vel"], inp["charges"], inp["x"], in_nf).to(inp["h"].dtype))


def without_edges(inp):
    e = torch.zeros(0, dtype=torch.int64)
    return dict(inp, edges=[e, e.clone()], edge_attr=inp["edge_attr"][:0].clone())


def random_multigraph(B, N, seed, self_loop=False, in_nf=1, dtype=torch.float64):
    """B graphs of N nodes with different edge counts, no edge between graphs.  In every graph node N-1 has no edge at
    all, node N-2 is no edge's row, node N-3 is no edge's col; some edges occur two or three times; the first graph has
    one self loop when asked to; the edge list is one random permutation over the whole batch (rows in random order)."""
    assert N >= 5
    g, x, vel, q, target = _nodes(B * N, seed)
    rows, cols = [], []
    for b in range(B):
        E = int(torch.randint(N, 3 * N + 1, (1,), generator=g)) + b
        r = torch.randint(0, N - 2, (E,), generator=g)                       # never N-2, N-1
        c = torch.randint(0, N - 2, (E,), generator=g)
        c = torch.where(c == N - 3, torch.full_like(c, N - 2), c)            # never N-3, N-1; N-2 receives
        c = torch.where(c == r, (c + 1) % (N - 3), c)                        # no self loop by accident
        n_dup = 2 + b % 2
        r = torch.cat([r, r[:n_dup], r[:1]])
        c = torch.cat([c, c[:n_dup], c[:1]])                                 # edge 0 three times, 1 .. n_dup-1 twice
        if self_loop and b == 0:
            r = torch.cat([r, torch.tensor([1])])
            c = torch.cat([c, torch.tensor([1])])
        rows.append(r + b * N)
        cols.append(c + b * N)
    row, col = torch.cat(rows), torch.cat(cols)
    p = torch.randperm(row.numel(), generator=g)
    return _batch(x, vel, q, target, row[p], col[p], in_nf, dtype)


def hub_graph(N, hub, seed, dtype=torch.float64):
    """One graph of N nodes: node `hub` is the row of an edge to every other node and the col of an edge from every other
    node (degree N-1, everyone else degree 1), then nodes with 1, 2 and 4 further edges (degrees 2, 3 and 5) and N // 2
    random edges among the rest (no duplicate of these, no self loop), in random order."""
    g, x, vel, q, target = _nodes(N, seed)
    others = torch.tensor([i for i in range(N) if i != hub])
    row = [torch.full((N - 1,), hub), others]
    col = [others, torch.full((N - 1,), hub)]
    special = {int(others[5]): 1, int(others[6]): 2, int(others[7]): 4}      # extra row edges -> degrees 2, 3, 5
    for node, extra in special.items():
        peers = [int(others[20 + k]) for k in range(extra)]
        row.append(torch.full((extra,), node))
        col.append(torch.tensor(peers))
    free = others[30:]
    k = N // 2
    r = free[torch.randint(0, free.numel(), (k,), generator=g)]
    c = others[torch.randint(0, others.numel(), (k,), generator=g)]
    keep = r != c
    row.append(r[keep])
    col.append(c[keep])
    row, col = torch.cat(row), torch.cat(col)
    p = torch.randperm(row.numel(), generator=g)
    return _batch(x, vel, q, target, row[p], col[p], 1, dtype), special


def degrees(inp):
    n = inp["x"].shape[0]
    return torch.zeros(n, dtype=torch.int64).index_add_(0, inp["edges"][0], torch.ones_like(inp["edges"][0]))


def thinned_complete(B, N, E, seed, dtype=torch.float64):
    """B complete graphs of N nodes (the runner's batch) with edges dropped at random until exactly E are left, in the
    runner's order."""
    from egnn_restatement import runner_batch
    inp = runner_batch(B, N, seed, dtype=torch.float64)
    full = inp["edges"][0].numel()
    assert 0 <= E <= full, (E, full)
    g = torch.Generator().manual_seed(seed + 7919)
    keep = torch.randperm(full, generator=g)[:E].sort().values
    out = dict(inp, edges=[inp["edges"][0][keep], inp["edges"][1][keep]], edge_attr=inp["edge_attr"][keep])
    return {k: (v if k == "edges" else v.to(dtype)) for k, v in out.items()}
