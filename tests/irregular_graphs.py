"""Irregular graphs for the fused path: kNN scenes of mixed sizes and one-component multigraphs, at the node and edge
caps of a k_fused group and around its tile boundaries.  Test helper, not a test module.

Every function returns the `make_batch` dictionary (without `meta`) for D = 2 or 3: node states from
`make_batch(1, n, D, seed)`, `edge_attr` from `aether_amd.edges.prepare_edge_attr`, the edge list in one seeded random
order (so `perm` of the graph view is no identity and the edges of a receiver are not adjacent in the input).

GRAPHS: name -> (builder(D, seed), structure).  `structure` is what the graph is there for, asserted from the edge list
alone by tests/test_update_metric.py::test_irregular_graphs_have_their_structure: nodes, edges, maximum in-degree (and
the bound it has to exceed), nodes without in-edge, duplicated edges, component sizes in node order."""
from __future__ import annotations

import torch

from aether_amd.edges import prepare_edge_attr
from aether_amd.synthetic import make_batch

MIXED = (2, 12, 7, 3, 9, 5, 11, 4)


def _finish(n, D, seed, send, recv):
    inp = {k: v for k, v in make_batch(1, n, D, seed=seed).items() if k != "meta"}
    order = torch.randperm(send.numel(), generator=torch.Generator().manual_seed(1000 + seed))
    send, recv = send[order].contiguous(), recv[order].contiguous()
    inp["edges"] = [send, recv]
    inp["edge_attr"] = prepare_edge_attr(inp["x"], inp["edges"], inp["charges"][send] * inp["charges"][recv])
    return inp


def knn_scenes(D, sizes, k, seed):
    """Consecutive scenes of `sizes` nodes; every node receives from its min(k, n - 1) nearest neighbours in its scene."""
    n_all = sum(sizes)
    x = make_batch(1, n_all, D, seed=seed)["x"]
    send, recv, base = [], [], 0
    for n in sizes:
        kk = min(k, n - 1)
        if kk > 0:
            d = torch.cdist(x[base:base + n].double(), x[base:base + n].double())
            d.fill_diagonal_(float("inf"))
            near = d.topk(kk, dim=1, largest=False).indices                 # [n, kk]: the senders of each receiver
            send.append(near.reshape(-1) + base)
            recv.append(torch.arange(n).repeat_interleave(kk) + base)
        base += n
    return _finish(n_all, D, seed, torch.cat(send), torch.cat(recv))


def multigraph(D, n, E, hub_in, seed):
    """One component on the first n - 2 nodes and two nodes without any edge.  Senders uniform in [0, n - 2), receivers
    uniform in [0, n - 3), the first `hub_in` edges all into node 0; no self loops (a drawn one takes the next sender).
    Node n - 3 only sends: with the two edge-less nodes, three nodes have no in-edge.  The topology is drawn under a
    seed of its own, from (n, E, hub_in) alone, so the graph view of a named graph does not move with the input seed;
    `seed` gives the node states and the order of the edge list."""
    g = torch.Generator().manual_seed(2000 + E + hub_in)
    send = torch.randint(0, n - 2, (E,), generator=g)
    recv = torch.randint(0, n - 3, (E,), generator=g)
    recv[:hub_in] = 0
    loop = send == recv
    send[loop] = (send[loop] + 1) % (n - 2)
    return _finish(n, D, seed, send, recv)


def _knn(sizes, k):
    return lambda D, seed: knn_scenes(D, sizes, k, seed)


def _multi(n, E, hub_in):
    return lambda D, seed: multigraph(D, n, E, hub_in, seed)


def _knn_structure(sizes, k):
    deg = [min(k, n - 1) for n in sizes]
    return dict(nodes=sum(sizes), edges=sum(n * d for n, d in zip(sizes, deg)), max_in=max(deg), max_in_above=0,
                no_in=0, duplicates=False, components=list(sizes))


def _multi_structure(n, E, hub_in, max_in, above):
    """`max_in`: the in-degree of node 0 as drawn; `above`: what the graph needs it to exceed."""
    return dict(nodes=n, edges=E, max_in=max_in, max_in_above=max(above, hub_in), no_in=3, duplicates=True,
                components=[n - 2, 1, 1])


GRAPHS = {
    "knn_mixed_k4": (_knn(MIXED, 4), _knn_structure(MIXED, 4)),
    "knn_mixed_k10": (_knn(MIXED, 10), _knn_structure(MIXED, 10)),
    "knn_2x24_k7": (_knn((24, 24), 7), _knn_structure((24, 24), 7)),
    "knn_2x30_k11": (_knn((30, 30), 11), _knn_structure((30, 30), 11)),
    "knn_32_k10": (_knn((32,), 10), _knn_structure((32,), 10)),
    "knn_2x32_k12": (_knn((32, 32), 12), _knn_structure((32, 32), 12)),
    "multi32_hub40": (_multi(32, 300, 40), _multi_structure(32, 300, 40, 46, 40)),
    "multi32_hub80": (_multi(32, 384, 80), _multi_structure(32, 384, 80, 86, 64)),
    "multi16_E170": (_multi(16, 170, 20), _multi_structure(16, 170, 20, 28, 16)),
    "multi16_E250": (_multi(16, 250, 20), _multi_structure(16, 250, 20, 38, 31)),
}


def build(name, D, seed):
    return GRAPHS[name][0](D, seed)


def structure(name):
    return GRAPHS[name][1]


def components(send, recv, n):
    """Sizes of the maximal node ranges that no edge crosses, in node order (the components the graph view packs)."""
    lo, hi = torch.minimum(send, recv), torch.maximum(send, recv)
    diff = torch.zeros(n + 1, dtype=torch.long)
    diff.index_add_(0, lo + 1, torch.ones_like(lo))
    diff.index_add_(0, hi + 1, -torch.ones_like(hi))
    cross = diff.cumsum(0)[:n]                              # cross[c]: edges with lo < c <= hi
    starts = [c for c in range(n) if c == 0 or cross[c] == 0] + [n]
    return [b - a for a, b in zip(starts, starts[1:])]
