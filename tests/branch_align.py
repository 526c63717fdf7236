"""Branch-aligned oracle: hold the HIP step to the reference at inputs where the reference's own geometry sits on a branch
cut (test helper, imported by test modules; not a conftest).

Anti-parallel headings put the ZYX Euler columns atan2(.)/pi of an edge on their +-1 cut, and a sender exactly behind
its receiver puts the symmetric bearing on its +-pi cut (oracle.aether_oracle.cut_margin).  There a 1-ulp difference in a
rotation matrix picks the other side, and since every graph is fully connected one flipped edge moves every later stage of
its graph.  So the kernel's layer-1 edge features (debug name ``efeat``) are compared with the oracle's first, and on the
cut columns only the whole periods between them become a per-edge constant ``edge_shift`` of the oracle.  A shift is
accepted only where the edge lies within MARGIN of a cut in the fp32 or the fp64 evaluation; anywhere else a difference
is a bug, not a branch choice.  The shifted oracle is differentiable as before and its autograd gives the gradients of
the side the kernel took (the backward reads the stored features and picks no side of its own).

Errors are scale-relative per row block (``blocks``): the zero-velocity slope of d/dvel in 3-D is 1e4 times every other
entry, and measured over the whole tensor it would hide any other error.
"""
import math

import torch

from oracle import aether_oracle as O

FPAD = 32          # layer-1 feature columns of the kernels (csrc/common.h), zero beyond 7D + D(D-1)/2 + 2
MARGIN = 1e-3      # radians


def n_local(D):
    """Columns of edge_attr_local: [r | euler | dist | bearing | R^T v_j | R^T f_j | rel_feat[recv]]."""
    return 7 * D + D * (D - 1) // 2


def cut_columns(D):
    """(column, period) of the features with a branch cut; the columns cut_margin measures."""
    return [(2, 2.0), (4, 2 * math.pi)] if D == 2 else [(3, 2.0), (5, 2.0), (7, 2 * math.pi)]


def kernel_features(m, edges, n_nodes):
    """Layer-1 edge features [E, FPAD] of m's last forward (FLAG_KEEP_INTERMEDIATES), in the caller's edge order.  A
    model narrower than 64 runs its zero-padded 64-wide engine, which holds the workspace."""
    eng = m.__dict__.get("_engine", m)
    E = edges[0].numel()
    es = eng.debug_fetch("efeat", n_nodes, E, FPAD).cpu()
    perm = eng.graph_perm(edges, n_nodes).cpu()
    feat = torch.empty_like(es)
    feat[perm] = es
    return feat


def branch_shifts(feat, ea64, ea32, D):
    """Shifts that put the fp64 and the fp32 oracle's features on the kernel's side of every cut: (shift64, shift32,
    number of edges shifted against fp64).  Asserts that only edges within MARGIN of a cut move."""
    margin = torch.minimum(O.cut_margin(ea64.double(), D), O.cut_margin(ea32.double(), D))
    out = []
    for ea in (ea64, ea32):
        s = torch.zeros(ea.shape, dtype=torch.float64)
        for c, period in cut_columns(D):
            s[:, c] = period * torch.round((feat[:, c].double() - ea[:, c].double()) / period)
        moved = (s != 0).any(1)
        bad = moved & ~(margin < MARGIN)
        assert not bool(bad.any()), ("cut column differs by a period away from any cut", bad.nonzero().flatten().tolist(),
                                     margin[bad].tolist())
        out.append(s)
    return out[0], out[1], int((out[0] != 0).any(1).sum())


def run_oracle(sd, inp, dtype, shift=None, num_nodes=None, grads=True):
    """The oracle in ``dtype`` with the branch shift: every stage, and (grads) the autograd gradients of
    mse_loss(out, target) with respect to every parameter and to x, vel, edge_attr."""
    c = lambda t: t.to(dtype) if t.is_floating_point() else t
    sdg = {k: c(v).clone().requires_grad_(grads and v.is_floating_point()) for k, v in sd.items()}
    leaves = {k: c(inp[k]).clone().requires_grad_(grads) for k in ("x", "vel", "edge_attr")}
    args = (sdg, leaves["x"], leaves["vel"], inp["edges"], leaves["edge_attr"], c(inp["charges"]))
    if num_nodes is None:
        res = O.aether_forward(*args, return_all=True, edge_shift=shift)
    else:
        res = O.dynamic_field_aether_forward(*args, num_nodes, return_all=True, edge_shift=shift)
    pg, ig = {}, {}
    if grads:
        torch.nn.functional.mse_loss(res["out"], c(inp["target"])).backward()
        pg = {k: v.grad for k, v in sdg.items() if v.grad is not None}
        ig = {k: v.grad for k, v in leaves.items()}
    return {k: v.detach() for k, v in res.items()}, pg, ig


def node_blocks(x, vel, graph_of):
    """Row blocks of a per-node tensor: (name, rows, scale rows).  Per graph, every degenerate node alone (zero or
    sub-1e-6 velocity, or a position shared with another node of its graph), measured against the larger of its own scale
    and that of its graph's regular nodes, then the graph's regular nodes together."""
    blocks = []
    for g in torch.unique(graph_of).tolist():
        rows = (graph_of == g).nonzero().flatten()
        xs = x[rows]
        shared = (xs[:, None, :] == xs[None, :, :]).all(-1).sum(1) > 1
        slow = vel[rows].abs().max(1).values < 1e-6
        deg = shared | slow
        reg = rows[~deg] if bool((~deg).any()) else rows
        blocks += [(f"graph {g} node {int(r)}", r.view(1), reg) for r in rows[deg]]
        if bool((~deg).any()):
            blocks.append((f"graph {g} regular", reg, reg))
    return blocks


def edge_blocks(recv, graph_of):
    """Row blocks of a per-edge tensor: per graph (of the receiver)."""
    ge = graph_of[recv]
    out = []
    for g in torch.unique(ge).tolist():
        rows = (ge == g).nonzero().flatten()
        out.append((f"graph {g} edges", rows, rows))
    return out


def block_errors(got, want, floor, blocks):
    """[(block name, scale-relative error of got, of the fp32 floor)] against want, block by block."""
    res = []
    for name, rows, scale_rows in blocks:
        w = want[rows].double()
        den = max(float(w.abs().max()), float(want[scale_rows].double().abs().max()), 1e-30)
        res.append((name, float((got[rows].double() - w).abs().max()) / den,
                    float((floor[rows].double() - w).abs().max()) / den))
    return res


def assert_blocks(got, want, floor, blocks, tol, what):
    """Every block within max(tol, 4 x the fp32 oracle's own distance to the fp64 one)."""
    assert torch.isfinite(got).all(), what
    for name, err, fl in block_errors(got, want, floor, blocks):
        assert err <= max(tol, 4.0 * fl), (what, name, err, fl)
