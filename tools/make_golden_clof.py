#!/usr/bin/env python3
"""Golden fixtures of the ClofNet models (the Lorentz runner's ``--model clof | clof_vel | clof_vel_gbf``) from the
imported reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (AETHER_REFERENCE, default /root/reference).  Imported, unmodified:
``nn.state2state.clof.clof.{ClofNet, ClofNet_vel, ClofNet_vel_gbf}`` (with the torch_scatter stand-in of
oracle/make_golden.py, which the reference's package imports need).  Parameters come from the classes' own constructors
under a fixed torch seed (the clamp case then scales coord_mlp.2's weight), inputs are built as
experiments/lorentz/main.py:266-271 builds them (tests/egnn_restatement.py::runner_batch).  Per case, one file
``tests/golden/clof_<case>.npz`` holding

  seed, variant, config (B, N, hidden_nf, n_layers, norm_diff, tanh, recurrent), coords_weight, coord_scale, keys
  (state_dict order), sum.* / abs.* checksums;
  param.*                     every parameter, in the one-layer cases of width 64 (the others are the seeded default
                              initialisation and are rebuilt from the seed; the 1 MiB file limit)
  in.*                        h, x, row, col, vel, edge_attr, target
  ref.out / ref.h<l> / ref.x<l>   the reference's fp32 forward: every layer's input h and centred x, and the output
  ref.grad.*                  fp32 parameter gradients of nn.MSELoss()(out, target) (main.py:86,288); ref.dead lists the
                              parameters whose .grad torch leaves None
  ref64.*                     the same after .double(); full fp64 gradients in the one-layer cases, sums (gsum / gabs)
                              in every case
  in_node_nf, graph           only in the cases that leave the runner's inputs: the width of h (h = [|vel|, q, |x|]) and
                              "multi" (tests/graph_cases.py::random_multigraph: duplicate edges, a self loop, a node
                              without edges, rows in random order) or "empty" (no edge at all)

The cases of width 128 with four layers are "slim": their fp32 gradient tensors alone would exceed the 1 MiB file limit,
so they hold no ref.grad.* and no param.*, and instead ref.gsum.* / ref.gabs.* / ref.gmax.* (sum, sum of |.|, max of |.|
of every fp32 gradient, as fp64 numbers) next to ref64.gsum.* / ref64.gabs.* / ref64.gmax.*.

No case has exactly 3 edges (torch.cross without dim would cross along the edge axis there).  Reruns reproduce the files
byte for byte (np.savez of deterministic CPU results; no timestamps).

Usage:  python tools/make_golden_clof.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("AETHER_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import make_golden as MG                      # noqa: E402  (torch_scatter stand-in)
import egnn_restatement as R                  # noqa: E402  (runner_batch)
import graph_cases as GC                      # noqa: E402  (inputs off the runner's graphs)

CLASSES = {"clof": "ClofNet", "clof_vel": "ClofNet_vel", "clof_vel_gbf": "ClofNet_vel_gbf"}

# name, model, seed, B, N, hidden_nf, n_layers, norm_diff, tanh, recurrent, coords_weight, pos_scale, coord_scale
CASES = [
    ("clof_vel_B2N5_H64_L4", "clof_vel", 6101, 2, 5, 64, 4, True, False, True, 1.0, 1.0, 1.0),
    ("clof_B2N5_H64_L4", "clof", 6102, 2, 5, 64, 4, True, False, True, 1.0, 1.0, 1.0),
    ("clof_vel_gbf_B2N5_H64_L4", "clof_vel_gbf", 6103, 2, 5, 64, 4, True, False, True, 1.0, 1.0, 1.0),
    # two nodes, centred: x_row = -x_col, so cross = 0 and vertical = 0 in the prologue's and the first layer's frames
    ("clof_vel_B1N2_H64_L4", "clof_vel", 6104, 1, 2, 64, 4, False, False, True, 1.0, 1.0, 1.0),
    ("clof_B1N2_H64_L1_norm", "clof", 6105, 1, 2, 64, 1, True, False, True, 1.0, 1.0, 1.0),
    ("clof_vel_B2N5_H128_L1", "clof_vel", 6106, 2, 5, 128, 1, True, False, True, 1.0, 1.0, 1.0),
    ("clof_B2N5_H64_L2_nonorm_tanh", "clof", 6107, 2, 5, 64, 2, False, True, True, 1.0, 1.0, 1.0),
    ("clof_vel_B2N5_H64_L2_norec_cw", "clof_vel", 6108, 2, 5, 64, 2, True, False, False, 0.5, 1.0, 1.0),
    ("clof_vel_gbf_B2N5_H64_L1_tanh", "clof_vel_gbf", 6109, 2, 5, 64, 1, False, True, True, 1.0, 1.0, 1.0),
    # |translation| > 100 on some edges: coord_mlp.2's weight x 4e6 (zero gradient there).  With norm_diff the frame
    # vectors are bounded by 1, so the translation is the coefficients themselves: no cancellation amplifies fp32 rounding
    ("clof_vel_B2N5_H64_L1_clamp", "clof_vel", 6110, 2, 5, 64, 1, True, False, True, 1.0, 1.0, 4e6),
    # width 128 at depth: the not-last node kernel and LayerNorm at 128 (slim files, see above)
    ("clof_vel_B2N5_H128_L4", "clof_vel", 6111, 2, 5, 128, 4, True, False, True, 1.0, 1.0, 1.0),
    ("clof_B2N5_H128_L4", "clof", 6112, 2, 5, 128, 4, True, False, True, 1.0, 1.0, 1.0),
    ("clof_vel_gbf_B2N5_H128_L4", "clof_vel_gbf", 6113, 2, 5, 128, 4, True, False, True, 1.0, 1.0, 1.0),
    ("clof_vel_B2N5_H64_L4_norec_cw_tanh", "clof_vel", 6114, 2, 5, 64, 4, True, True, False, 0.5, 1.0, 1.0),
    ("clof_vel_B2N5_H64_L2_innf3", "clof_vel", 6115, 2, 5, 64, 2, True, False, True, 1.0, 1.0, 1.0, dict(in_nf=3)),
    # a self loop: norm_diff off in the layers (sqrt at 0 has a NaN gradient in the reference)
    ("clof_vel_B2N6_H64_L2_multigraph", "clof_vel", 6116, 2, 6, 64, 2, False, False, True, 1.0, 1.0, 1.0,
     dict(graph="multi")),
    ("clof_vel_B2N5_H64_L2_noedges", "clof_vel", 6117, 2, 5, 64, 2, True, False, True, 1.0, 1.0, 1.0,
     dict(graph="empty")),
]


@contextlib.contextmanager
def reference():
    MG._install_scatter_standin()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import nn.state2state.clof.clof as A                              # noqa: WPS433 (reference import)
    yield A


def build_model(A, model, seed, H, L, norm_diff, tanh, recurrent, cw, coord_scale, in_nf=1):
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = getattr(A, CLASSES[model])(in_node_nf=in_nf, in_edge_nf=2, hidden_nf=H, device="cpu", n_layers=L,
                                       coords_weight=cw, recurrent=recurrent, norm_diff=norm_diff, tanh=tanh)
    if coord_scale != 1.0:
        with torch.no_grad():
            for l in range(L):
                m._modules["gcl_%d" % l].coord_mlp[2].weight.mul_(coord_scale)
    return m


def run(m, inp, L, N):
    """The reference forward (clof.py), step by step to record every layer's h and centred x."""
    x, vel, edges, ea = inp["x"], inp["vel"], inp["edges"], inp["edge_attr"]
    h = m.embedding_node(inp["h"])
    xb = x.reshape(-1, N, 3)
    centroid = torch.mean(xb, dim=1, keepdim=True)
    xc = (xb - centroid).reshape(-1, 3)
    if isinstance(m, sys.modules[type(m).__module__].ClofNet):
        ef = m.fuse_edge(torch.cat([ea, m.scalarization(edges, xc)], dim=-1))
    elif hasattr(m, "gbf"):
        ef = m.fuse_edge(m.scalarization(edges, xc, vel)) + m.embed_edge(ea[:, 0], ea[:, 1])
    else:
        ef = m.fuse_edge(torch.cat([ea, m.scalarization(edges, xc, vel)], dim=-1))
    hs, xs = [h.detach().clone()], [xc.detach().clone()]
    for i in range(L):
        h, xc, _ = m._modules["gcl_%d" % i](h, edges, xc, vel, edge_attr=ef, node_attr=None)
        hs.append(h.detach().clone())
        xs.append(xc.detach().clone())
    out = (xc.reshape(-1, N, 3) + centroid).reshape(-1, 3)
    # the whole forward once more through the class's own forward: the recorded output must be its output
    ref_out = m(inp["h"], x.clone(), edges, vel, ea, n_nodes=N)
    assert torch.equal(out, ref_out)
    return ref_out, hs, xs


def case_inputs(B, N, seed, pos_scale, in_nf, graph):
    if graph == "multi":
        inp = GC.random_multigraph(B, N, seed + 1, self_loop=True, dtype=torch.float32)
        row, col = inp["edges"]
        deg_r, deg_c = (torch.bincount(t, minlength=B * N) for t in (row, col))
        assert int((row == col).sum()) == 1 and int(((deg_r == 0) & (deg_c == 0)).sum()) >= B
        assert torch.unique(torch.stack([row, col]), dim=1).shape[1] < row.numel()           # duplicate edges
    else:
        inp = R.runner_batch(B, N, seed + 1, pos_scale=pos_scale)
        if graph == "empty":
            inp = GC.without_edges(inp)
    if in_nf != 1:
        inp = GC.with_wide_h(inp, in_nf)
    return inp


def case_fixture(A, name, model, seed, B, N, H, L, norm_diff, tanh, recurrent, cw, pos_scale, coord_scale, extra=None):
    extra = extra or {}
    in_nf, graph = extra.get("in_nf", 1), extra.get("graph", "runner")
    m = build_model(A, model, seed, H, L, norm_diff, tanh, recurrent, cw, coord_scale, in_nf)
    sd = m.state_dict()
    full = L == 1 and H == 64
    slim = L > 1 and H == 128
    inp = case_inputs(B, N, seed, pos_scale, in_nf, graph)
    assert inp["edges"][0].numel() != 3
    o = {"seed": np.int64(seed), "variant": np.array(model),
         "config": np.array([B, N, H, L, int(norm_diff), int(tanh), int(recurrent)], dtype=np.int64),
         "coords_weight": np.float64(cw), "coord_scale": np.float64(coord_scale), "keys": np.array(list(sd.keys()))}
    if extra:
        o["in_node_nf"], o["graph"] = np.int64(in_nf), np.array(graph)
    for k, v in sd.items():
        o["sum." + k] = np.float64(v.double().sum().item())
        o["abs." + k] = np.float64(v.double().abs().sum().item())
        if full:
            o["param." + k] = v.numpy().copy()
    for k in ("h", "x", "vel", "edge_attr", "target"):
        o["in." + k] = inp[k].numpy()
    o["in.row"], o["in.col"] = inp["edges"][0].numpy(), inp["edges"][1].numpy()
    if model == "clof_vel_gbf" and graph != "empty":                  # both edge types occur
        assert set((inp["edge_attr"][:, 0] * 0.5 + 0.5).long().tolist()) == {0, 1}
    for tag in ("ref", "ref64"):
        model_t = m if tag == "ref" else m.double()
        cast = (lambda t: t) if tag == "ref" else (lambda t: t.double())
        ci = {k: (cast(v) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}
        model_t.zero_grad(set_to_none=True)
        out, hs, xs = run(model_t, ci, L, N)
        loss = torch.nn.MSELoss()(out, ci["target"])
        loss.backward()
        o[tag + ".out"] = out.detach().numpy()
        o[tag + ".loss"] = np.float64(loss.item())
        for l in range(L + 1):
            o[f"{tag}.h{l}"] = hs[l].numpy()
            o[f"{tag}.x{l}"] = xs[l].numpy()
        dead = []
        for k, p in model_t.named_parameters():
            if p.grad is None:
                dead.append(k)
                continue
            g = p.grad.detach()
            if (tag == "ref" and not slim) or full:
                o[f"{tag}.grad.{k}"] = g.numpy().copy()
            if tag == "ref64" or slim:
                o[f"{tag}.gsum.{k}"] = np.float64(g.double().sum().item())
                o[f"{tag}.gabs.{k}"] = np.float64(g.double().abs().sum().item())
            if slim:
                o[f"{tag}.gmax.{k}"] = np.float64(g.double().abs().max().item())
        o[tag + ".dead"] = np.array(dead)
    if coord_scale != 1.0:         # the clamp must be active on some edges and inactive on others, in the first layer
        m32 = build_model(A, model, seed, H, L, norm_diff, tanh, recurrent, cw, coord_scale)
        raw = _first_layer_translation(m32, inp, N)
        n_clamped = int((raw.abs() > 100).sum())
        assert 0 < n_clamped < raw.numel(), n_clamped
        o["n_clamped"] = np.int64(n_clamped)
    return o


def _first_layer_translation(m, inp, N):
    """The first layer's translation before the clamp, through the reference's own sub-modules (ClofNet_vel)."""
    g = m._modules["gcl_0"]
    x, vel, edges, ea = inp["x"], inp["vel"], inp["edges"], inp["edge_attr"]
    xb = x.reshape(-1, N, 3)
    xc = (xb - xb.mean(1, keepdim=True)).reshape(-1, 3)
    h = m.embedding_node(inp["h"])
    ef = m.fuse_edge(torch.cat([ea, m.scalarization(edges, xc, vel)], dim=-1))
    row, col = edges
    radial, d, c, v = g.coord2localframe(edges, xc)
    k = g.coord_mlp(g.edge_model(h[row], h[col], radial, ef))
    return (d * k[:, :1] + c * k[:, 1:2] + v * k[:, 2:3]).detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    with reference() as A:
        for name, *cfg in CASES:
            o = case_fixture(A, name, *cfg)
            path = os.path.join(args.out, f"{name}.npz")
            np.savez(path, **o)
            print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
