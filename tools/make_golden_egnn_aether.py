#!/usr/bin/env python3
"""Golden fixtures of EGNN-Aether (the Lorentz runner's ``--model egnn_aether``) from the imported reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (AETHER_REFERENCE, default /root/reference).  Imported, unmodified:
``nn.state2state.egnn_aether.EGNN_vel_Aether`` (with the torch_scatter stand-in of oracle/make_golden.py, which the
reference's package imports need; EGNN-Aether itself does not call torch_scatter).  Parameters come from the class's own
constructor under a fixed torch seed (the clamp case then scales phi's last weight), inputs are built as
experiments/lorentz/main.py:204-259 builds them (tests/egnn_restatement.py::runner_batch).  Per case, one file
``tests/golden/egnn_aether_<case>.npz`` holding

  seed, config (B, N, hidden_nf, n_layers, norm_diff, tanh), keys (state_dict order), sum.* / abs.* checksums;
  param.*                     every parameter, in the cases with one layer of width 64 (the others are the seeded
                              default initialisation and are rebuilt from the seed; the 1 MiB file limit)
  in.*                        h, x, row, col, vel, edge_attr, charges, target
  ref.out / ref.h<l> / ref.x<l>   the reference's fp32 forward: every layer's input and the output (l = 0 .. L)
  ref.grad.*                  fp32 parameter gradients of nn.MSELoss()(out, target) (main.py:86,288)
  ref64.out / ref64.h<l> / ref64.x<l>   the same after .double()
  ref64.grad.*                fp64 gradients in the same cases; ref64.gsum.* / ref64.gabs.* (sum, sum of |.|) for every
                              case -- full fp64 gradients of the larger models would exceed the file size limit
  in_node_nf, graph           only in the cases that leave the runner's inputs: the width of h (h = [|vel|, q, |x|]) and
                              "multi" (tests/graph_cases.py::random_multigraph: duplicate edges, a self loop, a node
                              without edges, rows in random order) or "empty" (no edge at all)

The case of width 128 with four layers is "slim": its fp32 gradient tensors alone would exceed the 1 MiB file limit, so
it holds no ref.grad.* and instead ref.gsum.* / ref.gabs.* / ref.gmax.* (sum, sum of |.|, max of |.| of every fp32
gradient, as fp64 numbers) next to ref64.gsum.* / ref64.gabs.* / ref64.gmax.*.

Reruns reproduce the files byte for byte (np.savez of deterministic CPU results; no timestamps).

Usage:  python tools/make_golden_egnn_aether.py [--out tests/golden]
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

# name, seed, B, N, hidden_nf, n_layers, norm_diff, tanh, pos_scale, phi_scale
CASES = [
    ("B2N5_H64_L4", 5101, 2, 5, 64, 4, False, False, 1.0, 1.0),
    ("B2N5_H64_L4_norm_tanh", 5102, 2, 5, 64, 4, True, True, 1.0, 1.0),
    ("B1N2_H64_L4_tanh", 5103, 1, 2, 64, 4, False, True, 1.0, 1.0),
    ("B1N2_H64_L1_norm", 5104, 1, 2, 64, 1, True, False, 1.0, 1.0),
    ("B2N5_H128_L1_norm_tanh", 5105, 2, 5, 128, 1, True, True, 1.0, 1.0),
    ("B1N2_H128_L1", 5106, 1, 2, 128, 1, False, False, 1.0, 1.0),
    # |d * phi| > 100 on some edges: positions x 30 and phi's last weight x 3000 (the clamp's gradient is zero there)
    ("B2N5_H64_L1_clamp", 5107, 2, 5, 64, 1, False, False, 30.0, 3000.0),
    ("B2N5_H128_L4_norm", 5108, 2, 5, 128, 4, True, False, 1.0, 1.0),                  # slim, see above
    # four layers: positions x 3 and phi x 30000.  At positions x 30 the fp32 reference's own gradients are 1.1e-4 from
    # the fp64 ones (max|a - b| / max|b|), past the 5e-5 bar of the GPU tests; here they are 1e-5 away
    ("B2N5_H64_L4_clamp", 5109, 2, 5, 64, 4, False, False, 3.0, 30000.0),
    ("B2N5_H64_L2_innf3", 5110, 2, 5, 64, 2, False, True, 1.0, 1.0, dict(in_nf=3)),
    # a self loop: norm_diff off (sqrt at 0 has a NaN gradient in the reference)
    ("B2N6_H64_L2_multigraph", 5111, 2, 6, 64, 2, False, False, 1.0, 1.0, dict(graph="multi")),
    ("B2N5_H64_L2_noedges", 5112, 2, 5, 64, 2, True, False, 1.0, 1.0, dict(graph="empty")),
]


@contextlib.contextmanager
def reference():
    MG._install_scatter_standin()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import nn.state2state.egnn_aether as A                            # noqa: WPS433 (reference import)
    yield A


def build_model(A, seed, H, L, norm_diff, tanh, phi_scale, in_nf=1):
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = A.EGNN_vel_Aether(in_node_nf=in_nf, in_edge_nf=8, hidden_nf=H, num_dims=3, device="cpu", n_layers=L,
                              recurrent=True, norm_diff=norm_diff, tanh=tanh)
    if phi_scale != 1.0:
        with torch.no_grad():
            for l in range(L):
                m._modules["gcl_%d" % l].coord_mlp[2].weight.mul_(phi_scale)
    return m


def run(m, inp, L):
    """The reference forward (egnn_aether.py:65-75), step by step to record every layer's h and x."""
    x = inp["x"].clone()            # the reference adds into x in place (egnn/gcl.py:97)
    h_in, vel, edges = inp["h"], inp["vel"], inp["edges"]
    predicted_field = m.field_net(torch.cat([x, vel], dim=-1), inp["charges"])
    h = m.embedding(h_in)
    hs, xs = [h.detach().clone()], [x.detach().clone()]
    for i in range(L):
        h, x, _ = m._modules["gcl_%d" % i](h, edges, x, vel, edge_attr=inp["edge_attr"], predicted_field=predicted_field)
        hs.append(h.detach().clone())
        xs.append(x.detach().clone())
    # the whole forward once more through EGNN_vel_Aether.forward itself: the recorded output must be its output
    out = m(h_in, inp["x"].clone(), edges, vel, inp["edge_attr"], inp["charges"])
    assert torch.equal(out, xs[-1])
    return out, hs, xs


def case_inputs(B, N, seed, pos_scale, in_nf, graph):
    if graph == "multi":
        inp = GC.random_multigraph(B, N, seed + 1, self_loop=True, dtype=torch.float32)
        row, col = inp["edges"]
        deg_r, deg_c = (torch.bincount(t, minlength=B * N) for t in (row, col))
        assert int((row == col).sum()) == 1 and int(((deg_r == 0) & (deg_c == 0)).sum()) >= B
        assert torch.unique(torch.stack([row, col]), dim=1).shape[1] < row.numel()           # duplicate edges
        assert row.numel() != 3
    else:
        inp = R.runner_batch(B, N, seed + 1, pos_scale=pos_scale)
        if graph == "empty":
            inp = GC.without_edges(inp)
    if in_nf != 1:
        inp = GC.with_wide_h(inp, in_nf)
    return inp


def case_fixture(A, name, seed, B, N, H, L, norm_diff, tanh, pos_scale, phi_scale, extra=None):
    extra = extra or {}
    in_nf, graph = extra.get("in_nf", 1), extra.get("graph", "runner")
    m = build_model(A, seed, H, L, norm_diff, tanh, phi_scale, in_nf)
    sd = m.state_dict()
    full = L == 1 and H == 64            # parameters and fp64 gradients in full (the others: size limit)
    slim = L > 1 and H == 128
    inp = case_inputs(B, N, seed, pos_scale, in_nf, graph)
    o = {"seed": np.int64(seed), "config": np.array([B, N, H, L, int(norm_diff), int(tanh)], dtype=np.int64),
         "keys": np.array(list(sd.keys())), "phi_scale": np.float64(phi_scale)}
    if extra:
        o["in_node_nf"], o["graph"] = np.int64(in_nf), np.array(graph)
    for k, v in sd.items():
        o["sum." + k] = np.float64(v.double().sum().item())
        o["abs." + k] = np.float64(v.double().abs().sum().item())
        if full:
            o["param." + k] = v.numpy().copy()
    for k in ("h", "x", "vel", "edge_attr", "charges", "target"):
        o["in." + k] = inp[k].numpy()
    o["in.row"], o["in.col"] = inp["edges"][0].numpy(), inp["edges"][1].numpy()
    for tag in ("ref", "ref64"):
        model = m if tag == "ref" else m.double()
        cast = (lambda t: t) if tag == "ref" else (lambda t: t.double())
        ci = {k: (cast(v) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}
        model.zero_grad(set_to_none=True)
        out, hs, xs = run(model, ci, L)
        loss = torch.nn.MSELoss()(out, ci["target"])
        loss.backward()
        o[tag + ".out"] = out.detach().numpy()
        o[tag + ".loss"] = np.float64(loss.item())
        for l in range(L + 1):
            o[f"{tag}.h{l}"] = hs[l].numpy()
            o[f"{tag}.x{l}"] = xs[l].numpy()
        for k, p in model.named_parameters():
            # the last layer's node_mlp does not reach the output x: torch leaves its .grad None, stored as zeros
            g = p.grad.detach() if p.grad is not None else torch.zeros_like(p)
            if (tag == "ref" and not slim) or full:
                o[f"{tag}.grad.{k}"] = g.numpy().copy()
            if tag == "ref64" or slim:
                o[f"{tag}.gsum.{k}"] = np.float64(g.double().sum().item())
                o[f"{tag}.gabs.{k}"] = np.float64(g.double().abs().sum().item())
            if slim:
                o[f"{tag}.gmax.{k}"] = np.float64(g.double().abs().max().item())
    if phi_scale != 1.0:           # the clamp must be active on some edges and inactive on others, in the first layer
        m32 = build_model(A, seed, H, L, norm_diff, tanh, phi_scale, in_nf)
        raw = _first_layer_translation(m32, inp)
        n_clamped = int((raw.abs() > 100).sum())
        assert 0 < n_clamped < raw.numel(), n_clamped
        o["n_clamped"] = np.int64(n_clamped)
    return o


def _first_layer_translation(m, inp):
    """d * phi(m) of layer 0 before the clamp, through the reference's own sub-modules."""
    g = m._modules["gcl_0"]
    x, vel, edges = inp["x"], inp["vel"], inp["edges"]
    f = m.field_net(torch.cat([x, vel], dim=-1), inp["charges"])
    h = m.embedding(inp["h"])
    row, col = edges
    radial, coord_diff = g.coord2radial(edges, x)
    ef = g.edge_model(h[row], h[col], radial, torch.cat([inp["edge_attr"], f[row], f[col]], dim=-1))
    return (coord_diff * g.coord_mlp(ef)).detach()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    with reference() as A:
        for name, *cfg in CASES:
            o = case_fixture(A, name, *cfg)
            path = os.path.join(args.out, f"egnn_aether_{name}.npz")
            np.savez(path, **o)
            print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
