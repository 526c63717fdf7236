#!/usr/bin/env python3
"""Golden fixtures of LoCS (the Lorentz runner's ``--model locs``) from the imported reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (AETHER_REFERENCE, default /root/reference).  Imported, unmodified:
``nn.state2state.locs.locs.LoCS`` (with the torch_scatter stand-in of oracle/make_golden.py).  Parameters come from the
class's own constructor under a fixed torch seed; inputs are built as experiments/lorentz/main.py:236-241 builds them
(``aether_amd.synthetic.make_batch``: edge_attr_orig = [q_i q_j, |x_i - x_j|], nodes = |vel|).  Per case, one file
``tests/golden/locs_<case>.npz`` holding

  seed, config (D, hidden, B, N, inputgrad, dropout x 1000), keys (state_dict order), shapes, sum.* / abs.* checksums;
  param.*                every parameter where the model is small (hidden 20); the others are the seeded default
                         initialisation and are rebuilt from the seed (the 1 MiB file limit)
  in.*                   h, x, vel, charges, edge_attr, target, send, recv
  ref.out / ref.loss     the reference's fp32 forward and nn.MSELoss()(out, target) (main.py:86,288)
  ref.grad.*             fp32 parameter gradients (hidden 128: the tensors of layer_1 and out_mlp and every bias; the
                         larger ones only as ref.gsum.* / ref.gabs.*)
  ref.ingrad.*           x, vel, edge_attr gradients (the inputgrad case)
  mask1 / mask2          the dropout case: the masks the reference's nn.Dropout layers drew (forward hooks on
                         gnn.out_mlp[2] / [5], as oracle/make_golden_dropout.py), scaled by 1 / (1 - p)
  ref64.out / ref64.loss the same after .double() (not in the dropout case: a new draw there)
  ref64.grad.*           fp64 gradients where the file stays small (hidden 20), ref64.gsum.* / ref64.gabs.* everywhere

Reruns reproduce the files byte for byte (np.savez of deterministic CPU results; no timestamps).

Usage:  python tools/make_golden_locs.py [--out tests/golden]
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
sys.path.insert(0, REPO)

import make_golden as MG                      # noqa: E402  (torch_scatter stand-in)
from aether_amd.synthetic import make_batch   # noqa: E402

# name, seed, D, hidden, B, N, inputgrad, dropout_prob
CASES = [
    ("D2_H64_B2N5", 6101, 2, 64, 2, 5, False, 0.0),
    ("D3_H64_B2N5", 6102, 3, 64, 2, 5, False, 0.0),
    ("D2_H20_B3N5", 6103, 2, 20, 3, 5, False, 0.0),
    ("D3_H20_B2N5", 6104, 3, 20, 2, 5, False, 0.0),
    ("D2_H128_B2N5", 6105, 2, 128, 2, 5, False, 0.0),
    ("D3_H128_B2N5", 6106, 3, 128, 2, 5, False, 0.0),
    ("D3_H64_B3N12_inputgrad", 6107, 3, 64, 3, 12, True, 0.0),
    ("D2_H64_B4N9_dropout", 6108, 2, 64, 4, 9, False, 0.25),
]


@contextlib.contextmanager
def reference():
    MG._install_scatter_standin()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import nn.state2state.locs.locs as L                              # noqa: WPS433 (reference import)
    yield L


def build_model(L, seed, D, H, p):
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        return L.LoCS(2 * D, H, p, D, device="cpu")


def _full_grad(H, key):
    """Whether a tensor's fp32 gradient is stored whole (hidden 128: layer_1, out_mlp and biases only)."""
    return H <= 64 or key.startswith("gnn.layer_1.") or key.startswith("gnn.out_mlp.") or key.endswith(".bias")


def case_fixture(L, name, seed, D, H, B, N, inputgrad, p):
    m = build_model(L, seed, D, H, p)
    sd = m.state_dict()
    small = H <= 20
    inp = make_batch(B, N, D, seed=seed + 1)
    o = {"seed": np.int64(seed), "config": np.array([D, H, B, N, int(inputgrad), int(round(p * 1000))], dtype=np.int64),
         "keys": np.array(list(sd.keys())), "shapes": np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()])}
    for k, v in sd.items():
        o["sum." + k] = np.float64(v.double().sum().item())
        o["abs." + k] = np.float64(v.double().abs().sum().item())
        if small:
            o["param." + k] = v.numpy().copy()
    for k in ("h", "x", "vel", "charges", "edge_attr", "target"):
        o["in." + k] = inp[k].numpy()
    o["in.send"], o["in.recv"] = inp["edges"][0].numpy(), inp["edges"][1].numpy()
    for tag in (("ref",) if p > 0 else ("ref", "ref64")):
        model = m if tag == "ref" else m.double()
        cast = (lambda t: t) if tag == "ref" else (lambda t: t.double())
        model.train() if p > 0 else model.eval()
        cap = {}

        def hook(key):
            def fn(_m, _i, out):
                cap[key] = (out != 0).to(out.dtype) / (1.0 - p)
            return fn

        hooks = ([model.gnn.out_mlp[2].register_forward_hook(hook("mask1")),
                  model.gnn.out_mlp[5].register_forward_hook(hook("mask2"))] if p > 0 else [])
        ins = {k: cast(inp[k]).clone().requires_grad_(inputgrad) for k in ("x", "vel", "edge_attr")}
        model.zero_grad(set_to_none=True)
        torch.manual_seed(seed + 2)
        out = model(cast(inp["h"]), ins["x"], inp["edges"], ins["vel"], ins["edge_attr"])
        loss = torch.nn.MSELoss()(out, cast(inp["target"]))
        loss.backward()
        for hk in hooks:
            hk.remove()
        o[tag + ".out"] = out.detach().numpy()
        o[tag + ".loss"] = np.float64(loss.item())
        if p > 0:
            o["mask1"], o["mask2"] = cap["mask1"].numpy(), cap["mask2"].numpy()
        if inputgrad:
            for k, t in ins.items():
                o[f"{tag}.ingrad.{k}"] = t.grad.numpy()
        for k, prm in model.named_parameters():
            g = prm.grad.detach()
            if (tag == "ref" and _full_grad(H, k)) or (tag == "ref64" and small):
                o[f"{tag}.grad.{k}"] = g.numpy().copy()
            o[f"{tag}.gsum.{k}"] = np.float64(g.double().sum().item())
            o[f"{tag}.gabs.{k}"] = np.float64(g.double().abs().sum().item())
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    with reference() as L:
        for name, *cfg in CASES:
            o = case_fixture(L, name, *cfg)
            path = os.path.join(args.out, f"locs_{name}.npz")
            np.savez(path, **o)
            print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
