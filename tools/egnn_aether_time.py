#!/usr/bin/env python3
"""Time EGNN-Aether (``--model egnn_aether``) at the dynamic_20body shape: B = 128 graphs of N = 20 (48,640 edges),
hidden_nf 64, 4 layers, the runner's defaults (norm_diff False, tanh False; experiments/lorentz/main.py:42-64,147).

Rows (one JSON line each, ms per call, median of `--reps` timed blocks of `--iters` calls between HIP events):
  hip_forward          EGNN_vel_Aether under torch.no_grad() (aether_egnn_forward)
  hip_train_step       GraphedTrainStep replay: forward + aether_egnn_backward + FusedAdamW as one graph
  torch_forward        the plain PyTorch restatement (tests/egnn_restatement.py) on the same GPU, fp32, eager
  torch_train_step     the same: forward, MSELoss backward and torch.optim.AdamW(fused=True), eager

Usage: python tools/egnn_aether_time.py [--iters 50] [--reps 5] [--out FILE]
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from aether_amd.nn.state2state.egnn_aether import EGNN_vel_Aether     # noqa: E402
from aether_amd.training import GraphedTrainStep                       # noqa: E402
import egnn_restatement as R                                           # noqa: E402


def timed(fn, iters, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, N, H, L = 128, 20, 64, 4
    dev = "cuda"
    inp = R.runner_batch(B, N, 2024)
    g = {k: ([e.to(dev) for e in v] if k == "edges" else v.to(dev)) for k, v in inp.items()}
    a = (g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"], g["charges"])
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = EGNN_vel_Aether(1, 8, H, 3, device=dev, n_layers=L, recurrent=True)
    rows = []
    base = dict(B=B, N=N, E=int(g["edges"][0].numel()), hidden_nf=H, n_layers=L, norm_diff=False, tanh=False,
                device=torch.cuda.get_device_name(0), iters=args.iters, reps=args.reps)

    def fwd():
        with torch.no_grad():
            m(*a)
    rows.append(dict(base, what="hip_forward", ms=timed(fwd, args.iters, args.reps)))
    step = GraphedTrainStep(m, a, g["target"], lr=5e-4, weight_decay=1e-12)
    rows.append(dict(base, what="hip_train_step", ms=timed(step.step, args.iters, args.reps)))
    step.check()

    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=5e-4, weight_decay=1e-12, fused=True)

    def tfwd():
        with torch.no_grad():
            R.forward(sd, g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"], g["charges"], L)

    def tstep():
        opt.zero_grad(set_to_none=True)
        out, _, _ = R.forward(sd, g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"], g["charges"], L)
        torch.nn.functional.mse_loss(out, g["target"]).backward()
        opt.step()
    rows.append(dict(base, what="torch_forward", ms=timed(tfwd, args.iters, args.reps)))
    rows.append(dict(base, what="torch_train_step", ms=timed(tstep, args.iters, args.reps)))
    lines = []
    for r in rows:
        med, lo, hi = r.pop("ms")
        r.update(ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
        lines.append(json.dumps(r))
    print("\n".join(lines))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
