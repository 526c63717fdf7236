#!/usr/bin/env python3
"""Time LoCS (``--model locs``) at the cfg2 shape: D = 2, B = 128 graphs of N = 20 (48,640 edges), hidden 64, dropout 0
(experiments/lorentz/main.py:42-64,140-141).

Rows (one JSON line each, ms per call, median of `--reps` timed blocks of `--iters` calls between HIP events):
  hip_forward            LoCS under torch.no_grad() (aether_forward_field with a zero field)
  hip_train_step         GraphedTrainStep replay: forward + aether_backward_field + FusedAdamW as one graph
  aether_hip_forward     the Aether drop-in at the same shape (the step LoCS rides on), for comparison
  aether_hip_train_step  the same for Aether's captured training step
  restatement_eager_forward     LoCS in eager PyTorch on the same GPU, fp32: the fp64-tested restatement
                                tests/locs_restatement.py (the reference's equations on plain torch ops).  It is not the
                                reference class itself, which is not part of this repository.
  restatement_eager_train_step  the same: forward, MSELoss backward and torch.optim.AdamW(fused=True), eager

Usage: python tools/locs_time.py [--iters 50] [--reps 5] [--out FILE]
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

from aether_amd.nn.state2state.aether import Aether                   # noqa: E402
from aether_amd.nn.state2state.locs import LoCS                       # noqa: E402
from aether_amd.synthetic import make_batch                           # noqa: E402
from aether_amd.training import GraphedTrainStep                      # noqa: E402
import locs_restatement as R                                          # noqa: E402


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
    D, B, N, H = 2, 128, 20, 64
    dev = "cuda"
    g = make_batch(B, N, D, seed=2024, device=dev)
    a = (g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"])
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = LoCS(2 * D, H, 0.0, D, device=dev)
        ae = Aether(2 * D, H, 0.0, D, device=dev)
    rows = []
    base = dict(D=D, B=B, N=N, E=int(g["edges"][0].numel()), hidden=H, device=torch.cuda.get_device_name(0),
                iters=args.iters, reps=args.reps)

    def fwd():
        with torch.no_grad():
            m(*a)
    rows.append(dict(base, what="hip_forward", ms=timed(fwd, args.iters, args.reps)))
    step = GraphedTrainStep(m, a, g["target"], lr=5e-4, weight_decay=1e-12)
    rows.append(dict(base, what="hip_train_step", ms=timed(step.step, args.iters, args.reps)))
    step.check()

    def afwd():
        with torch.no_grad():
            ae(*a, g["charges"])
    rows.append(dict(base, what="aether_hip_forward", ms=timed(afwd, args.iters, args.reps)))
    astep = GraphedTrainStep(ae, a + (g["charges"],), g["target"], lr=5e-4, weight_decay=1e-12)
    rows.append(dict(base, what="aether_hip_train_step", ms=timed(astep.step, args.iters, args.reps)))
    astep.check()

    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=5e-4, weight_decay=1e-12, fused=True)

    def tfwd():
        with torch.no_grad():
            R.forward(sd, g["x"], g["vel"], g["edges"], g["edge_attr"])

    def tstep():
        opt.zero_grad(set_to_none=True)
        out = R.forward(sd, g["x"], g["vel"], g["edges"], g["edge_attr"])
        torch.nn.functional.mse_loss(out, g["target"]).backward()
        opt.step()
    rows.append(dict(base, what="restatement_eager_forward", ms=timed(tfwd, args.iters, args.reps)))
    rows.append(dict(base, what="restatement_eager_train_step", ms=timed(tstep, args.iters, args.reps)))
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
