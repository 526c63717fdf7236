#!/usr/bin/env python3
"""Time ClofNet_vel (``--model clof_vel``) at the reference README's shape: B = 128 graphs of N = 20 (48,640 edges),
hidden_nf 64, 4 layers, norm_diff True (the README's clof_vel command; experiments/lorentz/main.py:152-157).

Rows (one JSON line each, ms per call, median of `--reps` timed blocks of `--iters` calls between HIP events):
  hip_forward          ClofNet_vel under torch.no_grad() (aether_clof_forward)
  hip_train_step       GraphedTrainStep replay: forward + aether_clof_backward + FusedAdamW as one graph
  torch_forward        the plain PyTorch restatement (tests/clof_restatement.py) on the same GPU, fp32, eager
  torch_train_step     the same: forward, MSELoss backward and torch.optim.AdamW(fused=True), eager

``--step-only N``: build the captured step and replay it N times, nothing else (for a kernel trace of the step).

Usage: python tools/clof_time.py [--iters 50] [--reps 5] [--out FILE] [--step-only N]
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

from aether_amd.nn.state2state.clof import ClofNet_vel               # noqa: E402
from aether_amd.training import GraphedTrainStep                       # noqa: E402
import clof_restatement as R                                           # noqa: E402


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
    ap.add_argument("--step-only", type=int, default=0)
    args = ap.parse_args()
    B, N, H, L = 128, 20, 64, 4
    dev = "cuda"
    inp = R.runner_batch(B, N, 2024)
    g = {k: ([e.to(dev) for e in v] if k == "edges" else v.to(dev)) for k, v in inp.items()}
    a = (g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"], None, N)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = ClofNet_vel(1, 2, H, device=dev, n_layers=L, recurrent=True, norm_diff=True)
    step = GraphedTrainStep(m, a, g["target"], lr=5e-4, weight_decay=1e-12)
    if args.step_only:
        for _ in range(args.step_only):
            step.step()
        step.check()
        return
    rows = []
    base = dict(model="clof_vel", B=B, N=N, E=int(g["edges"][0].numel()), hidden_nf=H, n_layers=L, norm_diff=True,
                tanh=False, device=torch.cuda.get_device_name(0), iters=args.iters, reps=args.reps)

    def fwd():
        with torch.no_grad():
            m(*a)
    rows.append(dict(base, what="hip_forward", ms=timed(fwd, args.iters, args.reps)))
    rows.append(dict(base, what="hip_train_step", ms=timed(step.step, args.iters, args.reps)))
    step.check()

    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=5e-4, weight_decay=1e-12, fused=True)

    def run():
        return R.forward(sd, 1, g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"], L, N, norm_diff=True)[0]

    def tfwd():
        with torch.no_grad():
            run()

    def tstep():
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.mse_loss(run(), g["target"]).backward()
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
