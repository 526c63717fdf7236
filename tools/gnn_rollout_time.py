#!/usr/bin/env python3
"""Time the device rollout of EGNN-Aether and ClofNet_vel (``.rollout``: aether_egnn_rollout / aether_clof_rollout)
against the loop of module calls it replaces (``aether_amd.rollout.rollout_stepwise_gnn``), in the same run: B = 128
graphs of N = 20 (48,640 edges), hidden_nf 64, 4 layers, 20 steps, dt 1.

Rows (one JSON line each, ms per 20-step rollout, median of `--reps` timed blocks of `--iters` rollouts between HIP
events, the four rows of a family taking turns block by block), per family:
  device_eager / device_graph        .rollout launched eagerly / replayed from a captured hipGraph
  stepwise_eager / stepwise_graph    the loop of module calls, likewise

Usage: python tools/gnn_rollout_time.py [--iters 10] [--reps 5] [--out FILE]   (FILE is appended to)
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

from aether_amd.nn.state2state.clof import ClofNet_vel                 # noqa: E402
from aether_amd.nn.state2state.egnn_aether import EGNN_vel_Aether      # noqa: E402
from aether_amd.rollout import rollout_stepwise_gnn                    # noqa: E402
import egnn_restatement as R                                           # noqa: E402


def timed(fns, iters, reps):
    """{name: (median, min, max) ms per call}: `reps` rounds, in each one block of `iters` calls per function in turn, so
    that the rows of one model see the same machine."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) / iters)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in out.items()}


def captured(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B, N, H, L, steps, dt = 128, 20, 64, 4, 20, 1.0
    dev = "cuda"
    inp = R.runner_batch(B, N, 2024)
    x, vel, q = (inp[k].to(dev) for k in ("x", "vel", "charges"))
    edges = [e.to(dev) for e in inp["edges"]]
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        models = {"egnn_aether": (EGNN_vel_Aether(1, 8, H, 3, device=dev, n_layers=L, recurrent=True), {}),
                  "clof_vel": (ClofNet_vel(1, 2, H, device=dev, n_layers=L), dict(n_nodes=N))}
    base = dict(B=B, N=N, E=int(edges[0].numel()), hidden_nf=H, n_layers=L, steps=steps, dt=dt,
                device=torch.cuda.get_device_name(0), iters=args.iters, reps=args.reps)
    lines = []
    for name, (m, kw) in models.items():
        calls = {"device": lambda: m.rollout(x, vel, edges, q, steps, dt, **kw),
                 "stepwise": lambda: rollout_stepwise_gnn(m, x, vel, edges, q, steps, dt, **kw)}
        eager = {k: f() for k, f in calls.items()}
        torch.cuda.synchronize()
        # untrained weights: EGNN-Aether's rollout may leave fp32's range before step 20; compare the finite steps
        fin = int(torch.isfinite(eager["stepwise"]).flatten(1).all(1).long().cumprod(0).sum())
        dv, sw = eager["device"][:fin], eager["stepwise"][:fin]
        diff = float((dv - sw).abs().max() / sw.abs().max()) if fin else None
        fns = {}
        for k, f in calls.items():
            g, out = captured(f)
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), eager[k].view(torch.int32)), (name, k)      # bit for bit
            fns[k + "_eager"], fns[k + "_graph"] = f, g.replay
        for what, (med, lo, hi) in timed(fns, args.iters, args.reps).items():
            lines.append(json.dumps(dict(base, model=name, what=what, ms_median=round(med, 4), ms_min=round(lo, 4),
                                         ms_max=round(hi, 4), finite_steps=fin, device_vs_stepwise=diff)))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
