#!/usr/bin/env python3
"""Time one training step on a k-step rollout loss at cfg2 (2-D, N = 20, B = 128: 2,560 nodes, 48,640 edges), hidden 64,
for K = 4 and K = 20 (``--steps``), for ``Aether`` or -- ``--model dynamic_field_aether`` -- ``DynamicFieldAether`` (the latent
field recomputed, and differentiated, every step).

Rows (one JSON line each, ms per training step, median of `--reps` timed blocks of `--iters` steps between HIP events,
the device synchronised at the end of every block):
  graphed    GraphedRolloutTrainStep replay: rollout forward + loss + backward through time as one hipGraph, FusedAdamW
  eager      zero_grad, rollout_loss (differentiable_rollout), backward, FusedAdamW.step -- launched eagerly
  stepwise   the loop this replaces: K differentiable ``forward`` calls with the runner's torch ops in between
             (``rollout_stepwise`` without no_grad), ``mse_loss``, ``backward`` through autograd, the same optimizer

``--repo DIR`` imports the package from another checkout: the ``stepwise`` row uses nothing newer than ``forward``, so it
can be (and for the committed profile was) measured at the parent commit; rows a checkout cannot run are left out.
``--out FILE`` is written anew; the committed profile is the runs of both models, own checkout and parent, one after the other.

Usage: python tools/rollout_train_time.py [--model aether|dynamic_field_aether] [--steps 4 20] [--iters 50] [--reps 5]
       [--repo DIR] [--out FILE]
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
    ap.add_argument("--model", choices=["aether", "dynamic_field_aether"], default="aether")
    ap.add_argument("--steps", type=int, nargs="+", default=[4, 20])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    own = os.path.samefile(args.repo, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.abspath(args.repo))
    from aether_amd import _lib
    from aether_amd.nn.state2state.aether import Aether
    from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
    from aether_amd.optim import FusedAdamW
    from aether_amd.synthetic import make_batch

    B, N, D, dt = 128, 20, 2, 1.0
    dev = "cuda"
    b = make_batch(B, N, D, seed=2024, device=dev)
    x, vel, edges, q = b["x"], b["vel"], b["edges"], b["charges"]
    rows, cols = edges
    qprod = q[rows] * q[cols]

    dyn = args.model == "dynamic_field_aether"
    cls = DynamicFieldAether if dyn else Aether
    extra = {"num_nodes": N} if dyn else {}           # the objects per graph, as in DynamicFieldAether.forward
    fwd_extra = (N,) if dyn else ()

    def model():
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            return cls(2 * D, 64, 0.0, D, device=dev)

    has_new = hasattr(cls, "differentiable_rollout")
    if has_new and dyn:                                # a checkout from before the model's rollout training: "not built"
        try:
            model().differentiable_rollout(x, vel, edges, q, 1, dt, **extra)
        except _lib.AetherHipError as ex:
            if "not built" not in str(ex):
                raise
            has_new = False
    lines = []
    for K in args.steps:
        g = torch.Generator().manual_seed(K)
        # targets near a ballistic continuation: the size of the loss does not change what is launched
        tgt = torch.stack([x + vel * dt * (t + 1) for t in range(K)]) + 0.05 * torch.randn(K, *x.shape, generator=g).to(dev)
        base = dict(model=args.model, B=B, N=N, D=D, K=K, E=int(rows.numel()), hidden=64, device=torch.cuda.get_device_name(0),
                    iters=args.iters, reps=args.reps, checkout="own" if own else os.path.basename(os.path.abspath(args.repo)))
        res = []
        if has_new:
            from aether_amd.training import GraphedRolloutTrainStep
            step = GraphedRolloutTrainStep(model(), (x, vel, edges, q) + fwd_extra, tgt, dt=dt, lr=5e-4, weight_decay=1e-12)
            res.append(("graphed", timed(step.step, args.iters, args.reps)))
            step.check()
            del step
            from aether_amd.rollout import rollout_loss
            m = model()
            opt = FusedAdamW(m.parameters(), lr=5e-4, weight_decay=1e-12)

            def eager():
                opt.zero_grad(set_to_none=True)
                rollout_loss(m, x, vel, edges, q, tgt, dt, **extra).backward()
                opt.step()
            res.append(("eager", timed(eager, args.iters, args.reps)))
            del m, opt
        m = model()
        opt = FusedAdamW(m.parameters(), lr=5e-4, weight_decay=1e-12)

        def stepwise():
            opt.zero_grad(set_to_none=True)
            xt, vt, traj = x, vel, []
            for _ in range(K):
                dist = torch.sqrt(torch.sum((xt[rows] - xt[cols]) ** 2, 1)).unsqueeze(1)
                ea = torch.cat([qprod, dist], 1)
                xn = m(vt.norm(dim=-1, keepdim=True), xt, edges, vt, ea, q, *fwd_extra)
                vt = (xn - xt) / dt
                xt = xn
                traj.append(xt)
            torch.nn.functional.mse_loss(torch.stack(traj), tgt).backward()
            opt.step()
        res.append(("stepwise", timed(stepwise, args.iters, args.reps)))
        del m, opt
        torch.cuda.empty_cache()
        for what, (med, lo, hi) in res:
            lines.append(json.dumps(dict(base, what=what, ms_median=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
