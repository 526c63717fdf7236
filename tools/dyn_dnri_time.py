#!/usr/bin/env python3
"""``DNRIDynamicVars.predict_future_packed`` against ``AetherDynamicVars.predict_future_packed`` on the SAME scene packs: the
variable-N family's baseline next to its model, which is the yardstick (its code is what it was before the baseline existed).

Sizes: one scene of 20 object rows, and BASELINE config 4 (64 scenes x 20 object rows), 50 frames each.  Protocol of
tools/dyn_pack_time.py: every shape is warmed up, then ``--reps`` blocks of ``--iters`` calls in which the two models alternate
(other work shares the host and the device); ms per step = ms per call / 49, median [min - max] over the blocks, ``wall`` = host
clock around the calls ending in a device synchronise, ``device`` = HIP events around the same calls.  The Aether leg's own
spread (max / min) is reported so that the ratio can be read against noise.  Launches per step: device activities (kernels,
and memset / memcpy nodes) of one call counted by torch.profiler, the same way for both models, divided by the 49 steps.  The
workspace bytes of both rollouts for the same sizes come from the library's size functions.

Usage:  python tools/dyn_dnri_time.py [--reps 7] [--iters 3] [--out profiles/dyn_dnri_timing.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
from aether_amd import _lib                                                             # noqa: E402
from aether_amd.nn.dynamicvars.aether_dynamicvars import AetherDynamicVars, pack_scenes  # noqa: E402
from aether_amd.nn.dynamicvars.dnri_dynamicvars import DNRIDynamicVars                   # noqa: E402
import dyn_pack_time as DP                                                              # noqa: E402

T, N = DP.T, DP.N


def launches(fn):
    """(kernels, all device activities) of one call of ``fn``."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if str(e.device_type).endswith("CUDA")]
    other = [e for e in dev if "memset" in e.name.lower() or "memcpy" in e.name.lower()]
    return len(dev) - len(other), len(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dyn_dnri_timing.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dyn_dnri_time: no GPU; nothing is measured without one")
    lib = _lib.load()
    torch.manual_seed(5)
    aether = AetherDynamicVars(dict(DP.MP), device="cuda").eval()
    dnri = DNRIDynamicVars(dict(DP.MP), device="cuda").eval()
    inputs, masks, burn = DP.scenes()
    S = T - 1
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for B in (1, DP.B):
        x, m, b = inputs[:B].contiguous(), masks[:B].contiguous(), burn[:B].contiguous()
        pack = pack_scenes(x, m)
        n, e, _ = pack.counts()
        fns = {"AetherDynamicVars": lambda: aether.predict_future_packed(x, m, b, pack),
               "DNRIDynamicVars": lambda: dnri.predict_future_packed(x, m, b, pack)}
        for fn in fns.values():
            out = fn(); fn()
            if not bool(torch.isfinite(out).all()):
                sys.exit("dyn_dnri_time: a prediction is not finite; not timing")
        res = DP.blocks(fns, args.iters, args.reps)
        cfg_a, cfg_d = aether._step_config(), dnri._step_config()
        size = (B, N, S, pack.n_present, pack.n_edges, pack.in_degree)
        ws = {"AetherDynamicVars": lib.aether_dyn_rollout_batched_workspace_bytes(C.byref(cfg_a), *size),
              "DNRIDynamicVars": lib.aether_dyn_dnri_rollout_batched_workspace_bytes(C.byref(cfg_d), *size)}
        try:
            count = {k: launches(fn) for k, fn in fns.items()}
        except Exception as exc:                               # the timing stands without the count; say why it is missing
            print(f"dyn_dnri_time: launch count not available ({type(exc).__name__}: {exc})", file=sys.stderr)
            count = {k: (None, None) for k in fns}
        base = dict(B=B, N=N, frames=T, steps=S, present_objects=int(n[:S].sum()), edges=int(e[:S].sum()),
                    device=torch.cuda.get_device_name(0), iters=args.iters, reps=args.reps)
        med = {k: statistics.median(v[1]) / S for k, v in res.items()}
        a_dev = res["AetherDynamicVars"][1]
        with open(args.out, "a") as f:
            for name, (wall, dev) in res.items():
                per = lambda v: round(v / S, 4)
                row = dict(base, what=name + ".predict_future_packed", wall_ms_per_step_median=per(statistics.median(wall)),
                           wall_ms_per_step_min=per(min(wall)), wall_ms_per_step_max=per(max(wall)),
                           device_ms_per_step_median=per(statistics.median(dev)), device_ms_per_step_min=per(min(dev)),
                           device_ms_per_step_max=per(max(dev)), blocks=len(wall), workspace_bytes=ws[name],
                           kernels_per_step=None if count[name][0] is None else round(count[name][0] / S, 2),
                           device_activities_per_step=None if count[name][1] is None else round(count[name][1] / S, 2))
                print(json.dumps(row), flush=True)
                f.write(json.dumps(row) + "\n")
            row = dict(base, what="ratio DNRIDynamicVars / AetherDynamicVars (device ms per step, medians)",
                       ratio=round(med["DNRIDynamicVars"] / med["AetherDynamicVars"], 4),
                       aether_spread_max_over_min=round(max(a_dev) / min(a_dev), 4),
                       workspace_ratio=round(ws["DNRIDynamicVars"] / ws["AetherDynamicVars"], 4))
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
