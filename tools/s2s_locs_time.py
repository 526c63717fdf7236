#!/usr/bin/env python3
"""Time the fused step of the seq2seq LoCS baseline (aether_s2s_locs_rollout) against the plain seq2seq Aether's
(aether_s2s_rollout) at the same sizes: the two alternated block by block in one process, every block one device-side rollout
of --steps steps between two device synchronisations, medians over the blocks (the reference's configuration: hidden
512 / 512 / 64).  The spread of the Aether step in the same run (min / max over its blocks) is what a ratio is read against.

  --lib PATH          load that libaether_hip.so instead of the tree's (the parent commit's build, for the yardstick: with it
                      only the plain model is timed)
  --kernel-stats CSV  a rocprofv3 --kernel-trace --stats kernel_stats.csv of a run of this tool: adds the filter GEMM's time
                      per launch by feature count (11 / 24, 18 / 39) and the kernel launches per step
  --decoder ref_mlp   both models with the Markov decoder
Prints one JSON line per call (append it to profiles/s2s_locs_timing.jsonl)."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--dims", type=int, default=2)
ap.add_argument("--nodes", type=int, default=5)
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=15)
ap.add_argument("--lib", default=None)
ap.add_argument("--kernel-stats", default=None)
ap.add_argument("--decoder", choices=["recurrent", "ref_mlp"], default="recurrent")
ap.add_argument("--only", choices=["plain", "locs"], default=None, help="time one model only (kernel traces)")
a = ap.parse_args()

from aether_amd import _lib                                                # noqa: E402
if a.lib:
    _lib.load(a.lib)
from aether_amd.nn.seq2seq.aether import Aether                            # noqa: E402

D, N, B, T = a.dims, a.nodes, a.batch, a.steps
H, HD, R, K = 512, 512, 64, 2
params = {"num_vars": N, "input_size": 2 * D, "gpu": True, "decoder_hidden": HD, "num_edge_types": K, "skip_first": False,
          "decoder_dropout": 0.0, "use_3d": D == 3, "encoder_dropout": 0.0, "encoder_hidden": H, "encoder_rnn_hidden": R,
          "encoder_rnn_type": "lstm", "encoder_mlp_num_layers": 3, "encoder_mlp_hidden": 256, "prior_num_layers": 3,
          "prior_hidden_size": 256, "pos_representation": "polar", "gumbel_temp": 0.5, "rff_std": 1.0}
if a.decoder == "ref_mlp":
    params["decoder_type"] = "ref_mlp"
E = N * (N - 1)
torch.manual_seed(0)
x = torch.randn(B, N, 2 * D, device="cuda")
ps = (torch.zeros(B, E, R, device="cuda"), torch.zeros(B, E, R, device="cuda"))
U = torch.rand(T, B, E, K, device="cuda")
models = {}
if a.only != "locs":
    models["plain"] = Aether(params, device="cuda").eval()
if not a.lib and a.only != "plain":
    from aether_amd.nn.seq2seq.locs import LoCS
    models["locs"] = LoCS(params, device="cuda").eval()


def rollout(m):
    dh = torch.zeros(B, N, HD, device="cuda")
    return m._fused_rollout(None, x, dh, ps, T, U, False)


times = {k: [] for k in models}
for k, m in models.items():                                                # plan, workspaces, first-use costs
    rollout(m)
    rollout(m)
torch.cuda.synchronize()
for _ in range(a.blocks):
    for k, m in models.items():                                            # alternated
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rollout(m)
        torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) / T * 1e3)
out = {"tool": "s2s_locs_time", "dims": D, "nodes": N, "batch": B, "hidden": [H, HD, R], "decoder": a.decoder, "steps": T,
       "blocks": a.blocks, "lib": "parent build" if a.lib else "tree"}
for k, v in times.items():
    out[k + "_step_ms_median"] = round(statistics.median(v), 4)
    out[k + "_step_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
if len(times) == 2:
    out["ratio_locs_over_plain"] = round(statistics.median(times["locs"]) / statistics.median(times["plain"]), 4)
    out["plain_spread_rel"] = round((max(times["plain"]) - min(times["plain"])) / statistics.median(times["plain"]), 4)
if a.kernel_stats:
    # launches per step: the kernels a step launches are those launched a whole multiple of the traced run's step count
    # (2 warm-up rollouts + --blocks, the same --blocks as the traced run); plan and start-up kernels run once
    traced_steps, per_step, filt = (2 + a.blocks) * T, 0, {}
    for row in csv.DictReader(open(a.kernel_stats)):
        if int(row["Calls"]) % traced_steps == 0:
            per_step += int(row["Calls"]) // traced_steps
        m = re.search(r"k_s2s_filter_split(?:ILi|<)(\d+)", row["Name"])
        if m:
            filt[m.group(1)] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
    out["filter_kernel_by_features"] = filt
    out["kernel_launches_per_step"] = per_step
print(json.dumps(out))
