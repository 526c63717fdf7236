#!/usr/bin/env python3
"""Time the fused step of the seq2seq dNRI baseline (aether_s2s_dnri_rollout) against the seq2seq LoCS's (aether_s2s_locs_rollout,
code this model does not touch) at the same sizes, for both decoders and N = 5 and N = 20: the two models alternated block by
block in one process, every block one device-side rollout of --steps steps between two device synchronisations, medians over
the blocks (the reference's configuration: hidden 512 / 512 / 64, B = 128).  dNRI runs a subset of LoCS's stages -- no frames,
no edge attributes, no filter GEMM, no present messages -- so its step must not be slower than LoCS's beyond the run-to-run
spread of the LoCS measurement, which the same run gives as (max - min) / median over LoCS's blocks.

Prints one JSON line per (N, decoder) (append them to profiles/s2s_dnri_timing.jsonl)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--dims", type=int, default=2)
ap.add_argument("--nodes", type=int, nargs="+", default=[5, 20])
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=15)
ap.add_argument("--decoders", nargs="+", choices=["recurrent", "ref_mlp"], default=["recurrent", "ref_mlp"])
a = ap.parse_args()

from aether_amd.nn.seq2seq.dnri import DNRI                                # noqa: E402
from aether_amd.nn.seq2seq.locs import LoCS                                # noqa: E402

assert torch.cuda.is_available(), "timing needs an MI355X"
D, B, T = a.dims, a.batch, a.steps
H, HD, R, K = 512, 512, 64, 2
for N in a.nodes:
    for decoder in a.decoders:
        params = {"num_vars": N, "input_size": 2 * D, "gpu": True, "decoder_hidden": HD, "num_edge_types": K, "skip_first": False,
                  "decoder_dropout": 0.0, "use_3d": D == 3, "encoder_dropout": 0.0, "encoder_hidden": H, "encoder_rnn_hidden": R,
                  "encoder_rnn_type": "lstm", "encoder_mlp_num_layers": 3, "encoder_mlp_hidden": 256, "prior_num_layers": 3,
                  "prior_hidden_size": 256, "pos_representation": "polar", "gumbel_temp": 0.5}
        if decoder == "ref_mlp":
            params["decoder_type"] = "ref_mlp"
        E = N * (N - 1)
        torch.manual_seed(0)
        x = torch.randn(B, N, 2 * D, device="cuda")
        ps = (torch.zeros(B, E, R, device="cuda"), torch.zeros(B, E, R, device="cuda"))
        U = torch.rand(T, B, E, K, device="cuda")
        models = {"locs": LoCS(params, device="cuda").eval(), "dnri": DNRI(params, device="cuda").eval()}

        def rollout(m):
            dh = torch.zeros(B, N, HD, device="cuda")
            return m._fused_rollout(None, x, dh, ps, T, U, False)

        times = {k: [] for k in models}
        for m in models.values():                                          # plan, workspaces, first-use costs
            rollout(m)
            rollout(m)
        torch.cuda.synchronize()
        for _ in range(a.blocks):
            for k, m in models.items():                                    # alternated
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rollout(m)
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) / T * 1e3)
        out = {"tool": "s2s_dnri_time", "dims": D, "nodes": N, "batch": B, "hidden": [H, HD, R], "decoder": decoder, "steps": T,
               "blocks": a.blocks}
        for k, v in times.items():
            out[k + "_step_ms_median"] = round(statistics.median(v), 4)
            out[k + "_step_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        med = {k: statistics.median(v) for k, v in times.items()}
        out["ratio_dnri_over_locs"] = round(med["dnri"] / med["locs"], 4)
        out["locs_spread_rel"] = round((max(times["locs"]) - min(times["locs"])) / med["locs"], 4)
        out["dnri_not_slower_beyond_spread"] = bool(med["dnri"] <= med["locs"] * (1.0 + out["locs_spread_rel"]))
        print(json.dumps(out), flush=True)
        del models
