#!/usr/bin/env python3
"""Time the fused step of the seq2seq ablation DNRIAether (aether_s2s_dnri_aether_step / _rollout) next to the two models it
joins -- dNRI (aether_s2s_dnri_*) and Aether (aether_s2s_* / aether_s2s_markov_*) -- at the reference's own shape (N = 5,
B = 128, hidden 512 / 512 / 128), for both decoders: the models alternated block by block in one process, every block one
device-side rollout of --steps steps (or --steps eager single steps) between two device synchronisations, medians over the
blocks.  Also timed: the DNRIAether step with the field handed in (no field launch: what is left is the dNRI step on 3D
columns) and the field query alone (aether_s2s_field, the four launches the field adds to a step: Fourier features and three
layers).  The expectation from the code: DNRIAether's step costs dNRI's plus the field query's launches and nothing else.

Prints one JSON line per decoder (append them to profiles/s2s_dnri_aether_timing.jsonl)."""
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
ap.add_argument("--nodes", type=int, default=5)
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--blocks", type=int, default=15)
ap.add_argument("--decoders", nargs="+", choices=["recurrent", "ref_mlp"], default=["recurrent", "ref_mlp"])
a = ap.parse_args()

from aether_amd.nn.seq2seq.ablations.dnri_aether import DNRIAether         # noqa: E402
from aether_amd.nn.seq2seq.aether import Aether                            # noqa: E402
from aether_amd.nn.seq2seq.dnri import DNRI                                # noqa: E402

assert torch.cuda.is_available(), "timing needs an MI355X"
D, B, T, N = a.dims, a.batch, a.steps, a.nodes
H, HD, R, K = 512, 512, 128, 2
E = N * (N - 1)
for decoder in a.decoders:
    params = {"num_vars": N, "input_size": 2 * D, "gpu": True, "decoder_hidden": HD, "num_edge_types": K, "skip_first": False,
              "decoder_dropout": 0.0, "use_3d": D == 3, "encoder_dropout": 0.0, "encoder_hidden": H, "encoder_rnn_hidden": R,
              "encoder_rnn_type": "lstm", "encoder_mlp_num_layers": 3, "encoder_mlp_hidden": 256, "prior_num_layers": 3,
              "prior_hidden_size": 256, "pos_representation": "polar", "gumbel_temp": 0.5, "rff_std": 1.0}
    if decoder == "ref_mlp":
        params["decoder_type"] = "ref_mlp"
    torch.manual_seed(0)
    x = torch.randn(B, N, 2 * D, device="cuda")
    ps = (torch.zeros(B, E, R, device="cuda"), torch.zeros(B, E, R, device="cuda"))
    dh = torch.zeros(B, N, HD, device="cuda")
    U = torch.rand(T, B, E, K, device="cuda")
    models = {"dnri": DNRI(params, device="cuda").eval(), "dnri_aether": DNRIAether(params, device="cuda").eval(),
              "aether": Aether(params, device="cuda").eval()}
    field = models["dnri_aether"].predict_field(x)[0]

    def eager(m, **kw):                                                     # T single steps on the same state
        for t in range(T):
            m._fused_step(x, dh, ps, U[t], **kw)

    runs = {k + "_rollout": (lambda m=m: m._fused_rollout(None, x, dh, ps, T, U, False)) for k, m in models.items()}
    runs.update({k + "_step": (lambda m=m: eager(m)) for k, m in models.items()})
    runs["dnri_aether_step_field_given"] = lambda: eager(models["dnri_aether"], field=field)
    runs["field_query"] = lambda: [models["dnri_aether"].predict_field(x) for _ in range(T)]
    times = {k: [] for k in runs}
    for run in runs.values():                                              # plan, workspaces, first-use costs
        run()
        run()
    torch.cuda.synchronize()
    for _ in range(a.blocks):
        for k, run in runs.items():                                        # alternated
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / T * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {"tool": "s2s_dnri_aether_time", "dims": D, "nodes": N, "batch": B, "hidden": [H, HD, R], "decoder": decoder, "steps": T,
           "blocks": a.blocks}
    for k, v in times.items():
        out[k + "_ms_median"] = round(med[k], 4)
        out[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    out["rollout_ratio_over_dnri"] = round(med["dnri_aether_rollout"] / med["dnri_rollout"], 4)
    out["rollout_ratio_over_aether"] = round(med["dnri_aether_rollout"] / med["aether_rollout"], 4)
    out["rollout_ms_over_dnri"] = round(med["dnri_aether_rollout"] - med["dnri_rollout"], 4)
    out["rollout_ms_over_dnri_plus_field_query"] = round(med["dnri_aether_rollout"] - med["dnri_rollout"] - med["field_query"], 4)
    out["dnri_rollout_spread_rel"] = round((max(times["dnri_rollout"]) - min(times["dnri_rollout"])) / med["dnri_rollout"], 4)
    print(json.dumps(out), flush=True)
    del models, runs
