#!/usr/bin/env python3
"""Time the seq2seq autoregressive step with the Markov decoder (decoder_type 'ref_mlp') against the recurrent one at the
same sizes: per step, the loop of per-module entry points (eager), the device rollout (aether_s2s_markov_rollout /
aether_s2s_rollout) and hipGraph replay of that rollout, plus the decoder half's algorithmic FLOP per step from the shapes.
One JSON line per (D, N, decoder); --rollout-only runs only the Markov device rollout of one size (for rocprofv3).

Usage: tools/s2s_markov_time.py [--dims 2 3] [--nodes 5 20] [--batch 128] [--decoder-hidden 512] [--steps 20]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aether_amd.nn.seq2seq.aether import Aether  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--dims", type=int, nargs="+", default=[2, 3])
ap.add_argument("--nodes", type=int, nargs="+", default=[5, 20])
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--decoder-hidden", type=int, default=512)
ap.add_argument("--edge-types", type=int, default=2)
ap.add_argument("--skip-first", action="store_true")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--rollout-only", action="store_true")
a = ap.parse_args()
B, hd, K, T, H, R = a.batch, a.decoder_hidden, a.edge_types, a.steps, 512, 128
ku = K - (1 if a.skip_first else 0)


def model(D, N, markov):
    params = {"num_vars": N, "input_size": 2 * D, "gpu": True, "decoder_hidden": hd, "num_edge_types": K,
              "skip_first": a.skip_first, "decoder_dropout": 0.0, "use_3d": D == 3, "encoder_dropout": 0.0,
              "encoder_hidden": H, "encoder_rnn_hidden": R, "encoder_rnn_type": "lstm", "encoder_mlp_num_layers": 3,
              "encoder_mlp_hidden": 256, "prior_num_layers": 3, "prior_hidden_size": 256,
              "pos_representation": "polar" if D == 2 else "cart", "gumbel_temp": 0.5, "rff_std": 1.0}
    if markov:
        params["decoder_type"] = "ref_mlp"
    torch.manual_seed(0)
    return Aether(params, device="cuda").eval()


def decoder_flop(D, N, markov):
    """Multiply-adds x 2 of the decoder half per step; hard samples: one h x h product per edge of a used type (every
    edge counted: the upper bound, reached without skip_first)."""
    O = D * (D - 1) // 2
    NF = 4 * D + O
    RF, EA = 3 * D + NF, 2 * NF + 3 * D
    Nn, E = B * N, B * N * (N - 1)
    out = 2 * Nn * hd * hd * 2 + 2 * Nn * hd * 2 * D                       # out_mlp
    if markov:
        return out + 2 * E * EA * hd + 2 * E * hd * hd + 2 * Nn * RF * hd   # lin1, lin2 (one type per edge), res1
    msg = 2 * Nn * hd * 2 * hd * ku + 2 * E * hd * hd                      # msg_fc1 (receiver | sender halves), msg_fc2
    pmsg = 2 * E * EA * hd + 2 * E * hd * hd                               # present_msg_fc1, _fc2
    gates = 3 * 2 * Nn * RF * hd + 3 * 2 * Nn * hd * hd + 3 * 2 * Nn * hd * hd   # input_*, present_*, hidden_*
    return out + msg + pmsg + gates


def timed(fn, reps=5):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


for D in a.dims:
    for N in a.nodes:
        E = N * (N - 1)
        x = torch.randn(B, N, 2 * D, device="cuda")
        ps = (torch.zeros(B, E, R, device="cuda"), torch.zeros(B, E, R, device="cuda"))
        U = torch.rand(T, B, E, K, device="cuda")
        for markov in ((True,) if a.rollout_only else (True, False)):
            m = model(D, N, markov)
            dh = None if markov else torch.zeros(B, N, hd, device="cuda")
            if a.rollout_only:
                t_roll = timed(lambda: m.predict_from_state(x, dh, ps, T, uniform=U)) / T
                print("rollout D=%d N=%d B=%d hd=%d steps=%d %.3f ms/step" % (D, N, B, hd, T, t_roll), flush=True)
                continue
            t_eager = timed(lambda: m.predict_from_state_stepwise(x, dh, ps, T, uniform=U), reps=3) / T
            t_roll = timed(lambda: m.predict_from_state(x, dh, ps, T, uniform=U)) / T
            t_graph = timed(lambda: m.predict_from_state(x, dh, ps, T, uniform=U, graph=True)) / T
            print(json.dumps({"decoder": "ref_mlp" if markov else "recurrent", "D": D, "N": N, "B": B, "decoder_hidden": hd,
                              "edge_types": K, "skip_first": a.skip_first, "ms_per_step_eager": round(t_eager, 4),
                              "ms_per_step_rollout": round(t_roll, 4), "ms_per_step_graph": round(t_graph, 4),
                              "decoder_gflop_per_step": round(decoder_flop(D, N, markov) / 1e9, 3)}), flush=True)
            del m
            torch.cuda.empty_cache()
