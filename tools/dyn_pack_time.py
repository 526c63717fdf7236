#!/usr/bin/env python3
"""Host share of the variable-N family's ``predict_future`` at BASELINE config 4 (64 scenes x 20 object rows x 50 frames):
the list path (``predict_future`` on per-scene, per-frame Python lists, as the reference's data set hands them over)
against ``predict_future_packed`` on a device-built ``ScenePack``, on the same scenes; the list build, the pack build and
the metric call are reported separately.

Rows (one JSON line each, appended to --out): ms per call, median with range over ``--reps`` timed blocks of ``--iters``
calls; ``wall`` = host clock around the calls ending in a device synchronise, ``device`` = HIP events around the same
calls.  The two predict paths alternate inside every block (other work shares the host).  Every shape is warmed up first.
Before anything is timed the two paths are held to each other on the timed scenes with the same Gumbel draws (bit-equal).

Usage:  python tools/dyn_pack_time.py [--reps 7] [--iters 3] [--out profiles/dyn_pack_timing.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from aether_amd import _lib                                                             # noqa: E402
from aether_amd.knn import get_knn_graph_info                                           # noqa: E402
from aether_amd.nn.dynamicvars.aether_dynamicvars import AetherDynamicVars, pack_scenes  # noqa: E402

MP = {"input_size": 4, "gpu": True, "decoder_hidden": 256, "num_edge_types": 4, "skip_first": True, "decoder_dropout": 0.0,
      "pos_representation": "cart", "no_encoder_bn": False, "encoder_dropout": 0.0, "encoder_hidden": 256,
      "encoder_rnn_hidden": 64, "encoder_rnn_type": "lstm", "encoder_mlp_num_layers": 3, "encoder_mlp_hidden": 128,
      "prior_num_layers": 3, "prior_hidden_size": 128, "encoder_normalize_mode": "normalize_all", "train_data_len": 50,
      "field_hidden": 256, "gumbel_temp": 0.5}
B, T, N = 64, 50, 20


def scenes(seed=7):
    """Tracks enter and leave: every object row is present over one span of frames; at least two objects in every frame."""
    g = torch.Generator().manual_seed(seed)
    inputs = torch.randn(B, T, N, 4, generator=g)
    masks = torch.zeros(B, T, N)
    for b in range(B):
        masks[b, :, :2] = 1
        for j in range(2, int(torch.randint(2, N + 1, (1,), generator=g))):
            lo = int(torch.randint(0, T - 5, (1,), generator=g))
            masks[b, lo:lo + int(torch.randint(5, T, (1,), generator=g)), j] = 1
    burn = torch.zeros(B, T, N)
    burn[:, :10] = masks[:, :10]
    return inputs.cuda(), masks.cuda(), burn.cuda()


def host_lists(inputs, masks):
    """What the reference's data set does per scene and per frame (single_ind_data.py:70-89), with this project's kNN call."""
    node_inds, graph_info = [], []
    for b in range(B):
        ni_b, gi_b = [], []
        for t in range(T):
            ni_b.append(masks[b, t].nonzero()[:, -1])
            nv = int(ni_b[-1].numel())
            send, recv = get_knn_graph_info(inputs[b, t], masks[b, t], nv)
            gi_b.append((send, recv, torch.argsort(recv, stable=True).view(-1, min(10, nv - 1))))
        node_inds.append(ni_b); graph_info.append(gi_b)
    return node_inds, graph_info


def blocks(fns, iters, reps):
    """{name: ([wall ms per call per block], [device ms per call per block])}; the functions alternate inside a block."""
    out = {k: ([], []) for k in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            for _ in range(iters):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            out[name][0].append((time.perf_counter() - t0) * 1e3 / iters)
            out[name][1].append(ev[0].elapsed_time(ev[1]) / iters)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dyn_pack_timing.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dyn_pack_time: no GPU; nothing is measured without one")
    lib = _lib.load()
    model = AetherDynamicVars(dict(MP), device="cuda").eval()
    inputs, masks, burn = scenes()
    node_inds, graph_info = host_lists(inputs, masks)
    pack = pack_scenes(inputs, masks)
    n, e, _ = pack.counts()
    K = MP["num_edge_types"]
    # same draws, same result: the packed path is the list path
    g = torch.Generator(device="cuda").manual_seed(3)
    U = [[torch.rand(int(e[t, b]), K, device="cuda", generator=g) for b in range(B)] for t in range(T - 1)]
    a = model.predict_future_packed(inputs, masks, burn, pack, uniform=U)
    b = model.predict_future(inputs, masks, node_inds, graph_info, burn, uniform=U)
    if not torch.equal(a, b):
        sys.exit("dyn_pack_time: the packed and the list path disagree; not timing")
    S = T - 1
    need = lib.aether_dyn_eval_scratch_bytes(B, N, S)
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    acc = torch.zeros(4 * S, dtype=torch.float64, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    so = torch.tensor([1.0] * 4 + [0.0] * 4, device="cuda")
    truth = inputs[:, 1:].contiguous()
    stream = torch.cuda.current_stream().cuda_stream

    def metric():
        st = lib.aether_dyn_eval_accumulate(a.data_ptr(), truth.data_ptr(), 4, masks.data_ptr(), burn.data_ptr(), so.data_ptr(),
                                            so.data_ptr() + 16, None, 0, B, N, S, acc.data_ptr(), acc.data_ptr() + 3 * S * 8,
                                            stats.data_ptr(), scratch.data_ptr(), need, stream)
        _lib.check(st, "aether_dyn_eval_accumulate")

    fns = {"predict_future (host lists)": lambda: model.predict_future(inputs, masks, node_inds, graph_info, burn),
           "predict_future_packed": lambda: model.predict_future_packed(inputs, masks, burn, pack),
           "pack_scenes (device build of all graphs)": lambda: pack_scenes(inputs, masks),
           "aether_dyn_eval_accumulate": metric}
    for fn in fns.values():                                    # warm-up: every shape of the timed window
        fn(); fn()
    res = blocks(fns, args.iters, args.reps)
    res.update(blocks({"host list build (kNN, nonzero, argsort per scene and frame)": lambda: host_lists(inputs, masks)},
                      1, min(args.reps, 3)))
    base = dict(B=B, N=N, frames=T, steps=S, present_objects=int(n[:S].sum()), edges=int(e[:S].sum()),
                device=torch.cuda.get_device_name(0), iters=args.iters, reps=args.reps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for name, (wall, dev) in res.items():
            row = dict(base, what=name, wall_ms_median=round(statistics.median(wall), 3), wall_ms_min=round(min(wall), 3),
                       wall_ms_max=round(max(wall), 3), device_ms_median=round(statistics.median(dev), 3),
                       device_ms_min=round(min(dev), 3), device_ms_max=round(max(dev), 3), blocks=len(wall))
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
