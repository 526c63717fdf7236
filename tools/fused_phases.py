#!/usr/bin/env python3
"""Diagnostic: where does k_fused spend its time?  Builds the stamped library variant, runs the
headline workload and prints the median (over workgroups) time between phase stamps.
Run on the GPU box:  python tools/fused_phases.py [--dims 2] [--batch 128] [--nodes 20] [--lib STAMPED.so] [--opt name=value]"""
import argparse, contextlib, io, os, sys
import numpy as np
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from aether_amd import build as B, _lib
ap = argparse.ArgumentParser()
ap.add_argument("--dims", type=int, default=2); ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--nodes", type=int, default=20); ap.add_argument("--keep", action="store_true", help="time the save-for-backward variant")
ap.add_argument("--lib", default=None, help="a stamped library built beforehand (build.build_diagnostic) instead of building one")
ap.add_argument("--opt", action="append", default=[], help="name=value passed to aether_set_option (fused_waves12=0: the 8-wave kernel)")
a = ap.parse_args()
_lib.LIB_PATH = os.path.abspath(a.lib) if a.lib else B.build_diagnostic()
for kv in a.opt:
    _lib.check(_lib.load().aether_set_option(kv.split("=")[0].encode(), int(kv.split("=")[1])), "set_option")
from aether_amd.nn.state2state.aether import Aether
from aether_amd.synthetic import make_batch
torch.manual_seed(1)
with contextlib.redirect_stdout(io.StringIO()):
    m = Aether(2 * a.dims, 64, 0.0, a.dims, device="cuda")
inp = make_batch(a.batch, a.nodes, a.dims, seed=0, device="cuda")
if a.keep:
    m.flags = _lib.FLAG_KEEP_INTERMEDIATES
Nn, E = inp["x"].shape[0], inp["edges"][0].numel()
with torch.no_grad():
    for _ in range(20):
        m(inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"], inp["charges"])
torch.cuda.synchronize()
G = m.prepare_graph(inp["edges"], Nn)[1].n_groups
dst = torch.zeros(4096, 512, device="cuda")
lib = _lib.load()
_lib.check(lib.aether_debug_fetch(b"stamps", a.dims, Nn, E, m._last_ws.data_ptr(), dst.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream), "fetch stamps")
torch.cuda.synchronize()
st = dst.cpu().numpy()[:min(G, 4096)]
med = np.median(st, axis=0)
names = {0: "entry", 1: "w1 staged (issued)", 2: "field+frames+x0", 3: "edge features", 40: "out mlp + store"}
for l in range(4):
    b = 4 + 8 * l
    names[b + 2] = f"L{l+1} edge tiles (wave 0 done)"
    names[b + 3] = f"L{l+1} barrier (all tiles done)"
    names[b + 7] = f"L{l+1} n = x + mean"
    names[b + 4] = f"L{l+1} u = silu(W3 n)"
    names[b + 5] = f"L{l+1} x = n + W4 u"
    names[b + 6] = f"L{l+1} P_s, P_r"
prev = 0.0
print(f"groups={G}  (median over workgroups, microseconds)")
order = [0, 1, 2, 3] + [4 + 8 * l + o for l in range(4) for o in (2, 3, 7, 4, 5, 6)] + [40]
for k in order:
    if med[k] == 0 and k != 0:
        continue
    print(f"  {names[k]:32s} t={med[k]:8.2f}  d={med[k]-prev:7.2f}")
    prev = med[k]
clk = np.median(st[:, 41] / st[:, 40])
print(f"  shader clock during the kernel: {clk:.0f} MHz (s_memtime cycles / wall us)")
pv = med[400:409]                 # FUSED_PSTAMP: the field wave (wave 0) inside "field+frames+x0", cycles since entry
us = lambda c: c / clk
if pv[4] > 0:                     # 8-wave kernels: the field wave builds the frame and x0 itself
    print("  field wave (wave 0), cycles since kernel entry (microseconds at the shader clock):")
    for name, t0, t1 in (("entry -> first vector load issued", 0.0, pv[0]), ("-> vmcnt(0) passed", pv[0], pv[1]),
                         ("-> last MFMA of the field net", pv[1], pv[2]), ("-> frame stored", pv[2], pv[3]),
                         ("-> x0 stored", pv[3], pv[4])):
        print(f"   {name:36s} t={t1:7.0f}  d={t1 - t0:6.0f}  ({us(t1 - t0):5.2f} us)")
    print(f"   -> barrier behind P1 (thread 0)      t={med[2] * clk:7.0f}  d={med[2] * clk - pv[4]:6.0f}  ({med[2] - us(pv[4]):5.2f} us)")
elif pv[3] > 0:                   # 12-wave kernels: force alone; frames on wave 2 (FUSED_PSTAMP_W 5, 6), x0 on wave 4 (7, 8)
    print("  field wave (wave 0), cycles since kernel entry (microseconds at the shader clock):")
    for name, t0, t1 in (("entry -> first vector load issued", 0.0, pv[0]), ("-> vmcnt(0) passed", pv[0], pv[1]),
                         ("-> last MFMA of the field net", pv[1], pv[2]), ("-> force stored", pv[2], pv[3])):
        print(f"   {name:36s} t={t1:7.0f}  d={t1 - t0:6.0f}  ({us(t1 - t0):5.2f} us)")
    print(f"   -> barrier behind P1 (thread 0)      t={med[2] * clk:7.0f}  d={med[2] * clk - pv[3]:6.0f}  ({med[2] - us(pv[3]):5.2f} us)")
    print("  frame wave of node tile 0 (wave 2), beside the field net:")
    print(f"   entry -> x, vel landed               t={pv[5]:7.0f}  d={pv[5]:6.0f}  ({us(pv[5]):5.2f} us)")
    print(f"   -> frames stored                     t={pv[6]:7.0f}  d={pv[6] - pv[5]:6.0f}  ({us(pv[6] - pv[5]):5.2f} us)"
          f"   ({us(pv[3] - pv[6]):5.2f} us before the force)")
    print("  x0 wave of row block 0 (wave 4), behind the P1 barrier, beside the feature build:")
    print(f"   behind the barrier                   t={pv[7]:7.0f}")
    print(f"   -> x0 rows stored                    t={pv[8]:7.0f}  d={pv[8] - pv[7]:6.0f}  ({us(pv[8] - pv[7]):5.2f} us)"
          f"   (edge features, thread 0: {med[3] - med[2]:5.2f} us)")
print("  layer-2 per-wave tile timeline, cycles since kernel entry (median over workgroups):")
print("   wave round   start  wait rows  gemm1+silu1  gemm2+silu2+stage  sums   | total   [gemm1 | wait rows + receive | late add + silu1]")
sums = []
for w in range(12):            # 8 or 12 waves per workgroup (FUSED_WSTAMP: 24 slots per wave from slot 64, 64 + 24 * 12 <= FUSED_STAMPS)
    for r in range(3):
        v = med[64 + w * 24 + r * 8: 64 + w * 24 + r * 8 + 6]
        if v[5] == 0: continue
        d = [v[1] - v[0], v[2] - v[1], v[4] - v[2], v[5] - v[4]]      # stamps 0, 1, 2, 4 (tile parked, sums begin), 5
        sums.append(d[3])
        # stamp 3: first GEMM done; FUSED_WSTAMP_ROWS (slot 352 + 4 wave + round): rows there, tiles with a partner sender only
        rows = med[352 + 4 * w + r]
        late = f"   [{v[3]-v[1]:5.0f} | {rows-v[3]:5.0f} | {v[2]-rows:5.0f}]" if v[3] > 0 and rows > 0 else \
               f"   [{v[3]-v[1]:5.0f} |     - | {v[2]-v[3]:5.0f}]" if v[3] > 0 else ""
        print(f"   {w:4d} {r:5d} {v[0]:8.0f} {d[0]:9.0f} {d[1]:12.0f} {d[2]:18.0f} {d[3]:6.0f}    | {v[5]-v[0]:6.0f}{late}")
early = [(w, med[64 + w * 24 + 8], med[64 + w * 24 + 9]) for w in range(12)]     # FUSED_WSTAMP(2, 0, 8 / 9): 12-wave kernels only
if any(t1 > 0 for _, _, t1 in early):
    # the window a wave multiplies in, from the stamps themselves: thread 0's wall-clock stamps of layer 1's node phase
    # (post-edge barrier, n complete, u complete, step 3's barrier, closing barrier) against the product's first cycle
    b = 4
    edges = [("step 1", med[b + 3], med[b + 7]), ("step 2", med[b + 7], med[b + 4]), ("step 3", med[b + 4], med[b + 5]),
             ("step 4", med[b + 5], med[b + 6])]
    print("  layer 2's W_e e product under layer 1's node phase, cycles since kernel entry (window: the step whose barriers enclose its start):")
    groups = {}
    for w, t0, t1 in early:
        if t1 > 0:
            win = next((name for name, lo, hi in edges if lo * clk - 200 <= t0 < hi * clk - 200), "?")
            groups.setdefault(win, []).append(t1 - t0)
            print(f"   wave {w:2d}: {t0:8.0f} .. {t1:8.0f}  ({t1 - t0:5.0f})  {win}")
    for win, cyc in sorted(groups.items()):
        print(f"   {win}'s window: {len(cyc)} waves, product {min(cyc):.0f} .. {max(cyc):.0f} cycles (median {np.median(cyc):.0f})")
for w in range(12):            # the wave that copies the partner's rows (split groups): slots 6, 7 of its first round
    v = med[64 + w * 24: 64 + w * 24 + 8]
    if v[6] > 0:
        print(f"  partner-row receive on wave {w}: flag seen at {v[6]:.0f}, rows published at {v[7]:.0f} (copy {v[7]-v[6]:.0f} cycles)")
if sums:
    print(f"  receiver sums per tile (wait for the parked tile, column reads, adds, stores): median {np.median(sums):.0f}, "
          f"min {min(sums):.0f}, max {max(sums):.0f} cycles over {len(sums)} tiles")
print(f"  kernel span (max over WGs of last stamp): {st[:, 40].max():.2f} us; min start->end {st[:,40].min():.2f}")
