#!/usr/bin/env python3
"""Time the two graph-view builders -- aether_graph_build (two library radix sorts) and aether_graph_build_counting
(csrc/graph_build.h) -- on edge indices that are resident on the device: config 1 (B = 1, N = 5), config 2 (B = 128,
N = 20) and 64 kNN scenes (k = 10, N ~ U{2..40}) concatenated into one variable-topology batch.

Per builder and size: the median of --builds builds after --warmup warm-ups, each build between two HIP events (a build
ends with a stream synchronise, so the host clock around it is printed as well: it includes the call's host work).
The builders alternate inside one loop, so both see the same machine state.  The two views are compared first."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aether_amd import _lib
from aether_amd.knn import get_knn_graph_info
from aether_amd.synthetic import make_batch

ENTRIES = ("aether_graph_build", "aether_graph_build_counting")


def knn_batch(n_scenes=64, k=10, seed=0):
    g = torch.Generator().manual_seed(seed)
    sends, recvs, off = [], [], 0
    for n in torch.randint(2, 41, (n_scenes,), generator=g).tolist():
        x = (torch.randn(n, 2, generator=g) * 20).cuda()
        s, r = get_knn_graph_info(x, torch.ones(n, device="cuda"), num_vars=n, k=k)
        sends.append(s + off); recvs.append(r + off)
        off += n
    return torch.cat(sends).contiguous(), torch.cat(recvs).contiguous(), off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--builds", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if a.builds < 50 or a.warmup < 10:
        ap.error("at least 50 builds after at least 10 warm-ups")
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    cases = []
    for label, B, N in (("config 1 (B1 N5)", 1, 5), ("config 2 (B128 N20)", 128, 20)):
        send, recv = (e.cuda().contiguous() for e in make_batch(B, N, 2, seed=0)["edges"])
        cases.append((label, send, recv, B * N))
    cases.append(("64 kNN scenes (k 10, N 2..40)",) + knn_batch())
    print("%-32s %8s %8s  %-28s %10s %10s" % ("graph", "nodes", "edges", "builder", "event ms", "host ms"))
    for label, send, recv, n in cases:
        E = send.numel()
        nbytes = lib.aether_graph_bytes(E, n)
        bufs = {e: torch.empty(nbytes, dtype=torch.uint8, device="cuda") for e in ENTRIES}
        info = _lib.AetherGraphInfo()

        def build(entry):
            _lib.check(getattr(lib, entry)(send.data_ptr(), recv.data_ptr(), E, n, bufs[entry].data_ptr(), nbytes,
                                           C.byref(info), stream), entry)

        perms = {}
        for e in ENTRIES:
            build(e)
            perms[e] = torch.empty(E, dtype=torch.int32, device="cuda")
            _lib.check(lib.aether_graph_perm(bufs[e].data_ptr(), E, n, perms[e].data_ptr(), stream), "aether_graph_perm")
        torch.cuda.synchronize()
        if not torch.equal(perms[ENTRIES[0]], perms[ENTRIES[1]]):
            raise SystemExit(f"{label}: the two builders order the edges differently")
        ev = {e: [] for e in ENTRIES}
        host = {e: [] for e in ENTRIES}
        for it in range(a.warmup + a.builds):
            for e in ENTRIES:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                h0 = time.perf_counter()
                t0.record()
                build(e)
                t1.record()
                t1.synchronize()
                h1 = time.perf_counter()
                if it >= a.warmup:
                    ev[e].append(t0.elapsed_time(t1))
                    host[e].append((h1 - h0) * 1e3)
        for e in ENTRIES:
            print("%-32s %8d %8d  %-28s %10.4f %10.4f" % (label, n, E, e, statistics.median(ev[e]),
                                                          statistics.median(host[e])))
    print("median of %d builds after %d warm-ups; inputs resident" % (a.builds, a.warmup))


if __name__ == "__main__":
    main()
