"""Workspace sizes of the scene engine (both variable-N models) for a table of inputs, as a library build returns them:
    python tools/dyn_workspace_sizes.py [--lib PATH] [--out tests/golden/dyn_workspace_sizes.json]
Host arithmetic only (no GPU).  The committed fixture was written from the build BEFORE the two models' host drivers were
merged; tests/test_dyn_workspace_sizes.py holds every later build to it, entry by entry."""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# (field_hidden, encoder_hidden, rnn_hidden, prior_layers, prior_hidden, num_edge_types, decoder_hidden, skip_first)
CONFIGS = ((64, 128, 64, 3, 64, 3, 128, 1), (256, 256, 64, 1, 0, 2, 256, 0), (64, 128, 64, 1, 0, 2, 128, 1),
           (256, 256, 64, 3, 64, 4, 128, 0), (64, 128, 64, 3, 64, 4, 256, 1), (256, 128, 64, 1, 0, 3, 128, 0))
FUNCTIONS = ("aether_dyn_step_workspace_bytes", "aether_dyn_step_batched_workspace_bytes", "aether_dyn_rollout_workspace_bytes",
             "aether_dyn_rollout_batched_workspace_bytes", "aether_dyn_dnri_step_batched_workspace_bytes",
             "aether_dyn_dnri_rollout_batched_workspace_bytes", "aether_dyn_field_workspace_bytes",
             "aether_dyn_prior_workspace_bytes", "aether_dyn_decoder_workspace_bytes", "aether_dyn_dnri_prior_workspace_bytes",
             "aether_dyn_dnri_decoder_workspace_bytes", "aether_knn_workspace_bytes")
KNN_K = 10


def cases():
    """-> list of (config index, object rows, scenes, in_degree mode ('one' | 'knn'), steps, all_empty)."""
    out = []
    for n_max in (2, 5, 9, 20):
        for B in (1, 2, 6, 256):
            for mode in ("one", "knn"):
                for steps in (1, 3):
                    i = len(out)
                    out.append(((i + i // len(CONFIGS)) % len(CONFIGS), n_max, B, mode, steps, False))
    out += [(0, 9, 2, "knn", 1, True), (1, 20, 256, "one", 3, True)]               # nobody anywhere, at every step
    return out


def counts(n_max, B, steps, all_empty):
    """Present objects [steps][B]: a full scene, an empty one, two objects and sizes between, rotated from step to step; the
    middle step of three is empty everywhere (the step's all-empty branch inside a rollout)."""
    pattern = (n_max, 0, 2, max(2, n_max // 2), max(2, n_max - 1))
    return [[0 if all_empty or (steps == 3 and t == 1) else pattern[(b + t) % len(pattern)] for b in range(B)]
            for t in range(steps)]


def measure(lib, case):
    """The twelve sizes of one case, in the order of FUNCTIONS (0 where the entry refuses the input)."""
    from aether_amd.nn.dynamicvars.aether_dynamicvars import _DynStepConfig
    ci, n_max, B, mode, steps, all_empty = case
    fh, he, R, layers, ph, K, hd, skip = CONFIGS[ci]
    cfg = C.byref(_DynStepConfig(fh, he, R, layers, ph, K, hd, skip, 0, 0, KNN_K, 0.5))
    n = counts(n_max, B, steps, all_empty)
    k = lambda v: min(KNN_K, n_max - 1, v - 1)
    e = [[v * k(v) if v else 0 for v in row] for row in n]
    deg = [[(1 if mode == "one" else k(v)) if v else 0 for v in row] for row in n]
    i64 = lambda rows: (C.c_int64 * (len(rows) * B))(*[v for row in rows for v in row])
    i32 = lambda rows: (C.c_int * (len(rows) * B))(*[v for row in rows for v in row])
    one = lambda rows: (C.c_int64 * len(rows))(*[row[0] for row in rows])              # scene 0 alone, step by step
    nt, et = max(sum(n[0]), 1), max(sum(e[0]), 1)                                        # the stages refuse empty inputs
    return [lib.aether_dyn_step_workspace_bytes(cfg, n_max, n[0][0], e[0][0]),
            lib.aether_dyn_step_batched_workspace_bytes(cfg, B, n_max, i64(n[:1]), i64(e[:1]), i32(deg[:1])),
            lib.aether_dyn_rollout_workspace_bytes(cfg, n_max, steps, one(n), one(e)),
            lib.aether_dyn_rollout_batched_workspace_bytes(cfg, B, n_max, steps, i64(n), i64(e), i32(deg)),
            lib.aether_dyn_dnri_step_batched_workspace_bytes(cfg, B, n_max, i64(n[:1]), i64(e[:1]), i32(deg[:1])),
            lib.aether_dyn_dnri_rollout_batched_workspace_bytes(cfg, B, n_max, steps, i64(n), i64(e), i32(deg)),
            lib.aether_dyn_field_workspace_bytes(nt, fh), lib.aether_dyn_prior_workspace_bytes(he, R, ph, nt, et),
            lib.aether_dyn_decoder_workspace_bytes(hd, nt, et), lib.aether_dyn_dnri_prior_workspace_bytes(he, R, ph, nt, et),
            lib.aether_dyn_dnri_decoder_workspace_bytes(hd, K, nt, et),
            lib.aether_knn_workspace_bytes(B, n_max, min(KNN_K, n_max - 1))]


def table(lib):
    return {"functions": list(FUNCTIONS), "configs": [list(c) for c in CONFIGS],
            "cases": [{"case": list(c), "sizes": measure(lib, c)} for c in cases()]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of the library (default: the package's)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "dyn_workspace_sizes.json"))
    a = ap.parse_args()
    from aether_amd import _lib
    t = table(_lib.load(a.lib))
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": {json.dumps(t[k])}' for k in ("functions", "configs")) + ',\n "cases": [\n'
                + ",\n".join("  " + json.dumps(c) for c in t["cases"]) + "\n ]\n}\n")
    print(f"{len(t['cases'])} cases x {len(FUNCTIONS)} sizes -> {a.out}")
