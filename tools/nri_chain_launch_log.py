"""The job-table launches of the NRI host chain (prior, decoder, rollout of the seq2seq and the variable-N engines), call by
call, as a library build issues them:
    python tools/nri_chain_launch_log.py [--lib PATH] [--out tests/golden/nri_chain_launch_log.json]
Needs an MI355X (the calls run).  The committed fixture was written from the build BEFORE the host chains of csrc/host_*.inc
were merged into csrc/host_nri_chain.inc; tests/test_gpu_nri_chain_launches.py holds every later build to it, record for
record and in order.  A record is one s2s_launch_jobs launch (include/aether_hip.h, AetherS2SLaunchRecord)."""
import argparse
import ctypes as C
import functools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

FIELDS = ("kind", "jobs", "images", "wgs", "wg128", "min_n", "tiles64", "N", "M", "K", "K2")
S2S_CALLS = {"dnri_rec": ("step", "ext_logits", "encoder_features", "rollout"),
             "dnri_mlp": ("step", "ext_logits", "encoder_features", "rollout"), "aether_rec": ("step", "rollout")}
DYN_CALLS = ("prior_step", "decoder_step", "step_batched", "rollout_batched")


def cases():
    """-> list of (engine, model, size, call): the seq2seq models at 60 edge rows (fp32 job kernel, unfused cell) and at 2,280
    (the LSTM job on the split GEMM, the cell in its epilogue; one step), the variable-N dNRI on its two smallest fixture
    scenes (N3: no BatchNorm, skip_first; N2)."""
    out = [("s2s", kind, "small", call) for kind, calls in S2S_CALLS.items() for call in calls]
    out += [("s2s", kind, "e2280", "step") for kind in S2S_CALLS]
    out += [("dyn", "dnri", tag, call) for tag in ("N3", "N2") for call in DYN_CALLS]
    return out


def _cu(v):
    """Every tensor of a nested list / tuple on the device (the library is handed addresses: the modules check `x` only)."""
    if hasattr(v, "cuda"):
        return v.cuda()
    return type(v)(_cu(e) for e in v) if isinstance(v, (list, tuple)) else v


def _on_device(v):
    return v.is_cuda if hasattr(v, "is_cuda") else all(_on_device(e) for e in v) if isinstance(v, (list, tuple)) else True


@functools.lru_cache(maxsize=None)
def _s2s(kind, size):
    import update_s2s_cases as S2S
    case = (kind, 2, 61, 5) + (() if size == "small" else (size,))
    m = S2S.build(case, "cuda")
    g = {k: _cu(v) for k, v in S2S.inputs(case, m).items() if k not in ("gen", "rows")}
    assert _on_device(list(g.values()))
    return m, g


@functools.lru_cache(maxsize=None)
def _dyn(tag):
    import test_dyn_dnri as T
    model, _, d = T.build(tag, device="cuda")
    g = {k: _cu(v) for k, v in T.scene(d, tag).items()}
    assert _on_device(list(g.values()))
    return model, g


def _run_s2s(kind, size, call):
    m, g = _s2s(kind, size)
    state = (g["state"][0], g["state"][1])
    if call == "step":
        m._fused_step(g["x"], g["hidden"], state, g["u"])
    elif call == "ext_logits":                               # the decoder on given logits: the prior is skipped
        import torch
        logits = torch.randn(g["u"].shape, generator=torch.Generator().manual_seed(3)).cuda()
        m.single_step_forward(g["x"], g["hidden"], logits, True, uniform=g["u"])
    elif call == "encoder_features":
        m._encoder_forward(g["frames"])
    else:                                                    # one burn-in step, two predicted steps
        m.predict_future(g["frames"], 2, uniform=g["U"][:3])


def _run_dyn(tag, call):
    model, g = _dyn(tag)
    x0, m0 = g["inputs"][:, 0], g["masks"][:, 0]
    if call == "prior_step":
        model.encoder.single_step_forward(x0, m0, g["node_inds"][0], g["graph_info"][0], g["state0"])
    elif call == "decoder_step":
        model.decoder(x0, g["hidden0"], g["step_edges"], m0, g["graph_info"][0])
    elif call == "step_batched":
        ph, pc = model.encoder.get_initial_hidden(g["inputs"])
        dec = model.decoder.get_initial_hidden(g["inputs"])
        gs, gr, e2n = g["graph_info"][0]
        model._step_one_call(x0, m0, g["node_inds"][0], gs, gr, e2n, ph, pc, dec, g["uniform"][0])
    else:                                                    # two steps: three frames of the fixture scene
        model.predict_future(g["inputs"][:, :3].contiguous(), g["masks"][:, :3].contiguous(), [g["node_inds"][:3]],
                             [g["graph_info"][:3]], g["burn"][:, :3].contiguous(), uniform=g["uniform"][:2])


def measure(lib, case):
    """The launches of one call, in order -> (launches since the reset, [record as a list in the order of FIELDS]).  The call
    runs twice: the first makes the model's plan and workspaces, the second is logged."""
    import torch
    from aether_amd import _lib
    engine, model, size, call = case
    run = (lambda: _run_s2s(model, size, call)) if engine == "s2s" else (lambda: _run_dyn(size, call))
    lib.aether_set_option(b"gemm_split", 1)
    run()
    torch.cuda.synchronize()
    lib.aether_s2s_launch_stats_reset()
    run()
    torch.cuda.synchronize()
    st = _lib.AetherS2SLaunchStats()
    _lib.check(lib.aether_s2s_launch_stats(C.byref(st)), "aether_s2s_launch_stats")
    n = min(int(st.logged), _lib.S2S_LAUNCH_LOG)
    return int(st.logged), [[int(getattr(st.log[i], f)) for f in FIELDS] for i in range(n)]


def table(lib):
    rows = []
    for c in cases():
        logged, log = measure(lib, c)
        rows.append({"case": list(c), "logged": logged, "log": log})
    return {"fields": list(FIELDS), "cases": rows}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of the library (default: the package's)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "nri_chain_launch_log.json"))
    a = ap.parse_args()
    from aether_amd import _lib
    t = table(_lib.load(a.lib))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write('{\n "fields": ' + json.dumps(t["fields"]) + ',\n "cases": [\n'
                + ",\n".join("  " + json.dumps(c) for c in t["cases"]) + "\n ]\n}\n")
    print(f"{len(t['cases'])} calls, {sum(c['logged'] for c in t['cases'])} launches -> {a.out}")
