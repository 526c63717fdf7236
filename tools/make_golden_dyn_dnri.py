#!/usr/bin/env python3
"""Golden fixtures of the variable-N dNRI baseline from the imported reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (AETHER_REFERENCE, default /root/reference).  Imported, unmodified:
``nn.dynamicvars.dnri_dynamicvars.DNRIDynamicVars`` and ``experiments.ind.single_ind_data.get_knn_graph_info`` (the graph the
inD data set attaches to every frame).  Stand-ins as oracle/make_golden_dynamicvars.py uses them: the torch_scatter stand-in
of oracle/make_golden.py, the identity ``.cuda()``, ``MODEL_PARAMS`` and ``perturb_bn_``; parameters from the class's own
constructor under a fixed torch seed (the drop-in module creates the same tensors in the same order), and the seed, the
state_dict key list and a checksum of every tensor stored instead of the weights.  Writes tests/golden/dyn_dnri.npz, hidden
128 / rnn 64 / decoder 128, per case (prefix ``<case>.``):

  N9   9 slots, K = 3, skip_first, T = 6, burn-in ends after step 3, objects appearing and leaving (k = n - 1)
  N14  14 slots, 12-14 present, K = 2, k = 10 < n - 1: a true kNN graph; after burn-in the caller's graph (ground truth)
       differs from the encoder's (the model's own predictions)
  N3   3 slots, all present, 6 edges, no_encoder_bn
  N2   2 slots, one in-edge per object, divisor 1

Per case: inputs [1, T, Nmax, 4], masks, burn-in masks, the per-frame graphs, a non-zero initial LSTM state, one prior step
from it, one decoder step on the sample of its logits (one-hot) from a non-zero hidden state, and predict_future -- all in
fp32 (``ref.``) and after .double() under a float64 default dtype (``ref64.``).  The uniform draws are regenerated after the
call (same global seed); a noise seed is accepted only when every hard sample wins its race by MARGIN AND the fp64
restatement (tests/dyn_dnri_restatement.py) samples the same edge types everywhere, so that a difference in the samples can
only come from the code under test.  The seed of the one-step state is the first at which that step's sample is as clear and
the fp32 restatement's own update error against fp64 (tests/update_parity.py) is at least TYPICAL (cases N9 and N14, which
the update bar is held on): that floor is a maximum over the 28 / 48 elements of a case and spreads from 1.4e-8 to 3.3e-7
between seeds and by up to a factor 9 between two host CPUs on the same seed, with 1e-7 as its median -- a lucky 2e-8 says
nothing about a kernel held to 4 x of it (the CPU rule of tests/update_s2s_cases.py, decided without a
GPU).

Reruns reproduce the file bit for bit.   Usage:  python tools/make_golden_dyn_dnri.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("AETHER_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, REPO)

import make_golden as MG                      # noqa: E402  (torch_scatter stand-in)
from make_golden_dynamicvars import MODEL_PARAMS, perturb_bn_   # noqa: E402
from make_golden_s2s_locs import MARGIN, checksums, given_draws, min_margin, recorded_logits   # noqa: E402
from update_parity import update_floor      # noqa: E402

SEED = 8642
TAU = 0.5
TYPICAL = 1e-7                                # an update floor typical of this step: the median over seeds
UPDATE_CASES = ("N9", "N14")                  # the cases whose one-step prediction the update bar is held on (28 / 48 elements;
                                              # at the 12 / 8 elements of N3 / N2 the restatement's error is exactly 0 half the time)
CASES = {   # tag: (Nmax, K, skip_first, T, burn-in steps, no_encoder_bn)
    "N9": (9, 3, True, 6, 3, False),
    "N14": (14, 2, False, 5, 2, False),
    "N3": (3, 3, True, 4, 2, True),
    "N2": (2, 2, False, 4, 2, False),
}


def model_params(tag):
    _, K, skip, _, _, no_bn = CASES[tag]
    params = dict(MODEL_PARAMS)
    params.update({"encoder_hidden": 128, "encoder_rnn_hidden": 64, "decoder_hidden": 128, "num_edge_types": K,
                   "skip_first": skip, "no_encoder_bn": no_bn, "gumbel_temp": TAU})
    return params


def case_scene(ci, tag):
    """inputs [1, T, Nmax, 4], masks [1, T, Nmax], burn-in masks [1, T, Nmax] of the case."""
    Nmax, _, _, T, burn_steps, _ = CASES[tag]
    g = torch.Generator().manual_seed(5100 + ci)
    inputs = torch.randn(1, T, Nmax, 4, generator=g)
    masks = torch.ones(1, T, Nmax)
    if tag == "N9":                                      # objects appearing and leaving: 7-8 of 9 present
        masks[0, :2, 8] = 0; masks[0, 3:, 2] = 0; masks[0, 1:4, 5] = 0; masks[0, 4:, 7] = 0; masks[0, 0, 4] = 0
    elif tag == "N14":                                   # 12-14 of 14 present
        masks[0, 0, 13] = 0; masks[0, 0, 6] = 0; masks[0, 2:, 3] = 0; masks[0, 3, 9] = 0
    burn = torch.ones(1, T, Nmax)
    burn[:, burn_steps:] = 0
    return inputs, masks, burn


@contextlib.contextmanager
def reference():
    MG._install_scatter_standin()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import nn.dynamicvars.dnri_dynamicvars as L                      # noqa: WPS433 (reference import)
        from experiments.ind.single_ind_data import get_knn_graph_info   # noqa: WPS433
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield L, get_knn_graph_info
    finally:
        torch.Tensor.cuda = orig_cuda


def build_model(L, tag):
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        model = L.DNRIDynamicVars(model_params(tag)).eval()
    with torch.no_grad():
        perturb_bn_(model)
    return model


def one_step(model, x0, m0, ni0, gi0, state0, hidden0, z, dtype):
    """One prior step from ``state0`` and the decoder step on the sample z from ``hidden0``, in ``dtype``."""
    cast = lambda t: t.to(dtype)
    with contextlib.redirect_stdout(io.StringIO()):
        logits, (h1, c1) = model.encoder.single_step_forward(cast(x0), m0, ni0, gi0, (cast(state0[0]), cast(state0[1])))
        pred, hid = model.decoder(cast(x0), cast(hidden0), cast(z), m0, gi0)
    return {"logits": logits, "h1": h1, "c1": c1, "pred": pred, "hidden": hid}


def fixture(out, L, get_knn_graph_info, ci, tag):
    import dyn_dnri_restatement as RS
    from oracle import seq2seq_oracle as S
    Nmax, K, skip, T, _, _ = CASES[tag]
    model = build_model(L, tag)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    checksums(out, tag, sd)
    inputs, masks, burn = case_scene(ci, tag)
    node_inds = [[masks[0, t].nonzero()[:, -1] for t in range(T)]]
    graph_info = [[get_knn_graph_info(inputs[0, t], masks[0, t], int(masks[0, t].sum())) for t in range(T)]]
    E = [int(graph_info[0][t][0].numel()) for t in range(T)]
    rs64 = RS.Model(sd, torch.float64, 3, skip, TAU)
    for noise_seed in range(400):
        torch.manual_seed(8800 + noise_seed)
        with torch.no_grad(), recorded_logits(L) as seen:
            preds = model.predict_future(inputs, masks, node_inds, graph_info, burn)
        torch.manual_seed(8800 + noise_seed)
        U = [torch.rand(E[t], K) for t in range(T - 1)]
        if len(seen) != T - 1:
            continue
        m = min(min_margin(lg.reshape(-1, K), U[t], TAU) for t, lg in enumerate(seen))
        if m <= MARGIN:
            continue
        _, z64, _ = rs64.predict_future(inputs[0], masks[0], node_inds[0], graph_info[0], burn[0], [u.double() for u in U],
                                        return_all=True)
        zref = [S.gumbel_hard(lg.reshape(-1, K), U[t], TAU) for t, lg in enumerate(seen)]
        if all(torch.equal(a.argmax(-1), b.argmax(-1)) for a, b in zip(zref, z64)):
            break
    else:
        raise RuntimeError("no noise seed with unambiguous samples")
    slots = Nmax * (Nmax - 1)
    x0, m0, ni0, gi0 = inputs[:, 0], masks[:, 0], node_inds[0][0], graph_info[0][0]
    rs32 = RS.Model(sd, torch.float32, 3, skip, TAU)
    present = m0[0] != 0
    # The one-step state: the first seed at which the sample is clear and the fp32 restatement's own update error against fp64
    # (tests/update_parity.py: the floor the GPU test's bar is taken from) is typical, not a lucky small maximum over the few
    # elements of the case -- the CPU rule of tests/update_s2s_cases.py (TYPICAL), decided without a GPU.
    for state_seed in range(5200 + ci, 5200 + ci + 100 * 50, 100):
        g = torch.Generator().manual_seed(state_seed)
        state0 = (torch.randn(1, slots, 64, generator=g) * 0.2, torch.randn(1, slots, 64, generator=g) * 0.2)
        hidden0 = torch.randn(1, Nmax, 128, generator=g) * 0.3
        with torch.no_grad():
            s32 = one_step(model, x0, m0, ni0, gi0, state0, hidden0, torch.zeros(1, E[0], K), torch.float32)
        m0_margin = min_margin(s32["logits"].reshape(-1, K), U[0], TAU)
        if m0_margin <= MARGIN:
            continue
        z = S.gumbel_hard(s32["logits"].reshape(-1, K), U[0], TAU).view(1, E[0], K)
        w32, _ = rs32.decoder(x0[0], hidden0[0], z[0], m0[0], gi0)
        w64, _ = rs64.decoder(x0[0], hidden0[0], z[0], m0[0], gi0)
        floor = update_floor(w32[present], x0[0][present], w64[present])
        if floor >= TYPICAL or tag not in UPDATE_CASES:
            break
    else:
        raise RuntimeError("no one-step state with a clear sample and a typical floor")
    with torch.no_grad():
        s32 = one_step(model, x0, m0, ni0, gi0, state0, hidden0, z, torch.float32)
        m64 = model.double()
        torch.set_default_dtype(torch.float64)                      # (batch_edge2node's and the decoder's torch.zeros)
        try:
            s64 = one_step(m64, x0, m0, ni0, gi0, state0, hidden0, z, torch.float64)
            with given_draws(L, U):
                p64 = m64.predict_future(inputs.double(), masks, node_inds, graph_info, burn)
        finally:
            torch.set_default_dtype(torch.float32)
        model.float()
    z64_step = S.gumbel_hard(s64["logits"].reshape(-1, K), U[0].double(), TAU)
    assert torch.equal(z64_step.argmax(-1), z[0].argmax(-1))
    values = [preds, p64] + list(s32.values()) + list(s64.values())
    assert all(bool(torch.isfinite(v).all()) for v in values)
    assert float((p64 - preds.double()).abs().max()) <= 1e-3 * float(preds.abs().max()), "a sample flipped between fp32 and fp64"
    assert preds.shape == (1, T - 1, Nmax, 4)
    for k, v in (("in.inputs", inputs), ("in.masks", masks), ("in.burn", burn), ("in.state0_h", state0[0]),
                 ("in.state0_c", state0[1]), ("in.hidden0", hidden0), ("ref.step_edges", z), ("ref.predictions", preds),
                 ("ref64.predictions", p64)):
        out[f"{tag}.{k}"] = v.detach().numpy()
    for k, v in s32.items():
        out[f"{tag}.ref.{k}"] = v.detach().numpy()
    for k, v in s64.items():
        out[f"{tag}.ref64.{k}"] = v.detach().numpy()
    for t in range(T):
        out[f"{tag}.send.{t}"], out[f"{tag}.recv.{t}"], out[f"{tag}.e2n.{t}"] = (x.numpy() for x in graph_info[0][t])
        if t < T - 1:
            out[f"{tag}.uniform.{t}"] = U[t].numpy()
            out[f"{tag}.ref.edges.{t}"] = zref[t].numpy()
    out[f"{tag}.noise_seed"] = np.int64(8800 + noise_seed)
    out[f"{tag}.margin"] = np.float64(min(m, m0_margin))
    out[f"{tag}.state_seed"] = np.int64(state_seed)
    out[f"{tag}.update_floor"] = np.float64(floor)
    present = [int(masks[0, t].sum()) for t in range(T)]
    print(f"{tag}: {len(sd)} keys, present {present}, edges {E}, noise seed {8800 + noise_seed}, margin {min(m, m0_margin):.3g}, state seed {state_seed}, update floor {floor:.3g}")


def save_npz(path, out):
    """np.savez with fixed member timestamps: reruns reproduce the file bit for bit."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as zf:
        for name, value in out.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(value), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    torch.set_num_threads(1)                  # fixed reduction order: reruns reproduce the file bit for bit
    out = {"seed": np.int64(SEED), "hidden": np.int64(128), "rnn_hidden": np.int64(64), "cases": np.array(list(CASES))}
    with reference() as (L, get_knn_graph_info):
        for ci, tag in enumerate(CASES):
            fixture(out, L, get_knn_graph_info, ci, tag)
    save_npz(os.path.join(args.out, "dyn_dnri.npz"), out)
    print("wrote dyn_dnri.npz")


if __name__ == "__main__":
    main()
