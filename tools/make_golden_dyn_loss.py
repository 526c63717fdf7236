#!/usr/bin/env python3
"""Golden fixtures of ``calculate_loss(is_train=False, return_logits=True)`` of both variable-N models from the imported
reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (AETHER_REFERENCE, as tools/make_golden_dyn_dnri.py).  Imported, unmodified:
``nn.dynamicvars.aether_dynamicvars.AetherDynamicVars``, ``nn.dynamicvars.dnri_dynamicvars.DNRIDynamicVars`` and
``experiments.ind.single_ind_data.get_knn_graph_info``.  Stand-ins, helpers and scenes are those of
tools/make_golden_dyn_dnri.py (torch_scatter stand-in, identity ``.cuda()``, ``MODEL_PARAMS``, ``perturb_bn_``, the cases N9 /
N14 / N3 / N2); parameters come from the class's own constructor under a fixed torch seed, and the seed, the key list and a
checksum of every tensor are stored instead of the weights (``refill_filters_``: the orthogonally initialised filter weights are
redrawn from a generator, so that every host recreates the same bits).  The loss flags are the inD runner's: normalize_nll, normalize_kl,
nll_loss_type 'gaussian', prior_variance 5e-5, teacher_forcing_steps -1.  Writes tests/golden/dyn_loss.npz, hidden 128 / rnn 64
/ decoder 128, per model (``aether`` | ``dnri``) and case (prefix ``<model>.<case>.``):

  N9, N14, N3, N2   as tools/make_golden_dyn_dnri.py (N3 with BatchNorm for the Aether model, whose drop-in takes no
                    no_encoder_bn); teacher-forced settings; N3 and N2 free-running too
  L7                7 slots, K = 3, skip_first, T = 5, everyone present in frame 0 and objects only LEAVE afterwards (2 after
                    frame 1, 5 after frame 2); teacher-forced and free-running

A setting is (teacher_forcing, use_prior_logits): ``tf1.post``, ``tf1.prior`` and, for N3 / N2 / L7, ``tf0.post``, ``tf0.prior``.
Free-running cases have no object that first appears after frame 0: such an object would enter the decoder with the all-zero
row of the previous prediction (a frame at atan2(0, 0)), which is reproduced but not held to parity.

Per case: inputs, masks, per-frame graphs, the uniform draws of every step, the prior / posterior logits; per setting the
predictions, the three loss values and the last step's edges -- in fp32 (``ref.``) and after .double() under a float64 default
dtype (``ref64.``) -- and ``rel32.<scalar>``: the reference's own fp32-vs-fp64 relative difference of each loss value.  The
draws reach the reference through a wrapper of ``gumbel_softmax`` that applies the pinned formula to them.  A noise seed is
accepted only when every hard sample (of the posterior AND the prior logits) wins its race by MARGIN and the fp64 restatement
(tests/dyn_loss_restatement.py) draws the same edge types everywhere, so a difference in a sample can only come from the code
under test.

Reruns reproduce the file bit for bit.   Usage:  python tools/make_golden_dyn_loss.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))

import make_golden_dyn_dnri as MD             # noqa: E402  (sets the other paths; CASES, case_scene, save_npz)
import make_golden as MG                      # noqa: E402  (torch_scatter stand-in)
from make_golden_dynamicvars import MODEL_PARAMS, perturb_bn_   # noqa: E402
from make_golden_s2s_locs import MARGIN, checksums, min_margin   # noqa: E402

SEED = 8642
TAU = 0.5
LOSS_FLAGS = {"normalize_nll": True, "normalize_kl": True, "nll_loss_type": "gaussian", "prior_variance": 5e-5,
              "teacher_forcing_steps": -1}
CASES = dict(MD.CASES)                        # tag: (Nmax, K, skip_first, T, burn-in steps (unused), no_encoder_bn)
CASES["L7"] = (7, 3, True, 5, 0, False)
FREE_RUNNING = ("N3", "N2", "L7")
MODELS = ("aether", "dnri")


def settings(tag):
    out = [(True, False), (True, True)]
    if tag in FREE_RUNNING:
        out += [(False, False), (False, True)]
    return out


def setting_name(tf, use_prior):
    return f"tf{int(tf)}.{'prior' if use_prior else 'post'}"


def model_params(kind, tag):
    _, K, skip, _, _, no_bn = CASES[tag]
    params = dict(MODEL_PARAMS)
    params.update({"encoder_hidden": 128, "encoder_rnn_hidden": 64, "decoder_hidden": 128, "num_edge_types": K, "skip_first": skip,
                   "no_encoder_bn": no_bn and kind == "dnri", "gumbel_temp": TAU})
    params.update(LOSS_FLAGS)
    return params


def refill_filters_(model):
    """The anisotropic filters' weights from a private generator, in place.  Their constructor fills them with
    ``nn.init.orthogonal_``, which goes through LAPACK's QR: its rounding differs between host CPUs and thread counts (1e-7
    relative), too much for a fixture that stores checksums instead of weights and is held to 1e-12.  Gaussian values of the
    same scale (an orthogonal [rows, cols] matrix with rows > cols has entries of variance 1 / rows; the first layer's gain is
    sqrt(2)) are the same bits everywhere.  The dNRI model has no such tensor."""
    g = torch.Generator().manual_seed(707)
    for name, p in model.named_parameters():
        if "edge_filter" in name and name.endswith("weight"):
            gain = 2.0 ** 0.5 if name.endswith("edge_filter.0.weight") else 1.0
            p.copy_(torch.randn(p.shape, generator=g) * (gain / max(p.shape) ** 0.5))


def case_scene(ci, tag):
    if tag != "L7":
        return MD.case_scene(ci, tag)[:2]
    Nmax, _, _, T, _, _ = CASES[tag]
    g = torch.Generator().manual_seed(5100 + ci)
    inputs = torch.randn(1, T, Nmax, 4, generator=g)
    masks = torch.ones(1, T, Nmax)
    masks[0, 2:, 2] = 0; masks[0, 3:, 5] = 0
    return inputs, masks


@contextlib.contextmanager
def reference():
    MG._install_scatter_standin()
    if MD.REF not in sys.path:
        sys.path.insert(0, MD.REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import nn.dynamicvars.aether_dynamicvars as LA                  # noqa: WPS433 (reference import)
        import nn.dynamicvars.dnri_dynamicvars as LD                    # noqa: WPS433
        from experiments.ind.single_ind_data import get_knn_graph_info   # noqa: WPS433
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield {"aether": (LA, LA.AetherDynamicVars), "dnri": (LD, LD.DNRIDynamicVars)}, get_knn_graph_info
    finally:
        torch.Tensor.cuda = orig_cuda


@contextlib.contextmanager
def sampling(L, U):
    """gumbel_softmax(hard=True) of the module on the draws U[call]; records (logits, sample) of every call."""
    from oracle import seq2seq_oracle as S
    orig, seen = L.gumbel_softmax, []

    def wrapper(logits, tau=1, hard=False, eps=1e-10):
        z = S.gumbel_hard(logits, U[len(seen)].to(logits.dtype), tau)
        seen.append((logits.detach().clone(), z.detach().clone()))
        return z

    L.gumbel_softmax = wrapper
    try:
        yield seen
    finally:
        L.gumbel_softmax = orig


def run(L, model, inputs, masks, node_inds, graph_info, U, tf, use_prior):
    with torch.no_grad(), sampling(L, U) as seen, contextlib.redirect_stdout(io.StringIO()):
        loss, nll, kl, post, preds = model.calculate_loss(inputs, masks, node_inds, graph_info, is_train=False, teacher_forcing=tf,
                                                          return_logits=True, use_prior_logits=use_prior)
    sampled = torch.cat([lg for lg, _ in seen])                       # the logits the loop decoded with, [sum E, K]
    return {"loss": loss, "nll": nll, "kl": kl, "posterior": post[0], "predictions": preds[0], "sampled": sampled,
            "edges": seen[-1][1], "samples": [z for _, z in seen]}


def fixture(out, kind, L, cls, get_knn_graph_info, ci, tag):
    import dyn_loss_restatement as RL
    Nmax, K, skip, T, _, _ = CASES[tag]
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        model = cls(model_params(kind, tag)).eval()
    with torch.no_grad():
        perturb_bn_(model)
        refill_filters_(model)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    pre = f"{kind}.{tag}"
    checksums(out, pre, sd)
    inputs, masks = case_scene(ci, tag)
    node_inds = [[masks[0, t].nonzero()[:, -1] for t in range(T)]]
    graph_info = [[get_knn_graph_info(inputs[0, t], masks[0, t], int(masks[0, t].sum())) for t in range(T)]]
    E = [int(graph_info[0][t][0].numel()) for t in range(T - 1)]
    rs64 = RL.Model(kind, sd, torch.float64, skip, TAU)
    prior64, post64 = rs64.encode(inputs[0, :-1], masks[0, :-1])
    for noise_seed in range(400):
        g = torch.Generator().manual_seed(9900 + 1000 * ci + noise_seed)
        U = [torch.rand(E[t], K, generator=g) for t in range(T - 1)]
        Uall = torch.cat(U)
        r32 = {s: run(L, model, inputs, masks, node_inds, graph_info, U, *s) for s in settings(tag)}
        prior32, post32 = r32[(True, True)]["sampled"], r32[(True, False)]["sampled"]
        margin = min(min_margin(lg, Uall, TAU) for lg in (prior32, post32, prior64, post64))
        if margin <= MARGIN:
            continue
        r64rs = {s: rs64.calculate_loss(inputs[0], masks[0], graph_info[0], U, *s) for s in settings(tag)}
        if all(torch.equal(torch.cat(r32[s]["samples"]).argmax(-1), torch.cat(r64rs[s]["samples"]).argmax(-1)) for s in r32):
            break
    else:
        raise RuntimeError("no noise seed with unambiguous samples")
    m64 = model.double()
    torch.set_default_dtype(torch.float64)
    try:
        r64 = {s: run(L, m64, inputs.double(), masks, node_inds, graph_info, U, *s) for s in settings(tag)}
    finally:
        torch.set_default_dtype(torch.float32)
    model.float()
    for k, v in (("in.inputs", inputs), ("in.masks", masks)):
        out[f"{pre}.{k}"] = v.numpy()
    for t in range(T - 1):
        out[f"{pre}.send.{t}"], out[f"{pre}.recv.{t}"], out[f"{pre}.e2n.{t}"] = (x.numpy() for x in graph_info[0][t])
        out[f"{pre}.uniform.{t}"] = U[t].numpy()
    for name, r in (("ref", r32), ("ref64", r64)):
        out[f"{pre}.{name}.prior"] = r[(True, True)]["sampled"].numpy()
        out[f"{pre}.{name}.posterior"] = r[(True, False)]["posterior"].numpy()
    worst = 0.0
    for s in settings(tag):
        sn = setting_name(*s)
        a, b = r32[s], r64[s]
        assert torch.equal(torch.cat(a["samples"]).argmax(-1), torch.cat(b["samples"]).argmax(-1)), "a sample flipped in fp64"
        assert torch.equal(b["posterior"], r64[(True, False)]["posterior"]) and torch.equal(a["posterior"], r32[(True, False)]["posterior"])
        assert all(bool(torch.isfinite(v).all()) for r in (a, b) for v in (r["predictions"], r["loss"], r["nll"], r["kl"]))
        for name, r in (("ref", a), ("ref64", b)):
            out[f"{pre}.{sn}.{name}.predictions"] = r["predictions"].numpy()
            out[f"{pre}.{sn}.{name}.edges"] = r["edges"].numpy()
            for q in ("loss", "nll", "kl"):
                out[f"{pre}.{sn}.{name}.{q}"] = r[q].reshape(-1).numpy()
        for q in ("loss", "nll", "kl"):
            rel = abs(float(a[q].reshape(-1)[0]) - float(b[q].reshape(-1)[0])) / abs(float(b[q].reshape(-1)[0]))
            out[f"{pre}.{sn}.rel32.{q}"] = np.float64(rel)
            worst = max(worst, rel)
    out[f"{pre}.noise_seed"] = np.int64(9900 + 1000 * ci + noise_seed)
    out[f"{pre}.margin"] = np.float64(margin)
    present = [int(masks[0, t].sum()) for t in range(T)]
    print(f"{pre}: {len(sd)} keys, present {present}, edges {E}, noise seed {9900 + 1000 * ci + noise_seed}, margin {margin:.3g}, "
          f"nll {float(r64[(True, False)]['nll']):.6g}, kl {float(r64[(True, False)]['kl']):.6g}, worst fp32 rel {worst:.3g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    torch.set_num_threads(1)                  # fixed reduction order: reruns reproduce the file bit for bit
    out = {"seed": np.int64(SEED), "hidden": np.int64(128), "rnn_hidden": np.int64(64), "tau": np.float64(TAU),
           "cases": np.array(list(CASES)), "models": np.array(list(MODELS)), "free_running": np.array(list(FREE_RUNNING))}
    with reference() as (mods, get_knn_graph_info):
        for kind in MODELS:
            L, cls = mods[kind]
            for ci, tag in enumerate(CASES):
                fixture(out, kind, L, cls, get_knn_graph_info, ci, tag)
    MD.save_npz(os.path.join(args.out, "dyn_loss.npz"), out)
    print("wrote dyn_loss.npz")


if __name__ == "__main__":
    main()
