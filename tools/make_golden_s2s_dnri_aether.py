#!/usr/bin/env python3
"""Golden fixtures of the seq2seq ablation DNRIAether (dNRI with the latent field, no frames) from the imported reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (AETHER_REFERENCE, default /root/reference).  Imported, unmodified:
``nn.seq2seq.ablations.dnri_aether.DNRIAether``.  The recipe, the stand-ins, the cases, the sizes and the acceptance of a noise
seed are those of tools/make_golden_s2s_dnri.py, whose ``fixture`` / ``loss_fixture`` run here on this model's pieces.  Writes,
for D in {2, 3},

  s2s_dnri_aether_D{D}.npz   hidden 128 / 128 / 64, K = 2, both decoders (prefix ``rec.`` / ``mlp.``), cases B2N5, B3N5
                             (skip_first) and B1N2.  Per case: inputs, the uniform draws, the predicted field of frame 0, one
                             prior step / sample / decoder step from the zero state, predict_future (3 burn-in + 4 steps,
                             return_everything) in fp32 and after .double() (the fp64 prior state is left out: file size), and
                             calculate_loss(is_train=False) for the two LOSS_CONFIGS of oracle/make_golden_seq2seq.py at T = 5.
                             The field net is created behind the decoder, so the two decoders' models have different fields and
                             prior steps: both are stored.  The seed, the key list and per-tensor checksums stand for the
                             weights.

Reruns reproduce the files bit for bit.   Usage:  python tools/make_golden_s2s_dnri_aether.py [--out tests/golden]
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

import make_golden_s2s_dnri as MD              # noqa: E402  (sets the paths of oracle/, tests/ and the repository)
from make_golden_dynamicvars import perturb_bn_   # noqa: E402

SEED = 9753
CASES, DECODERS, R = MD.CASES, MD.DECODERS, MD.R
model_params = MD.model_params                # (use_3d follows D: oracle/make_golden_seq2seq.py::enc_params)


@contextlib.contextmanager
def reference():
    MD.MG._install_scatter_standin()
    if MD.REF not in sys.path:
        sys.path.insert(0, MD.REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import nn.utils.canonicalization as canon                       # noqa: WPS433 (reference import)
        sys.modules.setdefault("dnri.utils.canonicalization", canon)
        import nn.seq2seq.ablations.dnri_aether as L                     # noqa: WPS433
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield L
    finally:
        torch.Tensor.cuda = orig_cuda


def build_model(L, N, D, skip_first, decoder_type, extra=None):
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        model = L.DNRIAether(model_params(N, D, skip_first, decoder_type, extra)).eval()
    with torch.no_grad():
        perturb_bn_(model)
    return model


def one_step(model, x0, B, N, E, z, dtype):
    """The field of frame 0, one prior step from the zero state and the decoder step on the sample z, in ``dtype``."""
    x0 = x0.to(dtype)
    field, _ = model.predict_field(x0)
    zeros = (torch.zeros(B, E, R, dtype=dtype), torch.zeros(B, E, R, dtype=dtype))
    logits, (h1, c1) = model.encoder.single_step_forward(x0, zeros, field)
    hidden = model.decoder.get_initial_hidden(x0.unsqueeze(1))
    out, hid = model.decoder(x0, None if hidden is None else hidden.to(dtype), z.to(dtype), field)
    res = {"field": field, "prior_logits": logits, "prior_h": h1, "prior_c": c1, "decoder_out": out}
    if hid is not None:
        res["decoder_hidden"] = hid
    return res, logits


def main():
    import s2s_dnri_aether_restatement as RS
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    torch.set_num_threads(1)                  # fixed reduction order: reruns reproduce the files bit for bit
    kit = dict(reference=reference, build_model=build_model, RS=RS)
    for D in (2, 3):
        out = {"seed": np.int64(SEED), "hidden": np.int64(MD.H), "rnn_hidden": np.int64(R), "num_edge_types": np.int64(MD.K),
               "steps": np.int64(MD.STEPS), "cases": np.array(list(CASES)), "decoders": np.array(list(DECODERS))}
        for dec, decoder_type in DECODERS.items():
            MD.fixture(out, D, dec, decoder_type, one_step=one_step, shared_encoder=False, **kit)
            MD.loss_fixture(out, D, dec, decoder_type, **kit)
        np.savez(os.path.join(args.out, f"s2s_dnri_aether_D{D}.npz"), **out)
        print(f"wrote s2s_dnri_aether_D{D}.npz")


if __name__ == "__main__":
    main()
