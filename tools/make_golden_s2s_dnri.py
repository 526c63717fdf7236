#!/usr/bin/env python3
"""Golden fixtures of the seq2seq dNRI baseline from the imported reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (AETHER_REFERENCE, default /root/reference).  Imported, unmodified:
``nn.seq2seq.dnri.DNRI``.  As tools/make_golden_s2s_locs.py, with the same stand-ins: the torch_scatter stand-in of
oracle/make_golden.py, the alias of ``dnri.utils.canonicalization``, the identity ``.cuda()``; parameters from the class's own
constructor under a fixed torch seed (the drop-in module creates the same tensors in the same order), BatchNorm running
statistics perturbed by oracle/make_golden_dynamicvars.py::perturb_bn_, and the seed, the state_dict key list and a checksum
of every tensor stored instead of the weights.  Writes, for D in {2, 3},

  s2s_dnri_D{D}.npz   hidden 128 / 128 / 64, K = 2, both decoders (prefix ``rec.`` DNRI_Decoder, ``mlp.`` decoder_type 'ref_mlp').
                      Cases: B2N5 (skip_first False), B3N5 (skip_first True; 60 edges, no multiple of a tile height) and B1N2
                      (the smallest graph: one in-edge per node, N - 1 = 1).  Per case: inputs [B, 4, N, 2D], the uniform
                      draws, one prior step / sample / decoder step from the zero state, predict_future (3 burn-in + 4 steps,
                      return_everything: the burn-in steps' predictions in front) -- all in fp32 and after .double(), but the
                      prior state (h, c), which is stored in fp32 only: the fp64 logits computed from it are.  Both decoders'
                      models have the same encoder (created first, same seed): its outputs are stored under ``rec.`` only.
                      Under <dec>.loss.<config>: calculate_loss(is_train=False) for the two LOSS_CONFIGS of
                      oracle/make_golden_seq2seq.py on the B2N5 model (T = 5), fp32 and after .double().

The Gumbel draws are regenerated after the call (same global seed); a noise seed is accepted only when every sample wins its
race by MARGIN AND the fp64 restatement (tests/s2s_dnri_restatement.py) samples the same edge types everywhere, so that a
comparison through the hard samples can only be upset by the code under test.

Reruns reproduce the files bit for bit.   Usage:  python tools/make_golden_s2s_dnri.py [--out tests/golden]
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
REF = os.environ.get("AETHER_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, REPO)

import make_golden as MG                      # noqa: E402  (torch_scatter stand-in)
import make_golden_seq2seq as MS              # noqa: E402  (enc_params, LOSS_CONFIGS)
from make_golden_dynamicvars import perturb_bn_   # noqa: E402
from make_golden_s2s_locs import checksums, given_draws, min_margin, recorded_logits   # noqa: E402

SEED = 9753
H, R, K, T, STEPS = 128, 64, 2, 4, 4
MARGIN = 1e-3
DECODERS = {"rec": None, "mlp": "ref_mlp"}    # prefix: decoder_type
CASES = {   # tag: (B, N, skip_first)
    "B2N5": (2, 5, False),
    "B3N5": (3, 5, True),
    "B1N2": (1, 2, False),
}


def model_params(N, D, skip_first, decoder_type=None, extra=None):
    params = dict(MS.enc_params(N, D, H, R))
    params.update({"num_edge_types": K, "gpu": False, "decoder_hidden": H, "skip_first": skip_first, "decoder_dropout": 0.0,
                   "gumbel_temp": 0.5, "encoder_mlp_hidden": 64, "prior_hidden_size": 64})
    if decoder_type is not None:
        params["decoder_type"] = decoder_type
    params.update(extra or {})
    return params


def case_inputs(D, ci, tag):
    """The case's burn-in observations [B, T, N, 2D]."""
    B, N, _ = CASES[tag]
    g = torch.Generator().manual_seed(7000 + 10 * D + ci)
    return torch.randn(B, T, N, 2 * D, generator=g)


@contextlib.contextmanager
def reference():
    MG._install_scatter_standin()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import nn.utils.canonicalization as canon                       # noqa: WPS433 (reference import)
        sys.modules.setdefault("dnri.utils.canonicalization", canon)    # its old name (global_to_local.py:4)
        import nn.seq2seq.dnri as L                                      # noqa: WPS433
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield L
    finally:
        torch.Tensor.cuda = orig_cuda


def build_model(L, N, D, skip_first, decoder_type, extra=None):
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        model = L.DNRI(model_params(N, D, skip_first, decoder_type, extra)).eval()
    with torch.no_grad():
        perturb_bn_(model)
    return model


def one_step(model, x0, B, N, E, z, dtype):
    """One prior step from the zero state and the decoder step on the sample z, in ``dtype``."""
    x0 = x0.to(dtype)
    zeros = (torch.zeros(B, E, R, dtype=dtype), torch.zeros(B, E, R, dtype=dtype))
    logits, (h1, c1) = model.encoder.single_step_forward(x0, zeros)
    hidden = model.decoder.get_initial_hidden(x0.unsqueeze(1))
    out, hid = model.decoder(x0, None if hidden is None else hidden.to(dtype), z.to(dtype))
    res = {"prior_logits": logits, "prior_h": h1, "prior_c": c1, "decoder_out": out}
    if hid is not None:
        res["decoder_hidden"] = hid
    return res, logits


def fixture(out, D, dec, decoder_type, reference=reference, build_model=build_model, one_step=one_step, RS=None,
            shared_encoder=True):
    """The cases of one decoder into ``out``.  The keyword arguments are the model's own pieces: the generator of a model built
    on dNRI (tools/make_golden_s2s_dnri_aether.py) passes its reference import, constructor, step and restatement;
    ``shared_encoder``: both decoders' models compute the same prior step, which is stored once."""
    if RS is None:
        import s2s_dnri_restatement as RS
    from oracle import seq2seq_oracle as S
    with reference() as L:
        for ci, (tag, (B, N, skip)) in enumerate(CASES.items()):
            E = N * (N - 1)
            model = build_model(L, N, D, skip, decoder_type)
            sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
            if ci == 0:
                checksums(out, dec, sd)
            inputs = case_inputs(D, ci, tag)
            rs64 = RS.Model(sd, torch.float64, 3, skip, 0.5)
            for noise_seed in range(400):
                torch.manual_seed(8000 + noise_seed)
                with torch.no_grad(), recorded_logits(L) as seen:
                    preds, edges = model.predict_future(inputs, STEPS, return_edges=True, return_everything=True)
                torch.manual_seed(8000 + noise_seed)
                U = torch.stack([torch.rand(B * E, K) for _ in range(T - 1 + STEPS)])
                m = min(min_margin(lg.reshape(-1, K), U[t], 0.5) for t, lg in enumerate(seen))
                if len(seen) != T - 1 + STEPS or m <= MARGIN:
                    continue
                _, e64, lg64 = rs64.predict_future(inputs, STEPS, U.double(), return_all=True, everything=True)
                ref_all = torch.stack([S.gumbel_hard(lg.reshape(-1, K), U[t], 0.5) for t, lg in enumerate(seen)])
                r64_all = torch.stack([S.gumbel_hard(lg.reshape(-1, K), U[t].double(), 0.5) for t, lg in enumerate(lg64)])
                if torch.equal(ref_all.argmax(-1), r64_all.argmax(-1)) and torch.equal(edges.argmax(-1), e64.argmax(-1)):
                    break
            else:
                raise RuntimeError("no noise seed with unambiguous samples")
            with torch.no_grad():
                x0 = inputs[:, 0]
                s32, logits = one_step(model, x0, B, N, E, torch.zeros(B, E, K), torch.float32)
                z = S.gumbel_hard(logits.reshape(-1, K), U[0], 0.5).view(B, E, K)
                s32, _ = one_step(model, x0, B, N, E, z, torch.float32)
                m64 = model.double()
                torch.set_default_dtype(torch.float64)                              # (the decoder's torch.zeros accumulators)
                try:
                    s64, _ = one_step(m64, x0, B, N, E, z, torch.float64)
                    with given_draws(L, U):
                        p64, e64r = m64.predict_future(inputs.double(), STEPS, return_edges=True, return_everything=True)
                finally:
                    torch.set_default_dtype(torch.float32)
                model.float()
            values = [preds, edges, p64] + list(s32.values()) + list(s64.values())
            assert all(bool(torch.isfinite(v).all()) for v in values) and torch.equal(e64r.argmax(-1), edges.argmax(-1))
            assert preds.shape[1] == T - 1 + STEPS
            pre = f"{dec}.{tag}"
            # the encoder is created first under the same seed, so both decoders' models share it: the prior step is stored
            # once (rec.).  The prior state [B, E, R] is the largest entry: its fp64 copy is left out (file size) -- the fp64
            # prior logits, a function of it, are kept
            front = ("prior_logits", "prior_h", "prior_c")
            skip_keys = front if dec != "rec" and shared_encoder else ()
            for k, v in s32.items():
                if k not in skip_keys:
                    out[f"{pre}.ref.{k}"] = v.detach().numpy()
            for k, v in s64.items():
                if k not in skip_keys and k not in ("prior_h", "prior_c"):
                    out[f"{pre}.ref64.{k}"] = v.detach().numpy()
            for k, v in (("in.inputs", inputs), ("in.uniform", U), ("ref.step_edges", z), ("ref.everything", preds),
                         ("ref.everything_edges", edges), ("ref64.everything", p64)):
                out[f"{pre}.{k}"] = v.detach().numpy()
            out[f"{pre}.noise_seed"] = np.int64(8000 + noise_seed)
            out[f"{pre}.margin"] = np.float64(m)
            print(f"D={D} {dec} {tag}: noise seed {8000 + noise_seed}, margin {m:.3g}")


def loss_fixture(out, D, dec, decoder_type, reference=reference, build_model=build_model, RS=None):
    """calculate_loss(is_train=False, return_logits=True) for the two LOSS_CONFIGS of make_golden_seq2seq.py on the B2N5 case's
    model (T = 5: with val_teacher_forcing_steps 2 the last two steps run on the model's own predictions), fp32 and after
    .double(); under <dec>.loss.<config>.  Keyword arguments as ``fixture``."""
    if RS is None:
        import s2s_dnri_restatement as RS
    B, N, skip = CASES["B2N5"]
    E, TL = N * (N - 1), 5
    g = torch.Generator().manual_seed(7500 + D)
    inputs = torch.randn(B, TL, N, 2 * D, generator=g)
    out[f"{dec}.loss.in.inputs"] = inputs.numpy()
    with reference() as L:
        for name, cfg in MS.LOSS_CONFIGS.items():
            model = build_model(L, N, D, skip, decoder_type, cfg)
            sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
            full = dict(model_params(N, D, skip, decoder_type, cfg))
            rs64 = RS.Model(sd, torch.float64, 3, skip, 0.5)
            for noise_seed in range(400):
                torch.manual_seed(9000 + noise_seed)
                with torch.no_grad(), recorded_logits(L) as seen:
                    loss, nll, kl, post, preds = model.calculate_loss(inputs, is_train=False, return_logits=True)
                torch.manual_seed(9000 + noise_seed)
                U = torch.stack([torch.rand(B * E, K) for _ in range(TL - 1)])
                m = min(min_margin(lg.reshape(-1, K), U[t], 0.5) for t, lg in enumerate(seen))
                if len(seen) != TL - 1 or m <= MARGIN:
                    continue
                o64 = rs64.calculate_loss(full, inputs, U.double())
                if float((o64[4] - preds).abs().max()) <= 1e-4 * float(preds.abs().max()):     # no sample flipped
                    break
            else:
                raise RuntimeError("no noise seed with unambiguous samples")
            with torch.no_grad():
                m64 = model.double()
                torch.set_default_dtype(torch.float64)
                if getattr(m64, "log_prior", None) is not None:
                    m64.log_prior = m64.log_prior.double()
                try:
                    with given_draws(L, U):
                        r64 = m64.calculate_loss(inputs.double(), is_train=False, return_logits=True)
                finally:
                    torch.set_default_dtype(torch.float32)
            pre = f"{dec}.loss.{name}"
            for k, v in (("uniform", U), ("loss", loss), ("nll", nll), ("kl", kl), ("posterior", post), ("predictions", preds)):
                out[f"{pre}.{k}"] = v.detach().numpy()
            for k, v in zip(("loss", "nll", "kl", "posterior", "predictions"), r64):
                out[f"{pre}.ref64.{k}"] = v.detach().numpy()
            out[f"{pre}.noise_seed"] = np.int64(9000 + noise_seed)
            print(f"D={D} {dec} loss {name}: {float(loss):.6g} (fp64 {float(r64[0]):.6g}), noise seed {9000 + noise_seed}, "
                  f"margin {m:.3g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    torch.set_num_threads(1)                  # fixed reduction order: reruns reproduce the files bit for bit
    for D in (2, 3):
        out = {"seed": np.int64(SEED), "hidden": np.int64(H), "rnn_hidden": np.int64(R), "num_edge_types": np.int64(K),
               "steps": np.int64(STEPS), "cases": np.array(list(CASES)), "decoders": np.array(list(DECODERS))}
        for dec, decoder_type in DECODERS.items():
            fixture(out, D, dec, decoder_type)
            loss_fixture(out, D, dec, decoder_type)
        np.savez(os.path.join(args.out, f"s2s_dnri_D{D}.npz"), **out)
        print(f"wrote s2s_dnri_D{D}.npz")


if __name__ == "__main__":
    main()
