#!/usr/bin/env python3
"""Golden fixtures of the charge-aware seq2seq Aether from the imported reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (AETHER_REFERENCE, default /root/reference).  Imported, unmodified:
``nn.seq2seq.ablations.aether_charges.AetherCharges``, with the torch_scatter stand-in of oracle/make_golden.py and the
identity ``.cuda()`` as tools/make_golden_markov.py uses them.  Parameters come from the class's own constructor under a fixed
torch seed (the drop-in module creates the same tensors in the same order); the BatchNorm running statistics are perturbed as
oracle/make_golden_dynamicvars.py::perturb_bn_ does.  Every file stores the seed, the state_dict key list and a checksum of
every tensor instead of the weights.  Writes, for D in {2, 3},

  s2s_charges_D{D}.npz   hidden 128 / 128 / 64, K = 2; cases B2N5 (skip_first False), B3N5 (skip_first True), B1N2 (False);
                         charges all +1, all -1, mixed and with a 0 (index 0, as the reference's .long() gives).  Per case:
                         inputs [B, 4, N, 2D], charges, the uniform draws, and the reference's predict_field (3-D and 4-D x),
                         one prior step / sample / decoder step from the zero state (fp32 and after .double()), and
                         predict_future (3 burn-in + 4 steps).  Under loss.<config>: calculate_loss(is_train=False) for the two
                         LOSS_CONFIGS of oracle/make_golden_seq2seq.py (T = 5), fp32 and after .double().

The Gumbel draws are regenerated after the call (same global seed); a noise seed is accepted only when every sample wins its
race by a clear margin AND the fp64 restatement (tests/s2s_charges_restatement.py) samples the same edge types everywhere, so
that a comparison through the hard samples can only be upset by the code under test.

Reruns reproduce the files bit for bit.   Usage:  python tools/make_golden_s2s_charges.py [--out tests/golden]
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
sys.path.insert(0, REPO)

import make_golden as MG                      # noqa: E402  (torch_scatter stand-in)
import make_golden_seq2seq as MS              # noqa: E402  (enc_params)
from make_golden_dynamicvars import perturb_bn_   # noqa: E402

SEED = 9753
H, R, K, T, STEPS = 128, 64, 2, 4, 4
MARGIN = 1e-3
CASES = {   # tag: (B, N, skip_first, charges per graph)
    "B2N5": (2, 5, False, [[1, -1, 1, 1, -1], [1, 0, -1, -1, 1]]),
    "B3N5": (3, 5, True, [[1, 1, 1, 1, 1], [-1, -1, -1, -1, -1], [-1, 1, -1, 1, 1]]),
    "B1N2": (1, 2, False, [[1, -1]]),
}


def model_params(N, D, skip_first, extra=None):
    params = dict(MS.enc_params(N, D, H, R))
    params.update({"num_edge_types": K, "gpu": False, "decoder_hidden": H, "skip_first": skip_first, "decoder_dropout": 0.0,
                   "gumbel_temp": 0.5, "encoder_mlp_hidden": 64, "prior_hidden_size": 64, "rff_std": 1.0})
    params.update(extra or {})
    return params


@contextlib.contextmanager
def reference():
    MG._install_scatter_standin()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import nn.seq2seq.ablations.aether_charges as A                   # noqa: WPS433 (reference import)
    orig_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield A
    finally:
        torch.Tensor.cuda = orig_cuda


def checksums(out, sd):
    for k, v in sd.items():
        if v.dtype.is_floating_point:
            out["sum." + k] = np.float64(v.double().sum().item())
            out["abs." + k] = np.float64(v.double().abs().sum().item())
    out["keys"] = np.array(list(sd.keys()))
    out["shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])


@contextlib.contextmanager
def recorded_logits(A):
    seen = []
    orig = A.gumbel_softmax

    def wrapper(logits, *a, **k):
        seen.append(logits.detach().clone())
        return orig(logits, *a, **k)

    A.gumbel_softmax = wrapper
    try:
        yield seen
    finally:
        A.gumbel_softmax = orig


def min_margin(logits, U, tau):
    eps = 1e-10
    g = -torch.log(eps - torch.log(U + eps))
    y = (logits.double() + g.double()) / tau
    top = torch.topk(y, 2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


def build_model(A, N, D, skip_first):
    torch.manual_seed(SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        model = A.AetherCharges(model_params(N, D, skip_first)).eval()
    with torch.no_grad():
        perturb_bn_(model)
    return model


def fixture(out_dir, D):
    import s2s_charges_restatement as RS
    from oracle import seq2seq_oracle as S
    out = {"seed": np.int64(SEED), "hidden": np.int64(H), "rnn_hidden": np.int64(R), "num_edge_types": np.int64(K),
           "steps": np.int64(STEPS), "cases": np.array(list(CASES))}
    with reference() as A:
        for ci, (tag, (B, N, skip, ch)) in enumerate(CASES.items()):
            E = N * (N - 1)
            model = build_model(A, N, D, skip)
            sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
            if ci == 0:
                checksums(out, sd)
            g = torch.Generator().manual_seed(7000 + 10 * D + ci)
            inputs = torch.randn(B, T, N, 2 * D, generator=g)
            charges = torch.tensor(ch, dtype=torch.float32)
            cidx = A.AetherCharges.charge_to_index(charges)
            rs64 = RS.Model(sd, torch.float64, D == 3, "polar", 3, skip, 0.5, folded=False,
                            frames_dtype=torch.float32 if D == 3 else None)
            for noise_seed in range(200):
                torch.manual_seed(8000 + noise_seed)
                with torch.no_grad(), recorded_logits(A) as seen:
                    preds, edges = model.predict_future(inputs, STEPS, return_edges=True, charges=charges)
                torch.manual_seed(8000 + noise_seed)
                U = torch.stack([torch.rand(B * E, K) for _ in range(T - 1 + STEPS)])
                m = min(min_margin(lg.reshape(-1, K), U[t], 0.5) for t, lg in enumerate(seen))
                if len(seen) != T - 1 + STEPS or m <= MARGIN:
                    continue
                _, e64, lg64, _ = rs64.predict_future(inputs, STEPS, U.double(), cidx, return_all=True)
                ref_all = torch.stack([S.gumbel_hard(lg.reshape(-1, K), U[t], 0.5) for t, lg in enumerate(seen)])
                r64_all = torch.stack([S.gumbel_hard(lg.reshape(-1, K), U[t].double(), 0.5) for t, lg in enumerate(lg64)])
                if torch.equal(ref_all.argmax(-1), r64_all.argmax(-1)) and torch.equal(edges.argmax(-1), e64.argmax(-1)):
                    break
            else:
                raise RuntimeError("no noise seed with unambiguous samples")
            with torch.no_grad():
                cemb = model.charge_embedding(cidx)
                x = inputs[:, :-1].transpose(2, 1).contiguous()
                field4, _ = model.predict_field(x, cemb)                            # [B, N, T - 1, D]
                x0 = inputs[:, 0]
                field0, _ = model.predict_field(x0, cemb)
                zeros = (torch.zeros(B, E, R), torch.zeros(B, E, R))
                logits, (h1, c1) = model.encoder.single_step_forward(x0, zeros, field0, cemb)
                z = S.gumbel_hard(logits.reshape(-1, K), U[0], 0.5).view(B, E, K)
                dec_out, dec_hid = model.decoder(x0, torch.zeros(B, N, H), z, field0, cemb)
                m64 = model.double()                                                 # the same step in fp64 (same sample z)
                torch.set_default_dtype(torch.float64)                              # (the decoder's torch.zeros accumulators)
                cemb64 = m64.charge_embedding(cidx)
                f64, _ = m64.predict_field(x0.double(), cemb64)
                lg64s, (h64, c64) = m64.encoder.single_step_forward(x0.double(), tuple(t.double() for t in zeros), f64, cemb64)
                do64, dh64 = m64.decoder(x0.double(), torch.zeros(B, N, H, dtype=torch.float64), z.double(), f64, cemb64)
                torch.set_default_dtype(torch.float32)
                model.float()
            for k, v in (("ref64.field0", f64), ("ref64.prior_logits", lg64s), ("ref64.prior_h", h64), ("ref64.prior_c", c64),
                         ("ref64.decoder_out", do64), ("ref64.decoder_hidden", dh64)):
                out[f"{tag}.{k}"] = v.detach().numpy()
            for k, v in (("in.inputs", inputs), ("in.charges", charges), ("in.uniform", U), ("ref.field4", field4),
                         ("ref.field0", field0), ("ref.prior_logits", logits), ("ref.prior_h", h1), ("ref.prior_c", c1),
                         ("ref.step_edges", z), ("ref.decoder_out", dec_out), ("ref.decoder_hidden", dec_hid),
                         ("ref.predictions", preds), ("ref.edges", edges)):
                out[f"{tag}.{k}"] = v.detach().numpy()
            out[f"{tag}.skip_first"] = np.int64(skip)
            out[f"{tag}.noise_seed"] = np.int64(8000 + noise_seed)
            out[f"{tag}.margin"] = np.float64(m)
            print(f"D={D} {tag}: noise seed {8000 + noise_seed}, margin {m:.3g}")
    np.savez(os.path.join(out_dir, f"s2s_charges_D{D}.npz"), **out)
    print(f"wrote s2s_charges_D{D}.npz")


def loss_fixture(out_dir, D):
    """calculate_loss(is_train=False, return_logits=True, charges=) for the two LOSS_CONFIGS of make_golden_seq2seq.py on the
    B2N5 case's model (T = 5: with val_teacher_forcing_steps 2 the last two steps run on the model's own predictions),
    fp32 and after .double(); appended to s2s_charges_D{D}.npz under loss.<config>."""
    import s2s_charges_restatement as RS
    path = os.path.join(out_dir, f"s2s_charges_D{D}.npz")
    out = dict(np.load(path))
    B, N, skip, ch = CASES["B2N5"]
    E, TL = N * (N - 1), 5
    g = torch.Generator().manual_seed(7500 + D)
    inputs = torch.randn(B, TL, N, 2 * D, generator=g)
    charges = torch.tensor(ch, dtype=torch.float32)
    out["loss.in.inputs"], out["loss.in.charges"] = inputs.numpy(), charges.numpy()
    with reference() as A:
        cidx = A.AetherCharges.charge_to_index(charges)
        for name, cfg in MS.LOSS_CONFIGS.items():
            torch.manual_seed(SEED)
            with contextlib.redirect_stdout(io.StringIO()):
                model = A.AetherCharges(model_params(N, D, skip, cfg)).eval()
            with torch.no_grad():
                perturb_bn_(model)
            sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
            full = dict(model_params(N, D, skip, cfg))
            rs64 = RS.Model(sd, torch.float64, D == 3, "polar", 3, skip, 0.5, frames_dtype=torch.float32 if D == 3 else None)
            for noise_seed in range(200):
                torch.manual_seed(9000 + noise_seed)
                with torch.no_grad(), recorded_logits(A) as seen:
                    loss, nll, kl, post, preds = model.calculate_loss(inputs, is_train=False, return_logits=True, charges=charges)
                torch.manual_seed(9000 + noise_seed)
                U = torch.stack([torch.rand(B * E, K) for _ in range(TL - 1)])
                m = min(min_margin(lg.reshape(-1, K), U[t], 0.5) for t, lg in enumerate(seen))
                if len(seen) != TL - 1 or m <= MARGIN:
                    continue
                o64 = rs64.calculate_loss(full, inputs, U.double(), cidx)
                if float((o64[4] - preds).abs().max()) <= 1e-4 * float(preds.abs().max()):     # no sample flipped
                    break
            else:
                raise RuntimeError("no noise seed with unambiguous samples")
            with torch.no_grad():
                m64 = model.double()
                torch.set_default_dtype(torch.float64)
                if getattr(m64, "log_prior", None) is not None:
                    m64.log_prior = m64.log_prior.double()
                # the same draws: under a float64 default torch.rand would draw other numbers from the seed, so the fp64 run takes
                # its hard samples from U (the formula of gumbel_softmax(hard=True), pinned in tests/test_oracle_golden.py)
                from oracle import seq2seq_oracle as S
                orig, calls = A.gumbel_softmax, []

                def given_draws(logits, tau=1, hard=False, eps=1e-10):
                    calls.append(1)
                    return S.gumbel_hard(logits, U[len(calls) - 1].double(), tau)

                A.gumbel_softmax = given_draws
                try:
                    r64 = m64.calculate_loss(inputs.double(), is_train=False, return_logits=True, charges=charges.double())
                finally:
                    A.gumbel_softmax = orig
                    torch.set_default_dtype(torch.float32)
            for k, v in (("uniform", U), ("loss", loss), ("nll", nll), ("kl", kl), ("posterior", post), ("predictions", preds)):
                out[f"loss.{name}.{k}"] = v.detach().numpy()
            for k, v in zip(("loss", "nll", "kl", "posterior", "predictions"), r64):
                out[f"loss.{name}.ref64.{k}"] = v.detach().numpy()
            out[f"loss.{name}.noise_seed"] = np.int64(9000 + noise_seed)
            print(f"D={D} loss {name}: {float(loss):.6g} (fp64 {float(r64[0]):.6g}), noise seed {9000 + noise_seed}, margin {m:.3g}")
    np.savez(path, **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    torch.set_num_threads(1)                  # fixed reduction order: reruns reproduce the files bit for bit
    for D in (2, 3):
        fixture(args.out, D)
        loss_fixture(args.out, D)


if __name__ == "__main__":
    main()
