#!/usr/bin/env python3
"""Golden fixtures of the seq2seq Aether's Markov decoder (decoder_type 'ref_mlp') from the imported reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (AETHER_REFERENCE, default /root/reference).  Imported, unmodified:
``nn.seq2seq.aether.MarkovDecoder`` and ``nn.seq2seq.aether.Aether`` with ``decoder_type='ref_mlp'``, with the
torch_scatter stand-in of oracle/make_golden.py and the identity ``.cuda()`` exactly as
oracle/make_golden_seq2seq.py::future_fixture uses them.  Parameters come from the classes' own constructors under a
fixed torch seed; the drop-in modules create the same tensors in the same order, and every fixture stores the seed, the
state_dict key list and a checksum of every tensor.  Writes

  s2s_markov_decoder_D{2,3}.npz  MarkovDecoder.forward, K = 2 (skip_first False) and K = 3 (skip_first True), soft and
                                 one-hot weights, fp32 and after .double()
  s2s_markov_future_D2.npz       Aether.predict_future (K = 3, skip_first True): Gumbel draws regenerated; the noise seed is
                                 accepted only when every sample wins its Gumbel race by a clear margin
  s2s_markov_loss_D2.npz         Aether.calculate_loss(is_train=False) for the two LOSS_CONFIGS of make_golden_seq2seq.py

Reruns reproduce the files bit for bit (np.savez of deterministic CPU results; no timestamps).

Usage:  python tools/make_golden_markov.py [--out tests/golden]
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

import make_golden as MG                      # noqa: E402  (torch_scatter stand-in)
import make_golden_seq2seq as MS              # noqa: E402  (enc_params, LOSS_CONFIGS)

DEC_SEED, FUT_SEED, LOSS_SEED = 8642, 7531, 2222
MARGIN = 1e-3        # minimum gap between the winning and the runner-up Gumbel score, (logits + g) / tau


@contextlib.contextmanager
def reference():
    MG._install_scatter_standin()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import nn.seq2seq.aether as A                                     # noqa: WPS433 (reference import)
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


def markov_params(N, D, H, K, skip_first):
    return {"num_vars": N, "input_size": 2 * D, "gpu": False, "decoder_hidden": H, "num_edge_types": K,
            "skip_first": skip_first, "decoder_dropout": 0.0, "use_3d": D == 3, "decoder_type": "ref_mlp"}


def decoder_fixtures(out_dir):
    with reference() as A:
        for D in (2, 3):
            B, N, H = 2, 5, 256
            E = N * (N - 1)
            g = torch.Generator().manual_seed(600 + D)
            inputs = torch.randn(B, N, 2 * D, generator=g)
            field = torch.randn(B, N, D, generator=g) * 0.3
            out = {"in.inputs": inputs.numpy(), "in.field": field.numpy(), "seed": np.int64(DEC_SEED),
                   "hidden_size": np.int64(H), "num_vars": np.int64(N)}
            for K, skip in ((2, False), (3, True)):
                tag = f"K{K}"
                torch.manual_seed(DEC_SEED)
                with contextlib.redirect_stdout(io.StringIO()):
                    dec = A.MarkovDecoder(markov_params(N, D, H, K, skip)).eval()
                hard = torch.nn.functional.one_hot(torch.randint(0, K, (B, E), generator=g), K).float()
                soft = torch.softmax(torch.randn(B, E, K, generator=g), -1)
                out[f"{tag}.in.edges_hard"], out[f"{tag}.in.edges_soft"] = hard.numpy(), soft.numpy()
                out[f"{tag}.skip_first"] = np.int64(skip)
                with torch.no_grad():
                    for name, z in (("hard", hard), ("soft", soft)):
                        o, hid = dec(inputs, None, z, field)
                        assert hid is None
                        out[f"{tag}.ref.{name}.outputs"] = o.numpy()
                    dec64 = dec.double()
                    for name, z in (("hard", hard), ("soft", soft)):
                        o, _ = dec64(inputs.double(), None, z.double(), field.double())
                        out[f"{tag}.ref64.{name}.outputs"] = o.numpy()
                    dec.float()
                sd = dec.state_dict()
                sums = {}
                checksums(sums, sd)
                out.update({f"{tag}.{k}": v for k, v in sums.items()})
            np.savez(os.path.join(out_dir, f"s2s_markov_decoder_D{D}.npz"), **out)
            print("wrote s2s_markov_decoder_D%d.npz" % D)


def model_params(extra=None):
    D, N, H, R = 2, 5, 128, 64
    params = dict(MS.enc_params(N, D, H, R))
    params.update({"num_edge_types": 3, "gpu": False, "decoder_hidden": H, "skip_first": True, "decoder_dropout": 0.0,
                   "gumbel_temp": 0.5, "encoder_mlp_hidden": 64, "prior_hidden_size": 64, "rff_std": 1.0,
                   "decoder_type": "ref_mlp"})
    params.update(extra or {})
    return params


@contextlib.contextmanager
def recorded_logits(A):
    """Records the logits of every gumbel_softmax call of the reference model (the draws are regenerated afterwards)."""
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


def future_fixture(out_dir):
    with reference() as A:
        params = model_params()
        B, T, N, D, steps, K = 2, 4, 5, 2, 3, 3
        E = N * (N - 1)
        torch.manual_seed(FUT_SEED)
        with contextlib.redirect_stdout(io.StringIO()):
            model = A.Aether(params).eval()
        g = torch.Generator().manual_seed(910)
        inputs = torch.randn(B, T, N, 2 * D, generator=g)
        for noise_seed in range(50):
            torch.manual_seed(5000 + noise_seed)
            with torch.no_grad(), recorded_logits(A) as seen:
                preds, edges = model.predict_future(inputs, steps, return_edges=True)
            torch.manual_seed(5000 + noise_seed)
            U = torch.stack([torch.rand(B * E, K) for _ in range(T - 1 + steps)])
            m = min(min_margin(lg.reshape(-1, K), U[t], 0.5) for t, lg in enumerate(seen))
            if len(seen) == T - 1 + steps and m > MARGIN:
                break
        else:
            raise RuntimeError("no noise seed with unambiguous samples")
        out = {"in.inputs": inputs.numpy(), "in.uniform": U.numpy(), "ref.predictions": preds.numpy(),
               "ref.edges": edges.numpy(), "seed": np.int64(FUT_SEED), "noise_seed": np.int64(5000 + noise_seed),
               "steps": np.int64(steps), "margin": np.float64(m)}
        checksums(out, model.state_dict())
        np.savez(os.path.join(out_dir, "s2s_markov_future_D2.npz"), **out)
        print("wrote s2s_markov_future_D2.npz", tuple(preds.shape), "noise seed", 5000 + noise_seed, "margin", m)


def loss_fixture(out_dir):
    with reference() as A:
        B, T, N, D, K = 3, 6, 5, 2, 3
        E = N * (N - 1)
        g = torch.Generator().manual_seed(912)
        inputs = torch.randn(B, T, N, 2 * D, generator=g)
        out = {"in.inputs": inputs.numpy()}
        for name, cfg in MS.LOSS_CONFIGS.items():
            params = model_params(cfg)
            torch.manual_seed(LOSS_SEED)
            with contextlib.redirect_stdout(io.StringIO()):
                model = A.Aether(params).eval()
            for noise_seed in range(50):
                torch.manual_seed(6000 + noise_seed)
                with torch.no_grad(), recorded_logits(A) as seen:
                    loss, nll, kl, post, preds = model.calculate_loss(inputs, is_train=False, return_logits=True)
                torch.manual_seed(6000 + noise_seed)
                U = torch.stack([torch.rand(B * E, K) for _ in range(T - 1)])
                m = min(min_margin(lg.reshape(-1, K), U[t], 0.5) for t, lg in enumerate(seen))
                if len(seen) == T - 1 and m > MARGIN:
                    break
            else:
                raise RuntimeError("no noise seed with unambiguous samples")
            for k, v in (("uniform", U), ("loss", loss), ("nll", nll), ("kl", kl), ("posterior", post),
                         ("predictions", preds)):
                out[f"{name}.{k}"] = v.detach().numpy()
            out[f"{name}.noise_seed"] = np.int64(6000 + noise_seed)
            if name == list(MS.LOSS_CONFIGS)[0]:
                checksums(out, model.state_dict())
            print(name, "loss", float(loss), "noise seed", 6000 + noise_seed, "margin", m)
        out["seed"] = np.int64(LOSS_SEED)
        np.savez(os.path.join(out_dir, "s2s_markov_loss_D2.npz"), **out)
        print("wrote s2s_markov_loss_D2.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    torch.set_num_threads(1)                  # fixed reduction order: reruns reproduce the files bit for bit
    decoder_fixtures(args.out)
    future_fixture(args.out)
    loss_fixture(args.out)


if __name__ == "__main__":
    main()
