"""seq2seq Aether with decoder_type 'ref_mlp' (the reference's MarkovDecoder, nn/seq2seq/aether.py:413-503), host side:
construction (keys, order, shapes and seeded initial values equal the reference's), the refusals, and an fp64
restatement of the decoder step pinned to the golden vectors (tools/make_golden_markov.py).  The GPU tests
(test_gpu_s2s_markov.py) check the HIP step against that restatement on fresh shapes."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, scale_rel_err

sys.path.insert(0, os.path.join(REPO, "tools"))
from oracle import seq2seq_oracle as S                                   # noqa: E402


def markov_params(N, D, H, K, skip_first):
    return {"num_vars": N, "input_size": 2 * D, "gpu": False, "decoder_hidden": H, "num_edge_types": K,
            "skip_first": skip_first, "decoder_dropout": 0.0, "use_3d": D == 3, "decoder_type": "ref_mlp"}


def model_params(extra=None):
    import make_golden_markov as MGM
    return MGM.model_params(extra)


def check_checksums(sd, d, prefix=""):
    assert list(sd.keys()) == [str(k) for k in d[prefix + "keys"]]
    for k, v in sd.items():
        if v.dtype.is_floating_point:
            assert abs(float(v.double().sum()) - float(d[prefix + "sum." + k])) <= \
                1e-9 * max(1.0, float(d[prefix + "abs." + k])), k


def restate(sd, inputs, edges, field, use_3d, skip_first, frames_dtype=None):
    """MarkovDecoder.forward (aether.py:459-503) in the dtype of ``inputs`` from a state_dict with the module's own keys:
    localizer -> relu(lin2(relu(lin1(edge_attr)))) -> sum_k out[..., c Ku + k] w[..., k0 + k] -> receiver mean + res1 ->
    out_mlp -> globalise -> residual.  ``frames_dtype``: build the local frames in that dtype (then cast): in 3-D every
    node's origin edge has an Euler angle on its branch cut, +-pi by one rounding, so an fp64 restatement of an fp32
    evaluation takes the frames from fp32 as the fp32 evaluation does."""
    dt = inputs.dtype
    p = {k: v.to(dt) for k, v in sd.items()}
    lin = lambda x, name: x @ p[name + ".weight"].t() + p[name + ".bias"]
    B, N, _ = inputs.shape
    D = 3 if use_3d else 2
    k0 = 1 if skip_first else 0
    fd = frames_dtype or dt
    frames = S.augmented_localizer(torch.cat([inputs, field.to(dt)], -1).to(fd), use_3d, "polar")
    rel_feat, Rinv, edge_attr = (t.to(dt) for t in frames[:3])
    out = torch.relu(lin(torch.relu(lin(edge_attr, "edge_filter.lin1")), "edge_filter.lin2"))
    ku = edges.shape[-1] - k0
    msgs = (out.view(*out.shape[:-1], -1, ku) * edges.to(dt)[..., k0:].unsqueeze(-2)).sum(-1)
    _, recv = torch.where(~torch.eye(N, dtype=bool))
    aug = S._scatter_mean_dim1(msgs, recv, N) + lin(rel_feat, "res1")
    h = torch.relu(lin(torch.relu(lin(aug, "out_mlp.0")), "out_mlp.3"))
    pred = lin(h, "out_mlp.6")
    pred = torch.cat([(Rinv @ x.unsqueeze(-1)).squeeze(-1) for x in pred.split(D, -1)], -1)
    return inputs + pred


# -- construction -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("K", [2, 3])
def test_markov_decoder_matches_reference_init(D, K):
    from aether_amd.nn.seq2seq.markov import MarkovDecoder
    d = np.load(os.path.join(GOLDEN, f"s2s_markov_decoder_D{D}.npz"))
    H, N = int(d["hidden_size"]), int(d["num_vars"])
    torch.manual_seed(int(d["seed"]))
    dec = MarkovDecoder(markov_params(N, D, H, K, K == 3), device=None)
    sd = dec.state_dict()
    check_checksums(sd, d, f"K{K}.")
    ku = K - (K == 3)
    assert sd["edge_filter.lin2.weight"].shape == (H * ku, H)
    assert sd["edge_filter.lin1.weight"].shape == (H, 2 * (4 * D + D * (D - 1) // 2) + 3 * D)
    assert sd["res1.weight"].shape == (H, 7 * D + D * (D - 1) // 2)
    assert torch.all(sd["edge_filter.lin1.bias"] == 0.1) and torch.all(sd["edge_filter.lin2.bias"] == 0.1)
    assert dec.get_initial_hidden(torch.zeros(2, 5, 2 * D)) is None


@pytest.mark.parametrize("name", ["future", "loss"])
def test_aether_ref_mlp_constructs_like_the_reference(name):
    from aether_amd.nn.seq2seq.aether import Aether
    import make_golden_markov as MGM
    d = np.load(os.path.join(GOLDEN, f"s2s_markov_{name}_D2.npz"))
    extra = None if name == "future" else list(MGM.MS.LOSS_CONFIGS.values())[0]
    torch.manual_seed(int(d["seed"]))
    model = Aether(model_params(extra), device=None)
    check_checksums(model.state_dict(), d)
    keys = list(model.state_dict())
    dec = [i for i, k in enumerate(keys) if k.startswith("decoder.")]
    enc = [i for i, k in enumerate(keys) if k.startswith("encoder.")]
    fld = [i for i, k in enumerate(keys) if k.startswith("field_net.")]
    assert max(enc) < min(dec) and max(dec) < min(fld)                   # between the encoder and the field_net keys
    assert model.decoder.get_initial_hidden(torch.zeros(1, 3, 5, 4)) is None


def test_refusals():
    from aether_amd.nn.seq2seq.aether import Aether
    with pytest.raises(ValueError):
        Aether(model_params({"decoder_dropout": 0.1}), device=None)
    with pytest.raises(ValueError):                                      # Ku = 0: nothing would carry a message
        Aether(model_params({"num_edge_types": 1, "skip_first": True}), device=None)
    from aether_amd.nn.seq2seq.dynamic_field_aether import DynamicFieldAether
    import inspect
    assert "ref_mlp" in inspect.getsource(DynamicFieldAether.__init__)   # its refusal stays


def test_recurrent_decoder_is_still_the_default():
    from aether_amd.nn.seq2seq.aether import Aether
    from aether_amd.nn.seq2seq.decoder import RecurrentDecoder
    p = model_params()
    p.pop("decoder_type")
    assert isinstance(Aether(p, device=None).decoder, RecurrentDecoder)


# -- the fp64 restatement against the reference's own outputs ---------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("kind", ["hard", "soft"])
def test_restatement_reproduces_reference(D, K, kind):
    from aether_amd.nn.seq2seq.markov import MarkovDecoder
    d = np.load(os.path.join(GOLDEN, f"s2s_markov_decoder_D{D}.npz"))
    H, N = int(d["hidden_size"]), int(d["num_vars"])
    torch.manual_seed(int(d["seed"]))
    sd = MarkovDecoder(markov_params(N, D, H, K, K == 3), device=None).state_dict()
    inputs, field = torch.from_numpy(d["in.inputs"]), torch.from_numpy(d["in.field"])
    edges = torch.from_numpy(d[f"K{K}.in.edges_{kind}"])
    got64 = restate(sd, inputs.double(), edges, field, D == 3, K == 3)
    assert scale_rel_err(got64, torch.from_numpy(d[f"K{K}.ref64.{kind}.outputs"])) <= 1e-12
    got32 = restate(sd, inputs, edges, field, D == 3, K == 3)
    assert scale_rel_err(got32, torch.from_numpy(d[f"K{K}.ref.{kind}.outputs"])) <= 1e-6


def test_header_declares_the_markov_entries():
    from aether_amd import _lib
    for name in ("aether_s2s_markov_decoder_step", "aether_s2s_markov_decoder_workspace_bytes", "aether_s2s_markov_plan_bytes",
                 "aether_s2s_markov_plan_build", "aether_s2s_markov_step", "aether_s2s_markov_rollout"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    # plan sizes: the Markov plan holds no recurrent decoder tensors; Ku = 0 is refused
    assert 0 < lib.aether_s2s_markov_plan_bytes(2, 128, 512, 64, 3, 64, 3, 1) < lib.aether_s2s_plan_bytes(2, 128, 512, 64, 3, 64, 3)
    assert lib.aether_s2s_markov_plan_bytes(2, 128, 512, 64, 3, 64, 1, 1) == 0
    assert lib.aether_s2s_markov_decoder_workspace_bytes(2, 512, 10, 40) > 0
