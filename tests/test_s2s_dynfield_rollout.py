"""The fused step / device rollout of the seq2seq DynamicFieldAether (aether_s2s_dynfield_*), the parts a machine without a
GPU can check: the entries are declared and exported, the plan-size entry refuses the sizes the step does not take, and the
model with the Markov decoder (decoder_type 'ref_mlp') is constructed as the reference constructs it
(nn/seq2seq/dynamic_field_aether.py:22-27: encoder, then the decoder, before everything else)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import REPO

ENTRIES = ("aether_s2s_dynfield_plan_bytes", "aether_s2s_dynfield_plan_build", "aether_s2s_dynfield_step_workspace_bytes",
           "aether_s2s_dynfield_step", "aether_s2s_dynfield_rollout")


def model_params(N=5, D=3, markov=True, **extra):
    p = {"num_vars": N, "num_edge_types": 2, "encoder_dropout": 0.0, "encoder_hidden": 128, "encoder_rnn_hidden": 32,
         "encoder_rnn_type": "lstm", "input_size": 2 * D, "encoder_mlp_num_layers": 3, "encoder_mlp_hidden": 32,
         "prior_num_layers": 3, "prior_hidden_size": 32, "use_3d": D == 3, "pos_representation": "cart", "gpu": False,
         "decoder_hidden": 32, "skip_first": False, "decoder_dropout": 0.0, "gumbel_temp": 0.5, "rff_std": 1.0,
         "graph_hidden": 32, "mlp_hidden": 48, "field": None}
    if markov:
        p["decoder_type"] = "ref_mlp"
    p.update(extra)
    return p


def test_the_entries_are_declared_and_exported():
    from aether_amd import _lib
    header = open(os.path.join(REPO, "include", "aether_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "dynamic_field_aether.py:117-134" in header and "207-246" in header      # the reference lines they replace


def test_plan_bytes_refuses_what_the_step_does_not_take():
    from aether_amd import _lib
    lib = _lib.load()
    one = C.c_char_p(b"x")                     # only whether a decoder is given is looked at
    #            D, he, hd, R, prior layers, prior hidden, K, skip_first, mlp_hidden
    good = (3, 128, 32, 32, 3, 32, 2, 0, 48)
    rec, mar = lib.aether_s2s_dynfield_plan_bytes(one, None, *good), lib.aether_s2s_dynfield_plan_bytes(None, one, *good)
    assert rec > 0 and mar > 0 and rec != mar

    def with_(**kw):
        names = ("D", "he", "hd", "R", "layers", "ph", "K", "skip", "mh")
        return tuple(kw.get(n, v) for n, v in zip(names, good))

    assert lib.aether_s2s_dynfield_plan_bytes(one, None, *with_(he=192)) == 0          # he % 128 != 0
    assert lib.aether_s2s_dynfield_plan_bytes(one, None, *with_(mh=40)) == 0           # mlp_hidden % 16 != 0
    assert lib.aether_s2s_dynfield_plan_bytes(one, None, *with_(K=5)) == 0             # K > 4
    assert lib.aether_s2s_dynfield_plan_bytes(one, one, *good) == 0                    # both decoders
    assert lib.aether_s2s_dynfield_plan_bytes(None, None, *good) == 0                  # neither
    assert lib.aether_s2s_dynfield_plan_bytes(None, one, *with_(K=1, skip=1)) == 0     # Markov: no used edge type
    # mlp_hidden a multiple of 128: the plan also holds the fp16 x 2 images of linear_1 [mh][he] and linear_2 [mh][mh]
    small, big = lib.aether_s2s_dynfield_plan_bytes(one, None, *with_(mh=112)), lib.aether_s2s_dynfield_plan_bytes(one, None, *with_(mh=128))
    assert big - small == 128 * 128 * 4 + 128 * 128 * 4
    # workspace: hidden rows of the field query max(he, mlp_hidden) wide
    ws = lib.aether_s2s_dynfield_step_workspace_bytes
    assert ws(3, 128, 32, 32, 32, 2, 48, 35, 140) == lib.aether_s2s_step_workspace_bytes(3, 128, 32, 32, 32, 2, 35, 140)
    assert ws(3, 128, 32, 32, 32, 2, 256, 35, 140) > ws(3, 128, 32, 32, 32, 2, 48, 35, 140)
    assert ws(3, 128, 32, 32, 32, 2, 40, 35, 140) == 0


@pytest.mark.parametrize("D", [2, 3])
def test_ref_mlp_constructs_with_the_reference_key_set(D):
    from aether_amd.nn.seq2seq.aether import Aether
    from aether_amd.nn.seq2seq.dynamic_field_aether import DynamicFieldAether
    from aether_amd.nn.seq2seq.markov import MarkovDecoder
    p = model_params(D=D)
    model = DynamicFieldAether(p, device=None)
    assert isinstance(model.decoder, MarkovDecoder) and model.decoder.get_initial_hidden(torch.zeros(1, 3, 5, 2 * D)) is None
    keys = list(model.state_dict())
    base = [k for k in Aether(p, device=None).state_dict() if k.startswith(("encoder.", "decoder."))]
    rest = [k for k in keys if not k.startswith(("encoder.", "decoder."))]
    assert keys[:len(base)] == base                                    # encoder, then decoder, first (:22-27)
    assert rest and all(k.startswith(("graph_pooler.", "film_net.")) or k == "coordinate_embedding.B" for k in rest)
    assert {"coordinate_embedding.B", "film_net.linear_3.bias", "film_net.film_2.beta.2.weight",
            "graph_pooler.rnn.weight_hh_l0"} <= set(rest)


@pytest.mark.parametrize("seed", [0, 11])
def test_seeded_encoder_and_decoder_equal_those_of_aether(seed):
    from aether_amd.nn.seq2seq.aether import Aether
    from aether_amd.nn.seq2seq.dynamic_field_aether import DynamicFieldAether
    p = model_params()
    torch.manual_seed(seed)
    a = DynamicFieldAether(p, device=None).state_dict()
    torch.manual_seed(seed)
    b = Aether(p, device=None).state_dict()
    n = 0
    for k, v in b.items():
        if k.startswith(("encoder.", "decoder.")):
            assert torch.equal(a[k], v), k
            n += 1
    assert n > 20


def test_what_stays_refused():
    from aether_amd import _lib
    from aether_amd.nn.seq2seq.dynamic_field_aether import DynamicFieldAether
    with pytest.raises(ValueError):
        DynamicFieldAether(model_params(use_charges=True), device=None)
    model = DynamicFieldAether(model_params(), device=None)
    with pytest.raises(_lib.AetherHipError):
        model.calculate_loss(None, is_train=True)
    with pytest.raises(_lib.AetherHipError):
        model.single_step_forward(None, None, None, False, None)
    # a single frame leaves nothing to take the graph summary from (inputs[:, :-1] is empty): refused, not run
    for call in (model.predict_future, model.predict_future_stepwise):
        with pytest.raises(ValueError):
            call(torch.zeros(2, 1, 5, 6), 3)
    with pytest.raises(ValueError):
        model.predict_future(torch.zeros(2, 1, 5, 6), 3, return_everything=True)
