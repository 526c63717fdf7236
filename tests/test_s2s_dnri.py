"""The seq2seq dNRI baseline (nn/seq2seq/dnri.py), host side: construction (keys, order, shapes and seeded values equal the
reference's, for both decoders), the refusals, the library's entries and size arithmetic, and the restatement
(tests/s2s_dnri_restatement.py) pinned to the golden vectors of tools/make_golden_s2s_dnri.py: in fp64 against the reference
after .double() at 1e-12, in fp32 against its fp32 values at 1e-6 (the bars of tests/test_s2s_locs.py).  The GPU tests
(test_gpu_s2s_dnri.py) check the HIP path against the same vectors."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, scale_rel_err

sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import s2s_dnri_restatement as RS                                        # noqa: E402
import make_golden_s2s_dnri as MG                                        # noqa: E402
from make_golden_dynamicvars import perturb_bn_                          # noqa: E402
from aether_amd.nn.seq2seq.dnri import DNRI, DNRI_Decoder, DNRI_Encoder, DNRI_MLP_Decoder   # noqa: E402

CASES = tuple(MG.CASES)
DECODERS = tuple(MG.DECODERS)
LOSS_NAMES = ("gaussian_norm", "crossent_tf2_uniform")
N_KEYS = {"rec": 81, "mlp": 72}
T0 = MG.T - 1                                                            # burn-in steps in front of the predicted ones


def golden(D):
    return np.load(os.path.join(GOLDEN, f"s2s_dnri_D{D}.npz"))


def build(D, dec, tag, device=None, extra=None):
    """The drop-in model of fixture case ``tag`` with decoder ``dec``, constructed as the fixture's reference model was
    -> (model, params, fixture)."""
    d = golden(D)
    B, N, skip = MG.CASES[tag]
    params = MG.model_params(N, D, skip, MG.DECODERS[dec], extra)
    torch.manual_seed(int(d["seed"]))
    model = DNRI(params, device=None).eval()
    with torch.no_grad():
        perturb_bn_(model)
    return (model if device is None else model.to(device)), params, d


def restatement(model, tag, dtype):
    skip = MG.CASES[tag][2]
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return RS.Model(sd, dtype, 3, skip, 0.5)


@pytest.fixture
def one_thread():
    """The fixtures' fp32 values were computed on one thread (a fixed reduction order); the fp32 restatement is compared with
    them on one thread too."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# -- construction -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", DECODERS)
def test_constructs_like_the_reference(D, dec):
    model, _, d = build(D, dec, "B2N5")
    sd = model.state_dict()
    keys = [str(k) for k in d[f"{dec}.keys"]]
    assert len(keys) == N_KEYS[dec] and list(sd.keys()) == keys
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in d[f"{dec}.shapes"]]
    sums, absum = d[f"{dec}.sums"], d[f"{dec}.abs"]
    assert len(sums) == len(absum) == len(keys)
    for i, (k, v) in enumerate(sd.items()):
        bar = 1e-9 * max(1.0, float(absum[i]))
        assert abs(float(v.double().sum()) - float(sums[i])) <= bar, k
        assert abs(float(v.double().abs().sum()) - float(absum[i])) <= bar, k
    h, N, E = int(d["hidden"]), 5, 20
    assert isinstance(model.encoder, DNRI_Encoder)
    assert isinstance(model.decoder, DNRI_Decoder if dec == "rec" else DNRI_MLP_Decoder)
    # the non-trainable one-hot Parameters keep the reference's shapes and its edge order (receiver of edge e)
    assert sd["encoder.edge2node_mat"].shape == (N, E) and sd["decoder.edge2node_mat"].shape == (E, N)
    assert not model.encoder.edge2node_mat.requires_grad and not model.decoder.edge2node_mat.requires_grad
    send, recv = np.where(np.ones((N, N)) - np.eye(N))
    assert torch.equal(sd["decoder.edge2node_mat"].argmax(1), torch.from_numpy(recv))
    assert torch.equal(sd["encoder.edge2node_mat"], sd["decoder.edge2node_mat"].t())
    assert torch.equal(model.encoder.send_edges, torch.from_numpy(send))
    assert sd["encoder.mlp1.model.0.weight"].shape == (h, 2 * D) and sd["encoder.mlp2.model.0.weight"].shape == (h, 2 * h)
    assert sd["encoder.mlp4.model.0.weight"].shape == (h, 3 * h)
    if dec == "rec":
        assert sd["decoder.input_n.weight"].shape == (h, 2 * D) and sd["decoder.msg_fc1.1.weight"].shape == (h, 2 * h)
        assert not any(k.startswith("decoder.present") for k in sd)
    else:
        assert sd["decoder.msg_fc1.1.weight"].shape == (h, 4 * D) and sd["decoder.out_fc1.weight"].shape == (h, 2 * D + h)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})             # a checkpoint with the reference's keys loads


def test_constructor_and_refusal_surface():
    from aether_amd import _lib
    params = MG.model_params(5, 2, False)
    with pytest.raises(ValueError, match="input_size"):
        DNRI(dict(params, input_size=5), device=None)
    with pytest.raises(ValueError, match="lstm"):
        DNRI(dict(params, encoder_rnn_type="gru"), device=None)
    with pytest.raises(ValueError, match="used edge type"):
        DNRI(dict(params, num_edge_types=1, skip_first=True), device=None)
    model = DNRI(dict(params, kl_coef=0.25, teacher_forcing_steps=3, val_teacher_forcing_steps=2), device=None).eval()
    assert model.kl_coef == 0.25 and model.teacher_forcing_steps == 3 and model.val_teacher_forcing_steps == 2
    assert model.num_vars == 5 and model.num_edge_types == 2 and model.gumbel_temp == 0.5 and model.num_dims == 2
    x = torch.zeros(2, 4, 5, 4)
    with pytest.raises(_lib.AetherHipError, match="is_train"):
        model.calculate_loss(x, is_train=True)
    for call in (lambda: model.predict_future(x, 2), lambda: model.predict_future(x, 2, graph=True),
                 lambda: model.predict_future(x, 2, return_everything=True), lambda: model.calculate_loss(x, is_train=False),
                 lambda: model.encoder(x),
                 lambda: model.single_step_forward(x[:, 0], torch.zeros(2, 5, 128), torch.zeros(2, 20, 2), True)):
        with pytest.raises(_lib.AetherHipError):                          # CPU tensors: there is no CPU fallback
            call()
    with pytest.raises(_lib.AetherHipError, match="hard_sample"):
        model.single_step_forward(x[:, 0], torch.zeros(2, 5, 128), torch.zeros(2, 20, 2), False)
    # the modules' own steps run through the model
    with pytest.raises(_lib.AetherHipError, match="through the model"):
        model.decoder(x[:, 0], torch.zeros(2, 5, 128), torch.zeros(2, 20, 2))
    with pytest.raises(_lib.AetherHipError, match="through the model"):
        DNRI_Encoder(params)(x)                                           # (an encoder that belongs to no model)
    pf = inspect.signature(DNRI.predict_future).parameters
    assert list(pf)[1:] == ["inputs", "prediction_steps", "return_edges", "return_everything", "uniform", "graph"]
    cl = inspect.signature(DNRI.calculate_loss).parameters
    assert list(cl)[1:] == ["inputs", "is_train", "teacher_forcing", "return_edges", "return_logits", "use_prior_logits", "uniform"]
    ss = inspect.signature(DNRI.single_step_forward).parameters
    assert list(ss)[1:] == ["inputs", "decoder_hidden", "edge_logits", "hard_sample", "uniform"]
    assert model.decoder.get_initial_hidden(x).shape == (2, 5, 128)
    mlp = DNRI(dict(params, decoder_type="ref_mlp"), device=None)
    assert mlp.decoder.get_initial_hidden(x) is None
    for name in ("save", "load", "nll", "kl_categorical_learned", "kl_categorical_avg", "single_step_forward"):
        assert callable(getattr(model, name))
    p, t = torch.randn(2, 3, 5, 4), torch.randn(2, 3, 5, 4)
    assert torch.allclose(model.nll(p, t), torch.nn.functional.binary_cross_entropy_with_logits(p, t, reduction="none")
                          .view(2, -1).sum(1))


def test_save_and_load_round_trip(tmp_path):
    a, _, _ = build(2, "mlp", "B1N2")
    path = str(tmp_path / "dnri.pt")
    a.save(path)
    torch.manual_seed(1)
    b = DNRI(MG.model_params(2, 2, False, "ref_mlp"), device=None)
    b.load(path)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


def test_library_declares_the_dnri_entries():
    from aether_amd import _lib
    names = ("aether_s2s_dnri_plan_bytes", "aether_s2s_dnri_plan_build", "aether_s2s_dnri_workspace_bytes",
             "aether_s2s_dnri_step", "aether_s2s_dnri_rollout", "aether_s2s_dnri_encoder_features")
    hdr = open(os.path.join(REPO, "include", "aether_hip.h")).read()
    lib = _lib.load()
    for name in names:
        assert name in _lib.SIGNATURES and name + "(" in hdr and hasattr(lib, name), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name.replace("_dnri_", "_locs_")], name     # one for one
    # host-only size arithmetic.  The plan: a decoder must be named (a non-null pointer; only its nullness is read), bad
    # sizes give 0; it holds no filter image, so it is smaller than LoCS's.
    rec, mlp = (1, None), (None, 1)
    for D in (2, 3):
        assert 0 < lib.aether_s2s_dnri_plan_bytes(*rec, D, 128, 128, 64, 3, 64, 2, 0) < \
            lib.aether_s2s_locs_plan_bytes(*rec, D, 128, 128, 64, 3, 64, 2, 0)
        assert 0 < lib.aether_s2s_dnri_plan_bytes(*mlp, D, 128, 128, 64, 3, 64, 2, 1) < \
            lib.aether_s2s_locs_plan_bytes(*mlp, D, 128, 128, 64, 3, 64, 2, 1)
    assert lib.aether_s2s_dnri_plan_bytes(None, None, 2, 128, 128, 64, 3, 64, 2, 0) == 0
    assert lib.aether_s2s_dnri_plan_bytes(1, 1, 2, 128, 128, 64, 3, 64, 2, 0) == 0
    assert lib.aether_s2s_dnri_plan_bytes(*rec, 2, 100, 128, 64, 3, 64, 2, 0) == 0
    assert lib.aether_s2s_dnri_plan_bytes(*rec, 4, 128, 128, 64, 3, 64, 2, 0) == 0
    assert lib.aether_s2s_dnri_plan_bytes(*mlp, 2, 128, 128, 64, 3, 64, 1, 1) == 0      # no used edge type
    # the workspace is smaller than the LoCS step's at the same shape, by at least the frame, edge-attribute, filter and
    # present-message rows that step holds: rel_feat, Rinv, edge_attr (+ padded), edge_pos, the filtered rows [E][he] and the
    # present messages' K [E][hd] + [E][hd]
    for D, he, hd, Nn, E in ((2, 128, 128, 10, 40), (3, 128, 64, 15, 60), (2, 512, 512, 640, 2560), (3, 256, 256, 2560, 48640)):
        got = lib.aether_s2s_dnri_workspace_bytes(D, he, hd, 64, 64, 2, Nn, E)
        locs = lib.aether_s2s_locs_workspace_bytes(D, he, hd, 64, 64, 2, Nn, E)
        O = D * (D - 1) // 2
        EA = 5 * D + O
        frame_rows = 4 * (Nn * 2 * D + Nn * D * D + E * EA + E * 32 + E * (D + O) + E * he + 2 * E * hd + E * hd)
        assert 0 < got <= locs - frame_rows, (D, he, hd, Nn, E)
    assert lib.aether_s2s_dnri_workspace_bytes(3, 128, 128, 64, 64, 2, 0, 40) == 0
    assert lib.aether_s2s_dnri_workspace_bytes(4, 128, 128, 64, 64, 2, 10, 40) == 0
    assert lib.aether_s2s_dnri_workspace_bytes(2, 128, 128, 64, 64, 5, 10, 40) == 0


# -- the restatement against the reference's own outputs ----------------------------------------------------------------
def _case(d, dec, tag):
    t = lambda k: torch.from_numpy(d[f"{dec}.{tag}.{k}"])
    return t("in.inputs"), t("in.uniform")


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", DECODERS)
@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference_step(D, dec, tag, one_thread):
    model, _, d = build(D, dec, tag)
    B, N = MG.CASES[tag][:2]
    inputs, _ = _case(d, dec, tag)
    E, R = N * (N - 1), int(d["rnn_hidden"])
    z = torch.from_numpy(d[f"{dec}.{tag}.ref.step_edges"])
    for dtype, ref, bar in ((torch.float64, "ref64", 1e-12), (torch.float32, "ref", 1e-6)):
        m = restatement(model, tag, dtype)
        x0 = inputs[:, 0].to(dtype)
        logits, (h1, c1) = m.prior(x0, (torch.zeros(B, E, R, dtype=dtype), torch.zeros(B, E, R, dtype=dtype)))
        out, hid = m.decoder(x0, m.initial_hidden(B, N), z.to(dtype))
        got = {"prior_logits": logits, "prior_h": h1, "prior_c": c1, "decoder_out": out, "decoder_hidden": hid}
        names = ["decoder_out"] + (["decoder_hidden"] if dec == "rec" else [])
        # the encoder is the same for both decoders and stored once; the prior state is stored in fp32 only (its fp64 logits are)
        names += ["prior_logits"] + (["prior_h", "prior_c"] if ref == "ref" else [])
        for name in names:
            want = torch.from_numpy(d[f"{dec if name.startswith('decoder') else 'rec'}.{tag}.{ref}.{name}"])
            assert scale_rel_err(got[name], want) <= bar, (name, str(dtype))


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", DECODERS)
@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_predict_future(D, dec, tag, one_thread):
    """3 burn-in + 4 predicted steps through the hard samples, the burn-in steps' outputs included (return_everything): every
    sampled edge type equals the reference's (the generator accepted the noise seed on that condition); fp64 against the
    reference after .double() at 1e-12, fp32 against its fp32 values at the project's 1e-5 (seven steps of fp32 rounding)."""
    model, _, d = build(D, dec, tag)
    inputs, U = _case(d, dec, tag)
    want_e = torch.from_numpy(d[f"{dec}.{tag}.ref.everything_edges"])
    for dtype, ref, bar in ((torch.float64, "ref64", 1e-12), (torch.float32, "ref", 1e-5)):
        m = restatement(model, tag, dtype)
        preds, edges = m.predict_future(inputs, int(d["steps"]), U.to(dtype), everything=True)
        assert torch.equal(edges.argmax(-1), want_e.argmax(-1)), str(dtype)
        assert scale_rel_err(preds, torch.from_numpy(d[f"{dec}.{tag}.{ref}.everything"])) <= bar, str(dtype)
        plain, _ = m.predict_future(inputs, int(d["steps"]), U.to(dtype))
        assert torch.equal(plain, preds[:, T0:])


def loss_model(D, dec, name, device=None):
    """The drop-in model of the loss fixture ``name`` (the B2N5 case's model with that loss configuration)."""
    return build(D, dec, "B2N5", device, MG.MS.LOSS_CONFIGS[name])


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", DECODERS)
@pytest.mark.parametrize("name", LOSS_NAMES)
def test_restatement_reproduces_the_evaluation_loss(D, dec, name, one_thread):
    """DNRI_Encoder.forward and calculate_loss(is_train=False): posterior logits, predictions and the loss terms."""
    model, params, d = loss_model(D, dec, name)
    t = lambda k: torch.from_numpy(d[k])
    inputs, U = t(f"{dec}.loss.in.inputs"), t(f"{dec}.loss.{name}.uniform")
    for dtype, ref, bar in ((torch.float64, ".ref64", 1e-12), (torch.float32, "", 1e-6)):
        m = restatement(model, "B2N5", dtype)
        got = m.calculate_loss(params, inputs, U)
        for key, g in zip(("loss", "nll", "kl", "posterior", "predictions"), got):
            assert scale_rel_err(g, t(f"{dec}.loss.{name}{ref}.{key}")) <= bar, (key, str(dtype))


def test_eval_forward_prediction_takes_the_model_unchanged():
    """aether_amd.evaluate.eval_forward_prediction calls predict_future(inputs[:, :burn_in], steps, **kwargs): the signature
    of DNRI.predict_future takes that call, with and without the extra keywords a caller may pass on."""
    sig = inspect.signature(DNRI.predict_future)
    sig.bind(None, torch.zeros(1, 3, 5, 4), 4)
    sig.bind(None, torch.zeros(1, 3, 5, 4), 4, graph=True, uniform=None)
    assert "charges" not in sig.parameters                               # (evaluate.py passes charges only to models naming them)
