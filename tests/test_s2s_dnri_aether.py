"""The seq2seq ablation DNRIAether (nn/seq2seq/ablations/dnri_aether.py: dNRI with the latent field, no frames), host side:
construction (keys, order, shapes and seeded values equal the reference's, for both decoders), the refusals, the library's
entries and size arithmetic, and the restatement (tests/s2s_dnri_aether_restatement.py) pinned to the golden vectors of
tools/make_golden_s2s_dnri_aether.py: in fp64 against the reference after .double() at 1e-12, in fp32 on one thread against its
fp32 values at 1e-6 (1e-5 for the seven-step rollout) -- the bars of tests/test_s2s_dnri.py.  The GPU tests
(test_gpu_s2s_dnri_aether.py) check the HIP path against the same vectors."""
import importlib
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, scale_rel_err

sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import s2s_dnri_aether_restatement as RS                                 # noqa: E402
import make_golden_s2s_dnri_aether as MG                                 # noqa: E402
from make_golden_dynamicvars import perturb_bn_                          # noqa: E402
from make_golden_seq2seq import LOSS_CONFIGS                             # noqa: E402
from aether_amd.nn.seq2seq.ablations.dnri_aether import DNRIAether, DNRI_Decoder, DNRI_Encoder, DNRI_MLP_Decoder   # noqa: E402

CASES = tuple(MG.CASES)
DECODERS = tuple(MG.DECODERS)
LOSS_NAMES = ("gaussian_norm", "crossent_tf2_uniform")
N_KEYS = {"rec": 88, "mlp": 79}
T0 = MG.MD.T - 1                                                         # burn-in steps in front of the predicted ones
ENTRIES = tuple("aether_s2s_dnri_aether_" + n for n in ("plan_bytes", "plan_build", "workspace_bytes", "step", "rollout",
                                                        "encoder_features"))


def golden(D):
    return np.load(os.path.join(GOLDEN, f"s2s_dnri_aether_D{D}.npz"))


def make(params, seed):
    """The drop-in model as the fixtures' reference models were made: seeded constructor, perturbed BatchNorm statistics."""
    torch.manual_seed(seed)
    model = DNRIAether(params, device=None).eval()
    with torch.no_grad():
        perturb_bn_(model)
    return model


def build(D, dec, tag, device=None, extra=None):
    """The drop-in model of fixture case ``tag`` with decoder ``dec`` -> (model, params, fixture)."""
    d = golden(D)
    B, N, skip = MG.CASES[tag]
    params = MG.model_params(N, D, skip, MG.DECODERS[dec], extra)
    model = make(params, int(d["seed"]))
    return (model if device is None else model.to(device)), params, d


def restatement(model, skip, dtype):
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return RS.Model(sd, dtype, 3, skip, 0.5)


@pytest.fixture
def one_thread():
    """The fixtures' fp32 values were computed on one thread (a fixed reduction order)."""
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
    h = int(d["hidden"])
    assert isinstance(model.encoder, DNRI_Encoder)
    assert isinstance(model.decoder, DNRI_Decoder if dec == "rec" else DNRI_MLP_Decoder)
    # the reference creates encoder -> decoder -> field net -> Fourier features; every layer on the raw state has 3D columns
    assert keys[-7:] == [f"field_net.{l}.{p}" for l in (0, 2, 4) for p in ("weight", "bias")] + ["coordinate_embedding.B"]
    assert sd["field_net.4.weight"].shape == (D, h) and sd["coordinate_embedding.B"].shape == (D, h // 2)
    assert sd["encoder.mlp1.model.0.weight"].shape == (h, 3 * D) and sd["encoder.mlp2.model.0.weight"].shape == (h, 2 * h)
    if dec == "rec":
        assert sd["decoder.input_n.weight"].shape == (h, 3 * D) and sd["decoder.msg_fc1.1.weight"].shape == (h, 2 * h)
    else:
        assert sd["decoder.msg_fc1.1.weight"].shape == (h, 6 * D) and sd["decoder.out_fc1.weight"].shape == (h, 3 * D + h)
    assert sd["decoder.out_fc3.weight"].shape == (2 * D, h)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})             # a checkpoint with the reference's keys loads


def test_constructor_and_refusal_surface():
    from aether_amd import _lib
    params = MG.model_params(5, 2, False)
    with pytest.raises(ValueError, match="input_size"):
        DNRIAether(dict(params, input_size=5), device=None)
    with pytest.raises(ValueError, match="input_size"):
        DNRIAether(dict(params, use_3d=True), device=None)                # 3-D field, 2-D state
    with pytest.raises(ValueError, match="used edge type"):
        DNRIAether(dict(params, num_edge_types=1, skip_first=True), device=None)
    model = DNRIAether(dict(params, kl_coef=0.25, val_teacher_forcing_steps=2), device=None).eval()
    assert model.kl_coef == 0.25 and model.val_teacher_forcing_steps == 2 and model.num_dims == 2 and not model.use_3d
    assert model.num_vars == 5 and model.num_edge_types == 2 and model.gumbel_temp == 0.5
    x, f = torch.zeros(2, 4, 5, 4), torch.zeros(2, 5, 2)
    with pytest.raises(_lib.AetherHipError, match="is_train"):
        model.calculate_loss(x, is_train=True)
    for call in (lambda: model.predict_future(x, 2), lambda: model.predict_future(x, 2, graph=True),
                 lambda: model.predict_future(x, 2, return_everything=True), lambda: model.calculate_loss(x, is_train=False),
                 lambda: model.encoder(x, torch.zeros(2, 5, 4, 2)), lambda: model.predict_field(x[:, 0]),
                 lambda: model.single_step_forward(x[:, 0], torch.zeros(2, 5, 128), torch.zeros(2, 20, 2), True, f)):
        with pytest.raises(_lib.AetherHipError):                          # CPU tensors: there is no CPU fallback
            call()
    with pytest.raises(_lib.AetherHipError, match="hard_sample"):
        model.single_step_forward(x[:, 0], torch.zeros(2, 5, 128), torch.zeros(2, 20, 2), False, f)
    # the modules' own steps run through the model
    with pytest.raises(_lib.AetherHipError, match="through the model"):
        model.decoder(x[:, 0], torch.zeros(2, 5, 128), torch.zeros(2, 20, 2), f)
    with pytest.raises(_lib.AetherHipError, match="through the model"):
        model.encoder.single_step_forward(x[:, 0], None, f)
    with pytest.raises(_lib.AetherHipError, match="through the model"):
        DNRI_Encoder(params)(x, torch.zeros(2, 5, 4, 2))                  # (an encoder that belongs to no model)
    # the reference's signatures (dnri_aether.py:87, :96, :142) with the draws and the capture switch behind them
    pf = inspect.signature(DNRIAether.predict_future).parameters
    assert list(pf)[1:] == ["inputs", "prediction_steps", "return_edges", "return_everything", "uniform", "graph"]
    cl = inspect.signature(DNRIAether.calculate_loss).parameters
    assert list(cl)[1:] == ["inputs", "is_train", "teacher_forcing", "return_edges", "return_logits", "use_prior_logits", "uniform"]
    ss = inspect.signature(DNRIAether.single_step_forward).parameters
    assert list(ss)[1:] == ["inputs", "decoder_hidden", "edge_logits", "hard_sample", "predicted_field", "uniform"]
    assert list(inspect.signature(DNRI_Encoder.forward).parameters)[1:] == ["inputs", "predicted_field"]
    assert list(inspect.signature(DNRIAether.predict_field).parameters)[1:] == ["x"]
    assert model.decoder.get_initial_hidden(x).shape == (2, 5, 128)
    assert DNRIAether(dict(params, decoder_type="ref_mlp"), device=None).decoder.get_initial_hidden(x) is None
    # the runner's factory string, under the package
    module, _, name = "nn.seq2seq.ablations.dnri_aether.DNRIAether".rpartition(".")
    assert getattr(importlib.import_module("aether_amd." + module), name) is DNRIAether


def test_save_and_load_round_trip(tmp_path):
    a, _, _ = build(3, "mlp", "B1N2")
    path = str(tmp_path / "dnri_aether.pt")
    a.save(path)
    torch.manual_seed(1)
    b = DNRIAether(MG.model_params(2, 3, False, "ref_mlp"), device=None)
    assert not torch.equal(a.field_net[0].weight, b.field_net[0].weight)
    b.load(path)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


def test_library_declares_the_entries_and_sizes_them():
    from aether_amd import _lib
    hdr = open(os.path.join(REPO, "include", "aether_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name + "(" in hdr and hasattr(lib, name), name
    # the dNRI entries plus the field struct in front (size calls: the same) and the named field arguments
    sig = lambda n: _lib.SIGNATURES[n][1]
    for n in ("plan_bytes", "workspace_bytes"):
        assert _lib.SIGNATURES["aether_s2s_dnri_aether_" + n] == _lib.SIGNATURES["aether_s2s_dnri_" + n]
    assert len(sig("aether_s2s_dnri_aether_plan_build")) == len(sig("aether_s2s_dnri_plan_build")) + 1
    assert len(sig("aether_s2s_dnri_aether_step")) == len(sig("aether_s2s_dnri_step")) + 3           # fp, ext_field, field_out
    assert len(sig("aether_s2s_dnri_aether_rollout")) == len(sig("aether_s2s_dnri_rollout")) + 2     # fp, burn_in_field
    assert len(sig("aether_s2s_dnri_aether_encoder_features")) == len(sig("aether_s2s_dnri_encoder_features")) + 2
    # host-only size arithmetic.  The plan: dNRI's and the fp16 x 2 images of field_net.0 / .2 ([he][he] floats each); smaller
    # than Aether's, which holds the filter image and the frames' padded layers
    rec, mlp = (1, None), (None, 1)
    for D in (2, 3):
        for dec, skip in ((rec, 0), (mlp, 1)):
            for he in (128, 512):
                got = lib.aether_s2s_dnri_aether_plan_bytes(*dec, D, he, 128, 64, 3, 64, 2, skip)
                assert got == lib.aether_s2s_dnri_plan_bytes(*dec, D, he, 128, 64, 3, 64, 2, skip) + 2 * he * he * 4
        assert lib.aether_s2s_dnri_aether_plan_bytes(*rec, D, 128, 128, 64, 3, 64, 2, 0) < \
            lib.aether_s2s_plan_bytes(D, 128, 128, 64, 3, 64, 2)
    for bad in ((None, None, 2, 128, 128, 64, 3, 64, 2, 0), (1, 1, 2, 128, 128, 64, 3, 64, 2, 0),
                (1, None, 2, 100, 128, 64, 3, 64, 2, 0), (1, None, 4, 128, 128, 64, 3, 64, 2, 0),
                (None, 1, 2, 128, 128, 64, 3, 64, 1, 1)):
        assert lib.aether_s2s_dnri_aether_plan_bytes(*bad) == 0, bad
    # the workspace: dNRI's and exactly the field query's rows, each rounded up to 256 bytes -- Fourier features and two hidden
    # layers [n][he], the field [n][D], ext [n][3D]; smaller than Aether's, which holds the frames
    up = lambda floats: (floats * 4 + 255) // 256 * 256
    for D, he, hd, Nn, E in ((2, 128, 128, 10, 40), (3, 128, 64, 15, 60), (2, 512, 512, 640, 2560), (3, 256, 256, 2560, 48640)):
        got = lib.aether_s2s_dnri_aether_workspace_bytes(D, he, hd, 64, 64, 2, Nn, E)
        dnri = lib.aether_s2s_dnri_workspace_bytes(D, he, hd, 64, 64, 2, Nn, E)
        assert got == dnri + 3 * up(Nn * he) + up(Nn * D) + up(Nn * 3 * D), (D, he, hd, Nn, E)
        assert got < lib.aether_s2s_step_workspace_bytes(D, he, hd, 64, 64, 2, Nn, E)
    assert lib.aether_s2s_dnri_aether_workspace_bytes(3, 128, 128, 64, 64, 2, 0, 40) == 0
    assert lib.aether_s2s_dnri_aether_workspace_bytes(4, 128, 128, 64, 64, 2, 10, 40) == 0
    assert lib.aether_s2s_dnri_aether_workspace_bytes(2, 128, 128, 64, 64, 5, 10, 40) == 0


# -- the restatement against the reference's own outputs ----------------------------------------------------------------
def _case(d, dec, tag):
    t = lambda k: torch.from_numpy(d[f"{dec}.{tag}.{k}"])
    return t("in.inputs"), t("in.uniform")


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", DECODERS)
@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference_step(D, dec, tag, one_thread):
    model, _, d = build(D, dec, tag)
    B, N, skip = MG.CASES[tag]
    inputs, _ = _case(d, dec, tag)
    E, R = N * (N - 1), int(d["rnn_hidden"])
    z = torch.from_numpy(d[f"{dec}.{tag}.ref.step_edges"])
    for dtype, ref, bar in ((torch.float64, "ref64", 1e-12), (torch.float32, "ref", 1e-6)):
        m = restatement(model, skip, dtype)
        x0 = inputs[:, 0].to(dtype)
        field = m.field(x0)
        logits, (h1, c1) = m.prior(x0, (torch.zeros(B, E, R, dtype=dtype), torch.zeros(B, E, R, dtype=dtype)), field)
        out, hid = m.decoder(x0, m.initial_hidden(B, N), z.to(dtype), field)
        got = {"field": field, "prior_logits": logits, "prior_h": h1, "prior_c": c1, "decoder_out": out, "decoder_hidden": hid}
        names = ["field", "decoder_out", "prior_logits"] + (["decoder_hidden"] if dec == "rec" else [])
        names += ["prior_h", "prior_c"] if ref == "ref" else []          # (the prior state is stored in fp32 only)
        for name in names:
            assert scale_rel_err(got[name], torch.from_numpy(d[f"{dec}.{tag}.{ref}.{name}"])) <= bar, (name, str(dtype))


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", DECODERS)
@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_predict_future(D, dec, tag, one_thread):
    """3 burn-in + 4 predicted steps through the hard samples, the burn-in steps' outputs included (return_everything): every
    sampled edge type equals the reference's; fp64 at 1e-12, fp32 at 1e-5 (seven steps of fp32 rounding)."""
    model, _, d = build(D, dec, tag)
    inputs, U = _case(d, dec, tag)
    want_e = torch.from_numpy(d[f"{dec}.{tag}.ref.everything_edges"])
    for dtype, ref, bar in ((torch.float64, "ref64", 1e-12), (torch.float32, "ref", 1e-5)):
        m = restatement(model, MG.CASES[tag][2], dtype)
        preds, edges = m.predict_future(inputs, int(d["steps"]), U.to(dtype), everything=True)
        assert torch.equal(edges.argmax(-1), want_e.argmax(-1)), str(dtype)
        assert scale_rel_err(preds, torch.from_numpy(d[f"{dec}.{tag}.{ref}.everything"])) <= bar, str(dtype)
        plain, _ = m.predict_future(inputs, int(d["steps"]), U.to(dtype))
        assert torch.equal(plain, preds[:, T0:])


def loss_model(D, dec, name, device=None):
    """The drop-in model of the loss fixture ``name`` (the B2N5 case's model with that loss configuration)."""
    return build(D, dec, "B2N5", device, LOSS_CONFIGS[name])


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", DECODERS)
@pytest.mark.parametrize("name", LOSS_NAMES)
def test_restatement_reproduces_the_evaluation_loss(D, dec, name, one_thread):
    """DNRI_Encoder.forward on [inputs | field] and calculate_loss(is_train=False): posterior logits, predictions, loss terms."""
    model, params, d = loss_model(D, dec, name)
    t = lambda k: torch.from_numpy(d[k])
    inputs, U = t(f"{dec}.loss.in.inputs"), t(f"{dec}.loss.{name}.uniform")
    for dtype, ref, bar in ((torch.float64, ".ref64", 1e-12), (torch.float32, "", 1e-6)):
        m = restatement(model, False, dtype)
        got = m.calculate_loss(params, inputs, U)
        for key, g in zip(("loss", "nll", "kl", "posterior", "predictions"), got):
            assert scale_rel_err(g, t(f"{dec}.loss.{name}{ref}.{key}")) <= bar, (key, str(dtype))


def test_eval_forward_prediction_takes_the_model_unchanged():
    """aether_amd.evaluate.eval_forward_prediction calls predict_future(inputs[:, :burn_in], steps, **kwargs)."""
    sig = inspect.signature(DNRIAether.predict_future)
    sig.bind(None, torch.zeros(1, 3, 5, 4), 4)
    sig.bind(None, torch.zeros(1, 3, 5, 4), 4, graph=True, uniform=None)
    assert "charges" not in sig.parameters
