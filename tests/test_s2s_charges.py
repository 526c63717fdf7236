"""The charge-aware seq2seq Aether (nn/seq2seq/ablations/aether_charges.py), host side: construction (keys, order, shapes and
seeded values equal the reference's), the refusals, the restatement (tests/s2s_charges_restatement.py) pinned to the golden
vectors of tools/make_golden_s2s_charges.py, and the fold -- bias tables and four one-hot filter features instead of the
16-wide embedding -- held exact in fp64.  The GPU tests (test_gpu_s2s_charges.py) check the HIP path against both."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, scale_rel_err

sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import s2s_charges_restatement as RS                                     # noqa: E402

CASES = ("B2N5", "B3N5", "B1N2")


def golden(D):
    return np.load(os.path.join(GOLDEN, f"s2s_charges_D{D}.npz"))


def build(D, tag, device=None):
    """The drop-in model of fixture case ``tag``, constructed as the fixture's reference model was -> (model, fixture)."""
    import make_golden_s2s_charges as MG
    from make_golden_dynamicvars import perturb_bn_
    from aether_amd.nn.seq2seq.ablations.aether_charges import AetherCharges
    d = golden(D)
    B, N, skip, _ = MG.CASES[tag]
    torch.manual_seed(int(d["seed"]))
    model = AetherCharges(MG.model_params(N, D, skip), device=None).eval()
    with torch.no_grad():
        perturb_bn_(model)
    return (model if device is None else model.to(device)), d


def restatement(model, D, skip, dtype, folded=False, frames_dtype=None):
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return RS.Model(sd, dtype, D == 3, "polar", 3, skip, 0.5, folded=folded, frames_dtype=frames_dtype)


@pytest.fixture
def one_thread():
    """The fixtures' fp32 values were computed on one thread (tools/make_golden_s2s_charges.py: a fixed reduction order); the
    fp32 restatement is compared with them on one thread too, or its GEMMs sum in another order."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def case_inputs(d, tag):
    from aether_amd.nn.seq2seq.ablations.aether_charges import AetherCharges
    t = lambda k: torch.from_numpy(d[f"{tag}.{k}"])
    charges = t("in.charges")
    return t("in.inputs"), charges, AetherCharges.charge_to_index(charges), t("in.uniform")


# -- construction -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
def test_constructs_like_the_reference(D):
    model, d = build(D, "B2N5")
    sd = model.state_dict()
    keys = [str(k) for k in d["keys"]]
    assert len(keys) == 89 and list(sd.keys()) == keys
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in d["shapes"]]
    for k, v in sd.items():
        if v.dtype.is_floating_point:
            assert abs(float(v.double().sum()) - float(d["sum." + k])) <= 1e-9 * max(1.0, float(d["abs." + k])), k
            assert abs(float(v.double().abs().sum()) - float(d["abs." + k])) <= 1e-9 * max(1.0, float(d["abs." + k])), k
    first = lambda p: min(i for i, k in enumerate(keys) if k.startswith(p))
    assert first("encoder.") < first("decoder.") < first("field_net.") < first("coordinate_embedding.") < first("charge_embedding.")
    EA, RF, h = 2 * (4 * D + D * (D - 1) // 2) + 3 * D, 7 * D + D * (D - 1) // 2, int(d["hidden"])
    assert sd["field_net.0.weight"].shape == (h, h + 16) and sd["charge_embedding.weight"].shape == (2, 16)
    assert sd["encoder.res1.weight"].shape == (h, RF + 16) and sd["decoder.input_n.weight"].shape == (h, RF + 16)
    assert sd["encoder.edge_filter.edge_filter.2.weight"].shape == ((EA + 32) * h, h)
    assert sd["decoder.present_msg_fc1.1.weight"].shape == (h, EA + 32)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})             # a checkpoint with the reference's keys loads


def test_refusals_and_signatures():
    import make_golden_s2s_charges as MG
    from aether_amd import _lib
    from aether_amd.nn.seq2seq.ablations import AetherCharges
    with pytest.raises(ValueError, match="ref_mlp"):
        AetherCharges(MG.model_params(5, 2, False, {"decoder_type": "ref_mlp"}), device=None)
    model = AetherCharges(MG.model_params(5, 2, False), device=None).eval()
    x = torch.zeros(2, 4, 5, 4)
    with pytest.raises(ValueError, match="charges"):
        model.predict_future(x, 2)                                        # charges=None
    with pytest.raises(ValueError, match="charges"):
        model.calculate_loss(x, is_train=False)
    with pytest.raises(_lib.AetherHipError):                              # CPU tensors: there is no CPU fallback
        model.predict_future(x, 2, charges=torch.ones(2, 5))
    with pytest.raises(_lib.AetherHipError):
        model.predict_field(x[:, 0], torch.zeros(2, 5, dtype=torch.long))
    assert "charges" in inspect.signature(AetherCharges.calculate_loss).parameters     # the runner looks for it (train.py:96)
    pf = inspect.signature(AetherCharges.predict_future).parameters
    assert list(pf)[1:] == ["inputs", "prediction_steps", "return_edges", "return_everything", "charges", "uniform", "graph"]
    assert torch.equal(AetherCharges.charge_to_index(torch.tensor([1.0, -1.0, 0.0])), torch.tensor([1, 0, 0]))


def test_header_declares_the_charge_entries():
    from aether_amd import _lib
    names = ("aether_s2s_charges_plan_bytes", "aether_s2s_charges_plan_build", "aether_s2s_charges_workspace_bytes",
             "aether_s2s_charges_step", "aether_s2s_charges_rollout", "aether_s2s_charges_encoder_features",
             "aether_s2s_charges_field_workspace_bytes", "aether_s2s_charges_field")
    hdr = open(os.path.join(REPO, "include", "aether_hip.h")).read()
    lib = _lib.load()
    for name in names:
        assert name in _lib.SIGNATURES and name + "(" in hdr and hasattr(lib, name), name
    # host-only size arithmetic: the plan holds the plain plan and more, bad sizes give 0, and the filter image is the
    # ordinary 28- / 43-feature image
    assert lib.aether_s2s_charges_plan_bytes(2, 128, 128, 64, 3, 64, 2) > lib.aether_s2s_plan_bytes(2, 128, 128, 64, 3, 64, 2)
    assert lib.aether_s2s_charges_plan_bytes(2, 100, 128, 64, 3, 64, 2) == 0
    assert lib.aether_s2s_charges_workspace_bytes(3, 128, 128, 64, 64, 2, 10, 40) > \
        lib.aether_s2s_step_workspace_bytes(3, 128, 128, 64, 64, 2, 10, 40) + 40 * 43 * 4
    assert lib.aether_s2s_charges_workspace_bytes(3, 128, 128, 64, 64, 2, 0, 40) == 0
    assert lib.aether_s2s_filter_image_bytes(28, 128) > lib.aether_s2s_filter_image_bytes(24, 128)


# -- the restatement against the reference's own outputs ----------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference_step(D, tag, one_thread):
    """Field query, prior step and decoder step: fp64 against the reference after .double() at 1e-12, fp32 against its fp32
    values at 1e-6 (the bars of tests/test_s2s_markov.py)."""
    import make_golden_s2s_charges as MG
    model, d = build(D, tag)
    B, N, skip, _ = MG.CASES[tag]
    inputs, _, cidx, _ = case_inputs(d, tag)
    E, R, H = N * (N - 1), int(d["rnn_hidden"]), int(d["hidden"])
    z = torch.from_numpy(d[f"{tag}.ref.step_edges"])
    for dtype, ref, bar in ((torch.float64, "ref64", 1e-12), (torch.float32, "ref", 1e-6)):
        m = restatement(model, D, skip, dtype)
        x0 = inputs[:, 0].to(dtype)
        want = lambda k: torch.from_numpy(d[f"{tag}.{ref}.{k}"])
        field = m.field(x0, cidx)
        logits, (h1, c1) = m.prior(x0, (torch.zeros(B, E, R, dtype=dtype), torch.zeros(B, E, R, dtype=dtype)), field, cidx)
        out, hid = m.decoder(x0, torch.zeros(B, N, H, dtype=dtype), z.to(dtype), field, cidx)
        for name, got in (("field0", field), ("prior_logits", logits), ("prior_h", h1), ("prior_c", c1), ("decoder_out", out),
                          ("decoder_hidden", hid)):
            assert scale_rel_err(got, want(name)) <= bar, (name, str(dtype))
    m32 = restatement(model, D, skip, torch.float32)
    x4 = inputs[:, :-1].transpose(2, 1).contiguous()
    assert scale_rel_err(m32.field(x4, cidx), torch.from_numpy(d[f"{tag}.ref.field4"])) <= 1e-6


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_predict_future(D, tag, one_thread):
    """3 burn-in + 4 predicted steps through the hard samples: every sampled edge type equals the reference's (the generator
    accepted the noise seed on that condition), the trajectories agree at the project's 1e-5 (fp32 step by step)."""
    import make_golden_s2s_charges as MG
    model, d = build(D, tag)
    _, _, skip, _ = MG.CASES[tag]
    inputs, _, cidx, U = case_inputs(d, tag)
    want_p, want_e = torch.from_numpy(d[f"{tag}.ref.predictions"]), torch.from_numpy(d[f"{tag}.ref.edges"])
    for dtype, fd in ((torch.float32, None), (torch.float64, torch.float32 if D == 3 else None)):
        m = restatement(model, D, skip, dtype, frames_dtype=fd)
        preds, edges = m.predict_future(inputs, int(d["steps"]), U.to(dtype), cidx)
        assert torch.equal(edges.argmax(-1), want_e.argmax(-1)), str(dtype)
        assert scale_rel_err(preds, want_p) <= 1e-5, str(dtype)


def loss_model(D, name):
    """The drop-in model of the loss fixture ``name`` (the B2N5 case's model with that loss configuration)."""
    import make_golden_s2s_charges as MG
    from make_golden_dynamicvars import perturb_bn_
    from aether_amd.nn.seq2seq.ablations.aether_charges import AetherCharges
    d = golden(D)
    _, N, skip, _ = MG.CASES["B2N5"]
    params = MG.model_params(N, D, skip, MG.MS.LOSS_CONFIGS[name])
    torch.manual_seed(int(d["seed"]))
    model = AetherCharges(params, device=None).eval()
    with torch.no_grad():
        perturb_bn_(model)
    return model, params, d


LOSS_NAMES = ("gaussian_norm", "crossent_tf2_uniform")


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("name", LOSS_NAMES)
def test_restatement_reproduces_the_evaluation_loss(D, name, one_thread):
    """Encoder.forward and calculate_loss(is_train=False): posterior logits, predictions and the loss terms, fp64 against the
    reference after .double() at 1e-12 and fp32 against its fp32 values at 1e-6."""
    model, params, d = loss_model(D, name)
    t = lambda k: torch.from_numpy(d[k])
    inputs, charges, U = t("loss.in.inputs"), t("loss.in.charges"), t(f"loss.{name}.uniform")
    cidx = model.charge_to_index(charges)
    for dtype, ref, bar in ((torch.float64, ".ref64", 1e-12), (torch.float32, "", 1e-6)):
        m = restatement(model, D, params["skip_first"], dtype)
        got = m.calculate_loss(params, inputs, U, cidx)
        for key, g in zip(("loss", "nll", "kl", "posterior", "predictions"), got):
            assert scale_rel_err(g, t(f"loss.{name}{ref}.{key}")) <= bar, (key, str(dtype))


# -- the fold -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("tag", CASES)
def test_the_fold_is_exact_in_fp64(D, tag):
    """Bias tables (2 rows per node layer, 4 per edge layer) and the 28- / 43-feature folded filter against the 56- / 71-
    feature form with the embedding concatenated: the same algebra, <= 1e-12 scale-relative in fp64, step by step and
    through the whole rollout."""
    import make_golden_s2s_charges as MG
    model, d = build(D, tag)
    B, N, skip, _ = MG.CASES[tag]
    inputs, _, cidx, U = case_inputs(d, tag)
    if tag == "B2N5":                                                     # all four (recv, send) charge pairs are hit
        send, recv = torch.where(~torch.eye(N, dtype=bool))
        assert set((2 * cidx[:, recv] + cidx[:, send]).reshape(-1).tolist()) == {0, 1, 2, 3}
    E, R, H = N * (N - 1), int(d["rnn_hidden"]), int(d["hidden"])
    plain, folded = (restatement(model, D, skip, torch.float64, folded=f) for f in (False, True))
    EA = 2 * (4 * D + D * (D - 1) // 2) + 3 * D
    W2f, b2f = RS.fold_filter(folded.enc["edge_filter.edge_filter.2.weight"], folded.enc["edge_filter.edge_filter.2.bias"],
                              folded.emb_w, EA, H)
    assert W2f.shape == ((EA + 4) * H, H) and b2f.shape == ((EA + 4) * H,) and EA + 4 in (28, 43)
    x0 = inputs[:, 0].double()
    z = torch.from_numpy(d[f"{tag}.ref.step_edges"]).double()
    state0 = (torch.zeros(B, E, R, dtype=torch.float64), torch.zeros(B, E, R, dtype=torch.float64))
    outs = []
    for m in (plain, folded):
        field = m.field(x0, cidx)
        logits, (h1, c1) = m.prior(x0, state0, field, cidx)
        out, hid = m.decoder(x0, torch.zeros(B, N, H, dtype=torch.float64), z, field, cidx)
        preds, edges = m.predict_future(inputs, int(d["steps"]), U.double(), cidx)
        outs.append((field, logits, h1, c1, out, hid, preds, edges))
    for a, b in zip(*outs):
        assert scale_rel_err(b, a) <= 1e-12


# -- the metric passes the charges on -------------------------------------------------------------------------------------
def test_eval_forward_prediction_passes_charges_to_models_that_name_them():
    from aether_amd.evaluate import eval_forward_prediction

    class Data:
        feats = torch.arange(5 * 6 * 3 * 4, dtype=torch.float32).view(5, 6, 3, 4)
        charges = torch.tensor([[1., -1., 1.]] * 5) * torch.arange(1, 6).view(5, 1)
        ndim = 2
        torch_unnormalize = staticmethod(lambda t: t)
        __len__ = lambda self: 5

    class Base(torch.nn.Module):
        seen = None

        def _predict(self, inputs, steps):
            return inputs[:, -1:].repeat(1, steps, 1, 1)

    class WithCharges(Base):
        def predict_future(self, inputs, prediction_steps, charges=None):
            self.seen = (self.seen or []) + [charges]
            return self._predict(inputs, prediction_steps)

    class Without(Base):
        def predict_future(self, inputs, prediction_steps):
            return self._predict(inputs, prediction_steps)

    m = WithCharges()
    a = eval_forward_prediction(m, Data(), 3, 2, batch_size=2)
    assert [tuple(c.shape) for c in m.seen] == [(2, 3), (2, 3), (1, 3)]
    assert torch.equal(torch.cat(m.seen), Data.charges)                   # each batch its own rows
    b = eval_forward_prediction(Without(), Data(), 3, 2, batch_size=2)    # unchanged for every other model
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    own = torch.ones(5, 3)
    m.seen = None
    eval_forward_prediction(m, Data(), 3, 2, batch_size=5, charges=own)   # an explicit argument wins
    assert m.seen[0] is own
