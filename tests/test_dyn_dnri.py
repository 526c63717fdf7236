"""The variable-N dNRI baseline (nn/dynamicvars/dnri_dynamicvars.py), host side: construction (keys, order, shapes and seeded
values equal the reference's), save / load, the refusals, the library's entries and size arithmetic, and the restatement
(tests/dyn_dnri_restatement.py) pinned to the golden vectors of tools/make_golden_dyn_dnri.py: in fp64 against the reference
after .double() at 1e-12, in fp32 against its fp32 values at the fp32 floor (1e-6 for one step, 1e-5 through the loop: the
bars of tests/test_s2s_dnri.py), every hard sample equal.  The GPU tests (test_gpu_dyn_dnri.py) check the HIP path against
the same vectors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, scale_rel_err

sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import dyn_dnri_restatement as RS                                        # noqa: E402
import make_golden_dyn_dnri as MG                                        # noqa: E402
from make_golden_dynamicvars import perturb_bn_                          # noqa: E402

CASES = tuple(MG.CASES)
N_KEYS = {"N9": 83, "N14": 79, "N3": 63, "N2": 79}


def golden():
    return np.load(os.path.join(GOLDEN, "dyn_dnri.npz"))


def build(tag, device=None, extra=None):
    """The drop-in model of fixture case ``tag``, constructed as the fixture's reference model was -> (model, params, fixture)."""
    from aether_amd.nn.dynamicvars.dnri_dynamicvars import DNRIDynamicVars
    d = golden()
    params = dict(MG.model_params(tag), **(extra or {}))
    torch.manual_seed(int(d["seed"]))
    model = DNRIDynamicVars(params, device=None).eval()
    with torch.no_grad():
        perturb_bn_(model)
    return (model if device is None else model.to(device)), params, d


def restatement(model, tag, dtype):
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    return RS.Model(sd, dtype, 3, MG.CASES[tag][2], MG.TAU)


def scene(d, tag):
    """-> dict of the case's tensors: inputs [1, T, Nmax, 4], masks, burn, node_inds[t], graph_info[t], uniform[t]."""
    t = lambda k: torch.from_numpy(d[f"{tag}.{k}"])
    T = MG.CASES[tag][3]
    masks = t("in.masks")
    return dict(inputs=t("in.inputs"), masks=masks, burn=t("in.burn"), T=T,
                node_inds=[masks[0, s].nonzero()[:, -1] for s in range(T)],
                graph_info=[(t(f"send.{s}"), t(f"recv.{s}"), t(f"e2n.{s}")) for s in range(T)],
                uniform=[t(f"uniform.{s}") for s in range(T - 1)], edges=[t(f"ref.edges.{s}") for s in range(T - 1)],
                state0=(t("in.state0_h"), t("in.state0_c")), hidden0=t("in.hidden0"), step_edges=t("ref.step_edges"))


@pytest.fixture
def one_thread():
    """The fixtures' fp32 values were computed on one thread (a fixed reduction order); so is the fp32 restatement."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


# -- construction -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_constructs_like_the_reference(tag):
    from aether_amd.nn.dynamicvars.dnri_dynamicvars import DNRI_DynamicVars_Decoder, DNRI_DynamicVars_Encoder
    model, params, d = build(tag)
    sd = model.state_dict()
    keys = [str(k) for k in d[f"{tag}.keys"]]
    assert len(keys) == N_KEYS[tag] and list(sd.keys()) == keys
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in d[f"{tag}.shapes"]]
    sums, absum = d[f"{tag}.sums"], d[f"{tag}.abs"]
    for i, (k, v) in enumerate(sd.items()):
        bar = 1e-9 * max(1.0, float(absum[i]))
        assert abs(float(v.double().sum()) - float(sums[i])) <= bar, k
        assert abs(float(v.double().abs().sum()) - float(absum[i])) <= bar, k
    assert isinstance(model.encoder, DNRI_DynamicVars_Encoder) and isinstance(model.decoder, DNRI_DynamicVars_Decoder)
    # held as parameters, never read by the prediction path
    assert "encoder.reverse_rnn.weight_ih_l0" in sd and "encoder.encoder_fc_out.0.weight" in sd
    assert sd["encoder.mlp1.model.0.weight"].shape == (128, 4) and sd["encoder.mlp4.model.0.weight"].shape == (128, 384)
    assert sd["decoder.input_n.weight"].shape == (128, 4) and sd["decoder.msg_fc1.1.weight"].shape == (128, 256)
    assert ("encoder.mlp1.bn.weight" in sd) == (not params["no_encoder_bn"])
    assert not any("present" in k or "edge_filter" in k or "field" in k for k in sd)
    model.load_state_dict({k: v.clone() for k, v in sd.items()})             # a checkpoint with the reference's keys loads


def test_save_and_load_round_trip(tmp_path):
    from aether_amd.nn.dynamicvars.dnri_dynamicvars import DNRIDynamicVars
    a, params, _ = build("N9")
    path = str(tmp_path / "dyn_dnri.pt")
    a.save(path)
    torch.manual_seed(1)
    b = DNRIDynamicVars(params, device=None)
    b.load(path)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)


# -- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_are_raised_by_name():
    from aether_amd import _lib
    from aether_amd.nn.dynamicvars.dnri_dynamicvars import DNRIDynamicVars
    params = MG.model_params("N9")
    with pytest.raises(ValueError, match="decoder_dropout"):
        DNRIDynamicVars(dict(params, decoder_dropout=0.1), device=None)
    with pytest.raises(ValueError, match="lstm"):
        DNRIDynamicVars(dict(params, encoder_rnn_type="gru"), device=None)
    with pytest.raises(NotImplementedError, match="normalize_all"):
        DNRIDynamicVars(dict(params, encoder_normalize_mode="normalize_inp"), device=None)
    model, _, d = build("N9")
    s = scene(d, "N9")
    x, m = s["inputs"], s["masks"]
    ni, gi = [s["node_inds"]], [s["graph_info"]]
    for name in ("calculate_loss", "predict_future_fixedwindow", "get_prior_posterior", "get_edge_probs"):
        with pytest.raises(_lib.AetherHipError, match=name):
            getattr(model, name)(x, m, ni, gi)
    with pytest.raises(_lib.AetherHipError, match="posterior"):
        model.encoder(x, m, ni, gi)
    hidden, logits = torch.zeros(1, 9, 128), torch.zeros(1, 42, 3)
    with pytest.raises(_lib.AetherHipError, match="hard_sample"):
        model.single_step_forward(x[:, 0], m[:, 0], gi[0][0], hidden, logits, False)
    # CPU tensors: there is no CPU fallback, in any entry of the path
    state = model.encoder.get_initial_hidden(x)
    assert state[0].shape == (1, 72, 64) and model.decoder.get_initial_hidden(x).shape == (1, 9, 128)
    for call in (lambda: model.predict_future(x, m, ni, gi, s["burn"]),
                 lambda: model.predict_future_batched(x, m, ni, gi, s["burn"]),
                 lambda: model.predict_future_packed(x, m, s["burn"], None),
                 lambda: model.single_step_forward(x[:, 0], m[:, 0], gi[0][0], hidden, logits, True),
                 lambda: model.encoder.single_step_forward(x[:, 0], m[:, 0], ni[0][0], gi[0][0], state),
                 lambda: model.decoder(x[:, 0], hidden, logits, m[:, 0], gi[0][0])):
        with pytest.raises(_lib.AetherHipError, match="CPU tensor"):
            call()
    # training mode is refused before anything else is looked at (what can be checked without a device: the model's guard
    # comes behind the CPU check, so it is read off the code path with a tensor that claims to be on the device)
    model.train()

    class OnDevice:
        is_cuda = True

        def size(self, i):
            return 1
    with pytest.raises(_lib.AetherHipError, match="training mode"):
        model.predict_future(OnDevice(), m, ni, gi, s["burn"])
    with pytest.raises(_lib.AetherHipError, match="training mode"):
        model.predict_future_packed(OnDevice(), m, s["burn"], None)


def _config(K=3, skip=1):
    from aether_amd.nn.dynamicvars.aether_dynamicvars import _DynStepConfig
    return _DynStepConfig(64, 128, 64, 3, 64, K, 128, skip, 0, 0, 10, 0.5)


def test_library_declares_the_entries_and_refuses_on_the_host():
    """The new C-ABI symbols exist; the size arithmetic is host-only: the dNRI step's workspace is smaller than the Aether
    step's for the same sizes; a one-object scene and an edge count other than n min(k, n - 1) are refused by name, by the
    size function and by the rollout entry before it touches a pointer."""
    from aether_amd import _lib
    names = ("aether_dyn_dnri_prior_workspace_bytes", "aether_dyn_dnri_prior_step", "aether_dyn_dnri_decoder_workspace_bytes",
             "aether_dyn_dnri_decoder_step_batched", "aether_dyn_dnri_step_batched_workspace_bytes", "aether_dyn_dnri_step_batched",
             "aether_dyn_dnri_rollout_batched_workspace_bytes", "aether_dyn_dnri_rollout_batched")
    hdr = open(os.path.join(REPO, "include", "aether_hip.h")).read()
    lib = _lib.load()
    for name in names:
        assert name in _lib.SIGNATURES and name + "(" in hdr and hasattr(lib, name), name
    assert "AetherDynDnriPriorParams" in hdr and "AetherDynDnriDecoderParams" in hdr
    cfg = _config()
    i64 = lambda *v: (C.c_int64 * len(v))(*v)
    i32 = lambda *v: (C.c_int * len(v))(*v)
    for n_max, ns in ((9, (7,)), (20, (0, 2, 3, 7, 13, 20)), (20, (20,) * 64), (2, (2,))):
        B = len(ns)
        es = [n * min(10, n - 1) if n else 0 for n in ns]
        deg = [min(10, n - 1) if n else 0 for n in ns]
        got = lib.aether_dyn_dnri_step_batched_workspace_bytes(C.byref(cfg), B, n_max, i64(*ns), i64(*es), i32(*deg))
        aether = lib.aether_dyn_step_batched_workspace_bytes(C.byref(cfg), B, n_max, i64(*ns), i64(*es), i32(*deg))
        assert 0 < got < aether, (n_max, ns)
        roll = lib.aether_dyn_dnri_rollout_batched_workspace_bytes(C.byref(cfg), B, n_max, 1, i64(*ns), i64(*es), i32(*deg))
        assert got < roll < lib.aether_dyn_rollout_batched_workspace_bytes(C.byref(cfg), B, n_max, 1, i64(*ns), i64(*es), i32(*deg))
    # a one-object scene; an edge count that is not the kNN graph's
    assert lib.aether_dyn_dnri_step_batched_workspace_bytes(C.byref(cfg), 2, 9, i64(7, 1), i64(42, 0), i32(6, 0)) == 0
    assert "one present object" in lib.aether_last_error().decode()
    assert lib.aether_dyn_dnri_step_batched_workspace_bytes(C.byref(cfg), 1, 9, i64(7), i64(41), i32(6)) == 0
    assert "n_present * min(knn_k, n_present - 1)" in lib.aether_last_error().decode()
    # the rollout validates every step of every scene before anything is queued: step 1 of 2 holds the one-object scene.  The
    # device pointers are never read (placeholders), the call returns from its host checks.
    codes = _codes()
    fake = C.c_void_p(4096)
    ptrs = (C.c_void_p * 2)(4096, 4096)
    st = lib.aether_dyn_dnri_rollout_batched(fake, fake, C.byref(cfg), 1, 9, 2, fake, fake, fake, i64(7, 1), i64(42, 0), i32(6, 0),
                                             ptrs, ptrs, ptrs, ptrs, ptrs, fake, fake, fake, fake, fake, 1 << 30, None)
    assert st == codes["AETHER_EINVAL"] and "one present object" in lib.aether_last_error().decode()
    st = lib.aether_dyn_dnri_rollout_batched(fake, fake, C.byref(cfg), 1, 9, 2, fake, fake, fake, i64(7, 7), i64(42, 40), i32(6, 6),
                                             ptrs, ptrs, ptrs, ptrs, ptrs, fake, fake, fake, fake, fake, 1 << 30, None)
    assert st == codes["AETHER_EINVAL"] and "n_present * min(knn_k, n_present - 1)" in lib.aether_last_error().decode()
    # staged sizes: bad sizes give 0
    assert lib.aether_dyn_dnri_prior_workspace_bytes(128, 64, 64, 7, 42) > 0
    assert lib.aether_dyn_dnri_prior_workspace_bytes(128, 64, 64, 0, 42) == 0
    assert lib.aether_dyn_dnri_decoder_workspace_bytes(128, 3, 7, 42) > 0
    assert lib.aether_dyn_dnri_decoder_workspace_bytes(128, 5, 7, 42) == 0
    assert lib.aether_dyn_dnri_decoder_workspace_bytes(128, 3, 7, 42) < lib.aether_dyn_decoder_workspace_bytes(128, 7, 42)
    assert lib.aether_dyn_dnri_prior_workspace_bytes(128, 64, 64, 7, 42) < lib.aether_dyn_prior_workspace_bytes(128, 64, 64, 7, 42)


def _codes():
    import re
    header = os.path.join(REPO, "include", "aether_hip.h")
    return {k: int(v) for k, v in re.findall(r"#define (AETHER_E\w+) \((-\d+)\)", open(header).read())}


# -- the restatement against the reference's own outputs ----------------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference_step(tag, one_thread):
    model, _, d = build(tag)
    s = scene(d, tag)
    x0, m0 = s["inputs"][0, 0], s["masks"][0, 0]
    for dtype, ref, bar in ((torch.float64, "ref64", 1e-12), (torch.float32, "ref", 1e-6)):
        m = restatement(model, tag, dtype)
        state0 = tuple(t[0].to(dtype) for t in s["state0"])
        logits, (h, c), _ = m.prior(x0, m0, s["node_inds"][0], s["graph_info"][0], state0)
        pred, hid = m.decoder(x0, s["hidden0"][0], s["step_edges"][0], m0, s["graph_info"][0])
        got = {"logits": logits.unsqueeze(0), "h1": h.unsqueeze(0), "c1": c.unsqueeze(0), "pred": pred.unsqueeze(0),
               "hidden": hid.unsqueeze(0)}
        for name, v in got.items():
            want = torch.from_numpy(d[f"{tag}.{ref}.{name}"])
            assert v.shape == want.shape, name
            assert scale_rel_err(v, want) <= bar, (name, str(dtype))
        # the sample of these logits on the fixture's draw is the fixture's one-hot sample
        assert torch.equal(m.sample(logits, s["uniform"][0]).argmax(-1), s["step_edges"][0].argmax(-1))
        absent = m0 == 0
        assert torch.equal(pred[absent], torch.zeros_like(pred[absent]))


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_predict_future(tag, one_thread):
    """The whole loop through the hard samples: every sampled edge type equals the reference's (the generator accepted the
    noise seed on that condition); fp64 at 1e-12, fp32 at 1e-5 (up to five steps of fp32 rounding)."""
    model, _, d = build(tag)
    s = scene(d, tag)
    for dtype, ref, bar in ((torch.float64, "ref64", 1e-12), (torch.float32, "ref", 1e-5)):
        m = restatement(model, tag, dtype)
        preds, z, _ = m.predict_future(s["inputs"][0], s["masks"][0], s["node_inds"], s["graph_info"], s["burn"][0],
                                       [u.to(dtype) for u in s["uniform"]], return_all=True)
        for t, (a, b) in enumerate(zip(z, s["edges"])):
            assert torch.equal(a.argmax(-1), b.argmax(-1)), (t, str(dtype))
        want = torch.from_numpy(d[f"{tag}.{ref}.predictions"])[0]
        assert scale_rel_err(preds, want) <= bar, str(dtype)
        absent = s["masks"][0, :s["T"] - 1] == 0
        assert torch.equal(preds[absent], torch.zeros_like(preds[absent]))


def test_fixture_margins_and_shapes():
    d = golden()
    assert [str(c) for c in d["cases"]] == list(CASES)
    for tag in CASES:
        Nmax, K, _, T, _, _ = MG.CASES[tag]
        assert float(d[f"{tag}.margin"]) > MG.MARGIN
        assert d[f"{tag}.ref.predictions"].shape == (1, T - 1, Nmax, 4) and d[f"{tag}.ref.predictions"].dtype == np.float32
        assert d[f"{tag}.ref64.predictions"].dtype == np.float64 and np.isfinite(d[f"{tag}.ref64.predictions"]).all()
        for t in range(T):
            n = int(d[f"{tag}.in.masks"][0, t].sum())
            assert n >= 2 and d[f"{tag}.send.{t}"].shape[0] == n * min(10, n - 1)
    # the one-step states of the two cases the update bar is held on were taken where the restatement's own floor is typical
    for tag in MG.UPDATE_CASES:
        assert float(d[f"{tag}.update_floor"]) >= MG.TYPICAL
    # the true kNN case: fewer neighbours than the other present objects, and in-degrees that differ
    n0 = int(d["N14.in.masks"][0, 1].sum())
    assert n0 == 14 and d["N14.e2n.1"].shape == (14, 10)
    assert len(set(np.bincount(d["N14.recv.1"], minlength=14).tolist())) > 1
    assert d["N2.e2n.0"].shape == (2, 1) and d["N3.send.0"].shape[0] == 6
