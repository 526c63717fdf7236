"""calculate_loss(is_train=False) of the variable-N models, host side: the fp64 restatement (tests/dyn_loss_restatement.py)
against the reference's fp64 fixture (tools/make_golden_dyn_loss.py) -- which pins that the sequence encoder carries no LSTM
state between frames and never reads reverse_rnn --, the library's masked loss terms on the fixture's own predictions and
logits, the new symbols and size functions, and the refusals that need no device.  Fixtures only: the reference tree is never
read."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO, scale_rel_err

sys.path.insert(0, os.path.join(REPO, "tools"))
sys.path.insert(0, os.path.join(REPO, "oracle"))
import dyn_loss_restatement as RL                                        # noqa: E402
import make_golden_dyn_loss as ML                                        # noqa: E402
from make_golden_dynamicvars import perturb_bn_                          # noqa: E402
from test_dyn_dnri import _codes, _config                                # noqa: E402

MODELS, CASES = ML.MODELS, tuple(ML.CASES)
EVERY = [(kind, tag) for kind in MODELS for tag in CASES]
SCALARS = ("loss", "nll", "kl")
ENTRIES = ("aether_dyn_sequence_logits", "aether_dyn_dnri_sequence_logits", "aether_dyn_loss_rollout", "aether_dyn_dnri_loss_rollout")


def golden():
    return np.load(os.path.join(GOLDEN, "dyn_loss.npz"))


def build(kind, tag, device=None):
    """The drop-in model of a fixture case, constructed as the fixture's reference model was -> (model, fixture)."""
    from aether_amd.nn.dynamicvars.aether_dynamicvars import AetherDynamicVars
    from aether_amd.nn.dynamicvars.dnri_dynamicvars import DNRIDynamicVars
    d = golden()
    torch.manual_seed(int(d["seed"]))
    model = (AetherDynamicVars if kind == "aether" else DNRIDynamicVars)(ML.model_params(kind, tag), device=None).eval()
    with torch.no_grad():
        perturb_bn_(model)
        ML.refill_filters_(model)
    return (model if device is None else model.to(device)), d


def scene(d, kind, tag):
    """-> the case's tensors: inputs [1, T, Nmax, 4], masks [1, T, Nmax], node_inds[t], graph_info[t], uniform[t]."""
    t = lambda k: torch.from_numpy(d[f"{kind}.{tag}.{k}"])
    T = ML.CASES[tag][3]
    masks = t("in.masks")
    return dict(inputs=t("in.inputs"), masks=masks, T=T, node_inds=[masks[0, s].nonzero()[:, -1] for s in range(T)],
                graph_info=[(t(f"send.{s}"), t(f"recv.{s}"), t(f"e2n.{s}")) for s in range(T - 1)],
                uniform=[t(f"uniform.{s}") for s in range(T - 1)])


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


@pytest.mark.parametrize("kind,tag", EVERY)
def test_model_is_the_fixtures(kind, tag):
    """Same keys, shapes and checksums as the reference model the fixture came from (reverse_rnn.* included)."""
    model, d = build(kind, tag)
    sd = model.state_dict()
    assert list(sd) == list(d[f"{kind}.{tag}.keys"])
    assert any(k.startswith("encoder.reverse_rnn.") for k in sd)
    for k, s, a in zip(sd, d[f"{kind}.{tag}.sums"], d[f"{kind}.{tag}.abs"]):
        assert abs(float(sd[k].double().sum()) - s) <= 1e-9 * max(1.0, a), k
        assert abs(float(sd[k].double().abs().sum()) - a) <= 1e-9 * max(1.0, a), k


@pytest.mark.parametrize("kind,tag", EVERY)
def test_fp64_restatement_equals_the_reference(kind, tag):
    """Every tensor and scalar of every setting to 1e-12 scale-relative.  A restatement that carried the LSTM state from frame
    to frame, or that ran reverse_rnn, would miss this bar: the two quirks of the reference's encoder are pinned here."""
    model, d = build(kind, tag)
    s = scene(d, kind, tag)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    m = RL.Model(kind, sd, torch.float64, ML.CASES[tag][2], ML.TAU)
    pre = f"{kind}.{tag}"
    for tf, up in ML.settings(tag):
        sn = ML.setting_name(tf, up)
        got = m.calculate_loss(s["inputs"][0], s["masks"][0], s["graph_info"], s["uniform"], tf, up)
        want = lambda k: torch.from_numpy(d[f"{pre}.{k}"])
        assert scale_rel_err(got["prior"], want("ref64.prior")) <= 1e-12
        assert scale_rel_err(got["posterior"], want("ref64.posterior")) <= 1e-12
        assert scale_rel_err(got["predictions"], want(f"{sn}.ref64.predictions")) <= 1e-12, sn
        assert torch.equal(got["samples"][-1], want(f"{sn}.ref64.edges")), sn
        for q in SCALARS:
            assert rel(got[q], d[f"{pre}.{sn}.ref64.{q}"][0]) <= 1e-12, (sn, q)
    # the state really would matter: carrying it over changes the logits far beyond the bar
    f1 = m.features(s["inputs"][0, 1].double(), s["masks"][0, 1])
    R = m.enc["forward_rnn.weight_hh_l0"].shape[1]
    zero, some = torch.zeros(f1.shape[0], R, dtype=torch.float64), torch.full((f1.shape[0], R), 0.1, dtype=torch.float64)
    h_zero, h_some = RL.DO._lstm_cell(m.enc, "forward_rnn.", f1, zero, zero)[0], RL.DO._lstm_cell(m.enc, "forward_rnn.", f1, some, some)[0]
    assert scale_rel_err(h_some, h_zero) > 1e-3


@pytest.mark.parametrize("kind", MODELS)
def test_reverse_rnn_is_never_read(kind):
    tag = "N9"
    model, d = build(kind, tag)
    s = scene(d, kind, tag)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    a = RL.Model(kind, sd, torch.float64, ML.CASES[tag][2], ML.TAU).calculate_loss(s["inputs"][0], s["masks"][0], s["graph_info"],
                                                                                  s["uniform"])
    g = torch.Generator().manual_seed(1)
    for k in sd:
        if k.startswith("encoder.reverse_rnn."):
            sd[k] = torch.randn(sd[k].shape, generator=g)
    b = RL.Model(kind, sd, torch.float64, ML.CASES[tag][2], ML.TAU).calculate_loss(s["inputs"][0], s["masks"][0], s["graph_info"],
                                                                                  s["uniform"])
    for k in ("prior", "posterior", "predictions", "loss", "nll", "kl"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("kind,tag", EVERY)
def test_masked_loss_terms_of_the_library(kind, tag):
    """SceneLossMixin's NLL / KL / return shapes on the fixture's own fp64 predictions and logits give the fixture's scalars."""
    from aether_amd.nn.dynamicvars._loss import SceneLossMixin
    d = golden()
    s = scene(d, kind, tag)
    terms = type("Terms", (SceneLossMixin,), {})()
    terms._init_loss_config(ML.model_params(kind, tag))
    terms.kl_coef = 1.0
    pre = f"{kind}.{tag}"
    prior, post = (torch.from_numpy(d[f"{pre}.ref64.{k}"])[None] for k in ("prior", "posterior"))
    for tf, up in ML.settings(tag):
        sn = ML.setting_name(tf, up)
        preds = torch.from_numpy(d[f"{pre}.{sn}.ref64.predictions"])[None]
        edges = torch.from_numpy(d[f"{pre}.{sn}.ref64.edges"])[None]
        out = terms._loss_terms(s["inputs"].double(), s["masks"], preds, prior, post, edges, False, True)
        assert len(out) == 5 and out[3] is post and out[4] is preds
        for q, v in zip(SCALARS, out):
            assert rel(v, d[f"{pre}.{sn}.ref64.{q}"][0]) <= 1e-12, (sn, q)
        assert terms._loss_terms(s["inputs"].double(), s["masks"], preds, prior, post, edges, True, False)[3] is edges
        assert len(terms._loss_terms(s["inputs"].double(), s["masks"], preds, prior, post, edges, False, False)) == 3
    # an absent object contributes nothing, whatever its prediction row holds
    masks = s["masks"].clone()
    masks[0, 1:, 0] = 0
    preds2 = preds.clone()
    preds2[0, :, 0] += 5.0
    assert torch.equal(terms.nll(preds, s["inputs"][:, 1:].double(), ((masks[:, :-1] == 1) * (masks[:, 1:] == 1)).float()),
                       terms.nll(preds2, s["inputs"][:, 1:].double(), ((masks[:, :-1] == 1) * (masks[:, 1:] == 1)).float()))


def test_loss_combinations_the_reference_refuses():
    from aether_amd.nn.dynamicvars._loss import SceneLossMixin
    terms = type("Terms", (SceneLossMixin,), {})()
    p, t, m = torch.zeros(1, 2, 3, 4), torch.zeros(1, 2, 3, 4), torch.ones(1, 2, 3)
    lg = torch.zeros(1, 5, 2)
    for flags in ({"nll_loss_type": "gaussian", "prior_variance": 1.0}, {"nll_loss_type": "gaussian", "prior_variance": 1.0,
                  "normalize_nll": True, "normalize_nll_per_var": True}, {"nll_loss_type": "crossent"}, {"nll_loss_type": "poisson"}):
        terms._init_loss_config(flags)
        with pytest.raises(NotImplementedError):
            terms.nll(p, t, m)
    for flags in ({}, {"normalize_kl_per_var": True}):
        terms._init_loss_config(flags)
        with pytest.raises(NotImplementedError):
            terms.kl_categorical_learned(torch.softmax(lg, -1), lg)
    # crossent and Poisson as written (:350-362): elementwise loss, masked sum over the mask's sum
    g = torch.Generator().manual_seed(3)
    p, t = torch.randn(1, 2, 3, 4, generator=g), torch.rand(1, 2, 3, 4, generator=g)
    m[0, 1, 2] = 0
    for name, fn in (("crossent", torch.nn.BCEWithLogitsLoss(reduction="none")), ("poisson", torch.nn.PoissonNLLLoss(reduction="none"))):
        terms._init_loss_config({"nll_loss_type": name, "normalize_nll": True})
        want = (fn(p, t) * m.unsqueeze(-1)).view(1, -1).sum(-1) / m.view(1, -1).sum(1)
        assert torch.equal(terms.nll(p, t, m), want)


def test_python_side_refusals_need_no_device():
    from aether_amd import _lib
    for kind in MODELS:
        model, d = build(kind, "N3")
        s = scene(d, kind, "N3")
        args = (s["inputs"], s["masks"], [s["node_inds"]], [s["graph_info"]])
        with pytest.raises(_lib.AetherHipError, match="is_train=True"):
            model.calculate_loss(*args, is_train=True)
        with pytest.raises(_lib.AetherHipError, match="normalized_inputs"):
            model.calculate_loss(*args, normalized_inputs=[s["inputs"]])
        with pytest.raises(ValueError, match="Batching during forward not currently supported"):
            model.calculate_loss(s["inputs"].repeat(2, 1, 1, 1), s["masks"].repeat(2, 1, 1), [s["node_inds"]] * 2,
                                 [s["graph_info"]] * 2)
        with pytest.raises(_lib.AetherHipError, match="no CPU fallback"):
            model.calculate_loss(*args)
        with pytest.raises(_lib.AetherHipError, match="no CPU fallback"):
            model.encoder(s["inputs"][:, :-1], s["masks"][:, :-1], [s["node_inds"]], [s["graph_info"]])


def test_library_declares_the_entries():
    from aether_amd import _lib
    hdr = open(os.path.join(REPO, "include", "aether_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        for n in (name, name + "_workspace_bytes"):
            assert n in _lib.SIGNATURES and n + "(" in hdr and hasattr(lib, n), n
    assert "AetherDynPosteriorParams" in _lib.STRUCTS


def _sizes(n_max, ns, k=10):
    i64 = lambda v: (C.c_int64 * len(v))(*v)
    e = [n * min(k, n - 1, n_max - 1) for n in ns]
    return i64(ns), i64(e), (C.c_int * len(ns))(*[max(1, min(k, n - 1)) for n in ns])


def test_workspace_size_functions():
    """0 (+ aether_last_error) on bad sizes; positive and monotone in the frames, the objects and the posterior's width."""
    from aether_amd import _lib
    lib = _lib.load()
    cfg = _config()
    err = lambda: lib.aether_last_error().decode()
    edges = "dyn_step: n_edges must be n_present * min(knn_k, n_present - 1), the size of the encoder's own kNN graph"
    for kind in ("", "dnri_"):
        seq = getattr(lib, f"aether_dyn_{kind}sequence_logits_workspace_bytes")
        loss = getattr(lib, f"aether_dyn_{kind}loss_rollout_workspace_bytes")
        last_seq = last_loss = 0
        for n_max, ns in ((2, (2,)), (9, (7, 7)), (9, (7, 8, 9)), (20, (13, 20, 20)), (20, (20,) * 5), (20, (20,) * 49), (20, (20,) * 256)):
            n, e, deg = _sizes(n_max, ns)
            a = seq(C.byref(cfg), 3, 64, len(ns), n_max, n, e)
            b = loss(C.byref(cfg), n_max, len(ns), n, e, deg)
            assert a > last_seq and b >= last_loss and b > 0, (kind, n_max, ns)
            assert seq(C.byref(cfg), 3, 128, len(ns), n_max, n, e) > a > seq(C.byref(cfg), 1, 0, len(ns), n_max, n, e)
            last_seq, last_loss = a, b
        n, e, deg = _sizes(9, (7, 7))
        assert seq(C.byref(cfg), 3, 64, 257, 9, *_sizes(9, (7,) * 257)[:2]) == 0 and "1..256 frames" in err()
        assert seq(C.byref(cfg), 3, 64, 0, 9, n, e) == 0
        assert seq(C.byref(cfg), 0, 64, 2, 9, n, e) == 0 and seq(C.byref(cfg), 3, 24, 2, 9, n, e) == 0
        assert "encoder_fc_out" in err()
        assert seq(None, 3, 64, 2, 9, n, e) == 0 and seq(C.byref(cfg), 3, 64, 2, 9, None, e) == 0
        assert loss(C.byref(cfg), 9, 0, n, e, deg) == 0 and loss(C.byref(cfg), 9, 2, n, e, None) == 0
        e[1] = 41
        assert seq(C.byref(cfg), 3, 64, 2, 9, n, e) == 0 and err() == edges
        assert loss(C.byref(cfg), 9, 2, n, e, deg) == 0 and err() == edges
        for few in (1, 0):
            n, e, deg = _sizes(9, (7, 7))
            n[1], e[1] = few, 0
            assert seq(C.byref(cfg), 3, 64, 2, 9, n, e) == 0 and "a frame with fewer than two present objects" in err()
            assert loss(C.byref(cfg), 9, 2, n, e, deg) == 0 and "a frame with fewer than two present objects" in err()


def test_entries_refuse_on_the_host_before_touching_a_pointer():
    from aether_amd import _lib
    lib = _lib.load()
    cfg = _config()
    einval = _codes()["AETHER_EINVAL"]
    err = lambda: lib.aether_last_error().decode()
    fake = C.c_void_p(4096)
    ptrs = (C.c_void_p * 2)(4096, 4096)
    for kind, seq_head, loss_head in (("", (fake, fake), (fake, fake)), ("dnri_", (fake,), (fake,))):
        seq = getattr(lib, f"aether_dyn_{kind}sequence_logits")
        loss = getattr(lib, f"aether_dyn_{kind}loss_rollout")
        post = _lib.STRUCTS["AetherDynPosteriorParams"]()
        for l in range(3):
            post.w[l] = post.b[l] = 4096
        n, e, deg = _sizes(9, (7, 7))
        seq_tail = (fake, fake, fake, fake, fake, 1 << 30, None)
        loss_tail = (ptrs, ptrs, ptrs, fake, ptrs, fake, fake, fake, 1 << 30, None)
        for bad_n, bad_e, text in (((7, 1), (42, 0), "a frame with fewer than two present objects"), ((7, 7), (42, 40), "n_edges must be")):
            n2, e2 = (C.c_int64 * 2)(*bad_n), (C.c_int64 * 2)(*bad_e)
            assert seq(*seq_head, C.byref(post), C.byref(cfg), 3, 64, 2, 9, n2, e2, *seq_tail) == einval and text in err()
            assert loss(*loss_head, C.byref(cfg), 9, 2, -1, fake, fake, n2, e2, deg, *loss_tail) == einval and text in err()
        assert seq(*seq_head, None, C.byref(cfg), 3, 64, 2, 9, n, e, *seq_tail) == einval and err().endswith("sequence_logits: null pointer")
        assert seq(*seq_head, C.byref(post), C.byref(cfg), 4, 64, 2, 9, n, e, *seq_tail) == einval and "null encoder_fc_out weight" in err()
        assert loss(*loss_head, C.byref(cfg), 9, 2, -2, fake, fake, n, e, deg, *loss_tail) == einval and "teacher_forcing_steps" in err()
        nulls = (C.c_void_p * 2)(4096, 0)
        assert loss(*loss_head, C.byref(cfg), 9, 2, -1, fake, fake, n, e, deg, ptrs, ptrs, ptrs, fake, nulls, fake, fake, fake, 1 << 30,
                    None) == einval and "pointer is null" in err()
        assert loss(*loss_head, C.byref(cfg), 9, 2, -1, fake, fake, n, e, deg, *loss_tail[:-3], fake, 16, None) == _codes()["AETHER_ESPACE"]
