"""ClofNet (``--model clof | clof_vel | clof_vel_gbf``), host side: the fixtures of tools/make_golden_clof.py against the
fp64 restatement (tests/clof_restatement.py), the drop-ins' state_dict surface and seeded initialisation, loading a
reference checkpoint, what they refuse, and the C ABI's host-only functions.  The kernels: tests/test_gpu_clof.py."""
import contextlib
import glob
import io
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from aether_amd import _lib
from aether_amd.nn.state2state import clof as M

import clof_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "clof_*.npz")))
CLASSES = {"clof": M.ClofNet, "clof_vel": M.ClofNet_vel, "clof_vel_gbf": M.ClofNet_vel_gbf}


def load(case):
    d = np.load(os.path.join(GOLDEN, f"{case}.npz"))
    B, N, H, L, norm, tanh, rec = (int(v) for v in d["config"])
    cfg = dict(model=str(d["variant"]), B=B, N=N, H=H, L=L, norm_diff=bool(norm), tanh=bool(tanh), recurrent=bool(rec),
               coords_weight=float(d["coords_weight"]), seed=int(d["seed"]), coord_scale=float(d["coord_scale"]),
               in_nf=int(d["in_node_nf"]) if "in_node_nf" in d.files else 1,
               graph=str(d["graph"]) if "graph" in d.files else "runner")
    return d, cfg


def build(cfg, device="cpu"):
    """The drop-in under the case's seed (+ the clamp case's scaled coord_mlp.2 weight)."""
    torch.manual_seed(cfg["seed"])
    with contextlib.redirect_stdout(io.StringIO()):
        m = CLASSES[cfg["model"]](in_node_nf=cfg.get("in_nf", 1), in_edge_nf=2, hidden_nf=cfg["H"], device=device,
                                  n_layers=cfg["L"],
                                  coords_weight=cfg["coords_weight"], recurrent=cfg["recurrent"],
                                  norm_diff=cfg["norm_diff"], tanh=cfg["tanh"])
    if cfg["coord_scale"] != 1.0:
        with torch.no_grad():
            for l in range(cfg["L"]):
                getattr(m, f"gcl_{l}").coord_mlp[2].weight.mul_(cfg["coord_scale"])
    return m


def inputs(d, dtype=torch.float64):
    t = lambda k: torch.from_numpy(d["in." + k]).to(dtype)
    edges = [torch.from_numpy(d["in.row"]), torch.from_numpy(d["in.col"])]
    return dict(h=t("h"), x=t("x"), edges=edges, vel=t("vel"), edge_attr=t("edge_attr"), target=t("target"))


def kwargs(cfg):
    return dict(norm_diff=cfg["norm_diff"], tanh=cfg["tanh"], recurrent=cfg["recurrent"],
                coords_weight=cfg["coords_weight"])


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


@pytest.fixture(scope="module", params=CASES)
def case(request):
    return (request.param,) + load(request.param)


def test_every_fixture_case_is_there():
    cfgs = [load(c)[1] for c in CASES]
    assert len(cfgs) == 17, CASES
    assert {c["model"] for c in cfgs} == set(CLASSES)
    assert {(c["model"], c["B"], c["N"], c["H"], c["L"]) for c in cfgs} >= {
        (k, 2, 5, 64, 4) for k in CLASSES}
    assert (1, 2) in {(c["B"], c["N"]) for c in cfgs} and 128 in {c["H"] for c in cfgs}
    assert {c["norm_diff"] for c in cfgs} == {True, False} and {c["tanh"] for c in cfgs} == {True, False}
    assert {c["recurrent"] for c in cfgs} == {True, False}
    assert any(int(load(c)[0]["n_clamped"]) > 0 for c in CASES if "n_clamped" in load(c)[0].files)
    # width 128 at depth (every variant), the options together at depth, a wider h, a multigraph, no edges
    assert {(c["model"], c["B"], c["N"], c["H"], c["L"]) for c in cfgs} >= {(k, 2, 5, 128, 4) for k in CLASSES}
    assert any(c["L"] == 4 and not c["recurrent"] and c["coords_weight"] == 0.5 and c["tanh"] for c in cfgs)
    assert {c["in_nf"] for c in cfgs} == {1, 3} and {c["graph"] for c in cfgs} == {"runner", "multi", "empty"}
    for c in CASES:
        d, cfg = load(c)
        row, col = d["in.row"], d["in.col"]
        assert row.size != 3, c
        assert d["in.h"].shape == (cfg["B"] * cfg["N"], cfg["in_nf"]), c
        if cfg["graph"] == "empty":
            assert row.size == 0 and d["in.edge_attr"].shape == (0, 2), c
        if cfg["graph"] == "multi":
            assert not cfg["norm_diff"] and (row == col).sum() == 1, c                       # a self loop
            assert np.unique(np.stack([row, col]), axis=1).shape[1] < row.size, c            # duplicate edges
            touched = set(row.tolist()) | set(col.tolist())
            assert len(touched) < cfg["B"] * cfg["N"], c                                     # a node without edges
            assert not np.array_equal(row, np.sort(row)), c                                  # rows in random order
    for p in glob.glob(os.path.join(GOLDEN, "clof_*.npz")):
        assert os.path.getsize(p) < 1 << 20, p


def test_state_dict_surface_and_seeded_init(case):
    """Keys, shapes and order as the reference's; the default initialisation under the seed is the reference's, bit for
    bit (fp64 sums of identical fp32 tensors; whole tensors where the fixture holds them)."""
    name, d, cfg = case
    m = build(cfg)
    sd = m.state_dict()
    assert list(sd.keys()) == list(d["keys"])
    assert [k for k, _ in m.named_parameters()] == list(sd.keys())
    for k, v in sd.items():
        assert float(v.double().sum()) == float(d["sum." + k]), k
        assert float(v.double().abs().sum()) == float(d["abs." + k]), k
        if "param." + k in d.files:
            assert np.array_equal(v.numpy(), d["param." + k]), k


def test_dead_parameters_match_the_reference(case):
    name, d, cfg = case
    m = build(cfg)
    keys = [k for k, _ in m.named_parameters()]
    assert sorted(keys[i] for i in m._dead()) == sorted(d["ref.dead"].tolist())
    assert len(d["ref.dead"]) == (8 if cfg["model"] == "clof" else 6)


def test_restatement_matches_the_reference_forward(case):
    """fp64 restatement from the fixture's parameters against the reference's fp64 (tight) and fp32 runs, every layer."""
    name, d, cfg = case
    sd = {k: v.double() for k, v in build(cfg).state_dict().items()}
    inp = inputs(d)
    v = R.VARIANTS[cfg["model"]]
    out, hs, xs = R.forward(sd, v, inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"], cfg["L"], cfg["N"],
                            **kwargs(cfg))
    assert rel(out, d["ref64.out"]) < 1e-9
    for l in range(cfg["L"] + 1):
        assert rel(hs[l], d[f"ref64.h{l}"]) < 1e-9, l
        assert rel(xs[l], d[f"ref64.x{l}"]) < 1e-9, l
        assert rel(hs[l], d[f"ref.h{l}"]) < 1e-4, l
        assert rel(xs[l], d[f"ref.x{l}"]) < 1e-4, l


def test_restatement_matches_the_reference_gradients(case):
    name, d, cfg = case
    sd = {k: v.double() for k, v in build(cfg).state_dict().items()}
    inp = inputs(d)
    g, loss = R.grads(sd, R.VARIANTS[cfg["model"]], inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"],
                      inp["target"], cfg["L"], cfg["N"], **kwargs(cfg))
    assert abs(float(loss) - float(d["ref64.loss"])) <= 1e-9 * abs(float(d["ref64.loss"]))
    dead = set(d["ref64.dead"].tolist())
    for k, gv in g.items():
        if k in dead:
            assert gv is None, k
            continue
        s = float(d["ref64.gabs." + k])
        # the reference evaluates the Gaussian layer in fp32 at any model dtype: its gradients carry fp32 rounding
        tol = 1e-5 if k.startswith("gbf.") else 1e-8
        assert abs(float(gv.sum()) - float(d["ref64.gsum." + k])) <= tol * max(s, 1e-30), k
        if "ref64.grad." + k in d.files:
            assert rel(gv, d["ref64.grad." + k]) < tol, k
        if "ref.grad." + k in d.files:
            assert rel(gv, d["ref.grad." + k]) < 1e-3 or float(gv.abs().max()) < 1e-12, k
        else:                      # a slim case: the fp32 reference by its checksums, the fp64 one by all three
            assert abs(float(gv.abs().sum()) - s) <= tol * max(s, 1e-30), k
            assert abs(float(gv.abs().max()) - float(d["ref64.gmax." + k])) <= tol * float(d["ref64.gmax." + k]), k
            assert abs(float(gv.abs().sum()) - float(d["ref.gabs." + k])) <= 1e-3 * max(s, 1e-30), k


def test_reference_checkpoint_loads_both_ways(case):
    """A reference state_dict loads into the drop-in and back (strict), tensors equal."""
    name, d, cfg = case
    m = build(cfg)
    torch.manual_seed(cfg["seed"] + 99)
    other = build(dict(cfg, seed=cfg["seed"] + 99))
    m.load_state_dict(other.state_dict())
    for (k, a), (_, b) in zip(m.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k
    if "param." + list(d["keys"])[0] in d.files:
        ref_sd = {k: torch.from_numpy(d["param." + k]) for k in d["keys"]}
        m.load_state_dict(ref_sd)
        for k, v in m.state_dict().items():
            assert torch.equal(v, ref_sd[k]), k


@pytest.mark.parametrize("model", sorted(CLASSES))
def test_constructor_rejections(model):
    cls = CLASSES[model]
    ok = dict(in_node_nf=1, in_edge_nf=2, hidden_nf=64)
    with contextlib.redirect_stdout(io.StringIO()):
        cls(**ok)
        for bad in (dict(hidden_nf=32), dict(hidden_nf=96), dict(n_layers=0), dict(in_edge_nf=3),
                    dict(act_fn=nn.ReLU()), dict(in_node_nf=0)):
            with pytest.raises(ValueError):
                cls(**{**ok, **bad})


@pytest.mark.parametrize("model", sorted(CLASSES))
def test_forward_rejections_on_cpu(model):
    """node_attr, a node count that is not a multiple of n_nodes (ValueError), then a CPU tensor (AetherHipError)."""
    with contextlib.redirect_stdout(io.StringIO()):
        m = CLASSES[model](in_node_nf=1, in_edge_nf=2, hidden_nf=64, n_layers=1)
    inp = R.runner_batch(2, 5, 3)
    args = (inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"])
    with pytest.raises(ValueError):
        m(*args, node_attr=torch.ones(10, 1), n_nodes=5)
    with pytest.raises(ValueError):
        m(*args, n_nodes=3)
    with pytest.raises(_lib.AetherHipError):
        m(*args, n_nodes=5)


@pytest.mark.parametrize("model", sorted(CLASSES))
@pytest.mark.parametrize("H,L", [(64, 1), (64, 4), (128, 3)])
def test_gradient_layout_matches_the_library(model, H, L):
    """The flat gradient buffer of _grad_buffers (named_parameters order, 4-float padding) is the library's layout."""
    with contextlib.redirect_stdout(io.StringIO()):
        m = CLASSES[model](in_node_nf=1, in_edge_nf=2, hidden_nf=H, n_layers=L)
    off = sum((p.numel() + 3) // 4 * 4 for p in m.parameters())
    lib = _lib.load()
    assert lib.aether_clof_grad_floats(m._variant, H, L, 1) == off
    assert len(list(m.parameters())) == {"clof": 8, "clof_vel": 6, "clof_vel_gbf": 10}[model] + 19 * L
    assert lib.aether_clof_grad_floats(m._variant, 96, L, 1) < 0
    assert lib.aether_clof_workspace_bytes(m._variant, H, L, 1, 40, 360, 1) > \
        lib.aether_clof_workspace_bytes(m._variant, H, L, 1, 40, 360, 0) > 0
