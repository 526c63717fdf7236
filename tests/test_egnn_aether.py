"""EGNN-Aether (``--model egnn_aether``), host side: the fixtures of tools/make_golden_egnn_aether.py against the fp64
restatement (tests/egnn_restatement.py), the drop-in's state_dict surface and seeded initialisation, what it refuses,
and the C ABI's host-only functions.  The kernels themselves: tests/test_gpu_egnn_aether.py."""
import contextlib
import glob
import io
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from aether_amd import _lib
from aether_amd.nn.state2state.egnn_aether import EGNN_vel_Aether

from egnn_restatement import forward as ref_forward, grads as ref_grads

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("egnn_aether_"):-4] for p in glob.glob(os.path.join(GOLDEN, "egnn_aether_*.npz")))


def load(case):
    d = np.load(os.path.join(GOLDEN, f"egnn_aether_{case}.npz"))
    B, N, H, L, norm, tanh = (int(v) for v in d["config"])
    cfg = dict(B=B, N=N, H=H, L=L, norm_diff=bool(norm), tanh=bool(tanh), seed=int(d["seed"]),
               phi_scale=float(d["phi_scale"]), in_nf=int(d["in_node_nf"]) if "in_node_nf" in d.files else 1,
               graph=str(d["graph"]) if "graph" in d.files else "runner")
    return d, cfg


def build(cfg, device="cpu"):
    """The drop-in under the case's seed (+ the clamp case's scaled phi weight)."""
    torch.manual_seed(cfg["seed"])
    with contextlib.redirect_stdout(io.StringIO()):
        m = EGNN_vel_Aether(in_node_nf=cfg.get("in_nf", 1), in_edge_nf=8, hidden_nf=cfg["H"], num_dims=3, device=device,
                            n_layers=cfg["L"], recurrent=True, norm_diff=cfg["norm_diff"], tanh=cfg["tanh"])
    if cfg["phi_scale"] != 1.0:
        with torch.no_grad():
            for l in range(cfg["L"]):
                getattr(m, f"gcl_{l}").coord_mlp[2].weight.mul_(cfg["phi_scale"])
    return m


def inputs(d, dtype=torch.float64):
    t = lambda k: torch.from_numpy(d["in." + k]).to(dtype)
    edges = [torch.from_numpy(d["in.row"]), torch.from_numpy(d["in.col"])]
    return dict(h=t("h"), x=t("x"), edges=edges, vel=t("vel"), edge_attr=t("edge_attr"), charges=t("charges"),
                target=t("target"))


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


@pytest.fixture(scope="module", params=CASES)
def case(request):
    return (request.param,) + load(request.param)


def test_every_fixture_case_is_there():
    assert len(CASES) == 12, CASES
    cfgs = [load(c)[1] for c in CASES]
    assert {(c["B"], c["N"]) for c in cfgs} == {(2, 5), (1, 2), (2, 6)}
    assert {c["H"] for c in cfgs} == {64, 128} and {c["L"] for c in cfgs} == {1, 2, 4}
    # width 128 at depth, the clamp at depth, a wider h, a multigraph, no edges
    assert (128, 4) in {(c["H"], c["L"]) for c in cfgs}
    assert {c["L"] for c in cfgs if c["phi_scale"] != 1.0} == {1, 4}
    assert {c["in_nf"] for c in cfgs} == {1, 3} and {c["graph"] for c in cfgs} == {"runner", "multi", "empty"}
    for c in CASES:
        d, cfg = load(c)
        row, col = d["in.row"], d["in.col"]
        assert row.size != 3, c
        assert d["in.h"].shape == (cfg["B"] * cfg["N"], cfg["in_nf"]), c
        if cfg["phi_scale"] != 1.0:
            assert 0 < int(d["n_clamped"]) < 3 * row.size, c
        if cfg["graph"] == "empty":
            assert row.size == 0 and d["in.edge_attr"].shape == (0, 2), c
        if cfg["graph"] == "multi":
            assert not cfg["norm_diff"] and (row == col).sum() == 1, c                       # a self loop
            assert np.unique(np.stack([row, col]), axis=1).shape[1] < row.size, c            # duplicate edges
            touched = set(row.tolist()) | set(col.tolist())
            assert len(touched) < cfg["B"] * cfg["N"], c                                     # a node without edges
            assert not np.array_equal(row, np.sort(row)), c                                  # rows in random order
    assert {c["norm_diff"] for c in cfgs} == {True, False} and {c["tanh"] for c in cfgs} == {True, False}
    assert any(int(load(c)[0]["n_clamped"]) > 0 for c in CASES if "n_clamped" in load(c)[0].files)
    for p in glob.glob(os.path.join(GOLDEN, "egnn_aether_*.npz")):
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
            assert torch.equal(v, torch.from_numpy(d["param." + k])), k
            assert tuple(v.shape) == d["param." + k].shape


def test_load_state_dict_of_a_reference_checkpoint():
    d, cfg = load("B2N5_H64_L1_clamp")
    sd = {k: torch.from_numpy(d["param." + k]) for k in d["keys"]}
    with contextlib.redirect_stdout(io.StringIO()):
        m = EGNN_vel_Aether(1, 8, 64, 3, n_layers=1, recurrent=True)
    m.load_state_dict(sd)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_fixture_against_the_fp64_restatement(case):
    """Reference fp64 == restatement fp64 (same equations, independent code); reference fp32 within fp32 rounding."""
    name, d, cfg = case
    sd = {k: v.double() for k, v in build(cfg).state_dict().items()}
    inp = inputs(d)
    x_before = inp["x"].clone()
    out, hs, xs = ref_forward(sd, inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"], inp["charges"],
                              cfg["L"], cfg["norm_diff"], cfg["tanh"])
    assert torch.equal(inp["x"], x_before)
    assert rel(out, d["ref64.out"]) < 1e-12
    for l in range(cfg["L"] + 1):
        assert rel(hs[l], d[f"ref64.h{l}"]) < 1e-12, l
        assert rel(xs[l], d[f"ref64.x{l}"]) < 1e-12, l
        assert rel(hs[l], d[f"ref.h{l}"]) < 1e-5, l
        assert rel(xs[l], d[f"ref.x{l}"]) < 1e-5, l
    g, loss = ref_grads(sd, inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"], inp["charges"], inp["target"],
                        cfg["L"], cfg["norm_diff"], cfg["tanh"])
    assert abs(float(loss) - float(d["ref64.loss"])) <= 1e-12 * abs(float(loss))
    for k, gk in g.items():
        if "ref64.grad." + k in d.files:
            assert rel(gk, d["ref64.grad." + k]) < 1e-10, k
        s, a = float(d["ref64.gsum." + k]), float(d["ref64.gabs." + k])
        assert abs(float(gk.sum()) - s) <= 1e-10 * max(a, 1e-300), k
        assert abs(float(gk.abs().sum()) - a) <= 1e-10 * max(a, 1e-300), k
        if a > 0 and "ref.grad." + k in d.files:
            assert rel(gk, d["ref.grad." + k]) < 2e-4, k
        elif a > 0:                # the slim case: the fp32 reference by its checksum, the fp64 one by its maximum too
            assert abs(float(gk.abs().max()) - float(d["ref64.gmax." + k])) <= 1e-10 * float(d["ref64.gmax." + k]), k
            assert abs(float(gk.abs().sum()) - float(d["ref.gabs." + k])) <= 2e-4 * a, k


def test_clamp_case_has_zero_gradient_where_the_clamp_is_active():
    """In the clamp case the restatement's phi gradient differs from the unclamped one: the clamp's zero gradient is
    part of what the fixture pins."""
    d, cfg = load("B2N5_H64_L1_clamp")
    assert int(d["n_clamped"]) > 0
    sd = {k: v.double() for k, v in build(cfg).state_dict().items()}
    inp = inputs(d)
    g, _ = ref_grads(sd, inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"], inp["charges"], inp["target"],
                     1, False, False)
    assert rel(g["gcl_0.coord_mlp.2.weight"], d["ref.grad.gcl_0.coord_mlp.2.weight"]) < 2e-4


@pytest.mark.parametrize("kw", [dict(num_dims=2), dict(hidden_nf=96), dict(hidden_nf=32), dict(n_layers=0),
                                dict(recurrent=False), dict(coords_weight=2.0), dict(in_edge_nf=2), dict(act_fn=nn.ReLU()),
                                dict(in_node_nf=0)])
def test_ctor_rejects_unsupported(kw):
    args = dict(in_node_nf=1, in_edge_nf=8, hidden_nf=64, num_dims=3, n_layers=4, recurrent=True)
    args.update(kw)
    with pytest.raises(ValueError):
        with contextlib.redirect_stdout(io.StringIO()):
            EGNN_vel_Aether(**args)


def test_supported_options_construct():
    with contextlib.redirect_stdout(io.StringIO()):
        for H in (64, 128):
            for L in (1, 2, 4, 7):
                EGNN_vel_Aether(1, 8, H, 3, n_layers=L, recurrent=True, norm_diff=True, tanh=True)


def test_cpu_tensor_fails_loudly():
    d, cfg = load("B1N2_H64_L1_norm")
    m = build(cfg)
    inp = inputs(d, torch.float32)
    with pytest.raises(_lib.AetherHipError):
        m(inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"], inp["charges"])
    with pytest.raises(_lib.AetherHipError):
        with torch.no_grad():
            m(inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"], inp["charges"])


@pytest.mark.parametrize("H,L", [(64, 1), (64, 4), (128, 3)])
def test_gradient_layout_matches_the_library(H, L):
    """aether_egnn_backward's flat buffer: every parameter at the next multiple of 4 floats, named_parameters() order."""
    with contextlib.redirect_stdout(io.StringIO()):
        m = EGNN_vel_Aether(1, 8, H, 3, n_layers=L, recurrent=True)
    want = sum((p.numel() + 3) // 4 * 4 for p in m.parameters())
    assert _lib.load().aether_egnn_grad_floats(H, L, 1) == want
    assert _lib.load().aether_egnn_grad_floats(96, L, 1) < 0


def test_workspace_functions_are_host_only_arithmetic():
    lib = _lib.load()
    small = lib.aether_egnn_workspace_bytes(64, 4, 1, 2560, 48640, 0)
    keep = lib.aether_egnn_workspace_bytes(64, 4, 1, 2560, 48640, 1)
    assert 0 < small < keep
    assert keep > 48640 * (2 * 64 + 9) * 4          # the backward keeps every edge's input row
    assert lib.aether_egnn_workspace_bytes(96, 4, 1, 10, 10, 0) == 0
    assert lib.aether_egnn_workspace_bytes(64, 0, 1, 10, 10, 0) == 0
    offs = [lib.aether_egnn_workspace_offset(b"h", l, 64, 4, 1, 10, 90) for l in range(5)]
    assert all(b - a == 10 * 64 * 4 for a, b in zip(offs, offs[1:]))
    assert lib.aether_egnn_workspace_offset(b"x", 5, 64, 4, 1, 10, 90) < 0
    assert lib.aether_egnn_workspace_offset(b"nope", 0, 64, 4, 1, 10, 90) < 0
    assert lib.aether_egnn_workspace_offset(b"field", 0, 64, 4, 1, 10, 90) >= 0
