"""LoCS (``--model locs``), host side: the fixtures of tools/make_golden_locs.py against the fp64 restatement
(tests/locs_restatement.py), the drop-in's state_dict surface and seeded initialisation, checkpoints, what it refuses,
and the mapping of its first-layer weights onto Aether's.  The kernels themselves: tests/test_gpu_locs.py."""
import contextlib
import glob
import io
import os

import numpy as np
import pytest
import torch

from aether_amd import _lib
from aether_amd.nn.state2state.locs import LoCS, _locs_blocks, aether_state_dict

import locs_restatement as R
from oracle import aether_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = sorted(os.path.basename(p)[len("locs_"):-4] for p in glob.glob(os.path.join(GOLDEN, "locs_*.npz")))


def load(case):
    d = np.load(os.path.join(GOLDEN, f"locs_{case}.npz"))
    D, H, B, N, ig, p = (int(v) for v in d["config"])
    return d, dict(D=D, H=H, B=B, N=N, inputgrad=bool(ig), p=p / 1000.0, seed=int(d["seed"]))


def build(cfg, device="cpu"):
    """The drop-in under the case's seed."""
    torch.manual_seed(cfg["seed"])
    with contextlib.redirect_stdout(io.StringIO()):
        return LoCS(2 * cfg["D"], cfg["H"], cfg["p"], cfg["D"], device=device)


def inputs(d, dtype=torch.float64):
    t = lambda k: torch.from_numpy(d["in." + k]).to(dtype)
    return dict(h=t("h"), x=t("x"), vel=t("vel"), charges=t("charges"), edge_attr=t("edge_attr"), target=t("target"),
                edges=[torch.from_numpy(d["in.send"]), torch.from_numpy(d["in.recv"])])


def masks(d, dtype=torch.float64):
    return [torch.from_numpy(d["mask1"]).to(dtype), torch.from_numpy(d["mask2"]).to(dtype)] if "mask1" in d.files else None


def rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


@pytest.fixture(scope="module", params=CASES)
def case(request):
    return (request.param,) + load(request.param)


def test_every_fixture_case_is_there():
    assert len(CASES) == 8, CASES
    cfgs = [load(c)[1] for c in CASES]
    assert {c["D"] for c in cfgs} == {2, 3}
    assert {c["H"] for c in cfgs} == {20, 64, 128}
    assert any(c["inputgrad"] for c in cfgs) and any(c["p"] > 0 for c in cfgs)
    for p in glob.glob(os.path.join(GOLDEN, "locs_*.npz")):
        assert os.path.getsize(p) < 1 << 20, p


def test_state_dict_surface_and_seeded_init(case):
    """Keys, shapes and order as the reference's (40 tensors: Aether's 47 without field_net); the default initialisation
    under the seed is the reference's, bit for bit."""
    name, d, cfg = case
    m = build(cfg)
    sd = m.state_dict()
    assert len(sd) == 40
    assert list(sd.keys()) == list(d["keys"])
    assert [k for k, _ in m.named_parameters()] == list(sd.keys())
    for (k, v), shp in zip(sd.items(), d["shapes"]):
        assert list(v.shape) == [int(s) for s in shp if s], k
        assert float(v.double().sum()) == float(d["sum." + k]), k
        assert float(v.double().abs().sum()) == float(d["abs." + k]), k
        if "param." + k in d.files:
            assert torch.equal(v, torch.from_numpy(d["param." + k])), k
    assert m.params == str(sum(v.numel() for v in sd.values()))


def test_fixtures_match_the_restatement(case):
    """The reference's output, loss and gradients (fp32 and fp64) against the fp64 restatement."""
    name, d, cfg = case
    sd = {k: v.double() for k, v in build(cfg).state_dict().items()}
    i = inputs(d)
    mk = masks(d)
    out = R.forward(sd, i["x"], i["vel"], i["edges"], i["edge_attr"], mk)
    assert rel(d["ref.out"], out) <= 1e-5
    if "ref64.out" in d.files:
        assert rel(d["ref64.out"], out) <= 1e-12
        assert abs(float(d["ref64.loss"]) - float(torch.nn.functional.mse_loss(out, i["target"]))) <= 1e-12
    pg, ig, loss = R.grads(sd, i["x"], i["vel"], i["edges"], i["edge_attr"], i["target"], mk, inputs=cfg["inputgrad"])
    assert abs(float(d["ref.loss"]) - float(loss)) <= 1e-5 * abs(float(loss))
    for k, g in pg.items():
        if "ref.grad." + k in d.files:
            assert rel(d["ref.grad." + k], g) <= 5e-5, k
        assert abs(float(d["ref.gsum." + k]) - float(g.sum())) <= 5e-5 * float(g.abs().sum()) + 1e-12, k
        if "ref64.grad." + k in d.files:
            assert rel(d["ref64.grad." + k], g) <= 1e-10, k
        if "ref64.gsum." + k in d.files:
            assert abs(float(d["ref64.gsum." + k]) - float(g.sum())) <= 1e-10 * float(g.abs().sum()) + 1e-15, k
            assert abs(float(d["ref64.gabs." + k]) - float(g.abs().sum())) <= 1e-10 * float(g.abs().sum()) + 1e-15, k
    if cfg["inputgrad"]:
        for k, g in ig.items():
            assert rel(d["ref.ingrad." + k], g) <= 5e-5, k
            assert rel(d["ref64.ingrad." + k], g) <= 1e-10, k
    if mk is not None:                  # the masks are dropout's: zeros and 1 / (1 - p), both present
        for m_ in mk:
            vals = set(np.unique(m_.numpy()).tolist())
            assert vals == {0.0, float(np.float32(1.0 / (1.0 - cfg["p"])))}, vals


def test_a_reference_checkpoint_loads():
    """A state_dict with the reference's keys (here: the fixture's seeded model) loads, and the drop-in's own loads back."""
    d, cfg = load("D3_H20_B2N5")
    sd = {k[len("param."):]: torch.from_numpy(d[k]) for k in d.files if k.startswith("param.")}
    m = build(dict(cfg, seed=1))
    m.load_state_dict(sd)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    m2 = build(dict(cfg, seed=2))
    m2.load_state_dict(m.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))


@pytest.mark.parametrize("kwargs", [dict(hidden_size=4), dict(hidden_size=6, num_dims=3, input_size=6),
                                    dict(num_dims=4, input_size=8), dict(input_size=6), dict(dropout_prob=1.0),
                                    dict(hidden_size=0), dict(hidden_size=4097)])
def test_unsupported_options_raise(kwargs):
    args = dict(input_size=4, hidden_size=64, dropout_prob=0.0, num_dims=2, device="cpu")
    args.update(kwargs)
    with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
        LoCS(**args)


def test_cpu_tensors_raise():
    with contextlib.redirect_stdout(io.StringIO()):
        m = LoCS(4, 64, 0.0, 2, device="cpu")
    x = torch.zeros(3, 2)
    edges = [torch.tensor([0, 1]), torch.tensor([1, 2])]
    with pytest.raises(_lib.AetherHipError):
        m(None, x, edges, x, torch.zeros(2, 2))
    with pytest.raises(_lib.AetherHipError):
        m.rollout(x, x, edges, torch.ones(3, 1), 2)


@pytest.mark.parametrize("D,H,kw", [(2, 64, 64), (3, 64, 64), (2, 20, 64), (3, 128, 128), (2, 96, 128)])
def test_mapping_places_every_column(D, H, kw):
    """The table of the mapping: every LoCS entry where it says, the force columns (edge: [3D+O, 4D+O) and the canonical
    forces [6D+O, 7D+O); res: [2D, 3D)) and the padding zero."""
    O_ = D * (D - 1) // 2
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        m = LoCS(2 * D, H, 0.0, D, device="cpu")
    sd = m.state_dict()
    a = aether_state_dict(sd, D, kw)
    w, aw = sd["gnn.layer_1.message_fn.0.weight"], a["gnn.layer_1.message_fn.0.weight"]
    assert w.shape == (H, 5 * D + O_ + 2) and aw.shape == (kw, 7 * D + O_ + 2)
    assert torch.equal(aw[:H, :3 * D + O_], w[:, :3 * D + O_])
    assert torch.equal(aw[:H, 4 * D + O_:6 * D + O_], w[:, 3 * D + O_:5 * D + O_])
    assert torch.equal(aw[:H, -2:], w[:, -2:])
    assert not aw[:, 3 * D + O_:4 * D + O_].any() and not aw[:, 6 * D + O_:7 * D + O_].any() and not aw[H:].any()
    r, ar = sd["gnn.layer_1.res.weight"], a["gnn.layer_1.res.weight"]
    assert r.shape == (H, 2 * D) and ar.shape == (kw, 3 * D)
    assert torch.equal(ar[:H, :2 * D], r) and not ar[:, 2 * D:].any() and not ar[H:].any()
    assert (aw != 0).sum() == (w != 0).sum() and (ar != 0).sum() == (r != 0).sum()
    for k, v in sd.items():                           # every other tensor keeps all its entries
        assert float(a[k].double().abs().sum()) == float(v.double().abs().sum()), k
    assert all(not a[k].any() for k in a if k.startswith("field_net."))
    # the blocks of the message layer cover LoCS's columns exactly once
    cols = sorted(c for ss, _ in _locs_blocks("gnn.layer_1.message_fn.0.weight", w.shape, D, H, kw)
                  for c in range(ss[1].start, ss[1].stop))
    assert cols == list(range(w.shape[1]))


@pytest.mark.parametrize("case_name", ["D2_H64_B2N5", "D3_H64_B2N5", "D2_H20_B3N5"])
def test_mapped_aether_with_zero_field_is_locs(case_name):
    """In fp64 on the CPU: the Aether restatement with the mapped weights and a zero field computes the reference LoCS
    output of the fixture -- the argument the HIP path rests on."""
    d, cfg = load(case_name)
    sd = {k: v.double() for k, v in build(cfg).state_dict().items()}
    i = inputs(d)
    a = aether_state_dict(sd, cfg["D"])
    out = O.aether_forward(a, i["x"], i["vel"], i["edges"], i["edge_attr"], i["charges"], field=torch.zeros_like(i["x"]))
    assert rel(out, d["ref64.out"]) <= 1e-12
    # and the built-in field net of the mapped state_dict is the zero field (the rollout's route)
    out2 = O.aether_forward(a, i["x"], i["vel"], i["edges"], i["edge_attr"], i["charges"])
    assert torch.equal(out, out2)


@pytest.mark.parametrize("D,H", [(2, 64), (3, 20), (3, 128), (2, 96)])
def test_engine_images_and_gradient_cut_follow_the_mapping(D, H):
    """The module's own copies into the engine-shaped tensors (index_copy_ / slices) equal aether_state_dict at kernel
    width, and the gradient cut (index_select / slices) takes exactly those entries back."""
    torch.manual_seed(4)
    with contextlib.redirect_stdout(io.StringIO()):
        m = LoCS(2 * D, H, 0.0, D, device="cpu")
    a = aether_state_dict(m.state_dict(), D, m._kw)
    img = m._images(torch.device("cpu"), False)
    assert set(img) >= {"gnn.layer_1.message_fn.0.weight", "gnn.layer_1.res.weight"}
    # every tensor the kernels cannot read as it is (another shape) has an image
    assert set(img) >= {n for n, p in m.named_parameters() if p.shape != a[n].shape}
    for n, t in img.items():
        assert torch.equal(t, a[n]), n
    views = [torch.empty_like(p) for p in m.parameters()]
    m._cut(img, views)
    for (n, p), v in zip(m.named_parameters(), views):
        if n in img:
            assert torch.equal(v, p.detach()), n
