"""ClofNet (``--model clof | clof_vel | clof_vel_gbf``) on the MI355X: every layer's h and x and the parameter gradients
against the reference's fixtures (tools/make_golden_clof.py) and the fp64 restatement (tests/clof_restatement.py), the
README workload, run-to-run identity, self loops and edgeless nodes, the captured training step and what is refused."""
import pytest
import torch

from aether_amd import _lib
from aether_amd.training import GraphedTrainStep

import clof_restatement as R
from test_clof import CASES, CLASSES, build, inputs, kwargs, load, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_TOL, GRAD_TOL = 1e-5, 5e-5


def dev_inputs(inp):
    return {k: ([t.to(DEV) for t in v] if k == "edges" else v.to(DEV, torch.float32)) for k, v in inp.items()}


def args_of(gi):
    return gi["h"], gi["x"], gi["edges"], gi["vel"], gi["edge_attr"]


def ref64(cfg, m, inp):
    sd = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    v = R.VARIANTS[cfg["model"]]
    fw = R.forward(sd, v, inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"], cfg["L"], cfg["N"], **kwargs(cfg))
    g, _ = R.grads(sd, v, inp["h"], inp["x"], inp["edges"], inp["vel"], inp["edge_attr"], inp["target"], cfg["L"], cfg["N"],
                   **kwargs(cfg))
    return fw, g


def hip_grads(m, gi, N):
    m.zero_grad(set_to_none=True)
    out = m(*args_of(gi), n_nodes=N)
    torch.nn.functional.mse_loss(out, gi["target"]).backward()
    torch.cuda.synchronize()
    return out, {k: p.grad for k, p in m.named_parameters()}


@pytest.fixture(scope="module", params=CASES)
def case(request):
    return (request.param,) + load(request.param)


def test_layers_against_the_fixture_and_the_restatement(case):
    name, d, cfg = case
    m = build(cfg, DEV)
    inp = inputs(d)
    gi = dev_inputs(inp)
    x_before = gi["x"].clone()
    out, hs, xs = m.forward_layers(*args_of(gi), n_nodes=cfg["N"])
    assert torch.equal(gi["x"], x_before)
    (o64, hs64, xs64), _ = ref64(cfg, m, inp)
    L = cfg["L"]
    for l in range(L + 1):
        for tag in ("ref", "ref64"):
            assert rel(hs[l].cpu(), d[f"{tag}.h{l}"]) < FWD_TOL, (tag, "h", l)
            assert rel(xs[l].cpu(), d[f"{tag}.x{l}"]) < FWD_TOL, (tag, "x", l)
        assert rel(hs[l].cpu(), hs64[l]) < FWD_TOL and rel(xs[l].cpu(), xs64[l]) < FWD_TOL, l
    assert rel(out.cpu(), d["ref64.out"]) < FWD_TOL and rel(out.cpu(), o64) < FWD_TOL
    with torch.no_grad():
        plain = m(*args_of(gi), n_nodes=cfg["N"])
    assert torch.equal(plain, out)


def test_gradients_against_the_fixture_and_the_restatement(case):
    name, d, cfg = case
    m = build(cfg, DEV)
    inp = inputs(d)
    gi = dev_inputs(inp)
    _, g = hip_grads(m, gi, cfg["N"])
    _, g64 = ref64(cfg, m, inp)
    dead = set(d["ref.dead"].tolist())
    for k, gv in g.items():
        if k in dead:
            assert gv is None, k                    # as in the reference: no optimizer touches them
            continue
        assert gv is not None, k
        gc = gv.cpu()
        assert rel(gc, g64[k]) < GRAD_TOL, (k, rel(gc, g64[k]))
        if "ref.grad." + k not in d.files:
            # a slim case (width 128, four layers): the fixture holds sum, sum of |.| and max of |.| of every gradient.
            # max|a - b| < GRAD_TOL max|b| bounds each checksum's difference by numel GRAD_TOL max|b|
            for tag in ("ref", "ref64"):
                bound = gc.numel() * GRAD_TOL * float(d[f"{tag}.gmax.{k}"])
                assert abs(float(gc.double().sum()) - float(d[f"{tag}.gsum.{k}"])) <= bound, (tag, k)
                assert abs(float(gc.double().abs().sum()) - float(d[f"{tag}.gabs.{k}"])) <= bound, (tag, k)
                assert abs(float(gc.abs().max()) - float(d[f"{tag}.gmax.{k}"])) < GRAD_TOL * float(d[f"{tag}.gmax.{k}"])
            continue
        assert rel(gc, d["ref.grad." + k]) < GRAD_TOL, (k, rel(gc, d["ref.grad." + k]))
        if "ref64.grad." + k in d.files:
            assert rel(gc, d["ref64.grad." + k]) < GRAD_TOL, k


@pytest.mark.parametrize("model", sorted(CLASSES))
def test_readme_workload_against_the_restatement(model):
    """B 128, N 20, hidden 64, 4 layers, norm_diff (the reference README's clof_vel command, every variant)."""
    cfg = dict(model=model, B=128, N=20, H=64, L=4, norm_diff=True, tanh=False, recurrent=True, coords_weight=1.0,
               seed=77, coord_scale=1.0)
    m = build(cfg, DEV)
    inp = R.runner_batch(128, 20, 78, dtype=torch.float64)
    gi = dev_inputs(inp)
    out, g = hip_grads(m, gi, 20)
    (o64, _, _), g64 = ref64(cfg, m, inp)
    assert rel(out.detach().cpu(), o64) < FWD_TOL
    for k, gv in g.items():
        if g64[k] is None:
            assert gv is None, k
        else:
            assert rel(gv.cpu(), g64[k]) < GRAD_TOL, (k, rel(gv.cpu(), g64[k]))


def test_two_runs_are_bit_identical():
    cfg = dict(model="clof_vel_gbf", B=16, N=20, H=64, L=4, norm_diff=True, tanh=False, recurrent=True,
               coords_weight=1.0, seed=5, coord_scale=1.0)
    m = build(cfg, DEV)
    gi = dev_inputs(R.runner_batch(16, 20, 6))
    o1, g1 = hip_grads(m, gi, 20)
    g1 = {k: (v.clone() if v is not None else None) for k, v in g1.items()}
    o2, g2 = hip_grads(m, gi, 20)
    assert torch.equal(o1, o2)
    for k in g1:
        assert (g1[k] is None and g2[k] is None) or torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("model", sorted(CLASSES))
def test_self_loops_and_nodes_without_edges(model):
    """Self loops (diff = cross = 0) and a node with no edge at all (mean over an empty row: count clamped to 1)."""
    g = torch.Generator().manual_seed(11)
    N = 6
    rows = torch.tensor([0, 0, 1, 1, 2, 3, 3, 4, 2, 1], dtype=torch.int64)
    cols = torch.tensor([1, 0, 1, 2, 2, 4, 0, 3, 4, 3], dtype=torch.int64)       # node 5 has none
    x = torch.randn(N, 3, generator=g, dtype=torch.float64)
    vel = torch.randn(N, 3, generator=g, dtype=torch.float64)
    q = torch.tensor([1., -1., 1., 1., -1., -1.], dtype=torch.float64)
    ea = torch.stack([q[rows] * q[cols], ((x[rows] - x[cols]) ** 2).sum(1)], 1)
    inp = dict(h=vel.norm(dim=1, keepdim=True), x=x, edges=[rows, cols], vel=vel, edge_attr=ea,
               target=x + 0.1 * torch.randn(N, 3, generator=g, dtype=torch.float64))
    # norm_diff off in the layers: sqrt at 0 has an undefined (NaN) gradient in the reference
    cfg = dict(model=model, B=1, N=N, H=64, L=3, norm_diff=False, tanh=False, recurrent=True, coords_weight=1.0,
               seed=12, coord_scale=1.0)
    m = build(cfg, DEV)
    gi = dev_inputs(inp)
    out, gr = hip_grads(m, gi, N)
    (o64, _, _), g64 = ref64(cfg, m, inp)
    assert rel(out.detach().cpu(), o64) < FWD_TOL
    for k, gv in gr.items():
        if g64[k] is None:
            assert gv is None, k
        else:
            assert rel(gv.cpu(), g64[k]) < GRAD_TOL, (k, rel(gv.cpu(), g64[k]))


@pytest.mark.parametrize("model", sorted(CLASSES))
def test_graphed_train_step_replays_eager_steps(model):
    """Each GraphedTrainStep replay (FusedAdamW, weight_decay 1e-2) computes the gradients an eager forward / backward
    computes from the same parameters; the dead parameters keep .grad None and stay as they were."""
    cfg = dict(model=model, B=8, N=20, H=64, L=4, norm_diff=True, tanh=False, recurrent=True, coords_weight=1.0,
               seed=21, coord_scale=1.0)
    batches = [dev_inputs(R.runner_batch(8, 20, 100 + i)) for i in range(3)]
    graphed, eager = build(cfg, DEV), build(cfg, DEV)
    keys = [k for k, _ in graphed.named_parameters()]
    dead = [keys[i] for i in graphed._dead()]
    init = {k: v.detach().clone() for k, v in graphed.named_parameters()}
    b0 = batches[0]
    step = GraphedTrainStep(graphed, [b0["h"], b0["x"], b0["edges"], b0["vel"], b0["edge_attr"], None, 20], b0["target"],
                            lr=1e-3, weight_decay=1e-2)
    for b in batches:
        before = {k: v.detach().clone() for k, v in graphed.state_dict().items()}
        step.step([b["h"], b["x"], b["edges"], b["vel"], b["edge_attr"], None, 20], b["target"])
        torch.cuda.synchronize()
        eager.load_state_dict(before)
        _, ge = hip_grads(eager, b, 20)
        pg = dict(graphed.named_parameters())
        for k in keys:
            if k in dead:
                assert pg[k].grad is None and ge[k] is None, k
            else:
                # the captured step seeds the backward with aether_amd.optim.mse_loss_grad, the eager one through autograd
                assert rel(pg[k].grad.cpu(), ge[k].cpu()) < 1e-6, k
                assert not torch.equal(pg[k].detach(), before[k]), k
    step.check()
    pg = dict(graphed.named_parameters())
    for k in dead:
        assert torch.equal(pg[k].detach(), init[k]), k


@pytest.mark.parametrize("model", sorted(CLASSES))
def test_inputs_that_require_grad_fail_loudly(model):
    cfg = dict(model=model, B=2, N=5, H=64, L=1, norm_diff=True, tanh=False, recurrent=True, coords_weight=1.0,
               seed=3, coord_scale=1.0)
    m = build(cfg, DEV)
    gi = dev_inputs(R.runner_batch(2, 5, 4))
    x = gi["x"].clone().requires_grad_(True)
    with pytest.raises(_lib.AetherHipError):
        m(gi["h"], x, gi["edges"], gi["vel"], gi["edge_attr"], n_nodes=5)
