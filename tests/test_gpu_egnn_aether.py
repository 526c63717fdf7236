"""EGNN-Aether (``--model egnn_aether``) on the MI355X: aether_egnn_forward / aether_egnn_backward through the drop-in,
against the reference's fp32 run and the fp64 restatement (tests/egnn_restatement.py)."""
import pytest
import torch

from aether_amd import _lib
from aether_amd.optim import FusedAdamW, mse_loss_grad
from aether_amd.training import GraphedTrainStep

from conftest import scale_rel_err
from egnn_restatement import forward as ref_forward, grads as ref_grads, runner_batch
from test_egnn_aether import CASES, build, inputs, load

pytestmark = pytest.mark.gpu
TOL = 1e-5       # forward: the project's bar, max|a - b| / max|b|
GTOL = 5e-5      # gradients: as tests/test_gpu_backward.py


def _dev(inp):
    return {k: ([e.cuda() for e in v] if k == "edges" else v.to(device="cuda", dtype=torch.float32)) for k, v in inp.items()}


def _args(g):
    return (g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"], g["charges"])


def _grads(m, g):
    m.zero_grad(set_to_none=True)
    out = m(*_args(g))
    loss = torch.nn.functional.mse_loss(out, g["target"])
    loss.backward()
    torch.cuda.synchronize()
    return out.detach(), float(loss), {k: p.grad.detach().cpu() for k, p in m.named_parameters()}


def _model(cfg):
    return build(cfg, "cuda")


@pytest.mark.parametrize("case", CASES)
def test_forward_every_layer_matches_reference(case):
    d, cfg = load(case)
    m = _model(cfg)
    g = _dev(inputs(d))
    x_before = g["x"].clone()
    out, hs, xs = m.forward_layers(*_args(g))
    with torch.no_grad():
        out2 = m(*_args(g))
    torch.cuda.synchronize()
    assert torch.equal(g["x"], x_before)                        # the caller's x is not written
    assert torch.equal(out, out2)
    sd64 = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    i64 = inputs(d)
    _, rhs, rxs = ref_forward(sd64, i64["h"], i64["x"], i64["edges"], i64["vel"], i64["edge_attr"], i64["charges"],
                              cfg["L"], cfg["norm_diff"], cfg["tanh"])
    for l in range(cfg["L"] + 1):
        for got, key, r64 in ((hs[l], f"h{l}", rhs[l]), (xs[l], f"x{l}", rxs[l])):
            got = got.cpu()
            assert scale_rel_err(got, torch.from_numpy(d["ref." + key])) <= TOL, (key, "fp32 reference")
            assert scale_rel_err(got, torch.from_numpy(d["ref64." + key])) <= TOL, (key, "fp64 reference")
            assert scale_rel_err(got, r64) <= TOL, (key, "restatement")
    assert torch.equal(out.cpu(), xs[-1].cpu())
    assert scale_rel_err(out.cpu(), torch.from_numpy(d["ref.out"])) <= TOL


@pytest.mark.parametrize("case", CASES)
def test_parameter_gradients_match_reference(case):
    d, cfg = load(case)
    m = _model(cfg)
    g = _dev(inputs(d))
    x_before = g["x"].clone()
    out, loss, grads = _grads(m, g)
    assert torch.equal(g["x"], x_before)
    assert abs(loss - float(d["ref.loss"])) <= 1e-5 * abs(float(d["ref.loss"]))
    sd64 = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    i64 = inputs(d)
    g64, _ = ref_grads(sd64, i64["h"], i64["x"], i64["edges"], i64["vel"], i64["edge_attr"], i64["charges"], i64["target"],
                       cfg["L"], cfg["norm_diff"], cfg["tanh"])
    for k, gk in grads.items():
        assert torch.isfinite(gk).all(), k
        assert scale_rel_err(gk, g64[k]) <= GTOL, (k, "restatement")
        if "ref.grad." + k not in d.files:
            # the slim case (width 128, four layers): the fixture holds sum, sum of |.| and max of |.| of every gradient.
            # max|a - b| <= GTOL max|b| bounds each checksum's difference by numel GTOL max|b|
            for tag in ("ref", "ref64"):
                gmax = float(d[f"{tag}.gmax.{k}"])
                bound = gk.numel() * GTOL * gmax
                assert abs(float(gk.double().sum()) - float(d[f"{tag}.gsum.{k}"])) <= bound, (tag, k)
                assert abs(float(gk.double().abs().sum()) - float(d[f"{tag}.gabs.{k}"])) <= bound, (tag, k)
                assert abs(float(gk.abs().max()) - gmax) <= GTOL * gmax, (tag, k)
            continue
        assert scale_rel_err(gk, torch.from_numpy(d["ref.grad." + k])) <= GTOL, (k, "fp32 reference")
        if "ref64.grad." + k in d.files:
            assert scale_rel_err(gk, torch.from_numpy(d["ref64.grad." + k])) <= GTOL, (k, "fp64 reference")


def _big(H=64, L=4, norm_diff=True, tanh=False, B=128, N=20, seed=77):
    cfg = dict(B=B, N=N, H=H, L=L, norm_diff=norm_diff, tanh=tanh, seed=seed, phi_scale=1.0)
    return cfg, runner_batch(B, N, seed + 1)


def test_dynamic_20body_shape_matches_the_restatement():
    """B = 128, N = 20 (48,640 edges), the runner's defaults: finite, forward and gradients at the bars."""
    cfg, inp = _big()
    m = _model(cfg)
    g = _dev(inp)
    out, _, grads = _grads(m, g)
    assert torch.isfinite(out).all()
    sd64 = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    i64 = {k: ([e for e in v] if k == "edges" else v.double()) for k, v in inp.items()}
    want, _, _ = ref_forward(sd64, i64["h"], i64["x"], i64["edges"], i64["vel"], i64["edge_attr"], i64["charges"], 4, True,
                             False)
    assert scale_rel_err(out.cpu(), want) <= TOL
    g64, _ = ref_grads(sd64, i64["h"], i64["x"], i64["edges"], i64["vel"], i64["edge_attr"], i64["charges"], i64["target"],
                       4, True, False)
    for k, gk in grads.items():
        assert torch.isfinite(gk).all(), k
        assert scale_rel_err(gk, g64[k]) <= GTOL, k


def test_two_runs_are_bit_identical():
    cfg, inp = _big(tanh=True)
    m = _model(cfg)
    g = _dev(inp)
    o1, _, g1 = _grads(m, g)
    o2, _, g2 = _grads(m, g)
    with torch.no_grad():
        o3 = m(*_args(g))
        o4 = m(*_args(g))
    assert torch.equal(o1, o2) and torch.equal(o3, o4) and torch.equal(o1, o3)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


@pytest.mark.parametrize("H,L", [(128, 4), (64, 2)])
def test_wider_and_other_depths_match_the_restatement(H, L):
    cfg, inp = _big(H=H, L=L, norm_diff=False, tanh=True, B=3, N=7, seed=91)
    m = _model(cfg)
    out, _, grads = _grads(m, _dev(inp))
    sd64 = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    i64 = {k: ([e for e in v] if k == "edges" else v.double()) for k, v in inp.items()}
    want, _, _ = ref_forward(sd64, i64["h"], i64["x"], i64["edges"], i64["vel"], i64["edge_attr"], i64["charges"], L, False,
                             True)
    assert scale_rel_err(out.cpu(), want) <= TOL
    g64, _ = ref_grads(sd64, i64["h"], i64["x"], i64["edges"], i64["vel"], i64["edge_attr"], i64["charges"], i64["target"],
                       L, False, True)
    for k, gk in grads.items():
        assert scale_rel_err(gk, g64[k]) <= GTOL, k


def test_self_loops_and_nodes_without_edges():
    """A self loop (d = 0) and a node that is no edge's row (count clamped to 1, mean 0) or no edge's col."""
    cfg, inp = _big(norm_diff=False, tanh=False, B=1, N=6, seed=31)
    row = torch.tensor([0, 0, 1, 1, 2, 3, 3, 0, 2], dtype=torch.int64)       # node 4: no row; 5: neither
    col = torch.tensor([1, 0, 2, 1, 0, 0, 4, 3, 4], dtype=torch.int64)
    x = inp["x"]
    ea = torch.cat([inp["charges"][row] * inp["charges"][col], ((x[row] - x[col]) ** 2).sum(1, keepdim=True)], 1)
    inp = dict(inp, edges=[row, col], edge_attr=ea)
    m = _model(cfg)
    out, _, grads = _grads(m, _dev(inp))
    sd64 = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    i64 = {k: ([e for e in v] if k == "edges" else v.double()) for k, v in inp.items()}
    want, _, _ = ref_forward(sd64, i64["h"], i64["x"], i64["edges"], i64["vel"], i64["edge_attr"], i64["charges"], 4)
    assert scale_rel_err(out.cpu(), want) <= TOL
    g64, _ = ref_grads(sd64, i64["h"], i64["x"], i64["edges"], i64["vel"], i64["edge_attr"], i64["charges"], i64["target"], 4)
    for k, gk in grads.items():
        assert scale_rel_err(gk, g64[k]) <= GTOL, k


def test_graphed_train_step_equals_eager_steps():
    """Three GraphedTrainStep replays (forward + HIP backward + FusedAdamW as one graph) == three eager steps.  The
    step's constructor takes one eager warm-up step first, so both models take 1 + 3 steps."""
    cfg, inp = _big(B=16, N=20, seed=13)
    g = _dev(inp)
    m_eager, m_graph = _model(cfg), _model(cfg)
    opt = FusedAdamW(m_eager.parameters(), lr=5e-4, weight_decay=1e-12)
    eager_losses = []
    for _ in range(4):
        opt.zero_grad(set_to_none=True)
        out = m_eager(*_args(g))
        loss, grad = mse_loss_grad(out, g["target"])
        out.backward(grad)
        opt.step()
        eager_losses.append(float(loss))
    step = GraphedTrainStep(m_graph, _args(g), g["target"], lr=5e-4, weight_decay=1e-12, warmup=1)
    graph_losses = [float(step.step()) for _ in range(3)]
    step.check()
    assert graph_losses == eager_losses[1:], (graph_losses, eager_losses)
    for (k, p), q in zip(m_graph.named_parameters(), m_eager.parameters()):
        assert torch.equal(p.detach(), q.detach()), k
    assert eager_losses[-1] < eager_losses[0]


def test_inputs_that_require_grad_fail_loudly():
    cfg, inp = _big(B=1, N=3, seed=5)
    m = _model(cfg)
    g = _dev(inp)
    g["x"].requires_grad_(True)
    with pytest.raises(_lib.AetherHipError):
        m(*_args(g))
