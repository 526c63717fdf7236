"""LoCS (``--model locs``) on the MI355X: Aether's kernels through the external-field entry points with a zero field and
mapped first-layer weights, against the reference's fp32 / fp64 runs (tools/make_golden_locs.py) and the fp64
restatement (tests/locs_restatement.py)."""
import contextlib
import io
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

from aether_amd import _lib
from aether_amd.nn.state2state.aether import Aether
from aether_amd.nn.state2state.locs import LoCS, aether_state_dict
from aether_amd.optim import FusedAdamW, mse_loss_grad
from aether_amd.rollout import rollout
from aether_amd.synthetic import make_batch
from aether_amd.training import GraphedTrainStep

import locs_restatement as R
from conftest import REPO, scale_rel_err
from test_locs import CASES, build, inputs, load, masks

pytestmark = pytest.mark.gpu
TOL = 1e-5       # forward: the project's bar, max|a - b| / max|b|
GTOL = 5e-5      # gradients: as tests/test_gpu_backward.py


def _dev(inp):
    return {k: ([e.cuda() for e in v] if k == "edges" else v.to(device="cuda", dtype=torch.float32)) for k, v in inp.items()}


def _batch(B, N, D, seed):
    """make_batch on the device without its meta entry."""
    return _dev({k: v for k, v in make_batch(B, N, D, seed=seed).items() if k != "meta"})


def _args(g):
    return (g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"])


def _model(cfg, flags=0):
    m = build(cfg, "cuda")
    m.flags = flags
    return m


def _sd64(m):
    return {k: v.detach().cpu().double() for k, v in m.state_dict().items()}


def _grads(m, g, inputs_too=False):
    m.zero_grad(set_to_none=True)
    leaves = {k: g[k].clone().requires_grad_(inputs_too) for k in ("x", "vel", "edge_attr")}
    out = m(g["h"], leaves["x"], g["edges"], leaves["vel"], leaves["edge_attr"])
    loss = torch.nn.functional.mse_loss(out, g["target"])
    loss.backward()
    torch.cuda.synchronize()
    pg = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    ig = {k: t.grad.detach().cpu() for k, t in leaves.items()} if inputs_too else None
    return out.detach(), float(loss.detach()), pg, ig


@pytest.mark.parametrize("flags", [0, _lib.FLAG_FORCE_STREAMED])
@pytest.mark.parametrize("case", CASES)
def test_forward_matches_reference(case, flags):
    """Every fixture case, on the fused and the streamed path (hidden > 64: csrc/wide.h, which has one path)."""
    d, cfg = load(case)
    m = _model(cfg, flags)
    g = _dev(inputs(d))
    mk = masks(d)
    if mk is not None:                          # train() mode: the reference's own masks
        m.train()
        m._dropout_masks = torch.stack([t.float() for t in mk]).cuda()
    else:
        m.eval()
    with torch.no_grad():
        out = m(*_args(g)).cpu()
    i64 = inputs(d)
    want = R.forward(_sd64(m), i64["x"], i64["vel"], i64["edges"], i64["edge_attr"], mk)
    assert scale_rel_err(out, torch.from_numpy(d["ref.out"])) <= TOL, "fp32 reference"
    if "ref64.out" in d.files:
        assert scale_rel_err(out, torch.from_numpy(d["ref64.out"])) <= TOL, "fp64 reference"
    assert scale_rel_err(out, want) <= TOL, "restatement"


@pytest.mark.parametrize("case", CASES)
def test_gradients_match_reference(case):
    """Parameter gradients of nn.MSELoss on every case; input gradients in the inputgrad case; the dropout case with the
    masks the reference drew."""
    d, cfg = load(case)
    m = _model(cfg)
    mk = masks(d)
    if mk is not None:
        m.train()
        m._dropout_masks = torch.stack([t.float() for t in mk]).cuda()
    g = _dev(inputs(d))
    out, loss, pg, ig = _grads(m, g, cfg["inputgrad"])
    assert abs(loss - float(d["ref.loss"])) <= 1e-5 * abs(float(d["ref.loss"]))
    i64 = inputs(d)
    g64, ig64, _ = R.grads(_sd64(m), i64["x"], i64["vel"], i64["edges"], i64["edge_attr"], i64["target"], mk,
                           inputs=cfg["inputgrad"])
    for k, gk in pg.items():
        assert torch.isfinite(gk).all(), k
        assert scale_rel_err(gk, g64[k]) <= GTOL, (k, "restatement")
        if "ref.grad." + k in d.files:
            assert scale_rel_err(gk, torch.from_numpy(d["ref.grad." + k])) <= GTOL, (k, "fp32 reference")
        if "ref64.grad." + k in d.files:
            assert scale_rel_err(gk, torch.from_numpy(d["ref64.grad." + k])) <= GTOL, (k, "fp64 reference")
    if cfg["inputgrad"]:
        for k, gk in ig.items():
            assert scale_rel_err(gk, torch.from_numpy(d["ref.ingrad." + k])) <= GTOL, (k, "fp32 reference")
            assert scale_rel_err(gk, torch.from_numpy(d["ref64.ingrad." + k])) <= GTOL, (k, "fp64 reference")
            assert scale_rel_err(gk, ig64[k]) <= GTOL, (k, "restatement")


def _cfg(D=2, H=64, p=0.0, seed=77):
    return dict(D=D, H=H, p=p, seed=seed)


@pytest.mark.parametrize("H", [64, 20])
def test_20body_shape_and_two_runs_are_bit_identical(H):
    """B = 128, N = 20 (cfg2): forward and gradients at the bars, and two runs give the same bits."""
    cfg = _cfg(H=H)
    inp = {k: v for k, v in make_batch(128, 20, 2, seed=5).items() if k != "meta"}
    m = _model(cfg)
    g = _dev(inp)
    o1, _, g1, _ = _grads(m, g)
    o2, _, g2, _ = _grads(m, g)
    with torch.no_grad():
        o3 = m(*_args(g))
        o4 = m(*_args(g))
    assert torch.equal(o1, o2) and torch.equal(o3, o4) and torch.equal(o1, o3)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    sd64 = _sd64(m)
    i64 = {k: ([e for e in v] if k == "edges" else v.double()) for k, v in inp.items()}
    assert scale_rel_err(o1.cpu(), R.forward(sd64, i64["x"], i64["vel"], i64["edges"], i64["edge_attr"])) <= TOL
    w64, _, _ = R.grads(sd64, i64["x"], i64["vel"], i64["edges"], i64["edge_attr"], i64["target"])
    for k, gk in g1.items():
        assert scale_rel_err(gk, w64[k]) <= GTOL, k


@pytest.mark.parametrize("D,H", [(2, 64), (3, 64), (2, 20), (3, 128)])
def test_equals_mapped_aether_with_zero_field(D, H):
    """The drop-in LoCS against the drop-in Aether whose field net is zero and whose first-layer weights are mapped: the
    same step on the device (forward; gradients of the shared tensors, the mapped ones cut back)."""
    cfg = _cfg(D=D, H=H, seed=11)
    m = _model(cfg)
    with contextlib.redirect_stdout(io.StringIO()):
        a = Aether(2 * D, H, 0.0, D, device="cuda")
    a.load_state_dict(aether_state_dict(m.state_dict(), D))
    g = _batch(3, 7, D, 12)
    with torch.no_grad():
        ol = m(*_args(g))
        oa = a(*_args(g), g["charges"])
    assert scale_rel_err(ol.cpu(), oa.cpu()) <= 1e-6
    _, _, gl, _ = _grads(m, g)
    a.zero_grad(set_to_none=True)
    torch.nn.functional.mse_loss(a(*_args(g), g["charges"]), g["target"]).backward()
    O_ = D * (D - 1) // 2
    for k, p in a.named_parameters():
        if k.startswith("field_net."):
            continue
        gk = p.grad.detach().cpu()
        if k == "gnn.layer_1.message_fn.0.weight":
            gk = torch.cat([gk[:, :3 * D + O_], gk[:, 4 * D + O_:6 * D + O_], gk[:, -2:]], 1)
        elif k == "gnn.layer_1.res.weight":
            gk = gk[:, :2 * D]
        assert scale_rel_err(gl[k], gk) <= 1e-5, k


@pytest.mark.parametrize("H", [64, 20])
def test_graphed_train_step_equals_eager_steps(H):
    """Three GraphedTrainStep replays (forward + HIP backward + FusedAdamW as one graph, the engine's weight copies
    included) == three eager steps, bit for bit; the loss falls.  The step's constructor takes one eager warm-up step
    first, so both models take 1 + 3 steps."""
    cfg = _cfg(H=H, seed=13)
    g = _batch(16, 20, 2, 14)
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
    # the .grad tensors the optimizer reads are views of the flat buffer
    flat = m_graph._grad_buffers()[0]
    assert step._flat_gradient_buffer() is flat
    # an inference call after the replays sees the trained weights (engine copies refreshed)
    with torch.no_grad():
        o_g, o_e = m_graph(*_args(g)), m_eager(*_args(g))
    assert torch.equal(o_g, o_e)


@pytest.mark.parametrize("H", [64, 20])
def test_captured_step_survives_a_larger_forward_and_a_checkpoint_load(H):
    """The device buffers a captured step holds (zero field, engine images, gradient scratch, column index) outlive a
    forward on a larger batch (the zero buffer grows) and a load_state_dict; freed device memory is then overwritten with
    NaN, and the replays must still equal eager steps bit for bit."""
    cfg = _cfg(H=H, seed=17)
    g = _batch(8, 20, 2, 18)
    big = _batch(32, 20, 2, 19)
    m_eager, m_graph = _model(cfg), _model(cfg)
    opt = FusedAdamW(m_eager.parameters(), lr=5e-4, weight_decay=1e-12)

    def eager_step():
        opt.zero_grad(set_to_none=True)
        out = m_eager(*_args(g))
        loss, grad = mse_loss_grad(out, g["target"])
        out.backward(grad)
        opt.step()
        return float(loss)

    eager_losses = [eager_step() for _ in range(2)]
    step = GraphedTrainStep(m_graph, _args(g), g["target"], lr=5e-4, weight_decay=1e-12, warmup=1)
    graph_losses = [float(step.step())]
    with torch.no_grad():                      # a larger system: every size-dependent buffer grows
        for m in (m_graph, m_eager):
            m(*_args(big))
    ckpt = {k: v.clone() for k, v in m_eager.state_dict().items()}
    m_graph.load_state_dict(ckpt)              # the same values: the replays must not notice
    m_eager.load_state_dict(ckpt)
    torch.cuda.synchronize()
    junk = [torch.full((1 << 18,), float("nan"), device="cuda") for _ in range(64)]     # reuse freed blocks
    for _ in range(3):
        eager_losses.append(eager_step())
        graph_losses.append(float(step.step()))
    step.check()
    del junk
    assert graph_losses == eager_losses[1:], (graph_losses, eager_losses)
    for (k, p), q in zip(m_graph.named_parameters(), m_eager.parameters()):
        assert torch.equal(p.detach(), q.detach()), k


@pytest.mark.parametrize("D,H", [(2, 20), (3, 128), (2, 96)])
def test_input_gradients_narrow_and_wide(D, H):
    """x / vel / edge_attr gradients through the padded engine (hidden < 64) and csrc/wide.h (hidden > 64), against the
    fp64 restatement."""
    cfg = _cfg(D=D, H=H, seed=23)
    inp = {k: v for k, v in make_batch(3, 7, D, seed=24).items() if k != "meta"}
    m = _model(cfg)
    _, _, pg, ig = _grads(m, _dev(inp), inputs_too=True)
    i64 = {k: ([e for e in v] if k == "edges" else v.double()) for k, v in inp.items()}
    g64, ig64, _ = R.grads(_sd64(m), i64["x"], i64["vel"], i64["edges"], i64["edge_attr"], i64["target"], inputs=True)
    for k, gk in ig.items():
        assert torch.isfinite(gk).all(), k
        assert scale_rel_err(gk, ig64[k]) <= GTOL, k
    for k, gk in pg.items():
        assert scale_rel_err(gk, g64[k]) <= GTOL, k


def _stepwise(m, x, vel, edges, charges, steps, dt):
    """The loop of module calls around forward (experiments/lorentz/main.py:236-241)."""
    rows, cols = edges
    qprod = charges[rows] * charges[cols]
    traj = []
    with torch.no_grad():
        for _ in range(steps):
            ea = torch.cat([qprod, torch.sqrt(torch.sum((x[rows] - x[cols]) ** 2, 1)).unsqueeze(1)], 1)
            xn = m(vel.norm(dim=-1, keepdim=True), x, edges, vel, ea)
            vel = (xn - x) / dt
            x = xn
            traj.append(x)
    return torch.stack(traj)


@pytest.mark.parametrize("flags", [0, _lib.FLAG_FORCE_STREAMED])
@pytest.mark.parametrize("D,H", [(2, 64), (3, 64), (2, 20), (3, 128)])
def test_device_rollout_equals_loop_and_restatement(D, H, flags):
    cfg = _cfg(D=D, H=H, seed=21)
    m = _model(cfg, flags if H <= 64 else 0).eval()
    for (B, N, T, dt, seed) in [(4, 5, 6, 1.0, 3), (2, 9, 4, 0.5, 4)]:
        inp = make_batch(B, N, D, seed=seed, device="cuda")
        a = rollout(m, inp["x"], inp["vel"], inp["edges"], inp["charges"], T, dt)
        b = _stepwise(m, inp["x"], inp["vel"], inp["edges"], inp["charges"], T, dt)
        assert a.shape == (T, B * N, D)
        assert scale_rel_err(a[0].cpu(), b[0].cpu()) <= 1e-6          # one step: same arithmetic up to fma contraction
        assert scale_rel_err(a.cpu(), b.cpu()) <= TOL
        c = R.rollout(_sd64(m), inp["x"].cpu().double(), inp["vel"].cpu().double(), [e.cpu() for e in inp["edges"]],
                      inp["charges"].cpu().double(), T, dt)
        assert scale_rel_err(a.cpu(), c) <= 1e-4                      # T steps of a chaotic map: the error grows per step
    assert rollout(m, inp["x"], inp["vel"], inp["edges"], inp["charges"], 0).shape == (0, B * N, D)


def test_rollout_refuses_train_mode_dropout():
    m = _model(_cfg(p=0.1))
    inp = make_batch(1, 5, 2, seed=1, device="cuda")
    m.train()
    with pytest.raises(RuntimeError):
        m.rollout(inp["x"], inp["vel"], inp["edges"], inp["charges"], 2)
    m.eval()
    assert m.rollout(inp["x"], inp["vel"], inp["edges"], inp["charges"], 2).shape == (2, 5, 2)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, H):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from aether_amd.edges import get_edges, prepare_edge_attr
    from aether_amd.nn.state2state.locs import LoCS
    from aether_amd.parallel import attach_data_parallel, shard_graphs
    from aether_amd.synthetic import make_batch
    D, B, N = 2, 8, 20
    dev = torch.device("cuda", 0)
    torch.manual_seed(100 + rank)                        # ranks start from different weights
    with contextlib.redirect_stdout(io.StringIO()):
        m = LoCS(2 * D, H, 0.0, D, device=dev)
    attach_data_parallel(m)                              # broadcast from rank 0
    full = make_batch(B, N, D, seed=9)
    lo, hi = shard_graphs(B, rank, world)
    sl = slice(lo * N, hi * N)
    edges = get_edges(hi - lo, N, device=dev)
    x, v, q_, tgt = (full[k][sl].to(dev) for k in ("x", "vel", "charges", "target"))
    ea = prepare_edge_attr(x, edges, q_[edges[0]] * q_[edges[1]])
    start = {k: p.detach().cpu().numpy().copy() for k, p in m.named_parameters()}     # after the broadcast
    out = m(v.norm(dim=-1, keepdim=True), x, edges, v, ea)
    torch.nn.functional.mse_loss(out, tgt).backward()    # all-reduce + mean happen inside the backward
    grads = {k: p.grad.detach().cpu().numpy().copy() for k, p in m.named_parameters()}
    torch.cuda.synchronize()
    q.put((rank, grads, start, (lo, hi)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("H", [64, 20])
def test_two_ranks_on_one_gpu_match_single_process_gradients(H):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, H)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    D, B, N = 2, 8, 20
    with contextlib.redirect_stdout(io.StringIO()):
        m = LoCS(2 * D, H, 0.0, D, device="cuda")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in res[0][2].items()})          # rank 0's broadcast weights
    assert all((res[0][2][k] == res[1][2][k]).all() for k in res[0][2])
    full = make_batch(B, N, D, seed=9, device="cuda")
    out = m(full["h"], full["x"], full["edges"], full["vel"], full["edge_attr"])
    torch.nn.functional.mse_loss(out, full["target"]).backward()
    for rank, grads, _, _ in res:
        for k, p in m.named_parameters():
            assert scale_rel_err(torch.from_numpy(grads[k]), p.grad.cpu()) <= GTOL, (rank, k)
        assert all((grads[k] == res[0][1][k]).all() for k in grads)                    # both ranks hold the mean
