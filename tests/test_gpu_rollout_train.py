"""Training through the device rollout (``differentiable_rollout``: aether_rollout_train_forward / aether_rollout_backward)
against torch.autograd through the oracle's rollout in fp64.

Bound: the project's own for gradients (tests/test_gpu_backward.py), ``err <= max(GTOL, 4 err32)`` with ``scale_rel_err``,
``err32`` the same oracle gradient in fp32 against fp64 -- for every parameter tensor and for x0, vel0.  The CPU side
(tests/test_rollout_train_inputs.py) holds the inputs of every case here clear of branch cuts and err32 below GTOL.
"""
import ctypes as C

import pytest
import torch

from conftest import scale_rel_err
from aether_amd import _lib
from aether_amd.nn.state2state._frame import GraphCache
from aether_amd.nn.state2state.aether import Aether
from aether_amd.nn.state2state.locs import LoCS
from aether_amd.rollout import rollout_loss
from aether_amd.synthetic import make_batch
from rollout_train_cases import (GTOL, LAYOUT_SHAPES, MULTIGRAPH, SHAPES, TWO_STEPS, case, locs_case, multigraph_case,
                                 state_dict, step_loss)

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATHS = {"fused": _lib.FLAG_FORCE_FUSED, "streamed": _lib.FLAG_FORCE_STREAMED, "default": 0}


def _model(D, path="default", cls=Aether, sd=None):
    m = cls(2 * D, 64, 0.0, D, device=DEV)
    m.load_state_dict(state_dict(D) if sd is None else sd)
    m.flags = PATHS[path]
    return m


def _hip_grads(m, x, vel, edges, charges, targets, K, dt, leaves=True):
    """-> ({parameter key | "x0" | "vel0": gradient on the CPU}, trajectory on the CPU)."""
    m.zero_grad(set_to_none=True)
    x0 = x.to(DEV).clone().requires_grad_(leaves)
    v0 = vel.to(DEV).clone().requires_grad_(leaves)
    traj = m.differentiable_rollout(x0, v0, [e.to(DEV) for e in edges], charges.to(DEV), K, dt)
    step_loss(traj, targets.to(device=DEV, dtype=torch.float32)).backward()
    torch.cuda.synchronize()
    g = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}
    if leaves:
        g["x0"], g["vel0"] = x0.grad.cpu(), v0.grad.cpu()
    return g, traj.detach().cpu()


def _hold(tag, got, g64, g32):
    worst = (0.0, 0.0, "")
    for k, want in g64.items():
        assert torch.isfinite(got[k]).all(), (tag, k)
        err, err32 = scale_rel_err(got[k], want), scale_rel_err(g32[k], want)
        worst = max(worst, (err, err32, k))
        assert err <= max(GTOL, 4 * err32), (tag, k, err, err32)
    print(f"[rollout training] {tag}: worst gradient error {worst[0]:.2e} ({worst[2]}; fp32 oracle there {worst[1]:.2e})")


@pytest.mark.parametrize("path", ["fused", "streamed"])
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("D", [2, 3])
def test_rollout_gradients_match_oracle_autograd(D, shape, path):
    B, N, K, dt, seed = shape
    c = case(D, *shape)
    inp = c["inp"]
    got, traj = _hip_grads(_model(D, path), inp["x"], inp["vel"], inp["edges"], inp["charges"], c["targets"], K, dt)
    assert scale_rel_err(traj, c["traj64"]) <= 1e-5
    assert set(got) == set(c["g64"])
    _hold(f"D={D} {shape} {path}", got, c["g64"], c["g32"])


@pytest.mark.parametrize("path", ["fused", "streamed"])
@pytest.mark.parametrize("D", [2, 3])
def test_training_forward_gives_the_trajectory_of_rollout(D, path):
    """The keeping forward runs the inference rollout's arithmetic (same kernels with the save-for-backward stores, edge
    attributes derived in the kernels, the same velocity chain): the same bits."""
    inp = make_batch(5, 7, D, seed=6, device=DEV)
    m = _model(D, path)
    want = m.rollout(inp["x"], inp["vel"], inp["edges"], inp["charges"], 6, 0.5)
    got = m.differentiable_rollout(inp["x"], inp["vel"], inp["edges"], inp["charges"], 6, 0.5)
    assert got.requires_grad and got.shape == want.shape
    print(f"[rollout training] D={D} {path}: training forward vs rollout {scale_rel_err(got.detach().cpu(), want.cpu()):.2e}")
    assert scale_rel_err(got.detach().cpu(), want.cpu()) <= 1e-6
    assert torch.equal(got.detach(), want)
    m.eval()                                                     # train() and eval() alike
    assert torch.equal(m.differentiable_rollout(inp["x"], inp["vel"], inp["edges"], inp["charges"], 6, 0.5).detach(), want)


@pytest.mark.parametrize("D", [2, 3])
def test_one_step_equals_forward_and_backward(D):
    """K = 1: the gradients of ``forward`` + ``backward`` with the edge attributes built from x by torch (the distance
    term of d/dx0 comes from the chain kernel on one side and from autograd on the other)."""
    inp = make_batch(3, 5, D, seed=3, device=DEV)
    g = torch.Generator().manual_seed(103)
    target = (inp["x"] + inp["vel"]).cpu() + 0.05 * torch.randn(inp["x"].shape, generator=g)
    m = _model(D, "fused")
    got, traj = _hip_grads(m, inp["x"], inp["vel"], inp["edges"], inp["charges"], target[None], 1, 1.0)
    m.zero_grad(set_to_none=True)
    x0, v0 = inp["x"].clone().requires_grad_(True), inp["vel"].clone().requires_grad_(True)
    rows, cols = inp["edges"]
    dist = torch.sqrt(torch.sum((x0[rows] - x0[cols]) ** 2, 1)).unsqueeze(1)
    ea = torch.cat([inp["charges"][rows] * inp["charges"][cols], dist], 1)
    out = m(inp["h"], x0, inp["edges"], v0, ea, inp["charges"])
    step_loss(out[None], target[None].to(DEV)).backward()
    assert scale_rel_err(traj[0], out.detach().cpu()) <= 1e-6
    want = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    want["x0"], want["vel0"] = x0.grad.cpu(), v0.grad.cpu()
    for k in want:
        assert scale_rel_err(got[k], want[k]) <= GTOL, k


@pytest.mark.parametrize("path", ["fused", "streamed"])
@pytest.mark.parametrize("D", [2, 3])
def test_two_steps_the_first_link_of_the_velocity_chain(D, path):
    """K = 2: the smallest rollout in which x_1 feeds a later step as position AND as both ends of velocities."""
    B, N, K, dt, seed = TWO_STEPS
    c = case(D, *TWO_STEPS)
    inp = c["inp"]
    got, _ = _hip_grads(_model(D, path), inp["x"], inp["vel"], inp["edges"], inp["charges"], c["targets"], K, dt)
    _hold(f"D={D} K=2 {path}", got, c["g64"], c["g32"])


@pytest.mark.parametrize("D", [2, 3])
def test_multigraph_through_both_graph_builders(D):
    """Components of 1..40 nodes, repeated edges, isolated nodes, nodes without in- or out-edges, unsorted
    (rollout_train_cases.multigraph_batch)."""
    K, dt, seed = MULTIGRAPH
    c = multigraph_case(D)
    inp = c["inp"]
    lib = _lib.load()
    results = {}
    try:
        for builder in (1, 0):                                    # counting sort, radix sort
            _lib.check(lib.aether_set_option(b"graph_build", builder), "set_option")
            for path in ("default", "streamed"):
                m = _model(D, path)
                m._graphs = GraphCache()
                got, _ = _hip_grads(m, inp["x"], inp["vel"], inp["edges"], inp["charges"], c["targets"], K, dt)
                _hold(f"D={D} multigraph builder={builder} {path}", got, c["g64"], c["g32"])
                results[(builder, path)] = got
    finally:
        _lib.check(lib.aether_set_option(b"graph_build", 1), "set_option")
    for path in ("default", "streamed"):                          # the same view from both builders: the same bits
        for k, v in results[(1, path)].items():
            assert torch.equal(v, results[(0, path)][k]), (path, k)


@pytest.mark.parametrize("layout", list(LAYOUT_SHAPES))
@pytest.mark.parametrize("D", [2, 3])
def test_fused_group_layouts_match_oracle_autograd(D, layout):
    """Fused keeping forward + fused backward at every group layout of the fused kernels, and the streamed forward +
    layer-by-layer backward of the same rollout: both against the oracle, bound as everywhere."""
    lib = _lib.load()
    B, N, K, dt, seed = LAYOUT_SHAPES[layout]
    c = case(D, *LAYOUT_SHAPES[layout])
    inp = c["inp"]
    mf = _model(D, "fused")
    edges = [e.to(DEV) for e in inp["edges"]]                     # (the graph cache goes by the index tensors themselves)
    try:
        if layout == "two_tile_waves":                            # so few groups are split unless the view is built without
            _lib.check(lib.aether_set_option(b"fused_split", 0), "set_option")
        fused, t_f = _hip_grads(mf, inp["x"], inp["vel"], edges, inp["charges"], c["targets"], K, dt)
    finally:
        _lib.check(lib.aether_set_option(b"fused_split", 1), "set_option")
    _, ginfo = mf.prepare_graph(edges, B * N)                     # the view the rollout ran on
    tiles, split = (ginfo.max_group_edges + 15) // 16, bool(ginfo.reserved & 1)
    if layout == "one_node_tile":
        assert ginfo.max_group_nodes <= 16 and not split
    elif layout == "two_tile_waves":
        assert 8 < tiles <= 16 and not split                      # 8 waves: every wave owns two tiles
    else:
        assert split
    assert scale_rel_err(t_f, c["traj64"]) <= 1e-5
    _hold(f"D={D} {layout} fused", fused, c["g64"], c["g32"])
    try:
        _lib.check(lib.aether_set_option(b"fused_backward", 0), "set_option")
        layers, t_l = _hip_grads(_model(D, "streamed"), inp["x"], inp["vel"], inp["edges"], inp["charges"], c["targets"], K, dt)
    finally:
        _lib.check(lib.aether_set_option(b"fused_backward", 1), "set_option")
    assert scale_rel_err(t_l, c["traj64"]) <= 1e-5
    _hold(f"D={D} {layout} streamed + layer-by-layer backward", layers, c["g64"], c["g32"])


@pytest.mark.parametrize("path", ["fused", "streamed"])
def test_gradients_are_bit_identical_run_to_run(path):
    D = 2
    c = case(D, *SHAPES[3])
    inp = c["inp"]
    m = _model(D, path)
    runs = [_hip_grads(m, inp["x"], inp["vel"], inp["edges"], inp["charges"], c["targets"], 6, 1.0)[0] for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


@pytest.mark.parametrize("as_view", [True, False])
def test_grad_accumulates_across_calls_and_frozen_tensors_stay_out(as_view):
    D = 2
    a, b = case(D, *SHAPES[0]), case(D, *SHAPES[2])
    m = _model(D, "fused")
    m.grad_as_view = as_view

    def loss(c):
        i = c["inp"]
        return rollout_loss(m, i["x"].to(DEV), i["vel"].to(DEV), [e.to(DEV) for e in i["edges"]], i["charges"].to(DEV),
                            c["targets"].to(device=DEV, dtype=torch.float32), 1.0)

    def grads():
        return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    la = loss(a)
    la.backward()
    ga = grads()
    with torch.no_grad():                                         # the loss itself: torch's MSE of the same trajectory
        i = a["inp"]
        traj = m.rollout(i["x"].to(DEV), i["vel"].to(DEV), [e.to(DEV) for e in i["edges"]], i["charges"].to(DEV), SHAPES[0][2], 1.0)
        want = torch.nn.functional.mse_loss(traj, a["targets"].to(device=DEV, dtype=torch.float32))
    assert abs(float(la.detach()) - float(want)) <= 1e-6 * float(want)
    m.zero_grad(set_to_none=True)
    loss(b).backward()
    gb = grads()
    m.zero_grad(set_to_none=True)
    loss(a).backward()
    loss(b).backward()                                            # no zero_grad in between
    g2 = grads()
    m.zero_grad(set_to_none=True)
    (loss(a) + loss(b)).backward()                                # both rollouts in ONE autograd graph
    g3 = grads()
    for k in ga:
        want = ga[k] + gb[k]
        tol = 1e-6 * float(want.abs().max()) + 1e-12
        assert float((g2[k] - want).abs().max()) <= tol, k
        assert float((g3[k] - want).abs().max()) <= tol, k
    frozen = "gnn.layer_2.message_fn.0.weight"
    dict(m.named_parameters())[frozen].requires_grad_(False)
    m.zero_grad(set_to_none=True)
    loss(a).backward()
    gf = grads()
    assert frozen not in gf and set(gf) == set(ga) - {frozen}
    for k in gf:
        assert torch.equal(gf[k], ga[k]), k


@pytest.mark.parametrize("hidden", [64, 20])
@pytest.mark.parametrize("D", [2, 3])
def test_locs_rollout_gradients_match_its_restatement(D, hidden):
    """LoCS at SHAPES[0] against autograd through tests/locs_restatement.py::rollout; hidden 20: a narrow model, whose
    tensors the kernels read through engine-shaped images."""
    B, N, K, dt, seed = SHAPES[0]
    sd, c = locs_case(D, hidden)
    inp = c["inp"]
    m = LoCS(2 * D, hidden, 0.0, D, device=DEV)
    m.load_state_dict(sd)
    for path in ("fused", "streamed"):
        m.flags = PATHS[path]
        got, traj = _hip_grads(m, inp["x"], inp["vel"], inp["edges"], inp["charges"], c["targets"], K, dt)
        assert scale_rel_err(traj, c["traj64"]) <= 1e-5
        assert set(got) == set(c["g64"]) and all(got[k].shape == c["g64"][k].shape for k in got)
        _hold(f"LoCS D={D} hidden {hidden} {path}", got, c["g64"], c["g32"])


def test_graphed_rollout_train_step_matches_eager_steps():
    """One hipGraph of rollout forward + loss + backward through time, the optimizer as in GraphedTrainStep: three
    replays leave the parameters where three eager steps of the same kernels leave them."""
    from aether_amd.optim import FusedAdamW
    from aether_amd.training import GraphedRolloutTrainStep
    D, K, dt = 2, 3, 0.5
    c = case(D, *SHAPES[1])
    i = c["inp"]
    x, v, q = i["x"].to(DEV), i["vel"].to(DEV), i["charges"].to(DEV)
    edges = [e.to(DEV) for e in i["edges"]]
    tgt = c["targets"].to(device=DEV, dtype=torch.float32)
    m1, m2 = _model(D), _model(D)
    step = GraphedRolloutTrainStep(m1, (x, v, edges, q), tgt, dt=dt, lr=1e-3, weight_decay=1e-12, warmup=1)
    opt = FusedAdamW(m2.parameters(), lr=1e-3, weight_decay=1e-12)
    losses = []
    for k in range(4):                                            # the helper's one warm-up step, then three
        opt.zero_grad(set_to_none=True)
        loss = rollout_loss(m2, x, v, edges, q, tgt, dt)
        loss.backward()
        opt.step()
        if k:
            lg = float(step.step().detach())
            assert abs(lg - float(loss.detach())) <= 1e-6 * abs(lg)
            losses.append(lg)
    step.check()
    assert losses[-1] < losses[0]
    for (k, p), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert float((p.detach() - p2.detach()).abs().max()) <= 1e-6, k


def test_entry_checks_return_their_codes_and_leave_the_library_usable():
    lib = _lib.load()
    D, K = 2, 2
    inp = make_batch(2, 5, D, seed=1, device=DEV)
    m = _model(D)
    n, E = inp["x"].shape[0], inp["edges"][0].numel()
    gbuf, ginfo = m.prepare_graph(inp["edges"], n)
    ps = m._param_struct_ref()
    _, gstruct, _ = m._grad_buffers()
    nbytes = lib.aether_rollout_train_workspace_bytes(n, E, D, 64, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    traj = torch.empty(K, n, D, device=DEV)
    gt = torch.ones(K, n, D, device=DEV)
    gx, gv = torch.empty(n, D, device=DEV), torch.empty(n, D, device=DEV)
    x, v, q = inp["x"], inp["vel"], inp["charges"]
    st = torch.cuda.current_stream().cuda_stream
    other = _lib.AetherGraphInfo(n + 1, E, ginfo.n_groups, ginfo.max_group_nodes, ginfo.max_group_edges, ginfo.reserved)

    def fwd(ps=ps, D=D, H=64, x=x.data_ptr(), v=v.data_ptr(), q=q.data_ptr(), g=gbuf.data_ptr(), info=ginfo, ws=ws.data_ptr(),
            wsb=nbytes, traj=traj.data_ptr(), K=K, dt=1.0, flags=0):
        return lib.aether_rollout_train_forward(ps, D, H, n, E, x, v, q, g, C.byref(info), ws, wsb, traj, K, dt, flags, st)

    def bwd(ps=ps, gs=C.byref(gstruct), D=D, H=64, x=x.data_ptr(), v=v.data_ptr(), q=q.data_ptr(), g=gbuf.data_ptr(), info=ginfo,
            ws=ws.data_ptr(), wsb=nbytes, traj=traj.data_ptr(), gt=gt.data_ptr(), gx=gx.data_ptr(), gv=gv.data_ptr(), K=K, dt=1.0):
        return lib.aether_rollout_backward(ps, gs, D, H, n, E, x, v, q, g, C.byref(info), ws, wsb, traj, gt, gx, gv, K, dt, st)

    EINVAL, ESPACE = -1, -4
    for call in (fwd, bwd):
        for kw, code in [(dict(ps=None), EINVAL), (dict(x=None), EINVAL), (dict(v=None), EINVAL), (dict(q=None), EINVAL),
                         (dict(g=None), EINVAL), (dict(ws=None), EINVAL), (dict(traj=None), EINVAL), (dict(D=4), EINVAL),
                         (dict(info=other), EINVAL), (dict(K=0), EINVAL), (dict(dt=0.0), EINVAL), (dict(H=128), EINVAL),
                         (dict(H=32), EINVAL), (dict(wsb=nbytes - 1), ESPACE)]:
            assert call(**kw) == code, (call.__name__, kw)
            assert lib.aether_last_error()
    assert fwd(H=128) == EINVAL and b"rollout training: 64-wide engine only" in lib.aether_last_error()
    assert bwd(gs=None) == EINVAL and bwd(gt=None) == EINVAL
    null_grad = _lib.AetherParams.from_buffer_copy(gstruct)
    null_grad.out_b6 = None
    assert bwd(gs=C.byref(null_grad)) == EINVAL
    assert fwd(flags=_lib.FLAG_FORCE_FUSED, g=gbuf.data_ptr(),
               info=_lib.AetherGraphInfo(n, E, 0, 0, 0, 0)) == EINVAL                 # fused asked for, no groups
    # a valid pair after all of them; either input gradient may be left out (a backward consumes the forward's workspace:
    # one forward per backward)
    assert fwd() == 0 and bwd() == 0
    full = (gx.clone(), gv.clone())
    assert fwd() == 0 and bwd(gx=None) == 0 and fwd() == 0 and bwd(gv=None) == 0 and fwd() == 0 and bwd(gx=None, gv=None) == 0
    torch.cuda.synchronize()
    _lib.check(lib.aether_check_async_error(), "async")
    assert torch.isfinite(traj).all() and torch.isfinite(full[0]).all() and torch.isfinite(full[1]).all()
    assert torch.equal(gx, full[0]) and torch.equal(gv, full[1])


def test_python_error_paths():
    D = 2
    inp = make_batch(2, 5, D, seed=1, device=DEV)
    args = (inp["x"], inp["vel"], inp["edges"], inp["charges"])
    m = Aether(2 * D, 64, 0.25, D, device=DEV)
    with pytest.raises(RuntimeError):                             # train() with dropout_prob > 0: no per-step masks
        m.differentiable_rollout(*args, 2)
    m.eval()
    assert m.differentiable_rollout(*args, 2).requires_grad
    with pytest.raises(ValueError):
        m.differentiable_rollout(*args, 0)
    with pytest.raises(ValueError):
        m.differentiable_rollout(inp["x"], inp["vel"][:-1], inp["edges"], inp["charges"], 2)
    with pytest.raises(_lib.AetherHipError, match="64-wide engine only"):
        Aether(2 * D, 128, 0.0, D, device=DEV).differentiable_rollout(*args, 2)
    with pytest.raises(_lib.AetherHipError, match="64-wide engine only"):
        Aether(2 * D, 96, 0.0, D, device=DEV).differentiable_rollout(*args, 2)      # padded to 128
    with pytest.raises(_lib.AetherHipError, match="64-wide engine only"):
        Aether(2 * D, 32, 0.0, D, device=DEV).differentiable_rollout(*args, 2)      # runs on a padded engine: not built
    from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
    with pytest.raises(_lib.AetherHipError, match="not built"):
        DynamicFieldAether(2 * D, 64, 0.0, D, device=DEV).differentiable_rollout(*args, 2)
    traj = m.differentiable_rollout(*args, 2)                     # the first backward consumes the rollout's workspace
    traj.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        traj.sum().backward()
    with pytest.raises(RuntimeError):                             # Module.rollout keeps its own errors
        Aether(2 * D, 64, 0.25, D, device=DEV).rollout(*args, 2)
