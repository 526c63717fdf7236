"""Training DynamicFieldAether through the device rollout (``differentiable_rollout``:
aether_rollout_dynamic_field_train_forward / aether_rollout_dynamic_field_backward) against torch.autograd through the
oracle's protocol in fp64 (tests/dynfield_rollout_cases.py).

Bound: the project's own for gradients, ``err <= max(GTOL, 4 err32)`` with ``scale_rel_err``, ``err32`` the same oracle
gradient in fp32 against fp64 -- for every parameter tensor and for x0, vel0; the gate's last bias has an exactly zero
gradient (softmax is shift invariant): |g| <= 1e-9 on both sides instead.  The CPU side
(tests/test_dynfield_rollout_inputs.py) holds the inputs of every case here clear of branch cuts and err32 below GTOL.
"""
import ctypes as C

import pytest
import torch

from conftest import scale_rel_err
from aether_amd import _lib
from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether, _DynFieldParams
from aether_amd.rollout import rollout_loss
from aether_amd.synthetic import make_batch
from dynfield_rollout_cases import GTOL, LAYOUT_SHAPES, NARROW, SHAPES, TWO_STEPS, ZERO_GRAD, case, state_dict, step_loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATHS = {"fused": _lib.FLAG_FORCE_FUSED, "streamed": _lib.FLAG_FORCE_STREAMED, "default": 0}


def _model(D, path="default", H=64):
    m = DynamicFieldAether(2 * D, H, 0.0, D, device=DEV)
    m.load_state_dict(state_dict(D, H))
    m.flags = PATHS[path]
    return m


def _hip_grads(m, x, vel, edges, charges, targets, K, dt, N):
    """-> ({parameter key | "x0" | "vel0": gradient on the CPU}, trajectory on the CPU)."""
    m.zero_grad(set_to_none=True)
    x0, v0 = x.to(DEV).clone().requires_grad_(True), vel.to(DEV).clone().requires_grad_(True)
    edges = [e.to(DEV) for e in edges]
    traj = m.differentiable_rollout(x0, v0, edges, charges.to(DEV), K, dt, num_nodes=N)
    step_loss(traj, targets.to(device=DEV, dtype=torch.float32)).backward()
    torch.cuda.synchronize()
    _lib.check(_lib.load().aether_check_async_error(), "async")
    g = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}
    g["x0"], g["vel0"] = x0.grad.cpu(), v0.grad.cpu()
    return g, traj.detach().cpu()


def _hold(tag, got, g64, g32):
    worst = (0.0, 0.0, "")
    for k, want in g64.items():
        assert torch.isfinite(got[k]).all(), (tag, k)
        assert got[k].shape == want.shape, (tag, k)
        if k == ZERO_GRAD:
            print(f"[dynfield rollout training] {tag}: {k} |g| {float(got[k].abs().max()):.2e} (oracle {float(want.abs().max()):.2e})")
            assert float(got[k].abs().max()) <= 1e-9 and float(want.abs().max()) <= 1e-9, (tag, k)
            continue
        err, err32 = scale_rel_err(got[k], want), scale_rel_err(g32[k], want)
        worst = max(worst, (err, err32, k))
        assert err <= max(GTOL, 4 * err32), (tag, k, err, err32)
    print(f"[dynfield rollout training] {tag}: worst gradient error {worst[0]:.2e} ({worst[2]}; fp32 oracle there {worst[1]:.2e})")


def _check_case(D, shape, path):
    H, B, N, K, dt, seed = shape
    c = case(D, *shape)
    inp = c["inp"]
    m = _model(D, path, H)
    got, traj = _hip_grads(m, inp["x"], inp["vel"], inp["edges"], inp["charges"], c["targets"], K, dt, N)
    assert scale_rel_err(traj, c["traj64"]) <= 1e-5
    assert set(got) == set(k for k, _ in m.named_parameters()) | {"x0", "vel0"} == set(c["g64"])
    _hold(f"D={D} {shape} {path}", got, c["g64"], c["g32"])


@pytest.mark.parametrize("path", ["fused", "streamed"])
@pytest.mark.parametrize("shape", SHAPES + [TWO_STEPS])
@pytest.mark.parametrize("D", [2, 3])
def test_rollout_gradients_match_oracle_autograd(D, shape, path):
    _check_case(D, shape, path)


@pytest.mark.parametrize("layout", list(LAYOUT_SHAPES))
@pytest.mark.parametrize("D", [2, 3])
def test_fused_group_layouts_match_oracle_autograd(D, layout):
    """The fused keeping forward + fused backward at every group layout of the fused kernels; the view is built as
    tests/test_gpu_rollout_train.py builds it."""
    lib = _lib.load()
    shape = LAYOUT_SHAPES[layout]
    H, B, N, K, dt, seed = shape
    c = case(D, *shape)
    inp = c["inp"]
    m = _model(D, "fused")
    edges = [e.to(DEV) for e in inp["edges"]]                     # (the graph cache goes by the index tensors themselves)
    try:
        if layout == "two_tile_waves":                            # so few groups are split unless the view is built without
            _lib.check(lib.aether_set_option(b"fused_split", 0), "set_option")
        got, traj = _hip_grads(m, inp["x"], inp["vel"], edges, inp["charges"], c["targets"], K, dt, N)
    finally:
        _lib.check(lib.aether_set_option(b"fused_split", 1), "set_option")
    _, ginfo = m.prepare_graph(edges, B * N)                      # the view the rollout ran on
    tiles, split = (ginfo.max_group_edges + 15) // 16, bool(ginfo.reserved & 1)
    if layout == "one_node_tile":
        assert ginfo.max_group_nodes <= 16 and not split
    elif layout == "two_tile_waves":
        assert 8 < tiles <= 16 and not split
    else:
        assert split
    assert scale_rel_err(traj, c["traj64"]) <= 1e-5
    _hold(f"D={D} {layout} fused", got, c["g64"], c["g32"])


@pytest.mark.parametrize("path", ["fused", "streamed"])
@pytest.mark.parametrize("D", [2, 3])
def test_training_forward_gives_the_trajectory_of_rollout(D, path):
    """The keeping forward runs aether_rollout_dynamic_field's arithmetic: the same bits, in train() and in eval()."""
    inp = make_batch(5, 7, D, seed=6, device=DEV)
    args = (inp["x"], inp["vel"], inp["edges"], inp["charges"], 6, 0.5)
    m = _model(D, path)
    want = m.rollout(*args, num_nodes=7)
    got = m.differentiable_rollout(*args, num_nodes=7)
    assert got.requires_grad and got.shape == want.shape
    assert torch.equal(got.detach(), want)
    m.eval()
    assert torch.equal(m.differentiable_rollout(*args, num_nodes=7).detach(), want)


@pytest.mark.parametrize("D", [2, 3])
def test_one_step_equals_forward_and_backward(D):
    """K = 1: the gradients of the module's own ``forward`` + ``backward`` with the edge attributes built from x by torch."""
    N = 5
    inp = make_batch(3, N, D, seed=3, device=DEV)
    g = torch.Generator().manual_seed(103)
    target = (inp["x"] + inp["vel"]).cpu() + 0.05 * torch.randn(inp["x"].shape, generator=g)
    m = _model(D, "fused")
    got, traj = _hip_grads(m, inp["x"], inp["vel"], inp["edges"], inp["charges"], target[None], 1, 1.0, N)
    m.zero_grad(set_to_none=True)
    x0, v0 = inp["x"].clone().requires_grad_(True), inp["vel"].clone().requires_grad_(True)
    rows, cols = inp["edges"]
    dist = torch.sqrt(torch.sum((x0[rows] - x0[cols]) ** 2, 1)).unsqueeze(1)
    ea = torch.cat([inp["charges"][rows] * inp["charges"][cols], dist], 1)
    out = m(inp["h"], x0, inp["edges"], v0, ea, inp["charges"], N)
    step_loss(out[None], target[None].to(DEV)).backward()
    assert scale_rel_err(traj[0], out.detach().cpu()) <= 1e-6
    want = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    want["x0"], want["vel0"] = x0.grad.cpu(), v0.grad.cpu()
    assert set(got) == set(want)
    for k in want:
        if k == ZERO_GRAD:
            assert float(got[k].abs().max()) <= 1e-9 and float(want[k].abs().max()) <= 1e-9
            continue
        assert scale_rel_err(got[k], want[k]) <= GTOL, k


@pytest.mark.parametrize("path", ["fused", "streamed"])
def test_gradients_are_bit_identical_run_to_run(path):
    D = 2
    shape = SHAPES[3]
    H, B, N, K, dt, seed = shape
    c = case(D, *shape)
    inp = c["inp"]
    m = _model(D, path)
    runs = [_hip_grads(m, inp["x"], inp["vel"], inp["edges"], inp["charges"], c["targets"], K, dt, N)[0] for _ in range(2)]
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_grad_accumulates_across_calls_and_frozen_tensors_stay_out():
    D = 2
    a, b = case(D, *SHAPES[0]), case(D, *SHAPES[2])
    m = _model(D, "fused")

    def loss(c):
        i = c["inp"]
        return rollout_loss(m, i["x"].to(DEV), i["vel"].to(DEV), [e.to(DEV) for e in i["edges"]], i["charges"].to(DEV),
                            c["targets"].to(device=DEV, dtype=torch.float32), 1.0, num_nodes=c["num_nodes"])

    def grads():
        return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    loss(a).backward()
    ga = grads()
    assert set(ga) == set(k for k, _ in m.named_parameters())
    m.zero_grad(set_to_none=True)
    loss(b).backward()
    gb = grads()
    m.zero_grad(set_to_none=True)
    loss(a).backward()
    loss(b).backward()                                            # no zero_grad in between
    g2 = grads()
    for k in ga:
        want = ga[k] + gb[k]
        assert float((g2[k] - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-12, k
    frozen = ("gnn.layer_2.message_fn.0.weight", "field_net.wrapper.film_1.modulator.2.weight")
    for f in frozen:
        dict(m.named_parameters())[f].requires_grad_(False)
    m.zero_grad(set_to_none=True)
    loss(a).backward()
    gf = grads()
    assert set(gf) == set(ga) - set(frozen)
    assert all(dict(m.named_parameters())[f].grad is None for f in frozen)
    for k in gf:
        assert torch.equal(gf[k], ga[k]), k


@pytest.mark.parametrize("shape", NARROW)
@pytest.mark.parametrize("D", [2, 3])
def test_narrow_models_through_their_kernel_width_copies(D, shape):
    """hidden_size 20 and 32: the kernels run on zero-padded copies of the GNN parameters, the gradients come back cut to
    the parameters' shapes (held by ``_hold``)."""
    for path in ("fused", "streamed"):
        _check_case(D, shape, path)


def test_graphed_rollout_train_step_matches_eager_steps():
    """One hipGraph of rollout forward + loss + backward through time with 5-tuple args: three replays leave the
    parameters where three eager steps of the same kernels leave them (tolerances of tests/test_gpu_rollout_train.py)."""
    from aether_amd.optim import FusedAdamW
    from aether_amd.training import GraphedRolloutTrainStep
    D = 2
    H, B, N, K, dt, seed = SHAPES[1]
    c = case(D, *SHAPES[1])
    i = c["inp"]
    x, v, q = i["x"].to(DEV), i["vel"].to(DEV), i["charges"].to(DEV)
    edges = [e.to(DEV) for e in i["edges"]]
    tgt = c["targets"].to(device=DEV, dtype=torch.float32)
    m1, m2 = _model(D), _model(D)
    step = GraphedRolloutTrainStep(m1, (x, v, edges, q, N), tgt, dt=dt, lr=1e-3, weight_decay=1e-12, warmup=1)
    opt = FusedAdamW(m2.parameters(), lr=1e-3, weight_decay=1e-12)
    losses = []
    for k in range(4):                                            # the helper's one warm-up step, then three
        opt.zero_grad(set_to_none=True)
        loss = rollout_loss(m2, x, v, edges, q, tgt, dt, num_nodes=N)
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
    """Only checks that return before anything is queued."""
    lib = _lib.load()
    D, K, N = 2, 2, 5
    inp = make_batch(2, N, D, seed=1, device=DEV)
    m = _model(D)
    n, E = inp["x"].shape[0], inp["edges"][0].numel()
    gbuf, ginfo = m.prepare_graph(inp["edges"], n)
    ps, fps = m._rollout_train_params(torch.device(DEV))
    _, _, _, dst, _, (gs, gfs), _ = m._grad_destination()
    nbytes = lib.aether_rollout_dynamic_field_train_workspace_bytes(n, E, D, 64, N, K)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    traj = torch.empty(K, n, D, device=DEV)
    gt = torch.ones(K, n, D, device=DEV)
    gx, gv = torch.empty(n, D, device=DEV), torch.empty(n, D, device=DEV)
    x, v, q = inp["x"], inp["vel"], inp["charges"]
    st = torch.cuda.current_stream().cuda_stream
    other = _lib.AetherGraphInfo(n + 1, E, ginfo.n_groups, ginfo.max_group_nodes, ginfo.max_group_edges, ginfo.reserved)

    def fwd(ps=ps, fps=fps, D=D, H=64, N=N, x=x.data_ptr(), v=v.data_ptr(), q=q.data_ptr(), g=gbuf.data_ptr(), info=ginfo,
            ws=ws.data_ptr(), wsb=nbytes, traj=traj.data_ptr(), K=K, dt=1.0, flags=0):
        return lib.aether_rollout_dynamic_field_train_forward(ps, fps, D, H, n, E, N, x, v, q, g, C.byref(info), ws, wsb, traj,
                                                              K, dt, flags, st)

    def bwd(ps=ps, fps=fps, gs=gs, gfs=gfs, D=D, H=64, N=N, x=x.data_ptr(), v=v.data_ptr(), q=q.data_ptr(), g=gbuf.data_ptr(),
            info=ginfo, ws=ws.data_ptr(), wsb=nbytes, traj=traj.data_ptr(), gt=gt.data_ptr(), gx=gx.data_ptr(),
            gv=gv.data_ptr(), K=K, dt=1.0):
        return lib.aether_rollout_dynamic_field_backward(ps, fps, gs, gfs, D, H, n, E, N, x, v, q, g, C.byref(info), ws, wsb,
                                                         traj, gt, gx, gv, K, dt, st)

    EINVAL, ESPACE = -1, -4
    for call in (fwd, bwd):
        for kw, code in [(dict(ps=None), EINVAL), (dict(fps=None), EINVAL), (dict(x=None), EINVAL), (dict(v=None), EINVAL),
                         (dict(q=None), EINVAL), (dict(g=None), EINVAL), (dict(ws=None), EINVAL), (dict(traj=None), EINVAL),
                         (dict(D=4), EINVAL), (dict(info=other), EINVAL), (dict(K=0), EINVAL), (dict(dt=0.0), EINVAL),
                         (dict(H=128), EINVAL), (dict(H=32), EINVAL), (dict(N=3), EINVAL), (dict(N=0), EINVAL),
                         (dict(wsb=nbytes - 1), ESPACE)]:
            assert call(**kw) == code, (call.__name__, kw)
            assert lib.aether_last_error()
    assert fwd(H=128) == EINVAL and b"64-wide engine only" in lib.aether_last_error()
    assert bwd(gs=None) == EINVAL and bwd(gfs=None) == EINVAL and bwd(gt=None) == EINVAL
    null_dyn = _DynFieldParams.from_buffer_copy(gfs._obj)             # (byref keeps its struct)
    null_dyn.film2_b4 = None
    assert bwd(gfs=C.byref(null_dyn)) == EINVAL
    null_grad = _lib.AetherParams.from_buffer_copy(gs._obj)
    null_grad.out_b6 = None
    assert bwd(gs=C.byref(null_grad)) == EINVAL
    assert fwd(flags=_lib.FLAG_FORCE_FUSED, info=_lib.AetherGraphInfo(n, E, 0, 0, 0, 0)) == EINVAL   # fused asked for, no groups
    # a valid pair after all of them; either input gradient may be left out
    assert fwd() == 0 and bwd() == 0
    full = (gx.clone(), gv.clone(), [d.clone() for d in dst])
    assert fwd() == 0 and bwd(gx=None, gv=None) == 0
    torch.cuda.synchronize()
    _lib.check(lib.aether_check_async_error(), "async")
    assert torch.isfinite(traj).all() and torch.isfinite(full[0]).all() and torch.isfinite(full[1]).all()
    assert all(torch.equal(d, f) for d, f in zip(dst, full[2]))
    assert torch.equal(traj, m.rollout(x, v, inp["edges"], q, K, 1.0, num_nodes=N))


def test_python_error_paths():
    D, N = 2, 5
    inp = make_batch(2, N, D, seed=1, device=DEV)
    args = (inp["x"], inp["vel"], inp["edges"], inp["charges"])
    m = DynamicFieldAether(2 * D, 64, 0.25, D, device=DEV)
    with pytest.raises(RuntimeError):                             # train() with dropout_prob > 0: no per-step masks
        m.differentiable_rollout(*args, 2, num_nodes=N)
    m.eval()
    assert m.differentiable_rollout(*args, 2, num_nodes=N).requires_grad
    with pytest.raises(_lib.AetherHipError, match="not built"):
        m.differentiable_rollout(*args, 2)
    with pytest.raises(ValueError):
        m.differentiable_rollout(*args, 0, num_nodes=N)
    with pytest.raises(ValueError):
        m.differentiable_rollout(*args, 2, num_nodes=3)           # 10 nodes are no multiple of 3
    with pytest.raises(_lib.AetherHipError, match="64-wide engine only"):
        DynamicFieldAether(2 * D, 128, 0.0, D, device=DEV).differentiable_rollout(*args, 2, num_nodes=N)
    traj = m.differentiable_rollout(*args, 2, num_nodes=N)        # the first backward consumes the rollout's workspace
    traj.sum().backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second time"):
        traj.sum().backward()
