"""Buffer contract of the library calls: exact size, no reads before writes ("buffer contract").

Every case runs one operation twice on a fresh module: once with plain allocation (the baseline) and once inside
``guarded_alloc.GuardedAlloc``, where every ``torch.empty`` / ``torch.empty_like`` of the Python layer -- workspaces, graph
views, outputs, gradient destinations -- is exactly as large as requested, filled with 0xFF (NaN / -1) and fenced by 64 KiB
bands, and the inputs sit in ``guarded_copy`` buffers (NaN bands behind floats, zero bands behind indices).  Then

  (a) ``check()``: no byte of any band changed -- nothing wrote outside the buffer it was given;
  (b) the harness did guard something: a workspace of exactly the byte count the family's size function returns, every
      output tensor and, for the state2state modules, the graph view of ``aether_graph_bytes``;
  (c) every result is finite and ``torch.equal`` to the baseline: the kernels are bit-stable, so a difference is a read of
      a word nobody wrote or of something outside the inputs;
  (d) the forward output meets the fp64 oracle at the project's bars (1e-5 scale-relative; equal bits alone would pass if
      both runs were equally wrong).

Out of scope: captured steps (``GraphedTrainStep``, ``torch.cuda.graph``) -- the interposer passes through while the
stream is capturing, the graph's pool serves those allocations.  Buffers that torch's C++ side allocates (``torch.zeros``
gradient buffers and zero fields, ``clone``, operator results) are not guarded either; the ``torch.empty`` sites are.
"""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import load_state_dict, scale_rel_err
from guarded_alloc import BAND, GuardedAlloc, GuardError
from aether_amd import _lib
from aether_amd.nn.state2state._frame import GraphCache
from aether_amd.nn.state2state.aether import Aether
from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
from aether_amd.nn.state2state.locs import LoCS
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O
from oracle import knn_oracle as K

import graph_cases as GC
import locs_restatement as LR

pytestmark = pytest.mark.gpu
TOL = 1e-5           # forward, max|a - b| / max|b| (conftest.scale_rel_err)
STREAMED = _lib.FLAG_FORCE_STREAMED
# The library has no getter for its options: these are the initial values of the g_* globals of csrc/aether_hip.hip
# (g_fused_split, g_fused_waves12, g_graph_build, g_outer_defer_max_edges, g_edge_acc, g_gemm_split, g_fused_backward), the
# values the neighbouring files (test_gpu_graph_build.py, test_gpu_fused_waves12.py, test_gpu_seq2seq.py) restore as well.
DEFAULTS = {"fused_split": 1, "fused_waves12": 1, "graph_build": 1, "fused_backward": 1, "edge_acc": 1,
            "outer_defer_max_edges": 1 << 20, "gemm_split": 1}


@contextlib.contextmanager
def _options(**kv):
    """Library options for the block; each back at its default afterwards."""
    lib = _lib.load()
    try:
        for k, v in kv.items():
            _lib.check(lib.aether_set_option(k.encode(), v), "set_option")
        yield
    finally:
        for k in kv:
            _lib.check(lib.aether_set_option(k.encode(), DEFAULTS[k]), "set_option")


# ---- the two runs and the four assertions ---------------------------------------------------------------------------------
def _map(f, v):
    if torch.is_tensor(v):
        return f(v)
    if isinstance(v, (list, tuple)):
        return type(v)(_map(f, e) for e in v)
    if isinstance(v, dict):
        return {k: _map(f, e) for k, e in v.items()}
    return v


def _cuda(t):
    return t.to("cuda", torch.float32 if t.dtype.is_floating_point else t.dtype).contiguous()


class Run:
    """What one run of a case's body hands back: named results (compared bit for bit), the output tensors and the exact
    byte counts (workspaces, graph views) that must be among the guarded allocations, and the checks against the oracle."""

    def __init__(self):
        self.results, self.outputs, self.exact, self.shapes, self.oracle = {}, {}, [], [], []

    def result(self, name, t, output=False):
        self.results[name] = t.detach()
        if output:
            self.outputs[name] = t.detach()

    def workspace(self, label, nbytes):
        self.exact.append((label, int(nbytes)))

    def allocated(self, label, shape, dtype):
        """An allocation of this shape and dtype (a destination the caller does not get back as it is)."""
        self.shapes.append((label, tuple(shape), dtype))

    def against(self, name, want, tol=TOL):
        self.oracle.append((name, want, tol))


def contract(body, inputs, what=""):
    """``body(inputs on the device) -> Run``, plain and guarded; assertions (a) to (d) of the module docstring."""
    base = body(_map(_cuda, inputs))
    torch.cuda.synchronize()
    g = GuardedAlloc()
    guarded_inputs = _map(lambda t: g.guarded_copy(_cuda(t)), inputs)
    with g:
        got = body(guarded_inputs)
    g.check()                                                                                     # (a)
    n_guarded = len(g.find())
    print(f"[buffer contract] {what}: {n_guarded} guarded allocations, {len(got.results)} results")
    assert n_guarded > 0 and (got.exact or got.outputs or got.shapes), "the case guarded nothing"  # (b)
    sizes = g.sizes()
    for label, nbytes in got.exact:
        assert g.find(nbytes=nbytes, dtype=torch.uint8), (label, nbytes, sorted(set(sizes)))
    for name, t in got.outputs.items():
        rec = g.holds(t)
        assert rec is not None and rec.kind != "input", name
    for label, shape, dtype in got.shapes:
        assert g.find(shape=shape, dtype=dtype), (label, shape, dtype)
    assert base.results.keys() == got.results.keys() and got.results                               # (c)
    for k, v in got.results.items():
        assert torch.isfinite(v).all(), (k, "not finite inside the harness")
        assert torch.isfinite(base.results[k]).all(), (k, "not finite in the baseline")
        assert torch.equal(v, base.results[k]), (k, "differs from the plain run: a read of an unwritten word")
    for name, want, tol in got.oracle:                                                             # (d)
        err = scale_rel_err(got.results[name].cpu(), want)
        assert err <= tol, (name, err)
    return g, got


# ---- negative control -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["below", "above"])
def test_one_byte_written_into_a_band_is_found(side):
    """The harness on device memory: a single byte of a band, written through the raw buffer by a plain torch operation
    (memory this test owns), makes check() raise and name the allocation."""
    g = GuardedAlloc()
    with g:
        torch.empty(3, 7, dtype=torch.float32, device="cuda")
        t = torch.empty(5, 16, dtype=torch.float32, device="cuda")
    g.check()
    rec = g.holds(t)
    assert rec is g.allocations[1] and rec.raw.numel() == 2 * BAND + 320 and torch.isnan(t).all()
    rec.raw[BAND - 9 if side == "below" else BAND + 320 + 40] = 0
    with pytest.raises(GuardError, match=r"allocation #1 .*shape=\(5, 16\).*bytes=320 from tests/test_gpu_buffer_contract\.py:\d+: 1 byte\(s\) of the band " + side) as e:
        g.check()
    assert ("offsets -9..-9 " if side == "below" else "offsets 360..360 ") in str(e.value)


# ---- Aether ---------------------------------------------------------------------------------------------------------------
def _no_edges(inp):
    e = torch.zeros(0, dtype=torch.int64)
    return dict(inp, edges=[e, e.clone()], edge_attr=inp["edge_attr"][:0].clone())


@functools.lru_cache(maxsize=None)
def _aether_inputs(shape, D):
    """The named shapes -> (inputs, does the rollout trainer's protocol cover them: no self loops)."""
    if shape == "multigraph":
        from test_gpu_configs import _random_multigraph_batch
        inp = _random_multigraph_batch(11, D)
        g = torch.Generator().manual_seed(110 + D)
        return dict(inp, target=inp["x"] + 0.1 * torch.randn(inp["x"].shape, generator=g)), False
    if shape == "no_edges":
        return _no_edges({k: v for k, v in make_batch(3, 5, D, seed=40).items() if k != "meta"}), True
    B, N = {"B1N2": (1, 2), "B3N5": (3, 5), "B2N17": (2, 17), "B1N20": (1, 20), "B2N20": (2, 20), "B2N37": (2, 37),
            "B1N6": (1, 6)}[shape]
    return {k: v for k, v in make_batch(B, N, D, seed=40 + N).items() if k != "meta"}, True


def _new_aether(D, H, flags, seed=7):
    torch.manual_seed(seed)
    m = Aether(2 * D, H, 0.0, D, device="cuda")
    m.flags = flags
    return m


@functools.lru_cache(maxsize=None)
def _aether_oracle(shape, D, H):
    """fp64 forward of the module ``_new_aether`` builds, once per (shape, D, width)."""
    torch.manual_seed(7)
    sd = {k: v.detach().double() for k, v in Aether(2 * D, H, 0.0, D, device="cpu").state_dict().items()}
    inp, _ = _aether_inputs(shape, D)
    with torch.no_grad():
        return O.aether_forward(sd, inp["x"].double(), inp["vel"].double(), inp["edges"], inp["edge_attr"].double(),
                                inp["charges"].double())


def _forget_workspaces(m):
    """The next operation sizes and allocates its own workspace (a poisoned one inside the harness)."""
    for o in (m, m.__dict__.get("_engine")):
        if o is not None:
            o._ws = o._last_ws = o._train_ws = o._train_ws_token = None
            o._rollout_train_ws = o._rollout_train_ws_token = None
            o._ws_key = o._wimg_key = None


def _frame_sizes(m, n, E):
    """(graph view, inference workspace, training workspace) bytes of a FrameModule at this shape."""
    lib = _lib.load()
    return (max(lib.aether_graph_bytes(E, n), 256), lib.aether_workspace_bytes_h(n, E, m.num_dims, m._kw, 0),
            lib.aether_workspace_bytes_h(n, E, m.num_dims, m._kw, 1))


def _step_loss(traj, target):
    return ((traj - target.unsqueeze(0)) ** 2).mean()


def _aether_body(D, H, flags, diff_rollout, oracle):
    def body(g):
        r = Run()
        m = _new_aether(D, H, flags)
        n, E = g["x"].shape[0], g["edges"][0].numel()
        gbytes, inf_bytes, train_bytes = _frame_sizes(m, n, E)
        call = lambda x, vel, ea: m(g["h"], x, g["edges"], vel, ea, g["charges"])
        # inference forward
        with torch.no_grad():
            r.result("out", call(g["x"], g["vel"], g["edge_attr"]), output=True)
        r.workspace("graph view", gbytes)
        r.workspace("inference workspace", inf_bytes)
        if oracle is not None:
            r.against("out", oracle)
        # training forward + backward: all 47 parameter gradients
        _forget_workspaces(m)
        out = call(g["x"], g["vel"], g["edge_attr"])
        torch.nn.functional.mse_loss(out, g["target"]).backward()
        r.result("train.out", out, output=True)
        grads = {k: p.grad for k, p in m.named_parameters()}
        assert len(grads) == 47 and all(v is not None for v in grads.values())
        for k, v in grads.items():
            r.result("grad." + k, v.clone())
        r.workspace("training workspace", train_bytes)
        # the input gradients
        _forget_workspaces(m)
        m.zero_grad(set_to_none=True)
        leaves = [g[k].clone().requires_grad_(True) for k in ("x", "vel", "edge_attr")]
        out = call(*leaves)
        torch.nn.functional.mse_loss(out, g["target"]).backward()
        for k, t in zip(("x", "vel", "edge_attr"), leaves):
            r.result("dinput." + k, t.grad)
        for k, p in m.named_parameters():
            r.result("grad2." + k, p.grad.clone())
        r.allocated("edge_attr gradient", (E, 2), torch.float32)
        # 3-step device rollout
        _forget_workspaces(m)
        r.result("rollout", m.rollout(g["x"], g["vel"], g["edges"], g["charges"], 3, 0.5), output=True)
        # 2-step training rollout, parameters and initial state
        if diff_rollout:
            _forget_workspaces(m)
            m.zero_grad(set_to_none=True)
            x0, v0 = g["x"].clone().requires_grad_(True), g["vel"].clone().requires_grad_(True)
            traj = m.differentiable_rollout(x0, v0, g["edges"], g["charges"], 2, 0.5)
            _step_loss(traj, g["target"]).backward()
            r.result("train_rollout", traj, output=True)
            r.result("train_rollout.dx0", x0.grad)
            r.result("train_rollout.dvel0", v0.grad)
            for k, p in m.named_parameters():
                r.result("train_rollout.grad." + k, p.grad.clone())
            r.workspace("rollout training workspace",
                        max(_lib.load().aether_rollout_train_workspace_bytes(n, E, D, m._kw, 2), 256))
        return r
    return body


WIDTHS = {"fused64": (64, 0), "streamed64": (64, STREAMED), "narrow20": (20, 0), "wide96": (96, 0)}
AETHER_SHAPES = ["B1N2", "B3N5", "B2N17", "B1N20", "B2N37", "multigraph", "no_edges"]


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("width", list(WIDTHS))
@pytest.mark.parametrize("shape", AETHER_SHAPES)
def test_aether(shape, width, D):
    """Inference forward, training forward + backward (47 parameter gradients), input gradients, a 3-step rollout and,
    at width 64 on graphs without self loops, a 2-step differentiable_rollout with backward."""
    H, flags = WIDTHS[width]
    inp, trainable = _aether_inputs(shape, D)
    contract(_aether_body(D, H, flags, trainable and H == 64, _aether_oracle(shape, D, H)), inp, f"aether {shape} {width} D{D}")


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("shape,options", [("B1N20", dict(fused_waves12=0)), ("B2N20", dict(fused_split=0)),
                                           ("B2N17", dict(fused_waves12=0)), ("B2N20", {})])
def test_aether_fused_layouts(shape, options, D):
    """The group layouts of the fused kernels at width 64: B1N20 split on the 8-wave kernel (``fused_waves12`` 0; the
    12-wave kernel runs it in test_aether), B2N20 unsplit (three rounds) and split."""
    inp, _ = _aether_inputs(shape, D)
    with _options(**options):
        contract(_aether_body(D, 64, 0, True, _aether_oracle(shape, D, 64)), inp, f"aether {shape} {options} D{D}")


@pytest.mark.parametrize("edge_acc", [3, 0])
@pytest.mark.parametrize("shape,D", [("B2N37", 2), ("B2N37", 3), ("B1N6", 2), ("B1N6", 3)])
def test_aether_training_layout_without_deferral(shape, D, edge_acc):
    """``outer_defer_max_edges`` 0 with ``edge_acc`` on and off: the layers share one set of backward operands, and with
    edge_acc the row tensors shrink to 64 floats."""
    inp, _ = _aether_inputs(shape, D)
    with _options(outer_defer_max_edges=0, edge_acc=edge_acc):
        for width in ("fused64", "streamed64"):
            H, flags = WIDTHS[width]
            contract(_aether_body(D, H, flags, True, _aether_oracle(shape, D, H)), inp,
                     f"aether {shape} {width} D{D} defer 0 edge_acc {edge_acc}")


# ---- leftovers: one module, changing shapes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["fused64", "streamed64", "narrow20", "wide96"])
@pytest.mark.parametrize("mode", ["inference", "training"])
def test_aether_leftovers_of_another_shape_are_not_read(mode, width):
    """One module runs B2N20, B3N5, then B2N20 again after an in-place weight update, inside the harness: every call is a
    fresh module's result on the same weights, bit for bit (workspaces, graph cache and weight images are reused)."""
    D = 2
    H, flags = WIDTHS[width]
    seq = ["B2N20", "B3N5", "B2N20"]

    def step(m, g):
        if mode == "inference":
            with torch.no_grad():
                return {"out": m(g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"], g["charges"])}
        m.zero_grad(set_to_none=True)
        out = m(g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"], g["charges"])
        torch.nn.functional.mse_loss(out, g["target"]).backward()
        res = {"out": out.detach()}
        res.update({"grad." + k: p.grad.clone() for k, p in m.named_parameters()})
        return res

    def bump(m):
        with torch.no_grad():
            for i, p in enumerate(m.parameters()):
                p.add_(1e-3 * ((i % 3) - 1))

    guard = GuardedAlloc()
    m = _new_aether(D, H, flags)
    got, marks = [], []
    with guard:
        for i, shape in enumerate(seq):
            if i == 2:
                bump(m)
            got.append(step(m, _map(lambda t: guard.guarded_copy(_cuda(t)), _aether_inputs(shape, D)[0])))
            marks.append(len(guard.allocations))
    guard.check()
    # the harness held what the sequence reuses: the first call's exact-size workspace (the larger shape's; the second call
    # fits into it), one graph view per shape, every output -- and the third call took no new workspace or view at all
    keep = mode == "training"
    sizes = {}
    for shape in set(seq):
        x, edges = _aether_inputs(shape, D)[0]["x"], _aether_inputs(shape, D)[0]["edges"]
        gbytes, inf_bytes, train_bytes = _frame_sizes(m, x.shape[0], edges[0].numel())
        sizes[shape] = (gbytes, train_bytes if keep else inf_bytes)
    first = guard.allocations[:marks[0]]
    ws_big = sizes["B2N20"][1]
    assert sizes["B3N5"][1] < ws_big
    assert [a for a in first if a.kind != "input" and a.nbytes == ws_big and a.dtype == torch.uint8], "workspace of call 1"
    assert len(guard.find(nbytes=ws_big, dtype=torch.uint8)) == 1, "the workspace was allocated once and reused"
    for shape in set(seq):
        assert len(guard.find(nbytes=sizes[shape][0], dtype=torch.uint8)) == 1, ("graph view", shape)
    for i in range(3):
        rec = guard.holds(got[i]["out"])
        assert rec is not None and rec.kind != "input", i
    third = [a for a in guard.allocations[marks[1]:] if a.kind != "input"]
    assert third and not [a for a in third if a.dtype == torch.uint8], "the third call reuses the poisoned workspace and view"
    for i, shape in enumerate(seq):
        fresh = _new_aether(D, H, flags)
        if i == 2:
            bump(fresh)
        want = step(fresh, _map(_cuda, _aether_inputs(shape, D)[0]))
        assert want.keys() == got[i].keys()
        for k in want:
            assert torch.isfinite(got[i][k]).all(), (i, shape, k)
            assert torch.equal(got[i][k], want[k]), (i, shape, k)


# ---- graph view, both builders ------------------------------------------------------------------------------------------------
GRAPHS = ["h_empty", "a_B1N2", "b_B3N5", "c_B1N20", "d_multigraph", "f_knn", "g_star_cap_plus_1", "g_star_cap"]


@functools.lru_cache(maxsize=None)
def _graph_cases():
    from test_gpu_graph_build import _graphs
    return _graphs()


@pytest.mark.parametrize("builder", [1, 0], ids=["counting", "sorting"])
@pytest.mark.parametrize("name", GRAPHS)
def test_graph_view(name, builder):
    """The view of ``aether_graph_build_counting`` (option ``graph_build`` 1) and of the sorting builder (0) in a buffer of
    exactly ``aether_graph_bytes``: info, receiver order, and what reads the regions without an accessor -- an Aether
    forward and backward on the view, against the oracle."""
    from test_gpu_graph_build import INFO_FIELDS, _state
    send, recv, n = _graph_cases()[name]
    D = 2
    st = _state(n, send, recv, D, seed=31)
    inp = dict(st, edges=[send, recv])
    sd = load_state_dict(D)
    with torch.no_grad():
        want = O.aether_forward({k: v.double() for k, v in sd.items()}, st["x"].double(), st["vel"].double(), [send, recv],
                                st["edge_attr"].double(), st["charges"].double())

    def body(g):
        r = Run()
        s, rc = g["edges"]
        E = s.numel()
        lib = _lib.load()
        gbytes = max(lib.aether_graph_bytes(E, n), 256)
        buf, info = GraphCache().get(s, rc, n)
        assert buf.numel() == gbytes
        r.workspace("graph view", gbytes)
        r.result("info", torch.tensor([getattr(info, f) for f in INFO_FIELDS], dtype=torch.float64))
        assert lib.aether_graph_matches(s.data_ptr(), rc.data_ptr(), E, n, buf.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream) == 1
        m = Aether(2 * D, 64, 0.0, D, device="cuda")
        m.load_state_dict(sd)
        if E:
            perm = m.graph_perm(g["edges"], n)                    # (its own cache: the view is built a second time)
            assert torch.equal(perm.cpu(), torch.argsort(rc.cpu(), stable=True))
            r.result("perm", perm)
            r.allocated("receiver order", (E,), torch.int32)
        leaves = [g[k].clone().requires_grad_(True) for k in ("x", "vel", "edge_attr")]
        out = m(g["h"], leaves[0], g["edges"], leaves[1], leaves[2], g["charges"])
        torch.nn.functional.mse_loss(out, g["target"]).backward()
        r.result("out", out, output=True)
        r.against("out", want)
        for k, p in m.named_parameters():
            r.result("grad." + k, p.grad.clone())
        for i, t in enumerate(leaves):
            r.result("dinput.%d" % i, t.grad)
        return r

    with _options(graph_build=builder):
        contract(body, inp, f"graph view {name} builder {builder}")


# ---- LoCS, DynamicFieldAether, EGNN-Aether, ClofNet -------------------------------------------------------------------------------
def _gnn_inputs(shape, D=3):
    """B3N5 (the runner's batch) and graph_cases.random_multigraph(2, 6, seed, self_loop=True) -> (inputs, objects per graph)."""
    if shape == "B3N5":
        import egnn_restatement as ER
        return ER.runner_batch(3, 5, 21, dtype=torch.float64), 5
    return GC.random_multigraph(2, 6, 22, self_loop=True), 6


def _frame_body(make, call, rollout, oracle, num_nodes=None, train_rollout=False):
    """LoCS / DynamicFieldAether on Aether's kernels: forward, backward, 3-step rollout (+ the 2-step training rollout)."""
    def body(g):
        r = Run()
        m = make()
        n, E = g["x"].shape[0], g["edges"][0].numel()
        gbytes, inf_bytes, train_bytes = _frame_sizes(m, n, E)
        with torch.no_grad():
            r.result("out", call(m, g), output=True)
        r.workspace("graph view", gbytes)
        r.workspace("inference workspace", inf_bytes)
        r.against("out", oracle(m, g))
        _forget_workspaces(m)
        out = call(m, g)
        torch.nn.functional.mse_loss(out, g["target"]).backward()
        r.result("train.out", out, output=True)
        r.workspace("training workspace", train_bytes)
        for k, p in m.named_parameters():
            r.result("grad." + k, p.grad.clone())
        _forget_workspaces(m)
        r.result("rollout", rollout(m, g, 3), output=True)
        if train_rollout:
            _forget_workspaces(m)
            m.zero_grad(set_to_none=True)
            traj = m.differentiable_rollout(g["x"], g["vel"], g["edges"], g["charges"], 2, 0.5, num_nodes=num_nodes)
            _step_loss(traj, g["target"]).backward()
            r.result("train_rollout", traj, output=True)
            for k, p in m.named_parameters():
                r.result("train_rollout.grad." + k, p.grad.clone())
            r.workspace("rollout training workspace", max(_lib.load().aether_rollout_dynamic_field_train_workspace_bytes(
                n, E, m.num_dims, m._kw, num_nodes, 2), 256))
        return r
    return body


def _sd64(m):
    return {k: v.detach().cpu().double() for k, v in m.state_dict().items()}


def _cpu64(g, *keys):
    return [g[k].detach().cpu().double() for k in keys]


@pytest.mark.parametrize("flags", [0, STREAMED], ids=["default", "streamed"])
@pytest.mark.parametrize("shape", ["B3N5", "multigraph"])
def test_locs(shape, flags):
    inp, _ = _gnn_inputs(shape)

    def make():
        torch.manual_seed(5)
        m = LoCS(6, 64, 0.0, 3, device="cuda")
        m.flags = flags
        return m

    def oracle(m, g):
        x, vel, ea = _cpu64(g, "x", "vel", "edge_attr")
        with torch.no_grad():
            return LR.forward(_sd64(m), x, vel, [e.cpu() for e in g["edges"]], ea, None)

    contract(_frame_body(make, lambda m, g: m(g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"]),
                         lambda m, g, k: m.rollout(g["x"], g["vel"], g["edges"], g["charges"], k, 0.5), oracle),
             inp, f"locs {shape} flags {flags}")


@pytest.mark.parametrize("H,flags", [(64, 0), (64, STREAMED), (20, 0)], ids=["default", "streamed", "narrow20"])
@pytest.mark.parametrize("shape", ["B3N5", "multigraph"])
def test_dynamic_field_aether(shape, H, flags):
    """With ``num_nodes``; hidden 20 runs on zero-padded copies of the GNN parameters.  On the runner's batch also the
    input gradients (through the GNN and through the latent field) and the 2-step training rollout (the multigraph's
    self loop has no distance derivative in the rollout protocol)."""
    inp, per = _gnn_inputs(shape)

    def make():
        torch.manual_seed(6)
        m = DynamicFieldAether(6, H, 0.0, 3, device="cuda")
        m.flags = flags
        return m

    def oracle(m, g):
        x, vel, ea, q = _cpu64(g, "x", "vel", "edge_attr", "charges")
        with torch.no_grad():
            return O.dynamic_field_aether_forward(_sd64(m), x, vel, [e.cpu() for e in g["edges"]], ea, q, per)

    def body(g):
        r = _frame_body(make, lambda m, g: m(None, g["x"], g["edges"], g["vel"], g["edge_attr"], g["charges"], per),
                        lambda m, g, k: m.rollout(g["x"], g["vel"], g["edges"], g["charges"], k, 0.5, num_nodes=per),
                        oracle, num_nodes=per, train_rollout=shape == "B3N5")(g)
        n, D = g["x"].shape
        r.allocated("latent field", (n, D), torch.float32)
        r.workspace("field backward workspace", _lib.load().aether_dynamic_field_backward_workspace_bytes(D, n // per))
        if shape == "B3N5":
            m = make()
            leaves = [g[k].clone().requires_grad_(True) for k in ("x", "vel", "edge_attr")]
            out = m(None, leaves[0], g["edges"], leaves[1], leaves[2], g["charges"], per)
            torch.nn.functional.mse_loss(out, g["target"]).backward()
            for k, t in zip(("x", "vel", "edge_attr"), leaves):
                r.result("dinput." + k, t.grad)
            r.allocated("gradient through the latent field", (n, 2 * D), torch.float32)
        return r

    contract(body, inp, f"dynamic field {shape} H{H} flags {flags}")


def _paramgrad_body(K, cfg, per):
    """EGNN-Aether / ClofNet: forward, backward and a 3-step device rollout."""
    from gnn_shape_checks import cast, state64

    def body(g):
        r = Run()
        m = K.build(cfg, "cuda")
        n, E = g["x"].shape[0], g["edges"][0].numel()
        lib = _lib.load()
        a, kw = K.args(g, cfg)
        with torch.no_grad():
            r.result("out", m(*a, **kw), output=True)
        r.workspace("graph view", max(lib.aether_graph_bytes(E, n), 256))
        r.workspace("inference workspace", max(m._workspace_bytes(n, E, False), 256))
        host = {k: ([e.cpu() for e in v] if k == "edges" else v.detach().cpu()) for k, v in g.items()}
        r.against("out", K.restate(state64(m), cast(host, torch.float64), cfg)[0][0].detach())
        m._ws = None
        out = m(*a, **kw)
        torch.nn.functional.mse_loss(out, g["target"]).backward()
        r.result("train.out", out, output=True)
        r.workspace("training workspace", max(m._workspace_bytes(n, E, True), 256))
        dead = K.dead(m)
        for k, p in m.named_parameters():
            assert (p.grad is None) == (k in dead), k
            if p.grad is not None:
                r.result("grad." + k, p.grad.clone())
        extra = dict(n_nodes=per) if "n_nodes" in kw else {}
        r.result("rollout", m.rollout(g["x"], g["vel"], g["edges"], g["charges"], 3, 0.5, **extra), output=True)
        r.workspace("rollout workspace", max(m._entry("rollout_workspace_bytes")(*m._sizes(), n, E), 256))
        return r
    return body


@pytest.mark.parametrize("shape", ["B3N5", "multigraph"])
@pytest.mark.parametrize("model", ["egnn_aether", "clof_vel", "clof_vel_gbf"])
def test_egnn_aether_and_clofnet(model, shape):
    """(the layers run without norm_diff on the multigraph: its self loop has no normalised difference)"""
    import gnn_shape_checks as S
    K = S.Egnn if model == "egnn_aether" else S.Clof
    inp, per = _gnn_inputs(shape)
    cfg = K.cfg(model, 64, 3, 210, per, norm_diff=shape == "B3N5")
    contract(_paramgrad_body(K, cfg, per), inp, f"{model} {shape}")


# ---- kNN ----------------------------------------------------------------------------------------------------------------
def _knn_body(k):
    from aether_amd.knn import knn_edges

    def body(g):
        r = Run()
        x, masks = g["x"], g["masks"]
        send, recv, num = knn_edges(x, masks, k=k)
        r.result("send", send)
        r.result("recv", recv)
        r.result("num", num)
        N = x.shape[-2]
        S = x.numel() // (N * x.shape[-1])
        kk = min(k, N - 1)
        if kk >= 1:
            r.workspace("kNN workspace", _lib.load().aether_knn_workspace_bytes(S, N, kk))
            r.allocated("send / recv", (S * N * kk,), torch.int64)
        else:
            r.allocated("empty edge list", (0,), torch.int64)
        ws, wr, wn = K.knn_edges(x.cpu().numpy(), masks.cpu().numpy(), k)
        assert np.array_equal(send.cpu().numpy(), ws) and np.array_equal(recv.cpu().numpy(), wr)
        assert np.array_equal(num.cpu().numpy().reshape(-1), np.asarray(wn).reshape(-1))
        return r
    return body


@pytest.mark.parametrize("lattice", [False, True], ids=["random", "lattice"])
@pytest.mark.parametrize("S,N,k,p", [(5, 12, 1, 0.8), (2, 17, 16, 1.0), (3, 300, 10, 0.9), (1100, 3, 10, 0.7)])
def test_knn(S, N, k, p, lattice):
    """k = 1, the largest k, several passes per thread, and more scenes (1,100) than the scan kernel has threads; random
    positions and a coarse lattice with many exactly equal distances.  The index lists equal the oracle's."""
    g = torch.Generator().manual_seed(S * 1000 + N)
    x = torch.randn(S, N, 4, generator=g) * 20.0
    m = (torch.rand(S, N, generator=g) < p).float()
    if lattice:
        x = torch.round(x / 8.0)
    contract(_knn_body(k), dict(x=x, masks=m), f"knn S{S} N{N} k{k} lattice {lattice}")


@pytest.mark.parametrize("case", ["one_slot", "two_slots", "three_of_twelve"])
def test_knn_tiny_scenes(case):
    """The scenes of test_gpu_knn.py::test_knn_tiny_scenes: one object slot (k = min(10, 0) = 0: no launch, empty lists),
    two slots, and k larger than the number of present objects."""
    g = torch.Generator().manual_seed(3)
    if case == "one_slot":
        x, m = torch.randn(3, 4, 1, 2, generator=g), torch.ones(3, 4, 1)
    elif case == "two_slots":
        x, m = torch.randn(2, 3, 2, 2, generator=g), torch.ones(2, 3, 2)
        m[1, 2, 0] = 0
    else:
        x, m = torch.randn(1, 1, 12, 3, generator=g), torch.zeros(1, 1, 12)
        m[..., [1, 4, 9]] = 1
    contract(_knn_body(10), dict(x=x, masks=m), f"knn {case}")


# ---- seq2seq: the modules --------------------------------------------------------------------------------------------------
S2S_TOL = 2 * TOL    # tests/test_gpu_s2s_dynfield_rollout.py: wherever the FiLM field is involved


@pytest.mark.parametrize("D", [2, 3])
def test_s2s_field_query_at_a_ragged_point_count(D):
    from conftest import load_s2s_field
    from aether_amd.nn.seq2seq.field import FieldQuery
    from oracle import seq2seq_oracle as S
    d, sd = load_s2s_field(D)
    hidden = int(d["hidden"])
    x = torch.randn(63, 2 * D, generator=torch.Generator().manual_seed(5)) * 2.0        # 63 points: three tiles and 15 rows

    def body(g):
        r = Run()
        m = FieldQuery(D, hidden, 1.0, device="cuda")
        m.load_state_dict(sd, strict=True)
        field, _ = m(g["x"])
        r.result("field", field, output=True)
        r.against("field", S.predict_field(sd, x, D))
        r.workspace("field workspace", _lib.load().aether_s2s_field_workspace_bytes(63, hidden))
        return r

    contract(body, dict(x=x), f"s2s field query D{D}")


@pytest.mark.parametrize("D,B,N,rep", [(2, 7, 5, "cart"), (3, 1, 2, "polar"), (3, 3, 7, "cart")])
def test_s2s_localizer(D, B, N, rep):
    from aether_amd.nn.seq2seq.localizer import AugmentedLocalizer
    from oracle import seq2seq_oracle as S
    x = torch.randn(B, N, 3 * D, generator=torch.Generator().manual_seed(11))
    x[..., :D] *= 3.0
    wants = S.augmented_localizer(x, D == 3, rep)
    names = ("rel_feat", "Rinv", "edge_attr", "edge_pos")

    def body(g):
        r = Run()
        loc = AugmentedLocalizer(N, use_3d=D == 3, pos_representation=rep)
        for name, got, want in zip(names, loc(g["x"]), wants):
            r.result(name, got, output=True)
            r.against(name, want)
        return r

    contract(body, dict(x=x), f"s2s localizer D{D} B{B} N{N}")


@pytest.mark.parametrize("D", [2, 3])
def test_s2s_decoder_step_from_its_fixture(D):
    from conftest import load_s2s_decoder
    from aether_amd.nn.seq2seq.decoder import RecurrentDecoder
    d, sd, params = load_s2s_decoder(D)
    t = lambda k: torch.from_numpy(d[k])
    inp = dict(inputs=t("in.inputs"), hidden=t("in.hidden"), hard=t("in.edges_hard"), soft=t("in.edges_soft"), field=t("in.field"))

    def body(g):
        r = Run()
        dec = RecurrentDecoder(params, device="cuda")
        dec.load_state_dict(sd)
        B, N = g["inputs"].shape[:2]
        for name in ("hard", "soft"):
            dec._cache.pop("ws", None)
            out, hid = dec(g["inputs"], g["hidden"], g[name], g["field"])
            r.result(name + ".outputs", out, output=True)
            r.result(name + ".hidden", hid, output=True)
            r.against(name + ".outputs", t(f"ref.{name}.outputs"))
            r.against(name + ".hidden", t(f"ref.{name}.hidden"))
        r.workspace("decoder workspace", _lib.load().aether_s2s_decoder_workspace_bytes(
            D, int(d["hidden_size"]), B * N, B * N * (N - 1)))
        return r

    contract(body, inp, f"s2s decoder step D{D}")


@pytest.mark.parametrize("D", [2, 3])
def test_s2s_prior_step_from_its_fixture(D):
    from conftest import load_s2s_prior
    from aether_amd.nn.seq2seq.encoder import Encoder
    d, sd, params = load_s2s_prior(D)
    t = lambda k: torch.from_numpy(d[k])
    inp = dict(inputs=t("in.inputs"), h0=t("in.h0"), c0=t("in.c0"), field=t("in.field"))

    def body(g):
        r = Run()
        enc = Encoder(params, device="cuda").eval()
        enc.load_state_dict(sd)
        logits, (h1, c1) = enc.single_step_forward(g["inputs"], (g["h0"], g["c0"]), g["field"])
        for name, got in (("logits", logits), ("h1", h1), ("c1", c1)):
            r.result(name, got, output=True)
            r.against(name, t("ref." + name))
        B, N = g["inputs"].shape[:2]
        r.workspace("prior workspace", _lib.load().aether_s2s_prior_workspace_bytes(
            D, enc.hidden_size, enc.rnn_hidden_size, enc._param_struct()[2], B * N, B * N * (N - 1)))
        return r

    contract(body, inp, f"s2s prior step D{D}")


def test_s2s_encoder_forward_from_its_fixture():
    """Encoder.forward over the whole sequence (edge features of every frame, the filter GEMM, both LSTMs) against the
    reference's own prior / posterior logits and final prior state."""
    from conftest import load_s2s_loss
    c, model, params = load_s2s_loss("gaussian_norm")
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    inp = dict(inputs=c["inputs"][:, :-1].contiguous(), field=c["field"])

    def body(g):
        from aether_amd.nn.seq2seq.aether import Aether
        r = Run()
        m = Aether(params, device=None).eval()
        m.load_state_dict(sd)
        m = m.cuda()
        prior, post, (h, cc) = m.encoder(g["inputs"], g["field"])
        r.result("prior", prior)
        r.result("posterior", post)
        r.result("state.h", h.reshape(c["state.h"].shape))
        r.result("state.c", cc.reshape(c["state.c"].shape))
        for k in ("prior", "posterior", "state.h", "state.c"):
            r.against(k, c[k])
        B, T, N = g["inputs"].shape[:3]
        r.allocated("edge features of every frame", (T, B * N * (N - 1), params["encoder_hidden"]), torch.float32)
        return r

    contract(body, inp, "s2s encoder forward")


@pytest.mark.parametrize("D,K", [(2, 2), (3, 3)])
def test_s2s_markov_decoder_step_from_its_fixture(D, K):
    import os
    from conftest import GOLDEN
    from test_gpu_s2s_markov import _decoder
    d = np.load(os.path.join(GOLDEN, f"s2s_markov_decoder_D{D}.npz"))
    H, N = int(d["hidden_size"]), int(d["num_vars"])
    t = lambda k: torch.from_numpy(d[k])
    inp = dict(inputs=t("in.inputs"), field=t("in.field"), hard=t(f"K{K}.in.edges_hard"), soft=t(f"K{K}.in.edges_soft"))

    def body(g):
        r = Run()
        dec = _decoder(D, N, H, K, K == 3, int(d["seed"]))
        B = g["inputs"].shape[0]
        for kind in ("hard", "soft"):
            dec._cache.pop("ws", None)
            out, hid = dec(g["inputs"], None, g[kind], g["field"])
            assert hid is None
            r.result(kind, out, output=True)
            r.against(kind, t(f"K{K}.ref.{kind}.outputs"))
        r.workspace("Markov decoder workspace", _lib.load().aether_s2s_markov_decoder_workspace_bytes(D, H, B * N, B * N * (N - 1)))
        return r

    contract(body, inp, f"s2s markov decoder step D{D} K{K}")


def test_s2s_dynamic_field_summary_and_film_query():
    """The graph summary (GRU + attention pooling over 10 frames) and the standalone FiLM field query of the seq2seq
    DynamicFieldAether, graphs of 7 rows."""
    from aether_amd.nn.seq2seq.dynamic_field_aether import DynamicFieldAether
    from oracle import seq2seq_oracle as S
    D, B, N, T, H, GH, MH = 2, 3, 7, 10, 64, 32, 48
    params = {"num_vars": N, "num_edge_types": 2, "encoder_dropout": 0.0, "encoder_hidden": H, "encoder_rnn_hidden": 32,
              "encoder_rnn_type": "lstm", "input_size": 2 * D, "encoder_mlp_num_layers": 3, "encoder_mlp_hidden": 32,
              "prior_num_layers": 3, "prior_hidden_size": 32, "use_3d": D == 3, "pos_representation": "cart",
              "gpu": True, "decoder_hidden": H, "skip_first": False, "decoder_dropout": 0.0, "gumbel_temp": 0.5,
              "graph_hidden": GH, "mlp_hidden": MH, "field": None}
    gen = torch.Generator().manual_seed(71)
    x = torch.randn(B, N, T, 2 * D, generator=gen)
    x1 = torch.randn(B, N, 2 * D, generator=gen)

    def body(g):
        r = Run()
        torch.manual_seed(72)
        m = DynamicFieldAether(params, device="cuda").eval()
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        gp = {k[len("graph_pooler."):]: v for k, v in sd.items() if k.startswith("graph_pooler.")}
        want = S.graph_summary(gp, x)
        summary = m.graph_pooler(g["x"])
        r.result("summary", summary, output=True)
        r.against("summary", want)
        lib = _lib.load()
        r.workspace("summary workspace", lib.aether_s2s_graph_summary_workspace_bytes(B, N, T, 2 * D, m.graph_pooler.hidden_size))
        field, _ = m.predict_field(g["x1"], summary)
        r.result("field", field)
        r.against("field", S.film_field(sd, x1, want, D), S2S_TOL)
        r.workspace("FiLM field workspace", lib.aether_s2s_film_field_workspace_bytes(B * N, m.hidden_size, m.mlp_hidden))
        r.allocated("FiLM modulation", (lib.aether_s2s_film_modulation_bytes(B, m.mlp_hidden) // 4,), torch.float32)
        return r

    contract(body, dict(x=x, x1=x1), "s2s dynamic field summary + FiLM query")


# ---- seq2seq: the fused step and the device rollout -------------------------------------------------------------------------
def _s2s_sizes(m, B, N):
    """(plan bytes, step workspace bytes) of a seq2seq model's fused step, from the entries the module itself calls."""
    lib = _lib.load()
    hook = m._field_hook()
    D, he, hd, R, K = m._step_sizes()
    pe, n_layers, prior_hidden = m.encoder._param_struct(with_image=False)
    pd = m.decoder._param_struct()
    both = hook.decoders(m.decoder, pd) if hook.entries is not None else ()
    E1 = m.encoder.recv_edges.shape[0]
    return (getattr(lib, m._entries(hook)[0])(*both, D, he, hd, R, n_layers, prior_hidden, K, *hook.plan_tail),
            getattr(lib, m._entries(hook)[2])(D, he, hd, R, prior_hidden, K, *hook.ws_tail, B * N, B * E1))


def _s2s_oracle(sd64, D, K, skip, rep, layers, markov, x, dh, hc, u, edges, tau=0.5):
    """One step in fp64 on the sample the step drew: field -> prior step -> decoder step; also the oracle's own sample and
    the gap between its two largest Gumbel scores (tests/test_gpu_s2s_dynfield_rollout.py::_oracle_step)."""
    from oracle import seq2seq_oracle as S
    from test_gpu_s2s_dynfield_rollout import _frames_as_fp32, _sub
    from test_s2s_markov import restate
    x, hc, u = x.double(), tuple(v.double() for v in hc), u.double()
    field = S.predict_field(sd64, x, D)
    with _frames_as_fp32(D == 3):
        logits, hc1 = S.prior_step(_sub(sd64, "encoder."), x, hc, field, D == 3, rep, layers)
    z = S.gumbel_hard(logits.reshape(-1, K), u.reshape(-1, K), tau).view(logits.shape)
    top = ((logits - torch.log(1e-10 - torch.log(u + 1e-10))) / tau).topk(2, dim=-1).values if K > 1 else None
    gap = None if top is None else top[..., 0] - top[..., 1]
    dec = _sub(sd64, "decoder.")
    if markov:
        out, dh1 = restate(dec, x, edges.double(), field, D == 3, skip, frames_dtype=torch.float32 if D == 3 else None), None
    else:
        with _frames_as_fp32(D == 3):
            out, dh1 = S.decoder_step(dec, x, dh.double(), edges.double(), field, D == 3, skip)
    return out, dh1, hc1, z, gap


def _s2s_state(m, B, N, seed, steps=3, empty_type=False):
    g = torch.Generator().manual_seed(seed)
    D, he, hd, R, K = m._step_sizes()
    E = N * (N - 1)
    inp = dict(x=torch.randn(B, N, 2 * D, generator=g), dh=torch.randn(B, N, hd, generator=g) * 0.3,
               h=torch.randn(B, E, R, generator=g) * 0.3, c=torch.randn(B, E, R, generator=g) * 0.3,
               u=torch.rand(B, E, K, generator=g), U=torch.rand(steps, B, E, K, generator=g))
    if empty_type:           # every edge samples type 0: the other type's row list is empty
        inp["u"][..., 0], inp["u"][..., 1] = 1.0 - 1e-7, 1e-7
        inp["U"][..., 0], inp["U"][..., 1] = 1.0 - 1e-7, 1e-7
    return inp


def _s2s_body(make, B, N, layers, steps=3, oracle=True, rollout=True):
    def body(g):
        r = Run()
        m = make()
        markov = not m.decoder._has_state
        D, he, hd, R, K = m._step_sizes()
        plan_bytes, ws_bytes = _s2s_sizes(m, B, N)
        out, dh1, (h1, c1), edges = m._fused_step(g["x"], g["dh"], (g["h"], g["c"]), g["u"])
        for name, t in (("out", out), ("dh", dh1), ("h", h1), ("c", c1), ("edges", edges)):
            if t is not None:
                r.result(name, t, output=True)
        assert (dh1 is None) == markov
        r.workspace("plan", plan_bytes)
        r.workspace("step workspace", ws_bytes)
        if oracle:
            sd64 = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
            cpu = lambda t: t.detach().cpu()
            w_out, w_dh, (wh, wc), z, gap = _s2s_oracle(
                sd64, D, K, m.decoder.skip_first_edge_type, m.encoder.pos_representation, layers, markov, cpu(g["x"]),
                cpu(g["dh"]), (cpu(g["h"]), cpu(g["c"])), cpu(g["u"]), cpu(edges))
            r.against("out", w_out)
            r.against("h", wh)
            r.against("c", wc)
            if w_dh is not None:
                r.against("dh", w_dh)
            if gap is not None:      # the sample equals the oracle's wherever rounding cannot move it
                clear = gap > 1e-3
                assert clear.float().mean() > 0.9
                assert torch.equal(cpu(edges).argmax(-1)[clear], z.argmax(-1)[clear])
        if rollout:
            m.__dict__["_step_ws"] = None
            preds, e, (dh_end, (h_end, c_end)) = m._fused_rollout(None, g["x"], g["dh"], (g["h"], g["c"]), steps, g["U"], True)
            r.result("rollout", preds)
            r.result("rollout.edges", e)
            r.result("rollout.h", h_end)
            r.result("rollout.c", c_end)
            if dh_end is not None:
                r.result("rollout.dh", dh_end)
            E1 = m.encoder.recv_edges.shape[0]
            r.allocated("rollout predictions", (steps, B, N, 2 * D), torch.float32)
            r.allocated("rollout edges", (steps, B, E1, K), torch.float32)
        return r
    return body


@pytest.mark.parametrize("decoder", ["recurrent", "markov"])
@pytest.mark.parametrize("D,N,B,K,skip_first", [(2, 5, 7, 2, False), (3, 4, 5, 3, True)])
def test_s2s_fused_step_and_rollout(D, N, B, K, skip_first, decoder):
    from test_gpu_s2s_markov import _model as markov_model
    from test_gpu_seq2seq import _s2s_model
    layers = 3
    if decoder == "recurrent":
        make = lambda: _s2s_model(D, N, K, skip_first, layers=layers)
    else:
        make = lambda: markov_model(D, N, K, skip_first, layers=layers)
    contract(_s2s_body(make, B, N, layers), _s2s_state(make(), B, N, 62), f"s2s {decoder} D{D} N{N} B{B} K{K}")


@pytest.mark.parametrize("decoder", ["recurrent", "markov"])
def test_s2s_fused_step_with_an_empty_edge_type(decoder):
    from test_gpu_s2s_markov import _model as markov_model
    from test_gpu_seq2seq import _s2s_model
    D, N, K, B = 2, 20, 2, 6
    if decoder == "recurrent":
        make = lambda: _s2s_model(D, N, K, False, he=128, hd=128, R=32, layers=2)
    else:
        make = lambda: markov_model(D, N, K, False, layers=2)
    g, got = contract(_s2s_body(make, B, N, 2), _s2s_state(make(), B, N, 81, empty_type=True), f"s2s {decoder} empty type")
    assert float(got.results["edges"][..., 1].abs().max()) == 0.0 and float(got.results["rollout.edges"][..., 1].abs().max()) == 0.0


@pytest.mark.parametrize("structure", [2, 3])
def test_s2s_fused_step_split_gemm_structures(structure):
    """``gemm_split`` forced to either kernel structure at (he, hd, B) = (128, 128, 44): 16,720 edge rows, ragged last tile."""
    from test_gpu_seq2seq import _s2s_model
    D, N, K, B = 2, 20, 2, 44
    make = lambda: _s2s_model(D, N, K, False, he=128, hd=128, R=32, layers=3, seed=71)
    with _options(gemm_split=structure):
        contract(_s2s_body(make, B, N, 3), _s2s_state(make(), B, N, 72), f"s2s gemm_split {structure}")


@pytest.mark.parametrize("markov", [False, True], ids=["recurrent", "markov"])
def test_s2s_dynamic_field_step_and_rollout(markov):
    """The FiLM field query inside the fused step (aether_s2s_dynfield_step / _rollout), D = 3, graphs of 5 rows."""
    import test_gpu_s2s_dynfield_rollout as DF
    B, N, D, steps = 7, 5, 3, 3
    make = lambda: DF._model(40 + D, N=N, D=D, markov=markov, mlp_hidden=96)
    model, _ = make()
    g0 = torch.Generator().manual_seed(100 * B + N)
    x, dh, hc, summary, u = DF._state(model, B, N, g0)
    U = torch.rand(steps, B, N * (N - 1), 2, generator=g0)
    inp = dict(x=x, h=hc[0], c=hc[1], summary=summary, u=u, U=U)
    if dh is not None:
        inp["dh"] = dh

    def body(g):
        r = Run()
        m, sd64 = make()
        m._set_summary(g["summary"])
        plan_bytes, ws_bytes = _s2s_sizes(m, B, N)
        out, dh1, (h1, c1), edges, field = m._fused_step(g["x"], g.get("dh"), (g["h"], g["c"]), g["u"], None, return_field=True)
        for name, t in (("out", out), ("dh", dh1), ("h", h1), ("c", c1), ("edges", edges), ("field", field)):
            if t is not None:
                r.result(name, t, output=True)
        r.workspace("plan", plan_bytes)
        r.workspace("step workspace", ws_bytes)
        cpu = lambda t: None if t is None else t.detach().cpu()
        w_out, w_dh, (wh, wc), z, gap, w_field = DF._oracle_step(m, sd64, cpu(g["x"]), cpu(g.get("dh")), (cpu(g["h"]), cpu(g["c"])),
                                                                 cpu(g["summary"]), cpu(g["u"]), edges=cpu(edges))
        for name, want in (("out", w_out), ("dh", w_dh), ("h", wh), ("c", wc), ("field", w_field)):
            if want is not None:
                r.against(name, want, S2S_TOL)
        clear = gap > 1e-3
        assert clear.float().mean() > 0.9 and torch.equal(cpu(edges).argmax(-1)[clear], z.argmax(-1)[clear])
        m.__dict__["_step_ws"] = None
        preds, e = m.predict_from_state(g["x"], g.get("dh"), (g["h"], g["c"]), g["summary"], steps, uniform=g["U"],
                                        return_edges=True)
        r.result("rollout", preds)
        r.result("rollout.edges", e)
        return r

    contract(body, inp, f"s2s dynamic field markov {markov}")


# ---- variable-N -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenes", ["three", "one"])
def test_variable_n_step_and_rollout(scenes):
    """The batched step (a one-step rollout: frames 0 and 1) and a 3-step rollout on three scenes of 2 to 12 present
    objects, one of which is empty at a step (no edges; the library refuses a scene with ONE present object, so the
    smallest edge-less scene is the empty one), and on the first scene alone, where the single-scene step entry runs too.
    The oracle runs scene by scene."""
    from oracle import dynamicvars_oracle as DO
    counts = [[12, 7, 2, 5], [2, 0, 3, 4], [5, 12, 9, 2]]
    if scenes == "one":
        counts = counts[:1]
    from test_gpu_dynamicvars import _scene_model, _scenes
    N, B = 12, len(counts)
    cpu_model, sd, P = _scene_model()
    s = _scenes(counts, N, 52, P["num_edge_types"])
    T = len(counts[0])
    want = torch.cat([DO.predict_future(sd, s["inputs"][b:b + 1], s["masks"][b:b + 1], s["node_inds"][b], s["graph_info"][b],
                                        s["burn"][b:b + 1], [s["uniform"][t][b] for t in range(T - 1)], P["gumbel_temp"],
                                        P["skip_first"], P["pos_representation"]) for b in range(B)])

    def body(g):
        r = Run()
        m = _scene_model()[0].cuda()
        lib = _lib.load()
        uni = g["uniform"] if B > 1 else [u[0] for u in g["uniform"]]
        # one step: frames 0 and 1
        one = m.predict_future(g["inputs"][:, :2].contiguous(), g["masks"][:, :2].contiguous(), [n[:2] for n in g["node_inds"]],
                               [gi[:2] for gi in g["graph_info"]], g["burn"][:, :2].contiguous(), uniform=uni[:1])
        r.result("step", one)
        r.against("step", want[:, :1])
        r.allocated("step predictions", (1, B, N, 4), torch.float32)
        m.__dict__["_step_ws"] = None
        out, pack = m._predict_future_rollout(g["inputs"], g["masks"], g["node_inds"], g["graph_info"], g["burn"],
                                              [[u] for u in uni] if B == 1 else uni, return_pack=True)
        r.result("rollout", out)
        r.against("rollout", want)
        r.allocated("rollout predictions", (T - 1, B, N, 4), torch.float32)
        r.workspace("rollout workspace", lib.aether_dyn_rollout_batched_workspace_bytes(
            C.byref(pack["cfg"]), B, N, T - 1, pack["n_present"], pack["n_edges"], pack["in_degree"]))
        # the staged path (field query, prior step, sampling and decoder step as calls of their own, torch glue between):
        # the same stage kernels on the same rows
        for mod in (m, m.encoder, m.decoder):
            mod._ws = None
        m.one_call_step = False
        staged = m.predict_future(g["inputs"], g["masks"], g["node_inds"], g["graph_info"], g["burn"], uniform=uni)
        m.one_call_step = True
        assert torch.equal(staged, out)
        r.result("staged", staged)
        if B == 1:           # the single-scene step entry (aether_dyn_step) at frame 0: 12 present objects
            m.__dict__["_step_ws"] = None
            gs, gr, e2n = g["graph_info"][0][0]
            ph, pc = m.encoder.get_initial_hidden(g["inputs"])
            dec = m.decoder.get_initial_hidden(g["inputs"])
            pred, h1, c1, d1, et = m._step_one_call(g["inputs"][:, 0], g["masks"][:, 0], g["node_inds"][0][0], gs, gr, e2n,
                                                    ph, pc, dec, g["uniform"][0][0], return_edge_types=True)
            r.result("single.pred", pred, output=True)
            r.result("single.edge_types", et, output=True)
            r.result("single.h", h1)
            r.result("single.dec", d1)
            r.against("single.pred", want[:, :1].reshape(1, N, 4))
            r.workspace("step workspace", lib.aether_dyn_step_workspace_bytes(
                C.byref(m._step_config()), N, int(g["node_inds"][0][0].numel()), int(gs.numel())))
        return r

    contract(body, s, f"variable-N {scenes}")
    if B > 1:
        # why no scene of the case has ONE present object, as the issue of this test asked: the library refuses it on the
        # host before anything is queued (dyn_batch_check)
        m = cpu_model.cuda()
        g = _map(_cuda, s)
        g["node_inds"][1][0] = g["node_inds"][1][0][:1]
        with pytest.raises(_lib.AetherHipError, match="one present object"):
            m.predict_future(g["inputs"], g["masks"], g["node_inds"], g["graph_info"], g["burn"], uniform=g["uniform"])
        torch.cuda.synchronize()


# ---- aether_amd/optim.py ----------------------------------------------------------------------------------------------------
def test_adamw_step_and_mse_loss():
    """One FusedAdamW step and ``mse_loss_grad`` on a 5-parameter model whose parameters and gradients end exactly where
    their guard bands begin, against torch.optim.AdamW and the MSE in fp64.  Bound 1e-6 scale-relative: every compared
    value is a handful of fp32 operations (each within 2^-24 relative) on values of the tensor's own scale.  The MSE
    scratch ("zero before the first launch") must come from torch.zeros: it is not among the guarded allocations."""
    from aether_amd import optim
    gen = torch.Generator().manual_seed(17)
    shapes = [(1,), (7,), (33, 5), (1000,), (3, 1, 2)]
    inp = {"p%d" % i: torch.randn(s, generator=gen) for i, s in enumerate(shapes)}
    inp.update({"g%d" % i: torch.randn(s, generator=gen) * 0.1 for i, s in enumerate(shapes)})
    inp["pred"], inp["target"] = torch.randn(37, 3, generator=gen), torch.randn(37, 3, generator=gen)
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    ref = [inp["p%d" % i].double().clone().requires_grad_(True) for i in range(5)]
    for i, p in enumerate(ref):
        p.grad = inp["g%d" % i].double()
    ref_opt = torch.optim.AdamW(ref, **hyper)
    ref_opt.step()
    want_loss = ((inp["pred"].double() - inp["target"].double()) ** 2).mean()
    want_grad = 2.0 * (inp["pred"].double() - inp["target"].double()) / inp["pred"].numel()
    scratch_bytes = _lib.load().aether_mse_scratch_bytes()
    saved = dict(optim._MseScratch._bufs)

    def body(g):
        r = Run()
        optim._MseScratch._bufs.clear()              # the scratch is allocated by this call
        loss, grad = optim.mse_loss_grad(g["pred"], g["target"])
        r.result("loss", loss, output=True)
        r.result("dpred", grad, output=True)
        r.against("loss", want_loss, 1e-6)
        r.against("dpred", want_grad, 1e-6)
        params = [g["p%d" % i].requires_grad_(True) for i in range(5)]
        for i, p in enumerate(params):
            p.grad = g["g%d" % i]
        opt = optim.FusedAdamW(params, **hyper)
        opt.step()
        for i, p in enumerate(params):
            r.result("p%d" % i, p)
            r.against("p%d" % i, ref[i].detach(), 1e-6)
            r.result("m%d" % i, opt.state[p]["exp_avg"])
            r.against("m%d" % i, ref_opt.state[ref[i]]["exp_avg"], 1e-6)
            r.result("v%d" % i, opt.state[p]["exp_avg_sq"])
            r.against("v%d" % i, ref_opt.state[ref[i]]["exp_avg_sq"], 1e-6)
        assert opt.steps_taken() == 1
        return r

    try:
        guard, _ = contract(body, inp, "optim")
        assert len(optim._MseScratch._bufs) == 1 and not guard.find(nbytes=scratch_bytes, dtype=torch.uint8)
    finally:
        optim._MseScratch._bufs.clear()
        optim._MseScratch._bufs.update(saved)


# ---- debug_fetch on a workspace of the other layout ----------------------------------------------------------------------------
def test_debug_fetch_refuses_the_inference_layout_of_a_wide_model():
    """Width 96 (kernel width 128): the library computes e1's offset from the training layout.  After an eval forward the
    workspace has the inference layout: ValueError before any library call.  With FLAG_KEEP_INTERMEDIATES the fetch returns
    the layer's messages, held to the oracle."""
    D, H = 2, 96
    m = _new_aether(D, H, 0)
    inp, _ = _aether_inputs("B3N5", D)
    g = _map(_cuda, inp)
    n, E = g["x"].shape[0], g["edges"][0].numel()
    eng = m._engine
    with torch.no_grad():
        m(g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"], g["charges"])
    for name in ("e1", "e2", "e3", "e4"):
        with pytest.raises(ValueError, match="inference layout"):
            eng.debug_fetch(name, n, E, eng._kw)
    torch.manual_seed(7)
    sd = {k: v.detach().double() for k, v in Aether(2 * D, H, 0.0, D, device="cpu").state_dict().items()}
    with torch.no_grad():
        want = O.aether_forward(sd, inp["x"].double(), inp["vel"].double(), inp["edges"], inp["edge_attr"].double(),
                                inp["charges"].double(), return_all=True)
    # what the Python table lets through in the inference layout really sits where the library looks (WideLayout)
    for k in (1, 2, 3, 4):
        assert scale_rel_err(eng.debug_fetch(f"x{k}", n, E, eng._kw).cpu()[:, :H], want[f"x{k}"]) <= TOL, k
    feat = eng.debug_fetch("efeat", n, E, 32).cpu()
    assert torch.isfinite(feat).all() and float(feat.abs().max()) > 0
    m.flags = _lib.FLAG_KEEP_INTERMEDIATES
    with torch.no_grad():
        m(g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"], g["charges"])
    guard = GuardedAlloc()                          # the fetch's destination and the order's, exact and fenced
    with guard:
        perm = eng.graph_perm(g["edges"], n).cpu()
        for k in (1, 2, 3):
            ek = eng.debug_fetch(f"e{k}", n, E, eng._kw).cpu()
            assert (ek[:, H:] == 0).all() and scale_rel_err(ek[:, :H], want[f"e{k}"][perm]) <= TOL, k
            xk = eng.debug_fetch(f"x{k}", n, E, eng._kw).cpu()
            assert scale_rel_err(xk[:, :H], want[f"x{k}"]) <= TOL, k
    guard.check()
    assert len(guard.find(shape=(E, eng._kw), dtype=torch.float32)) == 3 and guard.find(shape=(E,), dtype=torch.int32)
    # a 64-wide model (WsLayout): node states and messages sit in the prefix both layouts share -- after an inference-layout
    # call of the streamed kernels, which write them to memory, they are the oracle's -- the layer-1 features do not
    m64 = _new_aether(D, 64, STREAMED)
    with torch.no_grad():
        m64(g["h"], g["x"], g["edges"], g["vel"], g["edge_attr"], g["charges"])
    assert m64._last_ws_keep is False
    torch.manual_seed(7)
    sd64 = {k: v.detach().double() for k, v in Aether(2 * D, 64, 0.0, D, device="cpu").state_dict().items()}
    with torch.no_grad():
        want64 = O.aether_forward(sd64, inp["x"].double(), inp["vel"].double(), inp["edges"], inp["edge_attr"].double(),
                                  inp["charges"].double(), return_all=True)
    perm64 = m64.graph_perm(g["edges"], n).cpu()
    for k in (1, 2, 3, 4):
        assert scale_rel_err(m64.debug_fetch(f"x{k}", n, E, 64).cpu(), want64[f"x{k}"]) <= TOL, k
    for k in (1, 2, 3):
        assert scale_rel_err(m64.debug_fetch(f"e{k}", n, E, 64).cpu(), want64[f"e{k}"][perm64]) <= TOL, k
    with pytest.raises(ValueError, match="inference layout"):
        m64.debug_fetch("efeat", n, E, 32)
