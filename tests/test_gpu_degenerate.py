"""The HIP step at the reference's degenerate geometry: zero velocity (every sign pattern of +-0), velocities along an axis,
coincident particles, anti-parallel headings, tiny and subnormal velocities, self loops and nodes without in-edges.

Every stage, the parameter gradients and the input gradients are held to the branch-aligned oracle (branch_align.py): the
oracle in fp64 (target) and fp32 (floor) with whole periods added on the cut columns of the edges where the kernel took the
other side of a branch cut -- only ever within branch_align.MARGIN of the cut.  Errors are scale-relative per graph and
per row block; tolerances are the suite's (TOL forward, GTOL gradients) or 4x the fp32 oracle's own distance to fp64."""
import numpy as np
import pytest
import torch

import branch_align as BA
from conftest import load_case, load_state_dict, scale_rel_err
from aether_amd import _lib
from aether_amd.edges import get_edges, prepare_edge_attr
from aether_amd.nn.state2state.aether import Aether
from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether

pytestmark = pytest.mark.gpu
TOL = 1e-5
GTOL = 5e-5
KEEP = _lib.FLAG_KEEP_INTERMEDIATES
PATHS = {"fused": _lib.FLAG_FORCE_FUSED | KEEP, "streamed": _lib.FLAG_FORCE_STREAMED | KEEP}


def _model(D, H=64, flags=KEEP, sd=None):
    if sd is None:
        torch.manual_seed(7)
    m = Aether(2 * D, H, 0.0, D, device="cuda")
    if sd is not None:
        m.load_state_dict(sd)
    m.flags = flags
    return m, {k: v.detach().cpu() for k, v in m.state_dict().items()}


def _dev(inp):
    return {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in inp.items() if k != "edges"}


def _forward(m, inp, grad):
    """One forward; grad: x, vel, edge_attr and the parameters are autograd leaves (the training launch)."""
    d = _dev(inp)
    edges = [e.cuda() for e in inp["edges"]]
    leaves = {k: d[k].clone().requires_grad_(grad) for k in ("x", "vel", "edge_attr")}
    m.zero_grad(set_to_none=True)
    with torch.set_grad_enabled(grad):
        out = m(None, leaves["x"], edges, leaves["vel"], leaves["edge_attr"], d["charges"])
    torch.cuda.synchronize()
    return out, leaves, edges


def _stages(m, edges, Nn, D):
    """Every fetched stage of m's last forward, edge tensors in the caller's edge order."""
    eng = m.__dict__.get("_engine", m)
    E = edges[0].numel()
    H = m.hidden_size
    perm = eng.graph_perm(edges, Nn).cpu()
    got = {"field": eng.debug_fetch("field", Nn, E, D).cpu(),
           "R": eng.debug_fetch("R", Nn, E, D * D).cpu().view(Nn, D, D)}
    got["rel_feat"] = torch.cat([torch.zeros(Nn, D), eng.debug_fetch("canon", Nn, E, 2 * D).cpu()], -1)
    for l in range(1, 5):
        got[f"x{l}"] = eng.debug_fetch(f"x{l}", Nn, E, m._kw).cpu()[:, :H]
        es = eng.debug_fetch(f"e{l}", Nn, E, m._kw).cpu()[:, :H]
        e = torch.empty_like(es)
        e[perm] = es
        got[f"e{l}"] = e
    return got


def _align(feat, sd, inp, num_nodes=None, grads=True):
    """Oracle in fp64 and fp32 (unshifted, for the shift) and branch-aligned to the kernel's features."""
    r64 = BA.run_oracle(sd, inp, torch.float64, num_nodes=num_nodes, grads=False)[0]
    r32 = BA.run_oracle(sd, inp, torch.float32, num_nodes=num_nodes, grads=False)[0]
    s64, s32, n = BA.branch_shifts(feat, r64["edge_attr_local"], r32["edge_attr_local"], inp["x"].shape[1])
    a64 = BA.run_oracle(sd, inp, torch.float64, shift=s64, num_nodes=num_nodes, grads=grads)
    a32 = BA.run_oracle(sd, inp, torch.float32, shift=s32, num_nodes=num_nodes, grads=grads)
    return a64, a32, n


def _check_features(feat, a64, a32, D, blocks, what):
    """The kernel's layer-1 features against the aligned oracle, column by column; the pad columns exactly zero."""
    nl = BA.n_local(D)
    want = torch.cat([a64["edge_attr_local"], a64["_edge_attr"]], -1)
    floor = torch.cat([a32["edge_attr_local"], a32["_edge_attr"]], -1)
    for c in range(nl + 2):
        for name, rows, _ in blocks:
            w = want[rows, c]
            den = max(float(w.abs().max()), 1.0)      # angles, distances, unit-scale vectors: absolute below 1
            err = float((feat[rows, c].double() - w).abs().max()) / den
            fl = float((floor[rows, c].double() - w).abs().max()) / den
            assert err <= max(TOL, 4 * fl), (what, "feature column", c, name, err, fl)
    assert torch.equal(feat[:, nl + 2:], torch.zeros_like(feat[:, nl + 2:])), (what, "pad columns")


def _check_stages(got, a64, a32, inp, graph_of, what, keys=("field", "R", "rel_feat", "x1", "x2", "x3", "x4", "e1", "e2",
                                                               "e3", "e4", "out")):
    nb = BA.node_blocks(inp["x"], inp["vel"], graph_of)
    eb = BA.edge_blocks(inp["edges"][1], graph_of)
    for k in keys:
        g = got[k].reshape(got[k].shape[0], -1)
        BA.assert_blocks(g, a64[k].reshape(g.shape), a32[k].reshape(g.shape), eb if k[0] == "e" else nb, TOL, (what, k))


def _check_input_grads(leaves, ig64, ig32, inp, graph_of, what):
    nb = BA.node_blocks(inp["x"], inp["vel"], graph_of)
    eb = BA.edge_blocks(inp["edges"][1], graph_of)
    for k in ("x", "vel", "edge_attr"):
        g = leaves[k].grad.cpu()
        for name, err, fl in BA.block_errors(g, ig64[k], ig32[k], eb if k == "edge_attr" else nb):
            print(f"[{what}] d/d{k} {name}: HIP {err:.2e}, oracle fp32 {fl:.2e}")
        BA.assert_blocks(g, ig64[k], ig32[k], eb if k == "edge_attr" else nb, GTOL, (what, "d/d" + k))


def _check_param_grads(m, pg64, pg32, what):
    for k, p in m.named_parameters():
        g = p.grad.cpu()
        assert torch.isfinite(g).all(), (what, k)
        err, fl = scale_rel_err(g, pg64[k]), scale_rel_err(pg32[k], pg64[k])
        assert err <= max(GTOL, 4 * fl), (what, k, err, fl)


def _with_edge_attr(res, inp):
    res["_edge_attr"] = inp["edge_attr"].double()
    return res


# ------------------------------------------------------------------------------------------------ the golden fixture
@pytest.mark.parametrize("path", ["fused", "streamed"])
@pytest.mark.parametrize("D", [2, 3])
def test_golden_edge_case_every_stage(D, path):
    """case_D{D}_edge_B2N5: graph 0 (nodes 0-4) is the degenerate one, graph 1 (nodes 5-9) is regular."""
    inp, ref, _, meta = load_case(f"case_D{D}_edge_B2N5.npz")
    sd = load_state_dict(D)
    m, _ = _model(D, flags=PATHS[path], sd=sd)
    Nn, N = inp["x"].shape[0], meta["N"]
    out, _, edges = _forward(m, inp, grad=False)
    got = _stages(m, edges, Nn, D)
    got["out"] = out.cpu()
    feat = BA.kernel_features(m, edges, Nn)
    graph_of = torch.arange(Nn) // N
    recv = inp["edges"][1]
    n1, e1 = graph_of == 1, graph_of[recv] == 1
    n0, e0 = ~n1, ~e1
    # graph 1: every stage against the reference itself
    nl = BA.n_local(D)
    got["efeat"] = feat[:, :nl]
    for k in ("field", "R", "rel_feat", "efeat", "x1", "x2", "x3", "x4", "e1", "e2", "e3", "e4", "out"):
        rk = ref["edge_attr_local" if k == "efeat" else k]
        rows = e1 if k[0] == "e" else n1
        assert scale_rel_err(got[k][rows], rk[rows]) <= TOL, ("graph 1", k)
    assert torch.equal(feat[:, nl:nl + 2], inp["edge_attr"])
    # graph 0, node stages: no cut
    for k in ("field", "R", "rel_feat"):
        assert scale_rel_err(got[k][n0], ref[k][n0]) <= TOL, ("graph 0", k)
    # graph 0, features: against the reference, whole periods on the cut columns only (and only near a cut)
    a64, a32, n64 = _align(feat, sd, inp, grads=False)
    a64, a32 = _with_edge_attr(a64[0], inp), _with_edge_attr(a32[0], inp)
    r64 = BA.run_oracle(sd, inp, torch.float64, grads=False)[0]
    s_ref, _, n_ref = BA.branch_shifts(feat, ref["edge_attr_local"], r64["edge_attr_local"], D)
    print(f"[edge case D={D} {path}] edges shifted: {n64} against the fp64 oracle, {n_ref} against the reference")
    ref_al = {"edge_attr_local": ref["edge_attr_local"].double() + s_ref, "_edge_attr": inp["edge_attr"].double()}
    eb = BA.edge_blocks(recv, graph_of)
    _check_features(feat, ref_al, a32, D, eb, ("reference", path))
    _check_features(feat, a64, a32, D, eb, ("fp64 oracle", path))
    # graph 0, later stages and the output: the aligned fp64 oracle
    _check_stages(got, a64, a32, inp, graph_of, ("edge case", D, path))
    if n_ref == 0:       # the kernel took the reference's side on every edge: the reference itself
        for k in ("x1", "x2", "x3", "x4", "e1", "e2", "e3", "e4", "out"):
            rows = e0 if k[0] == "e" else n0
            fl = scale_rel_err(a32[k][rows], a64[k][rows])
            assert scale_rel_err(got[k][rows], ref[k][rows]) <= max(TOL, 4 * fl), ("graph 0 vs reference", k)


VARIANTS = {"fused": ("fused", None), "streamed": ("streamed", None), "edge_acc8": ("streamed", 3),
            "edge_acc0": ("streamed", 0)}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("D", [2, 3])
def test_golden_edge_case_parameter_gradients(D, variant):
    """All 47 parameter gradients on case_D{D}_edge_B2N5: default backward on both paths, and the per-layer weight
    gradients accumulated in the edge kernel (edge_acc 3) or from row tensors (edge_acc 0)."""
    from test_gpu_backward import DEFAULT_EDGE_ACC
    inp, ref, _, meta = load_case(f"case_D{D}_edge_B2N5.npz")
    sd = load_state_dict(D)
    path, acc = VARIANTS[variant]
    m, _ = _model(D, flags=PATHS[path], sd=sd)
    lib = _lib.load()
    try:
        if acc is not None:
            _lib.check(lib.aether_set_option(b"outer_defer_max_edges", 0), "set_option")
            _lib.check(lib.aether_set_option(b"edge_acc", acc), "set_option")
        out, leaves, edges = _forward(m, inp, grad=True)
        feat = BA.kernel_features(m, edges, inp["x"].shape[0])
        torch.nn.functional.mse_loss(out, inp["target"].cuda()).backward()
        torch.cuda.synchronize()
    finally:
        _lib.check(lib.aether_set_option(b"outer_defer_max_edges", 1 << 20), "set_option")
        _lib.check(lib.aether_set_option(b"edge_acc", DEFAULT_EDGE_ACC), "set_option")
    (_, pg64, _), (_, pg32, _), n64 = _align(feat, sd, inp)
    r64 = BA.run_oracle(sd, inp, torch.float64, grads=False)[0]
    _, _, n_ref = BA.branch_shifts(feat, ref["edge_attr_local"], r64["edge_attr_local"], D)
    print(f"[edge case D={D} {variant}] edges shifted: {n64} against the fp64 oracle, {n_ref} against the reference")
    _check_param_grads(m, pg64, pg32, (D, variant))
    if n_ref == 0:
        for k, p in m.named_parameters():
            assert scale_rel_err(p.grad.cpu(), ref["grad." + k]) <= GTOL, ("reference", k)


@pytest.mark.parametrize("path", ["fused", "streamed"])
@pytest.mark.parametrize("D", [2, 3])
def test_golden_edge_case_input_gradients(D, path):
    """d/dx, d/dvel, d/dedge_attr on case_D{D}_edge_B2N5 against the aligned oracle's fp64 autograd and against the
    reference's own (case_D{D}_edgegrad.npz: d/dvel_z = -2.9e4 at the 3-D zero velocity, d/dx_z = +-58.5 at the
    coincident pair -- the polar angle's 1/eps slope)."""
    inp, ref, _, meta = load_case(f"case_D{D}_edgegrad.npz")
    sd = load_state_dict(D)
    m, _ = _model(D, flags=PATHS[path], sd=sd)
    out, leaves, edges = _forward(m, inp, grad=True)
    Nn = inp["x"].shape[0]
    feat = BA.kernel_features(m, edges, Nn)
    torch.nn.functional.mse_loss(out, inp["target"].cuda()).backward()
    torch.cuda.synchronize()
    (_, _, ig64), (_, _, ig32), n64 = _align(feat, sd, inp)
    e_ref = load_case(f"case_D{D}_edge_B2N5.npz")[1]
    r64 = BA.run_oracle(sd, inp, torch.float64, grads=False)[0]
    _, _, n_ref = BA.branch_shifts(feat, e_ref["edge_attr_local"], r64["edge_attr_local"], D)
    print(f"[edge case D={D} {path}] edges shifted: {n64} against the fp64 oracle, {n_ref} against the reference")
    graph_of = torch.arange(Nn) // meta["N"]
    _check_input_grads(leaves, ig64, ig32, inp, graph_of, ("edge case", D, path))
    if n_ref == 0:       # the reference's fp32 gradients sit as far from fp64 as any fp32 evaluation: both distances
        nb = BA.node_blocks(inp["x"], inp["vel"], graph_of)
        eb = BA.edge_blocks(inp["edges"][1], graph_of)
        for k in ("x", "vel", "edge_attr"):
            g, blocks = leaves[k].grad.cpu(), eb if k == "edge_attr" else nb
            assert torch.isfinite(g).all(), k
            for (name, err, _), (_, _, fl) in zip(BA.block_errors(g, ref["grad_in." + k], g, blocks),
                                                  BA.block_errors(g, ig64[k], ig32[k], blocks)):
                assert err <= max(2 * GTOL, 4 * fl), ("reference", "d/d" + k, name, err, fl)


# ------------------------------------------------------------------------------------- seeded synthetic batches
def _degenerate_batch(D, seed, forward_only):
    """Graphs of 8 nodes, each with a kind of degenerate node next to random regular ones.  forward_only adds what has no
    finite slope or none representable in fp32: |v| = 2 along z (v_z / (|v| + eps) rounds to 1) and velocities of 1e-20
    and 1e-41 (fp32 subnormal)."""
    g = torch.Generator().manual_seed(seed)
    N = 8
    zeros = [torch.tensor(s, dtype=torch.float32) * 0.0 for s in
             ([[a, b] for a in (1, -1) for b in (1, -1)] if D == 2 else
              [[a, b, c] for a in (1, -1) for b in (1, -1) for c in (1, -1)])]
    eye = torch.eye(D)
    rand_v = lambda: (lambda v: 0.5 * v / v.norm())(torch.randn(D, generator=g))
    graphs = []                                              # (velocities, position tweaks)
    graphs.append((zeros[:N], {}))                           # zero velocity, every sign pattern of +-0
    horiz = [0.5 * s * eye[a] for a in range(2) for s in (1, -1)]
    graphs.append((horiz, {}))                               # along +-x, +-y (anti-parallel pairs, exact theta = pi)
    if D == 3:                                               # along +-z, apart from horizontal / still ones (a gimbal)
        vert = [0.5 * eye[2], -0.5 * eye[2]] + ([2.0 * eye[2], -2.0 * eye[2]] if forward_only else [])
        graphs.append((vert, {}))
    w = torch.tensor([0.3, 0.0, -0.4][:D]) if D == 3 else torch.tensor([0.0, -0.5])
    u = torch.tensor([0.0, 0.5, 0.0][:D]) if D == 3 else torch.tensor([0.4, 0.0])
    graphs.append(([w, -w, u, -u, rand_v(), rand_v()], {1: 0, 3: 2, 5: 2}))   # anti-parallel v, -v; coincident pair, triple
    if forward_only:
        graphs.append(([1e-20 * rand_v(), 1e-20 * rand_v(), 1e-41 * eye[0], -1e-41 * eye[1], 2e-41 * rand_v() / 0.5],
                       {}))
    xs, vs = [], []
    for vel, same in graphs:
        x = torch.randn(N, D, generator=g)
        v = torch.stack([rand_v() for _ in range(N)])
        v[:len(vel)] = torch.stack(vel)
        for a, b in same.items():
            x[a] = x[b]
        xs.append(x)
        vs.append(v)
    x, vel = torch.cat(xs), torch.cat(vs)
    B = len(graphs)
    Nn = B * N
    send, recv = get_edges(B, N)
    keep = recv != 2 * N + 5                                 # node 5 of graph 2 receives nothing
    loops = torch.tensor([0, N + 1, 2 * N + 3, Nn - 1])      # self loops, one of them on a zero velocity
    send = torch.cat([send[keep], loops])
    recv = torch.cat([recv[keep], loops])
    charges = torch.randint(0, 3, (Nn, 1), generator=g).float() - 1.0
    edges = [send, recv]
    inp = dict(x=x, vel=vel, charges=charges, edges=edges,
               edge_attr=prepare_edge_attr(x, edges, charges[send] * charges[recv]),
               target=x + vel + 0.05 * torch.randn(Nn, D, generator=g))
    if D == 3:
        r64 = BA.run_oracle({k: v for k, v in load_state_dict(D).items()}, inp, torch.float64, grads=False)[0]
        R = r64["R"]
        M20 = (R[recv].transpose(-1, -2) @ R[send])[:, 2, 0]
        assert float((1.0 - M20.abs()).min()) > 1e-3, "the batch holds a gimbal edge"
        if not forward_only:                                 # the polar angles' slopes are finite in fp32
            r32 = BA.run_oracle(load_state_dict(D), inp, torch.float32, grads=False)[0]
            v32 = vel.float()
            c = v32[:, 2] / (v32.norm(dim=-1) + 1e-7)
            rr = r32["edge_attr_local"][:, :3]
            ce = rr[:, 2] / (rr.norm(dim=-1) + 1e-7)
            assert float(c.abs().max()) < 1.0 and float(ce.abs().max()) < 1.0
    return inp, N


SYNTH = {"fused": (64, _lib.FLAG_FORCE_FUSED | KEEP), "streamed": (64, _lib.FLAG_FORCE_STREAMED | KEEP),
         "narrow32": (32, KEEP), "wide128": (128, KEEP), "wide256": (256, KEEP)}


@pytest.mark.parametrize("variant", list(SYNTH))
@pytest.mark.parametrize("D", [2, 3])
def test_synthetic_degenerate_forward(D, variant):
    H, flags = SYNTH[variant]
    inp, N = _degenerate_batch(D, 100 + D, forward_only=True)
    m, sd = _model(D, H, flags, sd=load_state_dict(D) if H == 64 else None)
    Nn = inp["x"].shape[0]
    out, _, edges = _forward(m, inp, grad=False)
    got = _stages(m, edges, Nn, D)
    got["out"] = out.cpu()
    feat = BA.kernel_features(m, edges, Nn)
    a64, a32, n64 = _align(feat, sd, inp, grads=False)
    print(f"[synthetic D={D} {variant}] edges shifted against the fp64 oracle: {n64}")
    a64, a32 = _with_edge_attr(a64[0], inp), _with_edge_attr(a32[0], inp)
    graph_of = torch.arange(Nn) // N
    _check_features(feat, a64, a32, D, BA.edge_blocks(inp["edges"][1], graph_of), ("synthetic", variant))
    _check_stages(got, a64, a32, inp, graph_of, ("synthetic", D, variant))


@pytest.mark.parametrize("variant", list(SYNTH))
@pytest.mark.parametrize("D", [2, 3])
def test_synthetic_degenerate_gradients(D, variant):
    H, flags = SYNTH[variant]
    inp, N = _degenerate_batch(D, 200 + D, forward_only=False)
    m, sd = _model(D, H, flags, sd=load_state_dict(D) if H == 64 else None)
    Nn = inp["x"].shape[0]
    out, leaves, edges = _forward(m, inp, grad=True)
    feat = BA.kernel_features(m, edges, Nn)
    torch.nn.functional.mse_loss(out, inp["target"].cuda()).backward()
    torch.cuda.synchronize()
    (_, pg64, ig64), (_, pg32, ig32), n64 = _align(feat, sd, inp)
    print(f"[synthetic D={D} {variant}] edges shifted against the fp64 oracle: {n64}")
    _check_param_grads(m, pg64, pg32, ("synthetic", D, variant))
    _check_input_grads(leaves, ig64, ig32, inp, torch.arange(Nn) // N, ("synthetic", D, variant))


@pytest.mark.parametrize("D", [2, 3])
def test_synthetic_degenerate_dynamic_field(D):
    """The dynamic-field variant with the reference's parameters (dynfield_D{D}.npz): output, parameter and input
    gradients.  Its cut columns depend on positions and velocities only; the side of each cut is read from a plain
    64-wide step's features on the same inputs (same kernels, the field enters other columns)."""
    import os
    from conftest import GOLDEN
    d = np.load(os.path.join(GOLDEN, f"dynfield_D{D}.npz"))
    sd = {str(k): torch.from_numpy(d["sd." + str(k)]) for k in d["keys"]}
    dm = DynamicFieldAether(2 * D, 64, 0.0, D, device="cuda")
    dm.load_state_dict(sd)
    for forward_only in (True, False):
        inp, N = _degenerate_batch(D, 300 + D, forward_only=forward_only)
        Nn = inp["x"].shape[0]
        probe, _ = _model(D, 64, KEEP, sd=load_state_dict(D))
        _, _, edges = _forward(probe, inp, grad=False)
        feat = BA.kernel_features(probe, edges, Nn)
        graph_of = torch.arange(Nn) // N
        nb = BA.node_blocks(inp["x"], inp["vel"], graph_of)
        dv = _dev(inp)
        if forward_only:
            (a64, _, _), (a32, _, _), n64 = _align(feat, sd, inp, num_nodes=N, grads=False)
            with torch.no_grad():
                out = dm(None, dv["x"], edges, dv["vel"], dv["edge_attr"], dv["charges"], N)
            BA.assert_blocks(out.cpu(), a64["out"], a32["out"], nb, TOL, ("dynamic field", D, "out"))
            BA.assert_blocks(dm.last_field.cpu(), a64["field"], a32["field"], nb, TOL, ("dynamic field", D, "field"))
        else:
            (_, pg64, ig64), (_, pg32, ig32), n64 = _align(feat, sd, inp, num_nodes=N)
            leaves = {k: dv[k].clone().requires_grad_(True) for k in ("x", "vel", "edge_attr")}
            dm.zero_grad(set_to_none=True)
            out = dm(None, leaves["x"], edges, leaves["vel"], leaves["edge_attr"], dv["charges"], N)
            torch.nn.functional.mse_loss(out, dv["target"]).backward()
            torch.cuda.synchronize()
            _check_param_grads(dm, pg64, pg32, ("dynamic field", D))
            _check_input_grads(leaves, ig64, ig32, inp, graph_of, ("dynamic field", D))
        print(f"[dynamic field D={D} forward_only={forward_only}] edges shifted against the fp64 oracle: {n64}")
