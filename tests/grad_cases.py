"""The cases of tests/test_gpu_grad_parity.py -- inputs, weights and the fp32 / fp64 CPU gradients every bar is taken
against -- and the backward's arithmetic restated inside the oracle.  Test helper, not a test module.

`split_backward` is `update_cases.split_linears` with a backward: while active, every `gnn.*` Linear of the oracle is an
autograd function whose forward is the three-term product of fp16 pieces and whose backward forms dX = dY W and
dW = dY^T X from fp16 pieces of dY, W and X, three terms and an fp32 result each.  dY is split as csrc/common.h splits a
GEMM's activation operand (`split_scale_of`): per 16-row tile, as it is where the tile's maximum lies in 2^-6 .. 2^15, and
otherwise scaled by the power of two that brings the maximum to 2^13 .. 2^14 (the scale is exact and is taken out of
the fp32 result).  With an MSE loss over hundreds of elements every dY tile is below 2^-6, so the scaled path is the
one taken; a per-tensor scale would leave the small tiles of a batch with fewer significant bits than the kernels give
them.  `drop` leaves one cross term out of one product of one layer, `hi_only` keeps only hi x hi in both products.

References (g32: under ORDERS orders of the edge list, tests/grad_parity.py says why): the oracle's autograd (Aether, DynamicFieldAether), the restatements' `grads` (LoCS, EGNN-Aether, ClofNet)
and `rollout_train_cases.reference` (training through the rollout), in fp32 and fp64 on one thread, once per process.
Keys: parameter names, and "d/dx", "d/dvel", "d/dedge_attr" (steps) or "x0", "vel0" (rollouts) for the inputs.

Weights: each model built on the CPU under torch.manual_seed(MODEL_SEED = 11).  Input seeds: the first of 5, 6, 7, ...
at which the case's Q (tests/grad_parity.py) is not degenerate and, for the families whose restatement runs on the
oracle's `gnn.*` Linears, the emulation is at or under SEED_MARGIN = 0.9 of the bar (fp32 results move with the host
CPU; the test asserts the bar itself); for the rollouts also every edge of every step 1e-4 rad from a branch cut of the
feature map.  At D = 3 and B2N5 the emulation sits at 0.9 .. 1.3 of the bar on about every second seed: these shapes have
the fewest elements per tensor and the luckiest floors.  All of it is looked up on the CPU and asserted by
tests/test_grad_metric.py."""
from __future__ import annotations

import contextlib
import functools

import torch

import dynfield_rollout_cases as DR
import egnn_restatement as ER
import graph_cases as GC
import locs_restatement as LR
import rollout_train_cases as RT
import update_cases as U
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O
from update_cases import _pieces

BACKWARD_TERMS = ("dx:dy_lo*w_hi", "dx:dy_hi*w_lo", "dw:dy_lo*x_hi", "dw:dy_hi*x_lo")
TILE_ROWS = 16
MODEL_SEED = 11
SEED_MARGIN = 0.9
ORDERS = 8                                      # evaluations of the fp32 restatement per case, each on another edge order
INPUT_KEYS = {"x": "d/dx", "vel": "d/dvel", "edge_attr": "d/dedge_attr"}


def edge_orders(n_edges):
    """ORDERS permutations of the edge list, the given order first."""
    yield torch.arange(n_edges)
    for i in range(1, ORDERS):
        yield torch.randperm(n_edges, generator=torch.Generator().manual_seed(100 + i))


def reordered(inp, perm):
    """The same graph with its edge list (and the per-edge inputs) in another order."""
    return dict(inp, edges=[e[perm] for e in inp["edges"]], edge_attr=inp["edge_attr"][perm])


def _tile_scales(t32):
    """[rows, 1] powers of two, the rule of csrc/common.h (split_scale_of) per 16-row tile."""
    rows = t32.shape[0]
    pad = (-rows) % TILE_ROWS
    a = torch.cat([t32.abs(), t32.new_zeros(pad, t32.shape[1])]) if pad else t32.abs()
    mx = a.reshape(-1, TILE_ROWS * t32.shape[1]).max(dim=1).values.double()
    plain = (mx == 0) | ((mx >= 2.0 ** -6) & (mx < 2.0 ** 15))
    e = torch.floor(torch.log2(mx.clamp(min=1e-300)))
    sh = (13 - e).clamp(-40, 40)
    s = torch.where(plain, torch.ones_like(mx), 2.0 ** sh)
    return s.repeat_interleave(TILE_ROWS)[:rows, None]


def _scaled_pieces(t):
    """(hi, lo) of t as the backward GEMMs see it, with the tile scales already taken out again (exact in fp64)."""
    t32 = t.float()
    s = _tile_scales(t32)
    hi, lo = _pieces((t32.double() * s).float())
    return hi / s, lo / s


class _SplitLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, name, drop, hi_only):
        ctx.save_for_backward(x, w)
        ctx.name, ctx.drop, ctx.hi_only = name, drop, hi_only
        wh, wl = _pieces(w)
        xh, xl = _pieces(x)
        acc = xh @ wh.T + xl @ wh.T + xh @ wl.T
        return (acc.float() + b.float()).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        out = lambda term: ctx.hi_only or ctx.drop == (ctx.name, term)
        dyh, dyl = _scaled_pieces(dy)
        wh, wl = _pieces(w)
        xh, xl = _pieces(x)
        dx = dyh @ wh
        if not out("dx:dy_hi*w_lo"):
            dx = dx + dyh @ wl
        if not out("dx:dy_lo*w_hi"):
            dx = dx + dyl @ wh
        dw = dyh.T @ xh
        if not out("dw:dy_hi*x_lo"):
            dw = dw + dyh.T @ xl
        if not out("dw:dy_lo*x_hi"):
            dw = dw + dyl.T @ xh
        return dx.float().to(x.dtype), dw.float().to(w.dtype), dy.sum(0), None, None, None


@contextlib.contextmanager
def split_backward(drop=None, hi_only=False):
    """The design's arithmetic, forward and backward, in the oracle's `gnn.*` Linears while active.  `drop` = (layer
    name, one of BACKWARD_TERMS)."""
    assert drop is None or drop[1] in BACKWARD_TERMS, drop
    plain = O._linear

    def linear(sd, name, x):
        if not name.startswith("gnn."):
            return plain(sd, name, x)
        assert x.dim() == 2
        return _SplitLinear.apply(x, sd[name + ".weight"], sd[name + ".bias"], name, drop, hi_only)

    O._linear = linear
    try:
        yield
    finally:
        O._linear = plain


# ---- one training step of Aether, LoCS, DynamicFieldAether ----------------------------------------------------------------
def _classes():
    from aether_amd.nn.state2state.aether import Aether
    from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
    from aether_amd.nn.state2state.locs import LoCS
    return {"Aether": Aether, "LoCS": LoCS, "DynamicFieldAether": DynamicFieldAether}


def build(family, D, H, dropout=0.0, device="cpu"):
    """The drop-in under MODEL_SEED (initialised on the CPU whatever the device: the same weights)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(MODEL_SEED)
        return U._quiet(_classes()[family], 2 * D, H, dropout, D, device=device)


@functools.lru_cache(maxsize=None)
def state_dict(family, D, H):
    return U.state_of(build(family, D, H))


def _special_graph(name, seed, D=2):
    """The graphs of test_gpu_fused_waits.py's cases of that name (2-D) and of tests/irregular_graphs.py, under an input
    seed of this file's rule."""
    import irregular_graphs as IG
    import test_gpu_fused_waits as W
    if name in IG.GRAPHS:
        return IG.build(name, D, seed)
    assert D == 2, (name, D)
    return {"star_32": W._star, "isolated_n12": W._isolated}[name](seed)


@functools.lru_cache(maxsize=None)
def step_inputs(case):
    """case = (family, D, H, B, N, input seed, dropout, graph); graph "full", a case name of test_gpu_fused_waits.py or a graph of
    tests/irregular_graphs.py (B = 1, N = all its nodes).
    -> (inputs, the two dropout masks or None)."""
    family, D, H, B, N, seed, p, graph = case
    inp = make_batch(B, N, D, seed=seed) if graph == "full" else _special_graph(graph, seed, D)
    assert inp["x"].shape == (B * N, D)
    masks = None
    if p > 0:
        g = torch.Generator().manual_seed(seed)
        masks = (torch.rand(2, B * N, H, generator=g) >= p).float() / (1.0 - p)
    return {k: v for k, v in inp.items() if k != "meta"}, masks


def step_grads(family, sd32, inp, masks, num_nodes, dtype):
    """{parameter | d/dx | d/dvel | d/dedge_attr: gradient of MSELoss(out, target)} in `dtype`."""
    c = lambda t: U._cast(t.detach(), dtype)
    sd = {k: c(v) for k, v in sd32.items()}
    mk = None if masks is None else c(masks)
    if family == "LoCS":
        pg, ig, _ = LR.grads(sd, c(inp["x"]), c(inp["vel"]), inp["edges"], c(inp["edge_attr"]), c(inp["target"]), mk, inputs=True)
        return {**pg, **{INPUT_KEYS[k]: v for k, v in ig.items()}}
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    ins = {k: c(inp[k]).clone().requires_grad_(True) for k in INPUT_KEYS}
    a = (leaves, ins["x"], ins["vel"], inp["edges"], ins["edge_attr"], c(inp["charges"]))
    if family == "Aether":
        out = O.aether_forward(*a, dropout_masks=mk)
    else:
        out = O.dynamic_field_aether_forward(*a, num_nodes, dropout_masks=mk)
    loss = torch.nn.functional.mse_loss(out, c(inp["target"]))
    wrt = list(leaves.values()) + list(ins.values())
    g = torch.autograd.grad(loss, wrt)
    return dict(zip(list(leaves) + [INPUT_KEYS[k] for k in ins], g))


@functools.lru_cache(maxsize=None)
def step_case(case):
    """-> dict(sd, inp, masks, g32, g64) of one case of STEP_CASES; g32: one dict per edge order (`edge_orders`)."""
    family, D, H, B, N, seed, p, graph = case
    sd = state_dict(family, D, H)
    inp, masks = step_inputs(case)
    with U.one_thread():
        g64 = step_grads(family, sd, inp, masks, N, torch.float64)
        g32 = []
        for perm in edge_orders(inp["edges"][0].numel()):
            g = step_grads(family, sd, reordered(inp, perm), masks, N, torch.float32)
            g["d/dedge_attr"] = torch.zeros_like(g["d/dedge_attr"]).index_copy_(0, perm, g["d/dedge_attr"])
            g32.append(g)
    return dict(sd=sd, inp=inp, masks=masks, g32=g32, g64=g64)


@functools.lru_cache(maxsize=None)
def step_emulated(case, drop=None, hi_only=False):
    """The gradients the design's arithmetic gives on a case: the fp64 reference under `split_backward`."""
    family, D, H, B, N, seed, p, graph = case
    inp, masks = step_inputs(case)
    with U.one_thread(), split_backward(drop, hi_only):
        g = step_grads(family, state_dict(family, D, H), inp, masks, N, torch.float64)
    return {k: v.float() for k, v in g.items()}


def rounded_weights(sd, bits=None):
    """Every `gnn.*` weight matrix rounded to fp16 and back -- what a backward that lost every lo piece of W would use
    -- or, with `bits`, to that many significand bits."""
    def rnd(v):
        if bits is None:
            return v.half().to(v.dtype)
        m, e = torch.frexp(v)
        return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e)
    return {k: (rnd(v) if k.startswith("gnn.") and k.endswith(".weight") else v) for k, v in sd.items()}


def case_id(case):
    family, D, H, B, N, seed, p, graph = case
    tag = f"{family}-D{D}-H{H}-B{B}N{N}-s{seed}"
    return tag + (f"-p{p}" if p else "") + ("" if graph == "full" else f"-{graph}")




def _a(D, H, B, N, seed=5, family="Aether", p=0.0, graph="full"):
    return (family, D, H, B, N, seed, p, graph)


# Aether at hidden 64, on both dispatch paths: B2N5 -- one workgroup holds several graphs; B6N7; B16N20 -- two workgroups
# per graph with the hand-off
AETHER_BOTH = [_a(2, 64, 2, 5), _a(3, 64, 2, 5, 6), _a(3, 64, 6, 7), _a(2, 64, 16, 20)]
# fused only: D3 at two workgroups per graph; N = 18 -- the 12-wave layout of one-node-tile workgroups; one receiver for
# all edges; nodes without in-edges
AETHER_FUSED = [_a(3, 64, 2, 20), _a(2, 64, 4, 18), _a(2, 64, 1, 32, 8, graph="star_32"),
                _a(2, 64, 2, 12, 5, graph="isolated_n12")]
# streamed only: degree above 64 -- the row sums run as their own kernel
AETHER_STREAMED = [_a(2, 64, 1, 70)]
# the graphs of tests/irregular_graphs.py, B = 1 and N = all nodes.  k_fused_bwd: packed scenes of different sizes; with
# `fused_split` off 11 tiles in one workgroup (the three-tiles-per-wave round) beside an edge-less group; split halves of
# 11 tiles with the hand-off
IRREGULAR_FUSED = [_a(3, 64, 1, 53, 5, graph="knn_mixed_k10"), _a(2, 64, 1, 16, 5, graph="multi16_E170"),
                   _a(3, 64, 1, 60, 5, graph="knn_2x30_k11")]
IRREGULAR_FUSED_SPLIT = {"knn_mixed_k10": 1, "multi16_E170": 0, "knn_2x30_k11": 1}          # the `fused_split` option
# `fused_split` off: 19 tiles in one workgroup, more than k_fused_bwd takes -- the keeping k_fused, then the backward
# layer by layer
IRREGULAR_LAYERWISE = [_a(2, 64, 1, 32, 6, graph="multi32_hub40"), _a(3, 64, 1, 32, 5, graph="multi32_hub40")]
# streamed: in-degree 86 on duplicated edges -- the row sums run as their own kernel
IRREGULAR_STREAMED = [_a(2, 64, 1, 32, 6, graph="multi32_hub80")]
IRREGULAR_STEP_CASES = IRREGULAR_FUSED + IRREGULAR_LAYERWISE + IRREGULAR_STREAMED
FUSED_BWD_MAX_EDGES = 12 * 16                   # fused_backward_applies (csrc/aether_hip.hip): beyond, backward.h
EDGE_ACC_CASE = _a(3, 64, 6, 7)
EDGE_ACC_OPTIONS = (3, 0)                       # test_edge_level_weight_gradients_accumulated_in_the_edge_kernel
# narrow (zero-padded to 64), wide (k_wgemm backwards) and padded wide
_D3_SEEDS = {20: 6, 32: 6, 128: 5, 192: 9, 70: 5}
AETHER_WIDTHS = [c for H in (20, 32, 128, 192, 70) for c in (_a(2, H, 4, 20), _a(3, H, 2, 5, _D3_SEEDS[H]))]
DROPOUT_CASE = _a(3, 64, 6, 7, p=0.1)
_OTHER_SEEDS = {("LoCS", 3, 5): 7}
OTHER_CASES = [_a(D, 64, 2, N, _OTHER_SEEDS.get((f, D, N), 5), family=f) for f in ("LoCS", "DynamicFieldAether")
               for D in (2, 3) for N in (5, 20)]
STEP_CASES = AETHER_BOTH + AETHER_FUSED + AETHER_STREAMED + AETHER_WIDTHS + [DROPOUT_CASE] + OTHER_CASES + IRREGULAR_STEP_CASES
TEETH_CASE = AETHER_BOTH[0]


# ---- EGNN-Aether and the ClofNets: parameter gradients ------------------------------------------------------------------------
# (family name, layers, B, N, input seed, inputs): "runner" -- the Lorentz runner's batch, as the fixtures; "multigraph" --
# gnn_shape_checks.multigraph, 3 graphs of 7 nodes with repeated edges and uneven degrees (a partial node block)
GNN_FAMILIES = {f.name: f for f in (U.EGNN, U.CLOF, U.CLOF_VEL, U.CLOF_VEL_GBF)}
GNN_CASES = [(name, L, B, N, 5, kind) for name in GNN_FAMILIES
             for (L, B, N, kind) in ((2, 2, 5, "runner"), (2, 4, 5, "runner"), (3, 3, 7, "multigraph"))]


def gnn_cfg(case):
    name, L, B, N, seed, kind = case
    fam = GNN_FAMILIES[name]
    return fam.K.cfg(fam.model, 64, L, MODEL_SEED, N, norm_diff=True)


@functools.lru_cache(maxsize=None)
def gnn_case(case):
    """-> dict(cfg, sd, inp (fp32), g32, g64); a parameter that does not reach the output has None (ClofNet) or zeros
    (EGNN-Aether), as the restatements give them."""
    name, L, B, N, seed, kind = case
    fam, cfg = GNN_FAMILIES[name], gnn_cfg(case)
    sd = U.state_of(fam.K.build(cfg, "cpu"))
    inp = (ER.runner_batch(B, N, seed) if kind == "runner" else GC.random_multigraph(B, N, 300 + seed, dtype=torch.float32))
    def grads(i, dtype):
        sdd = {k: U._cast(v, dtype) for k, v in sd.items()}
        return fam.K.restate(sdd, {k: (v if k == "edges" else v.to(dtype)) for k, v in i.items()}, cfg)[1]

    with U.one_thread():
        g64 = grads(inp, torch.float64)
        g32 = [grads(reordered(inp, perm), torch.float32) for perm in edge_orders(inp["edges"][0].numel())]
    return dict(cfg=cfg, sd=sd, inp=inp, g64=g64, g32=g32)


def gnn_case_id(case):
    name, L, B, N, seed, kind = case
    return f"{name}-L{L}-B{B}N{N}-s{seed}-{kind}"


# ---- training through the device rollout ------------------------------------------------------------------------------------
ROLLOUT_STEPS, ROLLOUT_DT = 3, 1.0
MIN_MARGIN = 1e-4                               # rad from a branch cut, as tests/rollout_train_cases.py
# (family, D, B, N, input seed)
ROLLOUT_CASES = [(f, 2, 2, N, 6 if (f, N) == ("DynamicFieldAether", 20) else 5)
                 for f in ("Aether", "LoCS", "DynamicFieldAether") for N in (5, 20)]


def _rollout_fn(family, N):
    if family == "Aether":
        return O.rollout
    if family == "LoCS":
        return LR.rollout
    return lambda sd, x, v, e, q, steps, dt: DR.rollout(sd, x, v, e, q, steps, dt, N)


@functools.lru_cache(maxsize=None)
def rollout_case(case):
    """`rollout_train_cases.reference` (targets = the fp64 trajectory + 0.05 randn, loss = mean of the per-step MSE)
    -> dict(sd, inp, targets, g32, g64, traj64, margin); margin is None for LoCS, whose features have no field part."""
    family, D, B, N, seed = case
    sd = state_dict(family, D, 64)
    inp = make_batch(B, N, D, seed=seed)
    with U.one_thread():
        fn = _rollout_fn(family, N)
        ref = RT.reference(fn, sd, inp, ROLLOUT_STEPS, ROLLOUT_DT, seed)
        g32 = [ref["g32"]]
        for perm in list(edge_orders(inp["edges"][0].numel()))[1:]:
            g32.append(RT.rollout_grads(fn, sd, inp["x"], inp["vel"], [e[perm] for e in inp["edges"]], inp["charges"],
                                        ref["targets"], ROLLOUT_STEPS, ROLLOUT_DT, torch.float32)[0])
        ref["g32"] = g32
        margin = None
        sd64 = {k: v.double() for k, v in sd.items()}
        a = (sd64, inp["x"].double(), inp["vel"].double(), inp["edges"], inp["charges"].double(), ROLLOUT_STEPS, ROLLOUT_DT)
        with torch.no_grad():
            if family == "Aether":
                margin = float(O.rollout(*a, with_margin=True)[1].min())
            elif family == "DynamicFieldAether":
                margin = float(DR.rollout(*a, N, with_margin=True)[1].min())
    return dict(ref, sd=sd, margin=margin)


@functools.lru_cache(maxsize=None)
def rollout_emulated(case):
    family, D, B, N, seed = case
    c = rollout_case(case)
    inp = c["inp"]
    with U.one_thread(), split_backward():
        g, _ = RT.rollout_grads(_rollout_fn(family, N), c["sd"], inp["x"], inp["vel"], inp["edges"], inp["charges"],
                                c["targets"], ROLLOUT_STEPS, ROLLOUT_DT, torch.float64)
    return {k: v.float() for k, v in g.items()}


def rollout_case_id(case):
    family, D, B, N, seed = case
    return f"{family}-D{D}-B{B}N{N}-s{seed}-K{ROLLOUT_STEPS}"
