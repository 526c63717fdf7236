"""Gradient parity at the fp32 floor, per tensor.  The structural gradient tests hold every backward to
`scale_rel_err <= GTOL = 5e-5`, fifty times what three-term products of fp16 pieces give; one lost term of a
weight-gradient product passes that on every tensor (tests/test_grad_metric.py, on the CPU).  Here every parameter tensor,
and d/dx, d/dvel, d/dedge_attr (x0, vel0 of a rollout) where the model offers them, is held to
4 x max(its own floor, Q) (tests/grad_parity.py): the floor is the project's fp32 CPU restatement against fp64 on the
same inputs, the largest over eight orders of the edge list, and Q the upper quartile of the case's floors.  Loss: MSE (the rollouts: mean of the per-step MSE).

Cases, seeds and references: tests/grad_cases.py; the shapes are the smallest at which each backward kernel takes another
path.  Every test prints err, floor and err / bar per tensor before it asserts (pytest -s).

Not covered: the seq2seq models and the variable-N model have no backward here; k_adamw is held to torch at 2e-6
already (tests/test_gpu_training.py)."""
import pytest
import torch

import grad_cases as G
import update_cases as U
from aether_amd import _lib
from conftest import scale_rel_err
from gnn_shape_checks import dev as gnn_dev, hip_step
from grad_parity import check_grads, grad_ratios
from rollout_train_cases import step_loss

pytestmark = pytest.mark.gpu
GTOL = 5e-5                                          # tests/test_gpu_backward.py
FUSED, STREAMED = _lib.FLAG_FORCE_FUSED, _lib.FLAG_FORCE_STREAMED
PATHS = {"fused": FUSED, "streamed": STREAMED, "default": 0}
DEFAULT_EDGE_ACC = 3


def _set_option(name, value):
    _lib.check(_lib.load().aether_set_option(name, value), "set_option")


def _model(case, path, sd=None):
    family, D, H, B, N, seed, p, graph = case
    m = G.build(family, D, H, p, "cuda")
    m.load_state_dict(G.state_dict(family, D, H) if sd is None else sd)
    m.flags = PATHS[path]
    return m


def _step(m, case, inp, masks, g=None):
    """One forward / backward of MSELoss on the device -> {parameter | d/dx | d/dvel | d/dedge_attr: gradient}.  `g`: the
    inputs on the device, where the caller has them already."""
    family, N = case[0], case[4]
    g = U.to_cuda(inp) if g is None else g
    if masks is not None:
        m.train()
        m._dropout_masks = masks.cuda()
    m.zero_grad(set_to_none=True)
    leaves = {k: g[k].clone().requires_grad_(True) for k in G.INPUT_KEYS}
    if family == "Aether":
        out = m(g["h"], leaves["x"], g["edges"], leaves["vel"], leaves["edge_attr"], g["charges"])
    elif family == "LoCS":
        out = m(g["h"], leaves["x"], g["edges"], leaves["vel"], leaves["edge_attr"])
    else:
        out = m(None, leaves["x"], g["edges"], leaves["vel"], leaves["edge_attr"], g["charges"], N)
    torch.nn.functional.mse_loss(out, g["target"]).backward()
    torch.cuda.synchronize()
    _lib.check(_lib.load().aether_check_async_error(), "async")
    got = {k: p.grad.detach().cpu() for k, p in m.named_parameters()}
    got.update({G.INPUT_KEYS[k]: v.grad.detach().cpu() for k, v in leaves.items()})
    return got


def _check_step(case, path, tag="", prepare=None):
    """`prepare(m, inputs) -> inputs on the device`: called before the step, e.g. to build the graph view under an option."""
    r = G.step_case(case)
    m = _model(case, path)
    g = None if prepare is None else prepare(m, r["inp"])
    got = _step(m, case, r["inp"], r["masks"], g)
    return check_grads(f"{G.case_id(case)} {path}{tag}", got, r["g32"], r["g64"])


def _view_under(split, expect):
    """-> prepare(m, inp): builds the model's graph view with `fused_split` = split on the index tensors the step then
    runs on (it finds the view in the module's cache under these tensors) and asserts `expect(info)`."""
    def prepare(m, inp):
        g = U.to_cuda(inp)
        try:
            _set_option(b"fused_split", split)
            info = m.prepare_graph(g["edges"], inp["x"].shape[0])[1]
        finally:
            _set_option(b"fused_split", 1)
        assert info.n_groups > 0 and bool(info.reserved & 1) == bool(split), (info.n_groups, info.reserved)
        assert expect(info), (info.n_groups, info.max_group_nodes, info.max_group_edges, info.reserved)
        assert m.prepare_graph(g["edges"], inp["x"].shape[0])[1] is info
        return g
    return prepare


def _ids(cases):
    return [G.case_id(c) for c in cases]


@pytest.mark.parametrize("case", G.AETHER_BOTH + G.AETHER_FUSED, ids=_ids(G.AETHER_BOTH + G.AETHER_FUSED))
def test_aether_fused(case):
    """k_fused<KEEP> + k_fused_bwd + input_grad.h: several graphs per workgroup (B2N5), B6N7, two workgroups per graph with
    the hand-off (N = 20), the 12-wave layout (N = 18), one receiver for all edges, nodes without in-edges."""
    _check_step(case, "fused")


@pytest.mark.parametrize("case", G.AETHER_BOTH + G.AETHER_STREAMED, ids=_ids(G.AETHER_BOTH + G.AETHER_STREAMED))
def test_aether_streamed(case):
    """kb_node, kb_edge, kb_edge_acc8, kb_gather, kb_sum_g, k_outer + k_reduce_both; N = 70: degree above 64, the row sums
    run as their own kernel."""
    _check_step(case, "streamed")


@pytest.mark.parametrize("case", G.IRREGULAR_FUSED, ids=_ids(G.IRREGULAR_FUSED))
def test_aether_fused_on_irregular_graphs(case):
    """k_fused<KEEP> + k_fused_bwd on the graphs of tests/irregular_graphs.py: packed kNN scenes of 2 .. 12 nodes; 11 edge
    tiles in one workgroup (three tiles per wave) with a hub of in-degree 28, duplicated edges and an edge-less group;
    split halves of 11 tiles, the last one partial, with the hand-off."""
    split = G.IRREGULAR_FUSED_SPLIT[case[7]]
    tiles = {"knn_mixed_k10": lambda t: t <= 8, "multi16_E170": lambda t: t == 11, "knn_2x30_k11": lambda t: t == 11}[case[7]]
    fused_bwd = lambda info: info.max_group_edges <= G.FUSED_BWD_MAX_EDGES and tiles((info.max_group_edges + 15) // 16)
    _check_step(case, "fused", f" fused_split={split}", _view_under(split, fused_bwd))


@pytest.mark.parametrize("case", G.IRREGULAR_LAYERWISE, ids=_ids(G.IRREGULAR_LAYERWISE))
def test_aether_fused_forward_and_layerwise_backward_on_an_irregular_graph(case):
    """multi32_hub40 with `fused_split` off: 300 edges in one workgroup, more than 12 tiles, so `fused_backward_applies`
    is false -- k_fused<D, 8, 3, KEEP> and the layer-by-layer backward behind it."""
    layerwise = lambda info: info.max_group_edges > G.FUSED_BWD_MAX_EDGES
    _check_step(case, "fused", " fused_split=0", _view_under(0, layerwise))


@pytest.mark.parametrize("case", G.IRREGULAR_STREAMED, ids=_ids(G.IRREGULAR_STREAMED))
def test_aether_streamed_on_an_irregular_graph(case):
    """multi32_hub80: in-degree 86 on duplicated edges, the row sums as their own kernel."""
    _check_step(case, "streamed")


@pytest.mark.parametrize("edge_acc", G.EDGE_ACC_OPTIONS)
def test_aether_streamed_edge_level_weight_gradients(edge_acc):
    """Above `outer_defer_max_edges` (forced): the edge-level weight gradients accumulated in kb_edge_acc8's registers
    (edge_acc 3, the default) and from the row tensors through k_outer (0)."""
    try:
        _set_option(b"outer_defer_max_edges", 0)
        _set_option(b"edge_acc", edge_acc)
        _check_step(G.EDGE_ACC_CASE, "streamed", f" edge_acc={edge_acc}")
    finally:
        _set_option(b"outer_defer_max_edges", 1 << 20)
        _set_option(b"edge_acc", DEFAULT_EDGE_ACC)


@pytest.mark.parametrize("case", G.AETHER_WIDTHS, ids=_ids(G.AETHER_WIDTHS))
def test_aether_at_other_widths(case):
    """Hidden 20 and 32 (zero-padded to 64); 128, 192 and 70 (csrc/wide.h: k_wgemm backwards; 70 padded to 128)."""
    _check_step(case, "default")


@pytest.mark.parametrize("path", ["fused", "streamed"])
def test_aether_dropout_step_with_the_oracles_masks(path):
    """dropout_prob 0.1 in train() mode, the two out-MLP masks shared with the oracle."""
    _check_step(G.DROPOUT_CASE, path)


@pytest.mark.parametrize("path", ["fused", "streamed"])
@pytest.mark.parametrize("case", G.OTHER_CASES, ids=_ids(G.OTHER_CASES))
def test_locs_and_dynamic_field(case, path):
    _check_step(case, path)


@pytest.mark.parametrize("case", G.GNN_CASES, ids=[G.gnn_case_id(c) for c in G.GNN_CASES])
def test_egnn_aether_and_clofnets(case):
    """Parameter gradients at the fixtures' two smallest shapes and on gnn_shape_checks' multigraph."""
    r = G.gnn_case(case)
    K = G.GNN_FAMILIES[case[0]].K
    m = K.build(r["cfg"], "cuda")
    m.load_state_dict(r["sd"])
    _, g = hip_step(K, m, gnn_dev(r["inp"]), r["cfg"])
    got = {k: (None if v is None else v.detach().cpu()) for k, v in g.items()}
    check_grads(G.gnn_case_id(case), got, r["g32"], r["g64"])


@pytest.mark.parametrize("path", ["fused", "streamed"])
@pytest.mark.parametrize("case", G.ROLLOUT_CASES, ids=[G.rollout_case_id(c) for c in G.ROLLOUT_CASES])
def test_training_through_the_device_rollout(case, path):
    """rollout_bwd.h: three steps, parameters and the leaves x0, vel0."""
    family, D, B, N, seed = case
    r = G.rollout_case(case)
    inp = r["inp"]
    m = _model((family, D, 64, B, N, seed, 0.0, "full"), path)
    m.zero_grad(set_to_none=True)
    x0, v0 = inp["x"].cuda().requires_grad_(True), inp["vel"].cuda().requires_grad_(True)
    kw = dict(num_nodes=N) if family == "DynamicFieldAether" else {}
    traj = m.differentiable_rollout(x0, v0, [e.cuda() for e in inp["edges"]], inp["charges"].cuda(), G.ROLLOUT_STEPS,
                                    G.ROLLOUT_DT, **kw)
    step_loss(traj, r["targets"].to(device="cuda", dtype=torch.float32)).backward()
    torch.cuda.synchronize()
    _lib.check(_lib.load().aether_check_async_error(), "async")
    got = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}
    got["x0"], got["vel0"] = x0.grad.cpu(), v0.grad.cpu()
    assert scale_rel_err(traj.detach().cpu(), r["traj64"]) <= 1e-5
    check_grads(f"{G.rollout_case_id(case)} {path}", got, r["g32"], r["g64"])


@pytest.mark.parametrize("bits", [None, 16], ids=["fp16", "16_bits"])
def test_the_bar_sees_rounded_weights(bits):
    """The bar has teeth on the device, without touching a kernel: the model runs with every `gnn.*` weight matrix rounded
    to fp16 and back -- what a backward that lost every lo piece of W would use -- or to 16 significand bits, and is held
    to the fp64 gradients of the unrounded weights.  On the CPU the fp32 oracle on these weights is 820 and 18 bars out
    (tests/test_grad_metric.py); fp16 is coarse enough for GTOL to see it on most tensors, 16 bits pass GTOL on all."""
    case = G.TEETH_CASE
    r = G.step_case(case)
    got = _step(_model(case, "fused", G.rounded_weights(r["sd"], bits)), case, r["inp"], None)
    ratios, _ = grad_ratios(got, r["g32"], r["g64"])
    old = max(v[0] for v in ratios.values())
    print(f"rounded weights ({bits or 'fp16'}): worst scale_rel_err={old:.2e} (GTOL {GTOL:.0e}: "
          f"{sum(v[0] <= GTOL for v in ratios.values())} of {len(ratios)} tensors pass), "
          f"worst err/bar={max(v[2] for v in ratios.values()):.0f}")
    if bits is not None:
        assert old <= GTOL, old
    with pytest.raises(AssertionError):
        check_grads(f"{G.case_id(case)} fused, gnn.* weights rounded ({bits or 'fp16'})", got, r["g32"], r["g64"])
