"""EGNN-Aether (``--model egnn_aether``) at the shapes, graphs and autograd paths its first tests leave out: hidden 128 at depth, random multigraphs, a
hub, edge counts at the kernels' tile edges, no edges at all, in_node_nf > 1, the options at depth, and the flat gradient
buffer's plumbing (accumulation, frozen parameters, two forwards in flight, alternating batch sizes, a checkpoint load).
Every check is against the fp64 restatement at the project's bars (forward 1e-5, gradients 5e-5, max|a - b| / max|b|) or
bit for bit against a fresh module; tests/gnn_shape_checks.py holds the input sets and the checks."""
import pytest
import torch

from aether_amd.optim import FusedAdamW, mse_loss_grad
from aether_amd.training import GraphedTrainStep

import gnn_shape_checks as S
from gnn_shape_checks import Egnn as K

pytestmark = pytest.mark.gpu
MODELS = K.models
OPTION_NAMES = ["tanh", "norm"]          # recurrent=False and coords_weight != 1 are refused by the constructor


@pytest.mark.parametrize("model", MODELS)
def test_hidden_128_four_layers_B16_N20(model):
    """Hidden 128 with four layers had 3 x 7 nodes only.
    fp32 restatement vs fp64 on these inputs: forward 5.1e-07, gradients 8.0e-07."""
    cfg, inp = S.deep128(K, model)
    S.against_restatement(K, K.build(cfg, S.DEV), inp, cfg, layers=True)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("model", MODELS)
def test_random_multigraphs(model, H, seed):
    """Three graphs of 7 nodes with different edge counts: duplicate edges, nodes that are no edge's row, no edge's col
    or neither, rows in random order, 21 nodes (a partial block of NB = 4); odd seeds add a self loop (norm_diff off in
    the layers, as the self-loop test explains).
    fp32 restatement vs fp64 on these inputs: forward 3.4e-07, gradients 1.2e-05."""
    cfg, inp = S.multigraph(K, model, H, seed)
    row, col = inp["edges"]
    n = inp["x"].shape[0]
    deg_r, deg_c = torch.bincount(row, minlength=n), torch.bincount(col, minlength=n)
    assert int(((deg_r == 0) & (deg_c > 0)).sum()) >= 3 and int(((deg_c == 0) & (deg_r > 0)).sum()) >= 1
    assert int(((deg_r == 0) & (deg_c == 0)).sum()) >= 3 and n % 4 != 0
    assert torch.unique(torch.stack([row, col]), dim=1).shape[1] < row.numel() and not torch.equal(row, row.sort().values)
    assert len({int(((row >= 7 * b) & (row < 7 * b + 7)).sum()) for b in range(3)}) > 1
    assert int((row == col).sum()) == seed % 2
    S.against_restatement(K, K.build(cfg, S.DEV), inp, cfg, layers=True)


@pytest.mark.parametrize("last", [False, True], ids=["hub_first", "hub_last"])
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("model", MODELS)
def test_hub_of_degree_300(model, H, last):
    """301 nodes; one, at the first or the last node id, is the row of 300 edges, 75 groups of EB = 4 edges; other nodes have
    degree 1, 2, 3 and 5: a lone
    remainder group of 1, 2 and 3 edges, and a full group followed by a remainder of 1.
    fp32 restatement vs fp64 on these inputs: forward 8.3e-07, gradients 1.3e-06."""
    cfg, inp = S.hub(K, model, H, last)
    deg = S.GC.degrees(inp)
    assert int(deg[300 if last else 0]) == 300 and {1, 2, 3, 5} <= set(deg.tolist())
    S.against_restatement(K, K.build(cfg, S.DEV), inp, cfg, layers=True)


@pytest.mark.parametrize("E", S.TILE_E)
@pytest.mark.parametrize("model", MODELS)
def test_edge_counts_at_tile_edges_then_fewer_on_the_same_module(model, E):
    """E = 64 k and 128 k, each - 1 and + 1 (the weight-gradient chunks are 128 rows), by thinning a complete graph of 20 nodes; then E - 37 edges
    on the same module, bit for bit a fresh module's result: what the larger call left in the workspace is not read.
    fp32 restatement vs fp64 on these inputs: forward 3.0e-07, gradients 3.6e-06."""
    S.check_tile_edges(K, model, E)


@pytest.mark.parametrize("model", MODELS)
def test_edge_count_129_at_hidden_128(model):
    S.check_tile_edges(K, model, 129, H=128)


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("model", MODELS)
def test_no_edges_at_all(model, H):
    """An empty edge index: the output comes from the velocity term alone.  The reference runs it (the *_noedges
    fixtures): it leaves edge-side gradients zero, not None, and so must the kernels, exactly; the rest at the bars.
    fp32 restatement vs fp64 on these inputs: forward 1.6e-07, gradients 5.2e-07."""
    S.check_no_edges(K, model, H)


@pytest.mark.parametrize("in_nf,H", [(3, 64), (5, 128)])
@pytest.mark.parametrize("model", MODELS)
def test_wider_node_features(model, in_nf, H):
    """in_node_nf 3 and 5: the embedding in the prep kernel and its weight-gradient job (K = lda = in_node_nf).
    fp32 restatement vs fp64 on these inputs: forward 2.4e-07, gradients 3.5e-06."""
    cfg, inp = S.wide_h(K, model, in_nf, H)
    S.against_restatement(K, K.build(cfg, S.DEV), inp, cfg, layers=True)


@pytest.mark.parametrize("option", OPTION_NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_each_option_at_four_layers(model, option):
    """tanh=True and norm_diff=True, one at a time, B 2, N 5, four layers (the clamp at four layers is the fixture
    egnn_aether_B2N5_H64_L4_clamp, run by test_gpu_egnn_aether.py).
    fp32 restatement vs fp64 on these inputs: forward 5.0e-07, gradients 3.5e-06."""
    cfg, inp = S.options(K, model, [option])
    S.against_restatement(K, K.build(cfg, S.DEV), inp, cfg, layers=True)


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("model", MODELS)
def test_all_options_together_at_B16_N20(model, H):
    cfg, inp = S.options(K, model, OPTION_NAMES, 16, 20, H)
    S.against_restatement(K, K.build(cfg, S.DEV), inp, cfg, layers=True)


# ---- the flat gradient buffer behind torch.autograd ---------------------------------------------------------------------
@pytest.mark.parametrize("as_view", [True, False], ids=["grad_as_view", "grad_copies"])
@pytest.mark.parametrize("model", MODELS)
def test_gradient_accumulation_like_autograd(model, as_view):
    """Backward two and three times without zero_grad: .grad is the torch sum of the separately obtained gradients, bit
    for bit; zero_grad(set_to_none=False) then a step; some .grad replaced by foreign tensors before a backward."""
    S.check_accumulation(K, model, as_view)


@pytest.mark.parametrize("which", ["layer", "embedding"])
@pytest.mark.parametrize("model", MODELS)
def test_frozen_parameters(model, which):
    """gcl_1 or the embedding with requires_grad False: their .grad stays None, the others are the unfrozen run's."""
    S.check_frozen(K, model, which)


@pytest.mark.parametrize("first", ["a", "b"])
@pytest.mark.parametrize("model", MODELS)
def test_two_forwards_before_either_backward(model, first):
    """The second training forward finds the workspace busy and takes a fresh one: each backward, in either order, is
    its own single-forward result."""
    S.check_two_forwards(K, model, first)


@pytest.mark.parametrize("model", MODELS)
def test_alternating_batch_sizes_with_fresh_edge_tensors(model):
    """B 2 and B 32 in turn for ten steps: the workspace regrows, GraphCache looks up and evicts; every step is a fresh
    module's result bit for bit, the last one at the bars too.
    fp32 restatement vs fp64 on these inputs: forward 3.5e-07, gradients 1.6e-06."""
    S.check_alternating_sizes(K, model)


@pytest.mark.parametrize("model", MODELS)
def test_checkpoint_load_and_device_round_trip_between_steps(model):
    """load_state_dict of other weights between two steps, then .to('cpu') / .to('cuda'): the next step uses the new
    weights (the parameter-pointer cache follows), against the restatement and the other module."""
    S.check_checkpoint_load(K, model)


def test_graphed_train_step_at_hidden_128_four_layers():
    """As test_gpu_egnn_aether.py's captured-step test, at hidden 128 with four layers: three replays == three eager
    steps, losses and parameters bit for bit.  lr 1e-4: at the other test's 5e-4 the first AdamW steps overshoot at this
    width and depth (an fp64 run of the restatement with torch.optim.AdamW goes 0.080, 5.2, 0.41, 0.33; at 1e-4 it goes
    0.080, 0.089, 0.062, 0.015), and the test also wants the loss to fall."""
    cfg, inp = S.plain(K, "egnn_aether", 8, 121, H=128, L=4, N=20)
    g = S.dev(inp)
    args = K.step_args(g, cfg)
    m_eager, m_graph = K.build(cfg, S.DEV), K.build(cfg, S.DEV)
    opt = FusedAdamW(m_eager.parameters(), lr=1e-4, weight_decay=1e-12)
    eager_losses = []
    for _ in range(4):
        opt.zero_grad(set_to_none=True)
        out = m_eager(*args)
        loss, grad = mse_loss_grad(out, g["target"])
        out.backward(grad)
        opt.step()
        eager_losses.append(float(loss))
    step = GraphedTrainStep(m_graph, tuple(args), g["target"], lr=1e-4, weight_decay=1e-12, warmup=1)
    graph_losses = [float(step.step()) for _ in range(3)]
    step.check()
    assert graph_losses == eager_losses[1:], (graph_losses, eager_losses)
    for (k, p), q in zip(m_graph.named_parameters(), m_eager.parameters()):
        assert torch.equal(p.detach(), q.detach()), k
    assert eager_losses[-1] < eager_losses[0]

