"""ClofNet (``--model clof | clof_vel | clof_vel_gbf``) at the shapes, graphs and autograd paths its first tests leave out: hidden 128 at depth, random multigraphs, a
hub, edge counts at the kernels' tile edges, no edges at all, in_node_nf > 1, the options at depth, and the flat gradient
buffer's plumbing (accumulation, frozen parameters, two forwards in flight, alternating batch sizes, a checkpoint load).
Every check is against the fp64 restatement at the project's bars (forward 1e-5, gradients 5e-5, max|a - b| / max|b|) or
bit for bit against a fresh module; tests/gnn_shape_checks.py holds the input sets and the checks."""
import pytest
import torch

from aether_amd.training import GraphedTrainStep

import gnn_shape_checks as S
from gnn_shape_checks import Clof as K

pytestmark = pytest.mark.gpu
MODELS = K.models
OPTION_NAMES = ["norec", "cw", "tanh", "nonorm"]


@pytest.mark.parametrize("model", MODELS)
def test_hidden_128_four_layers_B16_N20(model):
    """k_clof_node<128, false, *> (node_mlp, the two-wave LayerNorm, node_proj feeding the next layer's P) and
    kb_clof_node<128, false> with xhat / rstd / glnw run only when hidden 128 has more than one layer.
    fp32 restatement vs fp64 on these inputs: forward 3.8e-07, gradients 3.9e-06."""
    cfg, inp = S.deep128(K, model)
    S.against_restatement(K, K.build(cfg, S.DEV), inp, cfg, layers=True)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("model", MODELS)
def test_random_multigraphs(model, H, seed):
    """Three graphs of 7 nodes with different edge counts: duplicate edges, nodes that are no edge's row, no edge's col
    or neither, rows in random order, 21 nodes (a partial block of NB = 4); odd seeds add a self loop (norm_diff off in
    the layers, as the self-loop test explains).
    fp32 restatement vs fp64 on these inputs: forward 3.8e-07, gradients 4.6e-06."""
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
    """301 nodes; one, at the first or the last node id, is the row of 300 edges: its rowptr segment spans three edge
    workgroups of ET = 128; other nodes have
    degree 1, 2, 3 and 5.
    fp32 restatement vs fp64 on these inputs: forward 6.5e-07, gradients 2.5e-06."""
    cfg, inp = S.hub(K, model, H, last)
    deg = S.GC.degrees(inp)
    assert int(deg[300 if last else 0]) == 300 and {1, 2, 3, 5} <= set(deg.tolist())
    S.against_restatement(K, K.build(cfg, S.DEV), inp, cfg, layers=True)


@pytest.mark.parametrize("E", S.TILE_E)
@pytest.mark.parametrize("model", MODELS)
def test_edge_counts_at_tile_edges_then_fewer_on_the_same_module(model, E):
    """E = 64 k and 128 k, each - 1 and + 1 (the prologue's 64 and the edge kernel's 128 edges per workgroup), by thinning a complete graph of 20 nodes; then E - 37 edges
    on the same module, bit for bit a fresh module's result: what the larger call left in the workspace is not read.
    fp32 restatement vs fp64 on these inputs: forward 2.9e-07, gradients 2.6e-06."""
    S.check_tile_edges(K, model, E)


@pytest.mark.parametrize("model", MODELS)
def test_edge_count_129_at_hidden_128(model):
    S.check_tile_edges(K, model, 129, H=128)


@pytest.mark.parametrize("H", [64, 128])
@pytest.mark.parametrize("model", MODELS)
def test_no_edges_at_all(model, H):
    """An empty edge index: the output comes from the velocity term alone.  The reference runs it (the *_noedges
    fixtures): it leaves edge-side gradients zero, not None, and so must the kernels, exactly; the rest at the bars.
    fp32 restatement vs fp64 on these inputs: forward 3.5e-07, gradients 7.9e-06."""
    S.check_no_edges(K, model, H)


@pytest.mark.parametrize("in_nf,H", [(3, 64), (5, 128)])
@pytest.mark.parametrize("model", MODELS)
def test_wider_node_features(model, in_nf, H):
    """in_node_nf 3 and 5: the embedding in the prep kernel and its weight-gradient job (K = lda = in_node_nf).
    fp32 restatement vs fp64 on these inputs: forward 2.6e-07, gradients 1.7e-06."""
    cfg, inp = S.wide_h(K, model, in_nf, H)
    S.against_restatement(K, K.build(cfg, S.DEV), inp, cfg, layers=True)


@pytest.mark.parametrize("option", OPTION_NAMES)
@pytest.mark.parametrize("model", MODELS)
def test_each_option_at_four_layers(model, option):
    """recurrent=False, coords_weight=0.5, tanh=True and norm_diff=False, one at a time, B 2, N 5, four layers.
    fp32 restatement vs fp64 on these inputs: forward 4.4e-07, gradients 5.2e-06."""
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
    fp32 restatement vs fp64 on these inputs: forward 3.8e-07, gradients 6.2e-06."""
    S.check_alternating_sizes(K, model)


@pytest.mark.parametrize("model", MODELS)
def test_checkpoint_load_and_device_round_trip_between_steps(model):
    """load_state_dict of other weights between two steps, then .to('cpu') / .to('cuda'): the next step uses the new
    weights (the parameter-pointer cache follows), against the restatement and the other module."""
    S.check_checkpoint_load(K, model)


def test_graphed_train_step_at_hidden_128_four_layers():
    """As test_gpu_clof.py's captured-step test, at hidden 128 with four layers: each replay computes the gradients an
    eager forward / backward computes from the same parameters; dead parameters keep .grad None and their values."""
    cfg, _ = S.plain(K, "clof_vel_gbf", 8, 0, H=128, L=4, N=20)
    batches = [S.dev(S.plain(K, "clof_vel_gbf", 8, 121 + i, H=128, L=4, N=20)[1]) for i in range(3)]
    graphed, eager = K.build(cfg, S.DEV), K.build(cfg, S.DEV)
    dead = K.dead(graphed)
    init = {k: v.detach().clone() for k, v in graphed.named_parameters()}
    step = GraphedTrainStep(graphed, K.step_args(batches[0], cfg), batches[0]["target"], lr=1e-3, weight_decay=1e-2)
    for b in batches:
        before = {k: v.detach().clone() for k, v in graphed.state_dict().items()}
        step.step(K.step_args(b, cfg), b["target"])
        torch.cuda.synchronize()
        eager.load_state_dict(before)
        _, ge = S.hip_step(K, eager, b, cfg)
        for k, p in graphed.named_parameters():
            if k in dead:
                assert p.grad is None and ge[k] is None, k
            else:
                # the captured step seeds the backward with aether_amd.optim.mse_loss_grad, the eager one through autograd
                assert S.rel(p.grad.cpu(), ge[k].cpu()) < 1e-6, k
                assert not torch.equal(p.detach(), before[k]), k
    step.check()
    for k, p in graphed.named_parameters():
        if k in dead:
            assert torch.equal(p.detach(), init[k]), k

