"""k_fused on irregular graphs, every instance, on the update metric.  The schedule tests hold each new k_fused to the
older 8-wave kernel bit for bit, and irregular topologies to builder-against-builder equality or the position bar
(1e-5, about 5e-4 of the update): an edge summed into the wrong row with a small weight, or a lost lo piece, on a
receiver run across tiles, a partial tile, an empty workgroup, an uneven split or a packed group would pass all of them.
Here the graphs of tests/irregular_graphs.py run through every instance `fused_impl` can launch and are held by
`check_update` (tests/update_parity.py) to 4 x the floor of the fp32 CPU restatement on the same inputs.

A case is (graph, D, fused_split, fused_granules, fused_waves12, kind) with the instance it has to reach,
(NW, ROUNDS, KEEP, GRAN), and the layout of its graph view (split: two workgroups per group).  Both are asserted from
the `AetherGraphInfo` of the view the launch uses, through `fused_cases.fused_instance`, before the launch.
`fused_split` is read when the view is built, the other two at every launch.  Weights: the module built under
MODEL_SEED; seeds: tests/update_cases.py (IRREGULAR_SEEDS), held to their rule on the CPU by tests/test_update_metric.py.
Every case prints err, floor and their ratio before it asserts (pytest -s)."""
import pytest
import torch

import update_cases as U
from aether_amd import _lib
from fused_cases import fused_instance, no_async_error, set_option, tiles_of
from fused_cases import options_restored  # noqa: F401  (autouse fixture: applies to the tests of this file)
from update_parity import check_update

pytestmark = pytest.mark.gpu
FUSED, KEEP, STREAMED = _lib.FLAG_FORCE_FUSED, _lib.FLAG_KEEP_INTERMEDIATES, _lib.FLAG_FORCE_STREAMED
FLAGS = {"inference": FUSED, "keep": FUSED | KEEP, "streamed": STREAMED}
SPLIT, WHOLE = True, False                               # the layout of the view: two workgroups per group, or one
F, T = False, True


def _c(graph, D, kind, instance, layout, split=1, granules=1, waves12=1):
    return (graph, D, split, granules, waves12, kind, instance, layout)


# fmt: off
CASES = [
    # ---- the split view (the default)
    # groups of 2 .. 12 nodes packed from scenes of different sizes, workgroups of one node and one edge
    _c("knn_mixed_k4", 2, "inference", (8, 1, F, F), SPLIT),
    _c("knn_mixed_k4", 3, "keep",      (8, 1, T, F), SPLIT),
    _c("knn_mixed_k10", 3, "inference", (8, 1, F, F), SPLIT),
    _c("knn_mixed_k10", 2, "keep",      (8, 1, T, F), SPLIT),
    # 15 + 15 nodes, 165 edges per half: 11 tiles, the last one partial
    _c("knn_2x30_k11", 2, "inference", (12, 1, F, T), SPLIT),
    _c("knn_2x30_k11", 3, "inference", (12, 1, F, T), SPLIT),
    _c("knn_2x30_k11", 3, "inference", (12, 1, F, F), SPLIT, granules=0),
    _c("knn_2x30_k11", 2, "inference", (8, 2, F, F), SPLIT, waves12=0),
    _c("knn_2x30_k11", 2, "keep",      (8, 2, T, F), SPLIT),
    # the node cap, 16 + 16
    _c("knn_32_k10", 2, "inference", (12, 1, F, T), SPLIT),
    _c("knn_32_k10", 3, "inference", (12, 1, F, F), SPLIT, granules=0),
    # both caps: 12 full tiles per half
    _c("knn_2x32_k12", 3, "inference", (12, 1, F, T), SPLIT),
    _c("knn_2x32_k12", 2, "inference", (12, 1, F, F), SPLIT, granules=0),
    _c("knn_2x32_k12", 3, "inference", (8, 2, F, F), SPLIT, waves12=0),
    _c("knn_2x32_k12", 2, "keep",      (8, 2, T, F), SPLIT),
    # uneven halves of more than 16 nodes, a receiver run over several tiles, workgroups of one node and m = 0 beside them
    _c("multi32_hub40", 3, "inference", (8, 2, F, F), SPLIT),
    _c("multi32_hub40", 3, "keep",      (8, 2, T, F), SPLIT),
    _c("multi32_hub80", 2, "inference", (8, 2, F, F), SPLIT),
    _c("multi32_hub80", 3, "keep",      (8, 2, T, F), SPLIT),
    _c("multi16_E170", 2, "inference", (8, 1, F, F), SPLIT),
    # the granule launch with 6 + 8-node halves and two workgroups of one node and m = 0
    _c("multi16_E250", 2, "inference", (12, 1, F, T), SPLIT),
    _c("multi16_E250", 3, "inference", (12, 1, F, T), SPLIT),
    _c("multi16_E250", 2, "inference", (12, 1, F, F), SPLIT, granules=0),
    _c("multi16_E250", 3, "inference", (8, 2, F, F), SPLIT, waves12=0),
    _c("multi16_E250", 3, "keep",      (8, 2, T, F), SPLIT),
    # ---- fused_split = 0: one workgroup per group
    _c("knn_mixed_k10", 2, "inference", (8, 1, F, F), WHOLE, split=0),         # exactly 8 tiles
    _c("knn_mixed_k10", 3, "keep",      (8, 1, T, F), WHOLE, split=0),
    _c("knn_2x24_k7", 3, "inference", (8, 2, F, F), WHOLE, split=0),           # 11 tiles on 24 nodes
    _c("knn_2x24_k7", 2, "keep",      (8, 2, T, F), WHOLE, split=0),
    _c("knn_2x30_k11", 2, "inference", (8, 3, F, F), WHOLE, split=0),          # 21 tiles
    _c("knn_2x30_k11", 3, "keep",      (8, 3, T, F), WHOLE, split=0),
    _c("knn_2x32_k12", 2, "keep",      (8, 3, T, F), WHOLE, split=0),          # 24 tiles on 32 nodes
    _c("multi32_hub40", 2, "inference", (8, 3, F, F), WHOLE, split=0),
    _c("multi32_hub40", 3, "keep",      (8, 3, T, F), WHOLE, split=0),
    _c("multi32_hub80", 3, "inference", (8, 3, F, F), WHOLE, split=0),         # the edge cap, in-degree 86
    # the 12-wave kernel without a partner, next to a 2-node group without edges
    _c("multi16_E170", 2, "inference", (12, 1, F, F), WHOLE, split=0),
    _c("multi16_E170", 3, "inference", (12, 1, F, F), WHOLE, split=0),
    _c("multi16_E170", 2, "inference", (8, 2, F, F), WHOLE, split=0, waves12=0),
    _c("multi16_E170", 3, "keep",      (8, 2, T, F), WHOLE, split=0),
    _c("multi16_E250", 2, "inference", (8, 2, F, F), WHOLE, split=0),          # 16 tiles
    # ---- streamed, on the same view
    _c("knn_mixed_k4", 2, "streamed", None, SPLIT),
    _c("multi32_hub80", 3, "streamed", None, SPLIT),
    _c("multi16_E250", 2, "streamed", None, SPLIT),
]
# fmt: on


def _id(case):
    graph, D, split, granules, waves12, kind, instance, layout = case
    return f"{graph}-D{D}-{kind}-split{split}-gran{granules}-w12_{waves12}"


_REFS = {}


def _model_and_references(graph, D, steps=0):
    """A new module under MODEL_SEED (its first call builds a new graph view) and (x, want64, want32) from its state
    dict, computed once per (graph, D, steps) and not changed afterwards."""
    case = U.irregular_case(graph, D)
    m = U.IRREGULAR.build(case, "cuda").eval()
    sd = U.state_of(m)
    key = (graph, D, steps)
    if key not in _REFS:
        _REFS[key] = (sd, U.references_from(U.IRREGULAR, case, sd, steps))
    sd0, refs = _REFS[key]
    assert sd.keys() == sd0.keys() and all(torch.equal(sd[k], sd0[k]) for k in sd)
    return m, case, refs


def _view(m, g, split):
    set_option(b"fused_split", split)                   # read when the graph view is built
    info = m.prepare_graph(g["edges"], g["x"].shape[0])[1]
    set_option(b"fused_split", 1)
    return info


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_update_matches_fp64_at_the_fp32_floor(case):
    graph, D, split, granules, waves12, kind, instance, layout = case
    m, ucase, (x, want64, want32) = _model_and_references(graph, D)
    m.flags = FLAGS[kind]
    g = U.to_cuda(U.IRREGULAR.inputs(ucase))
    info = _view(m, g, split)
    assert info.n_groups > 0 and bool(info.reserved & 1) == layout, (info.n_groups, info.reserved)
    if kind != "streamed":
        got_instance = fused_instance(info, kind == "keep", waves12, granules)
        assert got_instance == instance, (got_instance, tiles_of(info), info.max_group_nodes, info.reserved)
    set_option(b"fused_granules", granules)             # read at every launch
    set_option(b"fused_waves12", waves12)
    with torch.no_grad():
        got = U.IRREGULAR.call(m, g, ucase)
        again = U.IRREGULAR.call(m, g, ucase)
    torch.cuda.synchronize()
    no_async_error()
    got, again = got.cpu(), again.cpu()
    what = f"{_id(case)} tiles={tiles_of(info)} nodes<={info.max_group_nodes} wgs={info.n_groups} instance={instance}"
    check_update(what, got, want32, x, want64)
    assert torch.equal(again, got)                      # two calls on the same inputs


def test_the_table_reaches_every_instance():
    """Every k_fused instance `fused_impl` can launch, for D 2 and 3, and both layouts of the view where an instance
    runs on both (three rounds need more than 16 tiles, which a split view never has)."""
    fused = [c for c in CASES if c[5] != "streamed"]
    reached = {(c[1],) + c[6] for c in fused}
    every = {(D, 8, r, k, F) for D in (2, 3) for r in (1, 2, 3) for k in (F, T)} | {(D, 12, 1, F, g) for D in (2, 3) for g in (F, T)}
    assert len(every) == 16 and reached == every, (sorted(every - reached), sorted(reached - every))
    for nw, rounds in ((8, 1), (8, 2), (12, 1)):
        layouts = {c[7] for c in fused if c[6][:2] == (nw, rounds)}
        assert layouts == {SPLIT, WHOLE}, (nw, rounds, layouts)
    assert {c[0] for c in CASES} == {g for g, _ in U.IRREGULAR_SEEDS}


@pytest.mark.parametrize("fc", U.IRREGULAR_ROLLOUT_CASES, ids=U.case_id)
def test_device_rollout_step_by_step(fc):
    """Five steps, each held on its increment as tests/test_gpu_update_parity.py::test_device_rollout_step_by_step: the
    edge attributes are derived on the device through `perm`, from a shuffled edge list with packed scenes
    (knn_mixed_k10) and with duplicated edges (multi16_E250)."""
    family_name, case = fc
    family = U.FAMILIES[family_name]
    m, case, (x, want64, want32) = _model_and_references(case[3], case[0], U.ROLLOUT_STEPS)
    m.flags = FUSED
    g = U.to_cuda(family.inputs(case))
    info = _view(m, g, 1)
    assert info.n_groups > 0 and info.reserved & 1
    with torch.no_grad():
        got = family.rollout(m, g, case, U.ROLLOUT_STEPS)
    torch.cuda.synchronize()
    no_async_error()
    got = got.cpu()
    assert got.shape == want64.shape
    prev = torch.cat([x.double()[None], want64[:-1]])
    for t in range(U.ROLLOUT_STEPS):
        check_update(f"{U.case_id(fc)} rollout step {t}", got[t], want32[t], prev[t], want64[t])
