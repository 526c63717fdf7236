"""k_fused's receiver sums: every lane adds one column of the wave's 16-row tile in row order and stores the sum after
the last row of a segment (consecutive rows with one receiver inside one run of the workgroup's local edge order).  The
GPU tests hold the inference and the save-for-backward kernel to the fp64 oracle at the project's scale-relative bars
(1e-5 forward, 5e-5 gradients) on graphs chosen for their segment structure; the CPU test restates the local order and
the segments per tile in plain Python and asserts that every case has the structure it is there for, and that the fp32
oracle itself stays below a quarter of each bar on that input.

The restatement follows the graph builder on a 256-CU device (groups = whole components, two workgroups per group while
there are at most 128 groups).  What it shows about two of the cases: three 5-node graphs are three SPLIT groups (one tile
of six and one of four 2-edge segments each, the run boundary inside the tile), and sixteen 2-node graphs are 32
workgroups of one edge each -- one graph per group at these batch sizes.  Several graphs per workgroup, 4-edge segments
across graphs and sixteen segments in one tile need a batch that fills the device: the cases `n5_b512` and `pairs_2048`
are there for that, next to the two small ones.  And 17-node graphs split into whole tiles (9 x 16 and 8 x 16 in-edges):
the padding rows behind the last segment are the 18-node case's."""
import functools

import pytest
import torch

from conftest import load_state_dict, scale_rel_err
from aether_amd.edges import prepare_edge_attr
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O
from fused_cases import KERNELS, fused_model, oracle_of, run_model, to_device

TOL = 1e-5
GTOL = 5e-5
CUS = 256                      # the device the grouping is restated for
MAX_NODES, MAX_EDGES = 32, 384


# ------------------------------------------------------------------------------------------------------- the cases
def _with_edges(inp, send, recv):
    inp = dict(inp)
    inp["edges"] = [send, recv]
    inp["edge_attr"] = prepare_edge_attr(inp["x"], inp["edges"], inp["charges"][send] * inp["charges"][recv])
    return inp


def _full(N, B, D, seed):
    return make_batch(B, N, D, seed=seed)


def _star(seed):
    """32 nodes, 31 senders into node 0: one component, one receiver with 31 in-edges."""
    inp = make_batch(1, 32, 2, seed=seed)
    return _with_edges(inp, torch.arange(1, 32), torch.zeros(31, dtype=torch.long))


def _dropped(N, seed):
    """Two complete graphs with ~30 % of the edges dropped, and every in-edge of node 3 of each graph."""
    inp = make_batch(2, N, 2, seed=seed)
    send, recv = inp["edges"]
    g = torch.Generator().manual_seed(seed)
    keep = torch.rand(send.numel(), generator=g) < 0.7
    keep &= (recv % N) != 3
    return _with_edges(inp, send[keep].clone(), recv[keep].clone())


CASES = {
    "n20_b2_d2": lambda: _full(20, 2, 2, 811),
    "n20_b2_d3": lambda: _full(20, 2, 3, 812),
    "n17_b2": lambda: _full(17, 2, 2, 813),
    "n18_b2": lambda: _full(18, 2, 2, 814),
    "n5_b3": lambda: _full(5, 3, 2, 815),
    "n5_b512": lambda: _full(5, 512, 2, 816),
    "pairs_16": lambda: _full(2, 16, 2, 817),
    "pairs_2048": lambda: _full(2, 2048, 2, 818),
    "star_31": lambda: _star(819),
    "dropped_n12": lambda: _dropped(12, 820),
    "dropped_n20": lambda: _dropped(20, 821),
    "n18_b130": lambda: _full(18, 130, 2, 822),
}
GRAD_CASES = ["n20_b2_d2", "n5_b3"]


@functools.lru_cache(maxsize=None)
def _case(name):
    return CASES[name]()


def _dims(inp):
    return inp["x"].shape[1]


@functools.lru_cache(maxsize=None)
def _want64(name):
    inp = _case(name)
    return oracle_of(load_state_dict(_dims(inp)), inp)


@functools.lru_cache(maxsize=None)
def _oracle_grads(name, double):
    """(output, parameter gradients of the MSE against the case's target) of the oracle in fp64 or fp32."""
    inp = _case(name)
    cast = (lambda t: t.double()) if double else (lambda t: t)
    sdg = {k: cast(v).clone().requires_grad_(True) for k, v in load_state_dict(_dims(inp)).items()}
    out = O.aether_forward(sdg, cast(inp["x"]), cast(inp["vel"]), inp["edges"], cast(inp["edge_attr"]), cast(inp["charges"]))
    torch.nn.functional.mse_loss(out, cast(inp["target"])).backward()
    return out.detach(), {k: v.grad for k, v in sdg.items()}


# ------------------------------------------------------------------- the builder and k_graph_tiles, in plain Python
def tile_structure(send, recv, n_nodes, cus=CUS):
    """Workgroups of the fused step and, per workgroup, its tiles as lists of segments (receiver, run, rows).
    Receiver-sorted stable edge order; components = node ranges that no edge crosses; groups pack whole components up to
    max(largest component, total / 256); a group is split over two workgroups by receiver range while 2 * groups <= cus
    (not beyond 16 tiles per half); a workgroup walks the edges whose sender it owns first, each run receiver-sorted."""
    send, recv = send.tolist(), recv.tolist()
    order = sorted(range(len(recv)), key=lambda k: recv[k])            # stable
    ssend, srecv = [send[k] for k in order], [recv[k] for k in order]
    rowptr = [0] * (n_nodes + 1)
    for r in recv:
        rowptr[r + 1] += 1
    for c in range(n_nodes):
        rowptr[c + 1] += rowptr[c]
    diff = [0] * (n_nodes + 2)
    for s, r in zip(send, recv):
        if s != r:
            diff[min(s, r) + 1] += 1
            diff[max(s, r) + 1] -= 1
    cross, acc = [], 0
    for c in range(n_nodes + 1):
        acc += diff[c]
        cross.append(acc)
    comps, c0 = [], 0
    while c0 < n_nodes:
        c1 = c0 + 1
        while c1 < n_nodes and cross[c1] != 0:
            c1 += 1
        comps.append((c0, c1))
        c0 = c1
    max_cn = max(b - a for a, b in comps)
    max_ce = max(rowptr[b] - rowptr[a] for a, b in comps)
    assert max_cn <= MAX_NODES and max_ce <= MAX_EDGES, "not a fused-step graph"
    tgt_n = min(max((n_nodes + 255) // 256, max_cn), MAX_NODES)
    tgt_e = min(max((len(recv) + 255) // 256, max_ce), MAX_EDGES)
    grp, gs = [0], 0
    for a, b in comps:
        if a > gs and (b - gs > tgt_n or rowptr[b] - rowptr[gs] > tgt_e):
            grp.append(a)
            gs = a
    grp.append(n_nodes)
    n_grp = len(grp) - 1
    split = 2 * n_grp <= cus and all(grp[k + 1] - grp[k] >= 2 for k in range(n_grp))

    def split_point(a, b):
        tot, best, nm = rowptr[b] - rowptr[a], -1, a + 1
        for c in range(a + 1, b):
            d = abs(2 * (rowptr[c] - rowptr[a]) - tot)
            if best < 0 or d < best:
                best, nm = d, c
        return nm

    while True:
        ranges = []
        for k in range(n_grp):
            a, b = grp[k], grp[k + 1]
            ranges += [(a, split_point(a, b)), (split_point(a, b), b)] if split else [(a, b)]
        if split and max(rowptr[e] - rowptr[b] for b, e in ranges) > 256:
            split = False
            continue
        break
    wgs = []
    for nb, ne in ranges:
        pos = list(range(rowptr[nb], rowptr[ne]))
        own = [k for k in pos if not split or nb <= ssend[k] < ne]
        oth = [k for k in pos if split and not nb <= ssend[k] < ne]
        local = [(srecv[k] - nb, 0) for k in own] + [(srecv[k] - nb, 1) for k in oth]
        tiles = []
        for t in range(0, len(local), 16):
            segs = []
            for j, key in enumerate(local[t:t + 16]):
                if segs and segs[-1][0] == key:
                    segs[-1][1].append(j)
                else:
                    segs.append((key, [j]))
            tiles.append(segs)
        wgs.append(dict(n=ne - nb, m=len(local), na=len(own), split=split, tiles=tiles,
                        indeg=[rowptr[c + 1] - rowptr[c] for c in range(nb, ne)]))
    return wgs


def _facts(name):
    inp = _case(name)
    wgs = tile_structure(inp["edges"][0], inp["edges"][1], inp["x"].shape[0])
    f = dict(split=wgs[0]["split"], workgroups=len(wgs), max_tiles=max(len(w["tiles"]) for w in wgs),
             max_segments=max((len(t) for w in wgs for t in w["tiles"]), default=0),
             single_segment_full_tile=any(len(t) == 1 and len(t[0][1]) == 16 for w in wgs for t in w["tiles"]),
             run_boundary_inside_tile=any(0 < w["na"] < w["m"] and w["na"] % 16 for w in wgs),
             padding_rows=any(w["m"] % 16 for w in wgs),
             zero_indegree=any(d == 0 for w in wgs for d in w["indeg"]),
             segment_lengths={len(s[1]) for w in wgs for t in w["tiles"] for s in t},
             max_nodes=max(w["n"] for w in wgs))
    # a receiver's run continues in the next tile: last segment of a tile and first of the next share (receiver, run)
    f["segment_spans_tiles"] = any(a[-1][0] == b[0][0] for w in wgs for a, b in zip(w["tiles"], w["tiles"][1:]))
    # partial rows stay inside the kernel's table: receiver + tile (+ n in the second run)
    for w in wgs:
        rows = 2 * 32 + 16 if len(w["tiles"]) <= 16 else 32 + 24
        for t, segs in enumerate(w["tiles"]):
            assert len(segs) <= 16
            for (rcv, run), _ in segs:
                assert rcv + t + (w["n"] if run else 0) < rows
    return f


def test_cases_have_the_structure_they_are_there_for():
    f = {name: _facts(name) for name in CASES}
    for name in ("n20_b2_d2", "n20_b2_d3"):      # 10 + 10 nodes, 190 in-edges each: runs of 9 and 10 rows
        assert f[name]["split"] and f[name]["workgroups"] == 4 and f[name]["max_tiles"] == 12, f[name]
        assert f[name]["max_segments"] <= 3 and f[name]["run_boundary_inside_tile"], f[name]
        assert f[name]["segment_spans_tiles"] and f[name]["segment_lengths"] >= {9, 10}, f[name]
    for name in ("n17_b2", "n18_b2"):            # 9 + 8 and 9 + 9 nodes: segments of 8 (of 8 and 9) rows
        assert f[name]["split"] and 8 < f[name]["max_tiles"] <= 16 and f[name]["run_boundary_inside_tile"], f[name]
    assert f["n18_b2"]["padding_rows"] and f["n18_b2"]["segment_spans_tiles"], f["n18_b2"]    # 153 rows in 10 tiles
    assert not f["n17_b2"]["padding_rows"], f["n17_b2"]                    # 144 and 128 rows: whole tiles only
    assert f["n5_b3"]["split"] and f["n5_b3"]["workgroups"] == 6 and f["n5_b3"]["max_tiles"] == 1, f["n5_b3"]
    assert f["n5_b3"]["max_segments"] == 6 and f["n5_b3"]["run_boundary_inside_tile"] and f["n5_b3"]["padding_rows"]
    g = f["n5_b512"]                             # two graphs per workgroup, 40 edges: segments of 4, tiles across graphs
    assert not g["split"] and g["workgroups"] == 256 and g["max_nodes"] == 10 and g["max_tiles"] == 3, g
    assert g["segment_lengths"] == {4} and g["max_segments"] == 4 and g["padding_rows"], g
    assert f["pairs_16"]["workgroups"] == 32 and f["pairs_16"]["max_segments"] == 1 and f["pairs_16"]["padding_rows"]
    g = f["pairs_2048"]                          # eight graphs per workgroup: every row of the tile its own segment
    assert not g["split"] and g["workgroups"] == 256 and g["max_segments"] == 16 and g["segment_lengths"] == {1}, g
    g = f["star_31"]                             # node 0 alone in its workgroup: 16 + 15 rows of one receiver
    assert g["split"] and g["max_tiles"] == 2 and g["max_segments"] == 1 and g["single_segment_full_tile"], g
    assert g["segment_spans_tiles"] and g["zero_indegree"] and g["padding_rows"], g
    for name in ("dropped_n12", "dropped_n20"):
        assert f[name]["zero_indegree"] and len(f[name]["segment_lengths"]) >= 4, f[name]
        assert f[name]["run_boundary_inside_tile"], f[name]
    g = f["n18_b130"]                            # 2 * 130 > 256: one workgroup per graph, 306 edges in 20 tiles
    assert not g["split"] and g["workgroups"] == 130 and g["max_tiles"] == 20 and g["segment_spans_tiles"], g


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_oracle_stays_below_a_quarter_of_the_forward_bar(name):
    inp = _case(name)
    with torch.no_grad():
        got = O.aether_forward(load_state_dict(_dims(inp)), inp["x"], inp["vel"], inp["edges"], inp["edge_attr"],
                               inp["charges"])
    err = scale_rel_err(got, _want64(name))
    print(f"{name}: fp32 oracle {err:.2e}")
    assert err <= TOL / 4, err


@pytest.mark.parametrize("name", GRAD_CASES)
def test_fp32_oracle_stays_below_a_quarter_of_the_gradient_bar(name):
    _, g64 = _oracle_grads(name, True)
    _, g32 = _oracle_grads(name, False)
    worst = max(scale_rel_err(g32[k], g64[k]) for k in g64)
    print(f"{name}: fp32 oracle gradients {worst:.2e}")
    assert worst <= GTOL / 4, worst


# ------------------------------------------------------------------------------------------------------ on the GPU


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["inference", "keep"])
@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_the_fp64_oracle(name, kernel):
    inp = _case(name)
    m = fused_model(_dims(inp), KERNELS[kernel])
    d = to_device(inp)
    info = m.prepare_graph(d["edges"], inp["x"].shape[0])[1]
    f = _facts(name)
    assert info.n_groups == f["workgroups"], (info.n_groups, f["workgroups"])      # the restatement is the builder's
    assert (info.max_group_edges + 15) // 16 == f["max_tiles"], (info.max_group_edges, f["max_tiles"])
    out = run_model(m, d)
    err = scale_rel_err(out.double(), _want64(name))
    print(f"{name} {kernel}: workgroups={info.n_groups} tiles={f['max_tiles']} err={err:.2e}")
    assert torch.isfinite(out).all() and err <= TOL, err


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAD_CASES)
def test_training_forward_and_gradients(name):
    inp = _case(name)
    want, g64 = _oracle_grads(name, True)
    m = fused_model(_dims(inp), KERNELS["inference"])
    m.zero_grad(set_to_none=True)
    d = to_device(inp)
    out = m(d["h"], d["x"], d["edges"], d["vel"], d["edge_attr"], d["charges"])
    torch.nn.functional.mse_loss(out, d["target"]).backward()
    torch.cuda.synchronize()
    assert scale_rel_err(out.detach().cpu().double(), want) <= TOL
    for k, p in m.named_parameters():
        err = scale_rel_err(p.grad.detach().cpu(), g64[k])
        assert err <= GTOL, (k, err)


@pytest.mark.gpu
def test_twenty_calls_are_bit_equal():
    inp = _case("n20_b2_d2")
    d = to_device(inp)
    for kernel, flags in KERNELS.items():
        m = fused_model(2, flags)
        first = run_model(m, d)
        for _ in range(19):
            assert torch.equal(run_model(m, d), first), kernel


@pytest.mark.gpu
def test_rollout_of_three_steps_equals_three_rollouts_of_one():
    inp = _case("n20_b2_d2")
    d = to_device(inp)
    m = fused_model(2, KERNELS["inference"])
    whole = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    x, vel = d["x"], d["vel"]
    for t in range(3):
        nxt = m.rollout(x, vel, d["edges"], d["charges"], 1, 1.0)[0]
        assert torch.equal(nxt, whole[t]), t
        x, vel = nxt, (nxt - x) / 1.0          # the protocol's next velocity at dt = 1: one exact fp32 subtraction
    torch.cuda.synchronize()
