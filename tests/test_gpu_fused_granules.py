"""k_fused<D, 12, 1, false> on a split view: the two workgroups of a group hand their P_s rows over as tagged 8-byte
granules {layer, value} (option `fused_granules` = 1, the default) instead of rows, a store drain and a flag (= 0, the
protocol of the 8-wave kernels); DESIGN.md 4.1, HISTORY R16.  The transport changed, the arithmetic did not: the two
settings must give the same bits everywhere, and each is held to the fp64 oracle at the project's scale-relative forward
bar (1e-5).

What can go wrong with granules is a tag that matches although its value is not this launch's: a granule left over from
an earlier launch (the re-arm at the end of a launch did not reach it), from the other protocol, or from an earlier
replay of a captured graph.  So the tests below run many launches on ONE view -- same inputs, changing inputs, the two
protocols interleaved, graph replays, a busy machine -- and compare bits with a launch that cannot have seen a stale
granule (a fresh view, or the flag protocol).
"""
import functools

import pytest
import torch

from conftest import load_state_dict, scale_rel_err
from aether_amd import _lib
from aether_amd.nn.state2state.aether import Aether
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _option(name, value):
    _lib.check(_lib.load().aether_set_option(name, value), "set_option")


@pytest.fixture(autouse=True)
def _options_restored():
    """The options are back at their defaults after every test of this file, whatever it did."""
    try:
        yield
    finally:
        _option(b"fused_granules", 1)
        _option(b"fused_waves12", 1)
        _option(b"fused_split", 1)


def _uses_twelve_waves(info):
    """The dispatch rule of fused_impl for an inference launch with fused_waves12 = 1."""
    tiles = (info.max_group_edges + 15) // 16
    return 9 <= tiles <= 12 and info.max_group_nodes <= 16


@functools.lru_cache(maxsize=None)
def _inputs(D, N, B, seed=0):
    return make_batch(B, N, D, seed=1600 + 100 * seed + 10 * N + D)


@functools.lru_cache(maxsize=None)
def _oracle(D, N, B):
    inp = _inputs(D, N, B)
    sd64 = {k: v.double() for k, v in load_state_dict(D).items()}
    with torch.no_grad():
        return O.aether_forward(sd64, inp["x"].double(), inp["vel"].double(), inp["edges"], inp["edge_attr"].double(),
                                inp["charges"].double())


def _model(D):
    """A new module: its first call builds a new graph view (zeroed flags and granules)."""
    m = Aether(2 * D, 64, 0.0, D, device="cuda")
    m.load_state_dict(load_state_dict(D))
    m.flags = _lib.FLAG_FORCE_FUSED
    return m


def _dev(inp):
    d = {k: v.cuda() for k, v in inp.items() if torch.is_tensor(v)}
    d["edges"] = [e.cuda() for e in inp["edges"]]
    return d


def _call(m, d):
    with torch.no_grad():
        return m(d["h"], d["x"], d["edges"], d["vel"], d["edge_attr"], d["charges"])


def _run(m, d):
    out = _call(m, d)
    torch.cuda.synchronize()
    return out.cpu()


def _no_async_error():
    assert _lib.load().aether_check_async_error() == 0


def test_option_takes_zero_and_one_only():
    lib = _lib.load()
    assert lib.aether_set_option(b"fused_granules", 2) != 0
    assert lib.aether_set_option(b"fused_granules", -1) != 0
    assert lib.aether_set_option(b"fused_granules", 0) == 0
    assert lib.aether_set_option(b"fused_granules", 1) == 0


# split pairs at the smallest batches at which one exists; odd batches put the halves of a pair at other distances
@pytest.mark.parametrize("B", [1, 2, 3, 16])
@pytest.mark.parametrize("D,N", [(2, 20), (3, 20), (2, 17), (2, 18)])
def test_granules_and_flag_give_the_same_bits_and_match_the_oracle(D, N, B):
    d = _dev(_inputs(D, N, B))
    want = _oracle(D, N, B)
    m = _model(D)
    info = m.prepare_graph(d["edges"], B * N)[1]
    assert info.n_groups == 2 * B and info.reserved & 1 and _uses_twelve_waves(info), (info.n_groups, info.reserved)
    _option(b"fused_granules", 0)
    flag = _run(m, d)
    _option(b"fused_granules", 1)
    gran = _run(m, d)
    again = _run(m, d)
    err_g, err_f = scale_rel_err(gran.double(), want), scale_rel_err(flag.double(), want)
    print(f"D={D} N={N} B={B}: groups={info.n_groups} err granules={err_g:.2e} flag={err_f:.2e}")
    assert torch.isfinite(gran).all() and err_g <= TOL, err_g
    assert torch.isfinite(flag).all() and err_f <= TOL, err_f
    assert torch.equal(gran, flag)
    assert torch.equal(again, gran)
    _no_async_error()


def test_sixteen_partner_rows_take_a_second_sweep():
    """One sweep covers 10 partner rows.  A sparse graph of 32 nodes, every node with ten in-edges (a ring, neighbours
    1..10), splits into 16 + 16 nodes of 160 in-edges = 10 tiles each: the 12-wave kernel with 16 partner rows."""
    D, N, B = 2, 32, 2
    inp = make_batch(B, N, D, seed=1632)
    rows, cols = inp["edges"]
    keep = ((cols - rows) % N >= 1) & ((cols - rows) % N <= 10) & (rows // N == cols // N)
    inp = dict(inp, edges=[rows[keep], cols[keep]], edge_attr=inp["edge_attr"][keep])
    sd64 = {k: v.double() for k, v in load_state_dict(D).items()}
    with torch.no_grad():
        want = O.aether_forward(sd64, inp["x"].double(), inp["vel"].double(), inp["edges"], inp["edge_attr"].double(),
                                inp["charges"].double())
    d = _dev(inp)
    m = _model(D)
    info = m.prepare_graph(d["edges"], B * N)[1]
    assert info.n_groups == 2 * B and info.reserved & 1 and _uses_twelve_waves(info) and info.max_group_nodes == 16, \
        (info.n_groups, info.reserved, info.max_group_nodes, info.max_group_edges)
    _option(b"fused_granules", 0)
    flag = _run(m, d)
    _option(b"fused_granules", 1)
    outs = [_run(m, d) for _ in range(4)]
    err = scale_rel_err(outs[0].double(), want)
    assert torch.isfinite(outs[0]).all() and err <= TOL, err
    for o in outs:
        assert torch.equal(o, flag)
    _no_async_error()


def test_unsplit_twelve_wave_view_has_no_partner_and_no_granules():
    D, N, B = 2, 14, 2
    d = _dev(_inputs(D, N, B))
    m = _model(D)
    _option(b"fused_split", 0)                           # read when the graph view is built
    info = m.prepare_graph(d["edges"], B * N)[1]
    _option(b"fused_split", 1)
    assert info.n_groups == B and not info.reserved & 1 and _uses_twelve_waves(info)
    _option(b"fused_granules", 0)
    flag = _run(m, d)
    _option(b"fused_granules", 1)
    gran = _run(m, d)
    err = scale_rel_err(gran.double(), _oracle(D, N, B))
    assert torch.isfinite(gran).all() and err <= TOL, err
    assert torch.equal(gran, flag)
    _no_async_error()


def test_eight_tiles_stay_on_the_eight_wave_kernel_and_its_flag():
    D, N, B = 2, 16, 2
    d = _dev(_inputs(D, N, B))
    m = _model(D)
    info = m.prepare_graph(d["edges"], B * N)[1]
    assert info.n_groups == 2 * B and info.reserved & 1 and not _uses_twelve_waves(info)
    outs = []
    for waves12, granules in ((0, 0), (1, 0), (1, 1), (0, 1)):
        _option(b"fused_waves12", waves12)
        _option(b"fused_granules", granules)
        outs.append(_run(m, d))
    err = scale_rel_err(outs[2].double(), _oracle(D, N, B))
    assert torch.isfinite(outs[2]).all() and err <= TOL, err
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    _no_async_error()


def test_fifty_calls_on_one_view_never_meet_a_stale_tag():
    D, N, B = 2, 20, 2
    m = _model(D)
    d = _dev(_inputs(D, N, B))
    first = _run(m, d)
    assert scale_rel_err(first.double(), _oracle(D, N, B)) <= TOL
    outs = [_call(m, d).clone() for _ in range(50)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert torch.equal(o.cpu(), first), k
    _no_async_error()
    # the same view, other inputs in every call: what a fresh view (zeroed granules, first launch) gives for them
    variants = [_dev(_inputs(D, N, B, seed=s)) for s in range(1, 6)]
    fresh = [_run(_model(D), v) for v in variants]
    for a in range(len(fresh)):
        for b in range(a):
            assert not torch.equal(fresh[a], fresh[b])            # the inputs do differ
    outs = [_call(m, variants[k % len(variants)]).clone() for k in range(50)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert torch.equal(o.cpu(), fresh[k % len(variants)]), k
    _no_async_error()


def test_the_two_protocols_interleaved_on_one_view():
    D, N, B = 2, 20, 3
    m = _model(D)
    d = _dev(_inputs(D, N, B))
    outs = []
    for k in range(8):
        _option(b"fused_granules", 1 - k % 2)            # 1, 0, 1, 0, ...: each leaves the view armed for the other
        outs.append(_run(m, d))
    assert scale_rel_err(outs[0].double(), _oracle(D, N, B)) <= TOL
    for k, o in enumerate(outs):
        assert torch.equal(o, outs[0]), k
    _no_async_error()


def test_ten_captured_steps_replayed_five_times_equal_eager():
    D, N, B = 2, 20, 16
    m = _model(D)
    d = _dev(_inputs(D, N, B))
    eager = _run(m, d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _call(m, d)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = [_call(m, d) for _ in range(10)]
    for rep in range(5):
        for o in outs:
            o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            assert torch.equal(o.cpu(), eager), (rep, k)
    _no_async_error()


def test_rollout_of_three_steps_equals_three_single_steps():
    D, N, B = 2, 20, 2
    d = _dev(_inputs(D, N, B))
    m = _model(D)
    assert _uses_twelve_waves(m.prepare_graph(d["edges"], B * N)[1])
    whole = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    x, vel = d["x"], d["vel"]
    for t in range(3):
        nxt = m.rollout(x, vel, d["edges"], d["charges"], 1, 1.0)[0]
        assert torch.equal(nxt, whole[t]), t
        x, vel = nxt, (nxt - x) / 1.0          # the protocol's next velocity at dt = 1: one exact fp32 subtraction
    _option(b"fused_granules", 0)
    flag = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    torch.cuda.synchronize()
    assert torch.isfinite(whole).all() and torch.equal(whole, flag)
    _no_async_error()


def test_fifty_calls_next_to_large_copies_on_a_second_stream():
    """The flagship shape while another stream moves 1 GB per copy: some CUs and the fabric are busy, the two halves of a
    pair start apart.  A loaded machine, nothing more: no wait is meant to give up, and none may."""
    D, N, B = 2, 20, 128
    m = _model(D)
    d = _dev(_inputs(D, N, B))
    idle = _run(m, d)
    assert torch.isfinite(idle).all()
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(12):
            dst.copy_(src, non_blocking=True)
    outs = [_call(m, d).clone() for _ in range(50)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert torch.equal(o.cpu(), idle), k
    _no_async_error()
