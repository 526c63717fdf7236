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
from aether_amd.synthetic import make_batch
from fused_cases import (call_model, fused_model, no_async_error, oracle_of, run_model, set_option, to_device,
                         uses_twelve_waves)
from fused_cases import options_restored  # noqa: F401  (autouse fixture: applies to the tests of this file)

pytestmark = pytest.mark.gpu
TOL = 1e-5


@functools.lru_cache(maxsize=None)
def _inputs(D, N, B, seed=0):
    return make_batch(B, N, D, seed=1600 + 100 * seed + 10 * N + D)


@functools.lru_cache(maxsize=None)
def _oracle(D, N, B):
    return oracle_of(load_state_dict(D), _inputs(D, N, B))


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
    d = to_device(_inputs(D, N, B))
    want = _oracle(D, N, B)
    m = fused_model(D)
    info = m.prepare_graph(d["edges"], B * N)[1]
    assert info.n_groups == 2 * B and info.reserved & 1 and uses_twelve_waves(info), (info.n_groups, info.reserved)
    set_option(b"fused_granules", 0)
    flag = run_model(m, d)
    set_option(b"fused_granules", 1)
    gran = run_model(m, d)
    again = run_model(m, d)
    err_g, err_f = scale_rel_err(gran.double(), want), scale_rel_err(flag.double(), want)
    print(f"D={D} N={N} B={B}: groups={info.n_groups} err granules={err_g:.2e} flag={err_f:.2e}")
    assert torch.isfinite(gran).all() and err_g <= TOL, err_g
    assert torch.isfinite(flag).all() and err_f <= TOL, err_f
    assert torch.equal(gran, flag)
    assert torch.equal(again, gran)
    no_async_error()


def test_sixteen_partner_rows_take_a_second_sweep():
    """One sweep covers 10 partner rows.  A sparse graph of 32 nodes, every node with ten in-edges (a ring, neighbours
    1..10), splits into 16 + 16 nodes of 160 in-edges = 10 tiles each: the 12-wave kernel with 16 partner rows."""
    D, N, B = 2, 32, 2
    inp = make_batch(B, N, D, seed=1632)
    rows, cols = inp["edges"]
    keep = ((cols - rows) % N >= 1) & ((cols - rows) % N <= 10) & (rows // N == cols // N)
    inp = dict(inp, edges=[rows[keep], cols[keep]], edge_attr=inp["edge_attr"][keep])
    want = oracle_of(load_state_dict(D), inp)
    d = to_device(inp)
    m = fused_model(D)
    info = m.prepare_graph(d["edges"], B * N)[1]
    assert info.n_groups == 2 * B and info.reserved & 1 and uses_twelve_waves(info) and info.max_group_nodes == 16, \
        (info.n_groups, info.reserved, info.max_group_nodes, info.max_group_edges)
    set_option(b"fused_granules", 0)
    flag = run_model(m, d)
    set_option(b"fused_granules", 1)
    outs = [run_model(m, d) for _ in range(4)]
    err = scale_rel_err(outs[0].double(), want)
    assert torch.isfinite(outs[0]).all() and err <= TOL, err
    for o in outs:
        assert torch.equal(o, flag)
    no_async_error()


def test_unsplit_twelve_wave_view_has_no_partner_and_no_granules():
    D, N, B = 2, 14, 2
    d = to_device(_inputs(D, N, B))
    m = fused_model(D)
    set_option(b"fused_split", 0)                       # read when the graph view is built
    info = m.prepare_graph(d["edges"], B * N)[1]
    set_option(b"fused_split", 1)
    assert info.n_groups == B and not info.reserved & 1 and uses_twelve_waves(info)
    set_option(b"fused_granules", 0)
    flag = run_model(m, d)
    set_option(b"fused_granules", 1)
    gran = run_model(m, d)
    err = scale_rel_err(gran.double(), _oracle(D, N, B))
    assert torch.isfinite(gran).all() and err <= TOL, err
    assert torch.equal(gran, flag)
    no_async_error()


def test_eight_tiles_stay_on_the_eight_wave_kernel_and_its_flag():
    D, N, B = 2, 16, 2
    d = to_device(_inputs(D, N, B))
    m = fused_model(D)
    info = m.prepare_graph(d["edges"], B * N)[1]
    assert info.n_groups == 2 * B and info.reserved & 1 and not uses_twelve_waves(info)
    outs = []
    for waves12, granules in ((0, 0), (1, 0), (1, 1), (0, 1)):
        set_option(b"fused_waves12", waves12)
        set_option(b"fused_granules", granules)
        outs.append(run_model(m, d))
    err = scale_rel_err(outs[2].double(), _oracle(D, N, B))
    assert torch.isfinite(outs[2]).all() and err <= TOL, err
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    no_async_error()


def test_fifty_calls_on_one_view_never_meet_a_stale_tag():
    D, N, B = 2, 20, 2
    m = fused_model(D)
    d = to_device(_inputs(D, N, B))
    first = run_model(m, d)
    assert scale_rel_err(first.double(), _oracle(D, N, B)) <= TOL
    outs = [call_model(m, d).clone() for _ in range(50)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert torch.equal(o.cpu(), first), k
    no_async_error()
    # the same view, other inputs in every call: what a fresh view (zeroed granules, first launch) gives for them
    variants = [to_device(_inputs(D, N, B, seed=s)) for s in range(1, 6)]
    fresh = [run_model(fused_model(D), v) for v in variants]
    for a in range(len(fresh)):
        for b in range(a):
            assert not torch.equal(fresh[a], fresh[b])            # the inputs do differ
    outs = [call_model(m, variants[k % len(variants)]).clone() for k in range(50)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert torch.equal(o.cpu(), fresh[k % len(variants)]), k
    no_async_error()


def test_the_two_protocols_interleaved_on_one_view():
    D, N, B = 2, 20, 3
    m = fused_model(D)
    d = to_device(_inputs(D, N, B))
    outs = []
    for k in range(8):
        set_option(b"fused_granules", 1 - k % 2)        # 1, 0, 1, 0, ...: each leaves the view armed for the other
        outs.append(run_model(m, d))
    assert scale_rel_err(outs[0].double(), _oracle(D, N, B)) <= TOL
    for k, o in enumerate(outs):
        assert torch.equal(o, outs[0]), k
    no_async_error()


def test_ten_captured_steps_replayed_five_times_equal_eager():
    D, N, B = 2, 20, 16
    m = fused_model(D)
    d = to_device(_inputs(D, N, B))
    eager = run_model(m, d)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            call_model(m, d)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = [call_model(m, d) for _ in range(10)]
    for rep in range(5):
        for o in outs:
            o.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            assert torch.equal(o.cpu(), eager), (rep, k)
    no_async_error()


def test_rollout_of_three_steps_equals_three_single_steps():
    D, N, B = 2, 20, 2
    d = to_device(_inputs(D, N, B))
    m = fused_model(D)
    assert uses_twelve_waves(m.prepare_graph(d["edges"], B * N)[1])
    whole = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    x, vel = d["x"], d["vel"]
    for t in range(3):
        nxt = m.rollout(x, vel, d["edges"], d["charges"], 1, 1.0)[0]
        assert torch.equal(nxt, whole[t]), t
        x, vel = nxt, (nxt - x) / 1.0          # the protocol's next velocity at dt = 1: one exact fp32 subtraction
    set_option(b"fused_granules", 0)
    flag = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    torch.cuda.synchronize()
    assert torch.isfinite(whole).all() and torch.equal(whole, flag)
    no_async_error()


def test_fifty_calls_next_to_large_copies_on_a_second_stream():
    """The flagship shape while another stream moves 1 GB per copy: some CUs and the fabric are busy, the two halves of a
    pair start apart.  A loaded machine, nothing more: no wait is meant to give up, and none may."""
    D, N, B = 2, 20, 128
    m = fused_model(D)
    d = to_device(_inputs(D, N, B))
    idle = run_model(m, d)
    assert torch.isfinite(idle).all()
    src = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(12):
            dst.copy_(src, non_blocking=True)
    outs = [call_model(m, d).clone() for _ in range(50)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert torch.equal(o.cpu(), idle), k
    no_async_error()
