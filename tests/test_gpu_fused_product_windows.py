"""k_fused, 12-wave kernels: the next layer's W_e and constants block are copied into LDS a whole edge phase ahead -- W_e(2)
with the prologue, layer 1's own image A into the P_s rows -- and only W2 is left for the node phase, issued by the waves
that are idle in step 2 (HISTORY R31).  The W_e e product of the next layer keeps its windows: step 3's on
waves 0-7, step 4's on waves 8-11 (the deals with a product in step 1's or step 2's window were measured and dropped).
Who copies what when changed; the operations did not.  Every GPU case asks the 12-wave dispatches (granules, and
`fused_granules` 0: rows + flag) for the bits of `fused_waves12` 0 on the same view, whose kernels the change does not
touch, compared as int32 so that NaNs count.

What the move can break: a wave without a tile that has to issue and wait for its fragments and reach every barrier
(N = 17: 9 tiles on 12 waves), a view without a partner (the deal of the fragments leaves one wave out either way), a
product that reads wA before this launch's image has landed (the previous launch's W_e(4) is there, or another model's),
a layer-1 tile that reads the P_s rows before its image A has landed (the previous launch's P_s rows of layer 4 are
there), a constants slot overwritten while its block is still read, the operand-scale branch of the product (its operand W_e now lands a layer earlier), and a
non-finite value that leaves its graph.
"""
import functools

import pytest
import torch

from conftest import load_state_dict, scale_rel_err
from aether_amd import _lib
from aether_amd.synthetic import make_batch
from fused_cases import TOL, call_model, fused_model, no_async_error, oracle_of, run_model, set_option, tiles_of, to_device
from fused_cases import uses_twelve_waves
from fused_cases import options_restored  # noqa: F401  (autouse fixture: applies to the tests of this file)


def test_layer_one_image_fits_the_ps_rows():
    """Layout: image A of layer 1 (W1 padded to K = 32: 2 terms x 4 row blocks x 64 lanes x 16 bytes) against the 32 P_s rows
    of 72 floats, through the library's own constexprs."""
    role = _lib.load().aether_debug_fused_wave_role
    image, rows = role(4, 0), role(4, 1)
    assert image == 2 * 4 * 64 * 16 == 8192 and rows == 32 * 72 * 4 and image <= rows


def test_every_wave_multiplies_in_one_window_beside_the_waves_that_work_there():
    role = _lib.load().aether_debug_fused_wave_role
    window = {w: role(3, w) for w in range(12)}
    assert set(window.values()) == {3, 4}                                  # nobody in step 1's or step 2's window
    assert [w for w, s in window.items() if s == 3] == list(range(8))      # step 3 runs on waves 8-11
    assert [w for w, s in window.items() if s == 4] == [8, 9, 10, 11]      # ... which are idle in step 4
    assert role(3, 12) == -1 and role(3, -1) == -1 and role(4, 2) == -1 and role(5, 0) == -1


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def three_ways(run):
    """(eight waves, twelve waves rows + flag, twelve waves granules)"""
    set_option(b"fused_waves12", 0)
    eight = run()
    set_option(b"fused_waves12", 1)
    set_option(b"fused_granules", 0)
    flag = run()
    set_option(b"fused_granules", 1)
    return eight, flag, run()


def twelve_wave_view(m, d, n_nodes, split=1):
    set_option(b"fused_split", split)                   # read when the graph view is built
    info = m.prepare_graph(d["edges"], n_nodes)[1]
    set_option(b"fused_split", 1)
    assert uses_twelve_waves(info) and bool(info.reserved & 1) == bool(split), (tiles_of(info), info.max_group_nodes)
    return info


# (D, N, B, fused_split, tiles of the largest workgroup).  N = 17: waves 9-11 own no tile and still issue, wait and reach
# every barrier; unsplit N = 14 and N = 12: no partner, the deal of the fragments is the same.
SHAPES = [(2, 17, 1, 1, 9), (2, 17, 3, 1, 9), (2, 19, 1, 1, 12), (2, 20, 2, 1, 12), (3, 20, 1, 1, 12), (2, 14, 2, 0, 12),
          (2, 12, 2, 0, 9)]


@pytest.mark.gpu
@pytest.mark.parametrize("D,N,B,split,tiles", SHAPES)
def test_shapes_give_the_eight_wave_kernels_bits(D, N, B, split, tiles):
    d = to_device(make_batch(B, N, D, seed=3100 + 10 * N + D + B))
    m = fused_model(D)
    info = twelve_wave_view(m, d, B * N, split)
    assert tiles_of(info) == tiles and info.n_groups == (2 * B if split else B)
    eight, flag, gran = three_ways(lambda: run_model(m, d))
    assert torch.isfinite(gran).all() and same_bits(gran, eight) and same_bits(flag, eight)
    no_async_error()


@pytest.mark.gpu
@pytest.mark.parametrize("granules", [1, 0])
def test_two_models_alternate_on_one_view(granules):
    """Two weight sets in turn on one view for 20 calls: the W_e(1) image in the P_s rows, W_e(2) in wA and constants block 2
    in slot 0 -- all in place when the first tile starts -- must be this launch's, not what the previous launch left there."""
    N, B = 20, 2
    d = to_device(make_batch(B, N, 2, seed=3110))
    sd_a = load_state_dict(2)
    g = torch.Generator().manual_seed(3111)
    sd_b = {k: v + 0.05 * v.abs().max() * torch.randn(v.shape, generator=g) for k, v in sd_a.items()}
    ma, mb = fused_model(2, sd=sd_a), fused_model(2, sd=sd_b)
    twelve_wave_view(ma, d, B * N)
    twelve_wave_view(mb, d, B * N)
    set_option(b"fused_waves12", 0)
    want = [run_model(ma, d), run_model(mb, d)]
    assert torch.isfinite(want[0]).all() and torch.isfinite(want[1]).all() and not same_bits(want[0], want[1])
    set_option(b"fused_waves12", 1)
    set_option(b"fused_granules", granules)
    outs = [call_model((ma, mb)[k & 1], d).clone() for k in range(20)]
    torch.cuda.synchronize()
    for k, o in enumerate(outs):
        assert same_bits(o.cpu(), want[k & 1]), k
    no_async_error()


@pytest.mark.gpu
def test_ten_captured_steps_replayed_five_times_equal_the_eight_wave_kernel():
    N, B = 20, 2
    d = to_device(make_batch(B, N, 2, seed=3120))
    m = fused_model(2)
    twelve_wave_view(m, d, B * N)
    set_option(b"fused_waves12", 0)
    eight = run_model(m, d)
    set_option(b"fused_waves12", 1)
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
            assert same_bits(o.cpu(), eight), (rep, k)
    no_async_error()


@pytest.mark.gpu
def test_rollout_of_three_steps_equals_three_single_steps():
    N, B = 20, 2
    d = to_device(make_batch(B, N, 2, seed=3130))
    m = fused_model(2)
    twelve_wave_view(m, d, B * N)
    whole = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    x, vel = d["x"], d["vel"]
    for t in range(3):
        nxt = m.rollout(x, vel, d["edges"], d["charges"], 1, 1.0)[0]
        assert same_bits(nxt, whole[t]), t
        x, vel = nxt, (nxt - x) / 1.0          # the protocol's next velocity at dt = 1: one exact fp32 subtraction
    set_option(b"fused_waves12", 0)
    eight = m.rollout(d["x"], d["vel"], d["edges"], d["charges"], 3, 1.0)
    torch.cuda.synchronize()
    assert torch.isfinite(whole).all() and same_bits(whole, eight)
    no_async_error()


# layer 1's message MLP with its first Linear (weight and bias) times 2^a and its second times 2^b, as in
# tests/test_gpu_fused_early_product.py: (9, 9) puts every edge's largest layer-1 message above 2^15, (0, -10) the largest
# message of all below 2^-6 -- the scale fallback of the product, whose weight image now lands a layer ahead.
@pytest.mark.gpu
@pytest.mark.parametrize("a,b", [(9, 9), (0, -10)])
def test_operand_scale_branch_of_the_product(a, b):
    D, N, B = 2, 20, 2
    inp = make_batch(B, N, D, seed=1800 + 10 * N + D)
    sd = {n: v.clone() for n, v in load_state_dict(D).items()}
    for lin, p2 in (("0", a), ("2", b)):
        sd[f"gnn.layer_1.message_fn.{lin}.weight"] *= 2.0 ** p2
        sd[f"gnn.layer_1.message_fn.{lin}.bias"] *= 2.0 ** p2
    rowmax = oracle_of(sd, inp, return_all=True)["e1"].abs().max(dim=1).values
    assert (rowmax.min() >= 2.0 ** 15) if a + b > 0 else (0 < rowmax.max() < 2.0 ** -6), (rowmax.min(), rowmax.max())
    d = to_device(inp)
    m = fused_model(D, sd=sd)
    twelve_wave_view(m, d, B * N)
    eight, flag, gran = three_ways(lambda: run_model(m, d))
    assert torch.isfinite(gran).all() and same_bits(gran, eight) and same_bits(flag, eight)
    no_async_error()


@pytest.mark.gpu
def test_nan_velocity_stays_in_its_graph():
    N = 17
    inp = make_batch(3, N, 2, seed=3140)
    m = fused_model(2)
    clean = run_model(m, to_device(inp))
    inp["vel"][N + 5, 1] = float("nan")                      # graph 1
    d = to_device(inp)
    twelve_wave_view(m, d, 3 * N)
    eight, flag, gran = three_ways(lambda: run_model(m, d))
    assert torch.isnan(gran[N:2 * N]).any() and same_bits(gran, eight) and same_bits(flag, eight)
    assert torch.isfinite(clean).all() and same_bits(gran[:N], clean[:N]) and same_bits(gran[2 * N:], clean[2 * N:])
    again = run_model(m, to_device(make_batch(3, N, 2, seed=3140)))
    assert same_bits(again, clean)                           # nothing non-finite stays behind in LDS or the view
    no_async_error()


@functools.lru_cache(maxsize=None)
def _oracle_case():
    inp = make_batch(2, 20, 2, seed=3150)
    return inp, oracle_of(load_state_dict(2), inp)


@pytest.mark.gpu
def test_one_shape_against_the_fp64_oracle():
    inp, want = _oracle_case()
    d = to_device(inp)
    m = fused_model(2)
    twelve_wave_view(m, d, 40)
    out = run_model(m, d)
    err = scale_rel_err(out.double(), want)
    print(f"N=20 B=2 granules: err={err:.2e}")
    assert torch.isfinite(out).all() and err <= TOL
    no_async_error()
