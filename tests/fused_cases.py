"""What the tests/test_gpu_fused_*.py files share: the library options that pick a k_fused instance (and the fixture
that puts them back), the dispatch rule restated, a model on the GPU with the golden weights, one call of it, the same
call under the four dispatches `fused_waves12` {0, 1} x `fused_granules` {0, 1}, and the oracle on a dtype.  Inputs,
seeds, shapes and bars stay with the tests."""
import pytest
import torch

from conftest import load_state_dict, scale_rel_err
from aether_amd import _lib
from aether_amd.nn.state2state.aether import Aether
from oracle import aether_oracle as O

TOL = 1e-5                                               # the project's scale-relative forward bar
DISPATCHES = [(0, 0), (0, 1), (1, 0), (1, 1)]            # (fused_waves12, fused_granules)
KERNELS = {"inference": _lib.FLAG_FORCE_FUSED, "keep": _lib.FLAG_FORCE_FUSED | _lib.FLAG_KEEP_INTERMEDIATES}


def set_option(name, value):
    _lib.check(_lib.load().aether_set_option(name, value), "set_option")


@pytest.fixture(autouse=True)
def options_restored():
    """The options are back at their defaults after every test of the importing file, whatever it did."""
    try:
        yield
    finally:
        set_option(b"fused_granules", 1)
        set_option(b"fused_waves12", 1)
        set_option(b"fused_split", 1)


def tiles_of(info):
    return (info.max_group_edges + 15) // 16


def uses_twelve_waves(info):
    """The dispatch rule of fused_impl for an inference launch with fused_waves12 = 1."""
    return 9 <= tiles_of(info) <= 12 and info.max_group_nodes <= 16


def fused_instance(info, keep, waves12=1, granules=1):
    """The dispatch rule of fused_impl -> (NW, ROUNDS, KEEP, GRAN) of the k_fused instance a launch on this view runs.
    Twelve waves: not keeping, 9 .. 12 tiles, every workgroup within one node tile; the hand-off as granules where the
    view is split.  Otherwise eight waves with one, two or three rounds of edge tiles."""
    tiles, keep = tiles_of(info), bool(keep)
    if waves12 and not keep and 9 <= tiles <= 12 and info.max_group_nodes <= 16:
        return (12, 1, False, bool(granules and (info.reserved & 1)))
    return (8, 1 if tiles <= 8 else 2 if tiles <= 16 else 3, keep, False)


def oracle_of(sd, inp, dtype=torch.float64, **kw):
    c = lambda t: t.to(dtype)
    with torch.no_grad():
        return O.aether_forward({k: c(v) for k, v in sd.items()}, c(inp["x"]), c(inp["vel"]), inp["edges"],
                                c(inp["edge_attr"]), c(inp["charges"]), **kw)


def fused_model(D, flags=_lib.FLAG_FORCE_FUSED, sd=None):
    """A new module: its first call builds a new graph view (zeroed flags and granules)."""
    m = Aether(2 * D, 64, 0.0, D, device="cuda")
    m.load_state_dict(load_state_dict(D) if sd is None else sd)
    m.flags = flags
    return m


def to_device(inp):
    d = {k: v.cuda() for k, v in inp.items() if torch.is_tensor(v)}
    d["edges"] = [e.cuda() for e in inp["edges"]]
    return d


def call_model(m, d):
    with torch.no_grad():
        return m(d["h"], d["x"], d["edges"], d["vel"], d["edge_attr"], d["charges"])


def run_model(m, d):
    out = call_model(m, d)
    torch.cuda.synchronize()
    return out.cpu()


def four_ways(m, d):
    outs = []
    for waves12, granules in DISPATCHES:
        set_option(b"fused_waves12", waves12)
        set_option(b"fused_granules", granules)
        outs.append(run_model(m, d))
    set_option(b"fused_waves12", 1)
    set_option(b"fused_granules", 1)
    return outs


def no_async_error():
    assert _lib.load().aether_check_async_error() == 0


def check_four_ways(m, d, want, what, tol=TOL):
    outs = four_ways(m, d)
    for (waves12, granules), o in zip(DISPATCHES, outs):
        err = scale_rel_err(o.double(), want)
        print(f"{what} waves12={waves12} granules={granules}: err={err:.2e}")
        assert torch.isfinite(o).all() and err <= tol, (waves12, granules, err)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    no_async_error()
    return outs[0]
