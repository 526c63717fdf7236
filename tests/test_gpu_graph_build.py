"""aether_graph_build_counting (csrc/graph_build.h) against the sorting builder aether_graph_build: the same graph view,
bit for bit.  Every comparison is exact -- integers, or torch.equal on floats: the view holds no float and decides the
order of every sum, so equal views give equal bits."""
import contextlib
import ctypes as C

import pytest
import torch

from conftest import load_state_dict
from aether_amd import _lib
from aether_amd.edges import get_edges
from aether_amd.nn.state2state.aether import Aether

pytestmark = pytest.mark.gpu
CAP = 1024            # csrc/graph_build.h GB_CAP: the longest in- or out-edge list the counting builder orders itself
EINVAL, EINDEX = -1, -2
INFO_FIELDS = [f for f, _ in _lib.AetherGraphInfo._fields_]


def _multigraph():
    """37 nodes, 200 edges: repeated edges, nodes without in-edges (7, 30, 31 among them), nodes without out-edges
    (32, 33), the last node receiving an edge."""
    g = torch.Generator().manual_seed(4)
    send = torch.randint(0, 32, (200,), generator=g)            # 32..36 send nothing ...
    recv = torch.randint(0, 30, (200,), generator=g)            # ... 30, 31 receive nothing
    recv[recv == 7] = 32 + (send[recv == 7] % 5)                # 32..36 receive
    send[:4], recv[:4] = torch.tensor([34, 35, 36, 3]), torch.tensor([1, 2, 3, 36])     # 34..36 send after all
    send[10:13], recv[10:13] = send[20:23].clone(), recv[20:23].clone()                 # repeated edges
    assert not (recv == 30).any() and not (recv == 31).any() and not (send == 32).any() and not (send == 33).any()
    assert (recv == 36).any()
    return send, recv, 37


def _knn_scenes(n_scenes=6, seed=9):
    """Scenes of 2-12 present objects, k = 10, each in its own numbering, concatenated with node offsets."""
    from aether_amd.knn import get_knn_graph_info
    g = torch.Generator().manual_seed(seed)
    sends, recvs, off = [], [], 0
    sizes = [2, 12] + [int(v) for v in torch.randint(2, 13, (n_scenes - 2,), generator=g)]
    for n in sizes:
        x = torch.randn(n, 2, generator=g).cuda()
        s, r = get_knn_graph_info(x, torch.ones(n, device="cuda"), num_vars=n, k=10)
        sends.append(s.cpu() + off); recvs.append(r.cpu() + off)
        off += n
    return torch.cat(sends), torch.cat(recvs), off


def _star(n_edges):
    """n_edges distinct senders, one receiver (node 0)."""
    return torch.arange(1, n_edges + 1), torch.zeros(n_edges, dtype=torch.int64), n_edges + 1


def _graphs():
    out = {}
    for name, (B, N) in (("a_B1N2", (1, 2)), ("b_B3N5", (3, 5)), ("c_B1N20", (1, 20))):
        s, r = get_edges(B, N)
        out[name] = (s, r, B * N)
    out["d_multigraph"] = _multigraph()
    s, r, n = out["b_B3N5"]
    out["e_reversed"] = (s.flip(0), r.flip(0), n)
    p = torch.randperm(s.numel(), generator=torch.Generator().manual_seed(5))
    out["e_shuffled"] = (s[p], r[p], n)
    out["f_knn"] = _knn_scenes()
    out["g_star_cap_plus_1"] = _star(CAP + 1)
    out["g_star_cap"] = _star(CAP)
    e = torch.empty(0, dtype=torch.int64)
    out["h_empty"] = (e, e.clone(), 7)
    return out


@pytest.fixture(scope="module")
def graphs():
    return {k: (s.cuda().contiguous(), r.cuda().contiguous(), n) for k, (s, r, n) in _graphs().items()}


GRAPH_NAMES = ["a_B1N2", "b_B3N5", "c_B1N20", "d_multigraph", "e_reversed", "e_shuffled", "f_knn", "g_star_cap_plus_1",
               "g_star_cap", "h_empty"]


def _build(entry, send, recv, n_nodes):
    """-> (status, buffer, info) of one builder into a buffer of its own."""
    lib = _lib.load()
    E = send.numel()
    buf = torch.zeros(max(lib.aether_graph_bytes(E, n_nodes), 256), dtype=torch.uint8, device="cuda")
    info = _lib.AetherGraphInfo()
    st = getattr(lib, entry)(send.data_ptr(), recv.data_ptr(), E, n_nodes, buf.data_ptr(), buf.numel(), C.byref(info),
                             torch.cuda.current_stream().cuda_stream)
    return st, buf, info


def _perm(buf, E, n_nodes):
    perm = torch.empty(E, dtype=torch.int32, device="cuda")
    if E == 0:                        # nothing to copy (and an empty tensor has no address to copy to)
        return perm.cpu()
    _lib.check(_lib.load().aether_graph_perm(buf.data_ptr(), E, n_nodes, perm.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream), "aether_graph_perm")
    torch.cuda.synchronize()
    return perm.cpu()


@contextlib.contextmanager
def _options(**kv):
    """Library options for the block; every one back to its default afterwards (all defaults here are 1)."""
    lib = _lib.load()
    try:
        for k, v in kv.items():
            _lib.check(lib.aether_set_option(k.encode(), v), "set_option")
        yield
    finally:
        for k in kv:
            _lib.check(lib.aether_set_option(k.encode(), 1), "set_option")


def test_library_exports_the_counting_builder():
    assert hasattr(_lib.load(), "aether_graph_build_counting")
    assert "aether_graph_build_counting" in _lib.SIGNATURES


@pytest.mark.parametrize("name", GRAPH_NAMES)
def test_both_builders_fill_the_same_info_and_order(graphs, name):
    send, recv, n = graphs[name]
    E = send.numel()
    st_old, buf_old, info_old = _build("aether_graph_build", send, recv, n)
    st_new, buf_new, info_new = _build("aether_graph_build_counting", send, recv, n)
    assert st_old == 0 and st_new == 0
    for f in INFO_FIELDS:
        assert getattr(info_old, f) == getattr(info_new, f), f
    assert info_new.n_nodes == n and info_new.n_edges == E
    perm_old, perm_new = _perm(buf_old, E, n), _perm(buf_new, E, n)
    assert torch.equal(perm_old, perm_new)
    # the stable sort by receiver, restated: ascending (receiver, edge id)
    assert torch.equal(perm_new.long(), torch.argsort(recv.cpu(), stable=True))
    lib = _lib.load()
    assert lib.aether_graph_matches(send.data_ptr(), recv.data_ptr(), E, n, buf_new.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream) == 1


def _state(n_nodes, send, recv, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_nodes, D, generator=g)
    vel = torch.randn(n_nodes, D, generator=g) * 0.5
    q = torch.randint(0, 2, (n_nodes, 1), generator=g).float() * 2 - 1
    s, r = send.cpu(), recv.cpu()
    ea = torch.cat([q[s] * q[r], (x[s] - x[r]).norm(dim=-1, keepdim=True)], dim=-1)
    return dict(h=vel.norm(dim=-1, keepdim=True), x=x, vel=vel, charges=q, edge_attr=ea, target=x + vel)


def _aether_run(D, send, recv, n, flags):
    """Forward and backward of a fresh Aether (the weights the runner's seed 1 gives; a graph cache of its own, so the
    view is built here) -> output, parameter gradients, x / vel / edge_attr gradients."""
    m = Aether(2 * D, 64, 0.0, D, device="cuda")
    m.load_state_dict(load_state_dict(D))
    m.flags = flags
    inp = {k: v.cuda() for k, v in _state(n, send, recv, D, seed=31).items()}
    leaves = [inp[k].requires_grad_(True) for k in ("x", "vel", "edge_attr")]
    out = m(inp["h"], inp["x"], [send, recv], inp["vel"], inp["edge_attr"], inp["charges"])
    torch.nn.functional.mse_loss(out, inp["target"]).backward()
    torch.cuda.synchronize()
    res = {"out": out.detach()}
    res.update({"grad." + k: p.grad.detach().clone() for k, p in m.named_parameters()})
    res.update({"dinput.%d" % i: t.grad.detach().clone() for i, t in enumerate(leaves)})
    return res


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("name", [n for n in GRAPH_NAMES if n != "h_empty"])
def test_aether_on_the_new_view_equals_aether_on_the_old_view(graphs, name, D, fused):
    """The regions without an accessor (send_s, recv_s, rowptr, the tile tables, the sender lists, the fused kernel's
    workgroup tables) through what reads them: outputs, parameter gradients and input gradients, with the fused kernels
    and with the layer-by-layer ones."""
    send, recv, n = graphs[name]
    opts = {} if fused else {"fused_backward": 0}
    flags = 0 if fused else _lib.FLAG_FORCE_STREAMED
    with _options(graph_build=0, **opts):
        old = _aether_run(D, send, recv, n, flags)
    with _options(graph_build=1, **opts):
        new = _aether_run(D, send, recv, n, flags)
    assert old.keys() == new.keys() and len(old) == 1 + 47 + 3
    for k in old:
        assert torch.isfinite(new[k]).all(), k
        assert torch.equal(old[k], new[k]), k


@pytest.mark.parametrize("name", ["b_B3N5", "d_multigraph", "h_empty"])
def test_egnn_aether_on_the_new_view_equals_the_old_view(graphs, name):
    """A drop-in of the parameter-gradient base (row-sorted view: the index rows swapped), forward and backward."""
    from test_egnn_aether import build
    send, recv, n = graphs[name]
    # (norm_diff off: the multigraph has self loops, whose zero-length difference has no finite normalised gradient)
    cfg = dict(seed=1, H=64, L=2, norm_diff=False, tanh=True, phi_scale=1.0, in_nf=1)

    def run():
        m = build(cfg, "cuda")
        inp = {k: v.cuda() for k, v in _state(n, send, recv, 3, seed=32).items()}
        out = m(inp["h"], inp["x"], [send, recv], inp["vel"], inp["edge_attr"], inp["charges"])
        torch.nn.functional.mse_loss(out, inp["target"]).backward()
        torch.cuda.synchronize()
        res = {"out": out.detach()}
        res.update({k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
        return res

    with _options(graph_build=0):
        old = run()
    with _options(graph_build=1):
        new = run()
    assert old.keys() == new.keys() and len(old) > 1
    for k in old:
        assert torch.isfinite(new[k]).all(), k
        assert torch.equal(old[k], new[k]), k


@pytest.mark.parametrize("name", ["d_multigraph", "f_knn"])
def test_twenty_builds_give_one_order(graphs, name):
    """The atomics arrive in any order; the view does not depend on it."""
    send, recv, n = graphs[name]
    first = None
    for _ in range(20):
        st, buf, _info = _build("aether_graph_build_counting", send, recv, n)
        assert st == 0
        perm = _perm(buf, send.numel(), n)
        first = perm if first is None else first
        assert torch.equal(perm, first)


@pytest.mark.parametrize("entry", ["aether_graph_build", "aether_graph_build_counting"])
@pytest.mark.parametrize("bad", ["n_nodes", "minus_one"])
@pytest.mark.parametrize("where", ["send", "recv"])
def test_bad_index_is_reported(graphs, entry, bad, where):
    send, recv, n = graphs["b_B3N5"]
    send, recv = send.clone(), recv.clone()
    (send if where == "send" else recv)[17] = n if bad == "n_nodes" else -1
    st, _buf, _info = _build(entry, send, recv, n)
    assert st == EINDEX
    assert b"edge index" in _lib.load().aether_last_error()
    torch.cuda.synchronize()                      # nothing is launched on the buffer after the error


def test_option_graph_build():
    lib = _lib.load()
    try:
        assert lib.aether_set_option(b"graph_build", 0) == 0
        assert lib.aether_set_option(b"graph_build", 1) == 0
        for v in (2, -1, 64):
            assert lib.aether_set_option(b"graph_build", v) == EINVAL
    finally:
        assert lib.aether_set_option(b"graph_build", 1) == 0
