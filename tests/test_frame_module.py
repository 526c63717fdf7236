"""nn/state2state/_frame.py on the CPU: the shared constructor checks, the reuse-flag decision of the inference workspace
and the block helpers that place a model in its kernel-width engine."""
import contextlib
import io

import pytest
import torch

from aether_amd import _lib
from aether_amd.nn.state2state import _frame as F
from aether_amd.nn.state2state.aether import Aether
from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
from aether_amd.nn.state2state.locs import LoCS, _locs_blocks, aether_state_dict

REUSED, PREPARED = _lib.FLAG_WORKSPACE_REUSED, _lib.FLAG_WEIGHTS_PREPARED
CLASSES = [(Aether, 3), (DynamicFieldAether, 3), (LoCS, 2)]


def quiet(cls, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return cls(*a, device="cpu", **k)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("cls,factor", CLASSES)
def test_constructor_rejections(cls, factor, D):
    bad = [((2 * D, 0, 0.0, D), r"hidden_size must lie in \[1, 4096\] \(experiments/lorentz/main.py:42-43\)"),
           ((2 * D, 4097, 0.0, D), r"hidden_size must lie in \[1, 4096\]"),
           ((2 * D, 64, 0.0, 4), r"num_dims must be 2 or 3 and input_size == 2\*num_dims"),
           ((2 * D + 1, 64, 0.0, D), r"num_dims must be 2 or 3 and input_size == 2\*num_dims"),
           ((2 * D, factor * D, 0.0, D), rf"hidden_size == {factor} \* num_dims is not supported \(the reference then builds "
                                         r"layer_1 without its res Linear, locs.py:214-218\)"),
           ((2 * D, 64, 1.0, D), r"dropout_prob must lie in \[0, 1\)"),
           ((2 * D, 64, -0.1, D), r"dropout_prob must lie in \[0, 1\)")]
    for args, msg in bad:
        with pytest.raises(ValueError, match=msg):
            quiet(cls, *args)
    other = 5 - factor                           # the width the other family rejects is fine here
    m = quiet(cls, 2 * D, other * D, 0.0, D)
    assert m.hidden_size == other * D and m._kw == 64
    with pytest.raises(_lib.AetherHipError, match=rf"aether_amd\.{cls.__name__} runs on an MI355X only; got a CPU tensor"):
        m.rollout(torch.zeros(4, D), torch.zeros(4, D), [torch.zeros(2, dtype=torch.long)] * 2, torch.zeros(4, 1), 1,
                  **({"num_nodes": 2} if cls is DynamicFieldAether else {}))


def test_reuse_flag_decision():
    W0, W1 = ((0, 0), (10, 11)), ((0, 1), (10, 11))          # parameter (versions, addresses); W1: one version bumped
    key = (0x1000, 100, 1900, 2, False, 0x2000)              # workspace, n_nodes, n_edges, D, keep, graph

    def run(calls, last=(None, None)):
        got = []
        for kw, n_groups, E, flags, k, w in calls:
            bits, last = F.reuse_flags(last, kw, n_groups, E, flags, k, w)
            got.append(bits)
        return got, last

    call = lambda k=key, w=W0, kw=64, n_groups=3, E=1900, flags=0: (kw, n_groups, E, flags, k, w)
    assert run([call(), call()])[0] == [0, REUSED | PREPARED]
    other_graph = key[:5] + (0x3000,)
    assert run([call(), call(other_graph), call(other_graph)])[0] == [0, 0, REUSED | PREPARED]
    assert run([call(), call(w=W1), call(w=W1)])[0] == [0, REUSED, REUSED | PREPARED]
    for changed in (0, 1, 2, 3, 4):                          # another buffer, shape or layout: neither
        k2 = tuple(v + 1 if i == changed else v for i, v in enumerate(key))
        assert run([call(), call(k2)])[0] == [0, 0], changed
    # the streamed kernels, the wide path, no edges, an ungrouped graph: neither flag, and nothing is remembered
    for off in (dict(flags=_lib.FLAG_FORCE_STREAMED), dict(kw=128), dict(E=0), dict(n_groups=0)):
        got, last = run([call(**off), call(**off)])
        assert got == [0, 0] and last == (None, None), off
        assert run([call(), call(**off), call()])[0] == [0, 0, 0], off
    # DynamicFieldAether refreshes its padded copies every call: never PREPARED
    assert DynamicFieldAether.WEIGHTS_PREPARED is False and Aether.WEIGHTS_PREPARED and LoCS.WEIGHTS_PREPARED
    got, last = run([call(w=None), call(w=None), call(w=None)])
    assert got == [0, REUSED, REUSED] and last == (key, None)


@pytest.mark.parametrize("H,kw", [(20, 64), (48, 64), (70, 128)])
@pytest.mark.parametrize("D", [2, 3])
def test_block_helpers(D, H, kw):
    assert F._kernel_width(H) == kw
    shapes = F.engine_shapes(D, kw)

    def image_of(model, blocks_of):
        img = {}
        for n, p in model.named_parameters():
            if n not in shapes:
                continue
            blocks = blocks_of(n, p.shape)
            img[n] = F.place(torch.zeros(shapes[n]), p.detach(), blocks)
            # place, then cut: every entry back, bit for bit
            assert torch.equal(F.cut(torch.full_like(p, float("nan")), img[n], blocks), p.detach()), n
            # exactly zero outside the blocks
            inside = torch.zeros(shapes[n], dtype=torch.bool)
            for _, ds in blocks:
                inside[ds] = True
            assert int(inside.sum()) == p.numel() and not img[n][~inside].any(), n
        assert set(img) == set(shapes)
        return img

    torch.manual_seed(5)
    pad = lambda n, shape: F._pad_blocks(n, shape, H, kw)
    a = quiet(Aether, 2 * D, H, 0.0, D)
    img = image_of(a, pad)
    eng = dict(a._sync_engine().named_parameters())
    for n, t in img.items():
        assert torch.equal(t, eng[n].detach()), n
    for n, p in a.named_parameters():                        # the field net goes over as it is
        if n not in shapes:
            assert torch.equal(eng[n].detach(), p.detach()), n
    d = quiet(DynamicFieldAether, 2 * D, H, 0.0, D)
    img = image_of(d, pad)
    padded = d._padded_gnn(torch.device("cpu"))
    assert set(padded) == set(img)
    for n, t in img.items():
        assert torch.equal(t, padded[n]), n
    grads = {n: torch.randn(d._kernel_shapes()[n]) for n, _ in d.named_parameters()}
    for (n, p), (n2, g) in zip(d.named_parameters(), d._narrow_grads(grads).items()):
        assert n == n2 and g.shape == p.shape
        assert torch.equal(g, F.cut(torch.empty_like(p), grads[n], pad(n, p.shape)) if n in shapes else grads[n]), n
    m = quiet(LoCS, 2 * D, H, 0.0, D)
    img = image_of(m, lambda n, shape: _locs_blocks(n, shape, D, H, kw))
    want = aether_state_dict(m.state_dict(), D, kw)
    for n, t in img.items():
        assert torch.equal(t, want[n]), n
    assert {n: tuple(t.shape) for n, t in want.items() if n not in shapes} == F.field_slot_shapes(D)
    assert all(not want[n].any() for n in F.field_slot_shapes(D))


def test_pad_blocks_against_a_hand_written_image():
    """H = 2 in a 4-wide engine, written out by hand: layers 2-4 read [x_send | x_recv | e], so the three 2-column blocks
    of message_fn.0.weight go to the starts of the three 4-column blocks; every other tensor sits top-left."""
    w = torch.tensor([[1., 2., 3., 4., 5., 6.],
                      [7., 8., 9., 10., 11., 12.]])
    want = torch.tensor([[1., 2., 0., 0., 3., 4., 0., 0., 5., 6., 0., 0.],
                         [7., 8., 0., 0., 9., 10., 0., 0., 11., 12., 0., 0.],
                         [0.] * 12,
                         [0.] * 12])
    for layer in (2, 3, 4):
        blocks = F._pad_blocks(f"gnn.layer_{layer}.message_fn.0.weight", w.shape, 2, 4)
        assert torch.equal(F.place(torch.zeros(4, 12), w, blocks), want)
        assert torch.equal(F.cut(torch.zeros(2, 6), want, blocks), w)
    # layer_1's first message layer reads edge features only, and an update MLP's 2H-wide tensors: top-left
    for name in ("gnn.layer_1.message_fn.0.weight", "gnn.layer_2.update_fn.0.weight", "field_net.net.0.weight"):
        blocks = F._pad_blocks(name, w.shape, 2, 4)
        top_left = torch.zeros(4, 12)
        top_left[:2, :6] = w
        assert torch.equal(F.place(torch.zeros(4, 12), w, blocks), top_left), name
    b = torch.tensor([1., 2.])
    assert torch.equal(F.place(torch.zeros(4), b, F._pad_blocks("gnn.layer_2.message_fn.0.bias", b.shape, 2, 4)),
                       torch.tensor([1., 2., 0., 0.]))


def test_narrow_rollout_syncs_its_engine_without_autograd():
    """rollout is an inference path from its first line: with autograd on, a narrow Aether must not take _sync_engine's
    training branch (a copy of every parameter per call, and the engine key dropped)."""
    a = quiet(Aether, 4, 20, 0.0, 2)
    with torch.no_grad():
        a._sync_engine()
    key = a._engine_key
    assert key is not None
    seen = []
    sync = a._sync_engine
    a.__dict__["_require_gpu"] = lambda x: None                       # the engine's own check still raises
    a.__dict__["_sync_engine"] = lambda: (seen.append(torch.is_grad_enabled()), sync())[1]
    assert torch.is_grad_enabled() and all(p.requires_grad for p in a.parameters())
    with pytest.raises(_lib.AetherHipError, match="got a CPU tensor"):
        a.rollout(torch.zeros(4, 2), torch.zeros(4, 2), [torch.zeros(2, dtype=torch.long)] * 2, torch.zeros(4, 1), 1)
    assert seen == [False] and a._engine_key == key


@pytest.mark.parametrize("H,keep,refused", [
    (64, False, {"efeat"}), (64, True, set()), (20, False, {"efeat"}),
    (128, False, {"e1", "e2", "e3", "e4"}), (128, True, set())])
def test_debug_fetch_refuses_a_layout_that_does_not_hold_the_tensor(H, keep, refused, monkeypatch):
    """aether_debug_fetch_h computes per-layer offsets from the training layout.  After a call that wrote the inference
    layout, the tensors whose offset differs there (WsLayout: the layer-1 features, which follow the forward prefix;
    WideLayout: the messages, which follow the first region sized by the layout) raise ValueError before any library call."""
    m = quiet(Aether, 4, H, 0.0, 2)
    eng = m.__dict__.get("_engine", m)
    assert eng._last_ws is None and eng._last_ws_keep is False
    with pytest.raises(ValueError, match="no forward has left a workspace"):
        eng.debug_fetch("x1", 3, 6, eng._kw)
    eng._last_ws, eng._last_ws_keep = torch.zeros(16, dtype=torch.uint8), keep

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    names = F.FrameModule.PER_LAYER + ("field", "R", "canon")
    assert len(F.FrameModule.PER_LAYER) == 9
    for name in names:
        if name in refused:
            with pytest.raises(ValueError, match="inference layout"):
                eng.debug_fetch(name, 3, 6, eng._kw)
        else:
            with pytest.raises(AssertionError, match="the library was reached"):
                eng.debug_fetch(name, 3, 6, eng._kw)
