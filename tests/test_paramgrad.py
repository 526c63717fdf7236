"""The plumbing the parameter-gradient drop-ins share (aether_amd/nn/state2state/_paramgrad.py, aether._hand_over_grads),
on CPU tensors: what autograd gets back for each state a parameter's .grad can be in, and the flat gradient buffer's
layout.  The kernels behind it: tests/test_gpu_egnn_aether.py, tests/test_gpu_clof.py."""
import contextlib
import io

import pytest
import torch
import torch.nn as nn

from aether_amd.nn.state2state import _paramgrad as P
from aether_amd.nn.state2state.aether import _hand_over_grads
from aether_amd.nn.state2state.clof import ClofNet_vel_gbf
from aether_amd.nn.state2state.egnn_aether import EGNN_vel_Aether


class Stub(nn.Module):
    """Five parameters of sizes that need padding, and the attributes the helpers read."""

    def __init__(self):
        super().__init__()
        self.w = nn.ParameterList([nn.Parameter(torch.zeros(s)) for s in ((3, 5), (7,), (1,), (2, 2), (6,))])
        self.dp_group = None
        self.grad_as_view = True
        self._gbuf = self._gbuf2 = None

    def _param_list(self):
        return list(self.parameters())


def filled(module, second, base):
    flat, views = P._flat_grad_buffers(module, second)
    flat.copy_(torch.arange(flat.numel(), dtype=torch.float32) + base)
    return flat, views


def test_hand_over_covers_every_state_of_grad():
    m = Stub()
    plist = m._param_list()
    flat, views = filled(m, False, 100.0)
    flat2, views2 = filled(m, True, 1000.0)
    before = [v.clone() for v in views]

    # first backward: nothing aliased, the kernels wrote into the first buffer
    foreign = torch.full_like(plist[1], 5.0)
    plist[1].grad = foreign
    out = _hand_over_grads(m, plist, views, flat, views, False, [True, True, False, True, True], skip={3})
    assert out[0] is None and plist[0].grad is views[0]                       # unset .grad: the view itself
    assert torch.equal(out[1], views[1]) and out[1].data_ptr() != views[1].data_ptr()      # foreign .grad: a clone back
    assert plist[1].grad is foreign and torch.equal(foreign, torch.full_like(foreign, 5.0))
    assert out[2] is None and plist[2].grad is None                           # need = False
    assert out[3] is None and plist[3].grad is None                           # in the skip set
    assert out[4] is None and plist[4].grad is views[4]
    assert all(torch.equal(v, b) for v, b in zip(views, before))              # nothing was added anywhere

    # second backward without zero_grad: .grad of 0 and 4 alias the first buffer, the kernels wrote into the second
    out = _hand_over_grads(m, plist, views, flat2, views2, True, [True, True, False, True, True], skip={3})
    assert out[0] is None and plist[0].grad is views[0] and torch.equal(views[0], before[0] + views2[0])
    assert out[4] is None and torch.equal(views[4], before[4] + views2[4])
    assert torch.equal(out[1], views2[1]) and out[1].data_ptr() != views2[1].data_ptr()
    assert torch.equal(views[1], before[1])                                   # a foreign .grad's slot is not touched
    assert out[2] is None and plist[2].grad is None
    assert out[3] is None and plist[3].grad is None and torch.equal(views[3], before[3])


def test_hand_over_without_the_skip_set_is_unchanged():
    """Aether and LoCS call it without ``skip``: every needed parameter gets its view."""
    m = Stub()
    plist = m._param_list()
    flat, views = filled(m, False, 1.0)
    out = _hand_over_grads(m, plist, views, flat, views, False, [True] * 5)
    assert out == [None] * 5 and all(p.grad is v for p, v in zip(plist, views))
    m.grad_as_view = False
    for p in plist:
        p.grad = None
    out = _hand_over_grads(m, plist, views, flat, views, False, [True] * 5)
    assert all(torch.equal(o, v) and o.data_ptr() != v.data_ptr() for o, v in zip(out, views))
    assert all(p.grad is None for p in plist)


def check_layout(module):
    flat, views = module._grad_buffers()
    names = [n for n, _ in module.named_parameters()]
    params = [p for _, p in module.named_parameters()]
    assert len(views) == len(params) > 0
    off = 0
    for n, p, v in zip(names, params, views):
        assert v.shape == p.shape and v.dtype == torch.float32, n
        got = (v.data_ptr() - flat.data_ptr()) // 4
        assert got == off and got % 4 == 0, (n, got, off)
        off += (p.numel() + 3) // 4 * 4
    assert flat.numel() == off
    assert module._grad_buffers() is module._gbuf                             # cached
    flat2, views2 = module._grad_buffers(second=True)
    assert flat2.data_ptr() != flat.data_ptr() and flat2.numel() == off
    assert [(v.data_ptr() - flat2.data_ptr()) for v in views2] == [(v.data_ptr() - flat.data_ptr()) for v in views]


def test_flat_buffer_layout_of_the_stub():
    m = Stub()
    P._flat_grad_buffers(m)
    m._grad_buffers = lambda second=False: P._flat_grad_buffers(m, second)
    check_layout(m)
    assert m._gbuf[0].numel() == 16 + 8 + 4 + 4 + 8


@pytest.mark.parametrize("build", [
    lambda: EGNN_vel_Aether(in_node_nf=2, in_edge_nf=8, hidden_nf=64, n_layers=2, recurrent=True, tanh=True),
    lambda: ClofNet_vel_gbf(in_node_nf=1, in_edge_nf=2, hidden_nf=128, n_layers=3),
], ids=["egnn_aether", "clof_vel_gbf"])
def test_flat_buffer_layout_of_the_drop_ins(build):
    """Every tensor at a multiple of 4 floats, in named_parameters() order; the library's size check passes."""
    with contextlib.redirect_stdout(io.StringIO()):
        m = build()
    check_layout(m)
    m.float()                                                                 # _apply drops the cached buffers
    assert m._gbuf is None and m._gbuf2 is None
