"""Plumbing shared by the drop-ins whose gradients go to the parameters only, written by the library into one flat buffer
(``EGNN_vel_Aether``, ``ClofNet*``): parameter-pointer and gradient-buffer caches, workspaces, the library calls and the
autograd function around them.

A subclass supplies its constructor (argument checks and parameter holders, then ``_finish_init``), ``_inputs`` (validation;
returns what ``_run`` takes), ``NAME`` / ``ENTRY`` / ``KEEP``, ``_sizes`` and, where some parameters do not reach the
output, ``_dead``.  Its library entries are ``ENTRY_forward``, ``_backward``, ``_workspace_bytes``, ``_grad_floats``,
``_workspace_offset``, ``_rollout`` and ``_rollout_workspace_bytes`` (include/aether_hip.h); forward and backward take

    params, n_params, *_sizes(), flags, *call, n_nodes, n_edges, h, x, vel, *extra, graph, info, workspace, ...

where ``call`` (scalars of this call) and ``extra`` (tensors between vel and the graph) come from ``_inputs``.  ``rollout``
(the device rollout of metric 2) is shared: a subclass whose entry takes scalars of the call supplies ``_rollout_call``.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from ... import _lib
from ._frame import GraphCache, _grads_alias_flat, _hand_over_grads, _train_workspace, network_size


def _flat_grad_buffers(module, second=False, check=None):
    """Flat fp32 gradient buffer and per-parameter views into it: every tensor at the next multiple of 4 floats, in
    named_parameters() order.  Cached on the module (``_gbuf``; ``second``: ``_gbuf2``, a scratch buffer of the same
    layout, the destination of a backward whose result is ADDED to gradients that already live in the first one).
    ``check(floats)`` sees the total before anything is allocated."""
    slot = "_gbuf2" if second else "_gbuf"
    cur = getattr(module, slot, None)
    plist = module._param_list()
    if cur is not None and cur[0].device == plist[0].device:
        return cur
    offs, off = [], 0
    for p in plist:
        offs.append(off)
        off += (p.numel() + 3) // 4 * 4
    if check is not None:
        check(off)
    flat = torch.zeros(off, dtype=torch.float32, device=plist[0].device)
    cur = (flat, [flat[o:o + p.numel()].view_as(p) for o, p in zip(offs, plist)])
    setattr(module, slot, cur)
    return cur


class _ParamGradStep(torch.autograd.Function):
    """ENTRY_forward (keep-for-backward form) / ENTRY_backward behind torch.autograd; parameters only."""

    N_FIXED = 7          # module, h, x, vel, extra, call, graph precede the parameters

    @staticmethod
    def forward(ctx, module, h, x, vel, extra, call, graph, *params):
        out, ws, token = module._launch(h, x, vel, extra, call, graph, train=True)
        ctx.module = module
        ctx.saved = (h, x, vel, extra, call, graph, ws, token)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        module = ctx.module
        h, x, vel, extra, call, (graph, ginfo), ws, _token = ctx.saved
        flat, views = module._grad_buffers()
        plist = module._param_list()
        aliased = _grads_alias_flat(module, plist, views)        # ENTRY_backward OVERWRITES its destination
        dst_flat, dst_views = module._grad_buffers(second=True) if aliased else (flat, views)
        g = grad_out.to(torch.float32).contiguous()
        st = module._entry("backward")(module._ptrs(), len(plist), *module._sizes(), module._flags | module.KEEP, *call,
                                       x.shape[0], ginfo.n_edges, h.data_ptr(), x.data_ptr(), vel.data_ptr(),
                                       *[t.data_ptr() for t in extra], graph.data_ptr(), C.byref(ginfo), ws.data_ptr(),
                                       ws.numel(), g.data_ptr(), dst_flat.data_ptr(), dst_flat.numel(),
                                       torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, module.ENTRY + "_backward")
        out = _hand_over_grads(module, plist, views, dst_flat, dst_views, aliased,
                               ctx.needs_input_grad[_ParamGradStep.N_FIXED:], module._dead())
        return (None,) * _ParamGradStep.N_FIXED + tuple(out)


class ParamGradModule(nn.Module):
    NAME = None          # the class name error messages carry
    ENTRY = None         # prefix of the five library entries, e.g. "aether_egnn"
    KEEP = 0             # the entries' keep-for-backward flag bit

    def _finish_init(self):
        """End of a subclass constructor, after the parameter holders: caches, then the move to ``self.device``."""
        self._graphs = GraphCache()
        self.dp_group = None              # set by aether_amd.parallel.attach_data_parallel
        self.grad_as_view = True          # .grad tensors alias one flat buffer (see _ParamGradStep.backward)
        self._plist = None
        self._ptr_cache = None
        self._gbuf = None
        self._gbuf2 = None
        self._ws = None
        self._rollout_ws = None           # aether_*_rollout's workspace (inference workspace + the rollout's state)
        self._train_ws, self._train_ws_token = None, None
        self._last_ws = None
        self.to(self.device)
        self.params = self.__str__()

    __str__ = network_size

    # -- what a subclass supplies ----------------------------------------------------
    def _sizes(self):
        """Leading integer arguments of every library entry."""
        raise NotImplementedError

    def _dead(self):
        """Indices (named_parameters order) of the tensors that do not reach the output: their .grad stays None."""
        return ()

    # -- plumbing ------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._plist = None                # parameter storage may move (.to / .cuda / .float)
        self._ptr_cache = None
        self._gbuf = None
        self._gbuf2 = None
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._plist = None
        self._ptr_cache = None
        return super().load_state_dict(*a, **k)

    def _param_list(self):
        if self._plist is None:           # nn.Module.parameters() walks the module tree
            self._plist = [p for _, p in self.named_parameters()]
        return self._plist

    def _entry(self, what):
        return getattr(_lib.load(), f"{self.ENTRY}_{what}")

    def _ptrs(self):
        """Host array of the parameters' device pointers, named_parameters() order (include/aether_hip.h)."""
        plist = self._param_list()
        key = tuple(p.data_ptr() for p in plist)
        if self._ptr_cache is None or self._ptr_cache[0] != key:
            for p in plist:
                if not (p.dtype == torch.float32 and p.is_contiguous()):
                    raise _lib.AetherHipError(f"{self.NAME}: parameters must be contiguous fp32")
            self._ptr_cache = (key, (C.c_void_p * len(plist))(*key))
        return self._ptr_cache[1]

    def _check_grad_floats(self, floats):
        want = self._entry("grad_floats")(*self._sizes())
        if want != floats:
            raise _lib.AetherHipError(f"{self.NAME}: gradient layout mismatch ({floats} floats, library {want})")

    def _grad_buffers(self, second=False):
        """``_flat_grad_buffers``, checked against the layout ENTRY_backward writes."""
        return _flat_grad_buffers(self, second, self._check_grad_floats)

    def _workspace_bytes(self, n_nodes, n_edges, keep):
        return self._entry("workspace_bytes")(*self._sizes(), n_nodes, n_edges, 1 if keep else 0)

    def prepare_graph(self, edges, n_nodes):
        """Row-sorted view of ``edges = [row, col]``: aether_graph_build with the index rows swapped, so that the view
        groups the edges by edges[0], over which the layers sum and average (egnn/gcl.py:69-101)."""
        row, col = edges
        return self._graphs.get(col.contiguous(), row.contiguous(), n_nodes)

    def _launch(self, h, x, vel, extra, call, graph, train, keep=False):
        graph, ginfo = graph
        n_nodes, n_edges = x.shape[0], ginfo.n_edges
        keep = keep or train
        nbytes = max(self._workspace_bytes(n_nodes, n_edges, keep), 256)
        token = None
        if train:
            ws, token = _train_workspace(self, nbytes, x.device)
        else:
            if self._ws is None or self._ws.numel() < nbytes or self._ws.device != x.device:
                self._ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            ws = self._ws
        out = torch.empty_like(x)
        st = self._entry("forward")(self._ptrs(), len(self._param_list()), *self._sizes(),
                                    self._flags | (self.KEEP if keep else 0), *call, n_nodes, n_edges, h.data_ptr(),
                                    x.data_ptr(), vel.data_ptr(), *[t.data_ptr() for t in extra], graph.data_ptr(),
                                    C.byref(ginfo), ws.data_ptr(), ws.numel(), out.data_ptr(),
                                    torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, self.ENTRY + "_forward")
        self._last_ws = ws
        return out, ws, token

    def _run(self, h, x, vel, extra, call, graph):
        """The body of ``forward``, on what ``_inputs`` returned."""
        plist = self._param_list()
        if torch.is_grad_enabled() and any(p.requires_grad for p in plist):
            return _ParamGradStep.apply(self, h, x, vel, extra, call, graph, *plist)
        return self._launch(h, x, vel, extra, call, graph, train=False)[0]

    def _rollout_call(self, n_total):
        """Scalars of a rollout between the flags and n_nodes (``call`` of a forward), from ``rollout``'s further keyword
        arguments."""
        return ()

    @torch.no_grad()
    def rollout(self, x, vel, edges, charges, steps, dt=1.0, **call_kw):
        """``steps`` autoregressive steps on the device -> positions [steps, n_nodes, 3]: x_{t+1} = self(|v_t|, x_t, v_t,
        edge_attr_t), v_{t+1} = (x_{t+1} - x_t) / dt, ``edge_attr_t = [q_row q_col, |x_row - x_col|^2]`` rebuilt by the
        library every step (experiments/lorentz/main.py:254-271); one call of ENTRY_rollout, weight images prepared once.
        ``x`` and ``vel`` are not written."""
        if self.in_node_nf != 1:
            raise ValueError(f"{self.NAME}.rollout: in_node_nf must be 1 (h = |vel| is rebuilt every step)")
        row, col = edges
        n_nodes, E = x.shape[0], row.numel()
        call = self._rollout_call(n_nodes, **call_kw)
        if x.shape != (n_nodes, 3) or vel.shape != x.shape or n_nodes == 0:
            raise ValueError("x / vel must be [n_nodes, 3]")
        if col.numel() != E or charges.numel() != n_nodes:
            raise ValueError("edge index / charges shapes do not match")
        if row.dtype != torch.int64 or col.dtype != torch.int64:
            raise TypeError("edges must be int64 (torch.LongTensor), as in the reference")
        if not x.is_cuda:
            raise _lib.AetherHipError(f"aether_amd {self.NAME} runs on an MI355X only; got a CPU tensor "
                                      "(there is no CPU fallback)")
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        x, vel, charges, row, col = f32(x), f32(vel), f32(charges), row.contiguous(), col.contiguous()
        graph, ginfo = self.prepare_graph((row, col), n_nodes)
        steps = int(steps)
        traj = torch.empty(max(steps, 0), n_nodes, 3, dtype=torch.float32, device=x.device)
        if steps <= 0:
            return traj
        nbytes = max(self._entry("rollout_workspace_bytes")(*self._sizes(), n_nodes, E), 256)
        if self._rollout_ws is None or self._rollout_ws.numel() < nbytes or self._rollout_ws.device != x.device:
            self._rollout_ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        ws = self._rollout_ws
        st = self._entry("rollout")(self._ptrs(), len(self._param_list()), *self._sizes(), self._flags, *call, n_nodes, E,
                                    x.data_ptr(), vel.data_ptr(), charges.data_ptr(), col.data_ptr(), row.data_ptr(),
                                    graph.data_ptr(), C.byref(ginfo), ws.data_ptr(), ws.numel(), traj.data_ptr(), steps,
                                    float(dt), torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, self.ENTRY + "_rollout")
        return traj

    def _run_layers(self, h, x, vel, extra, call, graph):
        """The body of ``forward_layers`` (under torch.no_grad()): (out, [h_0 .. h_L], [x_0 .. x_L]) from a
        keep-for-backward forward."""
        out, ws, _ = self._launch(h, x, vel, extra, call, graph, train=False, keep=True)
        offset = self._entry("workspace_offset")
        n, H, L = x.shape[0], self.hidden_nf, self.n_layers
        E = graph[1].n_edges
        f = ws[: ws.numel() // 4 * 4].view(torch.float32)

        def at(name, layer, cols):
            off = offset(name.encode(), layer, *self._sizes(), n, E)
            _lib.check(off, self.ENTRY + "_workspace_offset")
            return f[off // 4: off // 4 + n * cols].view(n, cols).clone()

        hs = [at("h", l, H) for l in range(L + 1)]
        xs = [at("x", l, 3) for l in range(L + 1)]
        return out, hs, xs
