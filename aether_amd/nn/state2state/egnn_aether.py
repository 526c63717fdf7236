"""MI355X drop-in for the reference's ``nn.state2state.egnn_aether.EGNN_vel_Aether`` (the model
experiments/lorentz/main.py:147 builds for ``--model egnn_aether``).

Same constructor, ``forward(h, x, edges, vel, edge_attr, charges)`` signature and ``state_dict`` keys / shapes / order
(egnn_aether.py:12-56, gcl.py:8-50, egnn/gcl.py:17-51), and the same default initialisation under a torch seed.  The
computation runs in ``libaether_hip.so`` (``aether_egnn_forward`` / ``aether_egnn_backward``, csrc/egnn.h); there is no
PyTorch or CPU fallback.  With gradients enabled the step goes through ``_EgnnStep``: parameter gradients only, written
into one flat buffer (the runner detaches every input, main.py:254-259), so ``GraphedTrainStep``, ``FusedAdamW`` and
``attach_data_parallel`` work as they do for ``Aether``.

One difference, on purpose: the reference adds into the caller's ``x`` in place (egnn/gcl.py:97, gcl.py:81); this module
returns a new tensor and leaves ``x`` as it was.
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from .aether import GraphCache, _FieldNetwork, _WsToken

SUPPORTED_HIDDEN = (64, 128)


class E_GCL_vel_field(nn.Module):
    """Parameter holder with the reference's names; construction order as egnn/gcl.py:17-51 + gcl.py:16-48, so that
    the default initialisation under a torch seed is the reference's (phi's last Linear is created and initialised with
    xavier gain 0.001 BEFORE coord_mlp[0])."""

    def __init__(self, hidden_nf, edges_in_d, num_dims, tanh):
        super().__init__()
        act = nn.SiLU()
        self.edge_mlp = nn.Sequential(nn.Linear(2 * hidden_nf + 1 + edges_in_d, hidden_nf), act,
                                      nn.Linear(hidden_nf, hidden_nf), act)
        self.node_mlp = nn.Sequential(nn.Linear(2 * hidden_nf, hidden_nf), act, nn.Linear(hidden_nf, hidden_nf))
        layer = nn.Linear(hidden_nf, 1, bias=False)
        torch.nn.init.xavier_uniform_(layer.weight, gain=0.001)
        coord_mlp = [nn.Linear(hidden_nf, hidden_nf), act, layer]
        if tanh:
            coord_mlp.append(nn.Tanh())
        self.coord_mlp = nn.Sequential(*coord_mlp)
        self.coord_mlp_vel = nn.Sequential(nn.Linear(hidden_nf + num_dims, hidden_nf), act, nn.Linear(hidden_nf, 1))


class _EgnnStep(torch.autograd.Function):
    """aether_egnn_forward (keep-for-backward form) / aether_egnn_backward behind torch.autograd; parameters only."""

    N_FIXED = 7          # module, h, x, vel, edge_attr, charges, graph precede the parameters

    @staticmethod
    def forward(ctx, module, h, x, vel, ea, charges, graph, *params):
        out, ws, token = module._launch(h, x, vel, ea, charges, graph, train=True)
        ctx.module = module
        ctx.saved = (h, x, vel, ea, charges, graph, ws, token)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        module = ctx.module
        h, x, vel, ea, charges, (graph, ginfo), ws, _token = ctx.saved
        flat, views = module._grad_buffers()
        plist = module._param_list()
        # aether_egnn_backward OVERWRITES its destination: when a .grad already is a view of the flat buffer (a second
        # backward without zero_grad), the kernels write into a second buffer and the result is added
        aliased = module.grad_as_view and any(p.grad is not None and p.grad.data_ptr() == v.data_ptr()
                                              for p, v in zip(plist, views))
        dst_flat, dst_views = module._grad_buffers(second=True) if aliased else (flat, views)
        g = grad_out.to(torch.float32).contiguous()
        st = lib.aether_egnn_backward(module._ptrs(), len(plist), module.hidden_nf, module.n_layers, module.in_node_nf,
                                      module._flags | _lib.EGNN_KEEP, x.shape[0], ginfo.n_edges, h.data_ptr(), x.data_ptr(),
                                      vel.data_ptr(), ea.data_ptr(), charges.data_ptr(), graph.data_ptr(), C.byref(ginfo),
                                      ws.data_ptr(), ws.numel(), g.data_ptr(), dst_flat.data_ptr(), dst_flat.numel(),
                                      torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, "aether_egnn_backward")
        if module.dp_group is not None:            # one fused all-reduce of the flat buffer (RCCL)
            import torch.distributed as dist
            dist.all_reduce(dst_flat, group=module.dp_group)
            dst_flat.div_(dist.get_world_size(module.dp_group))
        need = ctx.needs_input_grad[_EgnnStep.N_FIXED:]
        out = []
        for p, v, dv, n in zip(plist, views, dst_views, need):
            if not n:
                out.append(None)
            elif module.grad_as_view and p.grad is None and not aliased:
                p.grad = v
                out.append(None)
            elif module.grad_as_view and p.grad is not None and p.grad.data_ptr() == v.data_ptr():
                v.add_(dv)
                out.append(None)
            else:
                out.append(dv.clone())
        return (None,) * _EgnnStep.N_FIXED + tuple(out)


class EGNN_vel_Aether(nn.Module):
    """Drop-in for nn/state2state/egnn_aether.py:12-75."""

    def __init__(self, in_node_nf, in_edge_nf, hidden_nf, num_dims=3, device="cpu", act_fn=nn.SiLU(), n_layers=4,
                 coords_weight=1.0, recurrent=False, norm_diff=False, tanh=False):
        super().__init__()
        if num_dims != 3:
            raise ValueError("EGNN_vel_Aether: num_dims must be 3 (the field net and the kernels are 3-D)")
        if hidden_nf not in SUPPORTED_HIDDEN:
            raise ValueError(f"EGNN_vel_Aether: hidden_nf must be one of {SUPPORTED_HIDDEN}")
        if not (1 <= int(n_layers) <= 64):
            raise ValueError("EGNN_vel_Aether: n_layers must lie in [1, 64]")
        if not (1 <= int(in_node_nf) <= 4096):
            raise ValueError("EGNN_vel_Aether: in_node_nf must lie in [1, 4096]")
        if in_edge_nf != 2 + 2 * num_dims:
            raise ValueError("EGNN_vel_Aether: in_edge_nf must be 8 (edge_attr [q_i q_j, |x_i - x_j|^2] + the field at "
                             "both ends, experiments/lorentz/main.py:147,254-259)")
        if not recurrent:
            raise ValueError("EGNN_vel_Aether: only recurrent=True is supported (the runner's setting)")
        if float(coords_weight) != 1.0:
            raise ValueError("EGNN_vel_Aether: only coords_weight=1 is supported")
        if type(act_fn) is not nn.SiLU:
            raise ValueError("EGNN_vel_Aether: only act_fn=nn.SiLU() is supported")
        self.hidden_nf = int(hidden_nf)
        self.in_node_nf = int(in_node_nf)
        self.device = device
        self.n_layers = int(n_layers)
        self.num_dims = num_dims
        self.norm_diff = bool(norm_diff)
        self.tanh = bool(tanh)
        self.embedding = nn.Linear(in_node_nf, self.hidden_nf)
        for i in range(self.n_layers):
            self.add_module("gcl_%d" % i, E_GCL_vel_field(self.hidden_nf, in_edge_nf, num_dims, self.tanh))
        self.field_net = _FieldNetwork(num_dims, 32, 16)
        self._flags = (_lib.EGNN_NORM_DIFF if self.norm_diff else 0) | (_lib.EGNN_TANH if self.tanh else 0)
        self._graphs = GraphCache()
        self.dp_group = None              # set by aether_amd.parallel.attach_data_parallel
        self.grad_as_view = True          # .grad tensors alias one flat buffer (see _EgnnStep.backward)
        self._plist = None
        self._ptr_cache = None
        self._gbuf = None
        self._gbuf2 = None
        self._ws = None
        self._train_ws, self._train_ws_token = None, None
        self._last_ws = None
        self.to(self.device)
        self.params = self.__str__()

    def __str__(self):
        params = sum(int(np.prod(p.size())) for p in self.parameters() if p.requires_grad)
        print("Network Size", params)
        return str(params)

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

    def _ptrs(self):
        """Host array of the parameters' device pointers, named_parameters() order (include/aether_hip.h)."""
        plist = self._param_list()
        key = tuple(p.data_ptr() for p in plist)
        if self._ptr_cache is None or self._ptr_cache[0] != key:
            for p in plist:
                if not (p.dtype == torch.float32 and p.is_contiguous()):
                    raise _lib.AetherHipError("EGNN_vel_Aether: parameters must be contiguous fp32")
            self._ptr_cache = (key, (C.c_void_p * len(plist))(*key))
        return self._ptr_cache[1]

    def _grad_buffers(self, second=False):
        """Flat fp32 gradient buffer and per-parameter views into it: every tensor at the next multiple of 4 floats, in
        named_parameters() order (the layout aether_egnn_backward writes).  ``second``: a scratch buffer of the same
        layout, the destination of a backward whose result is ADDED to gradients that already live in the first one."""
        slot = "_gbuf2" if second else "_gbuf"
        cur = getattr(self, slot, None)
        plist = self._param_list()
        if cur is not None and cur[0].device == plist[0].device:
            return cur
        offs, off = [], 0
        for p in plist:
            offs.append(off)
            off += (p.numel() + 3) // 4 * 4
        want = _lib.load().aether_egnn_grad_floats(self.hidden_nf, self.n_layers, self.in_node_nf)
        if want != off:
            raise _lib.AetherHipError(f"EGNN_vel_Aether: gradient layout mismatch ({off} floats, library {want})")
        flat = torch.zeros(off, dtype=torch.float32, device=plist[0].device)
        views = [flat[o:o + p.numel()].view_as(p) for o, p in zip(offs, plist)]
        cur = (flat, views)
        setattr(self, slot, cur)
        return cur

    def _workspace_bytes(self, n_nodes, n_edges, keep):
        return _lib.load().aether_egnn_workspace_bytes(self.hidden_nf, self.n_layers, self.in_node_nf, n_nodes, n_edges,
                                                       1 if keep else 0)

    def prepare_graph(self, edges, n_nodes):
        """Row-sorted view of ``edges = [row, col]``: aether_graph_build with the index rows swapped, so that the view
        groups the edges by edges[0], over which E_GCL sums and averages (egnn/gcl.py:69-101)."""
        row, col = edges
        return self._graphs.get(col.contiguous(), row.contiguous(), n_nodes)

    def _launch(self, h, x, vel, ea, charges, graph, train, keep=False):
        lib = _lib.load()
        graph, ginfo = graph
        n_nodes, n_edges = x.shape[0], ginfo.n_edges
        keep = keep or train
        nbytes = max(self._workspace_bytes(n_nodes, n_edges, keep), 256)
        token = None
        if train:
            # one workspace per forward still waiting for its backward (the token its autograd node holds); under
            # hipGraph capture the buffer comes from the graph's pool
            tw, tok = self._train_ws, self._train_ws_token
            busy = tok is not None and tok() is not None
            capturing = torch.cuda.is_current_stream_capturing()
            if tw is not None and not busy and tw.numel() >= nbytes and tw.device == x.device and not capturing:
                ws = tw
            else:
                ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
                if not capturing:
                    self._train_ws = ws
            if not capturing:
                token = _WsToken()
                self._train_ws_token = weakref.ref(token)
        else:
            if self._ws is None or self._ws.numel() < nbytes or self._ws.device != x.device:
                self._ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            ws = self._ws
        out = torch.empty_like(x)
        flags = self._flags | (_lib.EGNN_KEEP if keep else 0)
        st = lib.aether_egnn_forward(self._ptrs(), len(self._param_list()), self.hidden_nf, self.n_layers, self.in_node_nf,
                                     flags, n_nodes, n_edges, h.data_ptr(), x.data_ptr(), vel.data_ptr(), ea.data_ptr(),
                                     charges.data_ptr(), graph.data_ptr(), C.byref(ginfo), ws.data_ptr(), ws.numel(),
                                     out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, "aether_egnn_forward")
        self._last_ws = ws
        return out, ws, token

    def _inputs(self, h, x, edges, vel, edge_attr, charges):
        if not x.is_cuda:
            raise _lib.AetherHipError("aether_amd EGNN_vel_Aether runs on an MI355X only; got a CPU tensor "
                                      "(there is no CPU fallback)")
        if torch.is_grad_enabled() and any(t.requires_grad for t in (h, x, vel, edge_attr, charges)):
            raise _lib.AetherHipError("EGNN_vel_Aether: gradients flow to the parameters only (the runner detaches every "
                                      "input, experiments/lorentz/main.py:254-259); detach the inputs")
        row, col = edges
        if row.dtype != torch.int64 or col.dtype != torch.int64:
            raise TypeError("edges must be int64 (torch.LongTensor), as in the reference")
        n_nodes = x.shape[0]
        E = row.numel()
        if x.shape != (n_nodes, 3) or vel.shape != x.shape:
            raise ValueError("x / vel must be [n_nodes, 3]")
        if h.shape != (n_nodes, self.in_node_nf) or col.numel() != E or edge_attr.shape != (E, 2) or \
                charges.numel() != n_nodes:
            raise ValueError("h / edge index / edge_attr / charges shapes do not match")
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        graph = self.prepare_graph((row, col), n_nodes)
        return f32(h), f32(x), f32(vel), f32(edge_attr), f32(charges), graph

    # -- reference surface -----------------------------------------------------------
    def forward(self, h, x, edges, vel, edge_attr, charges):
        h, x, vel, ea, charges, graph = self._inputs(h, x, edges, vel, edge_attr, charges)
        plist = self._param_list()
        if torch.is_grad_enabled() and any(p.requires_grad for p in plist):
            return _EgnnStep.apply(self, h, x, vel, ea, charges, graph, *plist)
        return self._launch(h, x, vel, ea, charges, graph, train=False)[0]

    # -- test hook -------------------------------------------------------------------
    @torch.no_grad()
    def forward_layers(self, h, x, edges, vel, edge_attr, charges):
        """(out, [h_0 .. h_L], [x_0 .. x_L]): every layer's input h / x (the embedding's output, then each layer's), from
        a keep-for-backward forward."""
        h, x, vel, ea, charges, graph = self._inputs(h, x, edges, vel, edge_attr, charges)
        out, ws, _ = self._launch(h, x, vel, ea, charges, graph, train=False, keep=True)
        lib = _lib.load()
        n, H, L = x.shape[0], self.hidden_nf, self.n_layers
        E = graph[1].n_edges
        f = ws.view(torch.float32) if ws.numel() % 4 == 0 else ws[: ws.numel() // 4 * 4].view(torch.float32)

        def at(name, layer, cols):
            off = lib.aether_egnn_workspace_offset(name.encode(), layer, H, L, self.in_node_nf, n, E)
            _lib.check(off, "aether_egnn_workspace_offset")
            return f[off // 4: off // 4 + n * cols].view(n, cols).clone()

        hs = [at("h", l, H) for l in range(L + 1)]
        xs = [at("x", l, 3) for l in range(L + 1)]
        return out, hs, xs
