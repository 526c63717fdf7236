"""MI355X drop-ins for the reference's ``nn.state2state.clof.clof.{ClofNet, ClofNet_vel, ClofNet_vel_gbf}`` (the models
experiments/lorentz/main.py:152-157 builds for ``--model clof``, ``clof_vel`` and ``clof_vel_gbf``).

Same constructors, ``forward(h, x, edges, vel, edge_attr, node_attr=None, n_nodes=5)`` signature and ``state_dict`` keys /
shapes / order (clof.py, clof/gcl.py, clof/layers.py, egnn/gcl.py:17-51), and the same default initialisation under a
torch seed.  The computation runs in ``libaether_hip.so`` (``aether_clof_forward`` / ``aether_clof_backward``,
csrc/clof.h); there is no PyTorch or CPU fallback.  With gradients enabled the step goes through ``_ClofStep``: parameter
gradients only, written into one flat buffer (the runner detaches every input, main.py:266-271), so ``GraphedTrainStep``,
``FusedAdamW`` and ``attach_data_parallel`` work as they do for ``Aether``.  Parameters that do not reach the output --
the last layer's ``node_mlp`` and ``layer_norm``, ClofNet's ``embedding_edge`` -- keep ``.grad`` None, as in the
reference, so no optimizer touches them.

Differences, on purpose: the reference adds into its centred copy of x in place, this module never writes the caller's
x; the cross products are always per edge (``torch.cross`` without ``dim`` crosses along the edge axis when there are
exactly 3 edges); the Gaussian layer's edge type is clamped to [0, 7] (the reference raises an index error outside it).
"""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from .aether import GraphCache, _WsToken

SUPPORTED_HIDDEN = (64, 128)
_HEAD = {0: 8, 1: 6, 2: 10}           # tensors before gcl_0 (include/aether_hip.h)
_PER_LAYER = 19


class Clof_GCL(nn.Module):
    """Parameter holder with the reference's names; construction order as egnn/gcl.py:17-51 then clof/gcl.py:13-24, so
    that the default initialisation under a torch seed is the reference's: E_GCL builds a two-layer edge_mlp (its random
    numbers are used up, the module is then replaced in place by Clof_GCL's three-layer one), node_mlp, the xavier-gain-0.001
    basis layer, coord_mlp.0, then coord_mlp_vel, the new edge_mlp and layer_norm."""

    def __init__(self, hidden_nf, edges_in_d, tanh):
        super().__init__()
        act = nn.SiLU()
        H = hidden_nf
        kin = 2 * H + 1 + edges_in_d
        self.edge_mlp = nn.Sequential(nn.Linear(kin, H), act, nn.Linear(H, H), act)
        self.node_mlp = nn.Sequential(nn.Linear(2 * H, H), act, nn.Linear(H, H))
        layer = nn.Linear(H, 3, bias=False)
        torch.nn.init.xavier_uniform_(layer.weight, gain=0.001)
        coord_mlp = [nn.Linear(H, H), act, layer]
        if tanh:
            coord_mlp.append(nn.Tanh())
        self.coord_mlp = nn.Sequential(*coord_mlp)
        self.coord_mlp_vel = nn.Sequential(nn.Linear(H, H), act, nn.Linear(H, 1))
        self.edge_mlp = nn.Sequential(nn.Linear(kin, H), act, nn.Linear(H, H), act, nn.Linear(H, H), act)
        self.layer_norm = nn.LayerNorm(H)


class GaussianLayer(nn.Module):
    """clof/layers.py:GaussianLayer's parameters and initialisation (K = hidden_nf / 2, 8 edge types)."""

    def __init__(self, K, edge_types=8):
        super().__init__()
        self.K = K
        self.means = nn.Embedding(1, K)
        self.stds = nn.Embedding(1, K)
        self.mul = nn.Embedding(edge_types, 1)
        self.bias = nn.Embedding(edge_types, 1)
        nn.init.uniform_(self.means.weight, 0, 3)
        nn.init.uniform_(self.stds.weight, 0, 3)
        nn.init.constant_(self.bias.weight, 0)
        nn.init.constant_(self.mul.weight, 1)


class _ClofStep(torch.autograd.Function):
    """aether_clof_forward (keep-for-backward form) / aether_clof_backward behind torch.autograd; parameters only."""

    N_FIXED = 7          # module, h, x, vel, edge_attr, n_nodes, graph precede the parameters

    @staticmethod
    def forward(ctx, module, h, x, vel, ea, n_per, graph, *params):
        out, ws, token = module._launch(h, x, vel, ea, n_per, graph, train=True)
        ctx.module = module
        ctx.saved = (h, x, vel, ea, n_per, graph, ws, token)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        module = ctx.module
        h, x, vel, ea, n_per, (graph, ginfo), ws, _token = ctx.saved
        flat, views = module._grad_buffers()
        plist = module._param_list()
        # aether_clof_backward OVERWRITES its destination: when a .grad already is a view of the flat buffer (a second
        # backward without zero_grad), the kernels write into a second buffer and the result is added
        aliased = module.grad_as_view and any(p.grad is not None and p.grad.data_ptr() == v.data_ptr()
                                              for p, v in zip(plist, views))
        dst_flat, dst_views = module._grad_buffers(second=True) if aliased else (flat, views)
        g = grad_out.to(torch.float32).contiguous()
        st = lib.aether_clof_backward(module._ptrs(), len(plist), module._variant, module.hidden_nf, module.n_layers,
                                      module.in_node_nf, module._flags | _lib.CLOF_KEEP, module.coords_weight, n_per,
                                      x.shape[0], ginfo.n_edges, h.data_ptr(), x.data_ptr(), vel.data_ptr(),
                                      ea.data_ptr(), graph.data_ptr(), C.byref(ginfo), ws.data_ptr(), ws.numel(),
                                      g.data_ptr(), dst_flat.data_ptr(), dst_flat.numel(),
                                      torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, "aether_clof_backward")
        if module.dp_group is not None:            # one fused all-reduce of the flat buffer (RCCL)
            import torch.distributed as dist
            dist.all_reduce(dst_flat, group=module.dp_group)
            dst_flat.div_(dist.get_world_size(module.dp_group))
        need = ctx.needs_input_grad[_ClofStep.N_FIXED:]
        dead = module._dead()
        out = []
        for i, (p, v, dv, n) in enumerate(zip(plist, views, dst_views, need)):
            if not n or i in dead:
                out.append(None)
            elif module.grad_as_view and p.grad is None and not aliased:
                p.grad = v
                out.append(None)
            elif module.grad_as_view and p.grad is not None and p.grad.data_ptr() == v.data_ptr():
                v.add_(dv)
                out.append(None)
            else:
                out.append(dv.clone())
        return (None,) * _ClofStep.N_FIXED + tuple(out)


class _ClofBase(nn.Module):
    VARIANT = None
    NAME = None

    def __init__(self, in_node_nf, in_edge_nf, hidden_nf, device="cpu", act_fn=nn.SiLU(), n_layers=4, coords_weight=1.0,
                 recurrent=True, norm_diff=True, tanh=False):
        super().__init__()
        name = self.NAME
        if hidden_nf not in SUPPORTED_HIDDEN:
            raise ValueError(f"{name}: hidden_nf must be one of {SUPPORTED_HIDDEN}")
        if not (1 <= int(n_layers) <= 64):
            raise ValueError(f"{name}: n_layers must lie in [1, 64]")
        if not (1 <= int(in_node_nf) <= 4096):
            raise ValueError(f"{name}: in_node_nf must lie in [1, 4096]")
        if in_edge_nf != 2:
            raise ValueError(f"{name}: in_edge_nf must be 2 (edge_attr [q_i q_j, |x_i - x_j|^2], "
                             "experiments/lorentz/main.py:152-157,266-271)")
        if type(act_fn) is not nn.SiLU:
            raise ValueError(f"{name}: only act_fn=nn.SiLU() is supported")
        self.hidden_nf = int(hidden_nf)
        self.in_node_nf = int(in_node_nf)
        self.device = device
        self.n_layers = int(n_layers)
        self.coords_weight = float(coords_weight)
        self.recurrent = bool(recurrent)
        self.tanh = bool(tanh)
        self._layer_norm_diff = bool(norm_diff)
        self._variant = self.VARIANT
        H, H2 = self.hidden_nf, self.hidden_nf // 2
        self.embedding_node = nn.Linear(in_node_nf, H)
        if self.VARIANT == 0:
            self.embedding_edge = nn.Sequential(nn.Linear(in_edge_nf, 8), nn.SiLU())
        if self.VARIANT == 2:
            self.gbf = GaussianLayer(K=H2, edge_types=8)
        fuse_in = {0: 10, 1: 16, 2: 14}[self.VARIANT]
        self.fuse_edge = nn.Sequential(nn.Linear(fuse_in, H2), nn.SiLU(), nn.Linear(H2, H2), nn.SiLU())
        # ClofNet scalarizes with norm_diff; the _vel variants always normalise there (clof.py:113,190)
        self.norm_diff = bool(norm_diff) if self.VARIANT == 0 else True
        for i in range(self.n_layers):
            self.add_module("gcl_%d" % i, Clof_GCL(H, H2, self.tanh))
        self._flags = ((_lib.CLOF_NORM_DIFF if self._layer_norm_diff else 0) | (_lib.CLOF_TANH if self.tanh else 0) |
                       (_lib.CLOF_RECURRENT if self.recurrent else 0))
        self._graphs = GraphCache()
        self.dp_group = None              # set by aether_amd.parallel.attach_data_parallel
        self.grad_as_view = True          # .grad tensors alias one flat buffer (see _ClofStep.backward)
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
        if self._plist is None:
            self._plist = [p for _, p in self.named_parameters()]
        return self._plist

    def _dead(self):
        """Indices (named_parameters order) of the tensors that do not reach the output: the last layer's node_mlp and
        layer_norm, ClofNet's embedding_edge.  Their .grad stays None."""
        last = _HEAD[self._variant] + _PER_LAYER * (self.n_layers - 1)
        dead = {last + 6, last + 7, last + 8, last + 9, last + 17, last + 18}
        if self._variant == 0:
            dead |= {2, 3}
        return dead

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

    def _grad_buffers(self, second=False):
        """Flat fp32 gradient buffer and per-parameter views into it: every tensor at the next multiple of 4 floats, in
        named_parameters() order (the layout aether_clof_backward writes)."""
        slot = "_gbuf2" if second else "_gbuf"
        cur = getattr(self, slot, None)
        plist = self._param_list()
        if cur is not None and cur[0].device == plist[0].device:
            return cur
        offs, off = [], 0
        for p in plist:
            offs.append(off)
            off += (p.numel() + 3) // 4 * 4
        want = _lib.load().aether_clof_grad_floats(self._variant, self.hidden_nf, self.n_layers, self.in_node_nf)
        if want != off:
            raise _lib.AetherHipError(f"{self.NAME}: gradient layout mismatch ({off} floats, library {want})")
        flat = torch.zeros(off, dtype=torch.float32, device=plist[0].device)
        views = [flat[o:o + p.numel()].view_as(p) for o, p in zip(offs, plist)]
        cur = (flat, views)
        setattr(self, slot, cur)
        return cur

    def _workspace_bytes(self, n_nodes, n_edges, keep):
        return _lib.load().aether_clof_workspace_bytes(self._variant, self.hidden_nf, self.n_layers, self.in_node_nf,
                                                       n_nodes, n_edges, 1 if keep else 0)

    def prepare_graph(self, edges, n_nodes):
        """Row-sorted view of ``edges = [row, col]``: aether_graph_build with the index rows swapped, so that the view
        groups the edges by edges[0], over which Clof_GCL sums and averages."""
        row, col = edges
        return self._graphs.get(col.contiguous(), row.contiguous(), n_nodes)

    def _launch(self, h, x, vel, ea, n_per, graph, train, keep=False):
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
        flags = self._flags | (_lib.CLOF_KEEP if keep else 0)
        st = lib.aether_clof_forward(self._ptrs(), len(self._param_list()), self._variant, self.hidden_nf, self.n_layers,
                                     self.in_node_nf, flags, self.coords_weight, n_per, n_nodes, n_edges, h.data_ptr(),
                                     x.data_ptr(), vel.data_ptr(), ea.data_ptr(), graph.data_ptr(), C.byref(ginfo),
                                     ws.data_ptr(), ws.numel(), out.data_ptr(),
                                     torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, "aether_clof_forward")
        self._last_ws = ws
        return out, ws, token

    def _inputs(self, h, x, edges, vel, edge_attr, node_attr, n_nodes):
        if node_attr is not None:
            raise ValueError(f"{self.NAME}: node_attr must be None (Clof_GCL's node_mlp has no columns for it)")
        n_per = int(n_nodes)
        if n_per < 1 or x.shape[0] % n_per != 0:
            raise ValueError(f"{self.NAME}: the node count {x.shape[0]} is not a multiple of n_nodes={n_nodes}")
        if not x.is_cuda:
            raise _lib.AetherHipError(f"aether_amd {self.NAME} runs on an MI355X only; got a CPU tensor "
                                      "(there is no CPU fallback)")
        if torch.is_grad_enabled() and any(t.requires_grad for t in (h, x, vel, edge_attr)):
            raise _lib.AetherHipError(f"{self.NAME}: gradients flow to the parameters only (the runner detaches every "
                                      "input, experiments/lorentz/main.py:266-271); detach the inputs")
        row, col = edges
        if row.dtype != torch.int64 or col.dtype != torch.int64:
            raise TypeError("edges must be int64 (torch.LongTensor), as in the reference")
        N = x.shape[0]
        E = row.numel()
        if x.shape != (N, 3) or vel.shape != x.shape:
            raise ValueError("x / vel must be [n_nodes, 3]")
        if h.shape != (N, self.in_node_nf) or col.numel() != E or edge_attr.shape != (E, 2):
            raise ValueError("h / edge index / edge_attr shapes do not match")
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        graph = self.prepare_graph((row, col), N)
        return f32(h), f32(x), f32(vel), f32(edge_attr), n_per, graph

    # -- reference surface -----------------------------------------------------------
    def forward(self, h, x, edges, vel, edge_attr, node_attr=None, n_nodes=5):
        h, x, vel, ea, n_per, graph = self._inputs(h, x, edges, vel, edge_attr, node_attr, n_nodes)
        plist = self._param_list()
        if torch.is_grad_enabled() and any(p.requires_grad for p in plist):
            return _ClofStep.apply(self, h, x, vel, ea, n_per, graph, *plist)
        return self._launch(h, x, vel, ea, n_per, graph, train=False)[0]

    # -- test hook -------------------------------------------------------------------
    @torch.no_grad()
    def forward_layers(self, h, x, edges, vel, edge_attr, node_attr=None, n_nodes=5):
        """(out, [h_0 .. h_L], [x_0 .. x_L]): every layer's input h and centred x (the embedding's output and the
        centred input, then each layer's output), from a keep-for-backward forward."""
        h, x, vel, ea, n_per, graph = self._inputs(h, x, edges, vel, edge_attr, node_attr, n_nodes)
        out, ws, _ = self._launch(h, x, vel, ea, n_per, graph, train=False, keep=True)
        lib = _lib.load()
        n, H, L = x.shape[0], self.hidden_nf, self.n_layers
        E = graph[1].n_edges
        f = ws[: ws.numel() // 4 * 4].view(torch.float32)

        def at(name, layer, cols):
            off = lib.aether_clof_workspace_offset(name.encode(), layer, self._variant, H, L, self.in_node_nf, n, E)
            _lib.check(off, "aether_clof_workspace_offset")
            return f[off // 4: off // 4 + n * cols].view(n, cols).clone()

        hs = [at("h", l, H) for l in range(L + 1)]
        xs = [at("x", l, 3) for l in range(L + 1)]
        return out, hs, xs


class ClofNet(_ClofBase):
    """Drop-in for nn/state2state/clof/clof.py:ClofNet (``--model clof``)."""
    VARIANT = 0
    NAME = "ClofNet"


class ClofNet_vel(_ClofBase):
    """Drop-in for nn/state2state/clof/clof.py:ClofNet_vel (``--model clof_vel``)."""
    VARIANT = 1
    NAME = "ClofNet_vel"


class ClofNet_vel_gbf(_ClofBase):
    """Drop-in for nn/state2state/clof/clof.py:ClofNet_vel_gbf (``--model clof_vel_gbf``)."""
    VARIANT = 2
    NAME = "ClofNet_vel_gbf"
