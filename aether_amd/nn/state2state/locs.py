"""MI355X drop-in for the reference ``nn.state2state.locs.locs.LoCS`` (the Lorentz runner's ``--model locs``,
experiments/lorentz/main.py:140-141,236-241).

Same constructor, ``forward(h, x, edges, vel, edge_attr_orig)`` signature (no ``charges``), ``state_dict`` keys / shapes /
order and seeded initialisation as nn/state2state/locs/locs.py:104-135.  LoCS is the GNN that Aether embeds, without the
field: its localizer builds Aether's features minus the force columns (no rotated forces on edges, no canonical forces in
``rel_feat``) and the GNN has ``additional_features=0``.  It therefore runs on Aether's kernels through the external-field
entry points (``aether_forward_field`` / ``aether_backward_field`` / ``aether_backward_inputs``) with a field of zeros and
Aether-shaped first-layer weights whose force columns stay zero (``_locs_blocks``): every force feature is then exactly 0
and the step computes LoCS exactly.  No new kernel, no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from ._paramgrad import _flat_grad_buffers
from .aether import GraphCache, _GNN, _hand_over_grads, _kernel_width, _pad_blocks, _train_workspace


def _locs_blocks(name, shape, num_dims, hidden_size, kw):
    """Where a LoCS parameter lives inside the same-named parameter of the Aether-shaped, kw-wide engine: a list of
    (source slices, destination slices), the rest of the engine tensor stays zero.  With O = D(D-1)/2:
      gnn.layer_1.message_fn.0.weight: columns [0, 3D+O) (local-frame edge features) -> [0, 3D+O),
                                       [3D+O, 5D+O) (rel_feat[recv] = [0, R^T v]) -> [4D+O, 6D+O),
                                       the last 2 (edge_attr_orig) -> the last 2;
      gnn.layer_1.res.weight:          columns [0, 2D) -> [0, 2D);
    the rows of both, and every other tensor, as ``_pad_blocks`` places a narrow model in its padded engine."""
    D, H = num_dims, hidden_size
    O = D * (D - 1) // 2
    if name == "gnn.layer_1.message_fn.0.weight":
        L = 3 * D + O
        cols = ((0, L, 0), (L, 2 * D, 4 * D + O), (5 * D + O, 2, 7 * D + O))      # (source start, width, engine start)
        return [((slice(0, H), slice(s, s + w)), (slice(0, H), slice(d, d + w))) for s, w, d in cols]
    if name == "gnn.layer_1.res.weight":
        return [((slice(0, H), slice(0, 2 * D)), (slice(0, H), slice(0, 2 * D)))]
    return _pad_blocks(name, shape, H, kw)


_FIELD_SHAPES = lambda D: {"field_net.net.0.weight": (32, 2 * D + 16), "field_net.net.0.bias": (32,),
                           "field_net.net.2.weight": (32, 32), "field_net.net.2.bias": (32,),
                           "field_net.net.4.weight": (D, 32), "field_net.net.4.bias": (D,),
                           "field_net.class_embedding.weight": (3, 16)}


def aether_state_dict(state_dict, num_dims, hidden_size=None):
    """A LoCS ``state_dict`` as the ``state_dict`` of an ``Aether`` of width ``hidden_size`` (default: LoCS's own) that
    computes the same step: first-layer columns placed by ``_locs_blocks``, force columns zero, a zero field net."""
    D = num_dims
    H = state_dict["gnn.out_mlp.0.weight"].shape[0]
    kw = H if hidden_size is None else int(hidden_size)
    ref = next(iter(state_dict.values()))
    with torch.device("meta"):
        wide = _GNN(2 * D, kw, 0.0, D, additional_features=D)
    out = {}
    for n, p in wide.named_parameters():
        n = "gnn." + n
        t = torch.zeros(p.shape, dtype=ref.dtype, device=ref.device)
        src = state_dict[n]
        for ss, ds in _locs_blocks(n, src.shape, D, H, kw):
            t[ds] = src[ss]
        out[n] = t
    out.update({k: torch.zeros(s, dtype=ref.dtype, device=ref.device) for k, s in _FIELD_SHAPES(D).items()})
    return out


class _LoCSStep(torch.autograd.Function):
    """aether_forward_field / aether_backward_field (+ aether_backward_inputs) with a zero field behind torch.autograd."""

    N_FIXED = 6          # module, x, vel, edge_attr, graph, n_edges precede the parameters

    @staticmethod
    def forward(ctx, module, x, vel, ea, graph, n_edges, *params):
        out, ws, token = module._launch(x, vel, ea, graph, n_edges, train=True)
        ctx.module, ctx.saved = module, (x, vel, graph, ws, n_edges, token)
        if any(ctx.needs_input_grad[1:4]):       # x / vel / edge_attr: aether_backward_inputs recovers y = R^T (out - x)
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        module = ctx.module
        x, vel, (graph, ginfo), ws, n_edges, _token = ctx.saved
        D, n_nodes, kw = module.num_dims, x.shape[0], module._kw
        plist = module._param_list()
        flat, views = module._grad_buffers()
        # the kernels OVERWRITE their destination: when a .grad already is a view of the flat buffer (a second backward
        # without zero_grad), they write into a second buffer and the result is added
        aliased = module.grad_as_view and any(p.grad is not None and p.grad.data_ptr() == v.data_ptr()
                                              for p, v in zip(plist, views))
        dst_flat, dst_views = module._grad_buffers(second=True) if aliased else (flat, views)
        gs, kgrads = module._grad_struct(dst_views)
        zero = module._zeros(n_nodes, x.device)
        g = grad_out.to(torch.float32).contiguous()
        grad_field = torch.empty(n_nodes, D, dtype=torch.float32, device=x.device)       # dL/dfield: not needed
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if kw == 64:
            st = lib.aether_backward_field(C.byref(module._struct(x.device)), C.byref(gs), D, n_nodes, n_edges, x.data_ptr(),
                                           vel.data_ptr(), zero.data_ptr(), graph.data_ptr(), C.byref(ginfo), ws.data_ptr(),
                                           ws.numel(), g.data_ptr(), grad_field.data_ptr(), stream)
        else:
            st = lib.aether_backward_h(C.byref(module._struct(x.device)), C.byref(gs), D, kw, n_nodes, n_edges, x.data_ptr(),
                                       vel.data_ptr(), zero.data_ptr(), graph.data_ptr(), C.byref(ginfo), ws.data_ptr(),
                                       ws.numel(), g.data_ptr(), grad_field.data_ptr(), stream)
        _lib.check(st, "aether_backward_field")
        # engine-shaped gradients (the mapped first-layer tensors; every GNN tensor of a narrow model) cut to LoCS's shapes
        module._cut(kgrads, dst_views)
        gx = gv = gea = None
        if any(ctx.needs_input_grad[1:4]):
            # the field does not depend on x / vel: field_input_grad is a zero [n_nodes][2D] buffer (NULL would mean "the
            # built-in field net")
            (out_saved,) = ctx.saved_tensors
            gx, gv = torch.empty_like(x), torch.empty_like(x)
            if ctx.needs_input_grad[3]:
                gea = torch.empty(n_edges, 2, dtype=torch.float32, device=x.device)
            st = lib.aether_backward_inputs_h(C.byref(module._struct(x.device)), D, kw, n_nodes, n_edges, x.data_ptr(),
                                              vel.data_ptr(), zero.data_ptr(), graph.data_ptr(), C.byref(ginfo),
                                              ws.data_ptr(), ws.numel(), out_saved.data_ptr(), g.data_ptr(), gx.data_ptr(),
                                              gv.data_ptr(), gea.data_ptr() if gea is not None else None, zero.data_ptr(),
                                              stream)
            _lib.check(st, "aether_backward_inputs")
            if not ctx.needs_input_grad[1]:
                gx = None
            if not ctx.needs_input_grad[2]:
                gv = None
        out = _hand_over_grads(module, plist, views, dst_flat, dst_views, aliased, ctx.needs_input_grad[_LoCSStep.N_FIXED:])
        return (None, gx, gv, gea, None, None) + tuple(out)


class LoCS(nn.Module):
    """Drop-in for nn/state2state/locs/locs.py:104-135."""

    def __init__(self, input_size, hidden_size, dropout_prob, num_dims, device="cuda"):
        super().__init__()
        if not (1 <= hidden_size <= 4096):
            raise ValueError("hidden_size must lie in [1, 4096] (experiments/lorentz/main.py:42-43)")
        if num_dims not in (2, 3) or input_size != 2 * num_dims:
            raise ValueError("num_dims must be 2 or 3 and input_size == 2*num_dims")
        if hidden_size == 2 * num_dims:
            raise ValueError("hidden_size == 2 * num_dims is not supported (the reference then builds layer_1 without its "
                             "res Linear, locs.py:214-218)")
        if not (0.0 <= float(dropout_prob) < 1.0):
            raise ValueError("dropout_prob must lie in [0, 1)")
        # nn.Dropout in out_mlp (locs.py:160-168): identity in eval(); in train() with p > 0 the two scale masks (drawn with
        # bernoulli_, same distribution as nn.Dropout, not its random stream), as Aether
        self.dropout_prob = float(dropout_prob)
        self.gnn = _GNN(input_size, hidden_size, dropout_prob, num_dims, additional_features=0)
        self.num_dims = num_dims
        self.hidden_size = hidden_size
        # width the kernels run this model at: 64 (fused / streamed), or the next multiple of 64 above (csrc/wide.h)
        self._kw = _kernel_width(hidden_size)
        self._graphs = GraphCache()
        self.flags = 0                    # _lib.FLAG_* bits passed to the forward
        self.dp_group = None              # set by aether_amd.parallel.attach_data_parallel
        self.grad_as_view = True          # .grad tensors alias one flat buffer (see _LoCSStep.backward)
        self._reset_caches()
        self.to(device)
        self.params = self.__str__()

    def __str__(self):
        params = sum(int(np.prod(p.size())) for p in self.parameters() if p.requires_grad)
        print("Network Size", params)
        return str(params)

    # -- plumbing ------------------------------------------------------------------
    def _reset_caches(self):
        self._plist = None
        self._maps = None                 # {name: (rows, column index or None, engine shape)} of the engine-shaped tensors
        self._img = None                  # those tensors (zero outside LoCS's blocks)
        self._img_key = None              # parameter versions the images were last copied from (inference)
        self._dummy = None                # the field net's AetherParams slots: zeros, never a gradient destination
        self._dummy_grad = None
        self._kgrad = None                # engine-shaped gradient scratch of the mapped tensors
        self._pstruct = None
        self._gstruct = None
        self._gbuf = None
        self._gbuf2 = None
        self._zero = None
        self._zero_kept = []              # zero buffers a captured graph may still read (see _zeros)
        self._ws = None
        self._ws_key = None
        self._wimg_key = None
        self._train_ws, self._train_ws_token = None, None

    # Every device buffer above may be baked into a captured step (GraphedTrainStep): they are dropped only when the
    # parameters themselves moved, which invalidates such a graph anyway.
    def _apply(self, fn, *a, **k):
        before = [(p.data_ptr(), p.device, p.dtype) for p in self.parameters()]
        out = super()._apply(fn, *a, **k)
        if [(p.data_ptr(), p.device, p.dtype) for p in self.parameters()] != before:
            self._reset_caches()          # parameter storage moved (.to / .cuda / .float)
        return out

    def load_state_dict(self, *a, **k):
        # copies into the existing parameters in place: the buffers stay, only the engine images are out of date
        self._img_key = None
        self._wimg_key = None
        return super().load_state_dict(*a, **k)

    def _param_list(self):
        if self._plist is None:           # nn.Module.parameters() walks the module tree: keep the list
            self._plist = [p for _, p in self.named_parameters()]
        return self._plist

    def _mapping(self, device):
        """{name: (rows, column index tensor or None, engine shape)} for every parameter the kernels cannot read as it
        is: the two first-layer tensors, and every GNN tensor of a model whose hidden_size is not a kernel width.  Each
        block of ``_locs_blocks`` keeps its rows; a column remap is one index_copy_ / index_select."""
        if self._maps is None:
            D, H, kw = self.num_dims, self.hidden_size, self._kw
            with torch.device("meta"):
                wide = _GNN(2 * D, kw, 0.0, D, additional_features=D)
            kshape = {"gnn." + n: tuple(p.shape) for n, p in wide.named_parameters()}
            maps = {}
            for n, p in self.named_parameters():
                if tuple(p.shape) == kshape[n] and n not in ("gnn.layer_1.message_fn.0.weight", "gnn.layer_1.res.weight"):
                    continue
                blocks = _locs_blocks(n, p.shape, D, H, kw)
                rows = p.shape[0]
                assert all(ss[0] == slice(0, rows) and ds[0] == slice(0, rows) for ss, ds in blocks)
                if p.dim() == 1:
                    maps[n] = (rows, None, kshape[n])
                    continue
                cols = []
                for ss, ds in blocks:                          # source blocks are consecutive and cover every column
                    assert ss[1].start == len(cols)
                    cols += range(ds[1].start, ds[1].stop)
                assert len(cols) == p.shape[1]
                idx = torch.tensor(cols, dtype=torch.int64, device=device)
                maps[n] = (rows, None if cols == list(range(p.shape[1])) else idx, kshape[n])
            self._maps = maps
        return self._maps

    def _images(self, device, train):
        """The engine-shaped tensors, refreshed from the parameters when any of them changed -- and always in training (an
        optimizer step lies between two training forwards and leaves the version counters alone inside a captured step:
        the copies have to be part of the graph)."""
        maps = self._mapping(device)
        self._image_tensors(device)
        plist = self._param_list()
        key = tuple((p.data_ptr(), p._version) for p in plist)
        if train or self._img_key != key:
            with torch.no_grad():
                for n, p in self.named_parameters():
                    m = maps.get(n)
                    if m is None:
                        continue
                    rows, idx, _ = m
                    img = self._img[n]
                    if idx is not None:
                        img[:rows].index_copy_(1, idx, p)
                    elif p.dim() == 1:
                        img[:rows].copy_(p)
                    else:
                        img[:rows, :p.shape[1]].copy_(p)
            self._img_key = None if train else key
        return self._img

    def _image_tensors(self, device):
        if self._img is None:
            self._img = {n: torch.zeros(m[2], dtype=torch.float32, device=device) for n, m in self._mapping(device).items()}
            self._img_key = None
        return self._img

    def _dummies(self, device):
        if self._dummy is None:
            shapes = _FIELD_SHAPES(self.num_dims)
            self._dummy = {k: torch.zeros(s, dtype=torch.float32, device=device) for k, s in shapes.items()}
            self._dummy_grad = {k: torch.zeros(s, dtype=torch.float32, device=device) for k, s in shapes.items()}
        return self._dummy

    def _struct(self, device):
        """AetherParams of the engine: LoCS's own tensors where the kernels can read them, the images elsewhere, a zero
        field net (its output is exactly 0: the built-in field of aether_rollout is the zero field too)."""
        plist = self._param_list()
        key = tuple(p.data_ptr() for p in plist)
        if self._pstruct is None or self._pstruct[0] != key:
            tensors = dict(self.named_parameters())
            tensors.update(self._image_tensors(device))
            tensors.update(self._dummies(device))
            self._pstruct = (key, _lib.params_struct(tensors))
        return self._pstruct[1]

    def _grad_buffers(self, second=False):
        """Flat fp32 gradient buffer and per-parameter views into it: every tensor at the next multiple of 4 floats, in
        named_parameters() order (Aether._grad_buffers' layout; GraphedTrainStep, FusedAdamW and data parallelism use it).
        ``second``: a scratch buffer of the same layout, the destination of a backward whose result is ADDED to
        gradients that already live in the first one."""
        return _flat_grad_buffers(self, second)

    def _grad_struct(self, dst_views):
        """AetherParams of gradient destinations: the views themselves where the shapes agree, engine-shaped scratch for
        the mapped tensors (cut back by ``_cut``) -> (struct, {name: scratch})."""
        key = dst_views[0].data_ptr()
        if self._gstruct is None or self._gstruct[0] != key:
            dev = dst_views[0].device
            maps = self._mapping(dev)
            if self._kgrad is None:
                self._kgrad = {n: torch.zeros(m[2], dtype=torch.float32, device=dev) for n, m in maps.items()}
            self._dummies(dev)
            tensors = {n: v for (n, _), v in zip(self.named_parameters(), dst_views)}
            tensors.update(self._kgrad)
            tensors.update(self._dummy_grad)
            self._gstruct = (key, _lib.params_struct(tensors))
        return self._gstruct[1], self._kgrad

    def _cut(self, kgrads, dst_views):
        maps = self._mapping(dst_views[0].device)
        for (n, p), v in zip(self.named_parameters(), dst_views):
            m = maps.get(n)
            if m is None:
                continue
            rows, idx, _ = m
            g = kgrads[n]
            if idx is not None:
                torch.index_select(g[:rows], 1, idx, out=v)
            elif p.dim() == 1:
                v.copy_(g[:rows])
            else:
                v.copy_(g[:rows, :p.shape[1]])

    def _zeros(self, n_nodes, device):
        """One zero buffer of n_nodes * 2D floats: the field ([n][D], its first half), field_input_grad ([n][2D]) and the
        charges the kernels are handed ([n], not read for the result: they only index the zero field net's embedding)."""
        need = n_nodes * 2 * self.num_dims
        if self._zero is None or self._zero.numel() < need or self._zero.device != device:
            # a captured step may hold the old buffer's address: keep it alive rather than free it (growth is rare)
            if self._zero is not None:
                self._zero_kept.append(self._zero)
            self._zero = torch.zeros(need, dtype=torch.float32, device=device)
        return self._zero

    def _may_reuse_weight_images(self):
        # as Aether: while a hipGraph is being captured the decision is baked into the graph; only in eval mode
        return not (self.training and torch.cuda.is_current_stream_capturing())

    def _launch(self, x, vel, ea, graph, n_edges, train):
        lib = _lib.load()
        graph, ginfo = graph
        n_nodes, D, E, kw = x.shape[0], self.num_dims, n_edges, self._kw
        self._images(x.device, train)
        ps = self._struct(x.device)
        zero = self._zeros(n_nodes, x.device)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        flags = self.flags & ~_lib.FLAG_KEEP_INTERMEDIATES
        if kw != 64:
            flags &= ~(_lib.FLAG_FORCE_FUSED | _lib.FLAG_FORCE_STREAMED)
        ws_key = wkey = token = None
        if train:                          # the backward reads this forward's intermediates (reused as in Aether)
            ws, token = _train_workspace(self, lib.aether_workspace_bytes_h(n_nodes, E, D, kw, 1), x.device)
            flags |= _lib.FLAG_KEEP_INTERMEDIATES | (0 if self.flags & _lib.FLAG_KEEP_INTERMEDIATES else _lib.FLAG_BACKWARD_ONLY)
            if self.dropout_prob > 0.0 and self.training:
                # nn.Dropout after the two SiLUs of the out MLP (locs.py:163,166): scale masks into the training workspace
                off = lib.aether_dropout_mask_offset_h(n_nodes, E, D, kw)
                masks = ws[off:off + 2 * n_nodes * kw * 4].view(torch.float32).view(2, n_nodes, kw)
                given = self.__dict__.get("_dropout_masks")          # tests: explicit masks [2, n_nodes, width]
                if given is not None and given.shape[-1] != kw:      # a narrow model's masks: padded channels are zero anyway
                    given = torch.nn.functional.pad(given, (0, kw - given.shape[-1]), value=1.0)
                if given is not None:
                    masks.copy_(given.to(device=x.device, dtype=torch.float32))
                else:
                    masks.bernoulli_(1.0 - self.dropout_prob).mul_(1.0 / (1.0 - self.dropout_prob))
                flags |= _lib.FLAG_DROPOUT
            self._wimg_key = None          # an optimizer step follows: the weight images in the inference workspace go stale
        else:
            ws_bytes = lib.aether_workspace_bytes_h(n_nodes, E, D, kw, 0)
            if self._ws is None or self._ws.numel() < ws_bytes or self._ws.device != x.device:
                self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
            ws = self._ws
            # same buffer and shape as the last completed inference call: hand-off words re-armed, split weight images
            # still current (the key holds the parameters' versions and addresses), as in Aether
            fused = kw == 64 and ginfo.n_groups > 0 and E > 0 and not (flags & _lib.FLAG_FORCE_STREAMED)
            ws_key = (ws.data_ptr(), n_nodes, E, D, graph.data_ptr()) if fused else None
            if ws_key is not None and self._ws_key == ws_key:
                flags |= _lib.FLAG_WORKSPACE_REUSED
            wkey = (ws_key, tuple(p._version for p in self._param_list()), tuple(p.data_ptr() for p in self._param_list()))
            if ws_key is not None and self._wimg_key == wkey and self._may_reuse_weight_images():
                flags |= _lib.FLAG_WEIGHTS_PREPARED
        self._ws_key = None
        self._wimg_key = None
        out = torch.empty_like(x)
        if kw == 64:
            st = lib.aether_forward_field(C.byref(ps), D, n_nodes, E, x.data_ptr(), vel.data_ptr(), zero.data_ptr(),
                                          zero.data_ptr(), ea.data_ptr(), graph.data_ptr(), C.byref(ginfo),
                                          ws.data_ptr(), ws.numel(), out.data_ptr(), flags, stream)
        else:       # hidden_size > 64: csrc/wide.h with the external field
            st = lib.aether_forward_h(C.byref(ps), D, kw, n_nodes, E, x.data_ptr(), vel.data_ptr(), zero.data_ptr(),
                                      zero.data_ptr(), ea.data_ptr(), graph.data_ptr(), C.byref(ginfo),
                                      ws.data_ptr(), ws.numel(), out.data_ptr(), flags, stream)
        _lib.check(st, "aether_forward_field")
        if not train:
            self._ws_key, self._wimg_key = ws_key, wkey
        return out, ws, token

    def prepare_graph(self, edges, n_nodes):
        """Build (or fetch) the receiver-sorted view for ``edges = [send, recv]``."""
        send, recv = edges
        return self._graphs.get(send.contiguous(), recv.contiguous(), n_nodes)

    # -- reference surface -----------------------------------------------------------
    def forward(self, h, x, edges, vel, edge_attr_orig):
        """``h`` is ignored, as in the reference (locs.py:121-135)."""
        if not x.is_cuda:
            raise _lib.AetherHipError("aether_amd.LoCS runs on an MI355X only; got a CPU tensor (there is no CPU fallback)")
        send, recv = edges
        if send.dtype != torch.int64 or recv.dtype != torch.int64:
            raise TypeError("edges must be int64 (torch.LongTensor), as in the reference")
        n_nodes, D = x.shape
        if D != self.num_dims or vel.shape != x.shape:
            raise ValueError(f"x/vel must be [n_nodes, {self.num_dims}]")
        E = send.numel()
        if recv.numel() != E or edge_attr_orig.shape != (E, 2):
            raise ValueError("edge index / edge_attr shapes do not match")
        # differentiable in x / vel / edge_attr_orig, as the reference's forward (locs.py:121-135)
        wants_in = torch.is_grad_enabled() and (x.requires_grad or vel.requires_grad or edge_attr_orig.requires_grad)
        # nn.Dropout keys on the module's mode, not on autograd's: a train()-mode forward applies it even under no_grad
        drops = self.dropout_prob > 0.0 and self.training
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        f32g = (lambda t: t.to(torch.float32).contiguous() if t.requires_grad else f32(t)) if wants_in else f32
        graph = self.prepare_graph((send, recv), n_nodes)
        plist = self._param_list()
        if wants_in or (torch.is_grad_enabled() and any(p.requires_grad for p in plist)):
            return _LoCSStep.apply(self, f32g(x), f32g(vel), f32g(edge_attr_orig), graph, E, *plist)
        with torch.no_grad():
            return self._launch(f32(x), f32(vel), f32(edge_attr_orig), graph, E, train=drops)[0]

    # -- device rollout ---------------------------------------------------------------
    @torch.no_grad()
    def rollout(self, x, vel, edges, charges, steps, dt=1.0):
        """``steps`` autoregressive steps on the device (``aether_rollout``, the protocol of ``aether_amd.rollout``):
        x_{t+1} = self(x_t, v_t), v_{t+1} = (x_{t+1} - x_t) / dt, ``edge_attr = [q_i q_j, |x_i - x_j|]`` rebuilt inside
        the kernels every step (experiments/lorentz/main.py:236-241).  ``charges`` feed only that product; the engine's
        built-in field net has zero weights, so its field is exactly the zero field of ``forward``."""
        if not x.is_cuda:
            raise _lib.AetherHipError("aether_amd.LoCS runs on an MI355X only; got a CPU tensor (there is no CPU fallback)")
        if self.dropout_prob > 0.0 and self.training:
            raise RuntimeError("LoCS.rollout is an inference path (no dropout masks): call .eval() first")
        lib = _lib.load()
        send, recv = edges
        if send.dtype != torch.int64 or recv.dtype != torch.int64:
            raise TypeError("edges must be int64 (torch.LongTensor), as in the reference")
        n_nodes, D = x.shape
        if D != self.num_dims or vel.shape != x.shape or charges.numel() != n_nodes:
            raise ValueError(f"x/vel must be [n_nodes, {self.num_dims}], charges [n_nodes, 1]")
        E = send.numel()
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        x, vel, charges = f32(x), f32(vel), f32(charges)
        graph, ginfo = self.prepare_graph((send, recv), n_nodes)
        self._images(x.device, False)
        ps = self._struct(x.device)
        kw = self._kw
        ws_bytes = lib.aether_workspace_bytes_h(n_nodes, E, D, kw, 0)
        if self._ws is None or self._ws.numel() < ws_bytes or self._ws.device != x.device:
            self._ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
        self._ws_key = self._wimg_key = None      # the rollout leaves the workspace's hand-off words in their own state
        traj = torch.empty(int(steps), n_nodes, D, dtype=torch.float32, device=x.device)
        if int(steps) <= 0:
            return traj
        flags = self.flags & ~_lib.FLAG_KEEP_INTERMEDIATES
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if kw == 64:
            st = lib.aether_rollout(C.byref(ps), D, n_nodes, E, x.data_ptr(), vel.data_ptr(), charges.data_ptr(),
                                    graph.data_ptr(), C.byref(ginfo), self._ws.data_ptr(), self._ws.numel(), traj.data_ptr(),
                                    int(steps), float(dt), flags, stream)
        else:
            st = lib.aether_rollout_h(C.byref(ps), D, kw, n_nodes, E, x.data_ptr(), vel.data_ptr(), charges.data_ptr(),
                                      graph.data_ptr(), C.byref(ginfo), self._ws.data_ptr(), self._ws.numel(), traj.data_ptr(),
                                      int(steps), float(dt), 0, stream)
        _lib.check(st, "aether_rollout")
        return traj
