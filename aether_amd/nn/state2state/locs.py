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

import torch

from ... import _lib
from ._frame import (FrameModule, _GNN, _f32, _f32g, _grads_alias_flat, _hand_over_grads, _pad_blocks, engine_shapes,
                     field_slot_shapes, place)
from ._paramgrad import _flat_grad_buffers


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


def aether_state_dict(state_dict, num_dims, hidden_size=None):
    """A LoCS ``state_dict`` as the ``state_dict`` of an ``Aether`` of width ``hidden_size`` (default: LoCS's own) that
    computes the same step: first-layer columns placed by ``_locs_blocks``, force columns zero, a zero field net."""
    D = num_dims
    H = state_dict["gnn.out_mlp.0.weight"].shape[0]
    kw = H if hidden_size is None else int(hidden_size)
    ref = next(iter(state_dict.values()))
    zeros = lambda shape: torch.zeros(shape, dtype=ref.dtype, device=ref.device)
    out = {n: place(zeros(shape), state_dict[n], _locs_blocks(n, state_dict[n].shape, D, H, kw))
           for n, shape in engine_shapes(D, kw).items()}
    out.update({k: zeros(shape) for k, shape in field_slot_shapes(D).items()})
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
        module = ctx.module
        x, vel, graph, ws, n_edges, _token = ctx.saved
        n_nodes = x.shape[0]
        plist = module._param_list()
        flat, views = module._grad_buffers()
        aliased = _grads_alias_flat(module, plist, views)
        dst_flat, dst_views = module._grad_buffers(second=True) if aliased else (flat, views)
        gs, kgrads = module._grad_struct(dst_views)
        ps = C.byref(module._struct(x.device))
        zero = module._zeros(n_nodes, x.device)
        g = grad_out.to(torch.float32).contiguous()
        grad_field = torch.empty(n_nodes, module.num_dims, dtype=torch.float32, device=x.device)    # dL/dfield: not needed
        module._backward("aether_backward_field", ps, C.byref(gs), x, vel, zero, graph, ws, n_edges, g, grad_field)
        # engine-shaped gradients (the mapped first-layer tensors; every GNN tensor of a narrow model) cut to LoCS's shapes
        module._cut(kgrads, dst_views)
        gx = gv = gea = None
        if any(ctx.needs_input_grad[1:4]):
            # the field does not depend on x / vel: field_input_grad is a zero [n_nodes][2D] buffer (None would mean "the
            # built-in field net")
            gx, gv, gea = module._input_grads(ctx.needs_input_grad[1:4], ps, x, vel, zero, graph, ws, n_edges,
                                              ctx.saved_tensors[0], g, zero)
        out = _hand_over_grads(module, plist, views, dst_flat, dst_views, aliased, ctx.needs_input_grad[_LoCSStep.N_FIXED:])
        return (None, gx, gv, gea, None, None) + tuple(out)


class LoCS(FrameModule):
    """Drop-in for nn/state2state/locs/locs.py:104-135."""

    # load_state_dict copies into the existing parameters in place: the buffers stay, only the engine images are out of date
    DROP_ON_LOAD = ("_img_key", "_wimg_key")

    def __init__(self, input_size, hidden_size, dropout_prob, num_dims, device="cuda"):
        super().__init__()
        self._frame_init("LoCS", 2 * num_dims, input_size, hidden_size, dropout_prob, num_dims)
        self.gnn = _GNN(input_size, hidden_size, dropout_prob, num_dims, additional_features=0)
        self.grad_as_view = True          # .grad tensors alias one flat buffer (see _LoCSStep.backward)
        self._reset_caches()
        self.to(device)
        self.params = self.__str__()

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
        self._ws = self._last_ws = None
        self._ws_key = None
        self._wimg_key = None
        self._train_ws, self._train_ws_token = None, None
        self._rollout_train_ws, self._rollout_train_ws_token = None, None

    # Every device buffer above may be baked into a captured step (GraphedTrainStep): they are dropped only when the
    # parameters themselves moved, which invalidates such a graph anyway.
    def _apply(self, fn, *a, **k):
        before = [(p.data_ptr(), p.device, p.dtype) for p in self.parameters()]
        out = super()._apply(fn, *a, **k)
        if [(p.data_ptr(), p.device, p.dtype) for p in self.parameters()] != before:
            self._reset_caches()          # parameter storage moved (.to / .cuda / .float)
        return out

    def _mapping(self, device):
        """{name: (rows, column index tensor or None, engine shape)} for every parameter the kernels cannot read as it
        is: the two first-layer tensors, and every GNN tensor of a model whose hidden_size is not a kernel width.  Each
        block of ``_locs_blocks`` keeps its rows; a column remap is one index_copy_ / index_select."""
        if self._maps is None:
            D, H, kw = self.num_dims, self.hidden_size, self._kw
            kshape = engine_shapes(D, kw)
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
            shapes = field_slot_shapes(self.num_dims)
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

    def _launch(self, x, vel, ea, graph, n_edges, train):
        """One step with the zero field (also the charges the kernels are handed) -> (out, workspace, token)."""
        self._images(x.device, train)
        zero = self._zeros(x.shape[0], x.device)
        return self._step("aether_forward_field", C.byref(self._struct(x.device)), x, vel, zero, zero, ea, graph, n_edges,
                          train)

    def _rollout_params(self, device):
        self._images(device, False)
        return C.byref(self._struct(device)), None

    def _rollout_train_params(self, device, refresh=True):
        # As ``rollout``, not as ``forward``: the rollout entries take no external field, so the engine's built-in field
        # net runs on its all-zero weights (``_dummies``) -- a field of exactly 0 and, in the backward, zero input
        # gradients through it; its parameter gradients go to ``_dummy_grad`` and are dropped.  The charges are the real
        # ones (the edge attribute q_i q_j); they only index the zero embedding.
        if refresh:
            self._images(device, True)
        return C.byref(self._struct(device))

    def _grad_destination(self):
        plist = self._param_list()
        flat, views = self._grad_buffers()
        aliased = _grads_alias_flat(self, plist, views)
        dst_flat, dst_views = self._grad_buffers(second=True) if aliased else (flat, views)
        # engine-shaped gradients (the mapped first-layer tensors; every GNN tensor of a narrow model) cut to LoCS's shapes
        gs, kgrads = self._grad_struct(dst_views)
        return plist, views, dst_flat, dst_views, aliased, C.byref(gs), lambda: self._cut(kgrads, dst_views)

    # -- reference surface -----------------------------------------------------------
    def forward(self, h, x, edges, vel, edge_attr_orig):
        """``h`` is ignored, as in the reference (locs.py:121-135)."""
        send, recv, n_nodes, E = self._validate_forward(x, vel, edges, edge_attr_orig)
        # differentiable in x / vel / edge_attr_orig, as the reference's forward (locs.py:121-135)
        wants_in = torch.is_grad_enabled() and (x.requires_grad or vel.requires_grad or edge_attr_orig.requires_grad)
        # nn.Dropout keys on the module's mode, not on autograd's: a train()-mode forward applies it even under no_grad
        drops = self.dropout_prob > 0.0 and self.training
        graph = self.prepare_graph((send, recv), n_nodes)
        plist = self._param_list()
        if wants_in or (torch.is_grad_enabled() and any(p.requires_grad for p in plist)):
            f32g = _f32g if wants_in else _f32
            return _LoCSStep.apply(self, f32g(x), f32g(vel), f32g(edge_attr_orig), graph, E, *plist)
        with torch.no_grad():
            return self._launch(_f32(x), _f32(vel), _f32(edge_attr_orig), graph, E, train=drops)[0]

    @torch.no_grad()
    def rollout(self, x, vel, edges, charges, steps, dt=1.0):
        """``steps`` autoregressive steps on the device (``aether_rollout``, the protocol of ``aether_amd.rollout``;
        ``FrameModule._rollout``).  ``charges`` feed only the product in ``edge_attr`` (experiments/lorentz/main.py:236-241);
        the engine's built-in field net has zero weights, so its field is exactly the zero field of ``forward``."""
        return self._rollout(x, vel, edges, charges, steps, dt)
