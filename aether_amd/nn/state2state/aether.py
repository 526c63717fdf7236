"""MI355X drop-in for the reference ``nn.state2state.aether.Aether``.

Same constructor, ``forward(h, x, edges, vel, edge_attr_orig, charges)`` signature and
``state_dict`` keys/shapes as nn/state2state/aether.py:142-186, so a
checkpoint saved by either loads into the other.  The computation runs in
``libaether_hip.so`` (hand-written gfx950 kernels, include/aether_hip.h); there is no
PyTorch or CPU fallback -- on a machine without the library or a GPU tensor the call
raises.  The plumbing shared with ``DynamicFieldAether`` and ``LoCS`` is ``_frame.FrameModule``.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from ... import _lib
from ._frame import (FrameModule, GraphCache, _GNN, _f32, _f32g, _grads_alias_flat, _hand_over_grads,  # noqa: F401
                     _kernel_width, _pad_blocks, _train_workspace, cut, place)


class _AetherStep(torch.autograd.Function):
    """aether_forward / aether_backward behind torch.autograd (parameters only get gradients:
    the runner detaches positions and edge attributes, experiments/lorentz/main.py:243-247)."""

    N_FIXED = 7          # module, x, vel, edge_attr, charges, graph, n_edges precede the parameters

    @staticmethod
    def forward(ctx, module, x, vel, edge_attr, charges, graph, n_edges, *params):
        # only the training path comes through here (inside Function.forward grad mode is always off and
        # needs_input_grad reflects requires_grad even under torch.no_grad(): the caller decides)
        out, ws, token = module._step("aether_forward", module._param_struct_ref(), x, vel, charges, None, edge_attr,
                                      graph, n_edges, True)
        ctx.module = module
        ctx.saved = (x, vel, charges, graph, ws, n_edges, token)
        if any(ctx.needs_input_grad[1:4]):       # x / vel / edge_attr: aether_backward_inputs recovers y = R^T (out - x)
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        module = ctx.module
        x, vel, charges, graph, ws, n_edges, _token = ctx.saved
        flat, gstruct, views = module._grad_buffers()
        plist = module._param_list()
        aliased = _grads_alias_flat(module, plist, views)
        if aliased:
            dst_flat, dst_struct, dst_views = module._grad_buffers(second=True)
        else:
            dst_flat, dst_struct, dst_views = flat, gstruct, views
        g = grad_out.to(torch.float32).contiguous()
        ps = module._param_struct_ref()
        module._backward("aether_backward", ps, C.byref(dst_struct), x, vel, charges, graph, ws, n_edges, g)
        gx = gv = gea = None
        if any(ctx.needs_input_grad[1:4]):
            # gradients w.r.t. the inputs (the reference's forward is differentiable in them, aether.py:169-186): one more
            # kernel over what aether_backward left in the workspace
            gx, gv, gea = module._input_grads(ctx.needs_input_grad[1:4], ps, x, vel, charges, graph, ws, n_edges,
                                              ctx.saved_tensors[0], g)
        # hand the gradients over as views of the flat buffer (no 47 small copies)
        out = _hand_over_grads(module, plist, views, dst_flat, dst_views, aliased, ctx.needs_input_grad[_AetherStep.N_FIXED:])
        return (None, gx, gv, gea, None, None, None) + tuple(out)


class _PaddedStep(torch.autograd.Function):
    """forward / backward of a model whose hidden_size is not a kernel width (64, or a multiple of 64 above) through its
    zero-padded engine of that width (same kernels): the engine's autograd node is recorded in an inner graph, its
    parameter gradients are cut back to the narrow shapes."""

    N_FIXED = 7

    @staticmethod
    def forward(ctx, outer, x, send, recv, vel, edge_attr, charges, *params):
        eng = outer._engine
        # inputs that need a gradient become leaves of the inner graph
        need_in = (ctx.needs_input_grad[1], ctx.needs_input_grad[4], ctx.needs_input_grad[5])
        inner = [t.detach().requires_grad_(True) if n else t for t, n in zip((x, vel, edge_attr), need_in)]
        with torch.enable_grad():
            out = eng(None, inner[0], [send, recv], inner[1], inner[2], charges)
        ctx.outer, ctx.inner_out = outer, out
        ctx.inner_inputs = [t for t, n in zip(inner, need_in) if n]
        return out.detach()

    @staticmethod
    def backward(ctx, grad_out):
        outer = ctx.outer
        eng = outer._engine
        eparams = [p for _, p in eng.named_parameters()]
        grads = torch.autograd.grad(ctx.inner_out, eparams + ctx.inner_inputs, grad_out.contiguous(), allow_unused=True)
        gin = list(grads[len(eparams):])
        grads = grads[:len(eparams)]
        need_in = (ctx.needs_input_grad[1], ctx.needs_input_grad[4], ctx.needs_input_grad[5])
        gx, gv, gea = (gin.pop(0) if n else None for n in need_in)
        need = ctx.needs_input_grad[_PaddedStep.N_FIXED:]
        out = [cut(torch.empty_like(p), g, _pad_blocks(name, p.shape, outer.hidden_size, outer._kw))
               if n and g is not None else None for (name, p), g, n in zip(outer.named_parameters(), grads, need)]
        if outer.dp_group is not None:             # data-parallel: one all-reduce of the narrow gradients, flat
            import torch.distributed as dist
            have = [g for g in out if g is not None]
            flat = torch.cat([g.reshape(-1) for g in have])
            dist.all_reduce(flat, group=outer.dp_group)
            flat.div_(dist.get_world_size(outer.dp_group))
            torch._foreach_copy_(have, [c.view_as(g) for c, g in zip(flat.split([g.numel() for g in have]), have)])
        return (None, gx, None, None, gv, gea, None) + tuple(out)


class _FieldNetwork(nn.Module):
    """Parameter holder with the reference's names (aether.py:108-121)."""

    def __init__(self, num_dims, hidden_size, class_embedding_dim):
        super().__init__()
        self.num_dims = num_dims
        self.net = nn.Sequential(
            nn.Linear(2 * num_dims + class_embedding_dim, hidden_size), nn.SiLU(),
            nn.Linear(hidden_size, hidden_size), nn.SiLU(),
            nn.Linear(hidden_size, num_dims))
        self.class_embedding = nn.Embedding(3, class_embedding_dim)


class Aether(FrameModule):
    """Drop-in for nn/state2state/aether.py:142-186."""

    # forcing the 64-wide fused kernel on a wider model stays the library's error
    WIDE_FORWARD_STRIP = _lib.FLAG_FORCE_STREAMED
    EVAL_KEEP = True
    DROP_ON_APPLY = ("_pstruct", "_plist", "_gbuf", "_gbuf2")
    DROP_ON_LOAD = ("_pstruct", "_plist")

    def __init__(self, input_size, hidden_size, dropout_prob, num_dims, device="cuda"):
        super().__init__()
        self._frame_init("Aether", 3 * num_dims, input_size, hidden_size, dropout_prob, num_dims)
        self.gnn = _GNN(input_size, hidden_size, dropout_prob, num_dims,
                        additional_features=num_dims)
        self.field_net = _FieldNetwork(num_dims, 32, 16)
        self.grad_as_view = True          # .grad tensors alias one flat buffer (see _AetherStep.backward)
        self._train_ws, self._train_ws_token = None, None
        self._gbuf = None
        self._gbuf2 = None
        self._pstruct = None
        self.to(device)
        if hidden_size != self._kw:
            # the engine of kernel width: same class, its parameters are the zero-padded images of this model's (kept out of
            # state_dict / parameters(); its random initialisation is discarded and must not consume this model's RNG stream)
            import contextlib, io
            with torch.random.fork_rng(devices=[]), contextlib.redirect_stdout(io.StringIO()):
                eng = Aether(input_size, self._kw, dropout_prob, num_dims, device=device)
            eng.grad_as_view = False
            eng.requires_grad_(True)
            with torch.no_grad():
                for p_ in eng.parameters():
                    p_.zero_()
            self.__dict__["_engine"] = eng
            self.__dict__["_engine_key"] = None
        self.params = self.__str__()

    # -- plumbing ------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        eng = self.__dict__.get("_engine")
        if eng is not None:
            eng._apply(fn, *a, **k)
            self.__dict__["_engine_key"] = None
        return super()._apply(fn, *a, **k)

    def _sync_engine(self):
        """Copy this model's parameters into their places in the padded engine when any of them changed."""
        eng = self._engine
        plist = self._param_list()
        key = tuple((p.data_ptr(), p._version) for p in plist)
        # Training: always (an optimizer step lies between two training forwards and torch's fused AdamW leaves the version
        # counters alone; inside a captured training step the copies have to be part of the graph), and the call after a
        # training forward as well.
        train = torch.is_grad_enabled() and any(p.requires_grad for p in plist)
        if self._engine_key != key or train:
            with torch.no_grad():
                for (name, p), (_, ep) in zip(self.named_parameters(), eng.named_parameters()):
                    place(ep, p, _pad_blocks(name, p.shape, self.hidden_size, self._kw))
            self.__dict__["_engine_key"] = None if train else key
        eng.flags = self.flags
        eng.train(self.training)
        return eng

    def _param_struct(self):
        key = tuple([p.data_ptr() for p in self._param_list()])
        if self._pstruct is None or self._pstruct[0] != key:
            struct = _lib.params_struct(dict(self.named_parameters()))
            self._pstruct = (key, struct, C.byref(struct))
        return self._pstruct[1]

    def _param_struct_ref(self):
        self._param_struct()
        return self._pstruct[2]

    def _rollout_params(self, device):
        return self._param_struct_ref(), None

    def _rollout_train_params(self, device, refresh=True):
        return self._param_struct_ref()

    def _grad_destination(self):
        flat, gstruct, views = self._grad_buffers()
        plist = self._param_list()
        aliased = _grads_alias_flat(self, plist, views)
        dst_flat, dst_struct, dst_views = self._grad_buffers(second=True) if aliased else (flat, gstruct, views)
        return plist, views, dst_flat, dst_views, aliased, C.byref(dst_struct), None

    def _grad_buffers(self, second=False):
        """Flat fp32 gradient buffer + an AetherParams struct and per-parameter views into it.  ``second``: a
        scratch buffer of the same layout, the destination of a backward whose result has to be ADDED to gradients
        that already live in the first one."""
        slot = "_gbuf2" if second else "_gbuf"
        cur = getattr(self, slot, None)
        if cur is not None and self._plist is not None and cur[0].device == self._plist[0].device:
            return cur                        # parameter set and device unchanged (both reset _plist / _gbuf)
        named = list(self.named_parameters())
        total = sum((p.numel() + 3) // 4 * 4 for _, p in named)       # every tensor padded to 16 bytes (below)
        dev = named[0][1].device
        if cur is None or cur[0].device != dev or cur[0].numel() != total:
            # every tensor starts on a 16-byte boundary (the kernels use 16-byte accesses)
            offs, off = [], 0
            for _, p in named:
                offs.append(off)
                off += (p.numel() + 3) // 4 * 4
            flat = torch.zeros(off, dtype=torch.float32, device=dev)
            views = [flat[o:o + p.numel()].view_as(p) for o, (_, p) in zip(offs, named)]
            gstruct = _lib.params_struct({n: v for (n, _), v in zip(named, views)})
            cur = (flat, gstruct, views)
            setattr(self, slot, cur)
        return cur

    # -- reference surface -----------------------------------------------------------
    def forward(self, h, x, edges, vel, edge_attr_orig, charges):
        """``h`` is ignored, as in the reference (aether.py:169-186)."""
        send, recv, n_nodes, E = self._validate_forward(x, vel, edges, edge_attr_orig, charges)
        # the reference's forward is differentiable in x / vel / edge_attr_orig (aether.py:169-186): so is this one
        # (aether_backward_inputs); charges are an embedding index, no gradient flows to them there either
        wants_in = torch.is_grad_enabled() and (x.requires_grad or vel.requires_grad or edge_attr_orig.requires_grad)
        # nn.Dropout keys on the module's mode, not on autograd's: a train()-mode forward applies it even under no_grad
        drops = self.dropout_prob > 0.0 and self.training
        f32g = _f32g if wants_in else _f32
        narrow = self.hidden_size != self._kw      # not a kernel width: the zero-padded engine computes it (same kernels)
        eng = self._sync_engine() if narrow else None
        plist = self._param_list()
        train = drops or wants_in or (torch.is_grad_enabled() and any(p.requires_grad for p in plist))
        if narrow:
            if not train:
                with torch.no_grad():
                    return eng(h, x, edges, vel, edge_attr_orig, charges)
            return _PaddedStep.apply(self, f32g(x), send, recv, f32g(vel), f32g(edge_attr_orig), _f32(charges), *plist)
        graph = self.prepare_graph((send, recv), n_nodes)
        if not train:           # inference: no autograd node, no parameter list to marshal
            return self._step("aether_forward", self._param_struct_ref(), _f32(x), _f32(vel), _f32(charges), None,
                              _f32(edge_attr_orig), graph, E, False)[0]
        return _AetherStep.apply(self, f32g(x), f32g(vel), f32g(edge_attr_orig), _f32(charges), graph, E, *plist)

    @torch.no_grad()
    def rollout(self, x, vel, edges, charges, steps, dt=1.0):
        """``steps`` autoregressive steps on the device (``aether_rollout``): positions ``[steps, n_nodes, D]``, one
        kernel launch per step, no host-side gathers (``FrameModule._rollout``)."""
        if self.hidden_size != self._kw:
            self._require_gpu(x)
            return self._sync_engine().rollout(x, vel, edges, charges, steps, dt)
        return self._rollout(x, vel, edges, charges, steps, dt, reuse=True)

    def differentiable_rollout(self, x, vel, edges, charges, steps, dt=1.0):
        if self.hidden_size != self._kw:
            if int(steps) < 1:
                raise ValueError("differentiable_rollout: steps must be at least 1")
            self._require_gpu(x)
            raise _lib.AetherHipError("rollout training: 64-wide engine only (hidden_size must be 64; a narrower Aether runs "
                                      "on a zero-padded engine that has no rollout backward)")
        return super().differentiable_rollout(x, vel, edges, charges, steps, dt)
