"""MI355X drop-in for the reference's ``nn.state2state.dynamic_field_aether.DynamicFieldAether``
(the model experiments/lorentz/main.py:148-149 builds for ``--model dynamic_field_aether``).

Same constructor, ``forward(h, x, edges, vel, edge_attr_orig, charges, num_nodes)`` and ``state_dict`` keys
(dynamic_field_aether.py:51-100).  The field comes from ``aether_dynamic_field`` (attention-pooled graph
summary + FiLM field net, :11-48), everything after it from the same kernels as ``Aether``
(``aether_forward_field``).  With gradients enabled the step goes through ``_DynStep``: ``aether_backward_field``
(GNN gradients + dL/dfield) and ``aether_dynamic_field_backward`` (FiLM field net, modulators, attention pooling),
so the training loop of experiments/lorentz/main.py:200-260 works unchanged.  ``differentiable_rollout(..., num_nodes=N)``
trains through the device rollout (``_frame._RolloutStep``: ``aether_rollout_dynamic_field_train_forward`` /
``aether_rollout_dynamic_field_backward``).  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from ._frame import FrameModule, _GNN, _f32, _f32g, _pad_blocks, cut, engine_shapes, field_slot_shapes, place


class _AttentionalAggregation(nn.Module):
    """Parameter holder with torch_geometric's sub-module names (``gate_nn``, ``nn``)."""

    def __init__(self, gate_nn, nn_):
        super().__init__()
        self.gate_nn = gate_nn
        self.nn = nn_


class _GraphSummary(nn.Module):
    def __init__(self, input_size, hidden_size):                       # graph_pool.py:8-23
        super().__init__()
        self.summary_net = _AttentionalAggregation(
            nn.Sequential(nn.Linear(input_size, hidden_size), nn.SiLU(), nn.Linear(hidden_size, 1)),
            nn.Sequential(nn.Linear(input_size, hidden_size), nn.SiLU(), nn.Linear(hidden_size, hidden_size)))


class _FiLM(nn.Module):
    def __init__(self, x_size, z_size, hidden_size):                   # film.py:48-55
        super().__init__()
        self.modulator = nn.Sequential(nn.Linear(z_size, hidden_size), nn.SiLU(), nn.Linear(hidden_size, hidden_size),
                                       nn.SiLU(), nn.Linear(hidden_size, 2 * x_size))


class _FilmedNetwork(nn.Module):
    def __init__(self, x_size, z_size, hidden_size, out_size):         # film.py:12-24
        super().__init__()
        self.linear_1 = nn.Linear(x_size, hidden_size)
        self.linear_2 = nn.Linear(hidden_size, hidden_size)
        self.linear_3 = nn.Linear(hidden_size, out_size)
        self.film_1 = _FiLM(hidden_size, z_size, hidden_size)
        self.film_2 = _FiLM(hidden_size, z_size, hidden_size)


class _LatentFieldNetwork(nn.Module):
    def __init__(self, num_dims, hidden_size, class_embedding_dim):    # dynamic_field_aether.py:12-26
        super().__init__()
        self.summary_net = _GraphSummary(2 * num_dims, hidden_size)
        self.wrapper = _FilmedNetwork(2 * num_dims + class_embedding_dim, hidden_size, hidden_size, num_dims)
        self.class_embedding = nn.Embedding(3, class_embedding_dim)


_DynFieldParams = _lib.AetherDynFieldParams


class _DynStep(torch.autograd.Function):
    """aether_dynamic_field + aether_forward_field / their backward halves behind torch.autograd (parameters only
    get gradients: the runner detaches positions and edge attributes, experiments/lorentz/main.py:243-247)."""

    N_FIXED = 8

    @staticmethod
    def forward(ctx, module, x, vel, ea, charges, graph, n_edges, num_nodes, *params):
        out, field, ws = module._launch(x, vel, ea, charges, graph, n_edges, num_nodes, train=True)
        ctx.module, ctx.saved = module, (x, vel, charges, graph, ws, n_edges, num_nodes)
        if any(ctx.needs_input_grad[1:4]):       # x / vel / edge_attr: aether_backward_inputs recovers y = R^T (out - x)
            ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        lib = _lib.load()
        module = ctx.module
        x, vel, charges, graph, ws, n_edges, num_nodes = ctx.saved
        D, n_nodes = module.num_dims, x.shape[0]
        ps, fps = module._structs(x.device)
        ps = C.byref(ps)
        names, offsets, total = module._grad_layout()
        flat = torch.zeros(total, dtype=torch.float32, device=x.device)        # one buffer, one memset
        kshapes = module._kernel_shapes()
        # kernel-side views: a GNN tensor of a model whose hidden_size is not a kernel width has the padded shape
        kgrads = {n: flat[o:o + int(np.prod(kshapes[n]))].view(kshapes[n]) for n, o in zip(names, offsets)}
        gtensors = dict(kgrads)
        gtensors.update(module._dummy)                               # field_net.net.* slots: not written in this mode
        gs = _lib.params_struct(gtensors)
        gfs = module._dyn_struct(kgrads)
        g = grad_out.to(torch.float32).contiguous()
        grad_field = torch.empty(n_nodes, D, dtype=torch.float32, device=x.device)
        module._backward("aether_backward_field", ps, C.byref(gs), x, vel, charges, graph, ws, n_edges, g, grad_field)
        n_graphs = n_nodes // num_nodes
        need = lib.aether_dynamic_field_backward_workspace_bytes(D, n_graphs)
        dws = torch.empty(need, dtype=torch.uint8, device=x.device)
        want_in = any(ctx.needs_input_grad[1:4])
        gz = torch.empty(n_nodes, 2 * D, dtype=torch.float32, device=x.device) if want_in else None
        _lib.check(lib.aether_dynamic_field_backward_inputs(C.byref(fps), C.byref(gfs), D, n_graphs, num_nodes, x.data_ptr(),
                                                            vel.data_ptr(), charges.data_ptr(), grad_field.data_ptr(),
                                                            dws.data_ptr(), dws.numel(),
                                                            gz.data_ptr() if gz is not None else None,
                                                            torch.cuda.current_stream(x.device).cuda_stream),
                   "aether_dynamic_field_backward_inputs")
        module.last_grad_field = grad_field
        gx = gv = gea = None
        if want_in:
            # gradients w.r.t. the inputs (dynamic_field_aether.py:79-100 is differentiable in them): the GNN / frame part
            # from what aether_backward_field left in the workspace, the part through the latent field from gz
            gx, gv, gea = module._input_grads(ctx.needs_input_grad[1:4], ps, x, vel, charges, graph, ws, n_edges,
                                              ctx.saved_tensors[0], g, gz)
        if module.dp_group is not None:            # one all-reduce of the flat gradient buffer (RCCL), then the mean
            import torch.distributed as dist
            dist.all_reduce(flat, group=module.dp_group)
            flat.div_(dist.get_world_size(module.dp_group))
        need_g = ctx.needs_input_grad[_DynStep.N_FIXED:]
        grads = module._narrow_grads(kgrads)
        return (None, gx, gv, gea, None, None, None, None) + tuple(grads[n] if k else None for n, k in zip(names, need_g))


class DynamicFieldAether(FrameModule):
    """Drop-in for nn/state2state/dynamic_field_aether.py:51-100."""

    WEIGHTS_PREPARED = False     # the padded copies of the GNN parameters are refreshed every call (_padded_gnn)
    TRAIN_WS_PER_CALL = True     # (moving it to the cached training workspace changes its memory behaviour: DESIGN 4.15)
    DROP_ON_APPLY = ("_glayout", "_plist", "_struct_cache")
    DROP_ON_LOAD = ("_plist", "_struct_cache")

    def __init__(self, input_size, hidden_size, dropout_prob, num_dims, device="cuda"):
        super().__init__()
        # (the runner passes dropout 0.0, main.py:149; > 0: identity in eval(), the out MLP's two masks in train() -- as Aether)
        self._frame_init("DynamicFieldAether", 3 * num_dims, input_size, hidden_size, dropout_prob, num_dims)
        self.gnn = _GNN(input_size, hidden_size, dropout_prob, num_dims, additional_features=num_dims)
        # a model whose width is not a kernel width runs on zero-padded copies of its GNN parameters (exact: padded
        # channels stay zero), as Aether does
        self._kshapes = None
        self._padded = None
        self.field_net = _LatentFieldNetwork(num_dims, 32, 16)
        self._struct_cache = None
        self._dummy = None
        self._glayout = None
        self.to(device)
        self.params = self.__str__()

    def _structs(self, device):
        key = (str(device),) + tuple([p.data_ptr() for p in self._param_list()])
        if self._struct_cache is not None and self._struct_cache[0] == key:
            return self._struct_cache[1], self._struct_cache[2]
        ps, fps = self._build_structs(device)
        self._struct_cache = (key, ps, fps)
        return ps, fps

    def _build_structs(self, device):
        sd = dict(self.named_parameters())
        D = self.num_dims
        # the built-in field net is bypassed; its slots of AetherParams point at readable scratch of the right size
        # (the class embedding's slot is the model's own)
        dummy = {k: shape for k, shape in field_slot_shapes(D).items() if k.startswith("field_net.net.")}
        if self._dummy is None or next(iter(self._dummy.values())).device != device:
            self._dummy = {k: torch.zeros(*shape, device=device) for k, shape in dummy.items()}
        tensors = {k: v for k, v in sd.items()}
        if self.hidden_size != self._kw:
            tensors.update(self._padded_gnn(device))
        tensors.update(self._dummy)
        ps = _lib.params_struct(tensors)
        return ps, self._dyn_struct(sd)

    def _kernel_shapes(self):
        """{parameter name: shape of the tensor the kernels see} -- the GNN's at kernel width."""
        if self._kshapes is None:
            shapes = {n: tuple(p.shape) for n, p in self.named_parameters()}
            if self.hidden_size != self._kw:
                shapes.update(engine_shapes(self.num_dims, self._kw))
            self._kshapes = shapes
        return self._kshapes

    def _padded_gnn(self, device):
        """Zero-padded kernel-width copies of the GNN parameters, refreshed from the parameters (every call: an optimizer
        step may lie between two calls, and inside a captured step the copies have to be part of the graph)."""
        ks = self._kernel_shapes()
        if self._padded is None or next(iter(self._padded.values())).device != device:
            self._padded = {n: torch.zeros(ks[n], dtype=torch.float32, device=device)
                            for n, _ in self.named_parameters() if n.startswith("gnn.")}
            self._struct_cache = None
        with torch.no_grad():
            for n, p in self.named_parameters():
                if n.startswith("gnn."):
                    place(self._padded[n], p, _pad_blocks(n, p.shape, self.hidden_size, self._kw))
        return self._padded

    def _narrow_grads(self, kgrads):
        """Kernel-side gradients cut back to the parameters' shapes."""
        if self.hidden_size == self._kw:
            return kgrads
        return {n: cut(torch.empty_like(p), kgrads[n], _pad_blocks(n, p.shape, self.hidden_size, self._kw))
                if n.startswith("gnn.") else kgrads[n] for n, p in self.named_parameters()}

    _DYN_NAMES = ["summary_net.summary_net.gate_nn.0", "summary_net.summary_net.gate_nn.2", "summary_net.summary_net.nn.0",
                  "summary_net.summary_net.nn.2", "wrapper.linear_1", "wrapper.linear_2", "wrapper.linear_3",
                  "wrapper.film_1.modulator.0", "wrapper.film_1.modulator.2", "wrapper.film_1.modulator.4",
                  "wrapper.film_2.modulator.0", "wrapper.film_2.modulator.2", "wrapper.film_2.modulator.4"]

    def _grad_layout(self):
        """(parameter names, offsets into one flat gradient buffer (64-float aligned), total floats)."""
        if self._glayout is None:
            names, offsets, total = [], [], 0
            ks = self._kernel_shapes()
            for n, p in self.named_parameters():
                names.append(n)
                offsets.append(total)
                total += (int(np.prod(ks[n])) + 63) // 64 * 64
            self._glayout = (names, offsets, total)
        return self._glayout

    def _dyn_struct(self, tensors):
        """AetherDynFieldParams from {parameter name: tensor} (the parameters themselves or their gradients)."""
        ptrs = []
        for n in self._DYN_NAMES:
            ptrs += [tensors["field_net." + n + ".weight"].data_ptr(), tensors["field_net." + n + ".bias"].data_ptr()]
        ptrs.append(tensors["field_net.class_embedding.weight"].data_ptr())
        return _DynFieldParams(*ptrs)

    def _current_structs(self, device):
        if self.hidden_size != self._kw:
            self._padded_gnn(device)        # refresh the kernel-width copies of the GNN parameters
        return self._structs(device)

    def _rollout_params(self, device):
        ps, fps = self._current_structs(device)
        return C.byref(ps), C.byref(fps)

    def _launch(self, x, vel, ea, charges, graph, n_edges, num_nodes, train):
        n_nodes, D = x.shape[0], self.num_dims
        ps, fps = self._current_structs(x.device)
        field = torch.empty(n_nodes, D, dtype=torch.float32, device=x.device)
        _lib.check(_lib.load().aether_dynamic_field(C.byref(fps), D, n_nodes // int(num_nodes), int(num_nodes), x.data_ptr(),
                                                    vel.data_ptr(), charges.data_ptr(), field.data_ptr(),
                                                    torch.cuda.current_stream(x.device).cuda_stream),
                   "aether_dynamic_field")
        out, ws, _ = self._step("aether_forward_field", C.byref(ps), x, vel, charges, field, ea, graph, n_edges, train)
        self.last_field = field
        return out, field, ws

    @torch.no_grad()
    def rollout(self, x, vel, edges, charges, steps, dt=1.0, num_nodes=None):
        """``steps`` autoregressive steps on the device (``aether_rollout_dynamic_field``), the protocol of
        ``aether_amd.rollout`` (``FrameModule._rollout``); the latent field is recomputed from the current state every
        step.  -> [steps, n_nodes, D]."""
        self._require_gpu(x)
        if num_nodes is None:
            raise ValueError("num_nodes (objects per graph) is required, as in forward")
        return self._rollout(x, vel, edges, charges, steps, dt, num_nodes=num_nodes)

    # -- training through the rollout (``_RolloutStep``) -----------------------------------
    grad_as_view = False         # gradients are handed to autograd as tensors of their own (``_grad_destination``)

    def _rollout_train_params(self, device, refresh=True):
        ps, fps = self._current_structs(device) if refresh else self._structs(device)
        return C.byref(ps), C.byref(fps)

    def _grad_destination(self):
        """One fresh flat buffer per backward, as ``_DynStep``: the kernels write kernel-shaped tensors into it, a narrow
        model's GNN gradients are cut back to the parameters' shapes afterwards."""
        plist = self._param_list()
        names, offsets, total = self._grad_layout()
        flat = torch.zeros(total, dtype=torch.float32, device=plist[0].device)
        kshapes = self._kernel_shapes()
        kgrads = {n: flat[o:o + int(np.prod(kshapes[n]))].view(kshapes[n]) for n, o in zip(names, offsets)}
        gtensors = dict(kgrads)
        gtensors.update(self._dummy)                                 # field_net.net.* slots: not written in this mode
        gs, gfs = _lib.params_struct(gtensors), self._dyn_struct(kgrads)
        narrow = self.hidden_size != self._kw
        dst = [torch.empty_like(p) if narrow and n.startswith("gnn.") else kgrads[n] for n, p in zip(names, plist)]

        def finish():
            if self.dp_group is not None:          # one all-reduce of the flat gradient buffer (RCCL), then the mean
                import torch.distributed as dist
                dist.all_reduce(flat, group=self.dp_group)
                flat.div_(dist.get_world_size(self.dp_group))
            if narrow:
                for n, p, d in zip(names, plist, dst):
                    if n.startswith("gnn."):
                        cut(d, kgrads[n], _pad_blocks(n, p.shape, self.hidden_size, self._kw))
        return plist, dst, None, dst, False, (C.byref(gs), C.byref(gfs)), finish

    def differentiable_rollout(self, x, vel, edges, charges, steps, dt=1.0, num_nodes=None):
        """``rollout`` for training (``FrameModule.differentiable_rollout``) with the latent field recomputed from the
        current state every step, and differentiated with it: gradients for the GNN and the field net's parameters and,
        where they require one, ``x`` and ``vel`` (``aether_rollout_dynamic_field_train_forward`` /
        ``aether_rollout_dynamic_field_backward``).  ``num_nodes``: objects per graph, as in ``forward``."""
        if num_nodes is None:
            raise _lib.AetherHipError("DynamicFieldAether.differentiable_rollout: not built without num_nodes (the objects "
                                      "per graph cannot be inferred from the inputs: pass num_nodes, as in forward)")
        return self._rollout_grad(x, vel, edges, charges, steps, dt, num_nodes=int(num_nodes))

    def forward(self, h, x, edges, vel, edge_attr_orig, charges, num_nodes):
        """``h`` is ignored, as in the reference (dynamic_field_aether.py:79-100)."""
        send, recv, n_nodes, E = self._validate_forward(x, vel, edges, edge_attr_orig, charges, num_nodes)
        # differentiable in x / vel / edge_attr_orig, as the reference's forward (dynamic_field_aether.py:79-100)
        wants_in = torch.is_grad_enabled() and (x.requires_grad or vel.requires_grad or edge_attr_orig.requires_grad)
        f32g = _f32g if wants_in else _f32
        x, vel, ea, charges = f32g(x), f32g(vel), f32g(edge_attr_orig), _f32(charges)
        graph = self.prepare_graph((send, recv), n_nodes)
        if wants_in or (torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())):
            return _DynStep.apply(self, x, vel, ea, charges, graph, E, int(num_nodes), *self.parameters())
        with torch.no_grad():
            # (a train()-mode forward applies dropout even without autograd, as nn.Dropout does)
            drops = self.dropout_prob > 0.0 and self.training
            return self._launch(x, vel, ea, charges, graph, E, int(num_nodes), train=drops)[0]
