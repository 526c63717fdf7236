"""What the drop-ins that run on Aether's kernels share (``Aether``, ``DynamicFieldAether``, ``LoCS``): the graph cache and
parameter holders, the block helpers that place a model in its kernel-width engine, and ``FrameModule`` -- constructor
checks, input validation, workspaces, the reuse flags of the inference workspace, the dropout masks and every call into
the library (the ``_h`` entries of include/aether_hip.h, which take the width; at 64 they are the 64-wide entries).

A subclass supplies its parameter holders, its AetherParams (own tensors, padded copies or images) and its autograd
function: the parameter-gradient halves differ ("One frame for the three kernel drop-ins").
"""
from __future__ import annotations

import ctypes as C
import weakref
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from ... import _lib

_FORCED = _lib.FLAG_FORCE_FUSED | _lib.FLAG_FORCE_STREAMED


class GraphCache:
    """Receiver-sorted view of an edge index, built once per distinct edge tensor pair.

    The reference re-creates the same edge index every batch
    (experiments/lorentz/main.py:211-212); reusing the tensors (or calling
    ``Aether.prepare_graph``) makes this a dictionary lookup."""

    def __init__(self, max_entries=8):
        self.max_entries = max_entries
        self._d = OrderedDict()

    @staticmethod
    def _key(send, recv, n_nodes):
        return (send.data_ptr(), recv.data_ptr(), send.numel(), int(n_nodes), send._version,
                recv._version, send.device.index)

    def get(self, send, recv, n_nodes):
        key = self._key(send, recv, n_nodes)
        hit = self._d.get(key)
        if hit is not None:
            self._d.move_to_end(key)
            return hit[0]
        # Same index in new tensors (the runner rebuilds it every batch, main.py:211-212): one comparison kernel against
        # the view's own sorted copy + a 4-byte flag (aether_graph_matches, ~20 us) instead of sorting again (two
        # torch.equal calls cost 0.19 ms: several reductions and a blocking .item() each).
        lib = _lib.load()
        for k2, (val, s2, r2) in reversed(list(self._d.items())):
            if (k2[2], k2[3], k2[6]) == (key[2], key[3], key[6]):
                stream = torch.cuda.current_stream(send.device).cuda_stream
                same = lib.aether_graph_matches(send.data_ptr(), recv.data_ptr(), send.numel(), n_nodes, val[0].data_ptr(), stream)
                if same < 0:
                    _lib.check(same, "aether_graph_matches")
                if same == 1:
                    self._d[key] = (val, send, recv)
                    self._trim()
                    return val
        E = send.numel()
        nbytes = lib.aether_graph_bytes(E, n_nodes)
        buf = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=send.device)
        info = _lib.AetherGraphInfo()
        stream = torch.cuda.current_stream(send.device).cuda_stream
        # (the counting builder: the same view at a fraction of the sorting builder's time, so that a new topology on
        # every call is an ordinary case; aether_set_option("graph_build", 0) sends it through aether_graph_build)
        _lib.check(lib.aether_graph_build_counting(send.data_ptr(), recv.data_ptr(), E, n_nodes,
                                                   buf.data_ptr(), buf.numel(), C.byref(info), stream),
                   "aether_graph_build_counting")
        # keep the index tensors alive so the key (their addresses) stays unique
        self._d[key] = ((buf, info), send, recv)
        self._trim()
        return buf, info

    def _trim(self):
        while len(self._d) > self.max_entries:
            self._d.popitem(last=False)


class _WsToken:
    """Held by the autograd node of a training forward: while it is alive that forward's workspace is still needed."""
    __slots__ = ("__weakref__",)


def _train_workspace(module, ws_bytes, device, slot="_train_ws"):
    """The workspace of a training forward and the token its autograd node holds (None under capture).  ``slot``: the
    module attribute that caches it (a training rollout keeps its own, many times a step's).

    The backward reads this forward's intermediates: one workspace per forward that is still waiting for its backward.
    The usual loop (forward, backward, step) gets the module's cached buffer back every time -- a fresh torch.empty per
    call kept TWO of them alive across steps (this one and the previous step's, still referenced), which at the 33.5 M-edge
    shard of config 5 (~120 GB each) pushed the caching allocator into freeing and re-allocating device memory every step
    (0.44 s of a 0.55 s step).  Under hipGraph capture the buffer comes from the graph's pool as before.
    "Still waiting": the autograd node that saved the buffer is alive (a token it holds; after backward() without
    retain_graph the node and the token are gone).  The module keeps ``_train_ws`` and ``_train_ws_token`` -- and, for a
    training rollout (``slot``), ``_rollout_train_ws`` and its token: that buffer is the size of the longest rollout
    trained so far (one training workspace + what a forward keeps per further step: 0.8 GB for 4 steps, 2.0 GB for 20 at
    N=20, batch=128) and stays with the module until a larger one replaces it or the module goes."""
    tw, tok = getattr(module, slot, None), getattr(module, slot + "_token", None)
    busy = tok is not None and tok() is not None
    capturing = torch.cuda.is_current_stream_capturing()
    if tw is not None and not busy and tw.numel() >= ws_bytes and tw.device == device and not capturing:
        ws = tw
    else:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        if not capturing:
            setattr(module, slot, ws)
    token = _WsToken() if not capturing else None
    if token is not None:
        setattr(module, slot + "_token", weakref.ref(token))
    return ws, token


def _grads_alias_flat(module, plist, views):
    """Is some .grad already a view of the flat gradient buffer (a second backward without zero_grad, micro-batch
    accumulation, the module applied twice in one autograd graph)?  The backward kernels OVERWRITE their destination:
    they then write into a second buffer and the result is added, as torch.autograd would."""
    return module.grad_as_view and any(p.grad is not None and p.grad.data_ptr() == v.data_ptr()
                                       for p, v in zip(plist, views))


def _hand_over_grads(module, plist, views, dst_flat, dst_views, aliased, need, skip=()):
    """After a backward wrote its parameter gradients into ``dst_flat`` (``dst_views``): the data-parallel mean, then what
    autograd returns for the parameters.  A parameter whose .grad is unset gets the view of the flat buffer itself (like
    DDP's gradient_as_bucket_view); a .grad that already is that view is accumulated into in place (``aliased``: the
    backward wrote into the second buffer); any other existing .grad is accumulated by autograd.  ``skip``: indices of
    parameters that never get a gradient (they do not reach the output): None, .grad left as it is.  ``dst_flat`` None:
    ``dst_views`` are this call's own tensors, finished by the module (mean included) -- handed to autograd as they are."""
    if module.dp_group is not None and dst_flat is not None:      # one fused all-reduce of the flat buffer (RCCL)
        import torch.distributed as dist
        dist.all_reduce(dst_flat, group=module.dp_group)
        dst_flat.div_(dist.get_world_size(module.dp_group))
    out = []
    for i, (p, v, dv, n) in enumerate(zip(plist, views, dst_views, need)):
        if not n or i in skip:
            out.append(None)
        elif module.grad_as_view and p.grad is None and not aliased:
            p.grad = v
            out.append(None)
        elif module.grad_as_view and p.grad is not None and p.grad.data_ptr() == v.data_ptr():
            v.add_(dv)
            out.append(None)
        else:
            out.append(dv if dst_flat is None else dv.clone())
    return out


def network_size(module):
    """``__str__`` of every drop-in, as the reference's: prints and returns the number of trainable parameters."""
    params = sum(int(np.prod(p.size())) for p in module.parameters() if p.requires_grad)
    print("Network Size", params)
    return str(params)


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def _f32g(t):
    """As ``_f32``, but an input that requires a gradient stays attached."""
    return t.to(torch.float32).contiguous() if t.requires_grad else _f32(t)


class _RolloutStep(torch.autograd.Function):
    """aether_rollout_train_forward / aether_rollout_backward (for a model with a latent field, ``num_nodes`` not None:
    aether_rollout_dynamic_field_train_forward / aether_rollout_dynamic_field_backward) behind torch.autograd: the whole
    k-step rollout is ONE autograd node (parameters, and x / vel where they require a gradient)."""

    N_FIXED = 9          # module, x, vel, charges, graph, n_edges, steps, dt, num_nodes precede the parameters

    @staticmethod
    def forward(ctx, module, x, vel, charges, graph, n_edges, steps, dt, num_nodes, *params):
        ps = module._rollout_train_params(x.device)
        traj, ws, token = module._rollout_train_forward(ps, x, vel, charges, graph, n_edges, steps, dt, num_nodes)
        ctx.module = module
        ctx.saved = (x, vel, charges, graph, ws, n_edges, steps, dt, num_nodes, token)
        ctx.consumed = False
        ctx.save_for_backward(traj)
        return traj

    @staticmethod
    def backward(ctx, grad_traj):
        module = ctx.module
        if ctx.consumed:        # (aether_rollout_backward: a step's temporaries land on the later steps' kept intermediates)
            raise RuntimeError("trying to backward through a differentiable_rollout a second time: the first backward "
                               "consumed its workspace (call differentiable_rollout again)")
        ctx.consumed = True
        x, vel, charges, graph, ws, n_edges, steps, dt, num_nodes, _token = ctx.saved
        traj, = ctx.saved_tensors
        plist, views, dst_flat, dst_views, aliased, gs, finish = module._grad_destination()
        g = grad_traj.to(torch.float32).contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        gv = torch.empty_like(vel) if ctx.needs_input_grad[2] else None
        ps = module._rollout_train_params(x.device, refresh=False)
        module._rollout_train_backward(ps, gs, x, vel, charges, graph, ws, n_edges, traj, g, gx, gv, steps, dt, num_nodes)
        if finish is not None:
            finish()
        out = _hand_over_grads(module, plist, views, dst_flat, dst_views, aliased, ctx.needs_input_grad[_RolloutStep.N_FIXED:])
        return (None, gx, gv, None, None, None, None, None, None) + tuple(out)


# -- a model inside its kernel-width engine --------------------------------------------------------------------------
def _kernel_width(hidden_size):
    """Width the kernels compute a model of this hidden_size at: 64 (fused / streamed kernels) up to 64, the next multiple
    of 64 above (csrc/wide.h)."""
    return 64 if hidden_size <= 64 else -(-hidden_size // 64) * 64


def _pad_blocks(name, shape, H, kw=64):
    """Where a parameter of a model with hidden_size H lives inside the same-named parameter of the kw-wide model the
    kernels are built for (kw = 64, or the next multiple of 64 above H): a list of (source slices, destination slices).
    Hidden vectors sit at the start of their kw-wide (update MLP: 2 kw-wide) counterparts; the first message layer of
    layers 2-4 reads [x_send | x_recv | e], three H-wide column blocks that go to the starts of the three kw-wide blocks.
    Everything else in the wide parameters stays zero, which makes the padded channels exactly zero through SiLU, the mean
    and the residuals: the wide model computes the narrow one."""
    full = tuple(slice(0, n) for n in shape)
    if name.startswith("field_net."):
        return [(full, full)]
    if name.endswith("message_fn.0.weight") and not name.startswith("gnn.layer_1."):
        return [((slice(0, H), slice(b * H, (b + 1) * H)), (slice(0, H), slice(kw * b, kw * b + H))) for b in range(3)]
    return [(full, full)]                  # top / top-left aligned


def place(image, tensor, blocks):
    """Copy a model's tensor into its engine-shaped image by a block list; the rest of the image is left as it is (zero)."""
    for ss, ds in blocks:
        image[ds].copy_(tensor[ss])
    return image


def cut(tensor, image, blocks):
    """The inverse of ``place``: an engine-shaped tensor (a gradient) cut back into a model-shaped one."""
    for ss, ds in blocks:
        tensor[ss].copy_(image[ds])
    return tensor


class _GNNLayer(nn.Module):
    """Parameter holder, locs.py:197-225."""

    def __init__(self, input_size, hidden_size, only_edge_attr=False, num_edge_features=0):
        super().__init__()
        self.only_edge_attr = only_edge_attr
        num_edge_features = num_edge_features if only_edge_attr else 3 * hidden_size
        self.message_fn = nn.Sequential(
            nn.Linear(num_edge_features, hidden_size), nn.SiLU(),
            nn.Linear(hidden_size, hidden_size), nn.SiLU())
        self.res = nn.Linear(input_size, hidden_size) if input_size != hidden_size else nn.Identity()
        self.update_fn = nn.Sequential(
            nn.Linear(hidden_size, 2 * hidden_size), nn.SiLU(),
            nn.Linear(2 * hidden_size, hidden_size))


class _GNN(nn.Module):
    """Parameter holder, locs.py:142-181 (construction order kept so that the default
    initialisation under a given torch seed equals the reference's)."""

    def __init__(self, input_size, hidden_size, dropout_prob, num_dims, additional_features=0):
        super().__init__()
        out_size = input_size // 2
        num_orientations = num_dims * (num_dims - 1) // 2
        num_relative_features = input_size + num_dims + num_orientations
        self.out_mlp = nn.Sequential(
            nn.Linear(hidden_size, hidden_size), nn.SiLU(), nn.Dropout(p=dropout_prob),
            nn.Linear(hidden_size, hidden_size), nn.SiLU(), nn.Dropout(p=dropout_prob),
            nn.Linear(hidden_size, out_size))
        self.layer_1 = _GNNLayer(
            input_size + additional_features, hidden_size, only_edge_attr=True,
            num_edge_features=num_relative_features + input_size + 2 + 2 * additional_features)
        self.layer_2 = _GNNLayer(hidden_size, hidden_size)
        self.layer_3 = _GNNLayer(hidden_size, hidden_size)
        self.layer_4 = _GNNLayer(hidden_size, hidden_size)


def engine_shapes(num_dims, kw):
    """{"gnn.<name>": shape} of the GNN the kernels are built for at width kw: Aether's (force features in layer_1)."""
    with torch.device("meta"):
        wide = _GNN(2 * num_dims, kw, 0.0, num_dims, additional_features=num_dims)
    return {"gnn." + n: tuple(p.shape) for n, p in wide.named_parameters()}


def field_slot_shapes(D):
    """Shapes of the built-in field net's slots of AetherParams, for the models that fill them with zeros."""
    return {"field_net.net.0.weight": (32, 2 * D + 16), "field_net.net.0.bias": (32,),
            "field_net.net.2.weight": (32, 32), "field_net.net.2.bias": (32,),
            "field_net.net.4.weight": (D, 32), "field_net.net.4.bias": (D,),
            "field_net.class_embedding.weight": (3, 16)}


# -- the inference workspace --------------------------------------------------------------------------------------------
def reuse_flags(last, kw, n_groups, n_edges, flags, key, weights):
    """What an inference call may skip, as flag bits, from plain values -> (bits, (ws_key, wimg_key) to keep once the
    call has succeeded).

    ``last``: the pair the last completed inference call left.  ``key``: (workspace address, n_nodes, n_edges, D, keep,
    graph address) of this call.  ``weights``: the parameters' (versions, addresses), or None for a model whose
    AetherParams are copies it refreshes every call (DynamicFieldAether: never WEIGHTS_PREPARED).

    Only the 64-wide fused kernel has hand-off words and split weight images in the workspace: the wide path
    (aether_forward_h above 64) reads neither flag, the streamed kernels neither.  Same buffer, same layout, same graph
    as the last completed call: the fused kernel left its hand-off words re-armed (WORKSPACE_REUSED); the parameters
    unchanged as well: the weight images are still current (WEIGHTS_PREPARED).  ``keep`` belongs to the key because a
    model with FLAG_KEEP_INTERMEDIATES set runs its inference in the training layout."""
    fused = kw == 64 and n_groups > 0 and n_edges > 0 and not (flags & _lib.FLAG_FORCE_STREAMED)
    if not fused:
        return 0, (None, None)
    bits = _lib.FLAG_WORKSPACE_REUSED if last[0] == key else 0
    wkey = None if weights is None else (key, weights)
    if wkey is not None and last[1] == wkey:
        bits |= _lib.FLAG_WEIGHTS_PREPARED
    return bits, (key, wkey)


class FrameModule(nn.Module):
    """Base of ``Aether``, ``DynamicFieldAether`` and ``LoCS``."""

    # at a width above 64 a forward drops these bits (the wide path has one kernel sequence)
    WIDE_FORWARD_STRIP = _FORCED
    EVAL_KEEP = False            # does an inference call honour FLAG_KEEP_INTERMEDIATES in ``flags``? (Aether: debug_fetch)
    WEIGHTS_PREPARED = True      # may an inference call reuse the weight images of the last one?
    # False: training forwards share one cached workspace (_train_workspace).  True: a fresh one per call, freed with its
    # autograd node; the module keeps no reference to it.
    TRAIN_WS_PER_CALL = False
    DROP_ON_APPLY = ()           # caches that go when parameter storage may move (.to / .cuda / .float)
    DROP_ON_LOAD = ()            # caches that go with load_state_dict

    __str__ = network_size

    def _frame_init(self, name, no_res_width, input_size, hidden_size, dropout_prob, num_dims):
        """Start of a subclass constructor: the argument checks and everything that is not a parameter holder.
        ``no_res_width``: the hidden_size at which the reference builds layer_1 without its res Linear."""
        if not (1 <= hidden_size <= 4096):
            raise ValueError("hidden_size must lie in [1, 4096] (experiments/lorentz/main.py:42-43)")
        if num_dims not in (2, 3) or input_size != 2 * num_dims:
            raise ValueError("num_dims must be 2 or 3 and input_size == 2*num_dims")
        if hidden_size == no_res_width:
            raise ValueError(f"hidden_size == {no_res_width // num_dims} * num_dims is not supported (the reference then "
                             "builds layer_1 without its res Linear, locs.py:214-218)")
        if not (0.0 <= float(dropout_prob) < 1.0):
            raise ValueError("dropout_prob must lie in [0, 1)")
        # nn.Dropout sits between the layers of out_mlp (locs.py:160-168).  In eval() it is the identity, which is what
        # the kernels compute for any p; a train()-mode forward with p > 0 applies the two scale masks (_dropout: drawn
        # with bernoulli_, same distribution as nn.Dropout, not its random stream).  rollout() is an inference path:
        # it raises in train() mode with p > 0 instead of silently skipping the masks.
        self.dropout_prob = float(dropout_prob)
        self.num_dims = num_dims
        self.hidden_size = hidden_size
        # width the kernels run this model at: 64 (fused / streamed), or the next multiple of 64 above (csrc/wide.h)
        self._kw = _kernel_width(hidden_size)
        self._name = name
        self._graphs = GraphCache()
        self.flags = 0                    # _lib.FLAG_* bits passed to the forward
        self.dp_group = None              # set by aether_amd.parallel.attach_data_parallel
        self._plist = None
        self._ws = None
        self._ws_bytes = {}
        self._last_ws = None
        self._last_ws_keep = False        # was _last_ws written in the keep (training) layout? (debug_fetch)
        self._wimg_key = None             # (_ws_key, parameter versions) whose split weight images the workspace holds
        self._ws_key = None               # (workspace, shape, graph) of the last completed inference call
        self._rollout_train_ws, self._rollout_train_ws_token = None, None     # differentiable_rollout (_train_workspace)

    # -- caches ------------------------------------------------------------------------
    def _drop(self, names):
        for n in names:
            setattr(self, n, None)

    def _apply(self, fn, *a, **k):
        self._drop(self.DROP_ON_APPLY)
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._drop(self.DROP_ON_LOAD)
        return super().load_state_dict(*a, **k)

    def _param_list(self):
        if self._plist is None:           # nn.Module.parameters() walks the module tree (0.15 ms per call): keep the list
            self._plist = [p for _, p in self.named_parameters()]
        return self._plist

    def prepare_graph(self, edges, n_nodes):
        """Build (or fetch) the receiver-sorted view for ``edges = [send, recv]``."""
        send, recv = edges
        return self._graphs.get(send.contiguous(), recv.contiguous(), n_nodes)

    # -- input validation ------------------------------------------------------------------
    def _require_gpu(self, x):
        if not x.is_cuda:
            raise _lib.AetherHipError(f"aether_amd.{self._name} runs on an MI355X only; got a CPU tensor "
                                      "(there is no CPU fallback)")

    def _check_state(self, x, vel, edges, num_nodes):
        """What ``forward`` and ``rollout`` check alike -> (send, recv, n_nodes, n_edges, x / vel / num_nodes fit, the row
        count in words).  ``num_nodes``: objects per graph, for a model that pools over graphs (None: no such model)."""
        self._require_gpu(x)
        send, recv = edges
        if send.dtype != torch.int64 or recv.dtype != torch.int64:
            raise TypeError("edges must be int64 (torch.LongTensor), as in the reference")
        n_nodes, D = x.shape
        ok = D == self.num_dims and vel.shape == x.shape and (num_nodes is None or n_nodes % int(num_nodes) == 0)
        return send, recv, n_nodes, send.numel(), ok, "n_nodes" if num_nodes is None else "B * num_nodes"

    def _validate_forward(self, x, vel, edges, edge_attr, charges=None, num_nodes=None):
        """-> (send, recv, n_nodes, n_edges).  ``charges`` None: the model takes none (LoCS)."""
        send, recv, n_nodes, E, ok, rows = self._check_state(x, vel, edges, num_nodes)
        if not ok:
            raise ValueError(f"x/vel must be [{rows}, {self.num_dims if num_nodes is None else 'num_dims'}]")
        if charges is None:
            if recv.numel() != E or edge_attr.shape != (E, 2):
                raise ValueError("edge index / edge_attr shapes do not match")
        elif recv.numel() != E or edge_attr.shape != (E, 2) or charges.numel() != n_nodes:
            raise ValueError("edge index / edge_attr / charges shapes do not match")
        return send, recv, n_nodes, E

    def _validate_rollout(self, x, vel, edges, charges, num_nodes=None):
        """-> (send, recv, n_nodes, n_edges)."""
        send, recv, n_nodes, E, ok, rows = self._check_state(x, vel, edges, num_nodes)
        if not ok or charges.numel() != n_nodes:
            raise ValueError(f"x/vel must be [{rows}, {self.num_dims if num_nodes is None else 'num_dims'}], "
                             f"charges [{rows}, 1]")
        return send, recv, n_nodes, E

    # -- workspaces ------------------------------------------------------------------------
    def _workspace_bytes(self, n_nodes, n_edges, keep):
        lib = _lib.load()
        if keep:         # the training layout depends on a library option (outer_defer_max_edges): always ask
            return lib.aether_workspace_bytes_h(n_nodes, n_edges, self.num_dims, self._kw, 1)
        key = (n_nodes, n_edges)
        nbytes = self._ws_bytes.get(key)
        if nbytes is None:
            nbytes = lib.aether_workspace_bytes_h(n_nodes, n_edges, self.num_dims, self._kw, 0)
            if len(self._ws_bytes) > 64:
                self._ws_bytes.clear()
            self._ws_bytes[key] = nbytes
        return nbytes

    def _workspace(self, nbytes, device):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self._ws

    def _training_workspace(self, nbytes, device):
        if self.TRAIN_WS_PER_CALL:
            return torch.empty(nbytes, dtype=torch.uint8, device=device), None
        return _train_workspace(self, nbytes, device)

    def _may_reuse_weight_images(self):
        """Eagerly, the version check of ``reuse_flags`` is exact.  While a hipGraph is being captured the decision is
        baked into the graph, so the conversion kernel is only left out in eval mode -- a captured INFERENCE graph, which
        has to be re-captured when the weights change (as any graph whose kernels read prepared data)."""
        return not (self.training and torch.cuda.is_current_stream_capturing())

    def _reuse(self, flags, ws, n_nodes, n_edges, graph, ginfo):
        """``reuse_flags`` for this call.  Both keys are cleared here; the caller sets the returned pair once the library
        call has succeeded."""
        weights = None
        if self.WEIGHTS_PREPARED:         # in-place updates bump a parameter's version, re-assignment its address
            plist = self._param_list()
            weights = (tuple(p._version for p in plist), tuple(p.data_ptr() for p in plist))
        key = (ws.data_ptr(), n_nodes, n_edges, self.num_dims, bool(flags & _lib.FLAG_KEEP_INTERMEDIATES), graph.data_ptr())
        bits, pending = reuse_flags((self._ws_key, self._wimg_key), self._kw, ginfo.n_groups, n_edges, flags, key, weights)
        if bits & _lib.FLAG_WEIGHTS_PREPARED and not self._may_reuse_weight_images():
            bits &= ~_lib.FLAG_WEIGHTS_PREPARED
        self._ws_key = self._wimg_key = None
        return flags | bits, pending

    def _dropout(self, ws, n_nodes, n_edges):
        """nn.Dropout after the two SiLUs of the out MLP (locs.py:163,166): scale masks drawn by torch, written straight
        into their place in the training workspace (same distribution as nn.Dropout, not its random stream)."""
        kw = self._kw
        off = _lib.load().aether_dropout_mask_offset_h(n_nodes, n_edges, self.num_dims, kw)
        masks = ws[off:off + 2 * n_nodes * kw * 4].view(torch.float32).view(2, n_nodes, kw)
        given = self.__dict__.get("_dropout_masks")          # tests: explicit masks [2, n_nodes, width]
        if given is not None and given.shape[-1] != kw:      # a narrow model's masks: padded channels are zero anyway
            given = torch.nn.functional.pad(given, (0, kw - given.shape[-1]), value=1.0)
        if given is not None:
            masks.copy_(given.to(device=ws.device, dtype=torch.float32))
        else:
            keep_p = 1.0 - self.dropout_prob
            masks.bernoulli_(keep_p).mul_(1.0 / keep_p)

    # -- the library ---------------------------------------------------------------------
    # ``ps`` / ``gs``: C.byref of an AetherParams; ``graph``: the (buffer, info) pair of prepare_graph.
    def _step(self, label, ps, x, vel, charges, field, edge_attr, graph, n_edges, train):
        """One forward step -> (out, workspace, token of a training workspace or None).  ``train``: the training layout
        (what the backward reads, not the last layer's messages, which only debug_fetch reads) and, in train() mode with
        p > 0, the dropout masks.  ``field``: None for the built-in field net (``aether_forward``), else [n_nodes, D]
        (``aether_forward_field``)."""
        gbuf, ginfo = graph
        n_nodes = x.shape[0]
        if train:
            flags = self.flags | _lib.FLAG_KEEP_INTERMEDIATES
            if not (self.flags & _lib.FLAG_KEEP_INTERMEDIATES):
                flags |= _lib.FLAG_BACKWARD_ONLY
        else:
            flags = self.flags if self.EVAL_KEEP else self.flags & ~_lib.FLAG_KEEP_INTERMEDIATES
        nbytes = self._workspace_bytes(n_nodes, n_edges, bool(flags & _lib.FLAG_KEEP_INTERMEDIATES))
        token = None
        pending = (None, None)
        if train:
            ws, token = self._training_workspace(nbytes, x.device)
            # An optimizer step follows a training forward, and not every optimizer bumps the parameters' version
            # counters (torch's fused AdamW does not): the inference workspace's weight images are stale from here on.
            self._ws_key = self._wimg_key = None
            if self.dropout_prob > 0.0 and self.training:
                self._dropout(ws, n_nodes, n_edges)
                flags |= _lib.FLAG_DROPOUT
        else:
            ws = self._workspace(nbytes, x.device)
            flags, pending = self._reuse(flags, ws, n_nodes, n_edges, gbuf, ginfo)
        if self._kw != 64:
            flags &= ~self.WIDE_FORWARD_STRIP
        out = torch.empty_like(x)
        st = _lib.load().aether_forward_h(ps, self.num_dims, self._kw, n_nodes, n_edges, x.data_ptr(), vel.data_ptr(),
                                          charges.data_ptr(), None if field is None else field.data_ptr(),
                                          edge_attr.data_ptr(), gbuf.data_ptr(), C.byref(ginfo), ws.data_ptr(), ws.numel(),
                                          out.data_ptr(), flags, torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, label)
        self._ws_key, self._wimg_key = pending
        self._last_ws = None if train and self.TRAIN_WS_PER_CALL else ws          # (debug_fetch reads it)
        self._last_ws_keep = bool(flags & _lib.FLAG_KEEP_INTERMEDIATES)
        return out, ws, token

    def _backward(self, label, ps, gs, x, vel, charges, graph, ws, n_edges, grad_out, grad_field=None):
        """Parameter gradients into ``gs`` (overwritten).  ``grad_field``: None (``aether_backward``: the built-in field
        net's gradients too), else the [n_nodes, D] destination of dL/dfield (``aether_backward_field``)."""
        gbuf, ginfo = graph
        st = _lib.load().aether_backward_h(ps, gs, self.num_dims, self._kw, x.shape[0], n_edges, x.data_ptr(), vel.data_ptr(),
                                           charges.data_ptr(), gbuf.data_ptr(), C.byref(ginfo), ws.data_ptr(), ws.numel(),
                                           grad_out.data_ptr(), None if grad_field is None else grad_field.data_ptr(),
                                           torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, label)

    def _input_grads(self, need, ps, x, vel, charges, graph, ws, n_edges, out, grad_out, field_input_grad=None):
        """Gradients w.r.t. x / vel / edge_attr (``need``: which of the three are wanted) from what the backward left in
        the workspace -> (gx, gv, gea).  ``field_input_grad``: None for the built-in field net, else d(loss)/d[x | vel]
        through an external field, [n_nodes, 2D]."""
        gbuf, ginfo = graph
        gx, gv = torch.empty_like(x), torch.empty_like(x)
        gea = torch.empty(n_edges, 2, dtype=torch.float32, device=x.device) if need[2] else None
        st = _lib.load().aether_backward_inputs_h(ps, self.num_dims, self._kw, x.shape[0], n_edges, x.data_ptr(),
                                                  vel.data_ptr(), charges.data_ptr(), gbuf.data_ptr(), C.byref(ginfo),
                                                  ws.data_ptr(), ws.numel(), out.data_ptr(), grad_out.data_ptr(),
                                                  gx.data_ptr(), gv.data_ptr(), None if gea is None else gea.data_ptr(),
                                                  None if field_input_grad is None else field_input_grad.data_ptr(),
                                                  torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, "aether_backward_inputs")
        return gx if need[0] else None, gv if need[1] else None, gea

    def _rollout_params(self, device):
        """(byref of the AetherParams, byref of the AetherDynFieldParams or None) a rollout runs on, brought up to date."""
        raise NotImplementedError

    @torch.no_grad()
    def _rollout(self, x, vel, edges, charges, steps, dt, num_nodes=None, reuse=False):
        """``steps`` autoregressive steps on the device -> positions [steps, n_nodes, D]: x_{t+1} = self(x_t, v_t),
        v_{t+1} = (x_{t+1} - x_t) / dt, ``edge_attr = [q_i q_j, |x_i - x_j|]`` rebuilt inside the kernels every step
        (experiments/lorentz/main.py:243-246).  ``reuse``: the inference workspace's reuse flags, and its keys set
        afterwards; otherwise the rollout leaves them unset (the workspace's hand-off words are in the rollout's state)."""
        send, recv, n_nodes, E = self._validate_rollout(x, vel, edges, charges, num_nodes)
        if self.dropout_prob > 0.0 and self.training:
            raise RuntimeError(f"{self._name}.rollout is an inference path (no dropout masks): call .eval() first")
        x, vel, charges = _f32(x), _f32(vel), _f32(charges)
        gbuf, ginfo = self.prepare_graph((send, recv), n_nodes)
        ps, dyn = self._rollout_params(x.device)
        ws = self._workspace(self._workspace_bytes(n_nodes, E, False), x.device)
        flags = self.flags & ~_lib.FLAG_KEEP_INTERMEDIATES
        # the wide rollout reads two bits, to reject them: KEEP_INTERMEDIATES (cleared above) and FORCE_FUSED
        if self._kw != 64:
            flags &= ~_FORCED
        pending = (None, None)
        if reuse:
            flags, pending = self._reuse(flags, ws, n_nodes, E, gbuf, ginfo)
        else:
            self._ws_key = self._wimg_key = None
        D, steps = self.num_dims, int(steps)
        traj = torch.empty(steps, n_nodes, D, dtype=torch.float32, device=x.device)
        if steps <= 0:
            return traj
        lib = _lib.load()
        stream = torch.cuda.current_stream(x.device).cuda_stream
        if dyn is None:
            st = lib.aether_rollout_h(ps, D, self._kw, n_nodes, E, x.data_ptr(), vel.data_ptr(), charges.data_ptr(),
                                      gbuf.data_ptr(), C.byref(ginfo), ws.data_ptr(), ws.numel(), traj.data_ptr(), steps,
                                      float(dt), flags, stream)
            _lib.check(st, "aether_rollout")
        else:                             # the latent field recomputed from the current state every step
            field = torch.empty(n_nodes, D, dtype=torch.float32, device=x.device)
            st = lib.aether_rollout_dynamic_field_h(ps, dyn, D, self._kw, n_nodes, E, int(num_nodes), x.data_ptr(),
                                                    vel.data_ptr(), charges.data_ptr(), gbuf.data_ptr(), C.byref(ginfo),
                                                    ws.data_ptr(), ws.numel(), field.data_ptr(), traj.data_ptr(), steps,
                                                    float(dt), flags, stream)
            _lib.check(st, "aether_rollout_dynamic_field")
        self._ws_key, self._wimg_key = pending
        self._last_ws, self._last_ws_keep = ws, False
        return traj

    # -- training through the rollout ------------------------------------------------------
    def _rollout_train_params(self, device, refresh=True):
        """byref of the AetherParams a training rollout runs on -- for a model with a latent field the pair (that, byref of
        its AetherDynFieldParams); ``refresh``: bring copies of the parameters up to date first (the forward does, the
        backward reads what the forward read)."""
        raise NotImplementedError

    def _grad_destination(self):
        """Where a backward writes the parameter gradients -> (parameters, views of the flat gradient buffer, destination
        flat buffer and its views, is that the second buffer, byref of the destinations' AetherParams (with a latent field:
        the pair of ``_rollout_train_params``), a callable that finishes them (engine-shaped scratch cut to the model's
        shapes) or None)."""
        raise NotImplementedError

    def _rollout_train_forward(self, ps, x, vel, charges, graph, n_edges, steps, dt, num_nodes=None):
        """``aether_rollout_train_forward`` (``num_nodes`` None) or ``aether_rollout_dynamic_field_train_forward``
        -> (trajectory [steps, n_nodes, D], workspace, its token)."""
        gbuf, ginfo = graph
        n_nodes, D = x.shape
        lib = _lib.load()
        if num_nodes is None:
            nbytes = lib.aether_rollout_train_workspace_bytes(n_nodes, n_edges, D, self._kw, steps)
        else:
            nbytes = lib.aether_rollout_dynamic_field_train_workspace_bytes(n_nodes, n_edges, D, self._kw, num_nodes, steps)
        ws, token = _train_workspace(self, max(nbytes, 256), x.device, slot="_rollout_train_ws")
        # an optimizer step follows: the inference workspace's weight images are stale from here on (``_step``)
        self._ws_key = self._wimg_key = None
        traj = torch.empty(steps, n_nodes, D, dtype=torch.float32, device=x.device)
        tail = (x.data_ptr(), vel.data_ptr(), charges.data_ptr(), gbuf.data_ptr(), C.byref(ginfo), ws.data_ptr(), ws.numel(),
                traj.data_ptr(), steps, dt, self.flags & _FORCED, torch.cuda.current_stream(x.device).cuda_stream)
        if num_nodes is None:
            _lib.check(lib.aether_rollout_train_forward(ps, D, self._kw, n_nodes, n_edges, *tail), "aether_rollout_train_forward")
        else:
            _lib.check(lib.aether_rollout_dynamic_field_train_forward(*ps, D, self._kw, n_nodes, n_edges, num_nodes, *tail),
                       "aether_rollout_dynamic_field_train_forward")
        return traj, ws, token

    def _rollout_train_backward(self, ps, gs, x, vel, charges, graph, ws, n_edges, traj, grad_traj, gx, gv, steps, dt,
                                num_nodes=None):
        """``aether_rollout_backward`` (``num_nodes`` None) or ``aether_rollout_dynamic_field_backward`` into ``gs`` (the
        model's ``_grad_destination``) and ``gx`` / ``gv`` (None: not wanted).  Consumes ``ws``."""
        gbuf, ginfo = graph
        lib = _lib.load()
        tail = (x.data_ptr(), vel.data_ptr(), charges.data_ptr(), gbuf.data_ptr(), C.byref(ginfo), ws.data_ptr(), ws.numel(),
                traj.data_ptr(), grad_traj.data_ptr(), None if gx is None else gx.data_ptr(),
                None if gv is None else gv.data_ptr(), steps, dt, torch.cuda.current_stream(x.device).cuda_stream)
        if num_nodes is None:
            _lib.check(lib.aether_rollout_backward(ps, gs, self.num_dims, self._kw, x.shape[0], n_edges, *tail),
                       "aether_rollout_backward")
        else:
            _lib.check(lib.aether_rollout_dynamic_field_backward(*ps, *gs, self.num_dims, self._kw, x.shape[0], n_edges,
                                                                 num_nodes, *tail), "aether_rollout_dynamic_field_backward")

    def _rollout_grad(self, x, vel, edges, charges, steps, dt, num_nodes=None):
        """The rollout of ``_rollout`` attached to autograd (``_RolloutStep``): gradients for the parameters that require
        one and, where they require one, ``x`` and ``vel``."""
        steps = int(steps)
        if steps < 1:
            raise ValueError("differentiable_rollout: steps must be at least 1")
        send, recv, n_nodes, E = self._validate_rollout(x, vel, edges, charges, num_nodes)
        if self.dropout_prob > 0.0 and self.training:
            raise RuntimeError(f"{self._name}.differentiable_rollout draws no dropout masks (one pair per step would be "
                               "needed): call .eval() first or build the model with dropout_prob = 0")
        if self._kw != 64:
            raise _lib.AetherHipError("rollout training: 64-wide engine only")
        graph = self.prepare_graph((send, recv), n_nodes)
        return _RolloutStep.apply(self, _f32g(x), _f32g(vel), _f32(charges), graph, E, steps, float(dt),
                                  None if num_nodes is None else int(num_nodes), *self._param_list())

    def differentiable_rollout(self, x, vel, edges, charges, steps, dt=1.0):
        """``rollout`` for training: positions ``[steps, n_nodes, D]`` of the same protocol, attached to autograd for the
        parameters and, where they require a gradient, ``x`` and ``vel`` -- a k-step loss on it trains through all steps
        (``aether_rollout_train_forward`` / ``aether_rollout_backward``: the steps, the chain between them and the sum of
        the parameter gradients over the steps all run on the device).  Works in train() and eval(); in train() with
        dropout_prob > 0 it raises, as ``rollout`` does."""
        return self._rollout_grad(x, vel, edges, charges, steps, dt)

    # -- test hooks -------------------------------------------------------------------
    PER_LAYER = tuple(f"x{k}" for k in range(1, 5)) + tuple(f"e{k}" for k in range(1, 5)) + ("efeat",)

    def _fetchable(self, name):
        """Does the layout ``_last_ws`` was written with hold ``name`` where aether_debug_fetch_h looks for it?  The library
        computes per-layer offsets from the training layout, whatever the workspace's.  At width 64 (WsLayout) the node
        states and messages lie in the forward prefix both layouts share; the layer-1 features follow it and exist in the
        training layout only.  Above 64 (WideLayout) the features and node states precede the first region whose size
        depends on the layout; the messages follow it, and an inference workspace lets the layers share two of them.
        This table restates ``WsLayout`` (csrc/aether_hip.hip) and ``WideLayout`` (csrc/wide_impl.inc) because the check has
        to come before any library call; tests/test_gpu_buffer_contract.py holds it to them from outside: every tensor it
        lets through after an inference-layout call is fetched and compared with the oracle.
        Whether a tensor was WRITTEN is another matter and not decided here: a training forward without
        FLAG_KEEP_INTERMEDIATES in ``flags`` runs with FLAG_BACKWARD_ONLY and leaves e4 unwritten in a keep-layout
        workspace, and the fused inference kernel need not write its messages to memory at all."""
        if name not in self.PER_LAYER or self._last_ws_keep:
            return True
        if self._kw == 64:
            return name != "efeat"
        return name[0] == "x" or name == "efeat"

    def debug_fetch(self, name, n_nodes, n_edges, cols):
        if self._last_ws is None:
            raise ValueError("debug_fetch: no forward has left a workspace on this module")
        if not self._fetchable(name):
            raise ValueError(f"debug_fetch({name!r}): the last call wrote its workspace in the inference layout, which does "
                             "not hold this tensor where the training layout does; set FLAG_KEEP_INTERMEDIATES in "
                             "``flags`` (or run a training forward) first")
        dev = next(self.parameters()).device
        rows = n_edges if name.startswith("e") else n_nodes
        dst = torch.empty(rows, cols, dtype=torch.float32, device=dev)
        n = _lib.load().aether_debug_fetch_h(name.encode(), self.num_dims, self._kw, n_nodes, n_edges,
                                             self._last_ws.data_ptr(), dst.data_ptr(),
                                             torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(n, "aether_debug_fetch")
        assert n == rows * cols, (n, rows, cols)
        return dst

    def graph_perm(self, edges, n_nodes):
        g, _ = self.prepare_graph(edges, n_nodes)
        E = edges[0].numel()
        perm = torch.empty(E, dtype=torch.int32, device=edges[0].device)
        _lib.check(_lib.load().aether_graph_perm(g.data_ptr(), E, n_nodes, perm.data_ptr(),
                                                 torch.cuda.current_stream(perm.device).cuda_stream),
                   "aether_graph_perm")
        return perm.long()
