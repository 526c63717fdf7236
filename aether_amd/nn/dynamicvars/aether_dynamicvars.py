"""MI355X prediction path of the reference's variable-N model:
``nn.dynamicvars.aether_dynamicvars.AetherDynamicVars`` (aether_dynamicvars.py:15-273) -- ``predict_field``,
``single_step_forward`` and ``predict_future``, the path experiments/ind runs for its forecasting metrics.

Sub-modules carry the reference's names (``encoder``, ``decoder``, ``field_net``, ``coordinate_embedding``,
``angular_embedding``) and are created in its order, so a seeded construction or ``load_state_dict`` of a reference
checkpoint gives the same weights.  ``calculate_loss(is_train=False)`` -- the runner's validation NLL / KL -- is two
library calls (``_loss.SceneLossMixin``: the sequence encoder over all frames, the teacher-forced decoding loop); training
(``is_train=True``) is not part of this path.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from ... import _lib
from ..seq2seq.encoder import gumbel_softmax_hard
from ..seq2seq.field import _CoordinateEmbedding
from ._loss import SceneLossMixin
from ._rollout import SceneRolloutMixin
from ._scene import ScenePack, _DynStepConfig, cached_workspace, pack_scenes      # noqa: F401  (ScenePack, pack_scenes: re-exported)
from .decoder import Decoder
from .encoder import Encoder


_DynFieldQueryParams = _lib.AetherDynFieldQueryParams


class AetherDynamicVars(SceneLossMixin, SceneRolloutMixin, nn.Module):
    one_call_step = True       # predict_future's steps go through aether_dyn_step (False: the three staged calls + torch glue)
    _STEP_WS_CAPTURE_CHECK = "the step workspace must be reserved outside graph capture (reserve())"

    def __init__(self, params, device="cuda"):
        super().__init__()
        self.encoder = Encoder(params, device=None)                       # creation order of :19-62
        self.decoder = Decoder(params, device=None)
        self.num_edge_types = params.get("num_edge_types")
        self.gumbel_temp = params.get("gumbel_temp")
        self.kl_coef = params.get("kl_coef", 1.)                      # read by the training scripts
        self._init_loss_config(params)
        object.__setattr__(self.encoder, "_owner", self)              # Encoder.forward queries this model's field net
        self.num_dims = 2
        self.field_hidden = hidden_size = params["field_hidden"]
        if hidden_size % 32 != 0:
            raise ValueError("field_hidden must be a multiple of 32")
        self.field_net = nn.Sequential(nn.Linear(2 * hidden_size, hidden_size), nn.SiLU(),
                                       nn.Linear(hidden_size, hidden_size), nn.SiLU(), nn.Linear(hidden_size, 2))
        self.coordinate_embedding = _CoordinateEmbedding(2, hidden_size // 2, params.get("rff_std", 1.0))
        self.angular_embedding = nn.Linear(2, hidden_size)
        self._ws = None
        if device is not None:
            self.to(device)

    def _field_struct(self):
        fn = self.field_net
        tensors = [self.coordinate_embedding.B, self.angular_embedding.weight, self.angular_embedding.bias, fn[0].weight,
                   fn[0].bias, fn[2].weight, fn[2].bias, fn[4].weight, fn[4].bias]
        for t in tensors:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise _lib.AetherHipError("field parameters must be contiguous fp32 CUDA tensors")
        return _DynFieldQueryParams(*[t.data_ptr() for t in tensors])

    @torch.no_grad()
    def predict_field(self, x, masks=None, n_present=None):
        """:64-79.  x [..., Nmax, 4] -> (field [..., Nmax, 2], zero where masks is 0; coords of the present objects).
        ``n_present``: the number of non-zero mask entries when the caller knows it on the host (no device round trip)."""
        if not x.is_cuda:
            raise _lib.AetherHipError("aether_amd AetherDynamicVars runs on an MI355X only; got a CPU tensor "
                                      "(there is no CPU fallback)")
        lib = _lib.load()
        if masks is None:
            masks = torch.ones_like(x[..., 0], dtype=torch.bool)
        m = masks.to(x.device).bool()
        predicted_field = torch.zeros_like(x[..., :2], dtype=torch.float32)
        idx = None
        if n_present is None:
            xs = x[m].detach().to(torch.float32).contiguous()
        else:
            idx = torch.nonzero_static(m.reshape(-1), size=int(n_present))[:, 0]
            xs = x.detach().reshape(-1, x.shape[-1]).index_select(0, idx).to(torch.float32)
        coords = torch.cat([xs[..., :2], nn.functional.normalize(xs[..., 2:], dim=-1)], -1)
        n = xs.shape[0]
        if n == 0:
            return predicted_field, coords
        h = self.field_hidden
        ps = self._field_struct()
        need = lib.aether_dyn_field_workspace_bytes(n, h)
        ws = cached_workspace(self, "_ws", need, x.device)
        out = torch.empty(n, 2, dtype=torch.float32, device=x.device)
        st = lib.aether_dyn_field(C.byref(ps), h, n, xs.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(),
                                  torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, "aether_dyn_field")
        if idx is None:
            predicted_field[m] = out
        else:
            predicted_field.view(-1, 2).index_copy_(0, idx, out)
        return predicted_field, coords

    @torch.no_grad()
    def single_step_forward(self, inputs, node_masks, graph_info, decoder_hidden, edge_logits, hard_sample, current_field,
                            uniform=None, n_present=None):
        """:133-145.  ``uniform``: the U(0,1) draw of gumbel_softmax ([E, K]); drawn on the device when omitted."""
        if not hard_sample:
            raise _lib.AetherHipError("only hard_sample=True (evaluation / prediction) is part of this path")
        if isinstance(edge_logits, (list, tuple)):                     # B scenes (single_step_forward_batched of the encoder)
            # one sampling pass over the edges of all scenes (torch.rand fills a tensor in index order: the draws of scene b
            # differ from those of B separate calls, as any batched sampler's do; pass `uniform` to fix them)
            K = edge_logits[0].shape[-1]
            sizes = [lg.nelement() // K for lg in edge_logits]
            lg_all = torch.cat([lg.reshape(-1, K) for lg in edge_logits])
            if uniform is None:
                u_all = torch.rand(lg_all.shape, device=lg_all.device)
            else:
                u_all = torch.cat([uniform[b].reshape(-1, K).to(lg_all.device) for b in range(len(edge_logits))])
            edges = list(gumbel_softmax_hard(lg_all, u_all, self.gumbel_temp).reshape(-1, K).split(sizes)) if lg_all.numel() \
                else [lg.reshape(0, K) for lg in edge_logits]
            predictions, decoder_hidden = self.decoder.forward_batched(inputs, decoder_hidden, edges, node_masks, graph_info,
                                                                       current_field)
            return predictions, decoder_hidden, edges
        if edge_logits.nelement() != 0:
            if uniform is None:
                uniform = torch.rand(edge_logits.shape, device=edge_logits.device)
            edges = gumbel_softmax_hard(edge_logits, uniform.reshape(edge_logits.shape).to(edge_logits.device), self.gumbel_temp)
        else:
            edges = torch.empty_like(edge_logits)
        predictions, decoder_hidden = self.decoder(inputs, decoder_hidden, edges, node_masks, graph_info, current_field,
                                                   n_present=n_present)
        return predictions, decoder_hidden, edges

    def _step_config(self):
        enc, dec = self.encoder, self.decoder
        _, n_layers, prior_hidden = enc._param_struct()
        return _DynStepConfig(self.field_hidden, enc.hidden_size, enc.rnn_hidden_size, n_layers, prior_hidden,
                              self.num_edge_types, dec.msg_out_shape, 1 if dec.skip_first_edge_type else 0,
                              1 if enc.pos_representation == "polar" else 0, 1 if dec.pos_representation == "polar" else 0,
                              10, float(self.gumbel_temp))

    def _step_entries(self, lib):
        """One step of one scene (``SceneRolloutMixin._step_one_call``): the single-scene ``aether_dyn_step``, which sizes for
        the largest in_degree a step accepts and takes the actual one behind the graph."""
        def step(cfg, Nmax, n, E, in_degree, state, mask, node_inds, send, recv, e2n, *rest):
            head = (self._field_struct(), self.encoder._param_struct()[0], self.decoder._param_struct())
            return lib.aether_dyn_step(*(C.byref(h) for h in head), cfg, Nmax, n, E, state, mask, node_inds, send, recv, e2n,
                                       in_degree, *rest)
        return (lambda cfg, Nmax, n, E, in_degree: lib.aether_dyn_step_workspace_bytes(cfg, Nmax, n, E)), step, "aether_dyn_step"

    @torch.no_grad()
    def _step_core(self, state, present, node_inds_t, gsend, grecv, e2n, prior_h, prior_c, dec_state, uniform_t):
        """One step of ``predict_future`` for one scene: (prediction [1, Nmax, 4], prior state h, c, decoder state).  The
        number of present objects is ``node_inds_t.numel()`` (host-known): no stage reads a count back from the device."""
        if self.one_call_step:
            return self._step_one_call(state, present, node_inds_t, gsend, grecv, e2n, prior_h, prior_c, dec_state, uniform_t)
        n_t = int(node_inds_t.numel())
        gi = (gsend, grecv, e2n)
        field, _ = self.predict_field(state, present, n_present=n_t)
        logits, (new_h, new_c) = self.encoder.single_step_forward(state, present, node_inds_t, gi, (prior_h, prior_c), field,
                                                                   n_present=n_t)
        last, new_dec, _ = self.single_step_forward(state, present, gi, dec_state, logits, True, field, uniform_t,
                                                    n_present=n_t)
        return last, new_h, new_c, new_dec

    def reserve(self, n_objects_max, k=10):
        """Size the workspaces of the three stages for scenes of up to ``n_objects_max`` present objects (kNN graphs with
        ``k`` neighbours).  Captured steps (``predict_future(graph=True)``) bake workspace addresses into their graphs, so
        no stage may re-allocate after the first capture: this runs before it, outside any capture."""
        lib = _lib.load()
        dev = next(self.parameters()).device
        need_f = need_e = need_d = 0
        ps_e = self.encoder._param_struct()
        for n in range(2, int(n_objects_max) + 1):                    # host arithmetic only; the sizes need not be monotone
            E = n * min(int(k), n - 1)
            need_f = max(need_f, lib.aether_dyn_field_workspace_bytes(n, self.field_hidden))
            need_e = max(need_e, lib.aether_dyn_prior_workspace_bytes(self.encoder.hidden_size, self.encoder.rnn_hidden_size,
                                                                      ps_e[2], n, E))
            need_d = max(need_d, lib.aether_dyn_decoder_workspace_bytes(self.decoder.msg_out_shape, n, E))
        if self.one_call_step:
            cfg = self._step_config()
            need_s = 0
            for n in range(2, int(n_objects_max) + 1):
                need_s = max(need_s, lib.aether_dyn_step_workspace_bytes(C.byref(cfg), int(n_objects_max), n,
                                                                         n * min(int(k), n - 1)))
            cached_workspace(self, "_step_ws", need_s, dev, capture_check="reserve() must run outside graph capture")
        for mod, need in ((self, need_f), (self.encoder, need_e), (self.decoder, need_d)):
            cached_workspace(mod, "_ws", need, dev, capture_check="reserve() must run outside graph capture")

    def _captured_step(self, args):
        """``_step_core`` as a hipGraph replay, one graph per (present objects, edges, slots) signature.

        Round 2 tried this and met a GPU memory access fault at the largest scene of a test.  The recorded
        facts point at buffer lifetime, not at the kernels (the eager path launches the same ones): the stages re-allocated
        their workspace whenever a step needed more than the last -- inside a capture that is an allocation from the
        graph's pool, and the buffer it replaced went back to a pool that earlier graphs still write to on replay.  Here
        nothing persistent is allocated during capture: workspaces are sized for the largest scene first (``reserve``),
        weight-derived caches are built by an eager warm-up call of the same signature, and the capture is discarded if a
        workspace pointer moved nevertheless.  The warm-up also validates, once per signature, the sizes the host
        hands down: the mask really has ``n_present`` non-zero entries."""
        state, present, ni, gs, gr, e2n, ph, pc, dec, u = args
        key = (int(ni.numel()), int(gs.numel()), tuple(e2n.shape), tuple(state.shape), tuple(ph.shape), tuple(dec.shape))
        cache = self.__dict__.setdefault("_step_graphs", {})
        hit = cache.get(key)
        if hit is None:
            if int((present != 0).sum()) != key[0]:                  # one device round trip per NEW signature only
                raise ValueError("node_inds and the mask disagree about the number of present objects")
            self.reserve(state.shape[1])
            static = [a.clone() for a in args]
            self._step_core(*static)                                  # eager: image caches, pointer structs, lazy init
            torch.cuda.synchronize()
            wsp = lambda: (self._ws.data_ptr(), self.encoder._ws.data_ptr(), self.decoder._ws.data_ptr(),
                           self.__dict__["_step_ws"].data_ptr() if self.__dict__.get("_step_ws") is not None else 0)
            ptrs = wsp()
            g = torch.cuda.CUDAGraph()
            pool = self.__dict__.setdefault("_step_pool", torch.cuda.graph_pool_handle())
            with torch.cuda.graph(g, pool=pool):
                outs = self._step_core(*static)
            if ptrs != wsp():
                raise _lib.AetherHipError("a workspace was re-allocated during capture: the graph is not safe to replay")
            hit = cache[key] = (g, static, outs)
        g, static, outs = hit
        for dst, src in zip(static, args):
            dst.copy_(src)
        # one replay in flight at a time: replays of a captured step enqueued behind a running one ended in a GPU memory
        # access fault while the decoder's all-types filter kernel was a graph node (bisected to that node
        # and the runtime's graph packet capture; the library no longer launches it) -- kept as a second line of defence
        torch.cuda.current_stream(static[0].device).synchronize()
        g.replay()
        # graphs share one memory pool: a later replay of another signature may reuse these buffers
        return tuple(o.clone() for o in outs)

    @torch.no_grad()
    def predict_future(self, inputs, masks, node_inds, graph_info, burn_in_masks, uniform=None, graph=False):
        """:245-273.  inputs [1, T, Nmax, 4], masks / burn_in_masks [1, T, Nmax], node_inds[0][t], graph_info[0][t]: the
        present objects and their graph per time step.  ``uniform``: per-step Gumbel draws (list of [E_t, K]).
        With B > 1 scenes (inputs [B, T, Nmax, 4], node_inds[b][t], graph_info[b][t], uniform[t][b]) every time step is
        ONE batched call per stage (predict_future_batched) -- the reference raises on batch > 1 (:588-591).
        One scene, default: the whole loop is ONE library call (``_predict_future_rollout``: 52 launches per step, no host
        round trip, nothing left for a captured graph to save -- measured 0.35 ms per step against 0.41 ms for replays of a
        captured aether_dyn_step; ``graph=True`` is accepted and means the same thing there).  With ``one_call_step = False``
        (the staged calls + torch glue of rounds 1-2) ``graph=True`` replays a captured hipGraph per step signature
        (``_captured_step``); bit-identical to the eager loop either way."""
        return self._predict_future(inputs, masks, node_inds, graph_info, burn_in_masks, uniform, graph=graph)

    def _staged_step(self, state, present, ni_t, gi_t, prior_state, dec_state, uniform_t, graph=False):
        # the data set hands over the present objects of every step (node_inds, built from the masks): their number
        # is known on the host, which spares the three stages their device round trips (mask -> index list)
        dev = state.device
        n_t = int(ni_t.numel())
        if n_t >= 2:
            gs, gr, e2n = (g.to(dev) for g in gi_t)
            u_t = uniform_t if uniform_t is not None else torch.rand(gs.numel(), self.num_edge_types, device=dev)
            args = (state.to(torch.float32), present.to(dev).to(torch.float32), ni_t.to(dev), gs, gr, e2n,
                    prior_state[0], prior_state[1], dec_state.to(torch.float32),
                    u_t.to(dev).reshape(gs.numel(), self.num_edge_types).to(torch.float32))
            last, new_h, new_c, dec_state = self._captured_step(args) if graph else self._step_core(*args)
            return last, (new_h, new_c), dec_state
        # nobody or one object: the stages' own early exits
        field, _ = self.predict_field(state, present, n_present=n_t)
        logits, prior_state = self.encoder.single_step_forward(state, present, ni_t, gi_t, prior_state, field, n_present=n_t)
        last, dec_state, _ = self.single_step_forward(state, present, gi_t, dec_state, logits, True, field, uniform_t,
                                                      n_present=n_t)
        return last, prior_state, dec_state

    def _batched_staged_step(self, state, present, ni_t, gi_t, prior_state, dec_state, uniform_t):
        """B scenes through the staged calls (``one_call_step = False``, or more than 256 scenes): one field query, one
        kNN + prior step, one sampling pass and one decoder step over the present objects of ALL scenes."""
        field, _ = self.predict_field(state, present)
        logits, prior_state = self.encoder.single_step_forward_batched(state, present, ni_t, gi_t, prior_state, field)
        last, dec_state, _ = self.single_step_forward(state, present, gi_t, dec_state, logits, True, field, uniform_t)
        return last, prior_state, dec_state

    # -- calculate_loss(is_train=False): _loss.SceneLossMixin ------------------------------------------------------------------
    def _encode_sequence(self, inputs, node_masks, node_inds, graph_info):
        return self.encoder(inputs, node_masks, node_inds, graph_info)

    def _loss_entries(self, lib):
        head = (self._field_struct(), self.decoder._param_struct())
        return (lib.aether_dyn_loss_rollout_workspace_bytes, lib.aether_dyn_loss_rollout, "aether_dyn_loss_rollout",
                tuple(C.byref(h) for h in head))

    def _loss_stage_step(self, state, mask, gi, decoder_hidden, logits, uniform_t, n_present):
        field, _ = self.predict_field(state, mask, n_present=n_present)
        return self.single_step_forward(state, mask, gi, decoder_hidden, logits, True, field, uniform_t, n_present=n_present)

    def _rollout_entries(self, lib):
        """The entries ``_predict_future_rollout`` / ``predict_future_packed`` (``_rollout.SceneRolloutMixin``) call."""
        head = (self._field_struct(), self.encoder._param_struct()[0], self.decoder._param_struct())
        return (lib.aether_dyn_rollout_batched_workspace_bytes, lib.aether_dyn_rollout_batched, "aether_dyn_rollout_batched",
                tuple(C.byref(h) for h in head))
