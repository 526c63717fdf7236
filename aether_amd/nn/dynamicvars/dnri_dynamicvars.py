"""MI355X prediction path of the reference's variable-N dNRI baseline:
``nn.dynamicvars.dnri_dynamicvars.DNRIDynamicVars`` (dnri_dynamicvars.py:12-688) -- ``single_step_forward`` and
``predict_future``, the path experiments/ind runs when it compares Aether against its baseline.

The model has no field, no local frames, no edge attributes and no filter.  The encoder's prior step (:386-461, :544-570)
is the NRI stack on the raw 4 columns of the present objects over the encoder's own kNN graph (``mlp1``, ``[x_send | x_recv]``,
``mlp2``, ``index_add_`` over the receiver -- a plain sum --, ``mlp3``, ``[x_send | x_recv | skip]``, ``mlp4``), one LSTM step per
edge in the slot of the CALLER's edge at the same position, and ``prior_fc_out``; the decoder (:618-688) passes tanh messages
between hidden states on the caller's graph, sums them over ``edge2node_inds`` / (num_vars - 1) and gates them GRU-style with
``input_r / _i / _n`` of the raw inputs.

Sub-modules carry the reference's names and are created in its order, so a seeded construction or ``load_state_dict`` of a
reference checkpoint gives the same weights (``encoder.reverse_rnn.*`` is held and never read: the reference's sequence encoder never calls it, :531-536).  The
computation runs in libaether_hip.so (``aether_dyn_dnri_*``, csrc/dyn_dnri.h, csrc/dyn_loss.h) on the scene engine of
``AetherDynamicVars``: the whole loop of 1 .. 256 scenes is ONE library call, and ``calculate_loss(is_train=False)`` -- the
runner's validation NLL / KL -- is two (``_loss.SceneLossMixin``).  Not part of this path, each raising by name:
``calculate_loss(is_train=True)``, ``predict_future_fixedwindow``, ``get_prior_posterior``, ``get_edge_probs``, training mode,
``hard_sample=False``, CPU tensors.  A (scene, step) with exactly
one present object is refused, as the engine refuses it for ``AetherDynamicVars``.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from ... import _lib
from ...knn import csr_by_receiver, knn_edges
from ..seq2seq.encoder import _RefNRIMLP, _mlp_out, gumbel_softmax_hard
from ._loss import SceneLossMixin, check_sequence_args, sequence_logits
from ._rollout import SceneRolloutMixin
from ._scene import _DynStepConfig, cached_workspace, f32

_NOT_HERE = ("is not part of the prediction path of aether_amd's DNRIDynamicVars (single_step_forward, predict_future, "
             "predict_future_packed)")
_ONE_OBJECT = ("a scene with one present object: the scene engine refuses it (aether_dyn_dnri_step_batched), as it does for "
               "AetherDynamicVars")
_KNN_K = 10                                              # knn_edges(..., k=10), dnri_dynamicvars.py:435


def _cpu_error(who):
    return _lib.AetherHipError(f"aether_amd {who} runs on an MI355X only; got a CPU tensor (there is no CPU fallback)")


def _check_params(module):
    for t in list(module.parameters()) + list(module.buffers()):
        if t.dtype.is_floating_point and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise _lib.AetherHipError(f"{type(module).__name__} parameters must be contiguous fp32 CUDA tensors")


def _mlp(n_in, n_hid, n_out, no_bn):
    m = _RefNRIMLP(n_in, n_hid, n_out)
    if no_bn:
        m.bn = None                                    # RefNRIMLP(no_bn=True): no BatchNorm module, no keys (creating one draws nothing)
    return m


class DNRI_DynamicVars_Encoder(nn.Module):
    """Parameter holder and staged prior step of ``DNRI_DynamicVars_Encoder`` (dnri_dynamicvars.py:284-570)."""

    def __init__(self, params, device=None):
        super().__init__()
        self.num_edges = params["num_edge_types"]
        no_bn = params["no_encoder_bn"]
        if params["encoder_dropout"] != 0.0:
            raise ValueError("encoder_dropout must be 0.0 (inference path)")
        hidden_size = params["encoder_hidden"]
        self.rnn_hidden_size = rnn_hidden_size = params["encoder_rnn_hidden"] or hidden_size
        if params["encoder_rnn_type"] != "lstm":
            raise ValueError("encoder_rnn_type must be 'lstm' (the GRU encoder is not part of this path)")
        if params["input_size"] != 4:
            raise ValueError("the variable-N encoder is 2-D (input_size 4)")
        if hidden_size % 128 != 0 or rnn_hidden_size % 16 != 0:
            raise ValueError("encoder_hidden must be a multiple of 128 and encoder_rnn_hidden of 16")
        if params["encoder_normalize_mode"] != "normalize_all":
            raise NotImplementedError("encoder_normalize_mode must be 'normalize_all' (as the reference, :545-548)")
        self.hidden_size = hidden_size
        inp_size = params["input_size"]
        # creation order of dnri_dynamicvars.py:300-344
        self.mlp1 = _mlp(inp_size, hidden_size, hidden_size, no_bn)
        self.mlp2 = _mlp(hidden_size * 2, hidden_size, hidden_size, no_bn)
        self.mlp3 = _mlp(hidden_size, hidden_size, hidden_size, no_bn)
        self.mlp4 = _mlp(hidden_size * 3, hidden_size, hidden_size, no_bn)
        self.train_data_len = params.get("train_data_len", -1)
        self.forward_rnn = nn.LSTM(hidden_size, rnn_hidden_size, batch_first=True)
        self.reverse_rnn = nn.LSTM(hidden_size, rnn_hidden_size, batch_first=True)
        self.encoder_fc_out = _mlp_out(2 * rnn_hidden_size, params.get("encoder_mlp_hidden"), self.num_edges,
                                       params["encoder_mlp_num_layers"])
        self.prior_layers = params["prior_num_layers"]
        self.prior_fc_out = _mlp_out(rnn_hidden_size, params.get("prior_hidden_size"), self.num_edges, self.prior_layers)
        self.normalize_mode = params["encoder_normalize_mode"]
        for m in self.modules():                                   # init_weights, :346-350
            if isinstance(m, nn.Linear):
                nn.init.xavier_normal_(m.weight.data)
                m.bias.data.fill_(0.1)
        self._ws = None
        if device is not None:
            self.to(device)

    def get_initial_hidden(self, inputs):
        batch = inputs.size(0) * inputs.size(2) * (inputs.size(2) - 1)               # :363-367
        return (torch.zeros(1, batch, self.rnn_hidden_size, device=inputs.device),
                torch.zeros(1, batch, self.rnn_hidden_size, device=inputs.device))

    def _param_struct(self):
        """-> (pointer struct, prior layers, prior hidden)."""
        _check_params(self)
        ps = _lib.AetherDynDnriPriorParams()
        ptr = lambda t: t.data_ptr()
        for l, name in enumerate(("mlp1", "mlp2", "mlp3", "mlp4")):
            m = getattr(self, name)
            ps.mlp_w0[l], ps.mlp_b0[l] = ptr(m.model[0].weight), ptr(m.model[0].bias)
            ps.mlp_w3[l], ps.mlp_b3[l] = ptr(m.model[3].weight), ptr(m.model[3].bias)
            if m.bn is not None:
                ps.mlp_bn_w[l], ps.mlp_bn_b[l] = ptr(m.bn.weight), ptr(m.bn.bias)
                ps.mlp_bn_mean[l], ps.mlp_bn_var[l] = ptr(m.bn.running_mean), ptr(m.bn.running_var)
        rnn = self.forward_rnn
        ps.lstm_w_ih, ps.lstm_w_hh = ptr(rnn.weight_ih_l0), ptr(rnn.weight_hh_l0)
        ps.lstm_b_ih, ps.lstm_b_hh = ptr(rnn.bias_ih_l0), ptr(rnn.bias_hh_l0)
        layers = [self.prior_fc_out] if isinstance(self.prior_fc_out, nn.Linear) else \
            [m for m in self.prior_fc_out if isinstance(m, nn.Linear)]
        for l, lin in enumerate(layers):
            ps.prior_w[l], ps.prior_b[l] = ptr(lin.weight), ptr(lin.bias)
        return ps, len(layers), (layers[0].out_features if len(layers) > 1 else 0)

    def _sequence_config(self):
        """The configuration the sequence entry reads (the decoder's members are placeholders that pass its checks)."""
        _, n_layers, prior_hidden = self._param_struct()
        return _DynStepConfig(0, self.hidden_size, self.rnn_hidden_size, n_layers, prior_hidden, self.num_edges, 128, 0, 0, 0,
                              _KNN_K, 1.0)

    @torch.no_grad()
    def forward(self, inputs, node_masks, all_node_inds, all_graph_info, normalized_inputs=None):
        """dnri_dynamicvars.py:463-542 as ONE library call (``aether_dyn_dnri_sequence_logits``).  inputs [1, F, Nmax, 4],
        node_masks [1, F, Nmax], all_node_inds[0][t]: the present objects of frame t (two or more) -> (prior_result,
        encoder_result [1, sum_t E_t, K], forward_state).  The reference drops the forward LSTM state it computes (:506-509)
        and never calls ``reverse_rnn`` (:531-536): every frame is an LSTM step from the zero state, the posterior head sees
        [h | 0], and ``forward_state`` comes back as zeros.  ``reverse_rnn.*`` stays in the state_dict and is never read."""
        if not inputs.is_cuda:
            raise _cpu_error("DNRI_DynamicVars_Encoder.forward (the sequence encoder: prior and posterior logits)")
        if self.training:
            raise _lib.AetherHipError("the encoder uses BatchNorm running statistics (training mode is not part of this path): "
                                      "call .eval() first")
        check_sequence_args(inputs, normalized_inputs)
        lib = _lib.load()
        entries = (lib.aether_dyn_dnri_sequence_logits_workspace_bytes, lib.aether_dyn_dnri_sequence_logits,
                   "aether_dyn_dnri_sequence_logits", (C.byref(self._param_struct()[0]),))
        return sequence_logits(self, entries, self._sequence_config(), inputs, node_masks, all_node_inds)

    @torch.no_grad()
    def single_step_forward(self, inputs, node_masks, node_inds, all_graph_info, forward_state):
        """dnri_dynamicvars.py:544-570.  inputs [1, Nmax, 4], node_masks [1, Nmax], node_inds: the present objects,
        all_graph_info = (send, recv, ...) in their numbering, forward_state (h, c) each [1, Nmax (Nmax - 1), R]
        -> (prior_logits [1, E, K], forward_state)."""
        if not inputs.is_cuda:
            raise _cpu_error("DNRI_DynamicVars_Encoder")
        if self.training:
            raise _lib.AetherHipError("the prior step uses BatchNorm running statistics (training mode is not part of this "
                                      "path): call .eval() first")
        lib = _lib.load()
        dev = inputs.device
        if inputs.size(0) != 1:
            raise ValueError("Batching during forward not currently supported")       # :464-465
        n = int(len(node_inds))
        if n == 0:                                                                   # :567-568
            return torch.empty(1, 0, self.num_edges, device=dev), forward_state
        if n == 1:
            raise _lib.AetherHipError(_ONE_OBJECT)
        Nmax, h, R, K = inputs.size(1), self.hidden_size, self.rnn_hidden_size, self.num_edges
        x = f32(inputs, dev)
        mask = node_masks.reshape(-1).to(dev)
        # the encoder's own kNN graph of the present objects, from the current inputs (:408); n is known on the host
        send, recv, _ = knn_edges(x, mask.reshape(1, -1).to(torch.float32), k=_KNN_K, n_present=n)
        idx = torch.nonzero_static(mask, size=n)[:, 0]
        cur_in = x[0].index_select(0, idx)
        E = send.numel()
        order, rowptr = csr_by_receiver(recv, n)
        # LSTM state rows of the caller's edges: one slot per fully connected pair (:554-556); row e of the features meets
        # the slot of edge e of the caller's graph
        gsend, grecv = all_graph_info[0].to(dev), all_graph_info[1].to(dev)
        node_inds = node_inds.to(dev)
        gs, gr = node_inds[gsend], node_inds[grecv]
        slot = gs * (Nmax - 1) + gr - (gr >= gs).long()
        if slot.numel() != E:
            raise ValueError("graph_info and the encoder's kNN graph list a different number of edges "
                             "(n_edges must be n_present * min(10, n_present - 1))")
        h0, c0 = f32(forward_state[0], dev)[0, slot].contiguous(), f32(forward_state[1], dev)[0, slot].contiguous()
        ps, n_layers, prior_hidden = self._param_struct()
        need = lib.aether_dyn_dnri_prior_workspace_bytes(h, R, prior_hidden, n, E)
        ws = cached_workspace(self, "_ws", need, dev)
        logits = torch.empty(E, K, dtype=torch.float32, device=dev)
        h1, c1 = torch.empty_like(h0), torch.empty_like(c0)
        st = lib.aether_dyn_dnri_prior_step(C.byref(ps), h, R, n_layers, prior_hidden, K, 0, n, E, cur_in.data_ptr(),
                                            h0.data_ptr(), c0.data_ptr(), send.data_ptr(), recv.data_ptr(), order.data_ptr(),
                                            rowptr.data_ptr(), ws.data_ptr(), ws.numel(), logits.data_ptr(),
                                            h1.data_ptr(), c1.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(st, "aether_dyn_dnri_prior_step")
        new_h, new_c = f32(forward_state[0], dev).clone(), f32(forward_state[1], dev).clone()
        new_h[0, slot], new_c[0, slot] = h1, c1
        return logits.unsqueeze(0), (new_h, new_c)


class DNRI_DynamicVars_Decoder(nn.Module):
    """Parameter holder and staged step of ``DNRI_DynamicVars_Decoder`` (dnri_dynamicvars.py:573-688); its ``init_weights``
    is never called by the reference: the layers keep torch's default initialisation."""

    def __init__(self, params, device=None):
        super().__init__()
        input_size = params["input_size"]
        self.gpu = params["gpu"]
        n_hid = params["decoder_hidden"]
        edge_types = params["num_edge_types"]
        skip_first = params["skip_first"]
        out_size = params["input_size"]
        self.dropout_prob = params["decoder_dropout"]
        if self.dropout_prob != 0.0:
            raise ValueError("decoder_dropout must be 0.0: the reference calls F.dropout without training=, so it drops in "
                             "evaluation mode too (:653, :678-679); that is refused, not reproduced")
        if input_size != 4:
            raise ValueError("the variable-N decoder is 2-D (input_size 4)")
        if n_hid % 128 != 0:
            raise ValueError("decoder_hidden must be a multiple of 128")
        if not 1 <= edge_types <= 4 or edge_types - (1 if skip_first else 0) < 1:
            raise ValueError("1..4 edge types with at least one used (num_edge_types - skip_first >= 1)")
        self.edge_types = edge_types
        self.msg_fc1 = nn.ModuleList([nn.Linear(2 * n_hid, n_hid) for _ in range(edge_types)])
        self.msg_fc2 = nn.ModuleList([nn.Linear(n_hid, n_hid) for _ in range(edge_types)])
        self.msg_out_shape = n_hid
        self.skip_first_edge_type = skip_first
        self.hidden_r = nn.Linear(n_hid, n_hid, bias=False)
        self.hidden_i = nn.Linear(n_hid, n_hid, bias=False)
        self.hidden_h = nn.Linear(n_hid, n_hid, bias=False)
        self.input_r = nn.Linear(input_size, n_hid, bias=True)
        self.input_i = nn.Linear(input_size, n_hid, bias=True)
        self.input_n = nn.Linear(input_size, n_hid, bias=True)
        self.out_fc1 = nn.Linear(n_hid, n_hid)
        self.out_fc2 = nn.Linear(n_hid, n_hid)
        self.out_fc3 = nn.Linear(n_hid, out_size)
        self._ws = None
        if device is not None:
            self.to(device)

    def get_initial_hidden(self, inputs):
        return torch.zeros(inputs.size(0), inputs.size(2), self.msg_out_shape, device=inputs.device)

    def _param_struct(self):
        _check_params(self)
        ps = _lib.AetherDynDnriDecoderParams()
        ptr = lambda t: t.data_ptr()
        for k in range(self.edge_types):
            ps.msg_fc1_w[k], ps.msg_fc1_b[k] = ptr(self.msg_fc1[k].weight), ptr(self.msg_fc1[k].bias)
            ps.msg_fc2_w[k], ps.msg_fc2_b[k] = ptr(self.msg_fc2[k].weight), ptr(self.msg_fc2[k].bias)
        ps.hidden_r_w, ps.hidden_i_w, ps.hidden_h_w = ptr(self.hidden_r.weight), ptr(self.hidden_i.weight), ptr(self.hidden_h.weight)
        for name in ("r", "i", "n"):
            lin = getattr(self, "input_" + name)
            setattr(ps, f"input_{name}_w", ptr(lin.weight)); setattr(ps, f"input_{name}_b", ptr(lin.bias))
        for idx in (1, 2, 3):
            lin = getattr(self, f"out_fc{idx}")
            setattr(ps, f"out{idx}_w", ptr(lin.weight)); setattr(ps, f"out{idx}_b", ptr(lin.bias))
        return ps

    @torch.no_grad()
    def forward(self, inputs, hidden, edges, node_masks, graph_info):
        """dnri_dynamicvars.py:618-688.  inputs [1, Nmax, 4], hidden [1, Nmax, h], edges [1, E, K] (one-hot rows: hard
        samples), node_masks [1, Nmax] (or [Nmax]), graph_info = (send_edges, recv_edges, edge2node_inds) in the numbering
        of the present objects -> (pred_all [1, Nmax, 4], hidden [1, Nmax, h])."""
        if not inputs.is_cuda:
            raise _cpu_error("DNRI_DynamicVars_Decoder")
        if inputs.size(0) != 1:
            raise ValueError("Batching during forward not currently supported: several scenes go through the model "
                             "(predict_future_batched / predict_future_packed)")
        lib = _lib.load()
        dev = inputs.device
        h, K = self.msg_out_shape, self.edge_types
        inputs, hidden = f32(inputs, dev), f32(hidden, dev)
        node_inds = node_masks.reshape(-1).to(dev).nonzero()[:, -1]
        nv = int(node_inds.numel())
        if nv == 0:                                                                    # :662-664
            return torch.zeros_like(inputs), hidden
        if nv == 1:
            raise _lib.AetherHipError(_ONE_OBJECT)
        send, recv, e2n = (t.to(device=dev, dtype=torch.int64).contiguous() for t in graph_info)
        E = send.numel()
        if recv.numel() != E or edges.shape != (1, E, K) or e2n.ndim != 2 or e2n.shape[0] != nv:
            raise ValueError("graph_info / edges do not match the present objects")
        if E and (int(e2n.min()) < 0 or int(e2n.max()) >= E):
            raise ValueError("graph_info: an edge2node entry names an edge the graph does not have")
        cur_in, cur_h = inputs[0, node_inds].contiguous(), hidden[0, node_inds].contiguous()
        rowptr = torch.arange(nv + 1, device=dev, dtype=torch.int64) * e2n.shape[1]
        order = e2n.reshape(-1).contiguous()
        ew = f32(edges, dev)[0]
        need = lib.aether_dyn_dnri_decoder_workspace_bytes(h, K, nv, E)
        ws = cached_workspace(self, "_ws", need, dev)
        out = torch.empty(nv, 4, dtype=torch.float32, device=dev)
        new_h = torch.empty(nv, h, dtype=torch.float32, device=dev)
        ps = self._param_struct()
        st = lib.aether_dyn_dnri_decoder_step_batched(C.byref(ps), h, K, 1 if self.skip_first_edge_type else 0, 0, nv, E,
                                                      cur_in.data_ptr(), cur_h.data_ptr(), ew.data_ptr(), send.data_ptr(),
                                                      recv.data_ptr(), order.data_ptr(), rowptr.data_ptr(), float(nv - 1), None,
                                                      ws.data_ptr(), ws.numel(), out.data_ptr(), new_h.data_ptr(),
                                                      torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(st, "aether_dyn_dnri_decoder_step_batched")
        hidden = hidden.clone()
        hidden[0, node_inds] = new_h
        pred_all = torch.zeros_like(inputs)
        pred_all[0, node_inds] = out
        return pred_all, hidden


class DNRIDynamicVars(SceneLossMixin, SceneRolloutMixin, nn.Module):
    one_call_step = True       # predict_future is ONE library call (False: the staged calls + torch glue, step by step)

    def __init__(self, params, device="cuda"):
        super().__init__()
        self.encoder = DNRI_DynamicVars_Encoder(params, device=None)              # creation order of :15-17
        self.decoder = DNRI_DynamicVars_Decoder(params, device=None)
        self.num_edge_types = params.get("num_edge_types")
        self.gumbel_temp = params.get("gumbel_temp")
        self.kl_coef = params.get("kl_coef", 1.)                          # read by the training scripts
        self._init_loss_config(params)
        if device is not None:
            self.to(device)

    # -- not part of the prediction path ---------------------------------------------------------------------------------------
    def predict_future_fixedwindow(self, *args, **kwargs):
        raise _lib.AetherHipError("DNRIDynamicVars.predict_future_fixedwindow " + _NOT_HERE)

    def get_prior_posterior(self, *args, **kwargs):
        raise _lib.AetherHipError("DNRIDynamicVars.get_prior_posterior " + _NOT_HERE)

    def get_edge_probs(self, *args, **kwargs):
        raise _lib.AetherHipError("DNRIDynamicVars.get_edge_probs " + _NOT_HERE)

    # -- the prediction path ---------------------------------------------------------------------------------------------------
    _TRAINING_REFUSAL = ("training mode is not part of this path (the prior step uses BatchNorm running statistics): call "
                         ".eval() first")

    def _in_training(self):
        return self.training or self.encoder.training

    @torch.no_grad()
    def single_step_forward(self, inputs, node_masks, graph_info, decoder_hidden, edge_logits, hard_sample, uniform=None):
        """:53-63.  ``uniform``: the U(0,1) draw of gumbel_softmax ([E, K]); drawn on the device when omitted."""
        if not hard_sample:
            raise _lib.AetherHipError("hard_sample=False (training) is not part of this path: only hard samples are decoded")
        self._guard(inputs)
        if edge_logits.nelement() != 0:
            if uniform is None:
                uniform = torch.rand(edge_logits.shape, device=edge_logits.device)
            edges = gumbel_softmax_hard(edge_logits, uniform.reshape(edge_logits.shape).to(edge_logits.device), self.gumbel_temp)
        else:
            edges = torch.empty_like(edge_logits)
        predictions, decoder_hidden = self.decoder(inputs, decoder_hidden, edges, node_masks, graph_info)
        return predictions, decoder_hidden, edges

    def _step_config(self):
        enc, dec = self.encoder, self.decoder
        _, n_layers, prior_hidden = enc._param_struct()
        # field_hidden and the two polar members are not read by the dNRI entries
        return _DynStepConfig(0, enc.hidden_size, enc.rnn_hidden_size, n_layers, prior_hidden, self.num_edge_types,
                              dec.msg_out_shape, 1 if dec.skip_first_edge_type else 0, 0, 0, _KNN_K, float(self.gumbel_temp))

    def _rollout_entries(self, lib):
        head = (self.encoder._param_struct()[0], self.decoder._param_struct())
        return (lib.aether_dyn_dnri_rollout_batched_workspace_bytes, lib.aether_dyn_dnri_rollout_batched,
                "aether_dyn_dnri_rollout_batched", tuple(C.byref(h) for h in head))

    def _step_entries(self, lib):
        """One step of one scene (``SceneRolloutMixin._step_one_call``): ``aether_dyn_dnri_step_batched`` with n_scenes = 1."""
        arrays = lambda n, E, in_degree: ((C.c_int64 * 1)(n), (C.c_int64 * 1)(E), (C.c_int * 1)(in_degree))

        def step(cfg, Nmax, n, E, in_degree, *rest):
            head = (self.encoder._param_struct()[0], self.decoder._param_struct())
            return lib.aether_dyn_dnri_step_batched(*(C.byref(h) for h in head), cfg, 1, Nmax, *arrays(n, E, in_degree), *rest)
        return (lambda cfg, Nmax, n, E, in_degree: lib.aether_dyn_dnri_step_batched_workspace_bytes(
            cfg, 1, Nmax, *arrays(n, E, in_degree))), step, "aether_dyn_dnri_step_batched"

    @torch.no_grad()
    def predict_future(self, inputs, masks, node_inds, graph_info, burn_in_masks, uniform=None):
        """:152-175.  inputs [1, T, Nmax, 4], masks / burn_in_masks [1, T, Nmax], node_inds[0][t], graph_info[0][t]: the present
        objects and their graph per time step.  ``uniform``: per-step Gumbel draws (list of [E_t, K]).  With B > 1 scenes
        (node_inds[b][t], graph_info[b][t], uniform[t][b]) see ``predict_future_batched`` -- the reference raises there.
        Default: the whole loop is ONE library call; ``one_call_step = False`` runs the staged calls step by step."""
        return self._predict_future(inputs, masks, node_inds, graph_info, burn_in_masks, uniform)

    # -- calculate_loss(is_train=False): _loss.SceneLossMixin ------------------------------------------------------------------
    def _encode_sequence(self, inputs, node_masks, node_inds, graph_info):
        return self.encoder(inputs, node_masks, node_inds, graph_info)

    def _loss_entries(self, lib):
        return (lib.aether_dyn_dnri_loss_rollout_workspace_bytes, lib.aether_dyn_dnri_loss_rollout, "aether_dyn_dnri_loss_rollout",
                (C.byref(self.decoder._param_struct()),))

    def _loss_stage_step(self, state, mask, gi, decoder_hidden, logits, uniform_t, n_present):
        return self.single_step_forward(state, mask, gi, decoder_hidden, logits, True, uniform_t)

    def _staged_step(self, state, present, ni_t, gi_t, prior_state, dec_state, uniform_t):
        logits, prior_state = self.encoder.single_step_forward(state, present, ni_t, gi_t, prior_state)
        last, dec_state, _ = self.single_step_forward(state, present, gi_t, dec_state, logits, True, uniform_t)
        return last, prior_state, dec_state
