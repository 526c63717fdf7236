"""MI355X prediction path of the seq2seq dNRI baseline (``nn.seq2seq.dnri.DNRI``).

The reference's baseline (nn/seq2seq/dnri.py:9-624) has no local frames: the encoder is the NRI stack on the raw state
(``mlp1`` on the nodes, ``node2edge``, ``mlp2``, ``edge2node``, ``mlp3``, ``node2edge`` with the skip, ``mlp4``), an LSTM per edge
and two heads (``prior_fc_out`` causal, ``encoder_fc_out`` on both directions); the decoders read the raw inputs --
``DNRI_Decoder`` (:427-534) passes tanh messages between hidden states and gates them GRU-style with ``input_r / _i / _n`` of the
inputs, ``DNRI_MLP_Decoder`` (``decoder_type='ref_mlp'``, :537-624) passes ReLU messages between the inputs themselves and has no
state.  Both return ``inputs + prediction``.  Sub-modules carry the reference's names in its creation order, the non-trainable
``edge2node_mat`` Parameters keep their shapes, so a seeded construction gives its initial values and ``load_state_dict`` of a
reference checkpoint works (81 keys with the recurrent decoder, 72 with the MLP decoder at three prior layers).

The computation runs in libaether_hip.so (``aether_s2s_dnri_step`` / ``_rollout`` / ``_encoder_features``, csrc/s2s_dnri.h) on the
job-table engine of the other seq2seq models: ``predict_future`` (eager or one captured hipGraph), ``single_step_forward`` (the
decoder on given logits), ``calculate_loss(is_train=False)`` and the full-sequence ``encoder(inputs)``.  No frame, edge-attribute
or filter kernel is launched.  Training and ``predict_future_fixedwindow`` are not part of this library, and there is no CPU
fallback.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from ... import _lib
from .aether import _EvalLoss, _FieldHook, _StepLoop
from .decoder import RecurrentDecoder
from .encoder import Encoder, _mlp_out, _RefNRIMLP

_ENTRIES = ("aether_s2s_dnri_plan_bytes", "aether_s2s_dnri_plan_build", "aether_s2s_dnri_workspace_bytes",
            "aether_s2s_dnri_step", "aether_s2s_dnri_rollout")
_CPU = "aether_amd seq2seq models run on an MI355X only; got a CPU tensor (there is no CPU fallback)"
_THROUGH_MODEL = ("of the seq2seq dNRI runs through the model (DNRI.single_step_forward, DNRI.predict_future, DNRI.encoder: "
                  "aether_s2s_dnri_*), not as a call of the module")


_DnriPriorParams = _lib.AetherS2SDnriPriorParams
_DnriDecoderParams = _lib.AetherS2SDnriDecoderParams


_DnriMlpParams = _lib.AetherS2SDnriMlpParams


def _edges(num_vars):
    """send, recv of the fully connected graph without self-loops, as np.where(ones - eye) (dnri.py:271-273)."""
    return torch.where(~torch.eye(num_vars, dtype=bool))


def _onehot(recv, num_vars):
    """encode_onehot(recv_edges) (nn/utils/model_utils.py:7-11) as a float tensor [E, N]."""
    m = torch.zeros(recv.shape[0], num_vars, dtype=torch.float32)
    m[torch.arange(recv.shape[0]), recv] = 1.0
    return m


def _num_dims(params):
    if params["input_size"] not in (4, 6):
        raise ValueError("input_size must be 4 (2-D positions and velocities) or 6 (3-D)")
    return params["input_size"] // 2


def _no_field_cols(params):
    """Columns a layer on the raw state reads besides the state itself: none in dNRI; the field's D in the sub-modules of
    ``ablations.dnri_aether.DNRIAether``, which override ``_field_cols``."""
    return 0


class DNRI_Encoder(nn.Module):
    """Parameter holder of ``DNRI_Encoder`` (dnri.py:262-332), same creation / init order.  ``forward(inputs)`` is the
    full-sequence encoder in evaluation mode once the module belongs to a ``DNRI`` (the library's entries take the model's
    plan); ``single_step_forward`` is part of the model's fused step."""

    def __init__(self, params, device=None):
        super().__init__()
        self.num_vars = num_vars = params["num_vars"]
        self.num_edges = params["num_edge_types"]
        self.sepaate_prior_encoder = params.get("separate_prior_encoder", False)
        if params["encoder_dropout"] != 0.0:
            raise ValueError("encoder_dropout must be 0.0 (inference path)")
        self.send_edges, self.recv_edges = _edges(num_vars)
        self.edge2node_mat = nn.Parameter(_onehot(self.recv_edges, num_vars).t().contiguous(), requires_grad=False)   # [N, E]
        self.save_eval_memory = params.get("encoder_save_eval_memory", False)
        hidden_size = params["encoder_hidden"]
        rnn_hidden_size = params["encoder_rnn_hidden"] or hidden_size
        if params["encoder_rnn_type"] != "lstm":
            raise ValueError("encoder_rnn_type must be 'lstm'")
        if hidden_size % 32 != 0 or rnn_hidden_size % 32 != 0:
            raise ValueError("encoder_hidden and encoder_rnn_hidden must be multiples of 32")
        inp_size = params["input_size"]
        self.num_dims = _num_dims(params)
        self.hidden_size, self.rnn_hidden_size = hidden_size, rnn_hidden_size
        self.mlp1 = _RefNRIMLP(inp_size + self._field_cols(params), hidden_size, hidden_size)
        self.mlp2 = _RefNRIMLP(hidden_size * 2, hidden_size, hidden_size)
        self.mlp3 = _RefNRIMLP(hidden_size, hidden_size, hidden_size)
        self.mlp4 = _RefNRIMLP(hidden_size * 3, hidden_size, hidden_size)
        self.forward_rnn = nn.LSTM(hidden_size, rnn_hidden_size, batch_first=True)
        self.reverse_rnn = nn.LSTM(hidden_size, rnn_hidden_size, batch_first=True)
        self.encoder_fc_out = _mlp_out(2 * rnn_hidden_size, params.get("encoder_mlp_hidden"), self.num_edges,
                                       params["encoder_mlp_num_layers"])
        self.prior_layers = params["prior_num_layers"]
        self.prior_fc_out = _mlp_out(rnn_hidden_size, params.get("prior_hidden_size"), self.num_edges, self.prior_layers)
        for m in self.modules():                                   # init_weights, dnri.py:328-332
            if isinstance(m, nn.Linear):
                nn.init.xavier_normal_(m.weight.data)
                m.bias.data.fill_(0.1)
        self.pos_representation = "cart"                           # (read by the shared step loop; the model has no frames)
        self._cache = {}
        if device is not None:
            self.to(device)

    _field_cols = staticmethod(_no_field_cols)
    _graph = Encoder._graph
    _head = Encoder._head
    _sequence_heads = Encoder._sequence_heads

    def _param_struct(self, with_image=False):
        ps = _DnriPriorParams()
        ptr = lambda t: t.data_ptr()
        for l, name in enumerate(("mlp1", "mlp2", "mlp3", "mlp4")):
            m = getattr(self, name)
            ps.mlp_w0[l], ps.mlp_b0[l] = ptr(m.model[0].weight), ptr(m.model[0].bias)
            ps.mlp_w3[l], ps.mlp_b3[l] = ptr(m.model[3].weight), ptr(m.model[3].bias)
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

    def forward(self, inputs):
        """dnri.py:371-401 in evaluation mode: inputs [B, T, N, 2D] -> (prior_logits, posterior_logits [B, T, E, K], prior_state
        (h, c) each [B, E, rnn])."""
        model = self.__dict__.get("_owner")
        if model is None:
            raise _lib.AetherHipError("DNRI_Encoder.forward " + _THROUGH_MODEL)
        return model._encoder_forward(inputs)

    def single_step_forward(self, inputs, prior_state):
        raise _lib.AetherHipError("DNRI_Encoder.single_step_forward " + _THROUGH_MODEL)


class DNRI_Decoder(nn.Module):
    """Parameter holder of ``DNRI_Decoder`` (dnri.py:427-477), same creation order (its ``init_weights`` is never called: the
    layers keep torch's default initialisation)."""

    def __init__(self, params, device=None):
        super().__init__()
        self.num_vars = num_vars = params["num_vars"]
        input_size = params["input_size"]
        self.num_dims = _num_dims(params)
        self.gpu = params["gpu"]
        n_hid = params["decoder_hidden"]
        edge_types = params["num_edge_types"]
        out_size = params["input_size"]
        self.dropout_prob = params["decoder_dropout"]
        if self.dropout_prob != 0.0:
            raise ValueError("decoder_dropout must be 0.0 (inference path; the reference zeroes it in eval)")
        if n_hid % 32 != 0:
            raise ValueError("decoder_hidden must be a multiple of 32")
        if edge_types - (1 if params["skip_first"] else 0) < 1:
            raise ValueError("the decoder needs at least one used edge type (num_edge_types - skip_first >= 1)")
        self.edge_types = edge_types
        self.msg_fc1 = nn.ModuleList([nn.Linear(2 * n_hid, n_hid) for _ in range(edge_types)])
        self.msg_fc2 = nn.ModuleList([nn.Linear(n_hid, n_hid) for _ in range(edge_types)])
        self.msg_out_shape = n_hid
        self.skip_first_edge_type = params["skip_first"]
        self.hidden_r = nn.Linear(n_hid, n_hid, bias=False)
        self.hidden_i = nn.Linear(n_hid, n_hid, bias=False)
        self.hidden_h = nn.Linear(n_hid, n_hid, bias=False)
        gate_in = input_size + self._field_cols(params)
        self.input_r = nn.Linear(gate_in, n_hid, bias=True)
        self.input_i = nn.Linear(gate_in, n_hid, bias=True)
        self.input_n = nn.Linear(gate_in, n_hid, bias=True)
        self.out_fc1 = nn.Linear(n_hid, n_hid)
        self.out_fc2 = nn.Linear(n_hid, n_hid)
        self.out_fc3 = nn.Linear(n_hid, out_size)
        self.send_edges, self.recv_edges = _edges(num_vars)
        self.edge2node_mat = nn.Parameter(_onehot(self.recv_edges, num_vars), requires_grad=False)                    # [E, N]
        self._cache = {}
        if device is not None:
            self.to(device)

    _has_state = True
    _field_cols = staticmethod(_no_field_cols)
    _graph = RecurrentDecoder._graph

    def get_initial_hidden(self, inputs):
        return torch.zeros(inputs.size(0), inputs.size(2), self.msg_out_shape, device=inputs.device)

    def _param_struct(self):
        ps = _DnriDecoderParams()
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

    def forward(self, inputs, hidden, edges):
        raise _lib.AetherHipError("the decoder step " + _THROUGH_MODEL)


class DNRI_MLP_Decoder(nn.Module):
    """Parameter holder of ``DNRI_MLP_Decoder`` (dnri.py:537-572), same creation order."""

    def __init__(self, params, device=None):
        super().__init__()
        num_vars = params["num_vars"]
        edge_types = params["num_edge_types"]
        n_hid = msg_hid = msg_out = params["decoder_hidden"]
        in_size = params["input_size"]
        self.num_dims = _num_dims(params)
        self.dropout_prob = params["decoder_dropout"]
        if self.dropout_prob != 0.0:
            raise ValueError("decoder_dropout must be 0.0 (inference path; the reference zeroes it in eval)")
        if n_hid % 32 != 0:
            raise ValueError("decoder_hidden must be a multiple of 32")
        if edge_types - (1 if params["skip_first"] else 0) < 1:
            raise ValueError("the decoder needs at least one used edge type (num_edge_types - skip_first >= 1)")
        self.edge_types = edge_types
        ext_size = in_size + self._field_cols(params)
        self.msg_fc1 = nn.ModuleList([nn.Linear(2 * ext_size, msg_hid) for _ in range(edge_types)])
        self.msg_fc2 = nn.ModuleList([nn.Linear(msg_hid, msg_out) for _ in range(edge_types)])
        self.msg_out_shape = msg_out
        self.skip_first_edge_type = params["skip_first"]
        self.out_fc1 = nn.Linear(ext_size + msg_out, n_hid)
        self.out_fc2 = nn.Linear(n_hid, n_hid)
        self.out_fc3 = nn.Linear(n_hid, in_size)
        self.num_vars = num_vars
        self.send_edges, self.recv_edges = _edges(num_vars)
        self.edge2node_mat = nn.Parameter(_onehot(self.recv_edges, num_vars), requires_grad=False)                    # [E, N]
        self._cache = {}
        if device is not None:
            self.to(device)

    _has_state = False
    _field_cols = staticmethod(_no_field_cols)
    _graph = RecurrentDecoder._graph

    def get_initial_hidden(self, inputs):
        return None

    def _param_struct(self):
        ps = _DnriMlpParams()
        ptr = lambda t: t.data_ptr()
        for k in range(self.edge_types):
            ps.msg_fc1_w[k], ps.msg_fc1_b[k] = ptr(self.msg_fc1[k].weight), ptr(self.msg_fc1[k].bias)
            ps.msg_fc2_w[k], ps.msg_fc2_b[k] = ptr(self.msg_fc2[k].weight), ptr(self.msg_fc2[k].bias)
        for idx in (1, 2, 3):
            lin = getattr(self, f"out_fc{idx}")
            setattr(ps, f"out{idx}_w", ptr(lin.weight)); setattr(ps, f"out{idx}_b", ptr(lin.bias))
        return ps

    def forward(self, inputs, hidden, edges):
        raise _lib.AetherHipError("the decoder step " + _THROUGH_MODEL)


class DNRI(_StepLoop, _EvalLoss, nn.Module):
    _encoder_class, _decoder_classes = DNRI_Encoder, (DNRI_Decoder, DNRI_MLP_Decoder)
    _features_entry = "aether_s2s_dnri_encoder_features"

    def __init__(self, params, device="cuda"):
        super().__init__()
        self.num_vars = params["num_vars"]
        self.encoder = self._encoder_class(params)                         # creation order of dnri.py:14-19
        self._markov = params.get("decoder_type", None) == "ref_mlp"
        self.decoder = self._decoder_classes[1 if self._markov else 0](params)
        self.num_edge_types = params.get("num_edge_types")
        # training parameters the runner's scripts read or set (dnri.py:23-38); only evaluation runs here
        self.gumbel_temp = params.get("gumbel_temp")
        self.train_hard_sample = params.get("train_hard_sample")
        self.teacher_forcing_steps = params.get("teacher_forcing_steps", -1)
        self.kl_coef = params.get("kl_coef", 1.)
        self.timesteps = params.get("timesteps", 0)
        self.burn_in_steps = params.get("train_burn_in_steps")
        self.teacher_forcing_prior = params.get("teacher_forcing_prior", False)
        self._init_loss_config(params)
        self.num_dims = _num_dims(params)
        # encoder(inputs) needs the model's plan.  Kept in the instance dictionary, not as a sub-module: parameters(),
        # state_dict() and .to() do not follow it, copy.deepcopy and pickle resolve the cycle to the copied model
        self.encoder.__dict__["_owner"] = self
        if device is not None:
            self.to(device)

    def save(self, path):
        torch.save(self.state_dict(), path)                       # as the reference's save / load

    def load(self, path):
        self.load_state_dict(torch.load(path))

    # -- plumbing of the fused step (aether._StepLoop) -----------------------------------------------------------------------
    def _field_hook(self):
        """The model has no field (``_FieldHook.no_field``): the hook names the entries and what follows num_edge_types in the
        plan calls.  Checks, once per call, that the tensors whose addresses go to the library are on the device."""
        for t in list(self.encoder.parameters()) + list(self.encoder.buffers()) + list(self.decoder.parameters()):
            if not t.is_cuda or (t.dtype.is_floating_point and not (t.dtype == torch.float32 and t.is_contiguous())):
                raise _lib.AetherHipError("DNRI parameters must be contiguous fp32 CUDA tensors: " + _CPU)
        return _FieldHook(None, [], entries=_ENTRIES, plan_tail=(1 if self.decoder.skip_first_edge_type else 0,), no_field=True)

    # -- the reference's methods ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def single_step_forward(self, inputs, decoder_hidden, edge_logits, hard_sample, uniform=None):
        """dnri.py:62-69: hard Gumbel sample of ``edge_logits`` [B, E, K] and the decoder step on it (``aether_s2s_dnri_step``
        with ext_logits: the prior is skipped).  ``uniform`` [B, E, K]: the U(0, 1) draw of ``gumbel_softmax`` (drawn on the
        device when omitted) -> (predictions, decoder_hidden, edges)."""
        if not hard_sample:
            raise _lib.AetherHipError("only hard_sample=True (evaluation / prediction) is part of this path")
        if not inputs.is_cuda:
            raise _lib.AetherHipError(_CPU)
        if uniform is None:
            uniform = torch.rand(edge_logits.shape, device=edge_logits.device)
        out, dh_out, _, edges = self._fused_step(inputs, decoder_hidden, None, uniform, logits=edge_logits)
        return out, dh_out, edges

    @torch.no_grad()
    def _encoder_forward(self, inputs, max_edges_per_call=400_000, field=None):
        """The full-sequence encoder (DNRI_Encoder.forward, dnri.py:371-401) in evaluation mode: inputs [B, T, N, 2D] ->
        (prior_logits, posterior_logits [B, T, E, K], prior_state).  The per-time-step features come from
        ``aether_s2s_dnri_encoder_features`` over chunks of T x B graphs, the recurrent half is the shared one
        (``Encoder._sequence_heads``).  ``field`` [T, B, N, D] (DNRIAether only, whose entry takes it behind the inputs): the
        field of the frames."""
        enc = self.encoder
        if enc.training:
            raise _lib.AetherHipError("the encoder uses BatchNorm running statistics: call .eval() first")
        if not inputs.is_cuda:
            raise _lib.AetherHipError(_CPU)
        lib = _lib.load()
        dev = inputs.device
        B, T, N, _ = inputs.shape
        D, he, hd, R, K = self._step_sizes()
        E1 = enc.recv_edges.shape[0]
        if inputs.shape[-1] != 2 * D or N != self.num_vars:
            raise ValueError("encoder: input shapes do not match the module")
        x = inputs.detach().to(torch.float32).transpose(0, 1).contiguous()                # [T, B, N, 2D]
        hook = self._field_hook()
        plan = self._plan(dev, hook)
        pe, n_layers, prior_hidden = enc._param_struct()
        pd = self.decoder._param_struct()
        feats = torch.empty(T, B * E1, he, dtype=torch.float32, device=dev)
        chunk = max(1, int(max_edges_per_call) // (B * E1))
        stream = torch.cuda.current_stream(dev).cuda_stream
        for t0 in range(0, T, chunk):
            t1 = min(T, t0 + chunk)
            G = (t1 - t0) * B
            send, recv, order, rowptr = enc._graph(G, N, dev)
            need = getattr(lib, self._entries(hook)[2])(D, he, hd, R, prior_hidden, K, G * N, G * E1)
            ws = enc._cache.get("ws_dnri")
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = enc._cache["ws_dnri"] = torch.empty(need, dtype=torch.uint8, device=dev)
            st = getattr(lib, self._features_entry)(
                *hook.field(), C.byref(pe), *hook.decoders(self.decoder, pd), plan.data_ptr(), D, he, hd, R, n_layers,
                prior_hidden, K, *hook.plan_tail, 0, N, G * N, G * E1, send.data_ptr(), recv.data_ptr(), order.data_ptr(),
                rowptr.data_ptr(), x[t0:t1].data_ptr(), *(() if field is None else (field[t0:t1].data_ptr(),)), ws.data_ptr(),
                ws.numel(), feats[t0:t1].data_ptr(), stream)
            _lib.check(st, self._features_entry)
        return enc._sequence_heads(feats, B)

    def _sequence_logits(self, inputs):
        """dnri.py:77: the full-sequence encoder; no field."""
        if not inputs.is_cuda:
            raise _lib.AetherHipError(_CPU)
        prior_logits, posterior_logits, _ = self._encoder_forward(inputs[:, :-1])
        return prior_logits, posterior_logits, None, None

    def _loss_step(self, inputs, decoder_hidden, logits, field, uniform):
        return self.single_step_forward(inputs, decoder_hidden, logits, True, uniform=uniform)

    @torch.no_grad()
    def predict_future(self, inputs, prediction_steps, return_edges=False, return_everything=False, uniform=None, graph=False):
        """dnri.py:111-136.  inputs [B, T, N, 2D] (burn-in observations); ``uniform`` [T - 1 + steps, B, E, K]: the Gumbel draws
        (drawn on the device when omitted).  ``return_everything``: the burn-in steps' predictions (and edges) in front of the
        predicted ones, as the reference.  ``graph``: the whole loop from ONE captured hipGraph; both ways run the same
        kernels and give identical results."""
        if not inputs.is_cuda:
            raise _lib.AetherHipError(_CPU)
        B, T, N, _ = inputs.shape
        E, R = N * (N - 1), self.encoder.rnn_hidden_size
        dev = inputs.device
        decoder_hidden = self.decoder.get_initial_hidden(inputs)
        prior_hidden = (torch.zeros(B, E, R, device=dev), torch.zeros(B, E, R, device=dev))
        steps = int(prediction_steps)
        if return_everything:
            return self._predict_everything(inputs, steps, decoder_hidden, prior_hidden, uniform, return_edges)
        burn = inputs[:, :T - 1].float() if T > 1 else None
        # (the burn-in half runs the same step: the forward LSTM and prior_fc_out are causal, :391, :398)
        run = self._graphed_rollout if graph else self._fused_rollout
        preds, edges, _ = run(burn, inputs[:, T - 1].float(), decoder_hidden, prior_hidden, steps, uniform, return_edges)
        return (preds, edges) if return_edges else preds

    def _predict_everything(self, inputs, steps, decoder_hidden, prior_hidden, uniform, return_edges):
        """``return_everything`` (:121-123): step by step, keeping what the burn-in steps predict."""
        B, T, N, _ = inputs.shape
        uniform = self._uniform(uniform, T - 1 + steps, B, N, inputs.device)
        preds, edges, x = [], [], None
        for t in range(T - 1 + steps):
            x_in = inputs[:, t].float() if t < T else x
            x, decoder_hidden, prior_hidden, z = self._fused_step(x_in, decoder_hidden, prior_hidden, uniform[t])
            preds.append(x)
            edges.append(z)
        preds = torch.stack(preds, 1)
        return (preds, torch.stack(edges, 1)) if return_edges else preds
