"""MI355X Markov decoder step of the seq2seq Aether (``decoder_type='ref_mlp'``).

Mirrors ``nn.seq2seq.aether.MarkovDecoder`` of the reference (aether.py:413-503, with ``MLPEdgeFilter`` of
nn/nn/anisotropic_filter.py:43-71): same ``params`` dictionary, parameters created in the same order with the same
shapes and the same re-initialisation of the edge filter (so the same torch seed gives the same initial weights and
``state_dict`` keys / order match a reference checkpoint), ``get_initial_hidden`` returning None and
``forward(inputs, hidden, edges, predicted_field) -> (outputs, None)``.  The computation runs in libaether_hip.so
(``aether_s2s_markov_decoder_step``); there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from ... import _lib
from .decoder import RecurrentDecoder
from .localizer import AugmentedLocalizer, Localizer


_MarkovParams = _lib.AetherS2SMarkovParams


class MLPEdgeFilter(nn.Module):
    """anisotropic_filter.py:43-71: relu(lin2(relu(lin1(edge_attr)))); output column c * Ku + k is channel c of used
    edge type k.  Holds the parameters only: MarkovDecoder.forward runs it inside the decoder step."""

    def __init__(self, in_size, hidden_size, out_size):
        super().__init__()
        self.lin1 = nn.Linear(in_size, hidden_size)
        self.lin2 = nn.Linear(hidden_size, out_size)
        for m in self.modules():                                   # init_weights (:56-63)
            if isinstance(m, nn.Linear):
                nn.init.xavier_normal_(m.weight.data)
                m.bias.data.fill_(0.1)


class MarkovDecoder(nn.Module):
    def __init__(self, params, device="cuda", localizer="augmented"):
        """``localizer='plain'``: the Markov decoder of the seq2seq LoCS (nn/seq2seq/locs.py:368-420) -- the plain ``Localizer``
        with ``params['pos_representation']``, 3D + O relative features, ``res1`` on the 2D-wide ``rel_feat`` created where
        the reference creates it (in front of ``out_mlp``).  Its step runs through the model (``aether_s2s_locs_step``):
        ``forward`` of the module raises."""
        super().__init__()
        if localizer not in ("augmented", "plain"):
            raise ValueError("localizer must be 'augmented' or 'plain'")
        self.localizer_kind = localizer
        plain = localizer == "plain"
        self.num_vars = params["num_vars"]
        self.edge_types = params["num_edge_types"]
        n_hid = params["decoder_hidden"]
        in_size = params["input_size"]
        self.skip_first_edge_type = params["skip_first"]
        self.dropout_prob = params["decoder_dropout"]
        if self.dropout_prob != 0.0:
            raise ValueError("decoder_dropout must be 0.0 (inference path; the reference zeroes it in eval)")
        self.num_used_edge_types = self.edge_types - 1 if self.skip_first_edge_type else self.edge_types
        if self.num_used_edge_types < 1:
            raise ValueError("the Markov decoder needs at least one used edge type (num_edge_types - skip_first >= 1)")
        if n_hid % 32 != 0:
            raise ValueError("decoder_hidden must be a multiple of 32")
        self.msg_out_shape = n_hid
        self.use_3d = params.get("use_3d", False)
        self.num_dims = D = 3 if self.use_3d else 2
        self.num_orientations = D * (D - 1) // 2
        self.num_relative_features = nrf = (3 if plain else 4) * D + self.num_orientations
        self.num_pos_features = D + self.num_orientations
        # creation order = the reference's (aether.py:426-453; locs.py:383-419): identical RNG consumption under a seed
        if plain:
            self.res1 = nn.Linear(in_size, n_hid)
        self.out_mlp = nn.Sequential(nn.Linear(n_hid, n_hid), nn.ReLU(), nn.Dropout(p=self.dropout_prob),
                                     nn.Linear(n_hid, n_hid), nn.ReLU(), nn.Dropout(p=self.dropout_prob),
                                     nn.Linear(n_hid, in_size))
        if plain:
            self.edge_filter = MLPEdgeFilter(nrf + in_size, n_hid, n_hid * self.num_used_edge_types)
            self.localizer = Localizer(self.num_vars, use_3d=self.use_3d, pos_representation=params["pos_representation"])
        else:
            self.res1 = nn.Linear(in_size + nrf + D, n_hid)
            self.edge_filter = MLPEdgeFilter(2 * nrf + in_size + D, n_hid, n_hid * self.num_used_edge_types)
            self.localizer = AugmentedLocalizer(self.num_vars, use_3d=self.use_3d, pos_representation="polar")
        self.send_edges, self.recv_edges = torch.where(~torch.eye(self.num_vars, dtype=bool))
        self._cache = {}
        if device is not None:
            self.to(device)

    _graph = RecurrentDecoder._graph

    # (as RecurrentDecoder's)
    _fused_entries = ("aether_s2s_markov_plan_bytes", "aether_s2s_markov_plan_build", "aether_s2s_markov_step",
                      "aether_s2s_markov_rollout")
    _has_state = False

    def _plan_extra(self):
        return (1 if self.skip_first_edge_type else 0,)

    def get_initial_hidden(self, inputs):
        return None

    def _param_struct(self):
        ef, om = self.edge_filter, self.out_mlp
        return _MarkovParams(*[t.data_ptr() for t in (ef.lin1.weight, ef.lin1.bias, ef.lin2.weight, ef.lin2.bias,
                                                      self.res1.weight, self.res1.bias, om[0].weight, om[0].bias,
                                                      om[3].weight, om[3].bias, om[6].weight, om[6].bias)])

    @torch.no_grad()
    def forward(self, inputs, hidden, edges, predicted_field):
        """aether.py:459-503.  inputs [B, N, 2D], edges [B, N(N-1), K] (one-hot or soft), predicted_field [B, N, D]
        -> (outputs [B, N, 2D], None).  ``hidden`` is ignored (the decoder has no state)."""
        if self.localizer_kind == "plain":
            raise _lib.AetherHipError("the decoder step of the seq2seq LoCS runs through the model (LoCS.single_step_forward: "
                                      "aether_s2s_locs_step), not as a call of the module")
        if not inputs.is_cuda:
            raise _lib.AetherHipError("aether_amd MarkovDecoder runs on an MI355X only; got a CPU tensor "
                                      "(there is no CPU fallback)")
        lib = _lib.load()
        B, N, F_in = inputs.shape
        D, h, K = self.num_dims, self.msg_out_shape, self.edge_types
        E1 = self.recv_edges.shape[0]
        if F_in != 2 * D or edges.shape != (B, E1, K) or predicted_field.shape != (B, N, D):
            raise ValueError("Markov decoder step: input shapes do not match the module")
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        inputs_f, edges_f, field_f = f32(inputs), f32(edges), f32(predicted_field)
        send, recv, order, rowptr = self._graph(B, N, inputs.device)
        need = lib.aether_s2s_markov_decoder_workspace_bytes(D, h, B * N, B * E1)
        ws = self._cache.get("ws")
        if ws is None or ws.numel() < need or ws.device != inputs.device:
            ws = self._cache["ws"] = torch.empty(need, dtype=torch.uint8, device=inputs.device)
        outputs = torch.empty(B, N, 2 * D, dtype=torch.float32, device=inputs.device)
        ps = self._param_struct()
        st = lib.aether_s2s_markov_decoder_step(C.byref(ps), D, h, K, 1 if self.skip_first_edge_type else 0, B * N, B * E1,
                                                inputs_f.data_ptr(), edges_f.data_ptr(), field_f.data_ptr(),
                                                send.data_ptr(), recv.data_ptr(), order.data_ptr(), rowptr.data_ptr(),
                                                ws.data_ptr(), ws.numel(), outputs.data_ptr(),
                                                torch.cuda.current_stream(inputs.device).cuda_stream)
        _lib.check(st, "aether_s2s_markov_decoder_step")
        return outputs, None
