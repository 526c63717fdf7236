"""MI355X prediction path of the seq2seq LoCS baseline (``nn.seq2seq.locs.LoCS``).

The reference's baseline (nn/seq2seq/locs.py:13-208) is the seq2seq ``Aether`` without a field: the same encoder (edge filter,
``edge2node``, ``res1``, ``mlp3``, ``mlp4``, LSTM cell, ``prior_fc_out``), the same two decoders, Gumbel sample, globaliser and
residual, on the plain ``Localizer`` -- no virtual origin node, no force columns, 3D + O relative features per edge, a 2D-wide
``rel_feat`` and a 5D + O = 11 / 18 wide edge attribute.  Sub-modules carry the reference's names in its creation order
(``encoder``, ``decoder``), so a seeded construction gives its initial values and ``load_state_dict`` of a reference checkpoint
works (81 keys with the recurrent decoder, 56 with ``decoder_type='ref_mlp'`` at three prior layers).

The computation runs in libaether_hip.so on the fused step of ``Aether`` with the plain localizer in front
(``aether_s2s_locs_step`` / ``_rollout`` / ``_encoder_features``, csrc/s2s_locs.h): ``predict_future`` (eager or one captured
hipGraph), ``single_step_forward`` (the decoder on given logits) and ``calculate_loss(is_train=False)``.  No field query is
launched or allocated, and the anisotropic filter runs on 11 / 18 features.  Training is not part of this library, and there
is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from ... import _lib
from .aether import _EvalLoss, _FieldHook, _StepLoop
from .decoder import RecurrentDecoder
from .encoder import Encoder
from .markov import MarkovDecoder

_ENTRIES = ("aether_s2s_locs_plan_bytes", "aether_s2s_locs_plan_build", "aether_s2s_locs_workspace_bytes",
            "aether_s2s_locs_step", "aether_s2s_locs_rollout")
_CPU = "aether_amd seq2seq models run on an MI355X only; got a CPU tensor (there is no CPU fallback)"


class LoCS(_StepLoop, _EvalLoss, nn.Module):
    def __init__(self, params, device="cuda"):
        super().__init__()
        self.num_vars = params["num_vars"]
        self.encoder = Encoder(params, device=None, localizer="plain")           # creation order of locs.py:19-24
        self._markov = params.get("decoder_type", None) == "ref_mlp"
        self.decoder = (MarkovDecoder if self._markov else RecurrentDecoder)(params, device=None, localizer="plain")
        self.num_edge_types = params.get("num_edge_types")
        # training parameters the runner's scripts read or set (locs.py:28-44); only evaluation runs here
        self.gumbel_temp = params.get("gumbel_temp")
        self.train_hard_sample = params.get("train_hard_sample")
        self.teacher_forcing_steps = params.get("teacher_forcing_steps", -1)
        self.kl_coef = params.get("kl_coef", 1.)
        self.timesteps = params.get("timesteps", 0)
        self.burn_in_steps = params.get("train_burn_in_steps")
        self.teacher_forcing_prior = params.get("teacher_forcing_prior", False)
        self.train_percent = 0.0                                       # (experiments/electrostatic/train.py:81 sets it per epoch)
        self._init_loss_config(params)
        self.use_3d = params.get("use_3d", False)
        self.num_dims = 3 if self.use_3d else 2
        if device is not None:
            self.to(device)

    def save(self, path):
        torch.save(self.state_dict(), path)                       # as the reference's save / load

    def load(self, path):
        self.load_state_dict(torch.load(path))

    # -- plumbing of the fused step (aether._StepLoop) -----------------------------------------------------------------------
    def _field_hook(self):
        """The model has no field (``_FieldHook.no_field``): the hook names the entries and what follows num_edge_types in the
        plan calls; the shared step, rollout and plan code of ``_StepLoop`` does the rest.  Checks, once per call, that the
        tensors whose addresses go to the library are on the device."""
        for t in list(self.encoder.parameters()) + list(self.encoder.buffers()) + list(self.decoder.parameters()):
            if not t.is_cuda or (t.dtype.is_floating_point and not (t.dtype == torch.float32 and t.is_contiguous())):
                raise _lib.AetherHipError("LoCS parameters must be contiguous fp32 CUDA tensors: " + _CPU)
        return _FieldHook(None, [], entries=_ENTRIES, plan_tail=(1 if self.decoder.skip_first_edge_type else 0,), no_field=True)

    # -- the reference's methods ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def single_step_forward(self, inputs, decoder_hidden, edge_logits, hard_sample, uniform=None):
        """locs.py:69-77: hard Gumbel sample of ``edge_logits`` [B, E, K] and the decoder step on it (``aether_s2s_locs_step``
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
    def _encoder_forward(self, inputs, max_edges_per_call=400_000):
        """The full-sequence encoder (Encoder.forward, locs.py:309-339) in evaluation mode: inputs [B, T, N, 2D] ->
        (prior_logits, posterior_logits [B, T, E, K], prior_state).  The per-time-step features come from
        ``aether_s2s_locs_encoder_features`` over chunks of T x B graphs, the recurrent half is the shared one
        (``Encoder._sequence_heads``)."""
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
        pe, n_layers, prior_hidden = enc._param_struct(with_image=False)
        pd = self.decoder._param_struct()
        feats = torch.empty(T, B * E1, he, dtype=torch.float32, device=dev)
        chunk = max(1, int(max_edges_per_call) // (B * E1))
        stream = torch.cuda.current_stream(dev).cuda_stream
        for t0 in range(0, T, chunk):
            t1 = min(T, t0 + chunk)
            G = (t1 - t0) * B
            send, recv, order, rowptr = enc._graph(G, N, dev)
            need = lib.aether_s2s_locs_workspace_bytes(D, he, hd, R, prior_hidden, K, G * N, G * E1)
            ws = enc._cache.get("ws_locs")
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = enc._cache["ws_locs"] = torch.empty(need, dtype=torch.uint8, device=dev)
            st = lib.aether_s2s_locs_encoder_features(
                C.byref(pe), *hook.decoders(self.decoder, pd), plan.data_ptr(), D, he, hd, R, n_layers, prior_hidden, K,
                *hook.plan_tail, 1 if enc.pos_representation == "polar" else 0, N, G * N, G * E1, send.data_ptr(),
                recv.data_ptr(), order.data_ptr(), rowptr.data_ptr(), x[t0:t1].data_ptr(), ws.data_ptr(), ws.numel(),
                feats[t0:t1].data_ptr(), stream)
            _lib.check(st, "aether_s2s_locs_encoder_features")
        return enc._sequence_heads(feats, B)

    def _sequence_logits(self, inputs):
        """locs.py:87: the full-sequence encoder; no field."""
        if not inputs.is_cuda:
            raise _lib.AetherHipError(_CPU)
        prior_logits, posterior_logits, _ = self._encoder_forward(inputs[:, :-1])
        return prior_logits, posterior_logits, None, None

    def _loss_step(self, inputs, decoder_hidden, logits, field, uniform):
        return self.single_step_forward(inputs, decoder_hidden, logits, True, uniform=uniform)

    @torch.no_grad()
    def predict_future(self, inputs, prediction_steps, return_edges=False, return_everything=False, uniform=None, graph=False):
        """locs.py:122-151.  inputs [B, T, N, 2D] (burn-in observations); ``uniform`` [T - 1 + steps, B, E, K]: the Gumbel draws
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
        # (the burn-in half runs the same step: the encoder's prior path is causal, as for Aether.predict_future)
        run = self._graphed_rollout if graph else self._fused_rollout
        preds, edges, _ = run(burn, inputs[:, T - 1].float(), decoder_hidden, prior_hidden, steps, uniform, return_edges)
        return (preds, edges) if return_edges else preds

    def _predict_everything(self, inputs, steps, decoder_hidden, prior_hidden, uniform, return_edges):
        """``return_everything`` (:134-136): step by step, keeping what the burn-in steps predict."""
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
