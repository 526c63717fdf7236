"""MI355X prediction path of the seq2seq ablation ``nn.seq2seq.ablations.dnri_aether.DNRIAether``: dNRI with the latent field,
without the equivariant frames.

The reference's model (nn/seq2seq/ablations/dnri_aether.py:11-678) is ``DNRI`` whose encoder and decoders also read the field
``Aether`` discovers: ``predict_field`` (:81-85) is ``field_net`` on random Fourier features of the position, and
``[inputs | field]`` (3D columns) takes the place of the raw state in ``mlp1`` of the encoder (:320, :416, :446), in
``input_r / _i / _n`` of ``DNRI_Decoder`` (:498-500, :564-569) and in ``msg_fc1`` / ``out_fc1`` of ``DNRI_MLP_Decoder`` (:601, :608,
:632-636).  Both decoders return ``inputs + prediction`` on the 2D-wide state.  Sub-modules carry the reference's names in its
creation order (encoder, decoder, field net, Fourier features), so a seeded construction gives its initial values and
``load_state_dict`` of a reference checkpoint works (88 keys with the recurrent decoder, 79 with the MLP decoder at three prior
layers).

The computation runs in libaether_hip.so (``aether_s2s_dnri_aether_*``, csrc/s2s_dnri_aether.h) on the dNRI engine with the
field query in front: ``predict_future`` (eager or one captured hipGraph), ``single_step_forward`` (the decoder on given logits
and a given field), ``calculate_loss(is_train=False)`` and the full-sequence ``encoder(inputs, predicted_field)``.  Training and
``predict_future_fixedwindow`` are not part of this library, and there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import torch

from .... import _lib
from ..aether import _EvalLoss, _FieldHook
from ..dnri import _CPU, DNRI
from ..dnri import DNRI_Decoder as _PlainDecoder
from ..dnri import DNRI_Encoder as _PlainEncoder
from ..dnri import DNRI_MLP_Decoder as _PlainMlpDecoder
from ..field import FieldQuery, _S2SFieldParams

_ENTRIES = ("aether_s2s_dnri_aether_plan_bytes", "aether_s2s_dnri_aether_plan_build", "aether_s2s_dnri_aether_workspace_bytes",
            "aether_s2s_dnri_aether_step", "aether_s2s_dnri_aether_rollout")
_THROUGH_MODEL = ("of the seq2seq DNRIAether runs through the model (DNRIAether.single_step_forward, DNRIAether.predict_future, "
                  "DNRIAether.encoder: aether_s2s_dnri_aether_*), not as a call of the module")


def _field_cols(params):
    """The field's columns behind the raw state: num_dims as the reference reads it (dnri_aether.py:318-319)."""
    D = 3 if params.get("use_3d", False) else 2
    if params["input_size"] != 2 * D:
        raise ValueError("input_size must be 4 without use_3d (2-D positions and velocities) and 6 with it")
    return D


class DNRI_Encoder(_PlainEncoder):
    """Parameter holder of the ablation's ``DNRI_Encoder`` (dnri_aether.py:298-370): dNRI's, ``mlp1`` on 3D columns."""
    _field_cols = staticmethod(_field_cols)

    def forward(self, inputs, predicted_field):
        """dnri_aether.py:409-441 in evaluation mode: inputs [B, T, N, 2D], predicted_field [B, N, T, D] -> (prior_logits,
        posterior_logits [B, T, E, K], prior_state (h, c) each [B, E, rnn])."""
        model = self.__dict__.get("_owner")
        if model is None:
            raise _lib.AetherHipError("DNRI_Encoder.forward " + _THROUGH_MODEL)
        return model._encoder_forward(inputs, predicted_field)

    def single_step_forward(self, inputs, prior_state, predicted_field):
        raise _lib.AetherHipError("DNRI_Encoder.single_step_forward " + _THROUGH_MODEL)


class DNRI_Decoder(_PlainDecoder):
    """Parameter holder of the ablation's ``DNRI_Decoder`` (dnri_aether.py:470-514): ``input_r / _i / _n`` on 3D columns."""
    _field_cols = staticmethod(_field_cols)

    def forward(self, inputs, hidden, edges, predicted_field):
        raise _lib.AetherHipError("the decoder step " + _THROUGH_MODEL)


class DNRI_MLP_Decoder(_PlainMlpDecoder):
    """Parameter holder of the ablation's ``DNRI_MLP_Decoder`` (dnri_aether.py:585-619): ``msg_fc1`` on 6D, ``out_fc1`` on
    3D + hidden columns."""
    _field_cols = staticmethod(_field_cols)

    def forward(self, inputs, hidden, edges, predicted_field):
        raise _lib.AetherHipError("the decoder step " + _THROUGH_MODEL)


class DNRIAether(DNRI):
    _encoder_class, _decoder_classes = DNRI_Encoder, (DNRI_Decoder, DNRI_MLP_Decoder)
    _features_entry = "aether_s2s_dnri_aether_encoder_features"

    def __init__(self, params, device="cuda"):
        super().__init__(params, device=None)                              # encoder, decoder (dnri_aether.py:15-21)
        self.use_3d = params.get("use_3d", False)
        if self.num_dims != (3 if self.use_3d else 2):
            raise ValueError("input_size must be 4 without use_3d (2-D positions and velocities) and 6 with it")
        fq = FieldQuery(self.num_dims, params["encoder_hidden"], params.get("rff_std", 1.0), device=None)      # :67-79
        self.field_net, self.coordinate_embedding = fq.field_net, fq.coordinate_embedding
        self._fq = [fq]                                                    # not a registered sub-module: no duplicate keys
        self._burn_field = None
        if device is not None:
            self.to(device)

    # -- plumbing of the fused step (aether._StepLoop) -----------------------------------------------------------------------
    def _field_hook(self):
        """The step's built-in field query is the plain field net (``aether_s2s_dnri_aether_*`` take its struct in front); the
        rollout is handed the burn-in frames' field, queried in one batch.  Checks, once per call, that the tensors whose
        addresses go to the library are on the device."""
        fn, ce = self.field_net, self.coordinate_embedding
        field = [ce.B] + list(fn.parameters())
        for t in list(self.encoder.parameters()) + list(self.encoder.buffers()) + list(self.decoder.parameters()) + field:
            if not t.is_cuda or (t.dtype.is_floating_point and not (t.dtype == torch.float32 and t.is_contiguous())):
                raise _lib.AetherHipError("DNRIAether parameters must be contiguous fp32 CUDA tensors: " + _CPU)
        pf = _S2SFieldParams(*[t.data_ptr() for t in (ce.B, fn[0].weight, fn[0].bias, fn[2].weight, fn[2].bias, fn[4].weight,
                                                      fn[4].bias)])

        def burn_field(burn_in):
            """The field of the burn-in frames [T0, B, N, 2D] -> [T0, B, N, D] in one batched query (dnri_aether.py:148-149):
            they are known before the loop starts; only the predicted steps query theirs inside the step."""
            if burn_in is None:
                return (None,)
            self._burn_field = field = self.predict_field(burn_in)[0].contiguous()     # (kept: the call that reads it comes next)
            return (field.data_ptr(),)

        return _FieldHook(pf, field, entries=_ENTRIES, plan_tail=(1 if self.decoder.skip_first_edge_type else 0,),
                          burn_field=burn_field)

    def _graph_keepalive(self):
        return super()._graph_keepalive() + [self._burn_field]

    @torch.no_grad()
    def _fused_step(self, x, decoder_hidden, prior_hidden, uniform, field=None, return_field=False, logits=None,
                    return_logits=False):
        """One autoregressive step (``aether_s2s_dnri_aether_step``): x [B, N, 2D], decoder_hidden [B, N, hd] (ignored and None
        with the MLP decoder), prior_hidden (h, c) [B, E, rnn], uniform [B, E, K] -> (predictions, decoder_hidden, (h, c),
        edges).  ``field`` [B, N, D] replaces the built-in field query (no field launch is made); ``logits`` [B, E, K] makes the
        step the decoder on given logits -- the prior is skipped, ``prior_hidden`` is not read and comes back as None.
        ``return_field`` / ``return_logits``: also the field the step used / the prior's logits the sample was taken from, in
        that order."""
        if not x.is_cuda:
            raise _lib.AetherHipError(_CPU)
        if logits is not None and return_logits:
            raise _lib.AetherHipError("logits / return_logits: the step takes given logits or returns the prior's, not both")
        B, N, _ = x.shape
        dev = x.device
        lib, plan, ws, (send, recv, order, rowptr), (pf, pe, pd), scal, hook = self._step_common(B, N, dev)
        D, he, hd, R, K = self._step_sizes()
        E1 = self.encoder.recv_edges.shape[0]
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        opt = lambda t: None if t is None else t.data_ptr()
        xf, uf = f32(x), f32(uniform)
        dhf = f32(decoder_hidden) if self.decoder._has_state else None
        ff = None if field is None else f32(field)
        lg = None if logits is None else f32(logits)
        h0 = c0 = h1 = c1 = None
        if lg is None:
            h0, c0 = f32(prior_hidden[0]), f32(prior_hidden[1])
            h1, c1 = torch.empty_like(h0), torch.empty_like(c0)
        if xf.shape != (B, N, 2 * D) or (dhf is not None and dhf.shape != (B, N, hd)) or uf.numel() != B * E1 * K or \
                (lg is None and (h0.shape != (B, E1, R) or c0.shape != h0.shape)) or \
                (lg is not None and lg.shape != (B, E1, K)) or (ff is not None and ff.shape != (B, N, D)):
            raise ValueError("fused step: input shapes do not match the model")
        out = torch.empty_like(xf)
        dh_out = None if dhf is None else torch.empty_like(dhf)
        edges = torch.empty(B, E1, K, dtype=torch.float32, device=dev)
        fout = torch.empty(B, N, D, dtype=torch.float32, device=dev) if return_field else None
        lout = torch.empty(B, E1, K, dtype=torch.float32, device=dev) if return_logits else None
        st = lib.aether_s2s_dnri_aether_step(
            C.byref(pf), C.byref(pe), *hook.decoders(self.decoder, pd), plan.data_ptr(), *scal, send.data_ptr(), recv.data_ptr(),
            order.data_ptr(), rowptr.data_ptr(), xf.data_ptr(), opt(ff), opt(lg), opt(dhf), opt(h0), opt(c0), uf.data_ptr(),
            ws.data_ptr(), ws.numel(), out.data_ptr(), opt(dh_out), opt(h1), opt(c1), edges.data_ptr(), opt(lout), opt(fout),
            torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(st, "aether_s2s_dnri_aether_step")
        res = (out, dh_out, None if lg is not None else (h1, c1), edges)
        return res + ((fout,) if return_field else ()) + ((lout,) if return_logits else ())

    # -- the reference's methods ----------------------------------------------------------------------------------------------
    def predict_field(self, x):
        """dnri_aether.py:81-85: x [..., >= D] -> (field [..., D], coords)."""
        return self._fq[0](x)

    @torch.no_grad()
    def single_step_forward(self, inputs, decoder_hidden, edge_logits, hard_sample, predicted_field, uniform=None):
        """dnri_aether.py:87-94: hard Gumbel sample of ``edge_logits`` [B, E, K] and the decoder step on it and on
        ``predicted_field`` [B, N, D] (``aether_s2s_dnri_aether_step`` with ext_logits and ext_field: neither the prior nor the
        field query runs).  ``uniform`` [B, E, K]: the U(0, 1) draw of ``gumbel_softmax`` (drawn on the device when omitted)
        -> (predictions, decoder_hidden, edges)."""
        if not hard_sample:
            raise _lib.AetherHipError("only hard_sample=True (evaluation / prediction) is part of this path")
        if not inputs.is_cuda:
            raise _lib.AetherHipError(_CPU)
        if uniform is None:
            uniform = torch.rand(edge_logits.shape, device=edge_logits.device)
        out, dh_out, _, edges = self._fused_step(inputs, decoder_hidden, None, uniform, field=predicted_field, logits=edge_logits)
        return out, dh_out, edges

    @torch.no_grad()
    def _encoder_forward(self, inputs, predicted_field, max_edges_per_call=400_000):
        """The full-sequence encoder (dnri_aether.py:409-441): inputs [B, T, N, 2D], predicted_field [B, N, T, D]."""
        B, T, N, _ = inputs.shape
        if not inputs.is_cuda or not predicted_field.is_cuda:
            raise _lib.AetherHipError(_CPU)
        if predicted_field.shape != (B, N, T, self.num_dims):
            raise ValueError("encoder: predicted_field must be [B, N, T, D]")
        f = predicted_field.detach().to(torch.float32).permute(2, 0, 1, 3).contiguous()   # [T, B, N, D]
        return super()._encoder_forward(inputs, max_edges_per_call, field=f)

    # (the evaluation loss of a model with a field: the field of the observed frames in one query, the encoder and every
    # decoder step are handed theirs, dnri_aether.py:102-122)
    _sequence_logits = _EvalLoss._sequence_logits
    _loss_step = _EvalLoss._loss_step

    def _sequence_field(self, inputs):
        if not inputs.is_cuda:
            raise _lib.AetherHipError(_CPU)
        return super()._sequence_field(inputs)

    def _predict_everything(self, inputs, steps, decoder_hidden, prior_hidden, uniform, return_edges):
        """``return_everything`` (:152-153): step by step, keeping what the burn-in steps predict.  As in the rollout, the
        burn-in frames' field comes from one batched query and the later steps query theirs."""
        B, T, N, _ = inputs.shape
        uniform = self._uniform(uniform, T - 1 + steps, B, N, inputs.device)
        burn_field = self.predict_field(inputs[:, :T - 1].float().transpose(0, 1).contiguous())[0] if T > 1 else None
        preds, edges, x = [], [], None
        for t in range(T - 1 + steps):
            x_in = inputs[:, t].float() if t < T else x
            field = burn_field[t] if t < T - 1 else None                   # [T - 1, B, N, D], the rollout's layout
            x, decoder_hidden, prior_hidden, z = self._fused_step(x_in, decoder_hidden, prior_hidden, uniform[t], field=field)
            preds.append(x)
            edges.append(z)
        preds = torch.stack(preds, 1)
        return (preds, torch.stack(edges, 1)) if return_edges else preds
