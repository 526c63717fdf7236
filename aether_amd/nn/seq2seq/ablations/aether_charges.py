"""MI355X prediction path of the charge-aware seq2seq Aether (``nn.seq2seq.ablations.aether_charges.AetherCharges``).

The reference's ablation (ablations/aether_charges.py:14-266) is the seq2seq ``Aether`` whose field query, encoder and
recurrent decoder also see a 16-wide ``nn.Embedding(2, 16)`` of every particle's charge sign -- the one model of the
electrostatic runner that the charges reach (experiments/electrostatic/train.py:96 passes ``charges=`` when
``calculate_loss`` names it).  Sub-modules carry the reference's names in its creation order -- ``encoder``, ``decoder``,
``field_net``, ``coordinate_embedding``, ``charge_embedding`` -- so a seeded construction gives its initial values and
``load_state_dict`` of a reference checkpoint works.

The embedding has two rows, so the library never multiplies by it: ``aether_s2s_charges_plan_build`` folds it into bias
tables (2 rows per node layer, 4 per edge layer) and into four one-hot features of the anisotropic filter, and the step
(``aether_s2s_charges_step`` / ``_rollout``, the fused step of ``Aether`` with a charge index per node) costs the plain
model's plus the four extra filter features.  Here: ``predict_field``, ``predict_future`` (eager or one captured hipGraph), the
fused step, ``single_step_forward`` (the decoder on given logits) and ``calculate_loss(is_train=False)`` with the charge-aware
full-sequence encoder (``aether_s2s_charges_encoder_features``); training is not part of this library.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from .... import _lib
from ..aether import _EvalLoss, _FieldHook, _StepLoop
from ..decoder import RecurrentDecoder
from ..encoder import Encoder
from ..field import FieldQuery, _S2SFieldParams

CHARGE_EMBEDDING_DIM = 16                                          # aether_charges.py:72

_ENTRIES = ("aether_s2s_charges_plan_bytes", "aether_s2s_charges_plan_build", "aether_s2s_charges_workspace_bytes",
            "aether_s2s_charges_step", "aether_s2s_charges_rollout")


class AetherCharges(_StepLoop, _EvalLoss, nn.Module):
    def __init__(self, params, device="cuda"):
        super().__init__()
        if params.get("decoder_type", None) == "ref_mlp":
            raise ValueError("AetherCharges: decoder_type 'ref_mlp' (the Markov decoder) is not part of the charge-aware "
                             "model here; the reference's scripts all use the recurrent decoder")
        ce = CHARGE_EMBEDDING_DIM
        self.num_vars = params["num_vars"]
        self.encoder = Encoder(params, device=None, charge_dim=ce)           # creation order of aether_charges.py:20-25,71-86
        self.decoder = RecurrentDecoder(params, device=None, charge_dim=ce)
        self.num_edge_types = params.get("num_edge_types")
        self.gumbel_temp = params.get("gumbel_temp")
        self.kl_coef = params.get("kl_coef", 1.)
        self._init_loss_config(params)
        self.use_3d = params.get("use_3d", False)
        self.num_dims = 3 if self.use_3d else 2
        fq = FieldQuery(self.num_dims, params["encoder_hidden"], params.get("rff_std", 1.0), device=None, charge_dim=ce)
        self.field_net, self.coordinate_embedding = fq.field_net, fq.coordinate_embedding
        self.charge_embedding = nn.Embedding(2, ce)
        self._fq = [fq]                                                    # not a registered sub-module: no duplicate keys
        self._cidx = None                                                  # int32 [B * N]: the charge index the step reads
        if device is not None:
            self.to(device)

    def save(self, path):
        torch.save(self.state_dict(), path)                       # as the reference's save / load

    def load(self, path):
        self.load_state_dict(torch.load(path))

    @staticmethod
    def charge_to_index(charges):
        return ((charges + 1) / 2).long()                         # aether_charges.py:100-102

    # -- the charge index ---------------------------------------------------------------------------------------------------
    def _index_of(self, charge_emb):
        """The table row of every item of ``charge_emb``: an integer tensor is the index itself; a float tensor [..., 16] is
        what ``charge_embedding(index)`` returned (the reference's argument) and is matched against the two rows -- a row that
        is neither gets index 2, which the library answers with NaN and its asynchronous error."""
        if not charge_emb.is_floating_point():
            return charge_emb.to(torch.int32)
        w = self.charge_embedding.weight.detach()
        if charge_emb.shape[-1] != w.shape[1]:
            raise ValueError("charge_emb must be charge_embedding(index) [..., 16] or the index itself")
        is0, is1 = (charge_emb == w[0]).all(-1), (charge_emb == w[1]).all(-1)
        two = torch.full(is0.shape, 2, dtype=torch.int32, device=charge_emb.device)
        return torch.where(is1, torch.ones_like(two), torch.where(is0, torch.zeros_like(two), two))

    def _set_charges(self, index, B, N, device):
        """Copies the index [B, N] into the static buffer the step entries (and the graphs captured around them) read."""
        buf = self._cidx
        if buf is None or buf.numel() != B * N or buf.device != torch.device(device):
            buf = self._cidx = torch.zeros(B * N, dtype=torch.int32, device=device)
        buf.copy_(index.reshape(-1).to(device=device, dtype=torch.int32))
        return buf

    def _charges_arg(self, charges, B, N, device):
        if charges is None:
            raise ValueError("AetherCharges needs the particles' charges: pass charges=[B, >= num_objects] (+-1)")
        if not charges.is_cuda:
            raise _lib.AetherHipError("aether_amd seq2seq models run on an MI355X only; got a CPU tensor (there is no CPU fallback)")
        if charges.dim() != 2 or charges.shape[0] != B or charges.shape[1] < N:
            raise ValueError("charges must be [B, >= num_objects]")
        return self._set_charges(self.charge_to_index(charges[:, :N]), B, N, device)      # charges[:, :num_objects], :127

    # -- plumbing of the fused step (aether._StepLoop) -----------------------------------------------------------------------
    def _field_struct_checked(self):
        fn, ce = self.field_net, self.coordinate_embedding
        tensors = [ce.B, fn[0].weight, fn[0].bias, fn[2].weight, fn[2].bias, fn[4].weight, fn[4].bias,
                   self.charge_embedding.weight]
        for t in tensors:
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise _lib.AetherHipError("AetherCharges parameters must be contiguous fp32 CUDA tensors")
        return _S2SFieldParams(*[t.data_ptr() for t in tensors[:7]])

    def _field_hook(self):
        pf = self._field_struct_checked()
        cidx = self._cidx
        return _FieldHook(pf, list(self.field_net.parameters()) + [self.charge_embedding.weight], names=_ENTRIES,
                          plan_head=(self.charge_embedding.weight.data_ptr(),),
                          call=lambda B, N: (self._checked_cidx(cidx, B, N),), after_field=(None,))

    @staticmethod
    def _checked_cidx(cidx, B, N):
        if cidx is None or cidx.numel() != B * N:
            raise _lib.AetherHipError("AetherCharges: no charge index for this batch (call through predict_future, or "
                                      "_set_charges first)")
        return cidx.data_ptr()

    def _graph_keepalive(self):
        return super()._graph_keepalive() + [self._cidx]

    # -- the reference's methods ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def predict_field(self, x, charge_emb):
        """aether_charges.py:88-98.  x [B, N, >= D] or [B, N, T, >= D]; charge_emb [B, N, 16] (``charge_embedding(index)``) or
        the index [B, N] -> (field [..., D], coords)."""
        if not x.is_cuda:
            raise _lib.AetherHipError("aether_amd seq2seq models run on an MI355X only; got a CPU tensor (there is no CPU fallback)")
        D, he = self.num_dims, self.encoder.hidden_size
        idx = self._index_of(charge_emb)
        if x.ndim == 4:
            idx = idx.unsqueeze(2).expand(x.shape[:3])            # the embedding repeated over time, :89-90
        if x.shape[-1] < D or tuple(idx.shape) != tuple(x.shape[:-1]):
            raise ValueError("predict_field: x [..., >= D] and one charge per leading index")
        coords = x[..., :D]
        pts = x.detach().to(torch.float32).reshape(-1, x.shape[-1]).contiguous()
        ci = idx.reshape(-1).to(torch.int32).contiguous()
        n = pts.shape[0]
        out = torch.empty(n, D, dtype=torch.float32, device=x.device)
        if n == 0:
            return out.reshape(*x.shape[:-1], D), coords
        lib = _lib.load()
        hook = self._field_hook()
        plan = self._plan(x.device, hook)
        need = lib.aether_s2s_charges_field_workspace_bytes(n, he)
        fq = self._fq[0]
        if fq._ws is None or fq._ws.numel() < need or fq._ws.device != x.device:
            fq._ws = torch.empty(need, dtype=torch.uint8, device=x.device)
        _, hd, R = self._step_sizes()[1:4]
        _, n_layers, prior_hidden = self.encoder._param_struct(with_image=False)
        st = lib.aether_s2s_charges_field(C.byref(hook.struct), plan.data_ptr(), D, he, hd, R, n_layers, prior_hidden,
                                          self.num_edge_types, n, pts.data_ptr(), pts.shape[1], ci.data_ptr(), fq._ws.data_ptr(),
                                          fq._ws.numel(), out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream)
        _lib.check(st, "aether_s2s_charges_field")
        return out.reshape(*x.shape[:-1], D), coords

    @torch.no_grad()
    def single_step_forward(self, inputs, decoder_hidden, edge_logits, hard_sample, predicted_field, charge_emb, uniform=None):
        """aether_charges.py:104-113: hard Gumbel sample of ``edge_logits`` [B, E, K] and the decoder step on it
        (``aether_s2s_charges_step`` with ext_logits: the prior is skipped).  ``charge_emb``: ``charge_embedding(index)`` or the
        index; ``uniform`` [B, E, K]: the U(0, 1) draw (drawn on the device when omitted)
        -> (predictions, decoder_hidden, edges)."""
        if not hard_sample:
            raise _lib.AetherHipError("only hard_sample=True (evaluation / prediction) is part of this path")
        if not inputs.is_cuda:
            raise _lib.AetherHipError("aether_amd seq2seq models run on an MI355X only; got a CPU tensor (there is no CPU fallback)")
        B, N, _ = inputs.shape
        dev = inputs.device
        self._set_charges(self._index_of(charge_emb), B, N, dev)
        lib, plan, ws, (send, recv, order, rowptr), (pf, pe, pd), scal, hook = self._step_common(B, N, dev)
        D, he, hd, R, K = self._step_sizes()
        E1 = self.encoder.recv_edges.shape[0]
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        if uniform is None:
            uniform = torch.rand(B, E1, K, device=dev)
        xf, dhf, lg, ff, uf = f32(inputs), f32(decoder_hidden), f32(edge_logits), f32(predicted_field), f32(uniform)
        if xf.shape != (B, N, 2 * D) or dhf.shape != (B, N, hd) or lg.shape != (B, E1, K) or ff.shape != (B, N, D) or \
                uf.numel() != B * E1 * K:
            raise ValueError("single_step_forward: input shapes do not match the model")
        out, dh_out = torch.empty_like(xf), torch.empty_like(dhf)
        edges = torch.empty(B, E1, K, dtype=torch.float32, device=dev)
        st = lib.aether_s2s_charges_step(C.byref(pf), C.byref(pe), C.byref(pd), plan.data_ptr(), *scal, send.data_ptr(),
                                         recv.data_ptr(), order.data_ptr(), rowptr.data_ptr(), xf.data_ptr(), ff.data_ptr(),
                                         lg.data_ptr(), dhf.data_ptr(), None, None, uf.data_ptr(), ws.data_ptr(), ws.numel(),
                                         out.data_ptr(), dh_out.data_ptr(), None, None, edges.data_ptr(),
                                         torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(st, "aether_s2s_charges_step")
        return out, dh_out, edges

    @torch.no_grad()
    def _encoder_forward(self, inputs, predicted_field, index, max_edges_per_call=400_000):
        """The charge-aware full-sequence encoder (Encoder.forward, aether_charges.py:368-402) in evaluation mode: inputs
        [B, T, N, 2D], predicted_field [B, N, T, D], index [B, N] -> (prior_logits, posterior_logits [B, T, E, K], prior_state).
        The per-time-step features come from ``aether_s2s_charges_encoder_features`` (filter on the folded image, ``res1`` with
        its table) over chunks of T x B graphs, the recurrent half is the plain encoder's."""
        enc = self.encoder
        if enc.training:
            raise _lib.AetherHipError("the encoder uses BatchNorm running statistics: call .eval() first")
        lib = _lib.load()
        dev = inputs.device
        B, T, N, _ = inputs.shape
        D, he, hd, R, K = self._step_sizes()
        E1 = enc.recv_edges.shape[0]
        if inputs.shape[-1] != 2 * D or predicted_field.shape != (B, N, T, D):
            raise ValueError("encoder: input shapes do not match the module")
        x = inputs.detach().to(torch.float32).transpose(0, 1).contiguous()                # [T, B, N, 2D]
        f = predicted_field.detach().to(torch.float32).permute(2, 0, 1, 3).contiguous()   # [T, B, N, D]
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
            ci = index.to(device=dev, dtype=torch.int32).reshape(1, B * N).expand(t1 - t0, B * N).contiguous()
            need = lib.aether_s2s_charges_workspace_bytes(D, he, hd, R, prior_hidden, K, G * N, G * E1)
            ws = enc._cache.get("ws_charges")
            if ws is None or ws.numel() < need or ws.device != dev:
                ws = enc._cache["ws_charges"] = torch.empty(need, dtype=torch.uint8, device=dev)
            st = lib.aether_s2s_charges_encoder_features(
                C.byref(hook.struct), C.byref(pe), C.byref(pd), plan.data_ptr(), D, he, hd, R, n_layers, prior_hidden, K,
                1 if enc.pos_representation == "polar" else 0, N, G * N, G * E1, ci.data_ptr(), send.data_ptr(), recv.data_ptr(),
                order.data_ptr(), rowptr.data_ptr(), x[t0:t1].data_ptr(), f[t0:t1].data_ptr(), ws.data_ptr(), ws.numel(),
                feats[t0:t1].data_ptr(), stream)
            _lib.check(st, "aether_s2s_charges_encoder_features")
        return enc._sequence_heads(feats, B)

    def calculate_loss(self, inputs, is_train=False, teacher_forcing=True, return_edges=False, return_logits=False,
                       use_prior_logits=False, charges=None, uniform=None):
        """aether_charges.py:115-167 in evaluation mode, as ``Aether.calculate_loss``: the charge-aware full-sequence encoder's
        prior / posterior logits, the decoder stepped through the sequence on hard samples of the posterior (teacher forcing
        per ``val_teacher_forcing_steps``), NLL and KL as the params dictionary selects.  ``charges`` [B, >= N] is in the
        signature because the runner looks for it there (experiments/electrostatic/train.py:96); ``uniform`` [T - 1, B, E, K]:
        the Gumbel draws (drawn on the device when omitted)."""
        if is_train:
            raise _lib.AetherHipError("calculate_loss(is_train=True) (training of the seq2seq model) is not part of this "
                                      "library; evaluation (is_train=False), predict_future and predict_field are")
        if charges is None:
            raise ValueError("AetherCharges needs the particles' charges: pass charges=[B, >= num_objects] (+-1)")
        if not inputs.is_cuda or not charges.is_cuda:
            raise _lib.AetherHipError("aether_amd seq2seq models run on an MI355X only; got a CPU tensor (there is no CPU fallback)")
        with torch.no_grad():           # (not a decorator: the runner inspects this method's argument names)
            B, T, N, _ = inputs.shape
            index = self.charge_to_index(charges[:, :N]).to(torch.int32)
            decoder_hidden = self.decoder.get_initial_hidden(inputs)
            x = inputs[:, :-1].transpose(2, 1).contiguous()
            predicted_field, _ = self.predict_field(x, index)                            # [B, N, T - 1, D]
            prior_logits, posterior_logits, _ = self._encoder_forward(inputs[:, :-1], predicted_field, index)
            tf_steps = self.val_teacher_forcing_steps
            all_predictions, edges, predictions = [], None, None
            for step in range(T - 1):
                if (teacher_forcing and (tf_steps == -1 or step < tf_steps)) or step == 0:
                    current_inputs, current_field = inputs[:, step], predicted_field[:, :, step].contiguous()
                else:
                    current_inputs = predictions
                    current_field, _ = self.predict_field(predictions, index)
                logits = (prior_logits if use_prior_logits else posterior_logits)[:, step].contiguous()
                predictions, decoder_hidden, edges = self.single_step_forward(
                    current_inputs, decoder_hidden, logits, True, current_field, index,
                    uniform=None if uniform is None else uniform[step])
                all_predictions.append(predictions)
            all_predictions = torch.stack(all_predictions, dim=1)
            return self._loss_terms(inputs, all_predictions, prior_logits, posterior_logits, edges, return_edges, return_logits)

    @torch.no_grad()
    def predict_future(self, inputs, prediction_steps, return_edges=False, return_everything=False, charges=None, uniform=None,
                       graph=False):
        """aether_charges.py:169-208.  inputs [B, T, N, 2D] (burn-in observations), charges [B, >= N] (+-1; the first N
        columns are used, :177-178); ``uniform`` [T - 1 + steps, B, E, K]: the Gumbel draws (drawn on the device when omitted).
        ``return_everything``: the burn-in steps' predictions (and edges) in front of the predicted ones, as the reference.
        ``graph``: the whole loop from ONE captured hipGraph; both ways run the same kernels and give identical results."""
        if charges is None:
            raise ValueError("AetherCharges needs the particles' charges: pass charges=[B, >= num_objects] (+-1)")
        if not inputs.is_cuda:
            raise _lib.AetherHipError("aether_amd seq2seq models run on an MI355X only; got a CPU tensor (there is no CPU fallback)")
        B, T, N, _ = inputs.shape
        E, R = N * (N - 1), self.encoder.rnn_hidden_size
        dev = inputs.device
        cidx = self._charges_arg(charges, B, N, dev)
        decoder_hidden = self.decoder.get_initial_hidden(inputs)
        prior_hidden = (torch.zeros(B, E, R, device=dev), torch.zeros(B, E, R, device=dev))
        steps = int(prediction_steps)
        if return_everything:
            return self._predict_everything(inputs, steps, decoder_hidden, prior_hidden, uniform, return_edges)
        burn = inputs[:, :T - 1].float() if T > 1 else None
        # (the burn-in half runs the same step: the encoder's prior path is causal, as for Aether.predict_future)
        if graph:
            preds, edges, _ = self._graphed_rollout(burn, inputs[:, T - 1].float(), decoder_hidden, prior_hidden, steps, uniform,
                                                    return_edges, extra_key=(cidx.data_ptr(),))
        else:
            preds, edges, _ = self._fused_rollout(burn, inputs[:, T - 1].float(), decoder_hidden, prior_hidden, steps, uniform,
                                                  return_edges)
        return (preds, edges) if return_edges else preds

    def _predict_everything(self, inputs, steps, decoder_hidden, prior_hidden, uniform, return_edges):
        """``return_everything`` (:189-191): step by step, keeping what the burn-in steps predict."""
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
