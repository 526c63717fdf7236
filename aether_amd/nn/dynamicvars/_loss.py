"""The evaluation half of ``calculate_loss`` of the variable-N models (``AetherDynamicVars``, ``DNRIDynamicVars``), as the inD
runner calls it for its validation NLL / KL (experiments/ind/train_dynamicvars.py:155-200): the sequence encoder as ONE
library call over all frames, the teacher-forced decoding loop as ONE library call, and the masked loss terms
(aether_dynamicvars.py:331-372, dnri_dynamicvars.py:233-275) as scalar reductions in plain torch on the device.

The reference's sequence encoder (``Encoder.forward``, aether_dynamicvars.py:588-670; dnri_dynamicvars.py:463-542) never
writes its forward LSTM state back -- ``tmp_state0`` / ``tmp_state1`` are built and dropped (:632-635 / :506-509) -- and its
reverse pass never calls ``reverse_rnn`` (:657-662 / :531-536).  Every frame therefore gives ``h_t = LSTMcell(x_t, (0, 0))``,
``prior = prior_fc_out(h_t)``, ``posterior = encoder_fc_out([h_t | 0])`` and a returned ``forward_state`` of zeros; parity with
that is what is built.  ``encoder.reverse_rnn.*`` stays in the ``state_dict`` and is never read.

A model supplies ``_encode_sequence`` (its ``encoder.forward``), ``_loss_entries(lib)`` -> (workspace_bytes_fn, entry, name,
head: the ``C.byref`` parameter structs in front of the configuration) and ``_loss_stage_step`` (one staged decoder step).
"""
from __future__ import annotations

import ctypes as C
import math

import torch
import torch.nn as nn

from ... import _lib
from ._scene import cached_workspace, f32, i64

SEQ_CHUNK = 256                     # frames per aether_dyn*_sequence_logits call (the scene engine's limit)
_TRAIN_REFUSAL = ("calculate_loss(is_train=True) (training of the variable-N model: gradients, soft samples) is not part of "
                  "this library; evaluation (is_train=False), predict_future and predict_field are")
_NORMALIZED_REFUSAL = "normalized_inputs is the training loop's cache of the feature transform: it must be None here"
_BATCH_REFUSAL = "Batching during forward not currently supported"          # the reference's words (:590-591 / :464-465)


def posterior_struct(encoder_fc_out):
    """-> (AetherDynPosteriorParams, layers, hidden) of an ``encoder_fc_out`` (``_mlp_out``: Linear, or Linear-ELU-..-Linear)."""
    layers = [encoder_fc_out] if isinstance(encoder_fc_out, nn.Linear) else [m for m in encoder_fc_out if isinstance(m, nn.Linear)]
    ps = _lib.STRUCTS["AetherDynPosteriorParams"]()
    for l, lin in enumerate(layers):
        ps.w[l], ps.b[l] = lin.weight.data_ptr(), lin.bias.data_ptr()
    return ps, len(layers), (layers[0].out_features if len(layers) > 1 else 0)


def check_sequence_args(inputs, normalized_inputs):
    if normalized_inputs is not None:
        raise _lib.AetherHipError(_NORMALIZED_REFUSAL)
    if inputs.size(0) > 1:
        raise ValueError(_BATCH_REFUSAL)


@torch.no_grad()
def sequence_logits(encoder, entries, cfg, inputs, node_masks, all_node_inds, chunk=None):
    """``Encoder.forward`` of both models: inputs [1, F, Nmax, 4], node_masks [1, F, Nmax], all_node_inds[0][t] the present rows
    -> (prior_logits, posterior_logits [1, sum_t E_t, K], forward_state: zeros of the reference's shape).  The F frames go
    through the library as scenes of one prior stage, ``chunk`` (default 256, the engine's limit) at a time -- an int, or the
    successive chunk lengths, the last repeating (``encoder._seq_chunk``: the tests' knob); the frames are independent, so the
    result does not depend on the split."""
    ws_bytes, entry, name, head = entries
    lib = _lib.load()
    dev = inputs.device
    F, Nmax = int(inputs.size(1)), int(inputs.size(2))
    K, R = encoder.num_edges, encoder.rnn_hidden_size
    chunk = chunk or encoder.__dict__.get("_seq_chunk") or SEQ_CHUNK
    sizes = [int(c) for c in (chunk if isinstance(chunk, (tuple, list)) else (chunk,))]
    if not all(1 <= c <= SEQ_CHUNK for c in sizes):
        raise ValueError("the sequence encoder takes 1..256 frames per call")
    frames, masks = f32(inputs, dev)[0], f32(node_masks, dev)[0]
    n = [int(len(all_node_inds[0][t])) for t in range(F)]
    k = min(cfg.knn_k, Nmax - 1)
    e = [n_t * min(k, n_t - 1) if n_t > 1 else 0 for n_t in n]
    post, post_layers, post_hidden = posterior_struct(encoder.encoder_fc_out)
    prior_logits = torch.empty(sum(e), K, dtype=torch.float32, device=dev)
    posterior_logits = torch.empty(sum(e), K, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    edge0 = a = 0
    while a < F:
        b = min(F, a + sizes[0])
        sizes = sizes[1:] or sizes
        n_host, e_host = (C.c_int64 * (b - a))(*n[a:b]), (C.c_int64 * (b - a))(*e[a:b])
        need = ws_bytes(C.byref(cfg), post_layers, post_hidden, b - a, Nmax, n_host, e_host)
        if need == 0:
            raise _lib.AetherHipError(f"{name}_workspace_bytes: " + lib.aether_last_error().decode())
        ws = cached_workspace(encoder, "_seq_ws", need, dev)
        st = entry(*head, C.byref(post), C.byref(cfg), post_layers, post_hidden, b - a, Nmax, n_host, e_host,
                   frames.data_ptr() + a * Nmax * 16, masks.data_ptr() + a * Nmax * 4, prior_logits.data_ptr() + edge0 * K * 4,
                   posterior_logits.data_ptr() + edge0 * K * 4, ws.data_ptr(), ws.numel(), stream)
        _lib.check(st, name)
        edge0 += sum(e[a:b])
        a = b
    slots = Nmax * (Nmax - 1)
    forward_state = (torch.zeros(1, slots, R, device=dev), torch.zeros(1, slots, R, device=dev))
    return prior_logits.unsqueeze(0), posterior_logits.unsqueeze(0), forward_state


class SceneLossMixin:
    """``calculate_loss(is_train=False)`` of the models on the scene engine, its staged twin and the masked loss terms."""

    def _init_loss_config(self, params):
        # the keys of aether_dynamicvars.py:24-46 / dnri_dynamicvars.py:21-40 that the evaluation loss reads (the seq2seq
        # models' _EvalLoss reads val_teacher_forcing_steps and an unmasked NLL: another configuration)
        self.teacher_forcing_steps = params.get("teacher_forcing_steps", -1)
        self.anneal_teacher_forcing = params.get("anneal_teacher_forcing", False)
        self.normalize_kl = params.get("normalize_kl", False)
        self.normalize_kl_per_var = params.get("normalize_kl_per_var", False)
        self.normalize_nll = params.get("normalize_nll", False)
        self.normalize_nll_per_var = params.get("normalize_nll_per_var", False)
        self.nll_loss_type = params.get("nll_loss_type", "crossent")
        self.prior_variance = params.get("prior_variance")

    # -- the call -----------------------------------------------------------------------------------------------------------------
    def calculate_loss(self, inputs, node_masks, node_inds, graph_info, is_train=False, teacher_forcing=True, return_edges=False,
                       return_logits=False, use_prior_logits=False, normalized_inputs=None, uniform=None):
        """aether_dynamicvars.py:152-207 / dnri_dynamicvars.py:70-114 in evaluation mode, called as the inD runner's validation
        block calls it (train_dynamicvars.py:171).  inputs [1, T, Nmax, 4], node_masks [1, T, Nmax], node_inds[0][t],
        graph_info[0][t] as ``predict_future`` takes them.  Two library calls: the sequence encoder over the T - 1 frames, and
        the decoding loop (per step: teacher-forced or previous prediction, hard sample of the posterior -- or prior -- logits,
        decoder step); then the masked NLL and the KL in torch.  ``uniform``: per-step Gumbel draws (list of [E_t, K]), drawn
        on the device when omitted.  Returns (loss, loss_nll, loss_kl[, last step's edges | posterior_logits [1, sum E, K],
        all_predictions [1, T - 1, Nmax, 4]]) as :202-207.  Every frame needs two or more present objects (the runner skips
        other sequences, :166-174).  In free-running mode an object that first appears after frame 0 enters the decoder with
        the all-zero row of the previous prediction, as in the reference (:176, :866-868)."""
        if is_train:
            raise _lib.AetherHipError(_TRAIN_REFUSAL)
        check_sequence_args(inputs, normalized_inputs)
        with torch.no_grad():
            return self._calculate_loss_eval(inputs, node_masks, node_inds, graph_info, teacher_forcing, return_edges,
                                             return_logits, use_prior_logits, uniform, stepwise=False)

    def _calculate_loss_stepwise(self, inputs, node_masks, node_inds, graph_info, teacher_forcing=True, return_edges=False,
                                 return_logits=False, use_prior_logits=False, uniform=None):
        """The same through ``encoder.forward`` and one staged ``single_step_forward`` per step: what the one-call loop is
        compared with."""
        check_sequence_args(inputs, None)
        with torch.no_grad():
            return self._calculate_loss_eval(inputs, node_masks, node_inds, graph_info, teacher_forcing, return_edges,
                                             return_logits, use_prior_logits, uniform, stepwise=True)

    def _teacher_steps(self, teacher_forcing, T):
        """-> the library's teacher_forcing_steps: -1 every step, else the steps below it (:166-172)."""
        if not teacher_forcing:
            return 0
        if self.anneal_teacher_forcing:
            return int(math.ceil((1 - self.train_percent) * T))
        tfs = int(self.teacher_forcing_steps)
        if tfs < -1:
            raise ValueError("teacher_forcing_steps is -1 (always) or a step count")
        return tfs

    def _calculate_loss_eval(self, inputs, node_masks, node_inds, graph_info, teacher_forcing, return_edges, return_logits,
                             use_prior_logits, uniform, stepwise):
        if not inputs.is_cuda:
            raise _lib.AetherHipError(f"aether_amd {type(self).__name__}.calculate_loss runs on an MI355X only; got a CPU tensor "
                                      "(there is no CPU fallback)")
        self._guard(inputs)
        T = int(inputs.size(1))
        if T < 2:
            raise ValueError("calculate_loss needs at least two frames")
        prior_logits, posterior_logits, _ = self._encode_sequence(inputs[:, :-1], node_masks[:, :-1], node_inds, graph_info)
        logits = prior_logits if use_prior_logits else posterior_logits
        tfs = self._teacher_steps(teacher_forcing, T)
        loop = self._loss_loop_staged if stepwise else self._loss_loop
        all_predictions, edges = loop(inputs, node_masks, graph_info, logits, tfs, uniform)
        return self._loss_terms(inputs, node_masks, all_predictions, prior_logits, posterior_logits, edges, return_edges,
                                return_logits)

    def _step_sizes(self, node_masks, graph_info, n_steps, logits, uniform):
        """Per step (n_present is the graph's: edge2node has a row per present object): host sizes and device tensors."""
        dev = logits.device
        K = self.num_edge_types
        steps = []
        for t in range(n_steps):
            gs, gr, e2n = (i64(g, dev) for g in graph_info[0][t])
            E = int(gs.numel())
            if gr.numel() != E or e2n.ndim != 2:
                raise ValueError(f"graph_info of step {t}: (send [E], recv [E], edge2node [n, in_degree])")
            u = torch.rand(E, K, device=dev) if uniform is None else f32(uniform[t], dev).reshape(-1, K)
            if u.shape[0] != E:
                raise ValueError(f"uniform of step {t} must be [E, K]")
            steps.append((int(e2n.shape[0]), E, int(e2n.shape[1]), gs, gr, e2n, u))
        if sum(s[1] for s in steps) != logits.shape[1]:
            raise ValueError("graph_info and the encoder's kNN graphs list a different number of edges")
        return steps

    def _loss_loop(self, inputs, node_masks, graph_info, logits, tfs, uniform):
        """The decoding loop as ONE library call -> (all_predictions [1, T - 1, Nmax, 4], last step's edges [1, E, K])."""
        lib = _lib.load()
        dev = inputs.device
        n_steps, Nmax, K = int(inputs.size(1)) - 1, int(inputs.size(2)), self.num_edge_types
        steps = self._step_sizes(node_masks, graph_info, n_steps, logits, uniform)
        e2n_all = [s[5].reshape(-1) for s in steps if s[5].numel()]
        if e2n_all:                                                # (one device round trip for all steps)
            lo_hi = torch.stack([v for s in steps if s[5].numel() for v in torch.aminmax(s[5])]).cpu().tolist()
            for i, s in enumerate(s for s in steps if s[5].numel()):
                if lo_hi[2 * i] < 0 or lo_hi[2 * i + 1] >= s[1]:
                    raise ValueError("graph_info: an edge2node entry names an edge its step's graph does not have")
        n_host = (C.c_int64 * n_steps)(*[s[0] for s in steps])
        e_host = (C.c_int64 * n_steps)(*[s[1] for s in steps])
        deg = (C.c_int * n_steps)(*[s[2] for s in steps])
        ptrs = [(C.c_void_p * n_steps)(*[s[j].data_ptr() for s in steps]) for j in (3, 4, 5, 6)]
        x, m = f32(inputs, dev)[0], f32(node_masks, dev)[0]
        lg = f32(logits, dev)[0]
        cfg = self._step_config()
        ws_bytes, entry, name, head = self._loss_entries(lib)
        need = ws_bytes(C.byref(cfg), Nmax, n_steps, n_host, e_host, deg)
        if need == 0:
            raise _lib.AetherHipError(f"{name}_workspace_bytes: " + lib.aether_last_error().decode())
        ws = cached_workspace(self, "_loss_ws", need, dev)
        preds = torch.empty(n_steps, Nmax, 4, dtype=torch.float32, device=dev)
        edges = torch.empty(steps[-1][1], K, dtype=torch.float32, device=dev)
        st = entry(*head, C.byref(cfg), Nmax, n_steps, tfs, x.data_ptr(), m.data_ptr(), n_host, e_host, deg, *ptrs[:3],
                   lg.data_ptr(), ptrs[3], preds.data_ptr(), edges.data_ptr(), ws.data_ptr(), ws.numel(),
                   torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(st, name)
        return preds.unsqueeze(0), edges.unsqueeze(0)

    def _loss_loop_staged(self, inputs, node_masks, graph_info, logits, tfs, uniform):
        """The reference's loop (:171-193 / :83-100) around one staged decoder step (``_loss_stage_step``)."""
        n_steps = int(inputs.size(1)) - 1
        steps = self._step_sizes(node_masks, graph_info, n_steps, logits, uniform)
        decoder_hidden = self.decoder.get_initial_hidden(inputs)
        predictions, edges, all_predictions, edge0 = None, None, [], 0
        for t, (n, E, _, gs, gr, e2n, u) in enumerate(steps):
            teacher = t == 0 or tfs < 0 or t < tfs
            state = inputs[:, t] if teacher else predictions
            predictions, decoder_hidden, edges = self._loss_stage_step(state, node_masks[:, t], (gs, gr, e2n), decoder_hidden,
                                                                       logits[:, edge0:edge0 + E].contiguous(), u, n)
            edge0 += E
            all_predictions.append(predictions)
        return torch.stack(all_predictions, dim=1), edges

    # -- the loss terms (scalar reductions: plain torch on the device) -----------------------------------------------------------
    def _loss_terms(self, inputs, node_masks, all_predictions, prior_logits, posterior_logits, edges, return_edges, return_logits):
        # Reduced in fp64 and rounded once to the tensors' dtype: the KL of a trained model is of order 1e-3, a sum of
        # differences of logarithms of order 1, of which an fp32 reduction loses 1e-5 (measured 6e-6 at 220 edges) -- more
        # than the whole logit error the library is held to.  The tensors are a few thousand numbers.
        dev, dt = all_predictions.device, all_predictions.dtype
        target = inputs[:, 1:].to(device=dev, dtype=torch.float64)
        node_masks = node_masks.to(dev)
        target_masks = ((node_masks[:, :-1] == 1) * (node_masks[:, 1:] == 1)).float()                         # :196 (fp32, as there)
        loss_nll = self.nll(all_predictions.double(), target, target_masks)
        prob = torch.softmax(posterior_logits.double(), dim=-1)
        loss_kl = self.kl_categorical_learned(prob, prior_logits.double())
        loss = (loss_nll + self.kl_coef * loss_kl).mean().to(dt)
        loss_nll, loss_kl = loss_nll.to(dt), loss_kl.to(dt)
        if return_edges:
            return loss, loss_nll, loss_kl, edges
        if return_logits:
            return loss, loss_nll, loss_kl, posterior_logits, all_predictions
        return loss, loss_nll, loss_kl

    def nll(self, preds, target, masks):                                                                  # :331-337
        if self.nll_loss_type == "crossent":
            return self.nll_crossent(preds, target, masks)
        if self.nll_loss_type == "gaussian":
            return self.nll_gaussian(preds, target, masks)
        if self.nll_loss_type == "poisson":
            return self.nll_poisson(preds, target, masks)
        raise ValueError("nll_loss_type must be 'crossent', 'gaussian' or 'poisson'")

    def nll_gaussian(self, preds, target, masks):                                                         # :339-348
        neg_log_p = ((preds - target) ** 2 / (2 * self.prior_variance)) * masks.unsqueeze(-1)
        const = 0.5 * math.log(2 * math.pi * self.prior_variance)
        if self.normalize_nll_per_var or not self.normalize_nll:
            raise NotImplementedError()
        return (neg_log_p.sum(-1) + const * masks).view(preds.size(0), -1).sum(dim=-1) / (masks.view(masks.size(0), -1).sum(dim=1) + 1e-8)

    def _nll_elementwise(self, loss, preds, masks):
        if not self.normalize_nll:
            raise NotImplementedError()
        return (loss * masks.unsqueeze(-1)).view(preds.size(0), -1).sum(dim=-1) / masks.view(masks.size(0), -1).sum(dim=1)

    def nll_crossent(self, preds, target, masks):                                                         # :351-356
        return self._nll_elementwise(nn.functional.binary_cross_entropy_with_logits(preds, target, reduction="none"), preds, masks)

    def nll_poisson(self, preds, target, masks):                                                          # :358-363
        return self._nll_elementwise(nn.functional.poisson_nll_loss(preds, target, reduction="none"), preds, masks)

    def kl_categorical_learned(self, preds, prior_logits):                                                # :365-373
        log_prior = torch.log_softmax(prior_logits, dim=-1)
        kl_div = preds * (torch.log(preds + 1e-16) - log_prior)
        if not self.normalize_kl:
            raise NotImplementedError()
        return kl_div.sum(-1).view(preds.size(0), -1).mean(dim=1)
