"""Restatement of the charge-aware seq2seq Aether (nn/seq2seq/ablations/aether_charges.py) from a state_dict with the model's
own keys, in the dtype of its inputs, on the primitives of oracle/seq2seq_oracle.py (local frames, RefNRIMLP, Gumbel sample,
receiver means).  Two forms of every charge-dependent layer:

  folded=False  as the reference writes it: the 16-wide embedding emb[c] concatenated behind the features
                (field query :88-98, Encoder.single_step_forward :404-432, RecurrentDecoder.forward :615-680);
  folded=True   as the library computes it: a Linear over [f | emb[c]] is W_f f + (b + W_c emb[c]), one of 2 table rows per
                node (4 per edge: row 2 c_recv + c_send), and the anisotropic filter's 32 embedding features are four
                one-hot features whose weight blocks are sum_j emb[c][j] block_j (28 / 43 features instead of 56 / 71).

The two are the same algebra; tests/test_s2s_charges.py holds them equal in fp64.  ``frames_dtype``: build the local frames
in that dtype (in 3-D the origin edge's Euler angle sits on a branch cut: an fp64 restatement of an fp32 evaluation takes the
frames from fp32, as tests/test_s2s_markov.py::restate explains)."""
import torch
import torch.nn.functional as F

from oracle import seq2seq_oracle as S

CE = 16


def sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def _node_linear(p, name, feats, emb_w, cidx, folded):
    """Linear ``name`` over [feats | emb[c]] per node."""
    W, b = p[name + ".weight"], p[name + ".bias"]
    if not folded:
        return F.linear(torch.cat([feats, emb_w[cidx]], -1), W, b)
    nf = feats.shape[-1]
    table = b + emb_w @ W[:, nf:].t()                                   # [2, M]
    return feats @ W[:, :nf].t() + table[cidx]


def _edge_linear(p, name, feats, emb_w, cr, cs, folded):
    """Linear ``name`` over [feats | emb[c_recv] | emb[c_send]] per edge."""
    W, b = p[name + ".weight"], p[name + ".bias"]
    if not folded:
        return F.linear(torch.cat([feats, emb_w[cr], emb_w[cs]], -1), W, b)
    nf = feats.shape[-1]
    tr, ts = emb_w @ W[:, nf:nf + CE].t(), emb_w @ W[:, nf + CE:].t()   # [2, M] each
    table = (b + tr[:, None, :] + ts[None, :, :]).reshape(4, -1)        # row 2 c_recv + c_send
    return feats @ W[:, :nf].t() + table[2 * cr + cs]


def fold_filter(W2, b2, emb_w, EA, h):
    """[(EA + 32) h, h] / [(EA + 32) h] -> [(EA + 4) h, h] / [(EA + 4) h]: blocks [recv 0, recv 1, send 0, send 1] behind EA."""
    Wv, bv = W2.view(EA + 2 * CE, h, h), b2.view(EA + 2 * CE, h)
    parts_w, parts_b = [Wv[:EA]], [bv[:EA]]
    for s in range(2):
        blk_w, blk_b = Wv[EA + CE * s:EA + CE * (s + 1)], bv[EA + CE * s:EA + CE * (s + 1)]
        parts_w.append(torch.einsum("cj,joh->coh", emb_w, blk_w))
        parts_b.append(emb_w @ blk_b)
    return torch.cat(parts_w).reshape(-1, h), torch.cat(parts_b).reshape(-1)


def _refnri_mlp(p, prefix, x):
    """RefNRIMLP in evaluation mode (nn/utils/model_utils.py:15-55) with torch's own batch_norm, as the reference runs it."""
    x = F.elu(F.linear(x, p[prefix + ".model.0.weight"], p[prefix + ".model.0.bias"]))
    x = F.elu(F.linear(x, p[prefix + ".model.3.weight"], p[prefix + ".model.3.bias"]))
    flat = F.batch_norm(x.reshape(-1, x.shape[-1]), p[prefix + ".bn.running_mean"], p[prefix + ".bn.running_var"],
                        p[prefix + ".bn.weight"], p[prefix + ".bn.bias"], False, 0.0, 1e-5)
    return flat.view(x.shape)


def _lstm(p, prefix, x, state=None):
    """nn.LSTM(batch_first=True) itself on x [rows, T, h], as the reference runs it (:395-396, :429): the fp32 values then
    follow the reference's operation order bit for bit (an LSTM cell written out differs from it by an ulp)."""
    w_ih, w_hh = p[prefix + "weight_ih_l0"], p[prefix + "weight_hh_l0"]
    rnn = torch.nn.LSTM(w_ih.shape[1], w_hh.shape[1], batch_first=True).to(w_ih.dtype)
    with torch.no_grad():
        for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            getattr(rnn, name).copy_(p[prefix + name])
        return rnn(x.contiguous(), None if state is None else tuple(t.contiguous() for t in state))


def _frames(x, field, use_3d, pos_representation, frames_dtype):
    dt = x.dtype
    ext = torch.cat([x, field.to(dt)], -1).to(frames_dtype or dt)
    return tuple(t.to(dt) for t in S.augmented_localizer(ext, use_3d, pos_representation))


def _edges(N):
    return torch.where(~torch.eye(N, dtype=bool))                       # send, recv


def predict_field(sd, x, cidx, num_dims, folded=False):
    """aether_charges.py:88-98.  x [B, N, >= D] or [B, N, T, >= D], cidx [B, N] (long)."""
    emb_w = sd["charge_embedding.weight"].to(x.dtype)
    p = {k: v.to(x.dtype) for k, v in sd.items() if k.startswith("field_net.")}
    if x.ndim == 4:
        cidx = cidx.unsqueeze(2).expand(x.shape[:3])
    rff = S.fourier_features(x[..., :num_dims], sd["coordinate_embedding.B"])
    h = F.silu(_node_linear(p, "field_net.0", rff, emb_w, cidx, folded))
    h = F.silu(F.linear(h, p["field_net.2.weight"], p["field_net.2.bias"]))
    return F.linear(h, p["field_net.4.weight"], p["field_net.4.bias"])


def encoder_features(enc, emb_w, x, field, cidx, use_3d, pos_representation, folded=False, frames_dtype=None):
    """The per-time-step half of the encoder (:406-421 / :371-389): x [B, N, 2D] -> mlp4 output [B, E, h]."""
    B, N, _ = x.shape
    send, recv = _edges(N)
    rel_feat, _, edge_attr, edge_pos = _frames(x, field, use_3d, pos_representation, frames_dtype)
    cr, cs = cidx[:, recv], cidx[:, send]
    hw = F.elu(F.linear(edge_pos, enc["edge_filter.edge_filter.0.weight"], enc["edge_filter.edge_filter.0.bias"]))
    W2, b2 = enc["edge_filter.edge_filter.2.weight"], enc["edge_filter.edge_filter.2.bias"]
    h = W2.shape[1]
    if folded:
        W2, b2 = fold_filter(W2, b2, emb_w, edge_attr.shape[-1], h)
        feats = torch.cat([edge_attr, F.one_hot(cr, 2).to(x.dtype), F.one_hot(cs, 2).to(x.dtype)], -1)
    else:
        feats = torch.cat([edge_attr, emb_w[cr], emb_w[cs]], -1)
    ew = F.linear(hw, W2, b2)
    ew = ew.reshape(ew.shape[:-1] + (feats.shape[-1], h))
    ea = (feats.unsqueeze(-2) @ ew).squeeze(-2)
    res_x = _node_linear(enc, "res1", rel_feat, emb_w, cidx, folded)
    incoming = torch.zeros(B, N, h, dtype=x.dtype).index_add_(1, recv, ea)
    y = _refnri_mlp(enc, "mlp3", incoming / (N - 1) + res_x)
    y = torch.cat([y[:, send], y[:, recv], ea], -1)
    return _refnri_mlp(enc, "mlp4", y)


def prior_step(enc, emb_w, x, prior_state, field, cidx, use_3d=False, pos_representation="cart", prior_layers=3, folded=False,
               frames_dtype=None):
    """Encoder.single_step_forward (:404-432) -> (logits [B, E, K], (h', c'))."""
    y = encoder_features(enc, emb_w, x, field, cidx, use_3d, pos_representation, folded, frames_dtype)
    h0, c0 = prior_state
    shape = h0.shape
    _, (h1, c1) = _lstm(enc, "forward_rnn.", y.reshape(-1, 1, y.shape[-1]), (h0.reshape(1, -1, shape[-1]), c0.reshape(1, -1, shape[-1])))
    h1, c1 = h1.view(shape), c1.view(shape)
    y = h1
    for layer in range(prior_layers):
        name = "prior_fc_out" if prior_layers == 1 else f"prior_fc_out.{2 * layer}"
        y = F.linear(y, enc[name + ".weight"], enc[name + ".bias"])
        if layer + 1 < prior_layers:
            y = F.elu(y)
    return y, (h1, c1)


def decoder_step(dec, emb_w, x, hidden, edges, field, cidx, use_3d=False, skip_first=False, folded=False, frames_dtype=None):
    """RecurrentDecoder.forward (:615-680) -> (outputs [B, N, 2D], hidden')."""
    B, N, _ = x.shape
    D = 3 if use_3d else 2
    send, recv = _edges(N)
    K = edges.shape[-1]
    k0 = 1 if skip_first else 0
    lin = lambda name, v: F.linear(v, dec[name + ".weight"], dec.get(name + ".bias"))
    pre_msg = torch.cat([hidden[:, recv], hidden[:, send]], -1)
    all_msgs = torch.zeros(B, recv.shape[0], hidden.shape[-1], dtype=x.dtype)
    for k in range(k0, K):
        msg = torch.tanh(lin(f"msg_fc2.{k}", torch.tanh(lin(f"msg_fc1.{k}", pre_msg))))
        all_msgs = all_msgs + msg * edges[:, :, k:k + 1]
    agg = S._scatter_mean_dim1(all_msgs, recv, N)
    rel_feat, Rinv, edge_attr, _ = _frames(x, field, use_3d, "polar", frames_dtype)
    cr, cs = cidx[:, recv], cidx[:, send]
    present = torch.zeros_like(all_msgs)
    for k in range(k0, K):
        msg = torch.relu(_edge_linear(dec, f"present_msg_fc1.{k}", edge_attr, emb_w, cr, cs, folded))
        msg = torch.relu(lin(f"present_msg_fc2.{k}", msg))
        present = present + msg * edges[:, :, k:k + 1]
    pagg = S._scatter_mean_dim1(present, recv, N)
    if folded:                                                          # the table rows carry the sum of the gate's biases
        gate = lambda g: _node_linear({"w.weight": dec[f"input_{g}.weight"], "w.bias": dec[f"input_{g}.bias"] + dec[f"present_{g}.bias"]},
                                      "w", rel_feat, emb_w, cidx, True) + pagg @ dec[f"present_{g}.weight"].t()
    else:
        gate = lambda g: _node_linear(dec, f"input_{g}", rel_feat, emb_w, cidx, False) + lin(f"present_{g}", pagg)
    r = torch.sigmoid(gate("r") + lin("hidden_r", agg))
    i = torch.sigmoid(gate("i") + lin("hidden_i", agg))
    n = torch.tanh(gate("n") + r * lin("hidden_h", agg))
    hidden = (1 - i) * n + i * hidden
    pred = lin("out_mlp.6", torch.relu(lin("out_mlp.3", torch.relu(lin("out_mlp.0", hidden)))))
    pred = torch.cat([torch.einsum("...ij,...j->...i", Rinv, c) for c in pred.split(D, dim=-1)], -1)
    return x + pred, hidden


class Model:
    """The model's parts cast once to ``dtype``; ``cfg``: use_3d, pos_representation, prior_layers, skip_first, tau."""

    def __init__(self, sd, dtype, use_3d=False, pos_representation="cart", prior_layers=3, skip_first=False, tau=0.5,
                 folded=False, frames_dtype=None):
        self.sd = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}
        self.enc, self.dec = sub(self.sd, "encoder."), sub(self.sd, "decoder.")
        self.emb_w = self.sd["charge_embedding.weight"]
        self.use_3d, self.pos, self.prior_layers, self.skip_first, self.tau = use_3d, pos_representation, prior_layers, skip_first, tau
        self.folded, self.frames_dtype, self.dtype = folded, frames_dtype, dtype
        self.D = 3 if use_3d else 2

    def field(self, x, cidx):
        return predict_field(self.sd, x, cidx, self.D, self.folded)

    def prior(self, x, state, field, cidx):
        return prior_step(self.enc, self.emb_w, x, state, field, cidx, self.use_3d, self.pos, self.prior_layers, self.folded,
                          self.frames_dtype)

    def decoder(self, x, hidden, edges, field, cidx):
        return decoder_step(self.dec, self.emb_w, x, hidden, edges, field, cidx, self.use_3d, self.skip_first, self.folded,
                            self.frames_dtype)

    def step(self, x, hidden, state, uniform, cidx):
        """One autoregressive step -> (x', hidden', state', edges, logits, field)."""
        field = self.field(x, cidx)
        logits, state = self.prior(x, state, field, cidx)
        z = S.gumbel_hard(logits.reshape(-1, logits.shape[-1]), uniform.reshape(-1, logits.shape[-1]).to(self.dtype),
                          self.tau).view(logits.shape)
        out, hidden = self.decoder(x, hidden, z, field, cidx)
        return out, hidden, state, z, logits, field

    def encoder_forward(self, inputs, field, cidx):
        """Encoder.forward (:368-402): inputs [B, T, N, 2D], field [B, N, T, D] -> (prior_logits, posterior_logits
        [B, T, E, K], (h, c) of the forward LSTM [1, B E, R])."""
        B, T, N, _ = inputs.shape
        x = torch.stack([encoder_features(self.enc, self.emb_w, inputs[:, t], field[:, :, t], cidx, self.use_3d, self.pos,
                                          self.folded, self.frames_dtype) for t in range(T)], 2)       # [B, E, T, h]
        E = x.shape[1]
        x = x.reshape(B * E, T, x.shape[-1])
        forward_x, state = _lstm(self.enc, "forward_rnn.", x)
        reverse_x = _lstm(self.enc, "reverse_rnn.", x.flip(1))[0].flip(1)
        shape = lambda y: y.view(B, E, T, -1).transpose(1, 2).contiguous()
        prior = shape(S._head(self.enc, "prior_fc_out", forward_x))
        post = shape(S._head(self.enc, "encoder_fc_out", torch.cat([forward_x, reverse_x], -1)))
        return prior, post, state

    def calculate_loss(self, cfg, inputs, uniform, cidx, teacher_forcing=True, use_prior_logits=False):
        """calculate_loss(is_train=False) (:115-167) -> (loss, nll, kl, posterior_logits, predictions); ``cfg``: the params
        entries the loss reads, ``uniform`` [T - 1, B E, K]."""
        inputs = inputs.to(self.dtype)
        B, T, N, _ = inputs.shape
        field = self.field(inputs[:, :-1].transpose(2, 1).contiguous(), cidx)             # [B, N, T - 1, D]
        prior, post, _ = self.encoder_forward(inputs[:, :-1], field, cidx)
        hidden = torch.zeros(B, N, self.dec["hidden_r.weight"].shape[0], dtype=self.dtype)
        tf_steps = cfg.get("val_teacher_forcing_steps", -1)
        preds, predictions = [], None
        for step in range(T - 1):
            if (teacher_forcing and (tf_steps == -1 or step < tf_steps)) or step == 0:
                cur, cur_f = inputs[:, step], field[:, :, step]
            else:
                cur, cur_f = predictions, self.field(predictions, cidx)
            logits = (prior if use_prior_logits else post)[:, step]
            z = S.gumbel_hard(logits.reshape(-1, logits.shape[-1]), uniform[step].reshape(-1, logits.shape[-1]).to(self.dtype),
                              self.tau).view(logits.shape)
            predictions, hidden = self.decoder(cur, hidden, z, cur_f, cidx)
            preds.append(predictions)
        preds = torch.stack(preds, 1)
        nll, kl = S.nll_and_kl(cfg, preds, inputs[:, 1:], post, prior, N)
        return (nll + cfg.get("kl_coef", 1.0) * kl).mean(), nll, kl, post, preds

    def predict_future(self, inputs, steps, uniform, cidx, return_all=False):
        """predict_future (:169-208); the burn-in half step by step (the prior path is causal).  uniform [T - 1 + steps, ...].
        -> predictions [B, steps, N, 2D], edges [B, steps, E, K] (+ every step's logits when ``return_all``)."""
        inputs = inputs.to(self.dtype)
        B, T, N, _ = inputs.shape
        E = N * (N - 1)
        h = self.dec["hidden_r.weight"].shape[0]
        R = self.enc["forward_rnn.weight_hh_l0"].shape[1]
        hidden = torch.zeros(B, N, h, dtype=self.dtype)
        state = (torch.zeros(B, E, R, dtype=self.dtype), torch.zeros(B, E, R, dtype=self.dtype))
        preds, edges, logits_all = [], [], []
        x = None
        for t in range(T - 1 + steps):
            x_in = inputs[:, t] if t < T else x
            x, hidden, state, z, logits, _ = self.step(x_in, hidden, state, uniform[t], cidx)
            logits_all.append(logits)
            if t >= T - 1:
                preds.append(x)
                edges.append(z)
        out = (torch.stack(preds, 1), torch.stack(edges, 1))
        return out + (torch.stack(logits_all, 0), (hidden, state)) if return_all else out
