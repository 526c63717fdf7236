"""Restatement of the seq2seq LoCS baseline (nn/seq2seq/locs.py) from a state_dict with the model's own keys, in the dtype of
its inputs, on the primitives of oracle/seq2seq_oracle.py (rotations, edge features, Gumbel sample, receiver means, loss
terms) and of tests/s2s_charges_restatement.py (RefNRIMLP and nn.LSTM as the reference runs them).

The plain ``Localizer`` (nn/utils/global_to_local.py:46-62) is the augmented one without the virtual origin node and without
the force columns: the edge features of ``create_edge_attr_pos_vel`` / ``create_3d_edge_attr_pos_vel``
(nn/utils/canonicalization.py:78-108, :175-202) are the first 3D + O columns of the augmented ones, operation for operation, so
they are taken from ``oracle.seq2seq_oracle.augmented_edge_attr`` on a zero force."""
import torch
import torch.nn.functional as F

from oracle import seq2seq_oracle as S
from s2s_charges_restatement import _lstm, _refnri_mlp, sub


def _edges(N):
    return torch.where(~torch.eye(N, dtype=bool))                       # send, recv


def canonicalize(x, use_3d):
    """canonicalize_inputs (canonicalization.py:12-30) -> (rel_feat [.., 2D], Rinv)."""
    if use_3d:
        vel = x[..., 3:]
        _, theta, phi = S._spherical3(vel)
        Rinv = S._rot3(theta, phi)
        return torch.cat([torch.zeros_like(x[..., :3]), S._mv(Rinv.transpose(-1, -2), vel)], -1), Rinv
    vel = x[..., 2:4]
    Rinv = S._rot2(torch.atan2(vel[..., [1]], vel[..., [0]]))
    canon = torch.zeros_like(x)
    canon[..., 2] = torch.norm(vel, dim=-1)
    return canon, Rinv


def localizer(x, use_3d=False, pos_representation="polar"):
    """Localizer.forward for the fully connected graph: x [B, N, 2D] -> rel_feat [B, N, 2D], Rinv [B, N, D, D], edge_attr
    [B, E, 5D + O], edge_pos [B, E, D + O]."""
    B, N, _ = x.shape
    D = 3 if use_3d else 2
    send, recv = _edges(N)
    rel_feat, Rinv = canonicalize(x, use_3d)
    nf = 3 * D + D * (D - 1) // 2
    ea = S.augmented_edge_attr(torch.cat([x, torch.zeros_like(x[..., :D])], -1), send, recv, use_3d)[..., :nf]
    edge_pos = ea[..., S.EDGE_POS_IDX[(use_3d, pos_representation)]]
    return rel_feat, Rinv, torch.cat([ea, rel_feat[:, recv]], -1), edge_pos


def _frames(x, use_3d, pos_representation, frames_dtype):
    return tuple(t.to(x.dtype) for t in localizer(x.to(frames_dtype or x.dtype), use_3d, pos_representation))


def encoder_features(enc, x, use_3d, pos_representation, frames_dtype=None):
    """The per-time-step half of the encoder (locs.py:343-354 / :315-326): x [B, N, 2D] -> mlp4 output [B, E, h]."""
    B, N, _ = x.shape
    send, recv = _edges(N)
    rel_feat, _, edge_attr, edge_pos = _frames(x, use_3d, pos_representation, frames_dtype)
    hw = F.elu(F.linear(edge_pos, enc["edge_filter.edge_filter.0.weight"], enc["edge_filter.edge_filter.0.bias"]))
    W2, b2 = enc["edge_filter.edge_filter.2.weight"], enc["edge_filter.edge_filter.2.bias"]
    h = W2.shape[1]
    ew = F.linear(hw, W2, b2)
    ew = ew.reshape(ew.shape[:-1] + (edge_attr.shape[-1], h))
    ea = (edge_attr.unsqueeze(-2) @ ew).squeeze(-2)
    res_x = F.linear(rel_feat, enc["res1.weight"], enc["res1.bias"])
    incoming = torch.zeros(B, N, h, dtype=x.dtype).index_add_(1, recv, ea)
    y = _refnri_mlp(enc, "mlp3", incoming / (N - 1) + res_x)
    y = torch.cat([y[:, send], y[:, recv], ea], -1)
    return _refnri_mlp(enc, "mlp4", y)


def prior_step(enc, x, prior_state, use_3d=False, pos_representation="polar", prior_layers=3, frames_dtype=None):
    """Encoder.single_step_forward (locs.py:341-365) -> (logits [B, E, K], (h', c'))."""
    y = encoder_features(enc, x, use_3d, pos_representation, frames_dtype)
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


def _globalize(pred, Rinv, D):
    return torch.cat([torch.einsum("...ij,...j->...i", Rinv, c) for c in pred.split(D, dim=-1)], -1)


def recurrent_step(dec, x, hidden, edges, use_3d=False, pos_representation="polar", skip_first=False, frames_dtype=None):
    """RecurrentDecoder.forward (locs.py:542-604) -> (outputs [B, N, 2D], hidden')."""
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
    rel_feat, Rinv, edge_attr, _ = _frames(x, use_3d, pos_representation, frames_dtype)
    present = torch.zeros_like(all_msgs)
    for k in range(k0, K):
        msg = torch.relu(lin(f"present_msg_fc2.{k}", torch.relu(lin(f"present_msg_fc1.{k}", edge_attr))))
        present = present + msg * edges[:, :, k:k + 1]
    pagg = S._scatter_mean_dim1(present, recv, N)
    gate = lambda g: lin(f"input_{g}", rel_feat) + lin(f"present_{g}", pagg)
    r = torch.sigmoid(gate("r") + lin("hidden_r", agg))
    i = torch.sigmoid(gate("i") + lin("hidden_i", agg))
    n = torch.tanh(gate("n") + r * lin("hidden_h", agg))
    hidden = (1 - i) * n + i * hidden
    pred = lin("out_mlp.6", torch.relu(lin("out_mlp.3", torch.relu(lin("out_mlp.0", hidden)))))
    return x + _globalize(pred, Rinv, D), hidden


def markov_step(dec, x, edges, use_3d=False, pos_representation="polar", skip_first=False, frames_dtype=None):
    """MarkovDecoder.forward (locs.py:425-454) -> (outputs [B, N, 2D], None)."""
    B, N, _ = x.shape
    D = 3 if use_3d else 2
    send, recv = _edges(N)
    k0 = 1 if skip_first else 0
    lin = lambda name, v: F.linear(v, dec[name + ".weight"], dec[name + ".bias"])
    rel_feat, Rinv, edge_attr, _ = _frames(x, use_3d, pos_representation, frames_dtype)
    ea = torch.relu(lin("edge_filter.lin2", torch.relu(lin("edge_filter.lin1", edge_attr))))
    ku = edges.shape[-1] - k0
    all_msgs = torch.sum(ea.view(*ea.shape[:-1], -1, ku) * edges[..., k0:].unsqueeze(-2), -1)
    agg = S._scatter_mean_dim1(all_msgs, recv, N)
    aug = agg + lin("res1", rel_feat)
    pred = lin("out_mlp.6", torch.relu(lin("out_mlp.3", torch.relu(lin("out_mlp.0", aug)))))
    return x + _globalize(pred, Rinv, D), None


class Model:
    """The model's parts cast once to ``dtype``.  ``frames_dtype``: build the local frames in that dtype (an fp64 restatement
    of an fp32 evaluation whose angles sit near a branch cut takes the frames from fp32)."""

    def __init__(self, sd, dtype, use_3d=False, pos_representation="polar", prior_layers=3, skip_first=False, tau=0.5,
                 frames_dtype=None):
        self.sd = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}
        self.enc, self.dec = sub(self.sd, "encoder."), sub(self.sd, "decoder.")
        self.markov = "edge_filter.lin1.weight" in self.dec
        self.use_3d, self.pos, self.prior_layers, self.skip_first, self.tau = use_3d, pos_representation, prior_layers, skip_first, tau
        self.frames_dtype, self.dtype = frames_dtype, dtype
        self.hd = self.dec["out_mlp.0.weight"].shape[0]

    def prior(self, x, state):
        return prior_step(self.enc, x, state, self.use_3d, self.pos, self.prior_layers, self.frames_dtype)

    def decoder(self, x, hidden, edges):
        if self.markov:
            return markov_step(self.dec, x, edges, self.use_3d, self.pos, self.skip_first, self.frames_dtype)
        return recurrent_step(self.dec, x, hidden, edges, self.use_3d, self.pos, self.skip_first, self.frames_dtype)

    def sample(self, logits, uniform):
        K = logits.shape[-1]
        return S.gumbel_hard(logits.reshape(-1, K), uniform.reshape(-1, K).to(self.dtype), self.tau).view(logits.shape)

    def step(self, x, hidden, state, uniform):
        """One autoregressive step -> (x', hidden', state', edges, logits)."""
        logits, state = self.prior(x, state)
        z = self.sample(logits, uniform)
        out, hidden = self.decoder(x, hidden, z)
        return out, hidden, state, z, logits

    def initial_hidden(self, B, N):
        return None if self.markov else torch.zeros(B, N, self.hd, dtype=self.dtype)

    def encoder_forward(self, inputs):
        """Encoder.forward (locs.py:309-339): inputs [B, T, N, 2D] -> (prior_logits, posterior_logits [B, T, E, K], state)."""
        B, T, N, _ = inputs.shape
        x = torch.stack([encoder_features(self.enc, inputs[:, t], self.use_3d, self.pos, self.frames_dtype)
                         for t in range(T)], 2)                                            # [B, E, T, h]
        E = x.shape[1]
        x = x.reshape(B * E, T, x.shape[-1])
        forward_x, state = _lstm(self.enc, "forward_rnn.", x)
        reverse_x = _lstm(self.enc, "reverse_rnn.", x.flip(1))[0].flip(1)
        shape = lambda y: y.view(B, E, T, -1).transpose(1, 2).contiguous()
        prior = shape(S._head(self.enc, "prior_fc_out", forward_x))
        post = shape(S._head(self.enc, "encoder_fc_out", torch.cat([forward_x, reverse_x], -1)))
        return prior, post, state

    def calculate_loss(self, cfg, inputs, uniform, teacher_forcing=True, use_prior_logits=False):
        """calculate_loss(is_train=False) (locs.py:79-120) -> (loss, nll, kl, posterior_logits, predictions); ``cfg``: the
        params entries the loss reads, ``uniform`` [T - 1, B E, K]."""
        inputs = inputs.to(self.dtype)
        B, T, N, _ = inputs.shape
        prior, post, _ = self.encoder_forward(inputs[:, :-1])
        hidden = self.initial_hidden(B, N)
        tf_steps = cfg.get("val_teacher_forcing_steps", -1)
        preds, predictions = [], None
        for step in range(T - 1):
            cur = inputs[:, step] if (teacher_forcing and (tf_steps == -1 or step < tf_steps)) or step == 0 else predictions
            z = self.sample((prior if use_prior_logits else post)[:, step], uniform[step])
            predictions, hidden = self.decoder(cur, hidden, z)
            preds.append(predictions)
        preds = torch.stack(preds, 1)
        nll, kl = S.nll_and_kl(cfg, preds, inputs[:, 1:], post, prior, N)
        return (nll + cfg.get("kl_coef", 1.0) * kl).mean(), nll, kl, post, preds

    def predict_future(self, inputs, steps, uniform, return_all=False):
        """predict_future (locs.py:122-151); the burn-in half step by step (the prior path is causal).  uniform
        [T - 1 + steps, ...] -> predictions [B, steps, N, 2D], edges [B, steps, E, K] (+ every step's logits)."""
        inputs = inputs.to(self.dtype)
        B, T, N, _ = inputs.shape
        E = N * (N - 1)
        R = self.enc["forward_rnn.weight_hh_l0"].shape[1]
        hidden = self.initial_hidden(B, N)
        state = (torch.zeros(B, E, R, dtype=self.dtype), torch.zeros(B, E, R, dtype=self.dtype))
        preds, edges, logits_all = [], [], []
        x = None
        for t in range(T - 1 + steps):
            x_in = inputs[:, t] if t < T else x
            x, hidden, state, z, logits = self.step(x_in, hidden, state, uniform[t])
            logits_all.append(logits)
            if t >= T - 1:
                preds.append(x)
                edges.append(z)
        out = (torch.stack(preds, 1), torch.stack(edges, 1))
        return out + (torch.stack(logits_all, 0),) if return_all else out
