"""Restatement of the seq2seq dNRI baseline (nn/seq2seq/dnri.py) from a state_dict with the model's own keys, in the dtype of
its inputs: the three stages of a step -- the encoder's prior step, the hard Gumbel sample, either decoder -- and the loops
built on them, on the primitives of oracle/seq2seq_oracle.py (Gumbel sample, heads, loss terms) and of
tests/s2s_charges_restatement.py (RefNRIMLP and nn.LSTM as the reference runs them).  The model has no local frames: every
stage reads the raw state."""
import torch
import torch.nn.functional as F

from oracle import seq2seq_oracle as S
from s2s_charges_restatement import _lstm, _refnri_mlp, sub


def _edges(N):
    return torch.where(~torch.eye(N, dtype=bool))                       # send, recv


def _receiver_sum(v, recv, N):
    """edge2node_mat @ v (dnri.py:350, :515, :612): rows of v [B, E, h] summed per receiver, in edge order."""
    return torch.zeros(v.shape[0], N, v.shape[-1], dtype=v.dtype).index_add_(1, recv, v)


def encoder_features(enc, x):
    """The per-time-step half of the encoder (dnri.py:405-413 / :376-384): x [B, N, 2D] -> mlp4 output [B, E, h]."""
    N = x.shape[1]
    send, recv = _edges(N)
    y = _refnri_mlp(enc, "mlp1", x)
    y = _refnri_mlp(enc, "mlp2", torch.cat([y[:, send], y[:, recv]], -1))           # node2edge: [send | recv] (:334-342)
    skip = y
    y = _refnri_mlp(enc, "mlp3", _receiver_sum(y, recv, N) / (N - 1))               # edge2node (:344-351)
    y = torch.cat([y[:, send], y[:, recv], skip], -1)
    return _refnri_mlp(enc, "mlp4", y)


def prior_step(enc, x, prior_state, prior_layers=3):
    """DNRI_Encoder.single_step_forward (dnri.py:403-424) -> (logits [B, E, K], (h', c'))."""
    y = encoder_features(enc, x)
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


def recurrent_step(dec, x, hidden, edges, skip_first=False):
    """DNRI_Decoder.forward (dnri.py:479-534) -> (outputs [B, N, 2D], hidden')."""
    B, N, _ = x.shape
    send, recv = _edges(N)
    K = edges.shape[-1]
    k0 = 1 if skip_first else 0
    norm = float(K - k0)
    lin = lambda name, v: F.linear(v, dec[name + ".weight"], dec.get(name + ".bias"))
    pre_msg = torch.cat([hidden[:, recv], hidden[:, send]], -1)
    all_msgs = torch.zeros(B, recv.shape[0], hidden.shape[-1], dtype=x.dtype)
    for k in range(k0, K):
        msg = torch.tanh(lin(f"msg_fc2.{k}", torch.tanh(lin(f"msg_fc1.{k}", pre_msg))))
        all_msgs = all_msgs + msg * edges[:, :, k:k + 1] / norm
    agg = _receiver_sum(all_msgs, recv, N) / (N - 1)
    r = torch.sigmoid(lin("input_r", x) + lin("hidden_r", agg))
    i = torch.sigmoid(lin("input_i", x) + lin("hidden_i", agg))
    n = torch.tanh(lin("input_n", x) + r * lin("hidden_h", agg))
    hidden = (1 - i) * n + i * hidden
    pred = lin("out_fc3", torch.relu(lin("out_fc2", torch.relu(lin("out_fc1", hidden)))))
    return x + pred, hidden


def mlp_step(dec, x, edges, skip_first=False):
    """DNRI_MLP_Decoder.forward (dnri.py:574-624) -> (outputs [B, N, 2D], None)."""
    B, N, _ = x.shape
    send, recv = _edges(N)
    K = edges.shape[-1]
    k0 = 1 if skip_first else 0
    lin = lambda name, v: F.linear(v, dec[name + ".weight"], dec[name + ".bias"])
    pre_msg = torch.cat([x[:, recv], x[:, send]], -1)
    all_msgs = torch.zeros(B, recv.shape[0], dec["msg_fc2.0.weight"].shape[0], dtype=x.dtype)
    for k in range(k0, K):
        msg = torch.relu(lin(f"msg_fc2.{k}", torch.relu(lin(f"msg_fc1.{k}", pre_msg))))
        all_msgs = all_msgs + msg * edges[:, :, k:k + 1]
    agg = _receiver_sum(all_msgs, recv, N)                                          # a sum: no division (:612-613)
    pred = lin("out_fc3", torch.relu(lin("out_fc2", torch.relu(lin("out_fc1", torch.cat([x, agg], -1))))))
    return x + pred, None


class Model:
    """The model's parts cast once to ``dtype``."""

    def __init__(self, sd, dtype, prior_layers=3, skip_first=False, tau=0.5):
        self.sd = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}
        self.enc, self.dec = sub(self.sd, "encoder."), sub(self.sd, "decoder.")
        self.markov = "hidden_r.weight" not in self.dec
        self.prior_layers, self.skip_first, self.tau, self.dtype = prior_layers, skip_first, tau, dtype
        self.hd = self.dec["out_fc2.weight"].shape[0]

    def prior(self, x, state):
        return prior_step(self.enc, x, state, self.prior_layers)

    def decoder(self, x, hidden, edges):
        if self.markov:
            return mlp_step(self.dec, x, edges, self.skip_first)
        return recurrent_step(self.dec, x, hidden, edges, self.skip_first)

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
        """DNRI_Encoder.forward (dnri.py:371-401): inputs [B, T, N, 2D] -> (prior_logits, posterior_logits [B, T, E, K], state)."""
        B, T, N, _ = inputs.shape
        x = torch.stack([encoder_features(self.enc, inputs[:, t]) for t in range(T)], 2)                # [B, E, T, h]
        E = x.shape[1]
        x = x.reshape(B * E, T, x.shape[-1])
        forward_x, state = _lstm(self.enc, "forward_rnn.", x)
        reverse_x = _lstm(self.enc, "reverse_rnn.", x.flip(1))[0].flip(1)
        shape = lambda y: y.view(B, E, T, -1).transpose(1, 2).contiguous()
        prior = shape(S._head(self.enc, "prior_fc_out", forward_x))
        post = shape(S._head(self.enc, "encoder_fc_out", torch.cat([forward_x, reverse_x], -1)))
        return prior, post, state

    def calculate_loss(self, cfg, inputs, uniform, teacher_forcing=True, use_prior_logits=False):
        """calculate_loss(is_train=False) (dnri.py:71-109) -> (loss, nll, kl, posterior_logits, predictions); ``cfg``: the
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

    def predict_future(self, inputs, steps, uniform, return_all=False, everything=False):
        """predict_future (dnri.py:111-136); the burn-in half step by step (the prior path is causal).  uniform
        [T - 1 + steps, ...] -> predictions [B, steps, N, 2D], edges [B, steps, E, K] (+ every step's logits);
        ``everything``: the burn-in steps' outputs in front (return_everything)."""
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
            if everything or t >= T - 1:
                preds.append(x)
                edges.append(z)
        out = (torch.stack(preds, 1), torch.stack(edges, 1))
        return out + (torch.stack(logits_all, 0),) if return_all else out
