"""Restatement of the seq2seq ablation DNRIAether (nn/seq2seq/ablations/dnri_aether.py) from a state_dict with the model's own
keys, in the dtype of its inputs, on tests/s2s_dnri_restatement.py (the dNRI stages: the encoder's stack is the same function
of a wider row) and oracle/seq2seq_oracle.py (``predict_field``, the Gumbel sample, the heads and the loss terms).  Every layer
that reads the raw state in dNRI reads ext = [inputs | field] here; both decoders add their prediction to the 2D-wide inputs."""
import torch
import torch.nn.functional as F

import s2s_dnri_restatement as RS
from oracle import seq2seq_oracle as S


def recurrent_step(dec, x, field, hidden, edges, skip_first=False):
    """DNRI_Decoder.forward (dnri_aether.py:525-582) -> (outputs [B, N, 2D], hidden')."""
    B, N, _ = x.shape
    send, recv = RS._edges(N)
    K = edges.shape[-1]
    k0 = 1 if skip_first else 0
    norm = float(K - k0)
    lin = lambda name, v: F.linear(v, dec[name + ".weight"], dec.get(name + ".bias"))
    pre_msg = torch.cat([hidden[:, recv], hidden[:, send]], -1)
    all_msgs = torch.zeros(B, recv.shape[0], hidden.shape[-1], dtype=x.dtype)
    for k in range(k0, K):
        msg = torch.tanh(lin(f"msg_fc2.{k}", torch.tanh(lin(f"msg_fc1.{k}", pre_msg))))
        all_msgs = all_msgs + msg * edges[:, :, k:k + 1] / norm
    agg = RS._receiver_sum(all_msgs, recv, N) / (N - 1)
    ext = torch.cat([x, field], -1)                                                    # :564
    r = torch.sigmoid(lin("input_r", ext) + lin("hidden_r", agg))
    i = torch.sigmoid(lin("input_i", ext) + lin("hidden_i", agg))
    n = torch.tanh(lin("input_n", ext) + r * lin("hidden_h", agg))
    hidden = (1 - i) * n + i * hidden
    pred = lin("out_fc3", torch.relu(lin("out_fc2", torch.relu(lin("out_fc1", hidden)))))
    return x + pred, hidden


def mlp_step(dec, x, field, edges, skip_first=False):
    """DNRI_MLP_Decoder.forward (dnri_aether.py:624-677) -> (outputs [B, N, 2D], None)."""
    B, N, _ = x.shape
    send, recv = RS._edges(N)
    K = edges.shape[-1]
    k0 = 1 if skip_first else 0
    lin = lambda name, v: F.linear(v, dec[name + ".weight"], dec[name + ".bias"])
    ext = torch.cat([x, field], -1)                                                    # :633
    pre_msg = torch.cat([ext[:, recv], ext[:, send]], -1)
    all_msgs = torch.zeros(B, recv.shape[0], dec["msg_fc2.0.weight"].shape[0], dtype=x.dtype)
    for k in range(k0, K):
        msg = torch.relu(lin(f"msg_fc2.{k}", torch.relu(lin(f"msg_fc1.{k}", pre_msg))))
        all_msgs = all_msgs + msg * edges[:, :, k:k + 1]
    agg = RS._receiver_sum(all_msgs, recv, N)
    pred = lin("out_fc3", torch.relu(lin("out_fc2", torch.relu(lin("out_fc1", torch.cat([ext, agg], -1))))))
    return x + pred, None


class Model(RS.Model):
    """The model's parts cast once to ``dtype``; ``field(x)`` is predict_field (dnri_aether.py:81-85)."""

    def __init__(self, sd, dtype, prior_layers=3, skip_first=False, tau=0.5):
        super().__init__(sd, dtype, prior_layers, skip_first, tau)
        self.D = self.sd["field_net.4.weight"].shape[0]

    def field(self, x):
        return S.predict_field(self.sd, x, self.D)

    def prior(self, x, state, field=None):
        field = self.field(x) if field is None else field
        return RS.prior_step(self.enc, torch.cat([x, field], -1), state, self.prior_layers)

    def decoder(self, x, hidden, edges, field=None):
        field = self.field(x) if field is None else field
        if self.markov:
            return mlp_step(self.dec, x, field, edges, self.skip_first)
        return recurrent_step(self.dec, x, field, hidden, edges, self.skip_first)

    def step(self, x, hidden, state, uniform):
        """One autoregressive step -> (x', hidden', state', edges, logits); the field is queried once (:161-163)."""
        field = self.field(x)
        logits, state = self.prior(x, state, field)
        z = self.sample(logits, uniform)
        out, hidden = self.decoder(x, hidden, z, field)
        return out, hidden, state, z, logits

    def encoder_forward(self, inputs, field=None):
        """DNRI_Encoder.forward (dnri_aether.py:409-441): inputs [B, T, N, 2D], field [B, T, N, D] (queried when omitted)."""
        field = self.field(inputs) if field is None else field
        return super().encoder_forward(torch.cat([inputs, field], -1))

    def calculate_loss(self, cfg, inputs, uniform, teacher_forcing=True, use_prior_logits=False):
        """calculate_loss(is_train=False) (dnri_aether.py:96-140) -> (loss, nll, kl, posterior_logits, predictions)."""
        inputs = inputs.to(self.dtype)
        B, T, N, _ = inputs.shape
        field_all = self.field(inputs[:, :-1])                                         # [B, T - 1, N, D]
        prior, post, _ = self.encoder_forward(inputs[:, :-1], field_all)
        hidden = self.initial_hidden(B, N)
        tf_steps = cfg.get("val_teacher_forcing_steps", -1)
        preds, predictions = [], None
        for step in range(T - 1):
            forced = (teacher_forcing and (tf_steps == -1 or step < tf_steps)) or step == 0
            cur = inputs[:, step] if forced else predictions
            field = field_all[:, step] if forced else self.field(predictions)
            z = self.sample((prior if use_prior_logits else post)[:, step], uniform[step])
            predictions, hidden = self.decoder(cur, hidden, z, field)
            preds.append(predictions)
        preds = torch.stack(preds, 1)
        nll, kl = S.nll_and_kl(cfg, preds, inputs[:, 1:], post, prior, N)
        return (nll + cfg.get("kl_coef", 1.0) * kl).mean(), nll, kl, post, preds
