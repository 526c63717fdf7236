"""Restatement of the evaluation half of ``calculate_loss`` of both variable-N models (nn/dynamicvars/aether_dynamicvars.py:
152-207, dnri_dynamicvars.py:70-114) from a state_dict with the model's own keys, in the dtype it is given: the sequence
encoder, the decoding loop and the masked loss terms.  Built on tests/dyn_dnri_restatement.py (the dNRI stages) and
oracle/dynamicvars_oracle.py (the Aether stages).

The sequence encoder is restated as the reference computes it, not as it reads: the forward LSTM state is never written back
(``tmp_state0`` / ``tmp_state1`` are dropped, aether_dynamicvars.py:632-635, dnri_dynamicvars.py:506-509) and the reverse pass
never calls ``reverse_rnn`` (:657-662 / :531-536).  So no state is carried between frames -- every frame is an LSTM cell from
(0, 0) -- the posterior head sees [h | 0], and ``reverse_rnn.*`` is never read here.
"""
import math

import torch
import torch.nn.functional as F

import dyn_dnri_restatement as RS
from oracle import dynamicvars_oracle as DO
from oracle import seq2seq_oracle as S
from s2s_charges_restatement import sub

LOSS_FLAGS = {"normalize_nll": True, "normalize_kl": True, "nll_loss_type": "gaussian", "prior_variance": 5e-5,
              "teacher_forcing_steps": -1}                       # the inD runner's


def head(p, name, x):
    """``_mlp_out``: a Linear, or Linear-ELU-..-Linear (keys name.weight or name.0.weight, name.2.weight, ..)."""
    if name + ".weight" in p:
        return F.linear(x, p[name + ".weight"], p[name + ".bias"])
    idx = sorted(int(k[len(name) + 1:].split(".")[0]) for k in p if k.startswith(name + ".") and k.endswith(".weight"))
    for j, i in enumerate(idx):
        x = F.linear(x, p[f"{name}.{i}.weight"], p[f"{name}.{i}.bias"])
        if j + 1 < len(idx):
            x = F.elu(x)
    return x


def masked_loss(preds, inputs, masks, prior_logits, posterior_logits, prior_variance=LOSS_FLAGS["prior_variance"], kl_coef=1.0):
    """Gaussian NLL (normalize_nll) and kl_categorical_learned (normalize_kl), :331-372, on preds [1, T - 1, Nmax, 4], inputs
    [1, T, Nmax, 4], masks [1, T, Nmax], logits [1, sum E, K] -> (loss, loss_nll, loss_kl)."""
    target = inputs[:, 1:].to(preds.dtype)
    m = ((masks[:, :-1] == 1) * (masks[:, 1:] == 1)).float()          # fp32 in every dtype, as the reference's .float() (:196)
    neg_log_p = ((preds - target) ** 2 / (2 * prior_variance)) * m.unsqueeze(-1)
    const = 0.5 * math.log(2 * math.pi * prior_variance)
    nll = (neg_log_p.sum(-1) + const * m).view(preds.size(0), -1).sum(dim=-1) / (m.view(m.size(0), -1).sum(dim=1) + 1e-8)
    prob = torch.softmax(posterior_logits, dim=-1)
    kl = (prob * (torch.log(prob + 1e-16) - torch.log_softmax(prior_logits, dim=-1))).sum(-1).view(prob.size(0), -1).mean(dim=1)
    return (nll + kl_coef * kl).mean(), nll, kl


class Model:
    """``kind``: 'aether' or 'dnri'.  The parts cast once to ``dtype``."""

    def __init__(self, kind, sd, dtype, skip_first=False, tau=0.5, pos="cart"):
        assert kind in ("aether", "dnri")
        self.kind, self.dtype, self.skip_first, self.tau, self.pos = kind, dtype, skip_first, tau, pos
        self.sd = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}
        self.enc, self.dec = sub(self.sd, "encoder."), sub(self.sd, "decoder.")
        self.hd = self.dec["out_fc2.weight"].shape[0]

    def field(self, x, mask):
        return DO.predict_field(self.sd, x[None], mask[None]) if self.kind == "aether" else None

    def features(self, x, mask):
        """compute_feat_transform of one frame: x [Nmax, 4], mask [Nmax] -> [E, h], rows in the encoder's kNN order."""
        if self.kind == "aether":
            return DO.encoder_features(self.enc, x[None], mask, self.field(x, mask), self.pos)[0]
        return RS.edge_features(self.enc, x[mask != 0], *RS.knn_graph(x, mask))

    def encode(self, frames, masks):
        """Encoder.forward: frames [F, Nmax, 4], masks [F, Nmax] -> (prior_logits, posterior_logits) [sum E, K].  No state
        crosses a frame; reverse_rnn is not read."""
        prior, post = [], []
        for x, m in zip(frames.to(self.dtype), masks):
            f = self.features(x, m)
            zero = torch.zeros(f.shape[0], self.enc["forward_rnn.weight_hh_l0"].shape[1], dtype=self.dtype)
            h, _ = DO._lstm_cell(self.enc, "forward_rnn.", f, zero, zero)
            prior.append(head(self.enc, "prior_fc_out", h))
            post.append(head(self.enc, "encoder_fc_out", torch.cat([h, torch.zeros_like(h)], -1)))
        return torch.cat(prior), torch.cat(post)

    def decode(self, x, hidden, edges, mask, graph):
        if self.kind == "aether":
            pred, hid = DO.decoder_step(self.dec, x[None], hidden[None], edges[None], mask, graph, self.field(x, mask),
                                        self.skip_first, self.pos)
            return pred[0], hid[0]
        return RS.decoder_step(self.dec, x, hidden, edges, mask, graph, self.skip_first)

    def calculate_loss(self, inputs, masks, graph_info, uniform, teacher_forcing=True, use_prior_logits=False):
        """inputs [T, Nmax, 4], masks [T, Nmax], graph_info[t], uniform[t] ([E_t, K]) -> dict of prior / posterior logits,
        predictions [T - 1, Nmax, 4], the samples of every step and (loss, nll, kl)."""
        inputs = inputs.to(self.dtype)
        T = inputs.shape[0]
        prior, post = self.encode(inputs[:-1], masks[:-1])
        logits = prior if use_prior_logits else post
        K = logits.shape[-1]
        hidden = torch.zeros(inputs.shape[1], self.hd, dtype=self.dtype)
        preds, samples, e0, pred = [], [], 0, None
        for t in range(T - 1):
            x = inputs[t] if (teacher_forcing or t == 0) else pred
            E = graph_info[t][0].numel()
            z = S.gumbel_hard(logits[e0:e0 + E], uniform[t].reshape(-1, K).to(self.dtype), self.tau)
            e0 += E
            pred, hidden = self.decode(x, hidden, z, masks[t], graph_info[t])
            preds.append(pred)
            samples.append(z)
        assert e0 == logits.shape[0], "the data set's graphs and the encoder's kNN graphs differ in size"
        preds = torch.stack(preds)
        loss, nll, kl = masked_loss(preds[None], inputs[None], masks[None], prior[None], post[None])
        return {"prior": prior, "posterior": post, "predictions": preds, "samples": samples, "loss": loss, "nll": nll, "kl": kl}
