"""Restatement of the variable-N dNRI baseline's prediction path (nn/dynamicvars/dnri_dynamicvars.py) from a state_dict
with the model's own keys, in the dtype it is given: the encoder's own kNN graph, the prior step on the present objects, the
hard Gumbel sample, the decoder step, and the prediction loop built on them.  One scene at a time, as the reference runs; the
primitives are oracle/seq2seq_oracle.py's Gumbel sample and tests/s2s_charges_restatement.py's nn.LSTM.  The model has no
field and no frames: every stage reads the raw 4 columns."""
import torch
import torch.nn.functional as F

from oracle import seq2seq_oracle as S
from s2s_charges_restatement import _lstm, sub

KNN_K = 10


def knn_graph(x, mask, k=KNN_K):
    """The encoder's own graph of one frame: x [Nmax, >= 2], mask [Nmax] -> (send, recv) in the numbering of the present
    objects.  Every present object, in row order, sends to its min(k, Nmax - 1) nearest present neighbours by position,
    nearest first; neighbours that do not exist (fewer present objects than k + 1) are left out."""
    Nmax = x.shape[0]
    present = mask != 0
    k = min(k, Nmax - 1)
    pos = x[:, :2]
    d = (pos[:, None, :] - pos[None, :, :]).norm(dim=-1)
    d = d.masked_fill(~(present[:, None] & present[None, :]), float("inf"))
    d.fill_diagonal_(float("inf"))
    dist, nbr = d.topk(k, dim=-1, largest=False)
    compact = torch.cumsum(present.long(), 0) - 1
    keep = ~torch.isinf(dist)
    send = compact[torch.arange(Nmax)[:, None].expand(Nmax, k)][keep]
    recv = compact[nbr][keep]
    return send, recv


def _mlp(p, prefix, x):
    """RefNRIMLP in evaluation mode: Linear, ELU, Linear, ELU, BatchNorm on running statistics (none with no_encoder_bn)."""
    x = F.elu(F.linear(x, p[prefix + ".model.0.weight"], p[prefix + ".model.0.bias"]))
    x = F.elu(F.linear(x, p[prefix + ".model.3.weight"], p[prefix + ".model.3.bias"]))
    if prefix + ".bn.weight" not in p:
        return x
    return F.batch_norm(x, p[prefix + ".bn.running_mean"], p[prefix + ".bn.running_var"], p[prefix + ".bn.weight"],
                        p[prefix + ".bn.bias"], False, 0.0, 1e-5)


def edge_features(enc, x, send, recv):
    """x [n, 4]: the present objects; send / recv: the kNN graph -> mlp4 output [E, h]."""
    y = _mlp(enc, "mlp1", x)
    y = _mlp(enc, "mlp2", torch.cat([y[send], y[recv]], -1))
    skip = y
    y = torch.zeros(x.shape[0], y.shape[-1], dtype=y.dtype).index_add_(0, recv, y)       # a sum: no division
    y = _mlp(enc, "mlp3", y)
    return _mlp(enc, "mlp4", torch.cat([y[send], y[recv], skip], -1))


def prior_head(enc, h, prior_layers):
    y = h
    for layer in range(prior_layers):
        name = "prior_fc_out" if prior_layers == 1 else f"prior_fc_out.{2 * layer}"
        y = F.linear(y, enc[name + ".weight"], enc[name + ".bias"])
        if layer + 1 < prior_layers:
            y = F.elu(y)
    return y


def prior_step(enc, x, mask, node_inds, graph, state, prior_layers=3):
    """One prior step of one scene.  x [Nmax, 4], mask [Nmax], node_inds: rows of the present objects, graph = (send, recv, ..)
    of the caller in their numbering, state (h, c) each [Nmax (Nmax - 1), R] -> (logits [E, K], (h', c'), (h1, c1) [E, R])."""
    Nmax = x.shape[0]
    n = len(node_inds)
    if n <= 1:
        return torch.empty(0, prior_head(enc, state[0][:1], prior_layers).shape[-1], dtype=x.dtype), state, None
    ksend, krecv = knn_graph(x, mask)
    feats = edge_features(enc, x[mask != 0], ksend, krecv)
    gs, gr = node_inds[graph[0]], node_inds[graph[1]]
    slot = gs * (Nmax - 1) + gr - (gr >= gs).long()                      # row e of the features meets the caller's edge e
    assert slot.numel() == feats.shape[0], "the caller's graph and the encoder's kNN graph differ in size"
    _, (h1, c1) = _lstm(enc, "forward_rnn.", feats.unsqueeze(1), (state[0][slot].unsqueeze(0), state[1][slot].unsqueeze(0)))
    h1, c1 = h1[0], c1[0]
    new_h, new_c = state[0].clone(), state[1].clone()
    new_h[slot], new_c[slot] = h1, c1
    return prior_head(enc, h1, prior_layers), (new_h, new_c), (h1, c1)


def decoder_step(dec, x, hidden, edges, mask, graph, skip_first):
    """One decoder step of one scene.  x [Nmax, 4], hidden [Nmax, hd], edges [E, K], graph = (send, recv, edge2node [n, deg])
    -> (pred_all [Nmax, 4] -- zero at the absent rows --, hidden')."""
    node_inds = (mask != 0).nonzero()[:, 0]
    n = node_inds.numel()
    pred_all = torch.zeros_like(x)
    if n == 0:
        return pred_all, hidden
    assert n > 1, "a scene with one present object is not part of the path"
    send, recv, e2n = graph
    cur_h, cur_x = hidden[node_inds], x[node_inds]
    K = edges.shape[-1]
    k0 = 1 if skip_first else 0
    norm = float(K - k0)
    lin = lambda name, v: F.linear(v, dec[name + ".weight"], dec.get(name + ".bias"))
    pre_msg = torch.cat([cur_h[recv], cur_h[send]], -1)
    all_msgs = torch.zeros(send.numel(), cur_h.shape[-1], dtype=x.dtype)
    for k in range(k0, K):
        msg = torch.tanh(lin(f"msg_fc2.{k}", torch.tanh(lin(f"msg_fc1.{k}", pre_msg))))
        all_msgs = all_msgs + msg * edges[:, k:k + 1] / norm
    incoming = all_msgs[e2n[:, 0]].clone()
    for i in range(1, e2n.shape[1]):
        incoming = incoming + all_msgs[e2n[:, i]]
    agg = incoming / (n - 1)
    r = torch.sigmoid(lin("input_r", cur_x) + lin("hidden_r", agg))
    i = torch.sigmoid(lin("input_i", cur_x) + lin("hidden_i", agg))
    nn_ = torch.tanh(lin("input_n", cur_x) + r * lin("hidden_h", agg))
    cur_h = (1 - i) * nn_ + i * cur_h
    pred = cur_x + lin("out_fc3", torch.relu(lin("out_fc2", torch.relu(lin("out_fc1", cur_h)))))
    hidden = hidden.clone()
    hidden[node_inds] = cur_h
    pred_all[node_inds] = pred
    return pred_all, hidden


class Model:
    """The model's parts cast once to ``dtype``."""

    def __init__(self, sd, dtype, prior_layers=3, skip_first=False, tau=0.5):
        self.sd = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd.items()}
        self.enc, self.dec = sub(self.sd, "encoder."), sub(self.sd, "decoder.")
        self.prior_layers, self.skip_first, self.tau, self.dtype = prior_layers, skip_first, tau, dtype
        self.hd = self.dec["out_fc2.weight"].shape[0]
        self.R = self.enc["forward_rnn.weight_hh_l0"].shape[1]

    def prior(self, x, mask, node_inds, graph, state):
        return prior_step(self.enc, x.to(self.dtype), mask, node_inds, graph, state, self.prior_layers)

    def decoder(self, x, hidden, edges, mask, graph):
        return decoder_step(self.dec, x.to(self.dtype), hidden.to(self.dtype), edges.to(self.dtype), mask, graph,
                            self.skip_first)

    def sample(self, logits, uniform):
        K = logits.shape[-1]
        return S.gumbel_hard(logits.reshape(-1, K), uniform.reshape(-1, K).to(self.dtype), self.tau)

    def predict_future(self, inputs, masks, node_inds, graph_info, burn_in_masks, uniform, return_all=False):
        """predict_future of one scene.  inputs [T, Nmax, 4], masks / burn_in_masks [T, Nmax], node_inds[t], graph_info[t],
        uniform[t] ([E_t, K]) -> predictions [T - 1, Nmax, 4] (+ the samples and the logits of every step)."""
        inputs = inputs.to(self.dtype)
        T, Nmax, _ = inputs.shape
        slots = Nmax * (Nmax - 1)
        state = (torch.zeros(slots, self.R, dtype=self.dtype), torch.zeros(slots, self.R, dtype=self.dtype))
        hidden = torch.zeros(Nmax, self.hd, dtype=self.dtype)
        last = inputs[0]
        preds, samples, logits_all = [], [], []
        for t in range(T - 1):
            observed = burn_in_masks[t].unsqueeze(-1).to(self.dtype)
            x = observed * inputs[t] + (1 - observed) * last
            logits, state, _ = self.prior(x, masks[t], node_inds[t], graph_info[t], state)
            z = self.sample(logits, uniform[t]) if logits.numel() else logits
            last, hidden = self.decoder(x, hidden, z, masks[t], graph_info[t])
            preds.append(last)
            samples.append(z)
            logits_all.append(logits)
        out = torch.stack(preds, 0)
        return (out, samples, logits_all) if return_all else out
