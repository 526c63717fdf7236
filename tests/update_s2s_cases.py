"""The seq2seq / variable-N cases of tests/test_gpu_update_parity.py: the fused step and `predict_future` of the seq2seq
Aether (recurrent and Markov decoder), LoCS, AetherCharges and the gravitational DynamicFieldAether, N = 5, B = 3, D = 2 and 3.
Test helper, not a test module.

The update is "output state minus input state" over all 2D columns.  One step starts from a random state (decoder
hidden, prior LSTM state, for the dynamic field a random summary); `predict_future` runs one burn-in step on two frames
and three predicted steps, each held on its own increment (x = the fp64 loop's previous state), against the fp32 loop at
the same step.  Restatements: oracle/seq2seq_oracle.py, tests/test_s2s_markov.restate, tests/s2s_locs_restatement.py,
tests/s2s_charges_restatement.py, each run in fp64 and in fp32 on the state_dict of the module under test.

Two things about the references.  (1) In 3-D every node's origin edge has an Euler angle on its branch cut, +-pi by one
rounding (tests/test_s2s_markov.restate).  The existing seq2seq tests give the fp64 evaluation the local frames of
fp32; then the fp32 restatement and the reference share the rounding of the frames, the floor does not contain it, and
the kernels, which round their own, are charged for it alone (on the CPU the fp32 LoCS step moves from 1.3e-7 to
2.7e-7 when its frames are rounded another way).  Here the fp64 evaluation keeps its fp64 frames and takes from fp32
only the side of a cut (`_on_fp32_side`).  (2) A step draws its edge types with a hard Gumbel sample, which is discontinuous: the seeds are
those at which the two largest scores of every edge of the fp64 loop are at least GAP = 1e-3 apart -- five hundred
times the 1e-5 the logits are held to, over tau = 0.5 -- and the fp32 loop draws the same types (asserted without a GPU,
tests/test_update_metric.py); the kernels then have to draw them as well."""
from __future__ import annotations

import contextlib
import functools
import os
import sys

import torch

from conftest import REPO
from oracle import seq2seq_oracle as S
from update_cases import one_thread
from update_parity import check_update

for _p in ("tools", "oracle"):
    if os.path.join(REPO, _p) not in sys.path:
        sys.path.insert(0, os.path.join(REPO, _p))

B, N, TAU, GAP = 3, 5, 0.5, 1e-3
E = N * (N - 1)
FRAMES, STEPS = 2, 3
# (kind, D, model seed, input seed)
KINDS = ("aether_rec", "aether_markov", "locs", "charges", "dynfield")
SEEDS = {("aether_rec", 2): 7, ("aether_markov", 2): 7, ("dynfield", 2): 8}           # every other case: 5
CASES = [(kind, D, 61, SEEDS.get((kind, D), 5)) for kind in KINDS for D in (2, 3)]
TYPICAL = 5e-8


def case_id(c):
    return f"{c[0]}-D{c[1]}-s{c[3]}"


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def _on_fp32_side(localizer):
    """A localizer's fp64 outputs, except where its fp32 evaluation lands on the other side of a branch cut (an angle a
    period apart: no rounding moves an O(1) feature by 0.5): there the fp32 value, which is the cut's own +-pi."""
    def aligned(x, use_3d=False, pos_representation="polar"):
        hi, lo = localizer(x, use_3d, pos_representation), localizer(x.float(), use_3d, pos_representation)
        return tuple(torch.where((h - l.to(h.dtype)).abs() > 0.5, l.to(h.dtype), h) for h, l in zip(hi, lo))
    return aligned


@contextlib.contextmanager
def _frames_on_fp32_side(on):
    import s2s_locs_restatement as RL
    orig = S.augmented_localizer, RL.localizer
    if on:
        S.augmented_localizer, RL.localizer = _on_fp32_side(orig[0]), _on_fp32_side(orig[1])
    try:
        yield
    finally:
        S.augmented_localizer, RL.localizer = orig


def _aether_params(D, markov):
    p = {"num_vars": N, "input_size": 2 * D, "gpu": False, "decoder_hidden": 64, "num_edge_types": 2, "skip_first": False,
         "decoder_dropout": 0.0, "use_3d": D == 3, "encoder_dropout": 0.0, "encoder_hidden": 128, "encoder_rnn_hidden": 32,
         "encoder_rnn_type": "lstm", "encoder_mlp_num_layers": 1, "encoder_mlp_hidden": 32, "prior_num_layers": 3,
         "prior_hidden_size": 48, "pos_representation": "polar" if D == 2 else "cart", "gumbel_temp": TAU, "rff_std": 1.0}
    if markov:
        p["decoder_type"] = "ref_mlp"
    return p


def build(case, device=None):
    """The drop-in under the case's model seed, in eval mode, BatchNorm statistics away from their defaults."""
    from make_golden_dynamicvars import perturb_bn_
    kind, D, seed, _ = case
    torch.manual_seed(seed)
    if kind in ("aether_rec", "aether_markov"):
        from aether_amd.nn.seq2seq.aether import Aether
        m = Aether(_aether_params(D, kind == "aether_markov"), device=None)
    elif kind == "locs":
        import make_golden_s2s_locs as MG
        from aether_amd.nn.seq2seq.locs import LoCS
        m = LoCS(MG.model_params(N, D, False, "polar", None), device=None)
    elif kind == "charges":
        import make_golden_s2s_charges as MG
        from aether_amd.nn.seq2seq.ablations.aether_charges import AetherCharges
        m = AetherCharges(MG.model_params(N, D, False), device=None)
    else:
        from aether_amd.nn.seq2seq.dynamic_field_aether import DynamicFieldAether
        from test_s2s_dynfield_rollout import model_params
        m = DynamicFieldAether(model_params(N=N, D=D, markov=False, mlp_hidden=96), device=None)
    m = m.eval()
    with torch.no_grad():
        perturb_bn_(m)
    return m if device is None else m.to(device)


def _hidden_size(model):
    return model.state_dict()["decoder.hidden_r.weight"].shape[0]


def inputs(case, model):
    """fp32, on the CPU: the random step state and draw, and the frames and draws of predict_future."""
    kind, D, _, seed = case
    g = torch.Generator().manual_seed(seed)
    R = model.encoder.rnn_hidden_size
    inp = dict(x=torch.randn(B, N, 2 * D, generator=g),
               hidden=None if kind == "aether_markov" else torch.randn(B, N, _hidden_size(model), generator=g) * 0.2,
               state=(torch.randn(B, E, R, generator=g) * 0.2, torch.randn(B, E, R, generator=g) * 0.2),
               u=torch.rand(B, E, 2, generator=g), frames=torch.randn(B, FRAMES, N, 2 * D, generator=g),
               U=torch.rand(FRAMES - 1 + STEPS, B, E, 2, generator=g))
    if kind == "charges":
        inp["charges"] = torch.randint(0, 2, (B, N), generator=g).float() * 2 - 1
    if kind == "dynfield":
        inp["summary"] = torch.randn(B, model.graph_hidden, generator=g)
    return inp


class Restatement:
    """One model's step in `dtype`: step(x, hidden, state, u, ctx) -> (x', hidden', state', sample, logits); `ctx` is the
    charge index or the graph summary."""

    def __init__(self, case, sd32, dtype):
        self.kind, self.D = case[0], case[1]
        self.dtype, D = dtype, case[1]
        self.align = D == 3 and dtype == torch.float64
        self.sd = {k: (v.to(dtype) if v.dtype.is_floating_point else v) for k, v in sd32.items()}
        if self.kind == "locs":
            import s2s_locs_restatement as RS
            self.model = RS.Model(sd32, dtype, D == 3, "polar", 3, False, TAU)
        elif self.kind == "charges":
            import s2s_charges_restatement as RS
            self.model = RS.Model(sd32, dtype, D == 3, "polar", 3, False, TAU)
        else:
            self.enc, self.dec = _sub(self.sd, "encoder."), _sub(self.sd, "decoder.")
            self.pos = "cart" if (self.kind == "dynfield" or D == 3) else "polar"

    def context(self, inp, frames=None):
        if self.kind == "charges":
            return ((inp["charges"] + 1) / 2).long()
        if self.kind == "dynfield":
            if frames is None:
                return inp["summary"].to(self.dtype)
            return S.graph_summary(_sub(self.sd, "graph_pooler."), frames[:, :-1].transpose(2, 1).contiguous())
        return None

    def step(self, x, hidden, state, u, ctx):
        with _frames_on_fp32_side(self.align):
            return self._step(x, hidden, state, u, ctx)

    def _step(self, x, hidden, state, u, ctx):
        if self.kind == "locs":
            return self.model.step(x, hidden, state, u)
        if self.kind == "charges":
            return self.model.step(x, hidden, state, u, ctx)[:5]
        D = self.D
        field = S.film_field(self.sd, x, ctx, D) if self.kind == "dynfield" else S.predict_field(self.sd, x, D)
        logits, state = S.prior_step(self.enc, x, state, field, D == 3, self.pos, 3)
        z = S.gumbel_hard(logits.reshape(-1, 2), u.reshape(-1, 2), TAU).view(logits.shape)
        if self.kind == "aether_markov":
            from test_s2s_markov import restate
            out, hidden = restate(self.dec, x, z, field, D == 3, False), None
        else:
            out, hidden = S.decoder_step(self.dec, x, hidden, z, field, D == 3, False)
        return out, hidden, state, z, logits


def _gap(logits, u):
    score = (logits.double() - torch.log(1e-10 - torch.log(u.double() + 1e-10))) / TAU
    top = score.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


def references_from(case, sd32, inp, steps):
    """Per dtype (fp64, fp32): ([steps, B, N, 2D] states, [steps, B, E] drawn types, smallest score gap); and the
    [steps, B, N, 2D] input state of every step, from the fp64 loop.  steps == 1: the step from the random state."""
    c = lambda t, dt: None if t is None else t.to(dt)
    res = []
    with torch.no_grad(), one_thread():
        for dt in (torch.float64, torch.float32):
            rs = Restatement(case, sd32, dt)
            if steps == 1:
                ctx = rs.context(inp)
                out, _, _, z, logits = rs.step(c(inp["x"], dt), c(inp["hidden"], dt), tuple(c(t, dt) for t in inp["state"]),
                                               c(inp["u"], dt), ctx)
                res.append((out[None], z.argmax(-1)[None], _gap(logits, inp["u"]), c(inp["x"], dt)[None]))
                continue
            frames, U = c(inp["frames"], dt), c(inp["U"], dt)
            ctx = rs.context(inp, frames)
            R = inp["state"][0].shape[-1]
            hidden = None if inp["hidden"] is None else torch.zeros(B, N, inp["hidden"].shape[-1], dtype=dt)
            state = (torch.zeros(B, E, R, dtype=dt), torch.zeros(B, E, R, dtype=dt))
            gap = float("inf")
            for t in range(FRAMES - 1):
                _, hidden, state, _, logits = rs.step(frames[:, t], hidden, state, U[t], ctx)
                gap = min(gap, _gap(logits, inp["U"][t]))
            x, outs, zs, prev = frames[:, FRAMES - 1], [], [], []
            for s in range(steps):
                prev.append(x)
                x, hidden, state, z, logits = rs.step(x, hidden, state, U[FRAMES - 1 + s], ctx)
                gap = min(gap, _gap(logits, inp["U"][FRAMES - 1 + s]))
                outs.append(x)
                zs.append(z.argmax(-1))
            res.append((torch.stack(outs), torch.stack(zs), gap, torch.stack(prev)))
    (w64, z64, gap64, prev64), (w32, z32, _, _) = res
    return dict(want64=w64, want32=w32, types64=z64, types32=z32, gap=gap64, prev=prev64)


def state_of(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


@functools.lru_cache(maxsize=None)
def references(case, steps):
    """The same from a module built on the CPU under the case's seed."""
    m = build(case)
    return references_from(case, state_of(m), inputs(case, m), steps)


def check(case, steps):
    """The GPU side: the fused step (steps == 1) or predict_future, held step by step."""
    kind = case[0]
    m = build(case, "cuda")
    inp = inputs(case, m)
    ref = references_from(case, state_of(m), inp, steps)
    assert ref["gap"] >= GAP and torch.equal(ref["types64"], ref["types32"]), "choose another seed"
    cu = lambda t: None if t is None else t.cuda()
    if steps == 1:
        if kind == "charges":
            m._set_charges(((inp["charges"] + 1) / 2).long(), B, N, "cuda")
        if kind == "dynfield":
            m._set_summary(inp["summary"].cuda())
        out, _, _, edges = m._fused_step(cu(inp["x"]), cu(inp["hidden"]), tuple(cu(t) for t in inp["state"]), cu(inp["u"]))[:4]
        got, types = out[None].cpu(), edges.argmax(-1)[None].cpu()
    else:
        kw = dict(charges=inp["charges"].cuda()) if kind == "charges" else {}
        preds, edges = m.predict_future(inp["frames"].cuda(), steps, return_edges=True, uniform=inp["U"].cuda(), **kw)
        got, types = preds.transpose(0, 1).cpu(), edges.argmax(-1).transpose(0, 1).cpu()
    torch.cuda.synchronize()
    assert got.shape == ref["want64"].shape
    assert torch.equal(types, ref["types64"]), "an edge type drawn differently at a score gap of at least 1e-3"
    for t in range(steps):
        check_update(f"{case_id(case)} {'step' if steps == 1 else 'predict_future'} {t}", got[t], ref["want32"][t],
                     ref["prev"][t], ref["want64"][t])
