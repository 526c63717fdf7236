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
tests/test_update_metric.py); the kernels then have to draw them as well.

The large cases (LARGE_CASES, tests/test_gpu_s2s_split_parity.py) are the same step, of the same families and of dNRI
(tests/s2s_dnri_restatement.py), at the smallest sizes from which the dense layers leave the fp32 job kernel for the split
GEMMs.  No seed keeps thousands of Gumbel races GAP apart, so their draws are fixed against the fp64 loop alone
(`redrawing`): an edge whose race is closer than GAP gets new uniforms from the case's generator until none is.
tests/test_update_metric.py asserts, without a GPU, that the gap then holds, that at most 1 % of the edges were redrawn, that
the fp32 loop draws the fp64 loop's types and that no floor is degenerate."""
from __future__ import annotations

import contextlib
import functools
import os
import sys
from typing import NamedTuple, Optional

import torch

from conftest import REPO
from oracle import seq2seq_oracle as S
from update_cases import one_thread
from update_parity import DEGENERATE, FACTOR, check_update, update_err, update_floor

for _p in ("tools", "oracle"):
    if os.path.join(REPO, _p) not in sys.path:
        sys.path.insert(0, os.path.join(REPO, _p))

TAU, GAP = 0.5, 1e-3
FRAMES, STEPS = 2, 3


class Shape(NamedTuple):
    """The sizes of a case.  None: the width the family's small cases have.  steps: predicted steps of `predict_future` (behind
    one burn-in frame pair); redraw: the draws are fixed against the fp64 loop (`redrawing`); profile: some rows of the decoder
    hidden state and of the prior LSTM state are the K profiles of `steer_rows`."""
    B: int = 3
    N: int = 5
    he: Optional[int] = None
    hd: Optional[int] = None
    R: Optional[int] = None
    ph: Optional[int] = None
    steps: int = STEPS
    redraw: bool = False
    profile: bool = False


SMALL = Shape()
# The shapes that reach the split GEMMs (k_s2s_gemm_split / _r1, csrc/s2s_step.h; thresholds: s2s_launch_jobs): he 512, hd 256,
# rnn 128, prior hidden 256, the widths of the benchmark's seq2seq legs.  References (fp64 + fp32, one step, one thread) timed
# on the CPU the suite was written on -- see `references`.
_WIDE = dict(he=512, hd=256, R=128, ph=256, redraw=True)
LARGE = {
    # 2,280 / 2,560 edge rows, 120 / 640 nodes: the edge-level tables on 64-row tiles, ragged last tile (2,280 = 35 x 64 + 40)
    "e2280": Shape(B=6, N=20, steps=2, **_WIDE),
    "e2560": Shape(B=128, N=5, steps=2, **_WIDE),
    # 4,035 nodes (63 x 64 + 3), 8,070 edges (63 x 128 + 6): every node-level table split (the output MLP, 256 wide, needs more
    # than 4,032 rows), and the message table of four 256-wide jobs on 128-row tiles (64 x 8 = 512 workgroups)
    "n4035": Shape(B=1345, N=3, **_WIDE),
    "n4035-rows": Shape(B=1345, N=3, profile=True, **_WIDE),
}
# (kind, D, model seed, input seed)
KINDS = ("aether_rec", "aether_markov", "locs", "charges", "dynfield")
SEEDS = {("aether_rec", 2): 7, ("aether_markov", 2): 7, ("dynfield", 2): 8}           # every other case: 5
CASES = [(kind, D, 61, SEEDS.get((kind, D), 5)) for kind in KINDS for D in (2, 3)]
TYPICAL = 5e-8
# (kind, D, model seed, input seed, key of LARGE); every family on the 64-row tiles, the recurrent Aether on all of them
LARGE_KINDS = KINDS + ("dnri_rec", "dnri_mlp")
LARGE_CASES = [(kind, 2, 61, 5, "e2280") for kind in LARGE_KINDS] + \
              [("aether_rec", 3, 61, 5, "e2560"), ("aether_rec", 2, 61, 5, "n4035"), ("aether_rec", 2, 61, 5, "n4035-rows")]
ROLLOUT_CASES = [c for c in LARGE_CASES if c[0] == "aether_rec" and c[4] in ("e2280", "e2560")]
MAX_REDRAWN = 0.01


def shape_of(c):
    return LARGE[c[4]] if len(c) > 4 else SMALL


def case_id(c):
    return f"{c[0]}-D{c[1]}-s{c[3]}" + (f"-{c[4]}" if len(c) > 4 else "")


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


def _widths(shape):
    """The params entries a Shape sets (none for the small cases: every family keeps its own widths)."""
    names = (("encoder_hidden", shape.he), ("decoder_hidden", shape.hd), ("encoder_rnn_hidden", shape.R),
             ("prior_hidden_size", shape.ph))
    return {k: v for k, v in names if v is not None}


def _aether_params(D, markov, shape=SMALL):
    p = {"num_vars": shape.N, "input_size": 2 * D, "gpu": False, "decoder_hidden": 64, "num_edge_types": 2, "skip_first": False,
         "decoder_dropout": 0.0, "use_3d": D == 3, "encoder_dropout": 0.0, "encoder_hidden": 128, "encoder_rnn_hidden": 32,
         "encoder_rnn_type": "lstm", "encoder_mlp_num_layers": 1, "encoder_mlp_hidden": 32, "prior_num_layers": 3,
         "prior_hidden_size": 48, "pos_representation": "polar" if D == 2 else "cart", "gumbel_temp": TAU, "rff_std": 1.0}
    p.update(_widths(shape))
    if markov:
        p["decoder_type"] = "ref_mlp"
    return p


def build(case, device=None):
    """The drop-in under the case's model seed, in eval mode, BatchNorm statistics away from their defaults."""
    from make_golden_dynamicvars import perturb_bn_
    kind, D, seed = case[:3]
    shape = shape_of(case)
    N, wide = shape.N, _widths(shape)
    torch.manual_seed(seed)
    if kind in ("aether_rec", "aether_markov"):
        from aether_amd.nn.seq2seq.aether import Aether
        m = Aether(_aether_params(D, kind == "aether_markov", shape), device=None)
    elif kind == "locs":
        import make_golden_s2s_locs as MG
        from aether_amd.nn.seq2seq.locs import LoCS
        m = LoCS(MG.model_params(N, D, False, "polar", None, wide or None), device=None)
    elif kind == "charges":
        import make_golden_s2s_charges as MG
        from aether_amd.nn.seq2seq.ablations.aether_charges import AetherCharges
        m = AetherCharges(MG.model_params(N, D, False, wide or None), device=None)
    elif kind in ("dnri_rec", "dnri_mlp"):
        import make_golden_s2s_dnri as MG
        from aether_amd.nn.seq2seq.dnri import DNRI
        m = DNRI(MG.model_params(N, D, False, MG.DECODERS[kind[5:]], wide or None), device=None)
    else:
        from aether_amd.nn.seq2seq.dynamic_field_aether import DynamicFieldAether
        from test_s2s_dynfield_rollout import model_params
        # (the FiLM net's hidden layers have a weight image, and so a split GEMM, from 128 columns on)
        m = DynamicFieldAether(model_params(N=N, D=D, markov=False, mlp_hidden=128 if wide else 96, **wide), device=None)
    m = m.eval()
    with torch.no_grad():
        perturb_bn_(m)
    return m if device is None else m.to(device)


def _hidden_size(model):
    return model.state_dict()["decoder.hidden_r.weight"].shape[0]


STATELESS = ("aether_markov", "dnri_mlp")          # decoders without a hidden state
# The rows of `steer_rows`, by what their K profile does to the running row scale of the split GEMMs (csrc/s2s_step.h,
# x_settle: one power of two per row, set from the first 32 k so that their maximum lands in [2^13, 2^14), clamped to
# 2^+-40; lowered, and the accumulators rescaled, when a later block of 32 times the scale reaches 2^15)
PROFILES = ("zero_first", "tiny_first", "growing", "shrinking", "all_zero")
STATE_LEVELS = (0.0, 1e-3, 0.3, 0.99)


def steer_rows(hidden, state, g):
    """In place: node rows 7 p + 3 of the decoder hidden state [B N][hd] take profile p of PROFILES along K (O(1) noise times:
    zero / 1e-4 in the first 32 entries; x 4 per block of 32; / 4 per block; zero everywhere), five rows each; edge rows
    11 l + 5 (strides of 35 and 44 rows) of both prior LSTM states [B E][R] take magnitude STATE_LEVELS[l] (zero: what the first burn-in step has; h of
    an LSTM is inside (-1, 1)), five rows each.  -> {profile or level: row indices}."""
    rows = {}
    H = hidden.view(-1, hidden.shape[-1])
    blocks = torch.arange(H.shape[1]) // 32
    for p, name in enumerate(PROFILES):
        idx = torch.arange(5) * 7 * len(PROFILES) + 7 * p + 3
        # magnitudes in [1, 2): every block of 32 has its maximum in the binade its factor puts it in
        noise = (1 + torch.rand(5, H.shape[1], generator=g)) * (torch.randint(0, 2, (5, H.shape[1]), generator=g) * 2 - 1)
        scale = {"zero_first": (blocks > 0).float(), "tiny_first": torch.where(blocks > 0, 1.0, 1e-4),
                 "growing": 4.0 ** (blocks - int(blocks.max())).float(), "shrinking": 4.0 ** (-blocks).float(),
                 "all_zero": torch.zeros(H.shape[1])}[name]
        H[idx] = noise * scale
        rows[name] = idx
    for t in state:
        T = t.view(-1, t.shape[-1])
        for l, level in enumerate(STATE_LEVELS):
            idx = torch.arange(5) * 11 * len(STATE_LEVELS) + 11 * l + 5
            T[idx] = (torch.rand(5, T.shape[1], generator=g) * 2 - 1) * level
            rows[level] = idx
    return rows


def row_scale_walk(row):
    """What x_settle does with one row of X along K, restated on the host: -> (the scale the first block of 32 sets, the
    number of later blocks at which the row lowers its scale)."""
    def scale_for(m):
        if m == 0.0:
            return 2.0 ** 40
        e = int(torch.tensor(m, dtype=torch.float32).log2().floor())           # biased exponent - 127
        return 2.0 ** max(-40, min(40, 13 - e))
    blocks = row.float().abs().view(-1, 32).max(1).values.tolist()
    first = xs = scale_for(blocks[0])
    lowered = 0
    for m in blocks[1:]:
        if m * xs >= 32768.0:
            xs, lowered = min(xs, scale_for(m)), lowered + 1
    return first, lowered


def inputs(case, model):
    """fp32, on the CPU: the random step state and draw, and the frames and draws of predict_future.  `gen`: the generator
    behind them, for the draws `redrawing` replaces."""
    kind, D, seed = case[0], case[1], case[3]
    shape = shape_of(case)
    B, N = shape.B, shape.N
    E = N * (N - 1)
    g = torch.Generator().manual_seed(seed)
    R = model.encoder.rnn_hidden_size
    inp = dict(x=torch.randn(B, N, 2 * D, generator=g),
               hidden=None if kind in STATELESS else torch.randn(B, N, _hidden_size(model), generator=g) * 0.2,
               state=(torch.randn(B, E, R, generator=g) * 0.2, torch.randn(B, E, R, generator=g) * 0.2),
               u=torch.rand(B, E, 2, generator=g), frames=torch.randn(B, FRAMES, N, 2 * D, generator=g),
               U=torch.rand(FRAMES - 1 + shape.steps, B, E, 2, generator=g))
    if kind == "charges":
        inp["charges"] = torch.randint(0, 2, (B, N), generator=g).float() * 2 - 1
    if kind == "dynfield":
        inp["summary"] = torch.randn(B, model.graph_hidden, generator=g)
    if shape.profile:
        inp["rows"] = steer_rows(inp["hidden"], inp["state"], g)
    inp["gen"] = g
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
        elif self.kind in ("dnri_rec", "dnri_mlp"):
            import s2s_dnri_restatement as RS
            self.model = RS.Model(sd32, dtype, 3, False, TAU)
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
        if self.kind in ("locs", "dnri_rec", "dnri_mlp"):
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


def _gaps(logits, u):
    """Per edge: the distance between the two largest scores of the hard Gumbel sample (oracle gumbel_hard), in fp64."""
    score = (logits.double() - torch.log(1e-10 - torch.log(u.double() + 1e-10))) / TAU
    top = score.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


def _gap(logits, u):
    return float(_gaps(logits, u).min())


@contextlib.contextmanager
def redrawing(gen, fixed):
    """Inside, every hard Gumbel sample of the oracle first redraws, from `gen`, the uniforms of the edges whose two largest
    scores are closer than GAP, until none is, and samples with those.  It is put around the fp64 loop alone: among
    thousands of random draws some race is always closer than any rounding, and which ones is decided by the reference, never
    by the code under test.  Per sample, (the fp32 draws used [rows][K], the rows redrawn [rows]) is appended to `fixed`."""
    orig = S.gumbel_hard

    def sample(logits, uniform, tau):
        assert tau == TAU
        u = uniform.float().clone()                      # (the draws are fp32 values, cast by the restatements)
        ever = torch.zeros(u.shape[0], dtype=torch.bool)
        close = _gaps(logits, u) < GAP
        while bool(close.any()):
            ever |= close
            u[close] = torch.rand(int(close.sum()), u.shape[1], generator=gen)
            close = _gaps(logits, u) < GAP
        fixed.append((u, ever))
        return orig(logits, u.to(uniform.dtype), tau)

    S.gumbel_hard = sample
    try:
        yield
    finally:
        S.gumbel_hard = orig


def references_from(case, sd32, inp, steps):
    """Per dtype (fp64, fp32): ([steps, B, N, 2D] states, [steps, B, E] drawn types, smallest score gap); and the
    [steps, B, N, 2D] input state of every step, from the fp64 loop.  steps == 1: the step from the random state, and
    `held64` / `held32`: the tensors of that step the update does not see (decoder hidden state, prior h and c, logits).
    A case with `redraw` has its draws fixed along the fp64 loop (`redrawing`), step after step; `inp`: the inputs with the
    draws both loops, and then the device, take; `redrawn`: the largest share of a step's edges that were redrawn."""
    shape = shape_of(case)
    B, N = shape.B, shape.N
    E = N * (N - 1)
    c = lambda t, dt: None if t is None else t.to(dt)
    inp = dict(inp)
    res, held, redrawn = [], [], 0.0
    with torch.no_grad(), one_thread():
        for dt in (torch.float64, torch.float32):
            rs = Restatement(case, sd32, dt)
            fixed = []
            fix = redrawing(inp["gen"], fixed) if shape.redraw and dt == torch.float64 else contextlib.nullcontext()
            if steps == 1:
                ctx = rs.context(inp)
                with fix:
                    out, hid, st, z, logits = rs.step(c(inp["x"], dt), c(inp["hidden"], dt),
                                                      tuple(c(t, dt) for t in inp["state"]), c(inp["u"], dt), ctx)
                if fixed:
                    inp["u"], redrawn = fixed[0][0].view(B, E, 2), float(fixed[0][1].float().mean())
                res.append((out[None], z.argmax(-1)[None], _gap(logits, inp["u"]), c(inp["x"], dt)[None]))
                held.append(dict(hidden=hid, h=st[0], c=st[1], logits=logits))
                continue
            frames, U = c(inp["frames"], dt), c(inp["U"], dt)
            ctx = rs.context(inp, frames)
            R = inp["state"][0].shape[-1]
            hidden = None if inp["hidden"] is None else torch.zeros(B, N, inp["hidden"].shape[-1], dtype=dt)
            state = (torch.zeros(B, E, R, dtype=dt), torch.zeros(B, E, R, dtype=dt))
            gaps = []
            with fix:
                for t in range(FRAMES - 1):
                    _, hidden, state, _, logits = rs.step(frames[:, t], hidden, state, U[t], ctx)
                    gaps.append(logits)
                x, outs, zs, prev = frames[:, FRAMES - 1], [], [], []
                for s in range(steps):
                    prev.append(x)
                    x, hidden, state, z, logits = rs.step(x, hidden, state, U[FRAMES - 1 + s], ctx)
                    gaps.append(logits)
                    outs.append(x)
                    zs.append(z.argmax(-1))
            if fixed:
                assert len(fixed) == FRAMES - 1 + steps
                inp["U"] = torch.stack([u.view(B, E, 2) for u, _ in fixed])
                redrawn = max(float(ever.float().mean()) for _, ever in fixed)
            gap = min(_gap(l, inp["U"][t]) for t, l in enumerate(gaps))
            res.append((torch.stack(outs), torch.stack(zs), gap, torch.stack(prev)))
    (w64, z64, gap64, prev64), (w32, z32, _, _) = res
    ref = dict(want64=w64, want32=w32, types64=z64, types32=z32, gap=gap64, prev=prev64, inp=inp, redrawn=redrawn)
    if held:
        ref["held64"], ref["held32"] = held
    return ref


HELD = ("hidden", "h", "c", "logits")
ONE_ROUNDING = 2.0 ** -24


def held_figure(got, want64):
    return float((got.detach().cpu().double() - want64).abs().max() / want64.abs().max())


def step_bars(what, ref, out, types, held):
    """Every bar a large case's step is held to, printed: -> {name: (err, floor, passed)}.  `update`: tests/update_parity.py
    on the state; `types`: every sampled edge type the fp64 loop's; the tensors the update does not see (`held`: name ->
    tensor or None), max|got - want64| / max|want64| against FACTOR x the same figure of the fp32 restatement, which is never
    taken below one rounding."""
    bars = {}
    err = update_err(out, ref["prev"][0], ref["want64"][0])
    floor = update_floor(ref["want32"][0], ref["prev"][0], ref["want64"][0])
    bars["update"] = (err, floor, floor >= DEGENERATE and err <= FACTOR * floor)
    flipped = float((types.cpu() != ref["types64"][0]).float().mean())
    bars["types"] = (flipped, 0.0, flipped == 0.0)
    for name in HELD:
        if held.get(name) is None:
            continue
        err = held_figure(held[name], ref["held64"][name])
        floor = max(held_figure(ref["held32"][name], ref["held64"][name]), ONE_ROUNDING)
        bars[name] = (err, floor, err <= FACTOR * floor)
    for name, (err, floor, ok) in bars.items():
        print(f"split-parity {what} {name}: err={err:.3e} floor={floor:.3e} ratio={err / max(floor, 1e-300):.2f}"
              + ("" if ok else "  MISSED"))
    return bars


@contextlib.contextmanager
def split_layer(weights, drop=None):
    """Inside, every F.linear of the oracle whose weight is one of `weights` (the tensors themselves) is computed as the
    split GEMMs compute it (csrc/s2s_step.h): the weight in two fp16 pieces as it is, every row of x times a power of two that
    puts its maximum into [2^13, 2^14) in two fp16 pieces, w_hi x_hi + w_hi x_lo + w_lo x_hi, an fp32 result.  `drop`: one
    of update_cases.TERMS is left out."""
    import torch.nn.functional as F

    def pieces(t):
        hi = t.half()
        return hi.double(), (t - hi.float()).half().double()

    class Patched:
        def __getattr__(self, name):
            return getattr(F, name)

        @staticmethod
        def linear(x, w, b=None):
            if not any(w is t for t in weights):
                return F.linear(x, w, b)
            x32 = x.float()
            m = x32.abs().amax(-1, keepdim=True)
            s = torch.where(m > 0, 2.0 ** (13 - torch.floor(torch.log2(m.clamp(min=1e-30)))), torch.ones_like(m))
            (wh, wl), (xh, xl) = pieces(w.float()), pieces(x32 * s)
            acc = xh @ wh.T
            if drop != "w_hi*x_lo":
                acc = acc + xl @ wh.T
            if drop != "w_lo*x_hi":
                acc = acc + xh @ wl.T
            y = (acc / s.double()).float()
            return (y if b is None else y + b.float()).to(x.dtype)

    orig = S.F
    S.F = Patched()
    try:
        yield
    finally:
        S.F = orig


def state_of(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


@functools.lru_cache(maxsize=None)
def references(case, steps):
    """The same from a module built on the CPU under the case's seed; computed once per process and shared (the three GEMM
    structures of tests/test_gpu_s2s_split_parity.py take the same references).  Seconds for the fp64 + fp32 restatements of
    the large cases on one CPU thread, one step / burn-in + two predicted steps: e2280 aether_rec 1.7 / 4.5, aether_markov
    1.7, locs 1.1, charges 4.0, dynfield 2.0, dnri_rec 0.7, dnri_mlp 0.6; e2560 (D 3) aether_rec 3.1 / 7.1; n4035 6.8;
    n4035-rows 6.2.  (he 512 / hd 256 at 16,720 rows takes 9.5 s and at 48,400 rows 27 s: not used.)"""
    m = build(case)
    return references_from(case, state_of(m), inputs(case, m), steps)


def check(case, steps):
    """The GPU side: the fused step (steps == 1) or predict_future, held step by step."""
    kind = case[0]
    B, N = shape_of(case).B, shape_of(case).N
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
