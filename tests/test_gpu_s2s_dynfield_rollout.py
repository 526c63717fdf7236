"""The seq2seq DynamicFieldAether on the fused step with the FiLM field query inside (aether_s2s_dynfield_step / _rollout):
the in-step field, the step and the rollout against the fp64 oracle (oracle/seq2seq_oracle.py; the Markov decoder against the
restatement of tests/test_s2s_markov.py), the device rollout against the step-by-step loop, graph replay, sequence and weight
updates, and the argument checks of the entries.  Bars: TOL = 1e-5 scale-relative, 2 * TOL wherever the FiLM field is involved
(as test_gpu_seq2seq.test_dynamic_field_variant_vs_oracle has it for that quantity)."""
import contextlib
import ctypes as C
import os
import re

import pytest
import torch

from conftest import REPO, scale_rel_err
from oracle import seq2seq_oracle as S
from test_s2s_dynfield_rollout import model_params
from test_s2s_markov import restate

pytestmark = pytest.mark.gpu
TOL = 1e-5
TAU = 0.5


def _model(seed, **kw):
    from aether_amd.nn.seq2seq.dynamic_field_aether import DynamicFieldAether
    torch.manual_seed(seed)
    model = DynamicFieldAether(model_params(**kw), device=None).eval()
    sd64 = {k: v.detach().double() for k, v in model.state_dict().items()}
    return model.cuda(), sd64


@contextlib.contextmanager
def _frames_as_fp32(use_3d):
    """The fp64 oracle with the local frames of a 3-D step built in fp32 (then cast), as test_s2s_markov.restate's
    ``frames_dtype``: in 3-D every node's origin edge has an Euler angle on its branch cut, +-pi by ONE rounding, and the frames
    enter the layers linearly -- an fp64 evaluation of an fp32 input lands on either side of the cut where the reference's own
    fp32 evaluation lands on one (measured on the CPU for the data of test_step_vs_oracle_with_a_full_job_table[3-4-False]:
    prior state of the fp32 oracle vs the fp64 oracle 0.84 scale-relative, vs the fp64 oracle on fp32 frames 1.5e-6).  That is
    no rounding of the step; the step is held to the side the reference's fp32 evaluation takes."""
    orig = S.augmented_localizer
    if use_3d:
        S.augmented_localizer = lambda x, use_3d=False, pos_representation="polar": tuple(
            t.to(x.dtype) for t in orig(x.float(), use_3d, pos_representation))
    try:
        yield
    finally:
        S.augmented_localizer = orig


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def _state(model, B, N, g, scale=0.2):
    """A random step state (x, decoder hidden or None, (h, c)), a summary and one step's draws, on the CPU in fp32."""
    D, K = model.num_dims, model.num_edge_types
    E, R = N * (N - 1), model.encoder.rnn_hidden_size
    x = torch.randn(B, N, 2 * D, generator=g)
    dh = None if model._markov else torch.randn(B, N, model.decoder.msg_out_shape, generator=g) * scale
    hc = (torch.randn(B, E, R, generator=g) * scale, torch.randn(B, E, R, generator=g) * scale)
    summary = torch.randn(B, model.graph_hidden, generator=g)
    u = torch.rand(B, E, K, generator=g)
    return x, dh, hc, summary, u


def _cuda(t):
    return None if t is None else tuple(v.cuda() for v in t) if isinstance(t, tuple) else t.cuda()


def _oracle_step(model, sd64, x, dh, hc, summary, u, edges=None):
    """One step in fp64: film_field -> prior_step -> gumbel_hard -> decoder step -> (out, dh', (h', c'), sample, the two
    largest Gumbel scores' gap per edge).  ``edges``: decode with this sample instead of the oracle's own."""
    D, K = model.num_dims, model.num_edge_types
    skip = model.decoder.skip_first_edge_type
    x, hc, summary, u = x.double(), tuple(v.double() for v in hc), summary.double(), u.double()
    field = S.film_field(sd64, x, summary, D)
    with _frames_as_fp32(D == 3):
        logits, hc1 = S.prior_step(_sub(sd64, "encoder."), x, hc, field, D == 3, model.encoder.pos_representation, 3)
    z = S.gumbel_hard(logits.reshape(-1, K), u.reshape(-1, K), TAU).view(logits.shape)
    score = (logits - torch.log(1e-10 - torch.log(u + 1e-10))) / TAU
    top = score.topk(2, dim=-1).values
    gap = top[..., 0] - top[..., 1]
    w = z if edges is None else edges.double()
    dec = _sub(sd64, "decoder.")
    if model._markov:
        out, dh1 = restate(dec, x, w, field, D == 3, skip, frames_dtype=torch.float32 if D == 3 else None), None
    else:
        with _frames_as_fp32(D == 3):
            out, dh1 = S.decoder_step(dec, x, dh.double(), w, field, D == 3, skip)
    return out, dh1, hc1, z, gap, field


def _check_step(model, sd64, B, N, g):
    """The fused step with the field query inside against the fp64 composition.  A sampled edge type must equal the oracle's
    wherever the oracle's two largest Gumbel scores are further apart than rounding can move them (1e-3: a hundred times
    the 2 * TOL the logits are held to, divided by tau); the decoder half is compared on the sample the step drew."""
    x, dh, hc, summary, u = _state(model, B, N, g)
    model._set_summary(summary.cuda())
    out, dh1, (h1, c1), edges, field = model._fused_step(x.cuda(), _cuda(dh), _cuda(hc), u.cuda(), None, return_field=True)
    want_out, want_dh, (wh, wc), z, gap, want_field = _oracle_step(model, sd64, x, dh, hc, summary, u, edges=edges.cpu())
    assert scale_rel_err(field.cpu(), want_field) <= 2 * TOL
    assert scale_rel_err(h1.cpu(), wh) <= 2 * TOL and scale_rel_err(c1.cpu(), wc) <= 2 * TOL
    clear = gap > 1e-3
    assert clear.float().mean() > 0.9
    assert torch.equal(edges.cpu().argmax(-1)[clear], z.argmax(-1)[clear])
    assert scale_rel_err(out.cpu(), want_out) <= 2 * TOL
    if want_dh is not None:
        assert scale_rel_err(dh1.cpu(), want_dh) <= 2 * TOL
    return field


# -- 1. the field the step computes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", [(1, 3), (7, 5), (3, 7)])       # graphs of 5 / 7 rows straddle the 16- and 32-row tiles, last tile ragged
@pytest.mark.parametrize("MH", [128, 96, 48])                   # 128: the plan holds split images; 96, 48: none
@pytest.mark.parametrize("D", [2, 3])
def test_in_step_field_vs_oracle(D, MH, B, N):
    model, sd64 = _model(40 + D, N=N, D=D, markov=False, mlp_hidden=MH)
    g = torch.Generator().manual_seed(100 * B + N + MH)
    x, dh, hc, summary, u = _state(model, B, N, g)
    model._set_summary(summary.cuda())
    field = model._fused_step(x.cuda(), dh.cuda(), _cuda(hc), u.cuda(), None, return_field=True)[4]
    assert field.shape == (B, N, D)
    assert scale_rel_err(field.cpu(), S.film_field(sd64, x.double(), summary.double(), D)) <= 2 * TOL
    # and it is the field of the standalone query to rounding
    alone, _ = model.predict_field(x.cuda(), summary.cuda())
    assert scale_rel_err(field.cpu(), alone.cpu()) <= 2 * TOL


# -- 2. the full launch table -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,skip", [(4, False), (3, True)])      # K = 4: eight decoder jobs fill the table, the field job forces the flush
@pytest.mark.parametrize("D", [2, 3])
def test_step_vs_oracle_with_a_full_job_table(D, K, skip):
    model, sd64 = _model(50 + K, N=5, D=D, markov=False, mlp_hidden=96, num_edge_types=K, skip_first=skip)
    _check_step(model, sd64, 7, 5, torch.Generator().manual_seed(7 + K))


# -- 3. device rollout against the step-by-step loop ---------------------------------------------------------------------------
def _stepwise_from_state(model, x, dh, hc, summary, steps, U):
    preds, edges = [], []
    for t in range(steps):
        field, _ = model.predict_field(x, summary)
        x, dh, hc, e = model._fused_step(x, dh, hc, U[t], field)
        preds.append(x); edges.append(e)
    return torch.stack(preds, 1), torch.stack(edges, 1)


@pytest.mark.parametrize("steps", [1, 5])
@pytest.mark.parametrize("T0", [0, 1, 6])
def test_rollout_equals_stepwise_and_graph_replay(T0, steps):
    B, N, D = 3, 5, 3
    model, _ = _model(60, N=N, D=D, markov=False, mlp_hidden=96)
    g = torch.Generator().manual_seed(61 + T0)
    U = torch.rand(T0 + steps, B, N * (N - 1), 2, generator=g).cuda()
    if T0 == 0:            # no burn-in: the loop from a given state and a given summary (predict_future refuses a single
                           # frame, which leaves nothing to summarise: test_s2s_dynfield_rollout.test_what_stays_refused)
        x, dh, hc, summary, _ = (_cuda(t) for t in _state(model, B, N, g))
        want, want_e = _stepwise_from_state(model, x, dh, hc, summary, steps, U)
        run = lambda graph: model.predict_from_state(x, dh, hc, summary, steps, uniform=U, return_edges=True, graph=graph)
    else:
        inputs = torch.randn(B, T0 + 1, N, 2 * D, generator=g).cuda()
        want, want_e = model.predict_future_stepwise(inputs, steps, return_edges=True, uniform=U)
        run = lambda graph: model.predict_future(inputs, steps, return_edges=True, uniform=U, graph=graph)
    got, got_e = run(False)
    assert got.shape == (B, steps, N, 2 * D)
    assert torch.equal(got_e, want_e)
    assert scale_rel_err(got.cpu(), want.cpu()) <= 2 * TOL
    rep, rep_e = run(True)
    assert torch.equal(rep, got) and torch.equal(rep_e, got_e)
    assert len(model._runners) == 1
    if T0 > 0:             # no burn-in field handed in (the C entry's NULL): every burn-in step queries its own
        dh0, hc0 = model._start(inputs)
        own, own_e, _ = model._fused_rollout(inputs[:, :T0], inputs[:, T0], dh0, hc0, steps, U, True, batched_burn_in=False)
        assert torch.equal(own_e, want_e)
        assert scale_rel_err(own.cpu(), want.cpu()) <= 2 * TOL


# -- 4. device rollout against the fp64 oracle ---------------------------------------------------------------------------------
def test_rollout_vs_fp64_oracle():
    """D = 3, B = 8, N = 5, six frames (five burn-in steps), four prediction steps.  Trajectories are compared on the graphs
    whose samples all agree with the oracle's, which must be at least 0.9 of them.  The seed (model 21, data 22) was checked on
    the CPU: the oracle run in fp32 agrees with the oracle run in fp64 on every sample of every graph (8 of 8, predictions
    6.3e-8 apart scale-relative) -- the reference's own flip rate for this input is zero -- when both take the local frames
    from fp32 (_frames_as_fp32; 8 of 8 and 6.8e-8 as well when both take them from fp64).  With the frames in each run's own
    precision the 3-D oracle agrees with itself on 0 of 8 graphs, for this and every other seed tried (20 - 29): that is the
    branch cut _frames_as_fp32 describes, no sampling flip."""
    D, B, N, T, steps, seed = 3, 8, 5, 6, 4, 21
    model, sd64 = _model(seed, N=N, D=D, markov=False, mlp_hidden=96)
    g = torch.Generator().manual_seed(seed + 1)
    inputs = torch.randn(B, T, N, 2 * D, generator=g)
    U = torch.rand(T - 1 + steps, B * N * (N - 1), 2, generator=g)
    with _frames_as_fp32(True):
        want, want_e = S.predict_future_dynamic_field(sd64, inputs.double(), steps, U.double(), TAU, True, "cart", 3,
                                                      return_edges=True)
    got, got_e = model.predict_future(inputs.cuda(), steps, return_edges=True, uniform=U.cuda().view(-1, B, N * (N - 1), 2))
    ok = (got_e.cpu().argmax(-1) == want_e.argmax(-1)).reshape(B, -1).all(dim=1)
    assert ok.float().mean() >= 0.9
    assert scale_rel_err(got.cpu()[ok], want[ok]) <= 2 * TOL


# -- 5. a second sequence, changed weights ---------------------------------------------------------------------------------------
def test_second_sequence_and_weight_update_with_graph_replay():
    B, N, D, T, steps = 3, 5, 3, 4, 3
    g = torch.Generator().manual_seed(71)
    seqs = [torch.randn(B, T, N, 2 * D, generator=g).cuda() for _ in range(2)]
    U = torch.rand(T - 1 + steps, B, N * (N - 1), 2, generator=g).cuda()
    model, _ = _model(70, N=N, D=D, markov=False, mlp_hidden=128)
    first = model.predict_future(seqs[0], steps, uniform=U, graph=True)
    mod = model._mod_buf[(B, "cuda:0")]
    mod_ptr, mod_before = mod.data_ptr(), mod.clone()
    second = model.predict_future(seqs[1], steps, uniform=U, graph=True)          # new summary: modulation rewritten in place
    assert len(model._runners) == 1 and model._mod_buf[(B, "cuda:0")].data_ptr() == mod_ptr
    assert not torch.equal(model._mod_buf[(B, "cuda:0")], mod_before)
    fresh, _ = _model(70, N=N, D=D, markov=False, mlp_hidden=128)
    assert torch.equal(second, fresh.predict_future(seqs[1], steps, uniform=U))
    assert not torch.equal(first, second)
    # the next call follows changed weights: the plan (it holds linear_1's image) is rebuilt, the captured runner dropped
    runner = next(iter(model._runners.values()))
    plan_key = model._plan_cache[0]
    with torch.no_grad():
        model.film_net.linear_1.weight.mul_(1.5)
        fresh.film_net.linear_1.weight.mul_(1.5)
    third = model.predict_future(seqs[1], steps, uniform=U, graph=True)
    assert model._plan_cache[0] != plan_key and next(iter(model._runners.values())) is not runner
    assert torch.equal(third, fresh.predict_future(seqs[1], steps, uniform=U)) and not torch.equal(third, second)


# -- 6. the Markov decoder ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,K,skip", [(2, 2, False), (3, 3, True)])
def test_markov_step_and_rollout(D, K, skip):
    B, N, T, steps = 3, 5, 4, 3
    model, sd64 = _model(80 + D, N=N, D=D, markov=True, mlp_hidden=96, num_edge_types=K, skip_first=skip)
    g = torch.Generator().manual_seed(81)
    _check_step(model, sd64, B, N, g)                                    # restate + film_field + prior_step in fp64
    inputs = torch.randn(B, T, N, 2 * D, generator=g).cuda()
    U = torch.rand(T - 1 + steps, B, N * (N - 1), K, generator=g).cuda()
    got, got_e = model.predict_future(inputs, steps, return_edges=True, uniform=U)
    want, want_e = model.predict_future_stepwise(inputs, steps, return_edges=True, uniform=U)
    assert torch.equal(got_e, want_e) and scale_rel_err(got.cpu(), want.cpu()) <= 2 * TOL
    rep = model.predict_future(inputs, steps, uniform=U, graph=True)
    assert torch.equal(rep, got)
    # the rollout against the fp64 composition: the burn-in chains the prior step alone (no decoder runs), then every
    # prediction step is film_field -> prior_step -> restate on the sample the rollout drew, chained on the oracle's own output
    summary = model.graph_pooler(inputs[:, :-1].transpose(2, 1).contiguous())
    s64 = summary.cpu().double()
    R, E = model.encoder.rnn_hidden_size, N * (N - 1)
    hc = (torch.zeros(B, E, R, dtype=torch.float64), torch.zeros(B, E, R, dtype=torch.float64))
    for t in range(T - 1):
        xt = inputs[:, t].cpu().double()
        with _frames_as_fp32(D == 3):
            _, hc = S.prior_step(_sub(sd64, "encoder."), xt, hc, S.film_field(sd64, xt, s64, D), D == 3, "cart", 3)
    z = lambda: torch.zeros(B, E, R, device="cuda")
    _, _, (_, (h, c)) = model._fused_rollout(inputs[:, :T - 1], inputs[:, T - 1], None, (z(), z()), 1, U[:T], False)
    x = inputs[:, T - 1].cpu().double()
    for t in range(steps):
        x, _, hc, zs, gap, _ = _oracle_step(model, sd64, x, None, hc, s64, U[T - 1 + t].cpu(), edges=got_e[:, t].cpu())
        clear = gap > 1e-3
        assert torch.equal(got_e[:, t].cpu().argmax(-1)[clear], zs.argmax(-1)[clear])
        assert scale_rel_err(got[:, t].cpu(), x) <= 2 * TOL
        if t == 0:             # the prior state the burn-in and one more step leave
            assert scale_rel_err(h.cpu(), hc[0]) <= 2 * TOL and scale_rel_err(c.cpu(), hc[1]) <= 2 * TOL
    # predict_from_state continues a rollout: the tail of predict_future
    _, _, (_, (h2, c2)) = model._fused_rollout(inputs[:, :T - 1], inputs[:, T - 1], None, (z(), z()), 2, U[:T + 1], False)
    tail = model.predict_from_state(got[:, 1], None, (h2, c2), summary, steps - 2, uniform=U[T + 1:])
    assert torch.equal(tail, got[:, 2:])
    loss = model.calculate_loss(inputs, is_train=False, uniform=U[:T - 1])
    assert len(loss) == 3 and torch.isfinite(loss[0])


# -- 7. what the entries reject ------------------------------------------------------------------------------------------------------
def _codes():
    header = open(os.path.join(REPO, "include", "aether_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"#define (AETHER_E\w+) \((-\d+)\)", header)}


@pytest.fixture(scope="module")
def entry_calls():
    """call(entry, **defect) -> status of aether_s2s_dynfield_step / _rollout on real, correctly sized device buffers (the
    defect-free call succeeds); each defect changes one argument that the check must catch before anything is launched."""
    from aether_amd import _lib
    lib = _lib.load()
    B, N, D, T0, steps = 2, 3, 2, 1, 2
    model, _ = _model(90, N=N, D=D, markov=False, mlp_hidden=48)
    E, K, R, HD = N * (N - 1), 2, model.encoder.rnn_hidden_size, model.decoder.msg_out_shape
    g = torch.Generator().manual_seed(91)
    mod = model._set_summary(torch.randn(B, model.graph_hidden, generator=g).cuda())
    _, plan, ws, graph, (pf, pe, pd), scal, _ = model._step_common(B, N, torch.device("cuda:0"))
    model_markov = _model(90, N=N, D=D, markov=True, mlp_hidden=48)[0]
    mp = model_markov.decoder._param_struct()
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device="cuda")
    x, burn, dh, h, c = z(B, N, 2 * D), z(T0, B, N, 2 * D), z(B, N, HD), z(B, E, R), z(B, E, R)
    u = torch.full((T0 + steps, B, E, K), 0.5, device="cuda")
    out = dict(x1=z(B, N, 2 * D), dh1=z(B, N, HD), h1=z(B, E, R), c1=z(B, E, R), e1=z(B, E, K), preds=z(steps, B, N, 2 * D))
    p = lambda t: t.data_ptr()
    head, film = scal[:13], scal[13:]                   # (... n_nodes, n_edges), (mlp_hidden, mod, mod_bytes, batch, num_objects)
    assert film == (48, p(mod), mod.numel() * 4, B, N)
    keep = (model, model_markov, plan, ws, graph, pf, pe, pd, mp, mod, x, burn, dh, h, c, u, out)

    def call(entry, mod_ptr=p(mod), mod_bytes=mod.numel() * 4, n_nodes=B * N, ws_bytes=ws.numel(), markov=None):
        sc = head[:11] + (n_nodes, head[12]) + (48, mod_ptr, mod_bytes, B, N)
        first = (C.byref(pf), C.byref(pe), C.byref(pd), None if markov is None else C.byref(markov), p(plan), *sc,
                 *[p(t) for t in graph])
        if entry == "step":
            st = lib.aether_s2s_dynfield_step(*first, p(x), None, p(dh), p(h), p(c), p(u), p(ws), ws_bytes, p(out["x1"]),
                                              p(out["dh1"]), p(out["h1"]), p(out["c1"]), p(out["e1"]), None, None)
        else:
            st = lib.aether_s2s_dynfield_rollout(*first, T0, p(burn), None, steps, p(x), p(dh), p(h), p(c), p(u), p(ws), ws_bytes,
                                                 p(out["preds"]), None, None)
        torch.cuda.synchronize()
        return st

    call.keep, call.need, call.mod_bytes, call.markov, call.out = keep, ws.numel(), mod.numel() * 4, mp, out
    return call


@pytest.mark.parametrize("entry", ["step", "rollout"])
def test_entries_reject_bad_arguments(entry_calls, entry):
    call, code = entry_calls, _codes()
    for t in call.out.values():
        t.fill_(-7.0)
    assert call(entry, mod_ptr=None) == code["AETHER_EINVAL"]
    assert call(entry, mod_bytes=call.mod_bytes - 1) == code["AETHER_ESPACE"]
    assert call(entry, n_nodes=2 * 3 + 1) == code["AETHER_EINVAL"]                 # != batch * num_objects
    assert call(entry, ws_bytes=call.need - 1) == code["AETHER_ESPACE"]
    assert call(entry, markov=call.markov) == code["AETHER_EINVAL"]                # both decoders
    assert all(bool((t == -7.0).all()) for t in call.out.values())                 # nothing was launched
    assert call(entry) == 0
    written = call.out["x1"] if entry == "step" else call.out["preds"]
    assert not bool((written == -7.0).any())


# -- 8. the FiLM epilogue of the split GEMM kernels -----------------------------------------------------------------------------------
@pytest.mark.parametrize("structure", [3, 2])        # aether_set_option("gemm_split", ..): 3 the LDS-DMA ring kernel, 2 the registers-for-X one
def test_in_step_field_on_the_split_gemm(structure):
    """The job table takes the fp16 x 2 split GEMM from 128 workgroups of 64 rows x 128 columns on: 1,641 graphs of 5 nodes are
    8,205 rows -- 129 row tiles, the last one ragged, graph boundaries at no tile boundary -- for mlp_hidden = decoder_hidden =
    128 (every job of the first launch has an image).  Both kernel structures, forced in turn."""
    from aether_amd import _lib
    lib = _lib.load()
    B, N, D = 1641, 5, 3
    model, sd64 = _model(95, N=N, D=D, markov=False, mlp_hidden=128, decoder_hidden=128)
    g = torch.Generator().manual_seed(96)
    x, dh, hc, summary, u = _state(model, B, N, g)
    model._set_summary(summary.cuda())
    assert lib.aether_set_option(b"gemm_split", structure) == 0
    try:
        field = model._fused_step(x.cuda(), dh.cuda(), _cuda(hc), u.cuda(), None, return_field=True)[4]
    finally:
        assert lib.aether_set_option(b"gemm_split", 1) == 0
    assert scale_rel_err(field.cpu(), S.film_field(sd64, x.double(), summary.double(), D)) <= 2 * TOL
