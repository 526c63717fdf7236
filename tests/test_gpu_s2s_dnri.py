"""The seq2seq dNRI baseline on the MI355X: the fused step, the device rollout (eager and captured), return_everything, the
decoder on given logits and the evaluation loss against the reference's fp32 values (tools/make_golden_s2s_dnri.py), at the
project's bar max|a - b| <= 1e-5 max|ref| per tensor with every sampled edge type equal (the fixtures' noise seeds
leave every Gumbel race a margin of 1e-3).  Both decoders, D in {2, 3}, skip_first on and off, 60 edges (no multiple of a tile
height) and N = 2.  Then the predicted update against fp64 at 4 x the fp32 restatement's own error (tests/update_parity.py),
the entries' refusals and the buffer contract: nothing outside the given workspace and outputs is written, and the workspace
is the dNRI layout's -- smaller than the LoCS step's."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import REPO, scale_rel_err
import test_s2s_dnri as T
from update_parity import check_update

pytestmark = pytest.mark.gpu
TOL = 1e-5
MG = T.MG
T0 = T.T0


def _t(d, key):
    return torch.from_numpy(d[key])


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", T.DECODERS)
@pytest.mark.parametrize("tag", T.CASES)
def test_step_and_rollout_match_the_reference(D, dec, tag):
    model, _, d = T.build(D, dec, tag, device="cuda")
    B, N = MG.CASES[tag][:2]
    E, K, R, H, steps = N * (N - 1), int(d["num_edge_types"]), int(d["rnn_hidden"]), int(d["hidden"]), int(d["steps"])
    inputs, U = _t(d, f"{dec}.{tag}.in.inputs"), _t(d, f"{dec}.{tag}.in.uniform")
    want = lambda k: _t(d, f"{dec}.{tag}.ref.{k}")
    front = lambda k: _t(d, f"rec.{tag}.ref.{k}")                        # the shared encoder's values are stored once
    x = inputs.cuda()
    zeros = lambda *s: torch.zeros(*s, device="cuda")
    u0 = U[0].view(B, E, K).cuda()
    # one fused step from the zero state: prior logits and state, sample, decoder
    out, dh, (h1, c1), edges, logits = model._fused_step(x[:, 0], zeros(B, N, H), (zeros(B, E, R), zeros(B, E, R)), u0,
                                                         return_logits=True)
    assert torch.equal(edges.argmax(-1).cpu(), want("step_edges").argmax(-1))
    assert torch.equal(edges.cpu(), want("step_edges"))
    checks = [("decoder_out", out, want)] + ([("decoder_hidden", dh, want)] if dec == "rec" else [])
    checks += [("prior_logits", logits, front), ("prior_h", h1, front), ("prior_c", c1, front)]
    plain = model._fused_step(x[:, 0], zeros(B, N, H), (zeros(B, E, R), zeros(B, E, R)), u0)
    assert len(plain) == 4 and torch.equal(plain[0], out) and torch.equal(plain[3], edges)
    for name, got, ref in checks:
        err = scale_rel_err(got.cpu(), ref(name))
        print(f"[dnri D{D} {dec} {tag}] step {name}: {err:.3g}")
        assert err <= TOL, name
    assert (dh is None) == (dec == "mlp")
    # the decoder on given logits (single_step_forward): the fixture's prior logits, the same draw
    sp, sdh, se = model.single_step_forward(x[:, 0], None if dec == "mlp" else zeros(B, N, H), front("prior_logits").cuda(), True,
                                            uniform=u0)
    assert torch.equal(se.cpu(), want("step_edges"))
    assert scale_rel_err(sp.cpu(), want("decoder_out")) <= TOL
    if dec == "rec":
        assert scale_rel_err(sdh.cpu(), want("decoder_hidden")) <= TOL
    # 3 burn-in + 4 predicted steps on the device, with and without the edges
    u = U.view(-1, B, E, K).cuda()
    w_all, w_edges = want("everything"), want("everything_edges")
    preds, pe = model.predict_future(x, steps, return_edges=True, uniform=u)
    assert torch.equal(pe.argmax(-1).cpu(), w_edges[:, T0:].argmax(-1))
    err = scale_rel_err(preds.cpu(), w_all[:, T0:])
    print(f"[dnri D{D} {dec} {tag}] predict_future: {err:.3g}")
    assert err <= TOL
    assert torch.equal(model.predict_future(x, steps, uniform=u), preds)
    # the captured rollout is the eager one bit for bit, twice
    for _ in range(2):
        gp, ge = model.predict_future(x, steps, return_edges=True, uniform=u, graph=True)
        assert torch.equal(gp, preds) and torch.equal(ge, pe)
    # return_everything: the burn-in steps' predictions and samples in front, every one against the reference's
    everything, ee = model.predict_future(x, steps, return_edges=True, return_everything=True, uniform=u)
    assert everything.shape == w_all.shape and ee.shape == w_edges.shape
    assert torch.equal(ee.argmax(-1).cpu(), w_edges.argmax(-1))
    err = scale_rel_err(everything.cpu(), w_all)
    print(f"[dnri D{D} {dec} {tag}] return_everything: {err:.3g}")
    assert err <= TOL
    assert torch.equal(everything[:, T0:], preds)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", T.DECODERS)
@pytest.mark.parametrize("name", T.LOSS_NAMES)
def test_calculate_loss_matches_the_reference(D, dec, name):
    """calculate_loss(is_train=False) with the full-sequence encoder (aether_s2s_dnri_encoder_features) against the reference:
    posterior logits, every step's sample (re-derived from the logits and the draws), predictions and the loss terms."""
    from oracle import seq2seq_oracle as S
    model, _, d = T.loss_model(D, dec, name, device="cuda")
    inputs, U = _t(d, f"{dec}.loss.in.inputs"), _t(d, f"{dec}.loss.{name}.uniform")
    B, Tn, N, _ = inputs.shape
    E, K = N * (N - 1), U.shape[-1]
    u = U.view(Tn - 1, B, E, K).cuda()
    loss, nll, kl, post, preds = model.calculate_loss(inputs.cuda(), is_train=False, return_logits=True, uniform=u)
    want = lambda k: _t(d, f"{dec}.loss.{name}.{k}")
    assert scale_rel_err(post.cpu(), want("posterior")) <= TOL
    z_got = torch.stack([S.gumbel_hard(post.cpu()[:, s].reshape(-1, K), U[s], 0.5) for s in range(Tn - 1)])
    z_ref = torch.stack([S.gumbel_hard(want("posterior")[:, s].reshape(-1, K), U[s], 0.5) for s in range(Tn - 1)])
    assert torch.equal(z_got.argmax(-1), z_ref.argmax(-1))
    assert scale_rel_err(preds.cpu(), want("predictions")) <= TOL
    for key, got in (("loss", loss), ("nll", nll), ("kl", kl)):
        err = scale_rel_err(got.cpu(), want(key))
        print(f"[dnri D{D} {dec} loss {name}] {key}: {err:.3g}")
        assert err <= TOL, key
    _, _, _, e = model.calculate_loss(inputs.cuda(), is_train=False, return_edges=True, uniform=u)
    assert torch.equal(e.cpu().argmax(-1).reshape(-1), z_ref[-1].argmax(-1))
    # encoder(inputs): the module's own call gives the same logits as the loss used
    prior, post2, (h, c) = model.encoder(inputs[:, :-1].cuda())
    assert torch.equal(post2, post) and prior.shape == post.shape and h.shape == (B, E, int(d["rnn_hidden"]))
    # the prior's logits instead of the posterior's: the loss terms stay finite and the call takes the reference's keyword
    out = model.calculate_loss(inputs.cuda(), is_train=False, use_prior_logits=True, uniform=u)
    assert len(out) == 3 and all(torch.isfinite(v).all() for v in out)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", T.DECODERS)
def test_predicted_update_against_fp64(D, dec):
    """The model returns inputs + update: the update of one step from a random state (7 graphs of 5 objects, the decoder on
    the sample the device drew) is held to 4 x the error the fp32 CPU restatement of the same step has against fp64
    (tests/update_parity.py)."""
    tag, B, N = "B2N5", 7, 5
    model, _, _ = T.build(D, dec, tag, device="cuda")
    from test_gpu_buffer_contract import _s2s_state
    g = _s2s_state(model, B, N, 40 + D)
    out, dh, (h1, c1), edges = model._fused_step(g["x"].cuda(), g["dh"].cuda(), (g["h"].cuda(), g["c"].cuda()), g["u"].cuda())
    torch.cuda.synchronize()
    z = edges.cpu()
    hidden = None if dec == "mlp" else g["dh"]
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        want32, _ = T.restatement(model, tag, torch.float32).decoder(g["x"], hidden, z)
    finally:
        torch.set_num_threads(n)
    want64, _ = T.restatement(model, tag, torch.float64).decoder(g["x"].double(), None if hidden is None else hidden.double(),
                                                                   z.double())
    check_update(f"dnri D{D} {dec} step", out.cpu(), want32, g["x"], want64)


@pytest.mark.parametrize("structure,D,dec", [(2, 2, "rec"), (3, 3, "rec"), (2, 3, "mlp"), (3, 2, "mlp")])
def test_step_on_the_split_gemms(structure, D, dec):
    """600 nodes / 2,400 edges with decoder_hidden 512: the size from which the dense layers (the prior's, the message layers
    through the per-type lists, the hidden products of the gate, out_fc1 on the row whose first 32 columns hold the 2D-wide
    inputs) run on the two-piece fp16 GEMMs and the LSTM cell in their epilogue, in both of their structures; one step from a
    random state against the fp64 restatement."""
    from aether_amd import _lib
    from aether_amd.nn.seq2seq.dnri import DNRI
    N, B, K, H = 5, 120, 2, 512
    params = MG.model_params(N, D, False, MG.DECODERS[dec], {"decoder_hidden": H})
    torch.manual_seed(70 + D)
    model = DNRI(params, device=None).eval()
    with torch.no_grad():
        T.perturb_bn_(model)
    E, R = N * (N - 1), 64
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, N, 2 * D, generator=g)
    u = torch.rand(B, E, K, generator=g)
    state = (torch.randn(B, E, R, generator=g) * 0.3, torch.randn(B, E, R, generator=g) * 0.3)
    hidden = torch.randn(B, N, H, generator=g) * 0.3
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    rs = T.RS.Model(sd, torch.float64, 3, False, 0.5)
    w_out, w_dh, (w_h, w_c), w_z, _ = rs.step(x.double(), None if dec == "mlp" else hidden.double(),
                                              tuple(t.double() for t in state), u.double())
    model = model.cuda()
    lib = _lib.load()
    try:
        lib.aether_set_option(b"gemm_split", structure)
        out, dh, (h1, c1), z = model._fused_step(x.cuda(), hidden.cuda(), tuple(t.cuda() for t in state), u.cuda())
        torch.cuda.synchronize()
    finally:
        lib.aether_set_option(b"gemm_split", 1)
    assert scale_rel_err(h1.cpu(), w_h) <= TOL and scale_rel_err(c1.cpu(), w_c) <= TOL
    # random draws leave some Gumbel races closer than fp32 rounding: a graph with a flipped sample computes something else
    # from there on; at least 95 % of the samples agree and the graphs without a flipped one are held to the bar
    same_edge = z.cpu().argmax(-1) == w_z.argmax(-1)
    assert same_edge.float().mean() >= 0.95
    same = same_edge.all(-1)
    assert same.float().mean() >= 0.5
    assert scale_rel_err(out.cpu()[same], w_out[same]) <= TOL
    if dec == "rec":
        assert scale_rel_err(dh.cpu()[same], w_dh[same]) <= TOL


@pytest.mark.parametrize("D,dec,K,skip", [(2, "rec", 4, False), (3, "rec", 3, True), (2, "mlp", 4, False), (3, "mlp", 3, True)])
def test_three_and_four_edge_types(D, dec, K, skip):
    """The fixtures have two edge types.  Four used types make the recurrent decoder's eight first-layer products overflow the
    job table they share with mlp1 (it is launched in two parts); three types with skip_first leave type 0's lists and weights
    unused.  One step and a two-step rollout from a random state against the fp64 restatement, N = 4."""
    from aether_amd.nn.seq2seq.dnri import DNRI
    N, B, H, R = 4, 3, 128, 64
    params = MG.model_params(N, D, skip, MG.DECODERS[dec], {"num_edge_types": K})
    torch.manual_seed(90 + K)
    model = DNRI(params, device=None).eval()
    with torch.no_grad():
        T.perturb_bn_(model)
    E = N * (N - 1)
    g = torch.Generator().manual_seed(11 + D)
    x = torch.randn(B, N, 2 * D, generator=g)
    U = torch.rand(2, B, E, K, generator=g)
    state = (torch.randn(B, E, R, generator=g) * 0.3, torch.randn(B, E, R, generator=g) * 0.3)
    hidden = torch.randn(B, N, H, generator=g) * 0.3
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    rs = T.RS.Model(sd, torch.float64, 3, skip, 0.5)
    w_hidden = None if dec == "mlp" else hidden.double()
    w1 = rs.step(x.double(), w_hidden, tuple(t.double() for t in state), U[0].double())
    w2 = rs.step(w1[0], w1[1], w1[2], U[1].double())
    # the case is a test of the layers, not of a Gumbel race: its seeds leave every race of both steps a clear margin
    for w, u in ((w1, U[0]), (w2, U[1])):
        top = ((w[4] - torch.log(1e-10 - torch.log(u.double() + 1e-10))) / 0.5).topk(2, dim=-1).values
        assert float((top[..., 0] - top[..., 1]).min()) > 1e-3
    model = model.cuda()
    out, dh, (h1, c1), z = model._fused_step(x.cuda(), hidden.cuda(), tuple(t.cuda() for t in state), U[0].cuda())
    assert torch.equal(z.cpu().argmax(-1), w1[3].argmax(-1))
    assert scale_rel_err(out.cpu(), w1[0]) <= TOL and scale_rel_err(h1.cpu(), w1[2][0]) <= TOL
    assert scale_rel_err(c1.cpu(), w1[2][1]) <= TOL
    if dec == "rec":
        assert scale_rel_err(dh.cpu(), w1[1]) <= TOL
    preds, edges, _ = model._fused_rollout(None, x.cuda(), hidden.cuda(), tuple(t.cuda() for t in state), 2, U.cuda(), True)
    assert torch.equal(edges[:, 1].cpu().argmax(-1), w2[3].argmax(-1))
    assert torch.equal(preds[:, 0], out)
    assert scale_rel_err(preds[:, 1].cpu(), w2[0]) <= TOL


def test_eval_forward_prediction_takes_the_model():
    """aether_amd.evaluate.eval_forward_prediction (the runner's rollout MSE) on the model as it is: per-step errors of the
    fixture's trajectory equal those of predict_future called by hand."""
    from aether_amd.evaluate import eval_forward_prediction
    D, dec, tag = 2, "rec", "B3N5"
    model, _, d = T.build(D, dec, tag, device="cuda")
    inputs, U = _t(d, f"{dec}.{tag}.in.inputs"), _t(d, f"{dec}.{tag}.in.uniform")
    B, Tn, N, _ = inputs.shape
    burn, steps = 2, 2

    class Data:
        feats = inputs.cuda()
        ndim = D
        torch_unnormalize = staticmethod(lambda t: t)
        __len__ = lambda self: B

    u = U.view(-1, B, N * (N - 1), 2)[:burn - 1 + steps].cuda()
    mse, pos, vel = eval_forward_prediction(model, Data(), burn, steps, batch_size=B, uniform=u)
    preds = model.predict_future(Data.feats[:, :burn], steps, uniform=u)
    se = (preds - Data.feats[:, burn:burn + steps]) ** 2
    assert torch.equal(mse, se.flatten(2).mean(-1).mean(0)) and mse.shape == (steps,)
    assert torch.equal(pos, se[..., :D].flatten(2).mean(-1).mean(0)) and torch.equal(vel, se[..., D:].flatten(2).mean(-1).mean(0))
    assert torch.isfinite(mse).all()


# -- the entries' refusals ------------------------------------------------------------------------------------------------------
def _codes():
    header = os.path.join(REPO, "include", "aether_hip.h")
    return {k: int(v) for k, v in re.findall(r"#define (AETHER_E\w+) \((-\d+)\)", open(header).read())}


def _raw_calls(dec):
    """The step, rollout and encoder-features entries through the C ABI on real, full-size buffers and the model's plan:
    call(workspace_bytes=None, both=False) -> status."""
    from aether_amd import _lib
    lib = _lib.load()
    D, tag = 2, "B1N2"
    model, _, d = T.build(D, dec, tag, device="cuda")
    B, N = MG.CASES[tag][:2]
    E, K, R, H = N * (N - 1), 2, int(d["rnn_hidden"]), int(d["hidden"])
    _, plan, ws, graph, (_, pe, pd), scal, hook = model._step_common(B, N, torch.device("cuda:0"))
    need = lib.aether_s2s_dnri_workspace_bytes(D, H, H, R, 64, K, B * N, B * E)
    assert ws.numel() == need > 0
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    x, burn, dh, h, c = z(B, N, 2 * D), z(1, B, N, 2 * D), z(B, N, H), z(B, E, R), z(B, E, R)
    u = torch.full((3, B, E, K), 0.5, dtype=torch.float32, device="cuda")
    x1, dh1, h1, c1, e1, preds, feats = z(B, N, 2 * D), z(B, N, H), z(B, E, R), z(B, E, R), z(B, E, K), z(2, B, N, 2 * D), z(B * E, H)
    p = lambda t: t.data_ptr()
    g = [p(t) for t in graph]
    mlp = dec == "mlp"
    dstate = lambda t: None if mlp else p(t)

    def head(both):
        return (C.byref(pe), C.byref(pd), C.byref(pd)) if both else (C.byref(pe), *hook.decoders(model.decoder, pd))

    def step(workspace_bytes=None, both=False):
        st = lib.aether_s2s_dnri_step(*head(both), p(plan), *scal, *g, p(x), None, dstate(dh), p(h), p(c), p(u), p(ws),
                                      need if workspace_bytes is None else workspace_bytes, p(x1), dstate(dh1), p(h1), p(c1),
                                      p(e1), None, None)
        torch.cuda.synchronize()
        return st

    def rollout(workspace_bytes=None, both=False):
        st = lib.aether_s2s_dnri_rollout(*head(both), p(plan), *scal, *g, 1, p(burn), 2, p(x), dstate(dh), p(h), p(c), p(u), p(ws),
                                         need if workspace_bytes is None else workspace_bytes, p(preds), None, None)
        torch.cuda.synchronize()
        return st

    def features(workspace_bytes=None, both=False):
        st = lib.aether_s2s_dnri_encoder_features(*head(both), p(plan), *scal[:10], *scal[11:], *g, p(x), p(ws),
                                                  need if workspace_bytes is None else workspace_bytes, p(feats), None)
        torch.cuda.synchronize()
        return st

    keep = (model, plan, ws, pe, pd, x, burn, dh, h, c, u, x1, dh1, h1, c1, e1, preds, feats)
    return {"step": step, "rollout": rollout, "encoder_features": features}, need, keep


@pytest.mark.parametrize("dec", T.DECODERS)
def test_a_workspace_one_byte_short_is_refused(dec):
    """Each call has exactly one defect, and one that would do no harm if the check were lost: the buffer itself is full size."""
    calls, need, keep = _raw_calls(dec)
    codes = _codes()
    for name, call in calls.items():
        assert call() == 0, name
        assert call(workspace_bytes=need - 1) == codes["AETHER_ESPACE"], name
        assert call(both=True) == codes["AETHER_EINVAL"], name                 # both decoders named
        assert call() == 0, name
    del keep


# -- the buffer contract ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dec", T.DECODERS)
@pytest.mark.parametrize("D,B", [(2, 7), (3, 5)])
def test_buffer_contract_and_layout_sizes(D, B, dec):
    """The step, the rollout, the full-sequence encoder and the decoder on given logits inside guarded, poisoned buffers
    (test_gpu_buffer_contract.py, tests/guarded_alloc.py): no guard byte changes, the results equal the plain run's bit for bit
    and the fp64 restatement's at 1e-5.  The allocation record shows what a dNRI step is given: its plan and workspace have
    exactly the sizes of the dnri layouts, not those of the LoCS step."""
    from aether_amd import _lib
    from test_gpu_buffer_contract import _s2s_body, _s2s_sizes, _s2s_state, contract
    lib = _lib.load()
    tag, N = "B2N5", 5
    make = lambda: T.build(D, dec, tag, device="cuda")[0]
    base_body = _s2s_body(make, B, N, 3, oracle=False)
    seq = torch.randn(B, 3, N, 2 * D, generator=torch.Generator().manual_seed(9))

    def body(g):
        r = base_body(g)
        m = make()
        prior, post, (h, c) = m._encoder_forward(g["seq"])
        r.result("encoder.prior", prior)
        r.result("encoder.posterior", post)
        # the decoder on given logits (the step with ext_logits: the prior is skipped)
        m.__dict__["_step_ws"] = None
        given = prior[:, 0].contiguous()
        s_out, s_dh, s_edges = m.single_step_forward(g["x"], g["dh"], given, True, uniform=g["u"])
        r.result("given.out", s_out, output=True)
        r.result("given.edges", s_edges, output=True)
        if s_dh is not None:
            r.result("given.dh", s_dh, output=True)
        rs = T.restatement(m, tag, torch.float64)
        cpu = lambda t: t.detach().cpu().double()
        w_prior, w_post, _ = rs.encoder_forward(cpu(g["seq"]))
        r.against("encoder.prior", w_prior)
        r.against("encoder.posterior", w_post)
        hidden = None if dec == "mlp" else cpu(g["dh"])
        (w_logits, (w_h, w_c)) = rs.prior(cpu(g["x"]), (cpu(g["h"]), cpu(g["c"])))
        w_out, w_dh = rs.decoder(cpu(g["x"]), hidden, cpu(r.results["edges"]))
        r.against("out", w_out)
        r.against("h", w_h)
        r.against("c", w_c)
        if w_dh is not None:
            r.against("dh", w_dh)
        w_sout, w_sdh = rs.decoder(cpu(g["x"]), hidden, cpu(s_edges))
        r.against("given.out", w_sout)
        if w_sdh is not None:
            r.against("given.dh", w_sdh)
        gap = ((w_logits - torch.log(1e-10 - torch.log(cpu(g["u"]) + 1e-10))) / 0.5).topk(2, dim=-1).values
        clear = (gap[..., 0] - gap[..., 1]) > 1e-3
        assert clear.float().mean() > 0.9
        assert torch.equal(r.results["edges"].cpu().argmax(-1)[clear], rs.sample(w_logits, cpu(g["u"])).argmax(-1)[clear])
        return r

    inputs = dict(_s2s_state(make(), B, N, 62), seq=seq)
    guard, got = contract(body, inputs, f"s2s dnri {dec} D{D} B{B}")
    # the allocation record against the layouts: the dNRI sizes are there, the LoCS step's larger ones are not
    m = make()
    plan_bytes, ws_bytes = _s2s_sizes(m, B, N)
    E, he = B * N * (N - 1), 128
    rec = (1, None) if dec == "rec" else (None, 1)
    locs_plan = lib.aether_s2s_locs_plan_bytes(*rec, D, he, 128, 64, 3, 64, 2, 0)
    locs_ws = lib.aether_s2s_locs_workspace_bytes(D, he, 128, 64, 64, 2, B * N, E)
    assert plan_bytes == lib.aether_s2s_dnri_plan_bytes(*rec, D, he, 128, 64, 3, 64, 2, 0)
    assert ws_bytes == lib.aether_s2s_dnri_workspace_bytes(D, he, 128, 64, 64, 2, B * N, E)
    assert guard.find(nbytes=plan_bytes, dtype=torch.uint8) and guard.find(nbytes=ws_bytes, dtype=torch.uint8)
    assert plan_bytes < locs_plan and ws_bytes < locs_ws
    assert not guard.find(nbytes=locs_plan, dtype=torch.uint8) and not guard.find(nbytes=locs_ws, dtype=torch.uint8)
