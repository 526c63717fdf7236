"""The seq2seq ablation DNRIAether (dNRI with the latent field, no frames) on the MI355X, against the reference's fp32 values
(tools/make_golden_s2s_dnri_aether.py) at the project's bar max|a - b| <= 1e-5 max|ref| per tensor with every sampled edge type
equal (the fixtures' noise seeds leave every Gumbel race a margin of 1e-3): the fused step with the field, the decoder on given
logits and a given field, the device rollout (eager and captured), return_everything and the evaluation loss -- both decoders,
D = 3 (the 9-column rows the narrow dNRI kernels cannot hold) and 2, 60 edge rows (no multiple of a tile) and N = 2.  Then the
predicted update against fp64 (tests/update_parity.py), three and four edge types, the field layers on the split GEMMs, the
launch count next to dNRI's, the entries' refusals and the buffer contract."""
import ctypes as C

import pytest
import torch

from conftest import scale_rel_err
import test_s2s_dnri as TD
import test_s2s_dnri_aether as T
from test_gpu_s2s_dnri import _codes
from update_parity import check_update

pytestmark = pytest.mark.gpu
TOL = 1e-5
MG = T.MG
T0 = T.T0


def _t(d, key):
    return torch.from_numpy(d[key])


def _gap(logits, u, tau=0.5):
    """The gap between the two largest Gumbel scores of every race: logits, u [B, E, K] -> [B, E]."""
    top = ((logits - torch.log(1e-10 - torch.log(u + 1e-10))) / tau).topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


def _margin(logits, u, tau=0.5):
    """The smallest gap of a graph's races -> [B]."""
    return _gap(logits, u, tau).min(-1).values


def _stats(lib):
    from aether_amd import _lib
    st = _lib.AetherS2SLaunchStats()
    _lib.check(lib.aether_s2s_launch_stats(C.byref(st)), "aether_s2s_launch_stats")
    return st


# -- 1. the fixtures ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", T.DECODERS)
@pytest.mark.parametrize("tag", T.CASES)
def test_step_and_rollout_match_the_reference(D, dec, tag):
    model, _, d = T.build(D, dec, tag, device="cuda")
    B, N = MG.CASES[tag][:2]
    E, K, R, H, steps = N * (N - 1), int(d["num_edge_types"]), int(d["rnn_hidden"]), int(d["hidden"]), int(d["steps"])
    inputs, U = _t(d, f"{dec}.{tag}.in.inputs"), _t(d, f"{dec}.{tag}.in.uniform")
    want = lambda k: _t(d, f"{dec}.{tag}.ref.{k}")
    x = inputs.cuda()
    zeros = lambda *s: torch.zeros(*s, device="cuda")
    u0 = U[0].view(B, E, K).cuda()
    # one fused step from the zero state: field, prior logits and state, sample, decoder
    out, dh, (h1, c1), edges, field, logits = model._fused_step(x[:, 0], zeros(B, N, H), (zeros(B, E, R), zeros(B, E, R)), u0,
                                                                return_field=True, return_logits=True)
    assert torch.equal(edges.cpu(), want("step_edges"))
    checks = [("field", field), ("prior_logits", logits), ("prior_h", h1), ("prior_c", c1), ("decoder_out", out)]
    checks += [("decoder_hidden", dh)] if dec == "rec" else []
    for name, got in checks:
        err = scale_rel_err(got.cpu(), want(name))
        print(f"[dnri_aether D{D} {dec} {tag}] step {name}: {err:.3g}")
        assert err <= TOL, name
    assert (dh is None) == (dec == "mlp")
    plain = model._fused_step(x[:, 0], zeros(B, N, H), (zeros(B, E, R), zeros(B, E, R)), u0)
    assert len(plain) == 4 and torch.equal(plain[0], out) and torch.equal(plain[3], edges)
    assert torch.equal(model.predict_field(x[:, 0])[1], x[:, 0, :, :D])
    assert scale_rel_err(model.predict_field(x[:, 0])[0].cpu(), want("field")) <= TOL
    # the decoder on given logits with the field handed in (single_step_forward): the fixture's logits and field, the same draw
    sp, sdh, se = model.single_step_forward(x[:, 0], None if dec == "mlp" else zeros(B, N, H), want("prior_logits").cuda(), True,
                                            want("field").cuda(), uniform=u0)
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
    print(f"[dnri_aether D{D} {dec} {tag}] predict_future: {err:.3g}")
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
    print(f"[dnri_aether D{D} {dec} {tag}] return_everything: {err:.3g}")
    assert err <= TOL
    assert torch.equal(everything[:, T0:], preds)


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", T.DECODERS)
@pytest.mark.parametrize("name", T.LOSS_NAMES)
def test_calculate_loss_matches_the_reference(D, dec, name):
    """calculate_loss(is_train=False) with the full-sequence encoder (aether_s2s_dnri_aether_encoder_features, the field of
    the frames handed in) against the reference: posterior logits, every step's sample, predictions and the loss terms."""
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
        print(f"[dnri_aether D{D} {dec} loss {name}] {key}: {err:.3g}")
        assert err <= TOL, key
    _, _, _, e = model.calculate_loss(inputs.cuda(), is_train=False, return_edges=True, uniform=u)
    assert torch.equal(e.cpu().argmax(-1).reshape(-1), z_ref[-1].argmax(-1))
    # encoder(inputs, predicted_field): the module's own call gives the same logits as the loss used
    frames = inputs[:, :-1].cuda()
    field, _ = model.predict_field(frames.transpose(2, 1).contiguous())                    # [B, N, T - 1, D]
    prior, post2, (h, c) = model.encoder(frames, field)
    assert torch.equal(post2, post) and prior.shape == post.shape and h.shape == (B, E, int(d["rnn_hidden"]))
    out = model.calculate_loss(inputs.cuda(), is_train=False, use_prior_logits=True, uniform=u)
    assert len(out) == 3 and all(torch.isfinite(v).all() for v in out)


# -- 2. the predicted update ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", T.DECODERS)
def test_predicted_update_against_fp64(D, dec):
    """The model returns inputs + update: the update of one step from a random state (7 graphs of 5 objects, the decoder on
    the sample the device drew and the field it queried itself) is held to 4 x the error the fp32 CPU restatement of the same
    step has against fp64 (tests/update_parity.py)."""
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
        want32, _ = T.restatement(model, False, torch.float32).decoder(g["x"], hidden, z)
    finally:
        torch.set_num_threads(n)
    want64, _ = T.restatement(model, False, torch.float64).decoder(g["x"].double(), None if hidden is None else hidden.double(),
                                                                     z.double())
    check_update(f"dnri_aether D{D} {dec} step", out.cpu(), want32, g["x"], want64)


# -- 3. three and four edge types -------------------------------------------------------------------------------------------------
EDGE_TYPE_SEEDS = {(2, "rec", 4): (94, 13), (3, "rec", 3): (93, 14), (2, "mlp", 4): (94, 13), (3, "mlp", 3): (93, 14)}


def edge_type_case(D, dec, K, skip):
    """-> (model on the CPU, restatement in fp64, x, hidden, state, U [2, B, E, K]) of the case: N = 4, B = 3."""
    N, B, H, R = 4, 3, 128, 64
    model_seed, state_seed = EDGE_TYPE_SEEDS[(D, dec, K)]
    model = T.make(MG.model_params(N, D, skip, MG.DECODERS[dec], {"num_edge_types": K}), model_seed)
    E = N * (N - 1)
    g = torch.Generator().manual_seed(state_seed)
    x = torch.randn(B, N, 2 * D, generator=g)
    U = torch.rand(2, B, E, K, generator=g)
    state = (torch.randn(B, E, R, generator=g) * 0.3, torch.randn(B, E, R, generator=g) * 0.3)
    hidden = torch.randn(B, N, H, generator=g) * 0.3
    return model, T.restatement(model, skip, torch.float64), x, hidden, state, U


def edge_type_steps(rs, dec, x, hidden, state, U):
    """Two steps of the fp64 restatement and the smallest margin of their Gumbel races."""
    w1 = rs.step(x.double(), None if dec == "mlp" else hidden.double(), tuple(t.double() for t in state), U[0].double())
    w2 = rs.step(w1[0], w1[1], w1[2], U[1].double())
    return w1, w2, min(float(_margin(w[4], u.double()).min()) for w, u in ((w1, U[0]), (w2, U[1])))


@pytest.mark.parametrize("D,dec,K,skip", [(2, "rec", 4, False), (3, "rec", 3, True), (2, "mlp", 4, False), (3, "mlp", 3, True)])
def test_three_and_four_edge_types(D, dec, K, skip):
    """The fixtures have two edge types.  With four used types the recurrent decoder's eight first-layer products do not fit
    the job table they share with mlp1's second layer (it is launched in two parts, behind the two field layers); three types
    with skip_first leave type 0's lists and weights unused.  One step and a two-step rollout from a random state against the
    fp64 restatement, N = 4.  The case is a test of the layers, not of a Gumbel race: its seeds leave every race of both steps
    an fp64 margin above 1e-3."""
    model, rs, x, hidden, state, U = edge_type_case(D, dec, K, skip)
    w1, w2, margin = edge_type_steps(rs, dec, x, hidden, state, U)
    assert margin > 1e-3
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


# -- 4. the field layers on the split GEMMs -----------------------------------------------------------------------------------------
SPLIT_B, SPLIT_H = 410, 512


def split_case(D, dec):
    """One step from a random state with encoder_hidden 512, N = 5, B = 410 (2,050 nodes, 8,200 edges) -> (model on the CPU,
    inputs, the fp64 restatement's step, which graphs have all 20 races clear of 1e-3)."""
    N, K, R = 5, 2, 64
    model = T.make(MG.model_params(N, D, False, MG.DECODERS[dec], {"encoder_hidden": SPLIT_H}), 70 + D)
    E = N * (N - 1)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(SPLIT_B, N, 2 * D, generator=g)
    u = torch.rand(SPLIT_B, E, K, generator=g)
    state = (torch.randn(SPLIT_B, E, R, generator=g) * 0.3, torch.randn(SPLIT_B, E, R, generator=g) * 0.3)
    hidden = torch.randn(SPLIT_B, N, int(MG.MD.H), generator=g) * 0.3
    rs = T.restatement(model, False, torch.float64)
    want = rs.step(x.double(), None if dec == "mlp" else hidden.double(), tuple(t.double() for t in state), u.double())
    return model, (x, hidden, state, u), want, _margin(want[4], u.double()) > 1e-3


@pytest.mark.parametrize("structure,D,dec", [(2, 3, "rec"), (3, 2, "mlp")])
def test_field_layers_on_the_split_gemms(structure, D, dec):
    """By the dispatch rule of s2s_launch_jobs (tiles_big >= 128) 2,050 rows are where a lone 512-wide node layer first takes the
    two-piece fp16 GEMM: field_net.0 and field_net.2, the step's first two job tables, must have taken it -- in the structure
    the option names -- and the step is compared with the fp64 restatement: the prior state for every edge, the outputs for the
    graphs all of whose 20 Gumbel races have an fp64 margin above 1e-3 (at least 90 % of the graphs; the share depends on the
    inputs and the reference alone), every sample of those graphs equal."""
    from aether_amd import _lib
    model, (x, hidden, state, u), (w_out, w_dh, (w_h, w_c), w_z, _), clear = split_case(D, dec)
    assert clear.float().mean() >= 0.9
    model = model.cuda()
    lib = _lib.load()
    args = (x.cuda(), hidden.cuda(), tuple(t.cuda() for t in state), u.cuda())
    try:
        lib.aether_set_option(b"gemm_split", structure)
        model._fused_step(*args)                                         # (the plan and the workspace)
        torch.cuda.synchronize()
        lib.aether_s2s_launch_stats_reset()
        out, dh, (h1, c1), z = model._fused_step(*args)
        torch.cuda.synchronize()
        st = _stats(lib)
    finally:
        lib.aether_set_option(b"gemm_split", 1)
        lib.aether_s2s_launch_stats_reset()
    kind = {2: 3, 3: 1}[structure]                                       # k_s2s_gemm_split_r1<1> | k_s2s_gemm_split<1> (64-row tiles)
    for layer in (0, 1):
        r = st.log[layer]
        got = (r.kind, r.jobs, r.images, r.N, r.M, r.K)
        assert got == (kind, 1, 1, SPLIT_B * 5, SPLIT_H, SPLIT_H), (layer, got)
    assert scale_rel_err(h1.cpu(), w_h) <= TOL and scale_rel_err(c1.cpu(), w_c) <= TOL
    assert torch.equal(z.cpu()[clear], w_z[clear].float())
    err = scale_rel_err(out.cpu()[clear], w_out[clear])
    print(f"[dnri_aether D{D} {dec} split structure {structure}] out: {err:.3g}, clear graphs {float(clear.float().mean()):.3f}")
    assert err <= TOL
    if dec == "rec":
        assert scale_rel_err(dh.cpu()[clear], w_dh[clear]) <= TOL


# -- 5. the launch count ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("dec", T.DECODERS)
def test_job_table_launches_next_to_dnri(D, dec):
    """Job-table launches of a step at B2N5: the dNRI step's plus field_net.0 and field_net.2, and plus none when the field is
    handed in."""
    from aether_amd import _lib
    lib = _lib.load()
    tag = "B2N5"
    B, N = MG.CASES[tag][:2]
    E, K, R, H = N * (N - 1), 2, 64, 128
    z = lambda *s: torch.zeros(*s, device="cuda")
    args = (z(B, N, 2 * D), z(B, N, H), (z(B, E, R), z(B, E, R)), torch.full((B, E, K), 0.5, device="cuda"))

    def launches(model, **kw):
        model._fused_step(*args, **kw)
        torch.cuda.synchronize()
        lib.aether_s2s_launch_stats_reset()
        model._fused_step(*args, **kw)
        torch.cuda.synchronize()
        n = int(_stats(lib).logged)
        lib.aether_s2s_launch_stats_reset()
        return n

    dnri = launches(TD.build(D, dec, tag, device="cuda")[0])
    model = T.build(D, dec, tag, device="cuda")[0]
    own, given = launches(model), launches(model, field=z(B, N, D))
    print(f"[dnri_aether D{D} {dec}] job-table launches per step: dNRI {dnri}, DNRIAether {own}, field handed in {given}")
    assert dnri > 0 and given == dnri and dnri < own <= dnri + 2


# -- 6. refusals and the buffer contract --------------------------------------------------------------------------------------------
def _raw_calls(dec):
    """The step, rollout and encoder-features entries through the C ABI on real, full-size buffers and the model's plan:
    call(workspace_bytes=None, both=False, field=True) -> status."""
    from aether_amd import _lib
    lib = _lib.load()
    D, tag = 3, "B1N2"
    model, _, d = T.build(D, dec, tag, device="cuda")
    B, N = MG.CASES[tag][:2]
    E, K, R, H = N * (N - 1), 2, int(d["rnn_hidden"]), int(d["hidden"])
    _, plan, ws, graph, (pf, pe, pd), scal, hook = model._step_common(B, N, torch.device("cuda:0"))
    need = lib.aether_s2s_dnri_aether_workspace_bytes(D, H, H, R, 64, K, B * N, B * E)
    assert ws.numel() == need > 0
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    x, burn, dh, h, c = z(B, N, 2 * D), z(1, B, N, 2 * D), z(B, N, H), z(B, E, R), z(B, E, R)
    u = torch.full((3, B, E, K), 0.5, dtype=torch.float32, device="cuda")
    x1, dh1, h1, c1, e1, preds, feats = z(B, N, 2 * D), z(B, N, H), z(B, E, R), z(B, E, R), z(B, E, K), z(2, B, N, 2 * D), z(B * E, H)
    p = lambda t: t.data_ptr()
    g = [p(t) for t in graph]
    dstate = lambda t: None if dec == "mlp" else p(t)

    def head(both, field):
        decs = (C.byref(pd), C.byref(pd)) if both else hook.decoders(model.decoder, pd)
        return (C.byref(pf) if field else None, C.byref(pe), *decs)

    def step(workspace_bytes=None, both=False, field=True):
        st = lib.aether_s2s_dnri_aether_step(*head(both, field), p(plan), *scal, *g, p(x), None, None, dstate(dh), p(h), p(c), p(u),
                                             p(ws), need if workspace_bytes is None else workspace_bytes, p(x1), dstate(dh1),
                                             p(h1), p(c1), p(e1), None, None, None)
        torch.cuda.synchronize()
        return st

    def rollout(workspace_bytes=None, both=False, field=True):
        st = lib.aether_s2s_dnri_aether_rollout(*head(both, field), p(plan), *scal, *g, 1, p(burn), None, 2, p(x), dstate(dh), p(h),
                                                p(c), p(u), p(ws), need if workspace_bytes is None else workspace_bytes, p(preds),
                                                None, None)
        torch.cuda.synchronize()
        return st

    def features(workspace_bytes=None, both=False, field=True):
        st = lib.aether_s2s_dnri_aether_encoder_features(*head(both, field), p(plan), *scal[:10], *scal[11:], *g, p(x), None, p(ws),
                                                         need if workspace_bytes is None else workspace_bytes, p(feats), None)
        torch.cuda.synchronize()
        return st

    keep = (model, plan, ws, pf, pe, pd, x, burn, dh, h, c, u, x1, dh1, h1, c1, e1, preds, feats)
    return {"step": step, "rollout": rollout, "encoder_features": features}, need, keep


@pytest.mark.parametrize("dec", T.DECODERS)
def test_refusals_of_the_entries(dec):
    """Each call has exactly one defect, and one that would do no harm if the check were lost: the buffers are full size."""
    calls, need, keep = _raw_calls(dec)
    codes = _codes()
    for name, call in calls.items():
        assert call() == 0, name
        assert call(workspace_bytes=need - 1) == codes["AETHER_ESPACE"], name
        assert call(both=True) == codes["AETHER_EINVAL"], name                 # both decoders named
        assert call(field=False) == codes["AETHER_EINVAL"], name               # no field parameters and no field handed in
        assert call() == 0, name
    del keep


@pytest.mark.parametrize("dec", T.DECODERS)
@pytest.mark.parametrize("D,B", [(2, 7), (3, 5)])
def test_buffer_contract_and_layout_sizes(D, B, dec):
    """The step, the rollout, the full-sequence encoder and the decoder on given logits and a given field inside guarded,
    poisoned buffers (test_gpu_buffer_contract.py, tests/guarded_alloc.py): no guard byte changes, the results equal the plain
    run's bit for bit and the fp64 restatement's at 1e-5.  The allocation record shows what a step is given: a plan and a
    workspace of exactly the new layouts' sizes, not dNRI's smaller and not Aether's larger ones."""
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
        seq_field, _ = m.predict_field(g["seq"].transpose(2, 1).contiguous())              # [B, N, T, D]
        prior, post, (h, c) = m._encoder_forward(g["seq"], seq_field)
        r.result("encoder.prior", prior)
        r.result("encoder.posterior", post)
        # the decoder on given logits and a given field (the step with ext_logits and ext_field: no prior, no field launch)
        m.__dict__["_step_ws"] = None
        given = prior[:, 0].contiguous()
        field, _ = m.predict_field(g["x"])
        s_out, s_dh, s_edges = m.single_step_forward(g["x"], g["dh"], given, True, field, uniform=g["u"])
        r.result("given.out", s_out, output=True)
        r.result("given.edges", s_edges, output=True)
        if s_dh is not None:
            r.result("given.dh", s_dh, output=True)
        rs = T.restatement(m, False, torch.float64)
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
        clear = _gap(w_logits, cpu(g["u"])) > 1e-3                        # the sample equals the restatement's wherever
        assert clear.float().mean() > 0.9                                # rounding cannot move it
        assert torch.equal(r.results["edges"].cpu().argmax(-1)[clear], rs.sample(w_logits, cpu(g["u"])).argmax(-1)[clear])
        return r

    inputs = dict(_s2s_state(make(), B, N, 62), seq=seq)
    guard, got = contract(body, inputs, f"s2s dnri_aether {dec} D{D} B{B}")
    m = make()
    plan_bytes, ws_bytes = _s2s_sizes(m, B, N)
    E, he = B * N * (N - 1), 128
    rec = (1, None) if dec == "rec" else (None, 1)
    assert plan_bytes == lib.aether_s2s_dnri_aether_plan_bytes(*rec, D, he, 128, 64, 3, 64, 2, 0)
    assert ws_bytes == lib.aether_s2s_dnri_aether_workspace_bytes(D, he, 128, 64, 64, 2, B * N, E)
    assert guard.find(nbytes=plan_bytes, dtype=torch.uint8) and guard.find(nbytes=ws_bytes, dtype=torch.uint8)
    others = [lib.aether_s2s_dnri_plan_bytes(*rec, D, he, 128, 64, 3, 64, 2, 0),
              lib.aether_s2s_dnri_workspace_bytes(D, he, 128, 64, 64, 2, B * N, E),
              lib.aether_s2s_step_workspace_bytes(D, he, 128, 64, 64, 2, B * N, E)]
    assert others[0] < plan_bytes and others[1] < ws_bytes < others[2]
    assert not any(guard.find(nbytes=n, dtype=torch.uint8) for n in others)
