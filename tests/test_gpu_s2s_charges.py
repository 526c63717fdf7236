"""The charge-aware seq2seq Aether on the MI355X: the staged field query, the fused step and the device rollout against the
reference's values (tools/make_golden_s2s_charges.py) and against the fp64 restatement (tests/s2s_charges_restatement.py) on
fresh shapes, at the project's tolerance max|a - b| <= 1e-5 max|ref| per tensor.  Multi-step comparisons go through the hard
Gumbel sample: trajectories are compared where the sampled edge types agree, and at least 95 % of the (step, edge) samples
must (the fixtures' noise seeds were chosen so that the fp32 reference and the fp64 restatement agree on all of them)."""
import pytest
import torch

from conftest import scale_rel_err
import test_s2s_charges as T

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _params(D, N, K=2, skip=False, he=128, hd=128, R=64):
    return {"num_vars": N, "input_size": 2 * D, "gpu": True, "decoder_hidden": hd, "num_edge_types": K, "skip_first": skip,
            "decoder_dropout": 0.0, "use_3d": D == 3, "encoder_dropout": 0.0, "encoder_hidden": he, "encoder_rnn_hidden": R,
            "encoder_rnn_type": "lstm", "encoder_mlp_num_layers": 3, "encoder_mlp_hidden": 64, "prior_num_layers": 3,
            "prior_hidden_size": 64, "pos_representation": "polar", "gumbel_temp": 0.5, "rff_std": 1.0}


def _fresh_model(D, N, seed, **kw):
    from aether_amd.nn.seq2seq.ablations import AetherCharges
    from make_golden_dynamicvars import perturb_bn_
    torch.manual_seed(seed)
    model = AetherCharges(_params(D, N, **kw), device=None).eval()
    with torch.no_grad():
        perturb_bn_(model)
    return model.cuda()


def _agreeing(got_e, want_e, got, want, floor):
    """Trajectories [B, steps, N, F] where the samples [B, steps, E, K] agree, each graph up to its first flipped sample."""
    same_edge = (got_e.argmax(-1) == want_e.argmax(-1))
    assert same_edge.float().mean() >= floor, float(same_edge.float().mean())
    ok = same_edge.all(-1).cumprod(dim=1).bool()
    assert ok.any()
    err = ((got - want).abs().amax(dim=(-1, -2)) / want.abs().amax().clamp_min(1e-30))[ok]
    return float(err.max())


def _same_graphs(got_e, want_e, floor=0.95):
    """One step's samples [B, E, K]: at least ``floor`` of the (graph, edge) samples agree -> the graphs [B] without a flipped one
    (a graph with a flipped sample computes something else from there on and is compared no further)."""
    same_edge = got_e.argmax(-1) == want_e.argmax(-1)
    assert same_edge.float().mean() >= floor, float(same_edge.float().mean())
    same = same_edge.all(-1)
    assert same.any()
    return same


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("tag", T.CASES)
def test_field_step_and_rollout_match_the_reference(D, tag):
    import make_golden_s2s_charges as MG
    model, d = T.build(D, tag, device="cuda")
    B, N, skip, _ = MG.CASES[tag]
    inputs, charges, cidx, U = T.case_inputs(d, tag)
    E, K, R, H, steps = N * (N - 1), int(d["num_edge_types"]), int(d["rnn_hidden"]), int(d["hidden"]), int(d["steps"])
    want = lambda k: torch.from_numpy(d[f"{tag}.ref.{k}"])
    x, ch = inputs.cuda(), charges.cuda()
    # the staged field query: 3-D and 4-D x, with the embedding (the reference's argument) and with the index
    emb = model.charge_embedding(cidx.cuda())
    x4 = x[:, :-1].transpose(2, 1).contiguous()
    f4, coords = model.predict_field(x4, emb)
    assert torch.equal(coords, x4[..., :D])
    assert scale_rel_err(f4.cpu(), want("field4")) <= TOL
    f0, _ = model.predict_field(x[:, 0], cidx.cuda())
    assert scale_rel_err(f0.cpu(), want("field0")) <= TOL
    # one fused step from the zero state
    model._set_charges(cidx, B, N, "cuda")
    zeros = lambda *s: torch.zeros(*s, device="cuda")
    out, dh, (h1, c1), edges = model._fused_step(x[:, 0], zeros(B, N, H), (zeros(B, E, R), zeros(B, E, R)),
                                                 U[0].view(B, E, K).cuda())
    assert torch.equal(edges.argmax(-1).cpu(), want("step_edges").argmax(-1))
    for name, got in (("prior_h", h1), ("prior_c", c1), ("decoder_out", out), ("decoder_hidden", dh)):
        assert scale_rel_err(got.cpu(), want(name)) <= TOL, name
    # the decoder on given logits (single_step_forward): the fixture's prior logits, the same draw
    sp, sdh, se = model.single_step_forward(x[:, 0], zeros(B, N, H), want("prior_logits").cuda(), True, f0, emb,
                                            uniform=U[0].view(B, E, K).cuda())
    assert torch.equal(se.argmax(-1).cpu(), want("step_edges").argmax(-1))
    assert scale_rel_err(sp.cpu(), want("decoder_out")) <= TOL and scale_rel_err(sdh.cpu(), want("decoder_hidden")) <= TOL
    # 3 burn-in + 4 predicted steps on the device
    u = U.view(-1, B, E, K).cuda()
    preds, pe = model.predict_future(x, steps, return_edges=True, charges=ch, uniform=u)
    assert _agreeing(pe.cpu(), want("edges"), preds.cpu(), want("predictions"), 0.95) <= TOL
    # the captured rollout is the eager one bit for bit, twice
    for _ in range(2):
        gp, ge = model.predict_future(x, steps, return_edges=True, charges=ch, uniform=u, graph=True)
        assert torch.equal(gp, preds) and torch.equal(ge, pe)
    # return_everything: the burn-in steps' predictions in front of the same predictions
    everything = model.predict_future(x, steps, return_everything=True, charges=ch, uniform=u)
    assert everything.shape[1] == inputs.shape[1] - 1 + steps
    assert scale_rel_err(everything[:, -steps:].cpu(), preds.cpu()) <= TOL


@pytest.mark.parametrize("D", [2, 3])
def test_fresh_shapes_against_the_fp64_restatement(D):
    """N = 4, B = 3, K = 3 with skip_first, random charges (a 0 among them) and a random state."""
    N, B, K, steps, Tb = 4, 3, 3, 4, 4
    model = _fresh_model(D, N, 300 + D, K=K, skip=True)
    E, R, H = N * (N - 1), 64, 128
    g = torch.Generator().manual_seed(40 + D)
    inputs = torch.randn(B, Tb, N, 2 * D, generator=g)
    charges = torch.randint(-1, 2, (B, N), generator=g).float()
    cidx = model.charge_to_index(charges)
    U = torch.rand(Tb - 1 + steps, B, E, K, generator=g)
    state = (torch.randn(B, E, R, generator=g) * 0.3, torch.randn(B, E, R, generator=g) * 0.3)
    hidden = torch.randn(B, N, H, generator=g) * 0.3
    rs = T.restatement(model, D, True, torch.float64, frames_dtype=torch.float32 if D == 3 else None)
    x0 = inputs[:, 0].double()
    w_out, w_hid, (w_h, w_c), w_z, _, w_field = rs.step(x0, hidden.double(), tuple(t.double() for t in state), U[0].double(), cidx)
    f0, _ = model.predict_field(inputs[:, 0].cuda(), cidx.cuda())
    assert scale_rel_err(f0.cpu(), w_field) <= TOL
    model._set_charges(cidx, B, N, "cuda")
    out, dh, (h1, c1), z = model._fused_step(inputs[:, 0].cuda(), hidden.cuda(), tuple(t.cuda() for t in state), U[0].cuda())
    assert scale_rel_err(h1.cpu(), w_h) <= TOL and scale_rel_err(c1.cpu(), w_c) <= TOL
    same = _same_graphs(z.cpu(), w_z)
    assert scale_rel_err(out.cpu()[same], w_out[same]) <= TOL and scale_rel_err(dh.cpu()[same], w_hid[same]) <= TOL
    w_preds, w_edges = rs.predict_future(inputs, steps, U.double(), cidx)
    preds, edges = model.predict_future(inputs.cuda(), steps, return_edges=True, charges=charges.cuda(), uniform=U.cuda())
    assert _agreeing(edges.cpu(), w_edges, preds.cpu(), w_preds, 0.95) <= TOL


@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("name", T.LOSS_NAMES)
def test_calculate_loss_matches_the_reference(D, name):
    """calculate_loss(is_train=False, charges=) with the charge-aware full-sequence encoder against the reference's values:
    posterior logits, predictions (where the samples agree: every step's posterior sample is re-derived from the fixture's
    logits and draws) and the loss terms."""
    from oracle import seq2seq_oracle as S
    model, params, d = T.loss_model(D, name)
    model = model.cuda()
    t = lambda k: torch.from_numpy(d[k])
    inputs, charges, U = t("loss.in.inputs"), t("loss.in.charges"), t(f"loss.{name}.uniform")
    B, Tn, N, _ = inputs.shape
    E, K = N * (N - 1), U.shape[-1]
    u = U.view(Tn - 1, B, E, K).cuda()
    loss, nll, kl, post, preds = model.calculate_loss(inputs.cuda(), is_train=False, return_logits=True, charges=charges.cuda(),
                                                      uniform=u)
    want = lambda k: t(f"loss.{name}.{k}")
    assert scale_rel_err(post.cpu(), want("posterior")) <= TOL
    z_got = torch.stack([S.gumbel_hard(post.cpu()[:, s].reshape(-1, K), U[s], 0.5) for s in range(Tn - 1)])
    z_ref = torch.stack([S.gumbel_hard(want("posterior")[:, s].reshape(-1, K), U[s], 0.5) for s in range(Tn - 1)])
    assert torch.equal(z_got.argmax(-1), z_ref.argmax(-1))               # (the fixture's noise seed leaves a clear margin)
    assert scale_rel_err(preds.cpu(), want("predictions")) <= TOL
    for key, got in (("loss", loss), ("nll", nll), ("kl", kl)):
        assert scale_rel_err(got.cpu(), want(key)) <= TOL, key
    assert "charges" in __import__("inspect").signature(model.calculate_loss).parameters
    _, _, _, e = model.calculate_loss(inputs.cuda(), is_train=False, return_edges=True, charges=charges.cuda(), uniform=u)
    assert torch.equal(e.cpu().argmax(-1).reshape(-1), z_ref[-1].argmax(-1))


@pytest.mark.parametrize("structure", [2, 3])
def test_bias_tables_on_the_split_gemms(structure):
    """1,000 nodes / 4,000 edges with decoder_hidden 512: the field query's first layer, the present-message layer (its table
    row by edge id, behind the per-type row lists) and the gates run on the two-piece fp16 GEMMs, in both of their
    structures; one step against the fp64 restatement."""
    from aether_amd import _lib
    D, N, B, K = 2, 5, 200, 2
    model = _fresh_model(D, N, 77, K=K, hd=512)
    E, R, H = N * (N - 1), 64, 512
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, N, 2 * D, generator=g)
    charges = (torch.randint(0, 2, (B, N), generator=g) * 2 - 1).float()
    cidx = model.charge_to_index(charges)
    u = torch.rand(B, E, K, generator=g)
    state = (torch.randn(B, E, R, generator=g) * 0.3, torch.randn(B, E, R, generator=g) * 0.3)
    hidden = torch.randn(B, N, H, generator=g) * 0.3
    rs = T.restatement(model, D, False, torch.float64)
    w_out, w_hid, (w_h, w_c), w_z, _, _ = rs.step(x.double(), hidden.double(), tuple(t.double() for t in state), u.double(), cidx)
    model._set_charges(cidx, B, N, "cuda")
    lib = _lib.load()
    try:
        lib.aether_set_option(b"gemm_split", structure)
        out, dh, (h1, c1), z = model._fused_step(x.cuda(), hidden.cuda(), tuple(t.cuda() for t in state), u.cuda())
        torch.cuda.synchronize()
    finally:
        lib.aether_set_option(b"gemm_split", 1)
    assert scale_rel_err(h1.cpu(), w_h) <= TOL and scale_rel_err(c1.cpu(), w_c) <= TOL
    same = _same_graphs(z.cpu(), w_z)
    assert scale_rel_err(out.cpu()[same], w_out[same]) <= TOL and scale_rel_err(dh.cpu()[same], w_hid[same]) <= TOL


def test_a_charge_index_out_of_range_gives_nan_rows_and_an_error():
    """A well-formed launch with an index of 2: no table is read out of bounds; that node's outputs are NaN, the other graph's
    are what they are without it, and aether_check_async_error reports AETHER_EHIP once."""
    from aether_amd import _lib
    model, d = T.build(2, "B2N5", device="cuda")
    B, N, E, K, R, H = 2, 5, 20, 2, 64, 128
    inputs, _, cidx, U = T.case_inputs(d, "B2N5")
    x0, u0 = inputs[:, 0].cuda(), U[0].view(B, E, K).cuda()
    zeros = lambda *s: torch.zeros(*s, device="cuda")
    lib = _lib.load()
    lib.aether_check_async_error()                                        # (clear)
    model._set_charges(cidx, B, N, "cuda")
    good, good_dh, _, _ = model._fused_step(x0, zeros(B, N, H), (zeros(B, E, R), zeros(B, E, R)), u0)
    bad = cidx.clone()
    bad[0, 3] = 2
    model._set_charges(bad, B, N, "cuda")
    out, dh, _, _ = model._fused_step(x0, zeros(B, N, H), (zeros(B, E, R), zeros(B, E, R)), u0)
    torch.cuda.synchronize()
    assert torch.isnan(out[0, 3]).all() and torch.isnan(dh[0, 3]).all()
    assert torch.equal(out[1], good[1]) and torch.equal(dh[1], good_dh[1])
    assert lib.aether_check_async_error() == -3                           # AETHER_EHIP
    assert b"charge index" in lib.aether_last_error()
    assert lib.aether_check_async_error() == 0
    f, _ = model.predict_field(x0, bad.cuda())
    torch.cuda.synchronize()
    assert torch.isnan(f[0, 3]).all() and torch.isfinite(f[1]).all()
    assert lib.aether_check_async_error() == -3
