"""seq2seq Aether with decoder_type 'ref_mlp' on the MI355X: the HIP Markov decoder step (aether_s2s_markov_decoder_step)
against the reference's own outputs and the fp64 restatement of test_s2s_markov.py, predict_future / calculate_loss against
the reference, the fused step / rollout (aether_s2s_markov_step / _rollout) against the per-module loop, graph replay,
run-to-run stability and the batched teacher-forced evaluation."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, scale_rel_err
from test_s2s_markov import check_checksums, markov_params, model_params, restate

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _decoder(D, N, H, K, skip, seed):
    from aether_amd.nn.seq2seq.markov import MarkovDecoder
    torch.manual_seed(seed)
    return MarkovDecoder(markov_params(N, D, H, K, skip), device="cuda")


def _model(D, N, K, skip, he=128, hd=128, R=64, layers=3, seed=91):
    from aether_amd.nn.seq2seq.aether import Aether
    params = {"num_vars": N, "input_size": 2 * D, "gpu": True, "decoder_hidden": hd, "num_edge_types": K,
              "skip_first": skip, "decoder_dropout": 0.0, "use_3d": D == 3, "encoder_dropout": 0.0, "encoder_hidden": he,
              "encoder_rnn_hidden": R, "encoder_rnn_type": "lstm", "encoder_mlp_num_layers": 1, "encoder_mlp_hidden": 64,
              "prior_num_layers": layers, "prior_hidden_size": 64, "pos_representation": "polar" if D == 2 else "cart",
              "gumbel_temp": 0.5, "rff_std": 1.0, "decoder_type": "ref_mlp"}
    torch.manual_seed(seed)
    return Aether(params, device="cuda").eval()


# -- the module step --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("kind", ["hard", "soft"])
def test_markov_step_matches_reference(D, K, kind):
    d = np.load(os.path.join(GOLDEN, f"s2s_markov_decoder_D{D}.npz"))
    H, N = int(d["hidden_size"]), int(d["num_vars"])
    dec = _decoder(D, N, H, K, K == 3, int(d["seed"]))
    check_checksums({k: v.cpu() for k, v in dec.state_dict().items()}, d, f"K{K}.")
    inputs, field = torch.from_numpy(d["in.inputs"]), torch.from_numpy(d["in.field"])
    edges = torch.from_numpy(d[f"K{K}.in.edges_{kind}"])
    out, hid = dec(inputs.cuda(), None, edges.cuda(), field.cuda())
    assert hid is None
    assert scale_rel_err(out.cpu(), torch.from_numpy(d[f"K{K}.ref.{kind}.outputs"])) <= TOL
    if D == 2:      # in 3-D the reference's own fp32 and fp64 runs differ by ~5 %: every node's origin edge has an Euler angle
        # on its branch cut (+-pi by one rounding, test_s2s_markov.restate); the fp32 evaluation is the one to match
        assert scale_rel_err(out.cpu(), torch.from_numpy(d[f"K{K}.ref64.{kind}.outputs"])) <= TOL


@pytest.mark.parametrize("N", [2, 5, 20])
@pytest.mark.parametrize("B", [1, 3, 128])
@pytest.mark.parametrize("H", [128, 512])
def test_markov_step_fresh_shapes_vs_fp64(N, B, H):
    D, K, skip = (2, 3, True) if N != 5 else (3, 2, False)
    dec = _decoder(D, N, H, K, skip, 100 + N + B + H)
    sd = {k: v.detach().cpu() for k, v in dec.state_dict().items()}
    g = torch.Generator().manual_seed(N * 1000 + B)
    E = N * (N - 1)
    x = torch.randn(B, N, 2 * D, generator=g)
    f = torch.randn(B, N, D, generator=g) * 0.3
    soft = torch.softmax(torch.randn(B, E, K, generator=g), -1)
    hard = torch.nn.functional.one_hot(torch.randint(0, K, (B, E), generator=g), K).float()
    for w in (soft, hard):
        got, _ = dec(x.cuda(), None, w.cuda(), f.cuda())
        want = restate(sd, x.double(), w.double(), f.double(), D == 3, skip, frames_dtype=torch.float32)
        assert scale_rel_err(got.cpu(), want) <= TOL


# -- predict_future / calculate_loss against the reference ------------------------------------------------------------------
def _fixture_model(name):
    from aether_amd.nn.seq2seq.aether import Aether
    import make_golden_markov as MGM
    d = np.load(os.path.join(GOLDEN, f"s2s_markov_{name}_D2.npz"))
    extra = None if name == "future" else list(MGM.MS.LOSS_CONFIGS.values())[0]
    torch.manual_seed(int(d["seed"]))
    model = Aether(model_params(extra), device=None).eval()
    check_checksums(model.state_dict(), d)
    return d, model.cuda()


def test_predict_future_matches_reference_and_graph_replay_is_bit_identical():
    d, m = _fixture_model("future")
    inputs = torch.from_numpy(d["in.inputs"]).cuda()
    steps = int(d["steps"])
    B, T, N, _ = inputs.shape
    E, K = N * (N - 1), m.num_edge_types
    U = torch.from_numpy(d["in.uniform"]).cuda().view(T - 1 + steps, B, E, K)
    preds, edges = m.predict_future(inputs, steps, return_edges=True, uniform=U)
    ref_p, ref_e = torch.from_numpy(d["ref.predictions"]), torch.from_numpy(d["ref.edges"])
    assert torch.equal(edges.argmax(-1).cpu(), ref_e.argmax(-1))
    assert scale_rel_err(preds.cpu(), ref_p) <= TOL
    g1, ge = m.predict_future(inputs, steps, return_edges=True, uniform=U, graph=True)
    g2 = m.predict_future(inputs, steps, uniform=U, graph=True)
    assert torch.equal(g1, preds) and torch.equal(ge, edges) and torch.equal(g2, preds)


@pytest.mark.parametrize("name", ["gaussian_norm", "crossent_tf2_uniform"])
def test_calculate_loss_matches_reference(name):
    from aether_amd.nn.seq2seq.aether import Aether
    d = np.load(os.path.join(GOLDEN, "s2s_markov_loss_D2.npz"))
    import make_golden_markov as MGM
    torch.manual_seed(int(d["seed"]))
    m = Aether(model_params(MGM.MS.LOSS_CONFIGS[name]), device="cuda").eval()
    inputs = torch.from_numpy(d["in.inputs"]).cuda()
    B, T, N, _ = inputs.shape
    E, K = N * (N - 1), m.num_edge_types
    U = torch.from_numpy(d[f"{name}.uniform"]).cuda().view(T - 1, B, E, K)
    loss, nll, kl = m.calculate_loss(inputs, is_train=False, uniform=U)
    for got, key in ((loss, "loss"), (nll, "nll"), (kl, "kl")):
        assert scale_rel_err(got.cpu(), torch.from_numpy(d[f"{name}.{key}"])) <= TOL, key
    _, _, _, _, preds = m.calculate_loss(inputs, is_train=False, uniform=U, return_logits=True)
    assert scale_rel_err(preds.cpu(), torch.from_numpy(d[f"{name}.predictions"])) <= TOL


@pytest.mark.parametrize("tf", [-1, 2, 0])
def test_batched_teacher_forced_eval_equals_step_loop(tf):
    m = _model(2, 5, 3, True)
    m.val_teacher_forcing_steps = tf
    g = torch.Generator().manual_seed(40 + tf)
    B, T, N = 16, 7, 5
    E = N * (N - 1)
    inputs = torch.randn(B, T, N, 4, generator=g).cuda()
    U = torch.rand(T - 1, B, E, 3, generator=g).cuda()
    got = m.calculate_loss(inputs, is_train=False, uniform=U)
    want = m._calculate_loss_stepwise(inputs, True, U)
    for a, b in zip(got, want):
        assert scale_rel_err(a.cpu(), b.cpu()) <= TOL


# -- the fused step / rollout -----------------------------------------------------------------------------------------------
def _state(m, B, N, g):
    E, R = N * (N - 1), m.encoder.rnn_hidden_size
    return ((torch.randn(B, E, R, generator=g) * 0.3).cuda(), (torch.randn(B, E, R, generator=g) * 0.3).cuda())


@pytest.mark.parametrize("N", [5, 20])
@pytest.mark.parametrize("structure", [2, 3])
def test_fused_step_and_rollout_equal_stepwise(N, structure):
    from aether_amd import _lib
    D, B, K, steps = 2, 128, 3, 3
    m = _model(D, N, K, True, he=128, hd=512)
    g = torch.Generator().manual_seed(N + structure)
    E = N * (N - 1)
    x = torch.randn(B, N, 2 * D, generator=g).cuda()
    st = _state(m, B, N, g)
    u = torch.rand(steps, B, E, K, generator=g).cuda()
    lib = _lib.load()
    try:
        lib.aether_set_option(b"gemm_split", structure)
        field, _ = m.predict_field(x)
        logits, (h1, c1) = m.encoder.single_step_forward(x, st, field)
        want_x, want_dh, want_e = m.single_step_forward(x, None, logits, True, field, uniform=u[0])
        got_x, got_dh, (got_h, got_c), got_e = m._fused_step(x, None, st, u[0])
        assert want_dh is None and got_dh is None
        same = (got_e == want_e).all(dim=-1).all(dim=-1)                   # graphs without a sample on its rounding
        assert same.float().mean() > 0.99
        assert scale_rel_err(got_x[same].cpu(), want_x[same].cpu()) <= TOL
        assert scale_rel_err(got_h.cpu(), h1.cpu()) <= TOL and scale_rel_err(got_c.cpu(), c1.cpu()) <= TOL
        want, want_e = m.predict_from_state_stepwise(x, None, st, steps, uniform=u, return_edges=True)
        got, got_e = m.predict_from_state(x, None, st, steps, uniform=u, return_edges=True)
        again, again_e = m.predict_from_state(x, None, st, steps, uniform=u, return_edges=True)
    finally:
        lib.aether_set_option(b"gemm_split", 1)
    assert torch.equal(again, got) and torch.equal(again_e, got_e)     # run-to-run stable
    same = (got_e == want_e).all(dim=-1).all(dim=-1)
    assert same.float().mean() > 0.95
    ok = same.cumprod(dim=1).bool()                                     # up to the first flipped sample of each graph
    err = ((got - want).abs().amax(dim=(-1, -2)) / want.abs().amax().clamp_min(1.0))[ok]
    assert float(err.max()) <= TOL


@pytest.mark.parametrize("B", [6, 128])
def test_fused_step_with_an_empty_edge_type(B):
    """Type 1 never sampled (its Gumbel noise loses every race): its row list is empty; type 0 is skipped (skip_first)
    and its edges carry no message.  Fp32 job kernel (B = 6) and split GEMM (B = 128, 48,640 edges)."""
    D, N, K = 2, 20, 3
    m = _model(D, N, K, True, hd=512)
    g = torch.Generator().manual_seed(81 + B)
    E = N * (N - 1)
    x = torch.randn(B, N, 2 * D, generator=g).cuda()
    st = _state(m, B, N, g)
    u = torch.empty(B, E, K)
    u[..., 0], u[..., 1], u[..., 2] = 1.0 - 1e-7, 1e-7, 1.0 - 1e-7
    u = u.cuda()
    field, _ = m.predict_field(x)
    logits, _ = m.encoder.single_step_forward(x, st, field)
    want_x, _, want_e = m.single_step_forward(x, None, logits, True, field, uniform=u)
    assert float(want_e[..., 1].abs().max()) == 0.0                      # the premise: nobody picked type 1
    assert float(want_e[..., 0].abs().max()) > 0 and float(want_e[..., 2].abs().max()) > 0
    got_x, _, _, got_e = m._fused_step(x, None, st, u)
    assert torch.equal(got_e, want_e)
    assert scale_rel_err(got_x.cpu(), want_x.cpu()) <= TOL


def test_rollout_burn_in_runs_the_prior_only_and_is_stable():
    """The device rollout with burn-in equals chaining the fused step (burn-in predictions discarded, the same uniform rows
    consumed), graph replay equals the eager rollout bit for bit, and two identical rollouts are bit-identical."""
    D, N, B, K = 2, 5, 128, 3
    m = _model(D, N, K, True, hd=512)
    g = torch.Generator().manual_seed(7)
    E, T, steps = N * (N - 1), 4, 5
    inputs = torch.randn(B, T, N, 2 * D, generator=g).cuda()
    U = torch.rand(T - 1 + steps, B, E, K, generator=g).cuda()
    a = m.predict_future(inputs, steps, uniform=U)
    b = m.predict_future(inputs, steps, uniform=U)
    c = m.predict_future(inputs, steps, uniform=U, graph=True)
    assert torch.equal(a, b) and torch.equal(a, c)
    R = m.encoder.rnn_hidden_size
    st = (torch.zeros(B, E, R, device="cuda"), torch.zeros(B, E, R, device="cuda"))
    for t in range(T - 1):
        _, _, st, _ = m._fused_step(inputs[:, t], None, st, U[t])
    xx, outs = inputs[:, T - 1], []
    for t in range(steps):
        xx, _, st, _ = m._fused_step(xx, None, st, U[T - 1 + t])
        outs.append(xx)
    assert torch.equal(a, torch.stack(outs, 1))
