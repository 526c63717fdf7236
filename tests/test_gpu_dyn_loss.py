"""calculate_loss(is_train=False) of both variable-N models on the MI355X against the reference's values
(tools/make_golden_dyn_loss.py): logits and predictions at the project's bar max|a - b| <= 1e-5 max|ref| per tensor, in fp32
and in fp64, with every sampled edge type equal; the loss scalars against an fp64 reduction of the device's own tensors and
against the reference; the one-call path against the staged one; frame chunks; the encoder as a drop-in; the refusals; and the
buffer contract under guard bands and poison.  Fixtures only: the reference tree is never read.

Measured (MI355X): see DESIGN 4.8b -- worst tensor error and the scalars' ratios to their bars."""
import ctypes as C

import pytest
import torch

from conftest import scale_rel_err
from guarded_alloc import GuardedAlloc
import test_dyn_loss as T

pytestmark = pytest.mark.gpu
TOL = 1e-5
ML = T.ML
_BUILT = {}


def _cu(v):
    if torch.is_tensor(v):
        return v.cuda()
    if isinstance(v, (list, tuple)):
        return type(v)(_cu(e) for e in v)
    return v


def _case(kind, tag):
    """(model on the device -- built once, never modified --, fixture, host scene, device scene)."""
    if (kind, tag) not in _BUILT:
        model, d = T.build(kind, tag, device="cuda")
        s = T.scene(d, kind, tag)
        _BUILT[kind, tag] = (model, d, s, {k: _cu(v) for k, v in s.items()})
    return _BUILT[kind, tag]


def _args(g):
    return g["inputs"], g["masks"], [g["node_inds"]], [g["graph_info"]]


def _device_samples(logits, uniform, tau):
    """The edge types the loop samples from the device's ``logits`` [1, sum E, K] with the per-step draws (the library's sample
    kernel: the arithmetic of the loop's, statement for statement)."""
    from aether_amd.nn.seq2seq.encoder import gumbel_softmax_hard
    return gumbel_softmax_hard(logits[0], torch.cat(list(uniform)).to(logits.device), tau).argmax(-1).cpu()


def _reference_samples(logits, uniform, tau):
    """The edge types the reference sampled: the pinned formula on its own logits [sum E, K], in their dtype."""
    return T.RL.S.gumbel_hard(logits, torch.cat(list(uniform)).to(logits.dtype), tau).argmax(-1)


@pytest.mark.parametrize("kind,tag", T.EVERY)
def test_parity_with_the_reference(kind, tag):
    """Every setting of the case: prior / posterior logits and all_predictions within 1e-5 scale-relative of the fp32 AND the
    fp64 reference; the last step's edges equal; every one-hot sample equal, none excluded; the scalars two ways."""
    model, d, s, g = _case(kind, tag)
    pre = f"{kind}.{tag}"
    want = lambda k: torch.from_numpy(d[f"{pre}.{k}"])
    prior, post, state = model.encoder(g["inputs"][:, :-1], g["masks"][:, :-1], [g["node_inds"]], [g["graph_info"]])
    for ref in ("ref", "ref64"):
        for name, v in (("prior", prior), ("posterior", post)):
            assert v.shape == (1,) + want(f"{ref}.{name}").shape
            err = scale_rel_err(v[0].cpu(), want(f"{ref}.{name}"))
            print(f"[dyn loss {pre}] {name} logits vs {ref}: {err:.3g}")
            assert err <= TOL, (name, ref)
    for tf, up in ML.settings(tag):
        sn = ML.setting_name(tf, up)
        loss, nll, kl, logits, preds = model.calculate_loss(*_args(g), is_train=False, teacher_forcing=tf, return_logits=True,
                                                            use_prior_logits=up, uniform=g["uniform"])
        assert torch.equal(logits, post) and preds.shape == (1, s["T"] - 1, s["inputs"].shape[2], 4)
        for ref in ("ref", "ref64"):
            err = scale_rel_err(preds[0].cpu(), want(f"{sn}.{ref}.predictions"))
            print(f"[dyn loss {pre} {sn}] predictions vs {ref}: {err:.3g}")
            assert err <= TOL, (sn, ref)
        absent = s["masks"][:, :s["T"] - 1] == 0
        assert float(preds.cpu()[absent].abs().sum()) == 0.0
        # every sample of the loop is the reference's: the device's own logits, the fixture's draws, against the reference's
        # logits in both precisions -- and the last step's edges as the call returns them
        used = prior if up else post
        for ref in ("ref", "ref64"):
            ref_logits = want(f"{ref}.{'prior' if up else 'posterior'}")
            assert torch.equal(_device_samples(used, s["uniform"], ML.TAU), _reference_samples(ref_logits, s["uniform"], ML.TAU)), (sn, ref)
        edges = model.calculate_loss(*_args(g), teacher_forcing=tf, return_edges=True, use_prior_logits=up, uniform=g["uniform"])[3]
        for ref in ("ref", "ref64"):
            # the same one-hot rows; the straight-through form (hard - y) + y rounds a 1 or a 0 by an ulp of 1, no more
            w = want(f"{sn}.{ref}.edges")
            assert edges.shape == (1,) + w.shape and torch.equal(edges[0].cpu().argmax(-1), w.argmax(-1)), (sn, ref)
            assert float((edges[0].cpu().double() - w.double()).abs().max()) <= 2.0 ** -22, (sn, ref)
        # the reduction code: fp64 torch on the device's OWN predictions / logits (a few fp32 roundings over at most a few
        # thousand terms: 1e-6 relative)
        own = T.RL.masked_loss(preds.cpu().double(), s["inputs"].double(), s["masks"], prior.cpu().double(), post.cpu().double())
        for q, got, ref in zip(T.SCALARS, (loss, nll, kl), own):
            r = T.rel(got, ref)
            print(f"[dyn loss {pre} {sn}] {q} vs fp64 reduction of own tensors: {r:.3g}")
            assert r <= 1e-6, (sn, q)
        # each scalar against the reference's fp64 value: max(1e-5, 4 x the reference's own fp32-vs-fp64 difference)
        for q, got in zip(T.SCALARS, (loss, nll, kl)):
            bar = max(1e-5, 4 * float(d[f"{pre}.{sn}.rel32.{q}"]))
            r = T.rel(got, d[f"{pre}.{sn}.ref64.{q}"][0])
            print(f"[dyn loss {pre} {sn}] {q} vs ref64: {r:.3g} (bar {bar:.3g}, ratio {r / bar:.3g})")
            assert r <= bar, (sn, q)
        assert loss.shape == () and nll.shape == (1,) and kl.shape == (1,)
        assert len(model.calculate_loss(*_args(g), teacher_forcing=tf, use_prior_logits=up, uniform=g["uniform"])) == 3
    # the encoder as a drop-in: a zero forward_state of the reference's shape
    Nmax, R = s["inputs"].shape[2], model.encoder.rnn_hidden_size
    assert all(x.shape == (1, Nmax * (Nmax - 1), R) and not bool(x.any()) for x in state)


@pytest.mark.parametrize("kind", T.MODELS)
@pytest.mark.parametrize("tag", ("N9", "L7"))
def test_one_call_equals_staged_and_chunks_do_not_matter(kind, tag):
    """calculate_loss and _calculate_loss_stepwise run the same encoder call and the same decoder kernels in the same order:
    equal bytes.  The F = T - 1 frames in chunks of 2 + 3 (N9) / 2 + 2 (L7), or one at a time, give the same logits byte for
    byte: the frames are independent."""
    model, d, s, g = _case(kind, tag)
    for tf, up in ML.settings(tag):
        a = model.calculate_loss(*_args(g), teacher_forcing=tf, return_logits=True, use_prior_logits=up, uniform=g["uniform"])
        b = model._calculate_loss_stepwise(*_args(g), teacher_forcing=tf, return_logits=True, use_prior_logits=up, uniform=g["uniform"])
        for x, y in zip(a, b):
            assert torch.equal(x, y), (tf, up)
        ea = model.calculate_loss(*_args(g), teacher_forcing=tf, return_edges=True, use_prior_logits=up, uniform=g["uniform"])[3]
        eb = model._calculate_loss_stepwise(*_args(g), teacher_forcing=tf, return_edges=True, use_prior_logits=up, uniform=g["uniform"])[3]
        assert torch.equal(ea, eb)
    enc = (g["inputs"][:, :-1], g["masks"][:, :-1], [g["node_inds"]], [g["graph_info"]])
    whole = model.encoder(*enc)
    try:
        for chunk in ((2, 3), 1):
            model.encoder.__dict__["_seq_chunk"] = chunk
            parts = model.encoder(*enc)
            assert torch.equal(parts[0], whole[0]) and torch.equal(parts[1], whole[1]), chunk
    finally:
        model.encoder.__dict__.pop("_seq_chunk", None)


def _entry_args(model, kind, g, s):
    """The four entries' argument lists at the case's shape, from the module's own structs."""
    from aether_amd import _lib
    from aether_amd.nn.dynamicvars._loss import posterior_struct
    lib = _lib.load()
    T_, Nmax, K = s["T"], s["inputs"].shape[2], model.num_edge_types
    n = [int(x.numel()) for x in s["node_inds"][:T_ - 1]]
    e = [int(gi[0].numel()) for gi in s["graph_info"]]
    deg = [int(gi[2].shape[1]) for gi in s["graph_info"]]
    cfg = model._step_config()
    post, pl, ph = posterior_struct(model.encoder.encoder_fc_out)
    enc_ps = model.encoder._param_struct()[0]
    dec_ps = model.decoder._param_struct()
    if kind == "aether":
        fs = model._field_struct()
        seq_head, loss_head = (C.byref(fs), C.byref(enc_ps)), (C.byref(fs), C.byref(dec_ps))
        seq, loss = lib.aether_dyn_sequence_logits, lib.aether_dyn_loss_rollout
    else:
        seq_head, loss_head = (C.byref(enc_ps),), (C.byref(dec_ps),)
        seq, loss = lib.aether_dyn_dnri_sequence_logits, lib.aether_dyn_dnri_loss_rollout
    keep = (cfg, post, enc_ps, dec_ps)
    return lib, seq, loss, seq_head, loss_head, cfg, post, pl, ph, n, e, deg, keep


@pytest.mark.parametrize("kind", T.MODELS)
def test_refused_calls_queue_nothing_and_write_nothing(kind):
    """A frame with one present object, and a wrong n_edges: the error code, and outputs and workspace as they were."""
    from test_dyn_dnri import _codes
    model, d, s, g = _case(kind, "N3")
    lib, seq, loss, seq_head, loss_head, cfg, post, pl, ph, n, e, deg, keep = _entry_args(model, kind, g, s)
    F, Nmax, K = s["T"] - 1, 3, model.num_edge_types
    i64 = lambda v: (C.c_int64 * len(v))(*v)
    frames, masks = g["inputs"][0].contiguous(), g["masks"][0].contiguous()
    gi = [tuple(t.contiguous() for t in x) for x in g["graph_info"]]
    ptr = lambda j: (C.c_void_p * F)(*[x[j].data_ptr() for x in gi])
    u = (C.c_void_p * F)(*[x.data_ptr() for x in g["uniform"]])
    ws = torch.full((1 << 24,), 0x5A, dtype=torch.uint8, device="cuda")
    outs = [torch.full((sum(e), K), 7.0, device="cuda") for _ in range(2)] + [torch.full((F, Nmax, 4), 7.0, device="cuda"),
                                                                               torch.full((e[-1], K), 7.0, device="cuda")]
    stream = torch.cuda.current_stream().cuda_stream
    for bad_n, bad_e in (([3, 1, 3], [6, 0, 6]), ([3, 3, 3], [6, 5, 6])):
        torch.cuda.synchronize()
        st = seq(*seq_head, C.byref(post), C.byref(cfg), pl, ph, F, Nmax, i64(bad_n), i64(bad_e), frames.data_ptr(), masks.data_ptr(),
                 outs[0].data_ptr(), outs[1].data_ptr(), ws.data_ptr(), ws.numel(), stream)
        assert st == _codes()["AETHER_EINVAL"]
        st = loss(*loss_head, C.byref(cfg), Nmax, F, -1, frames.data_ptr(), masks.data_ptr(), i64(bad_n), i64(bad_e),
                  (C.c_int * F)(*deg), ptr(0), ptr(1), ptr(2), outs[0].data_ptr(), u, outs[2].data_ptr(), outs[3].data_ptr(),
                  ws.data_ptr(), ws.numel(), stream)
        assert st == _codes()["AETHER_EINVAL"]
        torch.cuda.synchronize()
        assert all(bool((o == 7.0).all()) for o in outs) and bool((ws == 0x5A).all())
    # and the module: a sequence with such a frame raises by name
    from aether_amd import _lib
    masks1 = g["masks"].clone()
    masks1[0, 1, 1:] = 0
    ni = [masks1[0, t].nonzero()[:, -1] for t in range(s["T"])]
    with pytest.raises(_lib.AetherHipError, match="fewer than two present objects"):
        model.calculate_loss(g["inputs"], masks1, [ni], [g["graph_info"]], uniform=g["uniform"])


@pytest.mark.parametrize("kind", T.MODELS)
def test_entries_keep_to_their_buffers(kind):
    """The four new entries at the N3 shape with every torch.empty buffer (outputs, the two workspaces) exact-sized, between
    guard bands and filled with NaN bytes: no band byte changes, and the results are those of the plain run -- nothing reads a
    word that nobody wrote."""
    model, d, s, g = _case(kind, "N3")
    plain = [model.calculate_loss(*_args(g), teacher_forcing=tf, return_logits=True, use_prior_logits=up, uniform=g["uniform"])
             for tf, up in ML.settings("N3")]
    model.__dict__.pop("_loss_ws", None)                          # so that both workspaces are allocated inside the harness
    model.encoder.__dict__.pop("_seq_ws", None)
    try:
        with GuardedAlloc() as G:
            guarded = [model.calculate_loss(*_args(g), teacher_forcing=tf, return_logits=True, use_prior_logits=up, uniform=g["uniform"])
                       for tf, up in ML.settings("N3")]
            G.check()
            assert G.holds(model.__dict__["_loss_ws"]) and G.holds(model.encoder.__dict__["_seq_ws"])
    finally:
        model.__dict__.pop("_loss_ws", None)
        model.encoder.__dict__.pop("_seq_ws", None)
    for a, b in zip(plain, guarded):
        for x, y in zip(a, b):
            assert torch.equal(x, y)
