"""The variable-N dNRI baseline on the MI355X: the staged prior and decoder steps, the one-call step and the device rollout
against the reference's values (tools/make_golden_dyn_dnri.py) at the project's bar max|a - b| <= 1e-5 max|ref| per tensor,
in fp32 and in fp64, with every sampled edge type equal (the fixtures' noise seeds leave every Gumbel race a margin of 1e-3);
one path (list, pack, one-call step and staged calls give equal bytes); many ragged scenes in one call against the fp64
restatement scene by scene; the predicted update at 4 x the fp32 restatement's floor (tests/update_parity.py); the buffer
contract; the refusals; and the inD metric on the model unchanged.  Fixtures only: the reference tree is never read."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import scale_rel_err
import test_dyn_dnri as T
from update_parity import check_update

pytestmark = pytest.mark.gpu
TOL = 1e-5
MG = T.MG
MARGIN = MG.MARGIN
_BUILT = {}


def _model(tag):
    """The case's model on the device, built once and never modified."""
    if tag not in _BUILT:
        _BUILT[tag] = T.build(tag, device="cuda")
    return _BUILT[tag]


def _cu(v):
    if torch.is_tensor(v):
        return v.cuda()
    if isinstance(v, (list, tuple)):
        return type(v)(_cu(e) for e in v)
    return v


def _scene(tag):
    model, _, d = _model(tag)
    s = T.scene(d, tag)
    return model, d, s, {k: _cu(v) for k, v in s.items()}


# -- one step -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", T.CASES)
def test_staged_steps_match_the_reference(tag):
    """The staged prior step from a non-zero LSTM state and the staged decoder step on the fixture's one-hot sample from a
    non-zero hidden state: logits, h1, c1 (the whole slot table), prediction and hidden state against fp32 and fp64."""
    model, d, s, g = _scene(tag)
    x0, m0 = g["inputs"][:, 0], g["masks"][:, 0]
    logits, (h1, c1) = model.encoder.single_step_forward(x0, m0, g["node_inds"][0], g["graph_info"][0], g["state0"])
    pred, hid = model.decoder(x0, g["hidden0"], g["step_edges"], m0, g["graph_info"][0])
    got = {"logits": logits, "h1": h1, "c1": c1, "pred": pred, "hidden": hid}
    for name, v in got.items():
        for ref in ("ref", "ref64"):
            want = torch.from_numpy(d[f"{tag}.{ref}.{name}"])
            assert v.shape == want.shape, name
            err = scale_rel_err(v.cpu(), want)
            print(f"[dyn dnri {tag}] step {name} vs {ref}: {err:.3g}")
            assert err <= TOL, (name, ref)
    absent = s["masks"][0, 0] == 0
    assert float(pred[0].cpu()[absent].abs().sum()) == 0.0
    # untouched where the step has no business: slots of pairs without an edge, hidden rows of absent objects
    slot_touched = (h1 != g["state0"][0]).any(-1)[0]
    assert int(slot_touched.sum()) <= s["graph_info"][0][0].numel()
    assert torch.equal(hid[0][absent.cuda()], g["hidden0"][0][absent.cuda()])
    # single_step_forward of the model samples with the given draw and decodes: the fixture's sample, the same prediction
    p2, h2, z = model.single_step_forward(x0, m0, g["graph_info"][0], g["hidden0"], logits, True, uniform=g["uniform"][0])
    assert torch.equal(z.cpu().argmax(-1), s["step_edges"].argmax(-1))
    assert torch.equal(p2, pred) and torch.equal(h2, hid)


# -- the loop, on one path ----------------------------------------------------------------------------------------------------
def _step_loop(model, g, T_):
    """predict_future as a host loop over the one-call step -> (predictions [1, T - 1, Nmax, 4], edge types per step)."""
    ph, pc = model.encoder.get_initial_hidden(g["inputs"])
    dec = model.decoder.get_initial_hidden(g["inputs"])
    last = g["inputs"][:, 0]
    preds, types = [], []
    for t in range(T_ - 1):
        obs = g["burn"][:, t].unsqueeze(-1)
        state = obs * g["inputs"][:, t] + (1 - obs) * last
        gs, gr, e2n = g["graph_info"][t]
        last, ph, pc, dec, et = model._step_one_call(state, g["masks"][:, t], g["node_inds"][t], gs, gr, e2n, ph, pc, dec,
                                                     g["uniform"][t], return_edge_types=True)
        preds.append(last)
        types.append(et)
    return torch.stack(preds, 1), types


@pytest.mark.parametrize("tag", T.CASES)
def test_rollout_matches_the_reference_on_one_path(tag):
    from aether_amd.nn.dynamicvars.aether_dynamicvars import pack_scenes
    model, d, s, g = _scene(tag)
    args = (g["inputs"], g["masks"], [g["node_inds"]], [g["graph_info"]], g["burn"])
    preds = model.predict_future(*args, uniform=g["uniform"])
    for ref in ("ref", "ref64"):
        err = scale_rel_err(preds.cpu(), torch.from_numpy(d[f"{tag}.{ref}.predictions"]))
        print(f"[dyn dnri {tag}] predict_future vs {ref}: {err:.3g}")
        assert err <= TOL, ref
    absent = s["masks"][:, :s["T"] - 1] == 0
    assert float(preds.cpu()[absent].abs().sum()) == 0.0                         # exactly zero, not merely small
    # the one-call step, step by step: equal bytes, and every step's sample is the reference's
    loop, types = _step_loop(model, g, s["T"])
    assert torch.equal(loop, preds)
    for t, (got, want) in enumerate(zip(types, s["edges"])):
        assert torch.equal(got.cpu().argmax(-1), want.argmax(-1)), t
        assert torch.equal(got.cpu(), want), t
    # the staged calls with torch glue, the batched entry point and the device-built pack of the same scene
    model.one_call_step = False
    try:
        staged = model.predict_future(*args, uniform=g["uniform"])
    finally:
        model.one_call_step = True
    assert torch.equal(staged, preds)
    assert torch.equal(model.predict_future_batched(*args, uniform=[[u] for u in g["uniform"]]), preds)
    pack = pack_scenes(g["inputs"], g["masks"])
    ni, gi = pack.as_lists()
    for t in range(s["T"] - 1):                                                  # the pack's graphs are the fixture's
        assert torch.equal(ni[0][t].cpu(), s["node_inds"][t])
        for a, b in zip(gi[0][t], s["graph_info"][t]):
            assert torch.equal(a.cpu(), b), t
    packed = model.predict_future_packed(g["inputs"], g["masks"], g["burn"], pack, uniform=[[u] for u in g["uniform"]])
    assert torch.equal(packed, preds)
    assert torch.equal(model.predict_future(*args, uniform=g["uniform"]), preds)  # two runs: equal bytes


# -- many scenes in one call ----------------------------------------------------------------------------------------------------
COUNTS = [[0, 0, 0, 0], [2, 2, 2, 2], [3, 0, 3, 3], [7, 7, 8, 7], [13, 13, 13, 12], [20, 20, 20, 20]]
_MANY = {}


def _many():
    """Six scenes of 20 slots with 0, 2, 3, 7, 13 and 20 present objects (scene 2 is empty at step 1), the N9 model, and the
    fp64 restatement of every scene alone.  The draws come from the first generator seed that leaves every Gumbel race of the
    fp64 restatement a margin of 1e-3: the case tests the layers, not a race.  Built once, never modified."""
    if _MANY:
        return _MANY
    from test_gpu_dynamicvars import _scenes
    model, _, _ = _model("N9")
    rs = T.restatement(model, "N9", torch.float64)
    K, N, B, Tn = 3, 20, len(COUNTS), len(COUNTS[0])
    for seed in range(70, 110):
        s = _scenes(COUNTS, N, seed, K)
        want, ok = [], True
        for b in range(B):
            u = [s["uniform"][t][b].double() for t in range(Tn - 1)]
            p, z, lg = rs.predict_future(s["inputs"][b], s["masks"][b], s["node_inds"][b], s["graph_info"][b], s["burn"][b], u,
                                         return_all=True)
            for t in range(Tn - 1):
                if lg[t].numel() and MG.min_margin(lg[t], u[t], MG.TAU) <= MARGIN:
                    ok = False
            want.append(p)
        if ok:
            break
    else:
        raise RuntimeError("no seed with unambiguous samples")
    _MANY.update(model=model, host=s, dev={k: _cu(v) for k, v in s.items()}, want=torch.stack(want), B=B, N=N, T=Tn, K=K)
    return _MANY


def _raw_rollout(model, pack, prior_h, prior_c, dec, preds, n_present=None, n_edges=None, masks=None, ws_short=0):
    """aether_dyn_dnri_rollout_batched on the arrays ``_predict_future_rollout(return_pack=True)`` marshalled -> status."""
    from aether_amd import _lib
    lib = _lib.load()
    cfg, B, N, S = pack["cfg"], preds.shape[1], pack["n_objects_max"], pack["n_steps"]
    n_present = pack["n_present"] if n_present is None else n_present
    n_edges = pack["n_edges"] if n_edges is None else n_edges
    need = lib.aether_dyn_dnri_rollout_batched_workspace_bytes(C.byref(cfg), B, N, S, pack["n_present"], pack["n_edges"],
                                                               pack["in_degree"])
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ps_e, ps_d = model.encoder._param_struct()[0], model.decoder._param_struct()
    p = pack["ptrs"]
    st = lib.aether_dyn_dnri_rollout_batched(C.byref(ps_e), C.byref(ps_d), C.byref(cfg), B, N, S, pack["inputs"].data_ptr(),
                                             (pack["masks"] if masks is None else masks).data_ptr(),
                                             pack["burn_in_masks"].data_ptr(), n_present, n_edges, pack["in_degree"], p["ni"],
                                             p["gs"], p["gr"], p["e2n"], p["u"], prior_h.data_ptr(), prior_c.data_ptr(),
                                             dec.data_ptr(), preds.data_ptr(), ws.data_ptr(), need - ws_short,
                                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st


def test_many_scenes_in_one_call():
    m = _many()
    model, g, B, N, Tn = m["model"], m["dev"], m["B"], m["N"], m["T"]
    got, pack = model._predict_future_rollout(g["inputs"], g["masks"], g["node_inds"], g["graph_info"], g["burn"], g["uniform"],
                                              return_pack=True)
    assert got.shape == (B, Tn - 1, N, 4)
    worst = 0.0
    for b in range(B):
        if not any(COUNTS[b][:Tn - 1]):
            assert float(got[b].abs().max()) == 0.0
            continue
        err = scale_rel_err(got[b].cpu(), m["want"][b])
        print(f"[dyn dnri many] scene {b} ({COUNTS[b]}) vs its fp64 restatement alone: {err:.3g}")
        assert err <= TOL, b
        # the same scene through the library alone: the batch against the single-scene call
        u_b = [g["uniform"][t][b] for t in range(Tn - 1)]
        alone = model.predict_future(g["inputs"][b:b + 1], g["masks"][b:b + 1], [g["node_inds"][b]], [g["graph_info"][b]],
                                     g["burn"][b:b + 1], uniform=u_b)
        worst = max(worst, scale_rel_err(got[b:b + 1].cpu(), alone.cpu()))
        assert scale_rel_err(alone.cpu(), m["want"][b:b + 1]) <= TOL
    print(f"[dyn dnri many] largest batch-against-single-scene difference: {worst:.3g}")
    assert worst <= TOL
    assert float(got[2, 1].abs().max()) == 0.0 and float(got[2, 0].abs().max()) > 0.0      # scene 2 is empty at step 1
    absent = m["host"]["masks"][:, :Tn - 1] == 0
    assert float(got.cpu()[absent].abs().sum()) == 0.0
    # the states through the C entry, from non-zero values: the empty scene's slots and hidden rows are untouched, every
    # other scene's moved; the predictions are the module's
    R, hd, slots = 64, 128, N * (N - 1)
    gen = torch.Generator().manual_seed(3)
    ph0, pc0 = torch.randn(B * slots, R, generator=gen).cuda() * 0.1, torch.randn(B * slots, R, generator=gen).cuda() * 0.1
    dec0 = torch.randn(B, N, hd, generator=gen).cuda() * 0.1
    ph, pc, dec = ph0.clone(), pc0.clone(), dec0.clone()
    preds = torch.empty(Tn - 1, B, N, 4, device="cuda")
    assert _raw_rollout(model, pack, ph, pc, dec, preds) == 0
    assert torch.isfinite(preds).all()
    assert torch.equal(ph[:slots], ph0[:slots]) and torch.equal(pc[:slots], pc0[:slots]) and torch.equal(dec[0], dec0[0])
    for b in range(1, B):
        assert not torch.equal(ph[b * slots:(b + 1) * slots], ph0[b * slots:(b + 1) * slots]), b
        assert not torch.equal(dec[b], dec0[b]), b
    zero = lambda: (torch.zeros_like(ph0), torch.zeros_like(pc0), torch.zeros_like(dec0))
    a, b_ = zero(), zero()
    pa, pb = torch.empty_like(preds), torch.empty_like(preds)
    assert _raw_rollout(model, pack, *a, pa) == 0 and _raw_rollout(model, pack, *b_, pb) == 0
    assert torch.equal(pa.transpose(0, 1), got) and torch.equal(pa, pb)
    for x, y in zip(a, b_):
        assert torch.equal(x, y)


# -- the smallest scenes, an empty step among them ----------------------------------------------------------------------------------
SMALLEST = [[2, 2, 0, 5, 3, 2], [3, 0, 2, 2, 5, 4]]


def test_smallest_scenes_and_an_empty_step_on_one_path():
    """Two scenes of 5 object rows over 6 steps (test_gpu_dynamicvars' smallest scenes): scene 0 has [2, 2, 0, 5, 3, 2] present
    objects -- k = 1 with two edges and in_degree 1, a step with nobody anywhere when it runs alone (the step's all-empty
    branch: zeros, states untouched), a full scene.  Scene 0 alone is exactly zero at step 2, equals the staged loop's bytes
    and is within TOL of its fp64 restatement; as scene 0 of two it is within 2 * TOL of itself alone (the stage GEMMs see
    other row counts then: the bar of the Aether test, for its reason), and the list path equals the device-built pack's
    bytes.  Draws as in ``_many``: the first seed that leaves every Gumbel race of the fp64 restatement a margin of 1e-3."""
    from aether_amd.nn.dynamicvars.aether_dynamicvars import pack_scenes
    from test_gpu_dynamicvars import _scenes
    model, _, _ = _model("N9")
    rs = T.restatement(model, "N9", torch.float64)
    K, N, B, Tn = 3, 5, len(SMALLEST), len(SMALLEST[0])
    for seed in range(52, 92):
        s = _scenes(SMALLEST, N, seed, K)
        want, ok = [], True
        for b in range(B):
            u = [s["uniform"][t][b].double() for t in range(Tn - 1)]
            p, _, lg = rs.predict_future(s["inputs"][b], s["masks"][b], s["node_inds"][b], s["graph_info"][b], s["burn"][b], u,
                                         return_all=True)
            ok = ok and all(MG.min_margin(lg[t], u[t], MG.TAU) > MARGIN for t in range(Tn - 1) if lg[t].numel())
            want.append(p)
        if ok:
            break
    else:
        raise RuntimeError("no seed with unambiguous samples")
    assert [gi[0].numel() for gi in s["graph_info"][0]] == [2, 2, 0, 20, 6, 2] and s["graph_info"][0][0][2].shape == (2, 1)
    g = {k: _cu(v) for k, v in s.items()}
    one = (g["inputs"][:1], g["masks"][:1], [g["node_inds"][0]], [g["graph_info"][0]], g["burn"][:1])
    u0 = [g["uniform"][t][0] for t in range(Tn - 1)]
    got = model.predict_future(*one, uniform=u0)
    assert got.shape == (1, Tn - 1, N, 4) and float(got[0, 2].abs().max()) == 0.0
    model.one_call_step = False
    try:
        staged = model.predict_future(*one, uniform=u0)
    finally:
        model.one_call_step = True
    assert torch.equal(got, staged)
    err = scale_rel_err(got[0].cpu(), want[0])
    print(f"[dyn dnri smallest] seed {seed}, scene 0 alone vs its fp64 restatement: {err:.3g}")
    assert err <= TOL
    both = model.predict_future(g["inputs"], g["masks"], g["node_inds"], g["graph_info"], g["burn"], uniform=g["uniform"])
    err2 = scale_rel_err(both[:1].cpu(), got.cpu())
    print(f"[dyn dnri smallest] scene 0 of two vs alone: {err2:.3g}")
    assert both.shape == (B, Tn - 1, N, 4) and err2 <= 2 * TOL
    packed = model.predict_future_packed(g["inputs"], g["masks"], g["burn"], pack_scenes(g["inputs"], g["masks"]),
                                         uniform=g["uniform"])
    assert torch.equal(packed, both)


# -- the predicted update ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["N9", "N14"])
def test_predicted_update_against_fp64(tag):
    """The model returns inputs + update: the update of the one-step prediction (the staged decoder on the fixture's sample,
    present rows) is held to 4 x the error the fp32 CPU restatement of the same step has against fp64.  Measured on the
    MI355X: 0.40 (N9) and 0.54 (N14) floors; over 16 candidate seeds of the one-step state per case 0.00-2.15 on 31 pairs and
    5.9 on the one whose floor was 2.0e-8 -- the fixture tool takes a seed with a typical floor."""
    model, d, s, g = _scene(tag)
    x0, m0 = g["inputs"][:, 0], g["masks"][:, 0]
    pred, _ = model.decoder(x0, g["hidden0"], g["step_edges"], m0, g["graph_info"][0])
    present = s["masks"][0, 0] != 0
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        want32, _ = T.restatement(model, tag, torch.float32).decoder(s["inputs"][0, 0], s["hidden0"][0], s["step_edges"][0],
                                                                     s["masks"][0, 0], s["graph_info"][0])
    finally:
        torch.set_num_threads(n)
    want64, _ = T.restatement(model, tag, torch.float64).decoder(s["inputs"][0, 0], s["hidden0"][0], s["step_edges"][0],
                                                                 s["masks"][0, 0], s["graph_info"][0])
    check_update(f"dyn dnri {tag} step", pred[0].cpu()[present], want32[present], s["inputs"][0, 0][present], want64[present])


# -- the buffer contract ------------------------------------------------------------------------------------------------------------
def test_buffer_contract_and_workspace_sizes():
    """The one-call step and the rollout of three ragged scenes inside guarded, poisoned buffers: no guard byte changes, the
    results equal the plain run's bit for bit and the fp64 restatement's at 1e-5, an allocation of exactly the dNRI
    workspace size is found, and none of the Aether step's size for the same shapes."""
    from aether_amd import _lib
    from test_gpu_buffer_contract import Run, contract
    lib = _lib.load()
    m = _many()
    B, N, Tn = 3, m["N"], m["T"]
    pick = [3, 2, 5]                                        # 7-8, 3 / 0 and 20 present objects
    h = m["host"]
    inp = dict(inputs=h["inputs"][pick], masks=h["masks"][pick], burn=h["burn"][pick],
               node_inds=[h["node_inds"][b] for b in pick], graph_info=[h["graph_info"][b] for b in pick],
               uniform=[[h["uniform"][t][b] for b in pick] for t in range(Tn - 1)])
    want = m["want"][pick]
    sizes = {}

    def body(g):
        r = Run()
        model = T.build("N9", device="cuda")[0]
        out, pack = model._predict_future_rollout(g["inputs"], g["masks"], g["node_inds"], g["graph_info"], g["burn"], g["uniform"],
                                                  return_pack=True)
        r.result("rollout", out)
        r.against("rollout", want)
        r.allocated("rollout predictions", (Tn - 1, B, N, 4), torch.float32)
        a = (C.byref(pack["cfg"]), B, N, Tn - 1, pack["n_present"], pack["n_edges"], pack["in_degree"])
        sizes["dnri"] = lib.aether_dyn_dnri_rollout_batched_workspace_bytes(*a)
        sizes["aether"] = lib.aether_dyn_rollout_batched_workspace_bytes(*a)
        r.workspace("rollout workspace", sizes["dnri"])
        # the one-call step of scene 0 at frame 0 (7 present objects)
        model.__dict__["_step_ws"] = None
        gs, gr, e2n = g["graph_info"][0][0]
        one = g["inputs"][:1]
        ph, pc = model.encoder.get_initial_hidden(one)
        dec = model.decoder.get_initial_hidden(one)
        pred, h1, c1, d1, et = model._step_one_call(one[:, 0], g["masks"][:1, 0], g["node_inds"][0][0], gs, gr, e2n, ph, pc, dec,
                                                    g["uniform"][0][0], return_edge_types=True)
        r.result("step.pred", pred, output=True)
        r.result("step.edge_types", et, output=True)
        r.result("step.h", h1)
        r.result("step.dec", d1)
        r.against("step.pred", want[:1, 0])
        n0, e0 = int(g["node_inds"][0][0].numel()), int(gs.numel())
        s_arr = ((C.c_int64 * 1)(n0), (C.c_int64 * 1)(e0), (C.c_int * 1)(int(e2n.shape[1])))
        sizes["dnri_step"] = lib.aether_dyn_dnri_step_batched_workspace_bytes(C.byref(pack["cfg"]), 1, N, *s_arr)
        sizes["aether_step"] = lib.aether_dyn_step_batched_workspace_bytes(C.byref(pack["cfg"]), 1, N, *s_arr)
        r.workspace("step workspace", sizes["dnri_step"])
        return r

    guard, _ = contract(body, inp, "variable-N dNRI")
    assert 0 < sizes["dnri"] < sizes["aether"] and 0 < sizes["dnri_step"] < sizes["aether_step"]
    assert guard.find(nbytes=sizes["dnri"], dtype=torch.uint8) and guard.find(nbytes=sizes["dnri_step"], dtype=torch.uint8)
    assert not guard.find(nbytes=sizes["aether"], dtype=torch.uint8)
    assert not guard.find(nbytes=sizes["aether_step"], dtype=torch.uint8)


# -- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_queue_nothing_and_a_wrong_mask_poisons():
    from aether_amd import _lib
    lib = _lib.load()
    codes = T._codes()
    m = _many()
    model, g, B, N, Tn = m["model"], m["dev"], m["B"], m["N"], m["T"]
    good, pack = model._predict_future_rollout(g["inputs"], g["masks"], g["node_inds"], g["graph_info"], g["burn"], g["uniform"],
                                               return_pack=True)
    R, hd, slots, S = 64, 128, N * (N - 1), Tn - 1
    gen = torch.Generator().manual_seed(4)
    ph0, pc0 = torch.randn(B * slots, R, generator=gen).cuda(), torch.randn(B * slots, R, generator=gen).cuda()
    dec0 = torch.randn(B, N, hd, generator=gen).cuda()
    sentinel = torch.full((S, B, N, 4), 7.0, device="cuda")

    def refused(code, **kw):
        ph, pc, dec, preds = ph0.clone(), pc0.clone(), dec0.clone(), sentinel.clone()
        assert _raw_rollout(model, pack, ph, pc, dec, preds, **kw) == codes[code], kw
        assert torch.equal(ph, ph0) and torch.equal(pc, pc0) and torch.equal(dec, dec0) and torch.equal(preds, sentinel)
        return lib.aether_last_error().decode()

    arr = lambda src, typ: (typ * len(src))(*list(src))
    # the LAST step of scene 3 lists one edge too few: found on the host before the first step is queued
    e_bad = arr(pack["n_edges"], C.c_int64)
    e_bad[(S - 1) * B + 3] -= 1
    assert "n_present * min(knn_k, n_present - 1)" in refused("AETHER_EINVAL", n_edges=e_bad)
    n_bad = arr(pack["n_present"], C.c_int64)
    n_bad[(S - 1) * B + 1] = 1
    assert "one present object" in refused("AETHER_EINVAL", n_present=n_bad)
    assert "workspace too small" in refused("AETHER_ESPACE", ws_short=1)
    # the module raises the same refusals by name
    ni = [list(n) for n in g["node_inds"]]
    ni[1][0] = ni[1][0][:1]
    with pytest.raises(_lib.AetherHipError, match="one present object"):
        model.predict_future(g["inputs"], g["masks"], ni, g["graph_info"], g["burn"], uniform=g["uniform"])
    one = [g[k][3:4] for k in ("inputs", "masks", "burn")]
    nv = 7
    fc_s, fc_r = torch.where(~torch.eye(nv, dtype=torch.bool))
    wrong = list(g["graph_info"][3])
    wrong[1] = (fc_s[:nv * 5].cuda(), fc_r[:nv * 5].cuda(), torch.zeros(nv, 5, dtype=torch.int64).cuda())
    with pytest.raises(_lib.AetherHipError, match="kNN graph"):
        model.predict_future(one[0], one[1], [g["node_inds"][3]], [wrong], one[2])
    e2n_bad = g["graph_info"][3][1][2].clone()
    e2n_bad[2, 1] = g["graph_info"][3][1][0].numel() + 5
    wrong = list(g["graph_info"][3])
    wrong[1] = (wrong[1][0], wrong[1][1], e2n_bad)
    with pytest.raises(ValueError, match="edge2node"):
        model.predict_future(one[0], one[1], [g["node_inds"][3]], [wrong], one[2])
    # a mask that says more objects than n_present: the step's outputs are NaN and the next call reports it (async error word)
    # (a one-step loop: nothing behind the step consumes the word before the explicit check)
    masks_bad = g["masks"].clone()
    masks_bad[3, 0, :] = 1                                   # scene 3, step 0: 20 objects in the mask, 7 in n_present
    out = model.predict_future(g["inputs"][:, :2].contiguous(), masks_bad[:, :2].contiguous(), g["node_inds"], g["graph_info"],
                               g["burn"][:, :2].contiguous(), uniform=g["uniform"][:1])
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert lib.aether_check_async_error() == codes["AETHER_EHIP"]
    assert lib.aether_check_async_error() == 0
    again = model.predict_future(g["inputs"], g["masks"], g["node_inds"], g["graph_info"], g["burn"], uniform=g["uniform"])
    assert torch.equal(again, good)                          # and the path is as it was


# -- the inD metric on the model as it is -------------------------------------------------------------------------------------------
def test_eval_forward_prediction_dynamicvars_takes_the_model():
    """eval_forward_prediction_dynamicvars on a SceneDataset of 4 small synthetic scenes (un-padded sizes differ; batches of
    3 and 1) equals the metric computed in fp64 (tests/ind_eval_restatement.py) from the fp64 restatement's predictions on the
    same draws, at the bar the inD evaluation test holds AetherDynamicVars to (1e-5 of the largest reference entry).  The
    device seed is the first that leaves every Gumbel race of the restatement a margin of 1e-3."""
    from aether_amd.data import SceneDataset
    from aether_amd.evaluate import eval_forward_prediction_dynamicvars
    import ind_eval_restatement as R
    model, _, _ = _model("N9")
    rs = T.restatement(model, "N9", torch.float64)
    K = 3
    gen = torch.Generator().manual_seed(17)
    shapes = [(5, 6), (4, 4), (5, 7), (3, 5)]                 # (frames, objects)
    feats, masks = [], []
    for t_, n_ in shapes:
        feats.append(torch.randn(t_, n_, 4, generator=gen) * 0.5)
        mk = torch.ones(t_, n_)
        mk[1:, n_ - 1] = 0                                     # an object that leaves after frame 0
        mk[0, 0] = 0                                           # and one that appears at frame 1
        masks.append(mk)
    stats = (torch.tensor([-3.0, -2.0, -1.0, -1.5]), torch.tensor([3.0, 2.5, 1.0, 2.0]))
    ds = SceneDataset(feats, masks, max_burn_in_count=2, stats=stats)
    batches = list(ds.batches(3))
    for seed in range(20, 60):
        want_preds, ok = [], True
        torch.cuda.manual_seed(seed)
        for batch in batches:
            pack = batch["pack"]
            B_, S = int(batch["inputs"].shape[0]), int(batch["inputs"].shape[1]) - 1
            _, e, _ = pack.counts()
            draws = torch.rand(int(e[:S].sum()), K, device="cuda").cpu().double()
            parts = list(draws.split([int(v) for v in e[:S].reshape(-1)]))
            ni, gi = pack.as_lists()
            for b in range(B_):
                u = [parts[t * B_ + b] for t in range(S)]
                cpu = lambda v: v.cpu()
                p, _, lg = rs.predict_future(batch["inputs"][b].cpu(), batch["masks"][b].cpu(), [cpu(v) for v in ni[b]],
                                             [tuple(cpu(v) for v in gg) for gg in gi[b]], batch["burn_in_masks"][b].cpu(), u,
                                             return_all=True)
                ok = ok and all(MG.min_margin(lg[t], u[t], MG.TAU) > MARGIN for t in range(S) if lg[t].numel())
                want_preds.append(p)
        if ok:
            break
    else:
        raise RuntimeError("no device seed with unambiguous samples")
    torch.cuda.manual_seed(seed)
    got = eval_forward_prediction_dynamicvars(model, ds, {"strict": -1, "report_error_norm": False}, batch_size=3,
                                              return_bad_count=True)
    z = {"min_feats": stats[0].numpy(), "max_feats": stats[1].numpy()}
    scale, offset = R.stats_scale_offset(z)
    want = R.accumulate(torch.stack(want_preds).numpy(), ds.feats[:, 1:].cpu().numpy(), ds.masks.cpu().numpy(),
                        ds.burn_in_masks.cpu().numpy(), scale, offset, None, False)
    assert got[4] == want["bad"] and len(got[0]) == want["length"] > 0
    assert np.array_equal(got[3].numpy(), want["counts"][:want["length"]])
    for key, a, b in zip(("errors", "pos_errors", "vel_errors"), got[:3], R.finish(want)):
        ok, err = R.close(a.numpy(), b)
        print(f"[dyn dnri metric] {key}: max abs diff {err:.3e}, max|ref| {np.nanmax(np.abs(b)):.3e}")
        assert ok, (key, err)
