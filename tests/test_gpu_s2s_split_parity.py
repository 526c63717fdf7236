"""The split GEMMs of the fused seq2seq step (k_s2s_gemm_split, k_s2s_gemm_split_r1, csrc/s2s_step.h) at the sizes that reach
them, against fp64 at the bars of tests/update_parity.py.  From about 2 K rows on every dense layer of the step leaves the
fp32 job kernel for them; the update metric of tests/test_gpu_update_parity.py runs at 60 edge rows and never meets them, and
the tests that do run these sizes compare at scale_rel_err <= 1e-5 on position + update and let Gumbel samples flip.

Cases, draws and references: tests/update_s2s_cases.py (LARGE_CASES; the CPU half of their conditions, and the demonstration
that the bars below see a lost cross term, are in tests/test_update_metric.py).  Every case runs one fused step under
aether_set_option("gemm_split", 1 | 2 | 3): the library's own choice of structure, k_s2s_gemm_split_r1 forced, k_s2s_gemm_split
forced.  Per run:
  * aether_s2s_launch_stats says which kernel every table of the step took.  Each launch is held to the rule of
    s2s_launch_jobs restated here (split from 128 tiles of 64 x 128 on when every job has an image, 128-row tiles from 512
    workgroups of 128 x 128 on, the _r1 structure above 256 workgroups unless one is forced), and the case to what it is
    there for: the edge-level tables split and the node-level ones not (e2280, e2560), or every table with an image split
    (n4035) -- for the recurrent Aether table by table;
  * every sampled edge type is the fp64 loop's (the draws were fixed against that loop alone: no race closer than 1e-3);
  * the update is within FACTOR x the fp32 restatement's floor (check_update), and so are the tensors the update does not
    see -- decoder hidden state, prior h and c, and the logits where the step entry returns them (LoCS, dNRI) -- each at
    max|got - want64| / max|want64| against the same figure of the fp32 restatement, never taken below one rounding;
  * a second call returns the same bits, and the device reports no error.
The two 64-row cases of the recurrent Aether also run predict_future over one burn-in frame pair and two predicted steps, the
draws fixed step after step along the fp64 loop."""
import collections
import ctypes as C
import functools

import pytest
import torch

import update_s2s_cases as S2S
from update_parity import check_update

pytestmark = pytest.mark.gpu
STRUCTURES = (1, 2, 3)
FP32, GS1, GS2, R1_1, R1_2 = range(5)                   # kinds of include/aether_hip.h (AetherS2SLaunchStats)
RETURNS_LOGITS = ("locs", "dnri_rec", "dnri_mlp")      # models without a field: their step entry has a logits output


def _lib():
    from aether_amd import _lib as L
    return L, L.load()


@functools.lru_cache(maxsize=None)
def _model(case):
    return S2S.build(case, "cuda")


def _stats():
    L, lib = _lib()
    st = L.AetherS2SLaunchStats()
    L.check(lib.aether_s2s_launch_stats(C.byref(st)), "aether_s2s_launch_stats")
    assert st.logged <= L.S2S_LAUNCH_LOG, "the log is shorter than the run"
    return st, [st.log[i] for i in range(st.logged)]


def expected_kind(r, structure):
    """s2s_launch_jobs (csrc/host_s2s_step.inc) on a record of the launch log."""
    if not (r.images and r.M >= 128 and r.tiles64 >= 128):
        return FP32
    r1 = structure == 2 or (structure != 3 and r.wgs > 256)
    return (R1_1 if r1 else GS1) + (1 if r.wg128 >= 512 else 0)


def _signature(r, Nn, E):
    level = "edge" if r.N == E else "node" if r.N == Nn else f"rows{r.N}"
    return (level, r.jobs, r.M, r.K, r.K2)


def _aether_rec_tables(shape):
    """One step of the recurrent Aether with two edge types, three prior layers and the built-in field query, table by table
    (s2s_front_impl, s2s_step_impl): (level, jobs, M, K, K2) of the job the tiling is chosen for -> launches."""
    he, hd, R, ph = shape.he, shape.hd, shape.R, shape.ph
    edge = collections.Counter({("edge", 1, he, he, 0): 2,             # mlp4's edge third with the gathers, mlp4's second layer
                                ("edge", 1, 4 * R, he, R): 1,          # [W_ih | W_hh] . [x | h0], the LSTM cell in the epilogue
                                ("edge", 4, hd, hd, 0): 1,             # msg_fc2 and present_msg_fc1 of both types, through the lists
                                ("edge", 2, hd, hd, 0): 1})            # present_msg_fc2 of both types
    prior = collections.Counter({("edge", 1, ph, R, 0): 1, ("edge", 1, ph, ph, 0): 1})
    node = collections.Counter({("node", 5, he, he, 0): 1,             # field_net.0 + msg_fc1's receiver / sender halves
                                ("node", 1, he, he, 0): 3,             # field_net.2, mlp3's two layers
                                ("node", 2, he, he, 0): 1,             # mlp4's sender / receiver thirds
                                ("node", 4, hd, 32 + 2 * hd, 0): 1,    # the K-concatenated gates + hidden_h
                                ("node", 1, hd, hd, 0): 2})            # out_mlp.0, out_mlp.3
    return edge, prior, node


def check_launches(case, structure, steps=1):
    """The counters after `steps` steps of the case under gemm_split = structure."""
    L, _ = _lib()
    shape = S2S.shape_of(case)
    Nn, E = shape.B * shape.N, shape.B * shape.N * (shape.N - 1)
    st, log = _stats()
    names = L.S2S_LAUNCH_KINDS
    print(f"launches {S2S.case_id(case)} gemm_split={structure}: " + ", ".join(f"{names[k]} x {st.launches[k]}" for k in range(5))
          + f"; filter splits 1 x {st.filter_one}, > 1 x {st.filter_many} (max {st.filter_max_splits})")
    for k in range(1, 5):
        if st.launches[k]:
            print(f"    {names[k]}: jobs {st.jobs[k]}, largest N {st.max_n[k]} M {st.max_m[k]} K {st.max_k[k]} K2 {st.max_k2[k]}")
    assert sum(st.launches) == st.logged == len(log) and all(st.launches[k] == sum(r.kind == k for r in log) for k in range(5))
    for r in log:
        assert r.kind == expected_kind(r, structure), (_signature(r, Nn, E), names[r.kind], r.tiles64, r.wg128, r.wgs)
        if r.kind != FP32:
            rows = 128 if r.kind in (GS2, R1_2) else 64
            assert r.M % 128 == 0 and r.K % 32 == 0 and r.K2 % 32 == 0
            if r.jobs == 1:                # the figures the choice was made by, from the job itself
                assert r.tiles64 == -(-r.N // 64) * (r.M // 128) and r.wg128 == -(-r.N // 128) * (r.M // 128)
                assert r.wgs == -(-(-(-r.N // rows)) // 8) * 8 * (r.M // 128)
            if structure == 2:
                assert r.kind in (R1_1, R1_2)
            if structure == 3:
                assert r.kind in (GS1, GS2)
    split = [r for r in log if r.kind != FP32]
    rest = [r for r in log if r.kind == FP32]
    assert split, "no table took a split GEMM"
    node_case = case[4].startswith("n")
    if node_case:                          # every table with an image is split; what is left has none or is 2 wide
        assert all(not r.images or r.M < 128 for r in rest), [_signature(r, Nn, E) for r in rest]
        assert any(r.N == Nn for r in split) and any(r.N == E for r in split)
        assert any(r.kind in (GS2, R1_2) for r in split), "no table on 128-row tiles"
    else:                                  # the edge-level tables split, on 64-row tiles; the node-level ones not
        assert all(r.N == r.min_n == E for r in split), [_signature(r, Nn, E) for r in split]
        assert all(r.kind in (GS1, R1_1) for r in split)
        assert all(r.N != Nn or r.kind == FP32 for r in log)
    # the LSTM's table ([W_ih | W_hh]: the only one with a second K segment as wide as the prior state) with its cell update
    assert sum(r.K2 == shape.R and r.M == 4 * shape.R for r in split) == steps
    if case[0] == "aether_rec":
        edge, prior, node = _aether_rec_tables(shape)
        want = edge + prior + node if node_case else edge
        got = collections.Counter(_signature(r, Nn, E) for r in split)
        assert got == collections.Counter({k: v * steps for k, v in want.items()}), (got, want)
        left = collections.Counter({("node", 1, shape.he, r.K, 0): steps for r in rest if r.M == shape.he and not r.images})
        left[("edge", 1, 2, shape.ph, 0)] = steps                                   # res1 (no image), the last prior layer
        if not node_case:
            left += collections.Counter({k: v * steps for k, v in (prior + node).items()})
        assert collections.Counter(_signature(r, Nn, E) for r in rest) == left
    assert st.filter_one + st.filter_many == (0 if case[0].startswith("dnri") else steps)      # (dNRI has no edge filter)
    return st


def _step(case, m, inp):
    kind, shape = case[0], S2S.shape_of(case)
    cu = lambda t: None if t is None else t.cuda()
    if kind == "charges":
        m._set_charges(((inp["charges"] + 1) / 2).long(), shape.B, shape.N, "cuda")
    if kind == "dynfield":
        m._set_summary(inp["summary"].cuda())
    kw = dict(return_logits=True) if kind in RETURNS_LOGITS else {}
    res = m._fused_step(cu(inp["x"]), cu(inp["hidden"]), tuple(cu(t) for t in inp["state"]), cu(inp["u"]), **kw)
    out, hidden, (h, c), edges = res[:4]
    return dict(out=out, hidden=hidden, h=h, c=c, edges=edges, logits=res[4] if kw else None)


@pytest.fixture(params=STRUCTURES, ids=lambda s: f"gemm_split{s}")
def structure(request):
    _, lib = _lib()
    lib.aether_set_option(b"gemm_split", request.param)
    try:
        yield request.param
    finally:
        lib.aether_set_option(b"gemm_split", 1)
        lib.aether_s2s_launch_stats_reset()


@pytest.mark.parametrize("case", S2S.LARGE_CASES, ids=S2S.case_id)
def test_one_step_on_the_split_gemms(case, structure):
    _, lib = _lib()
    ref = S2S.references(case, 1)
    m, inp = _model(case), ref["inp"]
    _step(case, m, inp)                                     # (the plan and the workspace are made here)
    torch.cuda.synchronize()
    lib.aether_s2s_launch_stats_reset()
    got = _step(case, m, inp)
    torch.cuda.synchronize()
    check_launches(case, structure)
    again = _step(case, m, inp)
    torch.cuda.synchronize()
    what = f"{S2S.case_id(case)} gemm_split={structure}"
    bars = S2S.step_bars(what, ref, got["out"].cpu(), got["edges"].argmax(-1).cpu(), got)
    assert (got["hidden"] is None) == (case[0] in S2S.STATELESS) and (got["logits"] is None) == (case[0] not in RETURNS_LOGITS)
    assert bars["types"][2], "an edge type drawn differently at a score gap of at least 1e-3"
    check_update(what, got["out"].cpu(), ref["want32"][0], ref["prev"][0], ref["want64"][0])
    missed = {k: v for k, v in bars.items() if not v[2]}
    assert not missed, missed
    assert set(bars) == {"update", "types", "h", "c"} | ({"hidden"} - ({"hidden"} if got["hidden"] is None else set())) \
        | ({"logits"} if got["logits"] is not None else set())
    for name, t in got.items():
        assert t is None or torch.equal(t, again[name]), f"{name}: a second call returned other bits"
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", S2S.ROLLOUT_CASES, ids=S2S.case_id)
def test_predict_future_on_the_split_gemms(case, structure):
    _, lib = _lib()
    steps = S2S.shape_of(case).steps
    ref = S2S.references(case, steps)
    m, inp = _model(case), ref["inp"]
    frames, U = inp["frames"].cuda(), inp["U"].cuda()
    m.predict_future(frames, steps, return_edges=True, uniform=U)
    torch.cuda.synchronize()
    lib.aether_s2s_launch_stats_reset()
    preds, edges = m.predict_future(frames, steps, return_edges=True, uniform=U)
    torch.cuda.synchronize()
    check_launches(case, structure, S2S.FRAMES - 1 + steps)
    got, types = preds.transpose(0, 1).cpu(), edges.argmax(-1).transpose(0, 1).cpu()
    assert got.shape == ref["want64"].shape
    assert torch.equal(types, ref["types64"]), "an edge type drawn differently at a score gap of at least 1e-3"
    for t in range(steps):
        check_update(f"{S2S.case_id(case)} gemm_split={structure} predict_future {t}", got[t], ref["want32"][t], ref["prev"][t],
                     ref["want64"][t])
    p2, e2 = m.predict_future(frames, steps, return_edges=True, uniform=U)
    assert torch.equal(p2, preds) and torch.equal(e2, edges), "a second call returned other bits"
    torch.cuda.synchronize()


def test_the_cases_reach_every_split_kernel_and_both_filter_forms():
    """k_s2s_gemm_split<1> and <2>, k_s2s_gemm_split_r1<1> and <2>, k_s2s_filter_split with splits == 1 and > 1: each is taken
    by a step of a case of the table above.  (128-row tiles mean at least 512 workgroups, above the 256 from which the
    library itself takes the _r1 structure: k_s2s_gemm_split<2> runs only where that structure is forced.)"""
    _, lib = _lib()
    reached, filters = collections.Counter(), collections.Counter()
    by_tag = {c[4]: c for c in S2S.LARGE_CASES if c[0] == "aether_rec"}
    try:
        for tag, structure in (("e2280", 1), ("n4035", 1), ("n4035", 3)):
            case = by_tag[tag]
            inp = S2S.references(case, 1)["inp"]
            lib.aether_set_option(b"gemm_split", structure)
            lib.aether_s2s_launch_stats_reset()
            _step(case, _model(case), inp)
            torch.cuda.synchronize()
            st, _ = _stats()
            for k in range(5):
                reached[(k, structure)] += st.launches[k]
            filters["one"] += st.filter_one
            filters["many"] += st.filter_many
    finally:
        lib.aether_set_option(b"gemm_split", 1)
        lib.aether_s2s_launch_stats_reset()
    print("reached:", dict(reached), dict(filters))
    assert reached[(GS1, 1)] and reached[(R1_1, 1)] and reached[(R1_2, 1)] and reached[(GS2, 3)] and reached[(GS1, 3)]
    assert reached[(GS2, 1)] == 0
    assert filters["one"] and filters["many"]
