"""The update metric of tests/update_parity.py sees a split GEMM lose one of its three terms; the position metric of the
forward parity tests does not.  CPU only: the kernels are not run, their arithmetic is restated inside the fp64 oracle.

csrc/common.h (gemm_split): every operand of a `gnn.*` Linear is two fp16 pieces, x = hi + lo with hi = fp16(x) and
lo = fp16(x - hi); the product is w_hi x_hi + w_hi x_lo + w_lo x_hi accumulated in fp32.  `split_linears` puts that
into the oracle (everything else stays fp64) and can leave one cross term out of one layer -- the slip a hand-scheduled
GEMM makes with a swapped fragment or a term lost in a re-ordering -- or keep only the hi piece of every weight.

Per case: (a) the full three-term arithmetic passes FACTOR x the fp32 restatement's floor, (b) every degraded variant
fails it, (c) every degraded variant passes scale_rel_err <= 1e-5, which is why test_gpu_update_parity.py exists.
(b) is a condition on the inputs (seeds below), not on any kernel.

The second half holds the inputs of tests/test_gpu_update_parity.py and tests/test_gpu_fused_irregular.py to the rule
their seeds were chosen by, on this machine's CPU: a floor that is not a lucky draw, a bar the design's arithmetic meets,
Gumbel samples away from a tie; the graphs of tests/irregular_graphs.py to the structure they are there for, and the
update bar to its teeth on one of them."""
import pytest
import torch

from conftest import scale_rel_err
import irregular_graphs as IG
import update_cases as U
import update_s2s_cases as S2S
from update_cases import split_linears
from update_parity import DEGENERATE, FACTOR, update_err, update_floor
from aether_amd.nn.state2state.aether import Aether
from aether_amd.synthetic import make_batch
from oracle import aether_oracle as O

OLD_TOL = 1e-5
LAYERS = ["gnn.layer_2.message_fn.0", "gnn.layer_3.update_fn.0", "gnn.out_mlp.3"]
TERMS = ["w_lo*x_hi", "w_hi*x_lo"]
# D, H, B, N, input seed (tests/update_cases.py says how a seed is chosen: B2N5 has 30 elements, and at seeds 5 .. 11 its
# floor is degenerate or the full arithmetic does not meet the bar)
CASES = [(2, 64, 16, 20, 5), (3, 64, 6, 7, 5), (2, 128, 4, 20, 5), (2, 32, 6, 7, 5), (3, 64, 2, 5, 12)]


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "D%d_H%d_B%dN%d_s%d" % c)
def case(request):
    D, H, B, N, seed = request.param
    torch.manual_seed(11)
    m = Aether(2 * D, H, 0.0, D, device="cpu")
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    sd64 = {k: v.double() for k, v in sd.items()}
    inp = make_batch(B, N, D, seed=seed)
    args64 = (inp["x"].double(), inp["vel"].double(), inp["edges"], inp["edge_attr"].double(), inp["charges"].double())
    with torch.no_grad(), U.one_thread():
        want = O.aether_forward(sd64, *args64)
        want32 = O.aether_forward(sd, inp["x"], inp["vel"], inp["edges"], inp["edge_attr"], inp["charges"])
    floor = update_floor(want32, inp["x"], want)

    def run(**kw):
        """out as the kernel forms it: fl32(x + update32)."""
        with torch.no_grad(), U.one_thread(), split_linears(**kw):
            out = O.aether_forward(sd64, *args64)
        return (inp["x"] + (out - inp["x"].double()).float())

    return dict(x=inp["x"], want=want, floor=floor, run=run)


def test_floor_is_not_degenerate(case):
    assert case["floor"] >= DEGENERATE, case["floor"]
    assert case["floor"] <= 1e-6, case["floor"]


def test_full_three_term_arithmetic_passes(case):
    err = update_err(case["run"](), case["x"], case["want"])
    print(f"all terms: new={err:.2e} floor={case['floor']:.2e}")
    assert err <= FACTOR * case["floor"], (err, case["floor"])


@pytest.mark.parametrize("term", TERMS)
@pytest.mark.parametrize("layer", LAYERS)
def test_one_dropped_term_fails_the_update_bar_and_passes_the_position_bar(case, layer, term):
    got = case["run"](drop=(layer, term))
    new, old = update_err(got, case["x"], case["want"]), scale_rel_err(got, case["want"])
    print(f"{layer} without {term}: old={old:.2e} new={new:.2e} floor={case['floor']:.2e} new/floor={new / case['floor']:.1f}")
    assert new > FACTOR * case["floor"], (new, case["floor"])
    assert old <= OLD_TOL, old


def test_hi_only_weights_fail_the_update_bar_and_pass_the_position_bar(case):
    got = case["run"](hi_only_weights=True)
    new, old = update_err(got, case["x"], case["want"]), scale_rel_err(got, case["want"])
    print(f"hi-only weights: old={old:.2e} new={new:.2e} floor={case['floor']:.2e} new/floor={new / case['floor']:.1f}")
    assert new > FACTOR * case["floor"], (new, case["floor"])
    assert old <= OLD_TOL, old


# ---- the cases of tests/test_gpu_update_parity.py, without a GPU -----------------------------------------------------------
@pytest.mark.parametrize("fc", U.FORWARD_CASES + U.IRREGULAR_CASES, ids=U.case_id)
def test_gpu_forward_case_has_a_typical_floor_and_a_bar_the_design_meets(fc):
    name, case = fc
    x, want64, want32 = U.references(name, case)
    floor = update_floor(want32, x, want64)
    print(f"{U.case_id(fc)}: floor={floor:.2e}")
    assert floor >= U.TYPICAL, floor
    if name in U.SPLIT_FAMILIES:
        err = update_err(U.emulated(name, case), x, want64)
        print(f"{U.case_id(fc)}: three-term split arithmetic err={err:.2e} ratio={err / floor:.2f}")
        assert err <= FACTOR * floor, (err, floor)


@pytest.mark.parametrize("fc", U.ROLLOUT_CASES + U.IRREGULAR_ROLLOUT_CASES, ids=U.case_id)
def test_gpu_rollout_case_has_a_typical_floor_at_every_step(fc):
    name, case = fc
    x, want64, want32 = U.references(name, case, U.ROLLOUT_STEPS)
    prev = torch.cat([x.double()[None], want64[:-1]])
    floors = [update_floor(want32[t], prev[t], want64[t]) for t in range(U.ROLLOUT_STEPS)]
    print(f"{U.case_id(fc)}: floors " + " ".join(f"{f:.2e}" for f in floors))
    assert torch.isfinite(want64).all() and min(floors) >= U.TYPICAL, floors


# ---- the graphs of tests/irregular_graphs.py (tests/test_gpu_fused_irregular.py) ----------------------------------------------
@pytest.mark.parametrize("D", [2, 3])
@pytest.mark.parametrize("name", list(IG.GRAPHS))
def test_irregular_graphs_have_their_structure(name, D):
    """From the edge list alone, at the seed the case runs under."""
    want = IG.structure(name)
    inp = IG.build(name, D, U.IRREGULAR_SEEDS[(name, D)])
    send, recv = inp["edges"]
    n = inp["x"].shape[0]
    assert inp["x"].shape == (n, D) and send.dtype == recv.dtype == torch.int64
    assert (n, send.numel(), recv.numel()) == (want["nodes"], want["edges"], want["edges"])
    assert inp["edge_attr"].shape == (want["edges"], 2)
    assert int(send.min()) >= 0 and int(recv.min()) >= 0 and int(send.max()) < n and int(recv.max()) < n
    indeg = torch.bincount(recv, minlength=n)
    assert int(indeg.max()) == want["max_in"] and want["max_in"] >= want["max_in_above"] + 1, int(indeg.max())
    assert int((indeg == 0).sum()) == want["no_in"]
    assert not bool((send == recv).any())
    pairs = send * n + recv
    assert (pairs.unique().numel() < pairs.numel()) == want["duplicates"]
    assert IG.components(send, recv, n) == want["components"]
    if want["duplicates"]:                          # the multigraphs: the last two nodes have no edge at all
        assert int(torch.bincount(send, minlength=n)[-2:].sum()) == 0 and int(indeg[-3:].sum()) == 0
        assert int(indeg[0]) == want["max_in"]
    else:                                           # the kNN scenes: every node receives min(k, n - 1) edges, in its scene
        sizes = torch.tensor(want["components"])
        assert torch.equal(indeg, torch.minimum(sizes - 1, torch.tensor(want["max_in"])).repeat_interleave(sizes))
    # not in receiver order: `perm` of the graph view is no identity
    assert not torch.equal(recv, recv.sort().values)


def test_one_dropped_term_on_an_irregular_graph_fails_the_update_bar_and_passes_the_position_bar():
    """multi32_hub40 at D 3: `gnn.layer_2.message_fn.0` without one cross term, the rest of the three-term arithmetic."""
    case = U.IRREGULAR_TEETH_CASE
    family = U.FAMILIES["Aether-irregular"]
    x, want64, want32 = U.references("Aether-irregular", case)
    floor = update_floor(want32, x, want64)
    sd = {k: U._cast(v, torch.float64) for k, v in U.state_of(family.build(case, "cpu")).items()}
    inp = U._in_dtype(family.inputs(case), torch.float64)
    for term in TERMS:
        with torch.no_grad(), U.one_thread(), split_linears(drop=("gnn.layer_2.message_fn.0", term)):
            out = family.restate(sd, inp, case)
        got = x + (out - x.double()).float()
        new, old = update_err(got, x, want64), scale_rel_err(got, want64)
        print(f"{U.case_id(('Aether-irregular', case))} without {term}: old={old:.2e} new={new:.2e} new/floor={new / floor:.1f}")
        assert new > FACTOR * floor, (term, new, floor)
        assert old <= OLD_TOL, (term, old)


@pytest.mark.parametrize("steps", [1, S2S.STEPS])
@pytest.mark.parametrize("case", S2S.CASES, ids=S2S.case_id)
def test_gpu_seq2seq_case_has_a_typical_floor_and_no_sample_near_a_tie(case, steps):
    ref = S2S.references(case, steps)
    floors = [update_floor(ref["want32"][t], ref["prev"][t], ref["want64"][t]) for t in range(steps)]
    print(f"{S2S.case_id(case)} steps={steps}: gap={ref['gap']:.1e} floors " + " ".join(f"{f:.2e}" for f in floors))
    assert min(floors) >= S2S.TYPICAL, floors
    assert ref["gap"] >= S2S.GAP, ref["gap"]
    assert torch.equal(ref["types64"], ref["types32"])


# ---- the large cases of tests/test_gpu_s2s_split_parity.py, without a GPU ---------------------------------------------------
def _large(case):
    return [(case, 1)] + ([(case, S2S.shape_of(case).steps)] if case in S2S.ROLLOUT_CASES else [])


@pytest.mark.parametrize("case,steps", [cs for c in S2S.LARGE_CASES for cs in _large(c)],
                         ids=lambda v: S2S.case_id(v) if isinstance(v, tuple) else f"steps{v}")
def test_gpu_split_case_has_fixed_draws_equal_types_and_a_floor(case, steps):
    """The draws are fixed against the fp64 loop alone (update_s2s_cases.redrawing): afterwards no race is closer than GAP,
    at most 1 % of a step's edges were redrawn, the fp32 loop draws the same types, and every floor carries information."""
    ref = S2S.references(case, steps)
    floors = [update_floor(ref["want32"][t], ref["prev"][t], ref["want64"][t]) for t in range(steps)]
    print(f"{S2S.case_id(case)} steps={steps}: gap={ref['gap']:.1e} redrawn={ref['redrawn']:.1e} floors "
          + " ".join(f"{f:.2e}" for f in floors))
    assert ref["gap"] >= S2S.GAP, ref["gap"]
    assert ref["redrawn"] <= S2S.MAX_REDRAWN, ref["redrawn"]
    assert torch.equal(ref["types64"], ref["types32"])
    assert min(floors) >= DEGENERATE, floors
    if steps == 1:
        for name in S2S.HELD:
            want = ref["held64"][name]
            assert (want is None) == (name == "hidden" and case[0] in S2S.STATELESS)
            if want is not None:
                fig = S2S.held_figure(ref["held32"][name], want)
                print(f"    {name}: fp32 restatement {fig:.2e}")
                assert torch.isfinite(want).all() and fig < 1e-4, (name, fig)


def test_steered_rows_cross_the_row_scale_rule():
    """The K profiles of update_s2s_cases.steer_rows against the rule of the split GEMMs' running row scale (csrc/s2s_step.h,
    x_settle), from the inputs alone: rows that start at zero take the clamped 2^40 and lower it at the first non-zero
    block; rows whose later blocks are larger lower their scale there (the growing profile at every block); the shrinking
    profile never does; the prior LSTM state has all-zero rows and rows at 1e-3, 0.3 and 0.99."""
    case = next(c for c in S2S.LARGE_CASES if S2S.shape_of(c).profile)
    m = S2S.build(case)
    inp = S2S.inputs(case, m)
    H = inp["hidden"].view(-1, inp["hidden"].shape[-1])
    blocks = H.shape[1] // 32
    assert blocks == 8
    walk = {name: [S2S.row_scale_walk(H[i]) for i in idx] for name, idx in inp["rows"].items() if name in S2S.PROFILES}
    for first, lowered in walk["zero_first"]:
        assert first == 2.0 ** 40 and lowered >= 1
    for i in inp["rows"]["zero_first"]:
        assert float(H[i, :32].abs().max()) == 0.0 and float(H[i, 32:64].abs().max()) * 2.0 ** 40 >= 2.0 ** 15
    for (first, lowered), i in zip(walk["tiny_first"], inp["rows"]["tiny_first"]):
        assert lowered >= 1 and float(H[i, 32:64].abs().max()) * first >= 2.0 ** 15
    for (first, lowered), i in zip(walk["growing"], inp["rows"]["growing"]):
        assert lowered == blocks - 1 and float(H[i, 32:64].abs().max()) * first >= 2.0 ** 15, lowered
    assert all(lowered == 0 for _, lowered in walk["shrinking"])
    assert all(first == 2.0 ** 40 and lowered == 0 for first, lowered in walk["all_zero"])
    for t in inp["state"]:
        T = t.view(-1, t.shape[-1])
        for level in S2S.STATE_LEVELS:
            got = T[inp["rows"][level]].abs().amax(1)
            assert bool((got <= level).all()) and (level == 0.0 or bool((got >= 0.9 * level).all())), (level, got)


SPLIT_LAYERS = ["encoder.mlp4.model.3", "encoder.forward_rnn.weight_ih_l0", "decoder.msg_fc2.0", "decoder.present_msg_fc2.1"]


@pytest.mark.parametrize("layer", SPLIT_LAYERS)
def test_a_dropped_term_of_a_split_layer_misses_a_bar_of_the_split_parity_test(layer):
    """aether_rec at 2,280 edge rows: one edge-level layer of the fp32 restatement in the three-term fp16 arithmetic of the
    split GEMMs (update_s2s_cases.split_layer).  In full it passes every bar tests/test_gpu_s2s_split_parity.py holds a step
    to; without w_hi x_lo it misses at least one of them, and still passes scale_rel_err <= 1e-5 on the state.  The encoder's
    layers reach the state only through the sample: it is the held prior state and logits that see them."""
    case = next(c for c in S2S.LARGE_CASES if c[0] == "aether_rec" and c[4] == "e2280")
    ref = S2S.references(case, 1)
    inp = ref["inp"]
    rs = S2S.Restatement(case, S2S.state_of(S2S.build(case)), torch.float32)
    name = layer if layer.endswith("_l0") else layer + ".weight"
    weight = rs.sd[name]
    assert weight.shape[1] in (256, 512) and weight.shape[0] % 128 == 0
    seen = {}
    for drop in (None, "w_hi*x_lo"):
        with torch.no_grad(), U.one_thread(), S2S.split_layer([weight], drop):
            out, hidden, (h, c), z, logits = rs.step(inp["x"], inp["hidden"], inp["state"], inp["u"], rs.context(inp))
        bars = S2S.step_bars(f"{layer} without {drop}", ref, out, z.argmax(-1), dict(hidden=hidden, h=h, c=c, logits=logits))
        seen[drop] = (bars, scale_rel_err(out, ref["want64"][0]))
    full, dropped = seen[None], seen["w_hi*x_lo"]
    assert all(ok for _, _, ok in full[0].values()), full[0]
    missed = [k for k, (_, _, ok) in dropped[0].items() if not ok]
    print(f"{layer}: the dropped term misses {missed}; old bar {dropped[1]:.2e}")
    assert missed, dropped[0]
    assert dropped[1] <= OLD_TOL, dropped[1]
