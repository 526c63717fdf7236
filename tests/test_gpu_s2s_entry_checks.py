"""The argument checks of the four fused seq2seq entries -- aether_s2s_step, aether_s2s_rollout, aether_s2s_markov_step,
aether_s2s_markov_rollout -- which share one check (s2s_entry_check): called through the C ABI with real, correctly sized
device buffers and a plan built by the model.  Each failing case has exactly one defect, and one that would do no harm if the
check were lost: a workspace size understated by one byte (the buffer itself is full size), tau = 0, a rollout of no steps.
The entries take rnn_hidden from 16 on, the model's constructor from 32 on: the model is built at 32 and the layers that have
that width are replaced by ones of width 16 before it builds its plan (_narrow_rnn)."""
import ctypes as C
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

D, N, B, K, HE, HD, R = 2, 3, 1, 2, 128, 32, 16
R_MODEL, PRIOR_HIDDEN = 32, 32        # R_MODEL: the smallest encoder_rnn_hidden Encoder.__init__ takes
E = N * (N - 1)
T0, STEPS = 1, 2
SCALARS = ("num_dims", "encoder_hidden", "decoder_hidden", "rnn_hidden", "prior_layers", "prior_hidden", "num_edge_types",
           "skip_first", "polar", "num_vars", "tau", "n_nodes", "n_edges")     # the scalar arguments of all four entries, in order
TAU = SCALARS.index("tau")
ENTRIES = ["aether_s2s_step", "aether_s2s_rollout", "aether_s2s_markov_step", "aether_s2s_markov_rollout"]


def _codes():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aether_hip.h")
    return {k: int(v) for k, v in re.findall(r"#define (AETHER_E\w+) \((-\d+)\)", open(header).read())}


def _narrow_rnn(m):
    """The encoder of m with rnn width R: the layers of that width made anew, as Encoder.__init__ makes them."""
    from aether_amd.nn.seq2seq.encoder import _mlp_out
    enc = m.encoder
    enc.rnn_hidden_size = R
    enc.forward_rnn = torch.nn.LSTM(HE, R, batch_first=True)
    enc.reverse_rnn = torch.nn.LSTM(HE, R, batch_first=True)
    enc.encoder_fc_out = _mlp_out(2 * R, 32, K, 1)
    enc.prior_fc_out = _mlp_out(R, PRIOR_HIDDEN, K, 2)
    return m.to("cuda").eval()


def _entries(lib, markov):
    """(step call, rollout call, scalar arguments, workspace bytes, tensors to keep alive) of one decoder; a call is
    call(scalars=None, workspace_bytes=None[, burn_in_steps=T0, steps=STEPS]) -> status, the defaults the defect-free call."""
    from aether_amd.nn.seq2seq.aether import Aether
    params = {"num_vars": N, "input_size": 2 * D, "gpu": True, "decoder_hidden": HD, "num_edge_types": K,
              "skip_first": False, "decoder_dropout": 0.0, "use_3d": False, "encoder_dropout": 0.0, "encoder_hidden": HE,
              "encoder_rnn_hidden": R_MODEL, "encoder_rnn_type": "lstm", "encoder_mlp_num_layers": 1, "encoder_mlp_hidden": 32,
              "prior_num_layers": 2, "prior_hidden_size": PRIOR_HIDDEN, "pos_representation": "polar", "gumbel_temp": 0.5,
              "rff_std": 1.0}
    if markov:
        params["decoder_type"] = "ref_mlp"
    torch.manual_seed(5)
    m = _narrow_rnn(Aether(params, device="cuda"))
    assert m._step_sizes() == (D, HE, HD, R, K)
    plan = m._plan("cuda:0")
    pe, n_layers, prior_hidden = m.encoder._param_struct(with_image=False)
    pd, pf = m.decoder._param_struct(), m._field_struct()
    scal = (D, HE, HD, R, n_layers, prior_hidden, K, 0, 1, N, 0.5, B * N, B * E)
    assert len(scal) == len(SCALARS)
    need = lib.aether_s2s_step_workspace_bytes(D, HE, HD, R, prior_hidden, K, B * N, B * E)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    graph = [t.data_ptr() for t in m.encoder._graph(B, N, "cuda:0")]
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device="cuda")
    x, burn, dh, h, c = z(B, N, 2 * D), z(T0, B, N, 2 * D), z(B, N, HD), z(B, E, R), z(B, E, R)
    u = torch.full((T0 + STEPS, B, E, K), 0.5, dtype=torch.float32, device="cuda")
    x1, dh1, h1, c1, e1 = z(B, N, 2 * D), z(B, N, HD), z(B, E, R), z(B, E, R), z(B, E, K)
    preds, edges = z(STEPS, B, N, 2 * D), z(STEPS, B, E, K)
    p = lambda t: t.data_ptr()
    head = (C.byref(pf), C.byref(pe), C.byref(pd), p(plan))
    dh_in, dh_out = ((), ()) if markov else ((p(dh),), (p(dh1),))            # the Markov entries take no decoder state
    step_fn, rollout_fn = getattr(lib, ENTRIES[2 * markov]), getattr(lib, ENTRIES[2 * markov + 1])

    def step(scalars=None, workspace_bytes=None):
        st = step_fn(*head, *(scalars or scal), *graph, p(x), None, *dh_in, p(h), p(c), p(u), p(ws),
                     need if workspace_bytes is None else workspace_bytes, p(x1), *dh_out, p(h1), p(c1), p(e1), None)
        torch.cuda.synchronize()
        return st

    def rollout(scalars=None, workspace_bytes=None, burn_in_steps=T0, steps=STEPS):
        st = rollout_fn(*head, *(scalars or scal), *graph, burn_in_steps, p(burn), steps, p(x), *dh_in, p(h), p(c), p(u), p(ws),
                        need if workspace_bytes is None else workspace_bytes, p(preds), p(edges), None)
        torch.cuda.synchronize()
        return st

    return step, rollout, scal, need, (m, plan, pe, pd, pf, ws, x, burn, dh, h, c, u, x1, dh1, h1, c1, e1, preds, edges)


@pytest.fixture(scope="module")
def calls():
    from aether_amd import _lib
    lib = _lib.load()
    out = {}
    for markov in (False, True):
        step, rollout, scal, need, keep = _entries(lib, markov)
        out[ENTRIES[2 * markov]], out[ENTRIES[2 * markov + 1]] = step, rollout
        out[("scal", markov)], out[("need", markov)], out[("keep", markov)] = scal, need, keep
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_defect_free_call_succeeds(calls, entry):
    assert calls[entry]() == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_workspace_one_byte_short_is_out_of_space(calls, entry):
    need = calls[("need", "markov" in entry)]
    assert calls[entry](workspace_bytes=need - 1) == _codes()["AETHER_ESPACE"]
    assert calls[entry](workspace_bytes=need) == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_tau_zero_is_an_invalid_argument(calls, entry):
    scal = list(calls[("scal", "markov" in entry)])
    scal[TAU] = 0.0
    assert calls[entry](scalars=tuple(scal)) == _codes()["AETHER_EINVAL"]


@pytest.mark.parametrize("entry", [e for e in ENTRIES if e.endswith("rollout")])
def test_a_rollout_of_no_steps_is_an_invalid_argument(calls, entry):
    assert calls[entry](burn_in_steps=0, steps=0) == _codes()["AETHER_EINVAL"]
