"""Device rollout of EGNN-Aether and ClofNet (``aether_egnn_rollout`` / ``aether_clof_rollout``), host side: the four
entries are declared, exported and bound, their workspace is the inference workspace plus the rollout's state, and
``.rollout`` refuses what it cannot serve before anything reaches the GPU.  The kernels: tests/test_gpu_gnn_rollout.py."""
import os
import re

import pytest
import torch

from aether_amd import _lib

from conftest import REPO
from egnn_restatement import runner_batch
from gnn_shape_checks import Clof, Egnn

ENTRIES = ("aether_egnn_rollout", "aether_egnn_rollout_workspace_bytes", "aether_clof_rollout",
           "aether_clof_rollout_workspace_bytes")
MODELS = [(Egnn, "egnn_aether"), (Clof, "clof"), (Clof, "clof_vel"), (Clof, "clof_vel_gbf")]


def _model(K, model, in_nf=1):
    return K.build(K.cfg(model, 64, 1, 3, 5, in_nf=in_nf))


def _state(B=2, N=5):
    inp = runner_batch(B, N, 4)
    return inp["x"], inp["vel"], inp["edges"], inp["charges"]


def test_entries_are_declared_exported_and_bound():
    hdr = open(os.path.join(REPO, "include", "aether_hip.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    # send / recv sit between the charges and the graph view; steps and dt between the trajectory and the stream
    for name, lead in (("aether_egnn_rollout", 8), ("aether_clof_rollout", 11)):
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == lead + 13, name
        assert args[-3] is _lib.C.c_int and args[-2] is _lib.C.c_float, name


def test_rollout_workspace_is_the_inference_workspace_plus_the_state():
    lib = _lib.load()
    n, E = 2560, 48640
    state = n * 3 * 4 + n * 4 + E * 2 * 4                       # vel, h, edge_attr
    fwd = lib.aether_egnn_workspace_bytes(64, 4, 1, n, E, 0)
    roll = lib.aether_egnn_rollout_workspace_bytes(64, 4, 1, n, E)
    assert fwd + state <= roll <= fwd + state + 4 * 256
    assert lib.aether_egnn_rollout_workspace_bytes(96, 4, 1, n, E) == 0
    assert lib.aether_egnn_rollout_workspace_bytes(64, 4, 1, 0, E) == 0
    for v in range(3):
        fwd = lib.aether_clof_workspace_bytes(v, 128, 4, 1, n, E, 0)
        roll = lib.aether_clof_rollout_workspace_bytes(v, 128, 4, 1, n, E)
        assert fwd + state <= roll <= fwd + state + 4 * 256, v
    assert lib.aether_clof_rollout_workspace_bytes(3, 64, 4, 1, n, E) == 0
    assert lib.aether_clof_rollout_workspace_bytes(0, 64, 4, 1, n, 0) > 0      # no edge: still a valid call


def _entry_call(family, in_nf, flags, steps, ws_bytes=None):
    """The entry with placeholder addresses: every rejection below is decided on the host, before anything is
    dereferenced or launched (the parameter list is a host array, the graph info a host struct)."""
    lib, C = _lib.load(), _lib.C
    n, E, L, fake = 10, 90, 1, 0x1000
    info = _lib.AetherGraphInfo()
    info.n_nodes, info.n_edges = n, E
    if family == "egnn":
        n_params, lead = 2 + 15 * L + 7, (64, L, in_nf, flags)
        need = lib.aether_egnn_rollout_workspace_bytes(64, L, 1, n, E)
    else:
        n_params, lead = 6 + 19 * L, (1, 64, L, in_nf, flags, 1.0, 5)
        need = lib.aether_clof_rollout_workspace_bytes(1, 64, L, 1, n, E)
    params = (C.c_void_p * n_params)(*([fake] * n_params))
    st = getattr(lib, f"aether_{family}_rollout")(params, n_params, *lead, n, E, fake, fake, fake, fake, fake, fake,
                                                  C.byref(info), fake, need if ws_bytes is None else ws_bytes, fake, steps,
                                                  1.0, None)
    return st, lib.aether_last_error().decode()


@pytest.mark.parametrize("family,keep", [("egnn", _lib.EGNN_KEEP), ("clof", _lib.CLOF_KEEP)])
def test_entry_rejections_and_zero_steps(family, keep):
    st, msg = _entry_call(family, 2, 0, 3)
    assert st < 0 and f"{family}_rollout" in msg and "in_node_nf must be 1" in msg
    st, msg = _entry_call(family, 1, keep, 3)
    assert st < 0 and "keep-for-backward" in msg
    st, msg = _entry_call(family, 1, 64, 3)
    assert st < 0 and "unknown flag" in msg
    st, msg = _entry_call(family, 1, 0, 3, ws_bytes=256)
    assert st < 0 and "workspace too small" in msg
    for steps in (0, -2):                                          # returns 0 and launches nothing
        assert _entry_call(family, 1, 0, steps)[0] == 0


@pytest.mark.parametrize("K,model", MODELS)
def test_cpu_tensor_fails_loudly(K, model):
    m = _model(K, model)
    with pytest.raises(_lib.AetherHipError, match="no CPU fallback"):
        m.rollout(*_state(), 3)
    with pytest.raises(_lib.AetherHipError, match="no CPU fallback"):
        m.rollout(*_state(), 0)


@pytest.mark.parametrize("K,model", MODELS)
def test_bad_shapes_raise(K, model):
    m = _model(K, model)
    x, vel, edges, q = _state()
    for bad in ((x[:, :2], vel[:, :2], edges, q), (x, vel[:-1], edges, q), (x, vel, [edges[0], edges[1][:-1]], q),
                (x, vel, edges, q[:-1])):
        with pytest.raises(ValueError):
            m.rollout(*bad, 2)
    with pytest.raises(TypeError):
        m.rollout(x, vel, [e.int() for e in edges], q, 2)
    if K is Clof:
        with pytest.raises(ValueError, match="multiple of n_nodes"):
            m.rollout(x, vel, edges, q, 2, n_nodes=3)
    else:
        with pytest.raises(TypeError):
            m.rollout(x, vel, edges, q, 2, n_nodes=5)              # EGNN-Aether's forward has no such argument


@pytest.mark.parametrize("K,model", MODELS)
def test_wider_node_features_are_refused(K, model):
    """h = |vel| is rebuilt every step: a model whose embedding takes more than one column has no rollout."""
    m = _model(K, model, in_nf=2)
    with pytest.raises(ValueError, match="in_node_nf must be 1"):
        m.rollout(*_state(), 2)


def test_stepwise_loop_runs_the_runner_protocol():
    """rollout_stepwise_gnn hands the model what the runner would: |vel|, the squared distance, the velocity from the
    last two positions; charges only where the forward takes them."""
    from aether_amd.rollout import rollout_stepwise_gnn

    class Probe(torch.nn.Module):
        def __init__(self, with_charges):
            super().__init__()
            self.calls = []
            if with_charges:
                self.forward = self._with
            else:
                self.forward = self._without

        def _with(self, h, x, edges, vel, edge_attr, charges):
            return self._without(h, x, edges, vel, edge_attr)

        def _without(self, h, x, edges, vel, edge_attr, n_nodes=5):
            self.calls.append((h, x, vel, edge_attr, n_nodes))
            return x + 0.5 * vel

    x, vel, edges, q = (t.double() if torch.is_tensor(t) else t for t in _state())
    r, c = edges
    for with_charges, kw in ((True, {}), (False, dict(n_nodes=10))):
        p = Probe(with_charges)
        traj = rollout_stepwise_gnn(p, x, vel, edges, q, 3, dt=0.5, **kw)
        assert traj.shape == (3, 10, 3) and len(p.calls) == 3
        xs = [x] + list(traj)
        for t, (h, xt, vt, ea, n_per) in enumerate(p.calls):
            assert torch.equal(xt, xs[t]) and n_per == kw.get("n_nodes", 5)
            assert torch.equal(vt, vel if t == 0 else (xs[t] - xs[t - 1]) / 0.5)
            assert torch.equal(h, torch.sqrt((vt ** 2).sum(1, keepdim=True)))
            assert torch.equal(ea[:, :1], q[r] * q[c])
            assert torch.equal(ea[:, 1], ((xt[r] - xt[c]) ** 2).sum(1))
    assert rollout_stepwise_gnn(Probe(True), x, vel, edges, q, 0).shape == (0, 10, 3)
