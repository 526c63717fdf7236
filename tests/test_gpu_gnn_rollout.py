"""Device rollout of EGNN-Aether and ClofNet on the MI355X (``aether_egnn_rollout`` / ``aether_clof_rollout`` through
``.rollout``) against the restatements (tests/egnn_restatement.py, tests/clof_restatement.py) looped on the CPU under the
protocol of metric 2: x_{t+1} = model(|v_t|, x_t, v_t, [q q, |dx|^2]), v_{t+1} = (x_{t+1} - x_t) / dt.

Errors are the project's: max|a - b| / max|b| per step, the worst step counts.  Inputs are fp32 values (the fp64 loop
starts from the same numbers the GPU gets).  Every input set was first run through the restatement loop alone, on the
CPU, in fp32 against fp64: the worst set held to the 1e-5 bar (4 steps at dt 0.5, EGNN-Aether with norm_diff) is at
9.7e-7, and in none of them does a translation come near the +-100 clamp (largest 4.0).  EGNN-Aether's rollout is not
stable for every state -- psi * vel feeds the velocity back -- so seeds whose fp64 loop leaves fp64's range within 20
steps (7 and 21 at B 2, N 5) are not used."""
import functools

import pytest
import torch

from aether_amd import rollout as RO

import clof_restatement as CR
import egnn_restatement as ER
import graph_cases as GC
import test_clof as TC
from conftest import scale_rel_err
from gnn_shape_checks import Clof, Egnn, state64

pytestmark = pytest.mark.gpu
TOL = 1e-5           # the bar of tests/test_gpu_egnn_aether.py / test_gpu_clof.py
GLUE_TOL = 1e-6      # same kernels, only the rounding of the glue between the steps differs

# hidden 64, 4 layers: EGNN-Aether with (norm_diff, tanh) = (True, False), (False, True); the three ClofNet variants
MODELS = {"egnn_norm": (Egnn, "egnn_aether", dict(norm_diff=True, tanh=False)),
          "egnn_tanh": (Egnn, "egnn_aether", dict(norm_diff=False, tanh=True)),
          "clof": (Clof, "clof", dict(norm_diff=True)),
          "clof_vel": (Clof, "clof_vel", dict(norm_diff=True)),
          "clof_vel_gbf": (Clof, "clof_vel_gbf", dict(norm_diff=True))}
ONE_PER_FAMILY = ("egnn_norm", "clof_vel")
LONG_SEED = 25       # chosen on the CPU: the fp64 loop stays finite and below the +-100 clamp for 20 steps (asserted)


def _cfg(name, N, seed=11):
    K, model, kw = MODELS[name]
    return K, K.cfg(model, 64, 4, seed, N, **kw)


@functools.lru_cache(maxsize=None)
def _module(name, N, seed=11):
    K, cfg = _cfg(name, N, seed)
    return K.build(cfg, "cuda")


@functools.lru_cache(maxsize=None)
def _inputs(graph, B, N, seed):
    """fp32 state on the CPU: x, vel, edges, charges.  graph: runner (fully connected), permuted (the same edges in a
    random order), sparse (graph_cases.random_multigraph: a node without edges, a self loop, duplicates, rows in random
    order), empty (no edge)."""
    if graph == "sparse":
        inp = GC.random_multigraph(B, N, seed, self_loop=True, dtype=torch.float32)
    else:
        inp = ER.runner_batch(B, N, seed)
    row, col = inp["edges"]
    if graph == "permuted":
        p = torch.randperm(row.numel(), generator=torch.Generator().manual_seed(seed + 1))
        row, col = row[p], col[p]
    if graph == "empty":
        row, col = row[:0], col[:0]
    return inp["x"], inp["vel"], (row, col), inp["charges"]


class _ClampWatch:
    """Largest |value| handed to the restatements' torch.clamp(..., -100, 100) while active."""

    def __enter__(self):
        self.worst, self._orig = 0.0, torch.clamp

        def clamp(t, *a, **k):
            if t.numel():
                self.worst = max(self.worst, float(t.detach().abs().max()))
            return self._orig(t, *a, **k)
        torch.clamp = clamp
        return self

    def __exit__(self, *exc):
        torch.clamp = self._orig


def _loop(K, cfg, sd, state, steps, dt, dtype):
    """The protocol around the restatement, in `dtype` -> ([steps, n, 3], largest |translation| before the clamp)."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    x, vel, (row, col), q = state
    x, vel, q = x.to(dtype), vel.to(dtype), q.to(dtype).reshape(-1, 1)
    qq = q[row] * q[col]
    traj = []
    with _ClampWatch() as watch, torch.no_grad():
        for _ in range(steps):
            ea = torch.cat([qq, ((x[row] - x[col]) ** 2).sum(1, keepdim=True)], 1)
            h = torch.sqrt((vel ** 2).sum(1, keepdim=True))
            if K is Egnn:
                xn = ER.forward(sd, h, x, (row, col), vel, ea, q, cfg["L"], cfg["norm_diff"], cfg["tanh"])[0]
            else:
                xn = CR.forward(sd, CR.VARIANTS[cfg["model"]], h, x, (row, col), vel, ea, cfg["L"], cfg["N"],
                                **TC.kwargs(cfg))[0]
            vel = (xn - x) / dt
            x = xn
            traj.append(x)
    return torch.stack(traj), watch.worst


@functools.lru_cache(maxsize=None)
def _reference(name, graph, B, N, seed, steps, dt, dtype=torch.float64):
    K, cfg = _cfg(name, N)
    return _loop(K, cfg, state64(_module(name, N)), _inputs(graph, B, N, seed), steps, dt, dtype)


def _worst_step(got, want):
    assert got.shape == want.shape
    return max(scale_rel_err(a, b) for a, b in zip(got.cpu(), want))


def _gpu_state(graph, B, N, seed):
    x, vel, (row, col), q = _inputs(graph, B, N, seed)
    return x.cuda(), vel.cuda(), [row.cuda(), col.cuda()], q.cuda()


def _kw(name, N):
    return dict(n_nodes=N) if MODELS[name][0] is Clof else {}


def _rollout(name, graph, B, N, seed, steps, dt):
    out = _module(name, N).rollout(*_gpu_state(graph, B, N, seed), steps, dt, **_kw(name, N))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dt", [1.0, 0.5])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_every_step_matches_the_fp64_loop(name, dt):
    got = _rollout(name, "runner", 2, 5, 25, 4, dt)
    want, _ = _reference(name, "runner", 2, 5, 25, 4, dt)
    assert got.shape == (4, 10, 3) and torch.isfinite(got).all()
    err = _worst_step(got, want)
    print(f"{name} dt {dt}: {err:.2e}")
    assert err <= TOL, err


@pytest.mark.parametrize("name", ONE_PER_FAMILY)
def test_twenty_steps_stay_within_four_times_the_fp32_restatement(name):
    """The bound comes from the reference: the fp32 restatement loop against the fp64 one (err32), times 4 for a
    different summation order per step, and never below the one-step bar.  Measured on the MI355X (err_hip / err32):
    egnn_norm 8.8e-07 / 6.9e-07, clof_vel 1.0e-06 / 7.2e-07; both figures are printed."""
    want, worst = _reference(name, "runner", 2, 5, LONG_SEED, 20, 1.0)
    assert torch.isfinite(want).all()
    assert worst < 100.0, worst                                   # the clamp is inactive all the way
    w32, _ = _reference(name, "runner", 2, 5, LONG_SEED, 20, 1.0, torch.float32)
    err32 = _worst_step(w32, want)
    got = _rollout(name, "runner", 2, 5, LONG_SEED, 20, 1.0)
    err_hip = _worst_step(got, want)
    print(f"{name}: err_hip {err_hip:.2e}, err32 {err32:.2e}")
    assert err_hip <= max(TOL, 4 * err32), (err_hip, err32)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_rollout_equals_the_loop_of_module_calls(name):
    """Same kernels; the glue between the steps may round a last bit differently (6e-8), and the rollout carries that
    forward.  How far is the reference's own figure: the fp32 restatement loop against the fp64 one, on the CPU, is at
    1.1e-7 .. 3.2e-7 after 4 steps at dt 1 -- room under the 1e-6 this test allows -- but at 9.7e-7 at dt 0.5 (every
    step doubles the velocity's rounding error), where fp32 arithmetic alone is at the bound and a comparison at 1e-6 says
    nothing about the glue.  So dt is 1 here.  (At dt 0.5 the MI355X gives 1.3e-7 .. 7.1e-7 and, for EGNN-Aether with
    tanh, 1.3e-6.)"""
    state = _gpu_state("runner", 2, 5, 25)
    got = _rollout(name, "runner", 2, 5, 25, 4, 1.0)
    loop = RO.rollout_stepwise_gnn(_module(name, 5), *state, 4, 1.0, **_kw(name, 5))
    err = _worst_step(got, loop.cpu())
    print(f"{name}: {err:.2e}")
    assert err <= GLUE_TOL, err


@pytest.mark.parametrize("name", ONE_PER_FAMILY)
def test_one_step_is_the_forward_and_nothing_is_left_behind(name):
    m = _module(name, 5)
    x, vel, edges, q = _gpu_state("runner", 2, 5, 25)
    row, col = edges
    ea = torch.cat([q[row] * q[col], ((x[row] - x[col]) ** 2).sum(1, keepdim=True)], 1)
    h = torch.sqrt((vel ** 2).sum(1, keepdim=True))
    args = (h, x, edges, vel, ea) + ((q,) if MODELS[name][0] is Egnn else ())
    x0, v0 = x.clone(), vel.clone()
    with torch.no_grad():
        before = m(*args, **_kw(name, 5)).clone()
    one = m.rollout(x, vel, edges, q, 1, **_kw(name, 5))
    m.rollout(x, vel, edges, q, 3, 0.5, **_kw(name, 5))
    with torch.no_grad():
        after = m(*args, **_kw(name, 5))
    torch.cuda.synchronize()
    assert one.shape == (1, 10, 3)
    assert scale_rel_err(one[0].cpu(), before.cpu()) <= GLUE_TOL
    assert torch.equal(before, after)                             # no stale weight images or workspace state
    assert torch.equal(x, x0) and torch.equal(vel, v0)            # the caller's state is not written
    empty = m.rollout(x, vel, edges, q, 0, **_kw(name, 5))
    assert empty.shape == (0, 10, 3) and empty.is_cuda


@pytest.mark.parametrize("graph,B,N", [("permuted", 2, 5), ("sparse", 3, 7)])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_edge_attr_is_rebuilt_in_the_callers_edge_order(name, graph, B, N):
    """A shuffled edge list, and a sparse graph with a node without edges and a self loop: the rebuilt edge_attr is read
    through the row-sorted view's permutation, so it has to be written in the caller's order."""
    row, col = _inputs(graph, B, N, 23)[2]
    assert not torch.equal(row, row.sort().values)
    if graph == "sparse":
        assert int((row == col).sum()) == 1 and len(set(row.tolist()) | set(col.tolist())) < B * N
    want, _ = _reference(name, graph, B, N, 23, 3, 1.0)
    assert torch.isfinite(want).all()
    err = _worst_step(_rollout(name, graph, B, N, 23, 3, 1.0), want)
    print(f"{name} {graph}: {err:.2e}")
    assert err <= TOL, err


@pytest.mark.parametrize("B,N", [(1, 7), (13, 20)])
@pytest.mark.parametrize("name", ONE_PER_FAMILY)
def test_sizes_across_a_workgroup_of_the_state_kernel(name, B, N):
    """7 nodes / 42 edges, and 260 nodes / 4940 edges: the elementwise grid ends inside, and spans more than, a
    workgroup of 256, for the node part and the edge part alike."""
    want, _ = _reference(name, "runner", B, N, 25, 2, 1.0)
    got = _rollout(name, "runner", B, N, 25, 2, 1.0)
    assert torch.isfinite(got).all()
    err = _worst_step(got, want)
    print(f"{name} B {B} N {N}: {err:.2e}")
    assert err <= TOL, err


@pytest.mark.parametrize("name", ONE_PER_FAMILY)
def test_a_graph_without_edges(name):
    want, _ = _reference(name, "empty", 2, 5, 27, 2, 1.0)
    got = _rollout(name, "empty", 2, 5, 27, 2, 1.0)
    assert torch.isfinite(got).all() and torch.isfinite(want).all()
    assert _worst_step(got, want) <= TOL


@pytest.mark.parametrize("name", ONE_PER_FAMILY)
def test_two_runs_are_bit_identical(name):
    a = _rollout(name, "runner", 13, 20, 25, 2, 1.0)
    b = _rollout(name, "runner", 13, 20, 25, 2, 1.0)
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", ONE_PER_FAMILY)
def test_captured_rollout_replays_the_eager_result(name):
    m = _module(name, 5)
    state = _gpu_state("runner", 2, 5, 25)
    kw = _kw(name, 5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = m.rollout(*state, 4, 0.5, **kw)                   # the warm-up call: graph view and workspace exist
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = m.rollout(*state, 4, 0.5, **kw)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


@pytest.mark.parametrize("name", ONE_PER_FAMILY)
def test_rollout_dispatch_reaches_the_drop_in(name):
    """aether_amd.rollout.rollout(model, x, vel, edges, charges, steps, dt), as for Aether: ClofNet with its default
    n_nodes = 5."""
    state = _gpu_state("runner", 2, 5, 25)
    got = RO.rollout(_module(name, 5), *state, 4, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(got, _rollout(name, "runner", 2, 5, 25, 4, 0.5))
