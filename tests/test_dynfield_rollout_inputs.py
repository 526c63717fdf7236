"""CPU side of the dynamic-field rollout-training checks (tests/test_gpu_dynfield_rollout_train.py): its inputs are fit to
hold the HIP path to ``max(GTOL, 4 err32)`` -- no edge of any step within 1e-4 rad of a branch cut of the feature map, the
fp32 oracle's own gradient error below GTOL, so the ``4 err32`` term cannot hide a failure -- plus the host-only parts of
the new entries (size query, Python error paths that need no GPU)."""
import pytest
import torch

from conftest import scale_rel_err
from aether_amd import _lib
from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
from dynfield_rollout_cases import ALL_CASES, GTOL, ZERO_GRAD, case


@pytest.mark.parametrize("shape", ALL_CASES)
@pytest.mark.parametrize("D", [2, 3])
def test_reference_inputs_are_clear_of_branch_cuts_and_fp32_noise(D, shape):
    c = case(D, *shape)
    print(f"[dynfield rollout inputs] D={D} {shape}: cut margin {c['margin']:.2e} rad, "
          f"trajectory fp32 vs fp64 {scale_rel_err(c['traj32'], c['traj64']):.2e}")
    assert c["margin"] >= 1e-4, c["margin"]
    assert set(c["g64"]) == set(c["sd"]) | {"x0", "vel0"}
    worst = 0.0
    for k, g in c["g64"].items():
        assert torch.isfinite(g).all(), k
        if k == ZERO_GRAD:                                            # exactly zero on both sides
            assert float(g.abs().max()) <= 1e-9 and float(c["g32"][k].abs().max()) <= 1e-9
            continue
        err32 = scale_rel_err(c["g32"][k], g)
        worst = max(worst, err32)
        assert err32 <= GTOL, (k, err32)
    print(f"[dynfield rollout inputs] D={D} {shape}: worst fp32 oracle gradient error {worst:.2e}")


def test_workspace_size_query_is_host_arithmetic():
    """The workspace of the rollout-training entries plus the latent field's buffers (one partial gradient row per graph,
    three per-node buffers): larger for the same sizes, the same growth per step; sizes the entry refuses give 0."""
    lib = _lib.load()
    q = lib.aether_rollout_dynamic_field_train_workspace_bytes
    n, E, N = 2560, 48640, 20
    total = {K: q(n, E, 2, 64, N, K) for K in (1, 2, 4, 20)}
    plain = {K: lib.aether_rollout_train_workspace_bytes(n, E, 2, 64, K) for K in (1, 2, 4, 20)}
    for K in total:
        assert total[K] > plain[K] > 0
        assert total[K] - plain[K] == total[1] - plain[1]             # the extras do not depend on the steps
    per_step = total[2] - total[1]
    assert per_step > 0 and per_step % 256 == 0
    assert total[4] - total[1] == 3 * per_step and total[20] - total[1] == 19 * per_step
    extras = lib.aether_dynamic_field_backward_workspace_bytes(2, n // N) + n * 2 * 4 * 4
    assert extras - 256 <= total[1] - plain[1] <= extras + 8 * 256
    assert q(n, E, 2, 128, N, 4) == 0                                 # the 64-wide engine only
    assert q(n, E, 2, 64, N, 0) == 0
    assert q(n, E, 2, 64, 7, 4) == 0                                  # n_nodes % nodes_per_graph != 0
    assert q(n, E, 4, 64, N, 4) == 0
    assert q(n, E, 2, 64, 0, 4) == 0
    assert q(4096, E, 2, 64, 4096, 4) == 0                            # more than 2048 nodes per graph
    assert q(0, 0, 2, 64, N, 4) == 0


def test_python_error_paths_without_a_gpu():
    e = [torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0])]
    x, v, q = torch.zeros(3, 2), torch.ones(3, 2), torch.ones(3, 1)
    m = DynamicFieldAether(4, 64, 0.0, 2, device="cpu")
    with pytest.raises(_lib.AetherHipError, match="not built"):       # the objects per graph cannot be inferred
        m.differentiable_rollout(x, v, e, q, 2)
    with pytest.raises(_lib.AetherHipError, match="not built"):
        m.differentiable_rollout(x, v, e, q, 0)                       # (this check comes first)
    with pytest.raises(ValueError):
        m.differentiable_rollout(x, v, e, q, 0, num_nodes=3)
    with pytest.raises(_lib.AetherHipError):                          # no CPU fallback
        m.differentiable_rollout(x, v, e, q, 2, num_nodes=3)
    from aether_amd.rollout import rollout_loss
    with pytest.raises(_lib.AetherHipError):
        rollout_loss(m, x, v, e, q, torch.zeros(2, 3, 2), num_nodes=3)
    with pytest.raises(ValueError):
        rollout_loss(m, x, v, e, q, torch.zeros(3, 2), num_nodes=3)
    from aether_amd.training import GraphedRolloutTrainStep
    for args in [(x, v, e), (x, v, e, q, 3, 1)]:                      # checked before anything touches a device
        with pytest.raises(ValueError, match="example_args"):
            GraphedRolloutTrainStep(m, args, torch.zeros(2, 3, 2))
