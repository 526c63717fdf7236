"""CPU side of the rollout-training checks: the inputs of tests/test_gpu_rollout_train.py are fit to hold the HIP path
to ``max(GTOL, 4 err32)`` -- no edge of any step sits near a branch cut of the feature map, and the fp32 oracle's own
gradient error is below GTOL, so the ``4 err32`` term cannot hide a failure -- plus the host-only parts of the new entries
(size query, Python error paths that need no GPU)."""
import pytest
import torch

from conftest import scale_rel_err
from aether_amd import _lib
from aether_amd.nn.state2state.aether import Aether
from aether_amd.nn.state2state.dynamic_field_aether import DynamicFieldAether
from aether_amd.nn.state2state.locs import LoCS
from rollout_train_cases import GTOL, LAYOUT_SHAPES, SHAPES, TWO_STEPS, case, locs_case, multigraph_case


def _fit(tag, c, margin=True):
    """No edge of any step within 1e-4 rad of a branch cut; the fp32 oracle's own gradient error below GTOL."""
    if margin:
        print(f"[rollout inputs] {tag}: cut margin {c['margin']:.2e} rad, "
              f"trajectory fp32 vs fp64 {scale_rel_err(c['traj32'], c['traj64']):.2e}")
        assert c["margin"] >= 1e-4, c["margin"]
    worst = 0.0
    for k, g in c["g64"].items():
        assert torch.isfinite(g).all(), k
        err32 = scale_rel_err(c["g32"][k], g)
        worst = max(worst, err32)
        assert err32 <= GTOL, (k, err32)
    print(f"[rollout inputs] {tag}: worst fp32 oracle gradient error {worst:.2e}")


@pytest.mark.parametrize("shape", SHAPES + [TWO_STEPS] + list(LAYOUT_SHAPES.values()))
@pytest.mark.parametrize("D", [2, 3])
def test_reference_inputs_are_clear_of_branch_cuts_and_fp32_noise(D, shape):
    _fit(f"D={D} {shape}", case(D, *shape))


@pytest.mark.parametrize("D", [2, 3])
def test_multigraph_and_locs_references_are_fit_too(D):
    """The other cases the GPU tests hold to max(GTOL, 4 err32): the random multigraph, and LoCS (hidden 64 and 20)
    against its restatement (whose rollout returns no margins: LoCS's edge features are Aether's first columns, on the
    same inputs as SHAPES[0])."""
    _fit(f"D={D} multigraph", multigraph_case(D))
    for hidden in (64, 20):
        _fit(f"D={D} LoCS hidden {hidden}", locs_case(D, hidden)[1], margin=False)


def test_workspace_size_query_is_host_arithmetic():
    """One whole training slice (the last step's) plus, per further step, only what a forward keeps for its backward --
    more than the inference workspace, far less than a training workspace -- plus the chain's scratch; sizes the entry
    refuses give 0."""
    lib = _lib.load()
    one, infer = lib.aether_workspace_bytes(2560, 48640, 2, 1), lib.aether_workspace_bytes(2560, 48640, 2, 0)
    total = {K: lib.aether_rollout_train_workspace_bytes(2560, 48640, 2, 64, K) for K in (1, 2, 4, 20)}
    assert one < total[1] <= one + (8 << 20)
    per_step = total[2] - total[1]
    assert infer < per_step < one // 4 and per_step % 256 == 0
    assert total[4] - total[1] == 3 * per_step and total[20] - total[1] == 19 * per_step
    assert lib.aether_rollout_train_workspace_bytes(2560, 48640, 2, 64, 0) == 0
    assert lib.aether_rollout_train_workspace_bytes(2560, 48640, 2, 128, 4) == 0        # the 64-wide engine only
    assert lib.aether_rollout_train_workspace_bytes(0, 0, 2, 64, 4) == 0
    assert lib.aether_rollout_train_workspace_bytes(10, 10, 4, 64, 4) == 0


def test_python_error_paths_without_a_gpu():
    e = [torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0])]
    x, v, q = torch.zeros(3, 2), torch.ones(3, 2), torch.ones(3, 1)
    for cls in (Aether, LoCS):
        m = cls(4, 64, 0.0, 2, device="cpu")
        with pytest.raises(ValueError):
            m.differentiable_rollout(x, v, e, q, 0)
        with pytest.raises(_lib.AetherHipError):                        # no CPU fallback
            m.differentiable_rollout(x, v, e, q, 2)
    with pytest.raises(_lib.AetherHipError, match="not built"):
        DynamicFieldAether(4, 64, 0.0, 2, device="cpu").differentiable_rollout(x, v, e, q, 2)
    from aether_amd.rollout import rollout_loss
    with pytest.raises(ValueError):
        rollout_loss(Aether(4, 64, 0.0, 2, device="cpu"), x, v, e, q, torch.zeros(3, 2))
