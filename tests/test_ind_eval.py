"""Variable-N (inD) family, host side of the device scene pack and the prediction metric: the fp64 restatement of the
metric against the golden results of the reference's own evaluate.py, the burn-in formula, and what the two new library
entries refuse before anything is queued.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from aether_amd import _lib
import ind_eval_restatement as R

NEW = ("aether_dyn_scene_pack_bytes", "aether_dyn_scene_pack", "aether_dyn_eval_scratch_bytes", "aether_dyn_eval_accumulate")
EINVAL, ESPACE = -1, -4


def _golden(name):
    return np.load(os.path.join(GOLDEN, f"ind_eval_{name}.npz"))


@pytest.mark.parametrize("name,norm,strict", R.VARIANTS)
def test_restatement_matches_the_reference(name, norm, strict):
    """All five scenes as ONE batch through the restatement: within 1e-5 * max|ref| of the reference's fp32 results
    (its own rounding sits 1.6e-6 from fp64 on this fixture), NaN positions equal; counts, bad count and length exact."""
    z = _golden(name)
    scale, offset = R.stats_scale_offset(z)
    keep = z["non_linear_masks"] if "non_linear_masks" in z else None
    acc = R.accumulate(z["preds"], z["inputs"][:, 1:], z["masks"], R.apply_strict(z["burn_in_masks"], strict), scale, offset,
                       keep, bool(norm))
    got, t = R.finish(acc), R.tag(norm, strict)
    for key, val in zip(("errors", "pos_errors", "vel_errors"), got):
        ok, err = R.close(val, z[f"{key}_{t}"])
        print(f"{name} {t} {key}: max abs diff {err:.3e}, max|ref| {np.nanmax(np.abs(z[f'{key}_{t}'])):.3e}")
        assert ok, (key, err)
    assert np.array_equal(got[3], z[f"counts_{t}"].astype(np.float64))
    assert acc["bad"] == int(z[f"bad_count_{t}"])
    assert acc["length"] == len(z[f"errors_{t}"])


def test_restatement_is_a_sequence_of_calls():
    """2 + 2 + 1 scenes accumulate to what one call over the five gives (fp64: to rounding)."""
    z = _golden("minmax")
    scale, offset = R.stats_scale_offset(z)
    burn = R.apply_strict(z["burn_in_masks"], 2)
    whole = R.accumulate(z["preds"], z["inputs"][:, 1:], z["masks"], burn, scale, offset)
    acc = None
    for lo, hi in ((0, 2), (2, 4), (4, 5)):
        acc = R.accumulate(z["preds"][lo:hi], z["inputs"][lo:hi, 1:], z["masks"][lo:hi], burn[lo:hi], scale, offset, acc=acc)
    np.testing.assert_allclose(acc["sums"], whole["sums"], rtol=1e-13, atol=0)
    assert np.array_equal(acc["counts"], whole["counts"]) and (acc["bad"], acc["length"]) == (whole["bad"], whole["length"])


def test_burn_in_formula_equals_the_loop():
    """masks * (exclusive cumsum over time < max_burn_in_count) is the reference's loop (single_ind_data.py:73-81): exact,
    on the golden masks and on random ones, for several limits (-1, the data set's default, included)."""
    from aether_amd.data import burn_in_masks_of
    z = _golden("minmax")
    masks = torch.from_numpy(z["masks"])
    assert torch.equal(burn_in_masks_of(masks, int(z["max_burn_in_count"])), torch.from_numpy(z["burn_in_masks"]))
    g = torch.Generator().manual_seed(3)
    rnd = (torch.rand(4, 11, 7, generator=g) > 0.35).float()
    for limit in (-1, 0, 1, 3, 20):
        assert np.array_equal(burn_in_masks_of(rnd, limit).numpy().astype(np.float64), R.burn_in_loop(rnd.numpy(), limit)), limit


def test_scene_dataset_statistics_follow_the_reference_formulas():
    """SceneDataset's scale / offset reproduce unnormalize_data (single_ind_data.py:122-141) in both modes (CPU tensors)."""
    from aether_amd.data import SceneDataset
    z = _golden("minmax")
    x, m = torch.from_numpy(z["inputs"]), torch.from_numpy(z["masks"])
    lo, hi = torch.from_numpy(z["min_feats"]), torch.from_numpy(z["max_feats"])
    ds = SceneDataset(x, m, max_burn_in_count=3, stats=(lo, hi), device="cpu")
    torch.testing.assert_close(ds.unnormalize_data(x), (x + 1) * (hi - lo) / 2.0 + lo, rtol=1e-6, atol=1e-5)
    assert torch.equal(ds.burn_in_masks, torch.from_numpy(z["burn_in_masks"])) and len(ds) == 5
    ds = SceneDataset(x, m, max_burn_in_count=3, stats=torch.tensor(7.5), device="cpu")
    assert torch.equal(ds.unnormalize_data(x), x * 7.5)


def test_new_entries_are_bound_and_sized():
    for name in NEW:
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    for shape in ((3, 12, 7, 10), (5, 6, 9, 10), (1, 12, 7, 10), (64, 20, 50, 10)):
        need = lib.aether_dyn_scene_pack_bytes(*shape)
        B, N, T, k = shape
        assert need >= T * B * N * 8 * (1 + 3 * k), shape
    for shape in ((5, 6, 8), (2, 6, 8), (1, 6, 8), (64, 20, 49)):
        B, N, S = shape
        assert lib.aether_dyn_eval_scratch_bytes(*shape) >= B * N * 4 * S * 8, shape


def test_scene_pack_refuses_bad_arguments_before_queueing():
    """Null pointers, n_scenes outside 1..256, k outside 1..16: AETHER_EINVAL; a short pack: AETHER_ESPACE -- decided on the
    host (this test has no device: nothing can have been queued), each with a message."""
    lib = _lib.load()
    B, N, T, k = 3, 12, 7, 10
    need = lib.aether_dyn_scene_pack_bytes(B, N, T, k)
    view = _lib.AetherDynScenePack()
    n, e, d = (C.c_int64 * (T * B))(), (C.c_int64 * (T * B))(), (C.c_int * (T * B))()
    fake = 4096                                                   # a non-null "device" address: never dereferenced
    call = lambda x=fake, m=fake, B=B, N=N, T=T, k=k, pack=fake, size=need, v=C.byref(view), n=n: \
        lib.aether_dyn_scene_pack(x, m, B, N, T, k, pack, size, v, n, e, d, None)
    for kwargs, code, word in ((dict(x=None), EINVAL, "null"), (dict(m=None), EINVAL, "null"), (dict(pack=None), EINVAL, "null"),
                               (dict(v=None), EINVAL, "null"), (dict(n=None), EINVAL, "null"),
                               (dict(B=0), EINVAL, "n_scenes"), (dict(B=257), EINVAL, "n_scenes"),
                               (dict(k=0), EINVAL, "k must"), (dict(k=17), EINVAL, "k must"),
                               (dict(size=need - 1), ESPACE, "too small")):
        assert call(**kwargs) == code, kwargs
        assert word in lib.aether_last_error().decode(), (kwargs, lib.aether_last_error())
    assert lib.aether_dyn_scene_pack_bytes(257, N, T, k) == 0 and lib.aether_dyn_scene_pack_bytes(B, N, T, 17) == 0


def test_eval_accumulate_refuses_bad_arguments_before_queueing():
    lib = _lib.load()
    B, N, S = 5, 6, 8
    need = lib.aether_dyn_eval_scratch_bytes(B, N, S)
    fake = 4096
    call = lambda preds=fake, F=4, scratch=fake, size=need, B=B: lib.aether_dyn_eval_accumulate(
        preds, fake, F, fake, fake, fake, fake, None, 0, B, N, S, fake, fake, fake, scratch, size, None)
    for kwargs, code in ((dict(preds=None), EINVAL), (dict(scratch=None), EINVAL), (dict(F=3), EINVAL), (dict(B=0), EINVAL),
                         (dict(size=need - 1), ESPACE)):
        assert call(**kwargs) == code, kwargs
        assert lib.aether_last_error().decode().startswith("dyn_eval"), kwargs
