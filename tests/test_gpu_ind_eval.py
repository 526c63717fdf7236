"""Variable-N (inD) family: the runner's forward-prediction metric on the device (``aether_dyn_eval_accumulate``,
``eval_forward_prediction_dynamicvars``) against the fp64 restatement that ``tests/test_ind_eval.py`` holds to the
reference's own results."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from aether_amd import _lib
from aether_amd.data import SceneDataset
from aether_amd.evaluate import eval_forward_prediction_dynamicvars
import ind_eval_restatement as R
from test_gpu_dynamicvars import _scene_model

pytestmark = pytest.mark.gpu
_Z = {}


def _golden(name):
    """The golden file on the device, loaded once: dict of numpy arrays + 'dev' (float32 CUDA tensors)."""
    if name not in _Z:
        z = dict(np.load(os.path.join(GOLDEN, f"ind_eval_{name}.npz")))
        z["dev"] = {k: torch.from_numpy(z[k]).cuda() for k in ("inputs", "masks", "burn_in_masks", "preds")}
        _Z[name] = z
    return _Z[name]


def _accumulate(z, norm, strict, splits):
    """``aether_dyn_eval_accumulate`` over the scenes [lo, hi) of ``splits``, one call each, into fresh accumulators
    -> (sums [3, S], counts [S], bad count, length) on the host."""
    lib, d = _lib.load(), z["dev"]
    S, N = d["preds"].shape[1], d["preds"].shape[2]
    scale, offset = R.stats_scale_offset(z)
    so = torch.tensor(np.concatenate([scale, offset]), dtype=torch.float32, device="cuda")
    keep_all = torch.from_numpy(z["non_linear_masks"]).cuda() if "non_linear_masks" in z else None
    burn_all = d["burn_in_masks"].clone()
    if strict > 0:
        burn_all[:, strict:] = 0.0
    acc = torch.zeros(4 * S, dtype=torch.float64, device="cuda")
    stats = torch.zeros(2, dtype=torch.int64, device="cuda")
    for lo, hi in splits:
        preds, truth = d["preds"][lo:hi].contiguous(), d["inputs"][lo:hi, 1:].contiguous()
        masks, burn = d["masks"][lo:hi].contiguous(), burn_all[lo:hi].contiguous()
        keep = None if keep_all is None else keep_all[lo:hi].contiguous()
        need = lib.aether_dyn_eval_scratch_bytes(hi - lo, N, S)
        scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
        st = lib.aether_dyn_eval_accumulate(preds.data_ptr(), truth.data_ptr(), 4, masks.data_ptr(), burn.data_ptr(),
                                            so.data_ptr(), so.data_ptr() + 16, None if keep is None else keep.data_ptr(),
                                            norm, hi - lo, N, S, acc.data_ptr(), acc.data_ptr() + 3 * S * 8, stats.data_ptr(),
                                            scratch.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
        _lib.check(st, "aether_dyn_eval_accumulate")
    host = acc.cpu().numpy()
    return host[:3 * S].reshape(3, S), host[3 * S:], int(stats[0]), int(stats[1])


def _restated(z, norm, strict, preds=None):
    scale, offset = R.stats_scale_offset(z)
    keep = z["non_linear_masks"] if "non_linear_masks" in z else None
    return R.accumulate(z["preds"] if preds is None else preds, z["inputs"][:, 1:], z["masks"],
                        R.apply_strict(z["burn_in_masks"], strict), scale, offset, keep, bool(norm))


@pytest.mark.parametrize("name,norm,strict", R.VARIANTS)
def test_accumulate_matches_the_restatement(name, norm, strict):
    z = _golden(name)
    sums, counts, bad, length = _accumulate(z, norm, strict, [(0, 5)])
    want = _restated(z, norm, strict)
    assert np.array_equal(counts, want["counts"]) and bad == want["bad"] and length == want["length"]
    assert bad == int(z[f"bad_count_{R.tag(norm, strict)}"]) and length == len(z[f"errors_{R.tag(norm, strict)}"])
    got = dict(sums=sums, counts=counts, length=length)
    for key, a, b in zip(("errors", "pos_errors", "vel_errors"), R.finish(got), R.finish(want)):
        ok, err = R.close(a, b)
        print(f"{name} {R.tag(norm, strict)} {key}: max abs diff {err:.3e}, max|ref| {np.nanmax(np.abs(b)):.3e}")
        assert ok, (key, err)
    assert not sums[:, length:].any() and not counts[length:].any()


def test_a_data_set_is_a_sequence_of_calls_in_fp64():
    """Five scenes in one call, as 2 + 2 + 1 and as five calls: the fp64 sums agree to 1e-12 relative (at most about 1e3
    terms at 1.1e-16 each; an fp32 accumulation anywhere would sit near 1e-7), counts and stats exactly."""
    z = _golden("minmax")
    whole = _accumulate(z, 0, 2, [(0, 5)])
    for splits in ([(0, 2), (2, 4), (4, 5)], [(i, i + 1) for i in range(5)]):
        part = _accumulate(z, 0, 2, splits)
        rel = np.abs(part[0] - whole[0]).max() / np.abs(whole[0]).max()
        print(f"{len(splits)} calls vs one: max relative difference of the sums {rel:.3e}")
        assert rel <= 1e-12
        assert np.array_equal(part[1], whole[1]) and part[2:] == whole[2:]


@pytest.mark.parametrize("name,norm,strict", [("minmax", 0, -1), ("velnorm", 1, 2)])
def test_eval_forward_prediction_dynamicvars(name, norm, strict):
    """The whole runner metric on a SceneDataset of the golden scenes (un-padded, batch_size 2: batches of 2, 2 and 1)
    equals the restatement fed with ``predict_future_packed``'s own predictions (same draws) within 1e-5."""
    z = _golden(name)
    shapes = [tuple(int(v) for v in s) for s in z["shapes"]]
    feats = [torch.from_numpy(z["inputs"][i, :t, :n]) for i, (t, n) in enumerate(shapes)]
    masks = [torch.from_numpy(z["masks"][i, :t, :n]) for i, (t, n) in enumerate(shapes)]
    stats = torch.from_numpy(z["vel_norm_max"]) if name == "velnorm" else (torch.from_numpy(z["min_feats"]),
                                                                          torch.from_numpy(z["max_feats"]))
    nl = [z["non_linear_masks"][i, :n] for i, (_, n) in enumerate(shapes)] if name == "velnorm" else None
    ds = SceneDataset(feats, masks, max_burn_in_count=int(z["max_burn_in_count"]), stats=stats, non_linear_masks=nl)
    assert len(ds) == 5 and torch.equal(ds.burn_in_masks.cpu(), torch.from_numpy(z["burn_in_masks"]))
    assert torch.equal(ds.feats.cpu(), torch.from_numpy(z["inputs"]))
    model = _scene_model()[0].cuda()
    params = {"strict": strict, "report_error_norm": bool(norm)}
    torch.cuda.manual_seed(11)
    got = eval_forward_prediction_dynamicvars(model, ds, params, batch_size=2, return_bad_count=True)
    torch.cuda.manual_seed(11)
    preds = []
    for batch in ds.batches(2):
        burn = batch["burn_in_masks"].clone()
        if strict > 0:
            burn[:, strict:] = 0.0
        preds.append(model.predict_future_packed(batch["inputs"], batch["masks"], burn, batch["pack"]).cpu())
    want = _restated(z, norm, strict, torch.cat(preds).numpy())
    assert got[4] == want["bad"] and len(got[0]) == want["length"]
    assert np.array_equal(got[3].numpy(), want["counts"][:want["length"]])
    for key, a, b in zip(("errors", "pos_errors", "vel_errors"), got[:3], R.finish(want)):
        ok, err = R.close(a.numpy(), b)
        print(f"{name} {key}: max abs diff {err:.3e}, max|ref| {np.nanmax(np.abs(b)):.3e}")
        assert ok, (key, err)
    # a data-set entry goes through the unchanged predict_future (scene 3 is 7 frames x 4 objects, un-padded)
    item = ds[3]
    assert item["inputs"].shape == (7, 4, 4) and len(item["node_inds"]) == 7 and len(item["graph_info"]) == 7
    out = model.predict_future(item["inputs"][None], item["masks"][None], [item["node_inds"]], [item["graph_info"]],
                               item["burn_in_masks"][None])
    assert out.shape == (1, 6, 4, 4) and bool(torch.isfinite(out).all())
