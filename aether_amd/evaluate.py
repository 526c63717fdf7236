"""The forward-prediction metric of the seq2seq runners on the device (metric 2).

``eval_forward_prediction`` follows experiments/electrostatic/evaluate.py:14-79: the model sees the first
``burn_in_steps`` frames of every trajectory, predicts ``forward_pred_steps`` more with ``predict_future``, and the
per-step mean squared error is taken over (particle, feature) on UN-normalised values -- total, positions only and
velocities only -- averaged over the data set.  Inputs stay in HBM (no DataLoader, no host copies).
"""
from __future__ import annotations

import inspect

import torch


@torch.no_grad()
def eval_forward_prediction(model, dataset, burn_in_steps, forward_pred_steps, batch_size=1000, num_dims=None,
                            return_total_errors=False, **predict_kwargs):
    """-> (mse, pos_mse, vel_mse), each [forward_pred_steps] (or the per-sample errors with ``return_total_errors``)."""
    model.eval()
    D = num_dims if num_dims is not None else getattr(dataset, "ndim", 2)
    feats = dataset.feats
    tot, pos, vel = [], [], []
    # a charge-aware model (AetherCharges) takes the batch's charges, as experiments/electrostatic/evaluate.py:42-45 passes them
    charges = getattr(dataset, "charges", None)
    takes_charges = charges is not None and "charges" in inspect.signature(model.predict_future).parameters
    for lo in range(0, len(dataset), batch_size):
        inputs = feats[lo:lo + batch_size]
        kwargs = dict(predict_kwargs)
        if takes_charges and "charges" not in kwargs:
            kwargs["charges"] = charges[lo:lo + batch_size].reshape(inputs.shape[0], -1).to(inputs.device)
        preds = model.predict_future(inputs[:, :burn_in_steps], forward_pred_steps, **kwargs)
        gt = inputs[:, burn_in_steps:burn_in_steps + forward_pred_steps]
        p, g = dataset.torch_unnormalize(preds), dataset.torch_unnormalize(gt)
        se = (p - g) ** 2
        tot.append(se.flatten(2).mean(-1))                                   # [B, steps]
        pos.append(se[..., :D].flatten(2).mean(-1))
        vel.append(se[..., D:].flatten(2).mean(-1))
    tot, pos, vel = torch.cat(tot), torch.cat(pos), torch.cat(vel)
    if return_total_errors:
        return tot, pos, vel
    return tot.mean(0), pos.mean(0), vel.mean(0)


@torch.no_grad()
def eval_forward_prediction_dynamicvars(model, dataset, params=None, batch_size=64, return_bad_count=False):
    """The inD runner's metric, ``eval_forward_prediction_dynamicvars_unnormalized`` (experiments/ind/evaluate.py:6-82), on a
    ``SceneDataset``: per batch one ``predict_future_packed`` and one ``aether_dyn_eval_accumulate`` (the per-object loop
    of :48-80 for all scenes of the batch), fp64 sums kept on the device, ONE device-to-host copy at the end.
    ``params``: ``strict`` (:26-28) and ``report_error_norm`` (:16).
    -> (errors, pos_errors, vel_errors, counts), each of the reference's length, on the host (fp64); with
    ``return_bad_count`` also the number of tracks whose predicted steps are not contiguous (:72-75)."""
    from . import _lib
    lib = _lib.load()
    params = params or {}
    strict, error_norm = params.get("strict", -1), 1 if params.get("report_error_norm", False) else 0
    model.eval()
    dev = dataset.feats.device
    n_steps = int(dataset.feats.shape[1]) - 1
    acc = torch.zeros(4 * n_steps + 2, dtype=torch.float64, device=dev)         # sums [3][S] | counts [S] | (pad)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)
    scale, offset = dataset.scale.contiguous(), dataset.offset.contiguous()
    scratch = None
    for batch in dataset.batches(batch_size):
        inputs, masks = batch["inputs"].contiguous(), batch["masks"].contiguous()
        burn = batch["burn_in_masks"].clone()
        if strict > 0:
            burn[:, strict:] = 0.0
        preds = model.predict_future_packed(inputs, masks, burn, batch["pack"])
        truth = inputs[:, 1:].contiguous()
        B, Nmax = int(inputs.shape[0]), int(inputs.shape[2])
        need = lib.aether_dyn_eval_scratch_bytes(B, Nmax, n_steps)
        if need == 0:
            raise _lib.AetherHipError("aether_dyn_eval_scratch_bytes: " + lib.aether_last_error().decode())
        if scratch is None or scratch.numel() < need:
            scratch = torch.empty(need, dtype=torch.uint8, device=dev)
        keep = batch["keep"]
        keep = None if keep is None else keep.contiguous()
        st = lib.aether_dyn_eval_accumulate(preds.data_ptr(), truth.data_ptr(), int(preds.shape[-1]), masks.data_ptr(),
                                            burn.data_ptr(), scale.data_ptr(), offset.data_ptr(),
                                            None if keep is None else keep.data_ptr(), error_norm, B, Nmax, n_steps,
                                            acc.data_ptr(), acc.data_ptr() + 3 * n_steps * 8, stats.data_ptr(),
                                            scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(st, "aether_dyn_eval_accumulate")
    acc[4 * n_steps:] = stats.to(torch.float64)                                 # (exact: both are small integers)
    host = acc.cpu()
    bad, length = int(host[4 * n_steps]), int(host[4 * n_steps + 1])
    sums, counts = host[:3 * n_steps].view(3, n_steps)[:, :length], host[3 * n_steps:4 * n_steps][:length]
    out = (sums[0] / counts, sums[1] / counts, sums[2] / counts, counts.clone())
    return out + (bad,) if return_bad_count else out
