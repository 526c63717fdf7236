"""fp64 restatement of the inD runner's forward-prediction metric for batches of padded scenes (a helper module like
``graph_cases.py``: no tests here).  experiments/ind/evaluate.py:29-82 of the reference, object by object, in numpy
float64; ``tests/test_ind_eval.py`` holds it to the golden results of the reference itself, the GPU tests hold the
library to it.
"""
from __future__ import annotations

import numpy as np


def apply_strict(burn_in_masks, strict):
    """:26-28 -- a copy of the burn-in masks [B, T, N] with the frames from ``strict`` on cleared (strict > 0)."""
    burn = np.array(burn_in_masks, dtype=np.float64, copy=True)
    if strict > 0:
        burn[:, strict:] = 0.0
    return burn


def burn_in_loop(masks, max_burn_in_count):
    """experiments/ind/single_ind_data.py:73-81, the loop itself, for masks [B, T, N]."""
    masks = np.asarray(masks, dtype=np.float64)
    out = np.zeros_like(masks)
    for b in range(masks.shape[0]):
        count = np.zeros(masks.shape[2])
        for t in range(masks.shape[1]):
            out[b, t] = (masks[b, t] == 1) * (count < max_burn_in_count)
            count += out[b, t]
    return out


def accumulate(preds, truth, masks, burn_in_masks, scale, offset, keep=None, error_norm=False, acc=None):
    """One batch.  preds, truth [B, S, N, F >= 4]; masks, burn_in_masks [B, S + 1, N] (after ``apply_strict``); scale,
    offset [4]; keep [B, N] or None.  ``acc``: the running state (None: fresh) -> dict(sums [3, S], counts [S], bad, length);
    a data set is a sequence of calls."""
    preds, truth = np.asarray(preds, dtype=np.float64)[..., :4], np.asarray(truth, dtype=np.float64)[..., :4]
    masks, burn = np.asarray(masks, dtype=np.float64), np.asarray(burn_in_masks, dtype=np.float64)
    scale, offset = np.asarray(scale, dtype=np.float64).reshape(4), np.asarray(offset, dtype=np.float64).reshape(4)
    B, S, N = preds.shape[:3]
    if acc is None:
        acc = dict(sums=np.zeros((3, S)), counts=np.zeros(S), bad=0, length=0)
    diff = (preds * scale + offset) - (truth * scale + offset)
    sq = diff ** 2
    for b in range(B):
        pred_masks = (masks[b] - burn[b])[1:]                                   # [S, N]  (:29)
        acc["length"] = max(acc["length"], int(pred_masks.sum(0).max()))        # :41
        for j in range(N):
            pm = pred_masks[:, j]
            if not burn[b, :, j].any():                                         # :52
                continue
            if keep is not None and not keep[b][j]:                             # :55-58
                continue
            total = sq[b, :, j].mean(-1) * pm                                   # :59-62
            if error_norm:                                                      # :63-68
                pos, vel = np.sqrt(sq[b, :, j, :2].sum(-1)) * pm, np.sqrt(sq[b, :, j, 2:].sum(-1)) * pm
            else:
                pos, vel = sq[b, :, j, :2].mean(-1) * pm, sq[b, :, j, 2:].mean(-1) * pm
            nz = np.nonzero(pm)[0]
            if len(nz) == 0:                                                    # :70
                continue
            if np.any(np.diff(nz) != 1):                                        # :72-75
                acc["bad"] += 1
            first, num = int(nz[0]), int(pm.sum())
            for row, val in zip(acc["sums"], (total, pos, vel)):
                row[:num] += val[first:first + num]
            acc["counts"][:num] += pm[first:first + num]
    return acc


def finish(acc):
    """:82 -> (errors, pos_errors, vel_errors, counts), each of length ``acc['length']`` (NaN where the count is 0)."""
    L = acc["length"]
    counts = acc["counts"][:L]
    with np.errstate(invalid="ignore", divide="ignore"):
        return tuple(acc["sums"][q, :L] / counts for q in range(3)) + (counts.copy(),)


def stats_scale_offset(z):
    """scale, offset of y = scale x + offset from a golden file's statistics (single_ind_data.py:122-141)."""
    if "vel_norm_max" in z:
        return np.full(4, float(z["vel_norm_max"])), np.zeros(4)
    lo, hi = z["min_feats"].astype(np.float64), z["max_feats"].astype(np.float64)
    return (hi - lo) / 2.0, (hi - lo) / 2.0 + lo


VARIANTS = [(name, norm, strict) for name in ("minmax", "velnorm") for norm in (0, 1) for strict in (-1, 2)]


def tag(norm, strict):
    return f"n{norm}_s{'m1' if strict < 0 else strict}"


def close(a, ref, rel=1e-5):
    """The project bar: max|a - ref| <= rel * max|ref| over the finite entries, NaN positions equal."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if a.shape != ref.shape or not np.array_equal(np.isnan(a), np.isnan(ref)):
        return False, float("inf")
    ok = ~np.isnan(ref)
    if not ok.any():
        return True, 0.0
    err = float(np.abs(a[ok] - ref[ok]).max())
    return err <= rel * float(np.abs(ref[ok]).max()), err
