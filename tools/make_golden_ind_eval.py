#!/usr/bin/env python3
"""Golden fixtures of the inD runner's forward-prediction metric from the imported reference.

TEST INFRASTRUCTURE ONLY; needs the reference tree (AETHER_REFERENCE, default /root/reference).  Imported, unmodified:
``experiments/ind/evaluate.py::eval_forward_prediction_dynamicvars_unnormalized`` (:6-82), run on the CPU with a stub
model whose ``predict_future`` returns recorded predictions and a stub data set of five scenes (no inD files: the
recordings are licensed).  The stub data set builds its burn-in masks with the loop of
experiments/ind/single_ind_data.py:73-81 and un-normalises as :122-141 does, with the statistics as tensors.

Five scenes, padded 9 frames x 6 object rows (scene 3 is 7 x 4), ``max_burn_in_count`` 3.  Tracks: present throughout;
leaving early; never present; entering late (with ``strict`` 2 they have no burn-in entry and are skipped); one with a gap
after its burn-in (the reference's bad count).  Every frame has two or more present objects, so the scenes also run
through the model.  Writes

  ind_eval_minmax.npz    statistics (min_feats, max_feats)
  ind_eval_velnorm.npz   statistics vel_norm_max; the data set has ``non_linear_masks``

each with inputs, masks, burn-in masks, predictions and, for report_error_norm in (0, 1) x strict in (-1, 2), the four
results and the bad count (keys ``errors_n{0,1}_s{m1,2}`` ...).  Reruns reproduce the files bit for bit.

Usage:  python tools/make_golden_ind_eval.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import contextlib
import importlib.util
import io
import os
import re

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("AETHER_REFERENCE", "/root/reference")
SEED, MAX_BURN_IN = 4711, 3
T, N = 9, 6

# presence per scene: rows = objects, (first frame, last frame + 1) spans; [] = never present
SCENES = [
    (9, 6, [[(0, 9)], [(0, 9)], [(0, 6)], [], [(4, 9)], [(0, 5), (6, 9)]]),
    (9, 6, [[(0, 9)], [(0, 9)], [(2, 9)], [(0, 4)], [], [(3, 8)]]),
    (9, 6, [[(0, 7)], [(0, 9)], [(1, 9)], [(0, 3), (5, 9)], [(0, 9)], []]),
    (7, 4, [[(0, 7)], [(0, 7)], [(3, 7)], [(0, 5)]]),
    (9, 6, [[(0, 9)], [(1, 9)], [(0, 9)], [(5, 9)], [(0, 2)], [(2, 6)]]),
]
NON_LINEAR = [[1, 1, 1, 1, 1, 1], [1, 0, 1, 1, 1, 1], [0, 1, 1, 1, 1, 1], [1, 1, 0, 1], [1, 1, 1, 1, 1, 0]]


def reference_eval():
    spec = importlib.util.spec_from_file_location("ind_reference_evaluate", os.path.join(REF, "experiments", "ind", "evaluate.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.eval_forward_prediction_dynamicvars_unnormalized


class StubData(torch.utils.data.Dataset):
    def __init__(self, feats, masks, stats, non_linear_masks=None):
        self.feats, self.masks, self.stats = feats, masks, stats
        self.vel_norm_norm = not isinstance(stats, tuple)
        if non_linear_masks is not None:
            self.non_linear_masks = non_linear_masks
        self.burn_in_masks = []
        for mask in masks:                                             # single_ind_data.py:73-81
            burn_in_mask = torch.zeros_like(mask, dtype=torch.float32)
            burn_in_count = torch.zeros(mask.size(1), dtype=torch.float32)
            for step in range(len(mask)):
                burn_in_mask[step] = (mask[step] == 1).float() * (burn_in_count < MAX_BURN_IN).float()
                burn_in_count += burn_in_mask[step]
            self.burn_in_masks.append(burn_in_mask)

    def unnormalize_data(self, feats):                                 # single_ind_data.py:122-141
        if self.vel_norm_norm:
            return feats * self.stats
        min_feats, max_feats = (s.view(1, 1, -1) for s in self.stats)
        return torch.cat([(feats[i] + 1) * (max_feats - min_feats) / 2.0 + min_feats for i in range(len(feats))])

    def __len__(self):
        return len(self.feats)

    def __getitem__(self, i):
        return {"inputs": self.feats[i], "masks": self.masks[i], "burn_in_masks": self.burn_in_masks[i].clone()}


class StubModel(torch.nn.Module):
    def __init__(self, preds):
        super().__init__()
        self.preds, self.calls = preds, 0

    def predict_future(self, inputs, masks, node_inds, graph_info, burn_in_masks):
        out = self.preds[self.calls][None]
        self.calls += 1
        return out


def scenes():
    g = torch.Generator().manual_seed(SEED)
    feats, masks, preds = [], [], []
    for t_s, n_s, rows in SCENES:
        m = torch.zeros(t_s, n_s)
        for j, spans in enumerate(rows):
            for lo, hi in spans:
                m[lo:hi, j] = 1
        assert all(int(c) == 0 or int(c) >= 2 for c in m.sum(1)), "every frame needs 0 or >= 2 present objects"
        x = 0.5 * torch.randn(t_s, n_s, 4, generator=g)
        feats.append(x)
        masks.append(m)
        preds.append(x[1:] + 0.1 * torch.randn(t_s - 1, n_s, 4, generator=g))
    return feats, masks, preds


def pad(ts, width):
    out = torch.zeros(len(ts), *width)
    for i, t in enumerate(ts):
        out[(i,) + tuple(slice(0, s) for s in t.shape)] = t
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden"))
    args = ap.parse_args()
    ref = reference_eval()
    feats, masks, preds = scenes()
    modes = {"minmax": (torch.tensor([-30.0, -20.0, -6.0, -5.0]), torch.tensor([40.0, 25.0, 7.0, 4.0])),
             "velnorm": torch.tensor(7.5)}
    for name, stats in modes.items():
        nl = [torch.tensor(r) for r in NON_LINEAR] if name == "velnorm" else None
        data = StubData(feats, masks, stats, nl)
        out = dict(inputs=pad(feats, (T, N, 4)).numpy(), masks=pad(masks, (T, N)).numpy(),
                   burn_in_masks=pad(data.burn_in_masks, (T, N)).numpy(), preds=pad(preds, (T - 1, N, 4)).numpy(),
                   shapes=np.array([(t_s, n_s) for t_s, n_s, _ in SCENES], dtype=np.int64),
                   max_burn_in_count=np.int64(MAX_BURN_IN))
        if name == "minmax":
            out["min_feats"], out["max_feats"] = stats[0].numpy(), stats[1].numpy()
        else:
            out["vel_norm_max"] = stats.numpy()
            out["non_linear_masks"] = pad([r.float() for r in nl], (N,)).numpy()
        for norm in (0, 1):
            for strict in (-1, 2):
                buf = io.StringIO()
                with contextlib.redirect_stdout(buf):
                    res = ref(StubModel(preds), data, {"report_error_norm": bool(norm), "strict": strict})
                bad = int(re.search(r"FINAL BAD COUNT:\s+(\d+)", buf.getvalue()).group(1))
                tag = f"n{norm}_s{'m1' if strict < 0 else strict}"
                for key, val in zip(("errors", "pos_errors", "vel_errors", "counts"), res):
                    out[f"{key}_{tag}"] = val.numpy()
                out[f"bad_count_{tag}"] = np.int64(bad)
        path = os.path.join(args.out, f"ind_eval_{name}.npz")
        np.savez(path, **out)
        print(path, {k: v.shape for k, v in out.items() if k.startswith("errors")}, [int(out[k]) for k in out if k.startswith("bad")])


if __name__ == "__main__":
    main()
