#!/usr/bin/env python3
"""Golden vectors of the 2D depth metrics: the REFERENCE's own ``calc_2d_depth_metrics`` and ``calc_2d_depth_metrics_batched``
(``mv3d/eval/metricfunctions.py:6-67``) executed on CPU torch from where they lie, through the import stand-ins of
_ref_import.py, on the seeded inputs of tests/metrics2d_oracle.py; around them the three stock calls of
``process_scene_2d_metrics`` (``mv3d/eval/processresults.py:160-165``: the float64 ground truth, ``F.interpolate(mode='nearest')``,
``valid = pred != 0 & ~isinf(pred)``).  Nothing of the reference's text is written to disk.

Run in the build container only:  python tests/golden/make_golden_metrics2d.py
Outputs tests/golden/M2d_*.npz (committed) -- data only.

Every fixture holds, for predictions ``pred`` [n, hp, wp] float32 and sensor depth ``gt_mm`` [n, H, W] uint16:
  batch        [9]  the reference on the whole batch with the derived mask (perc_valid, abs_rel, ..., d_125_3)
  batch_nomask [8]  the same without a mask (no perc_valid)
  rows      [n, 9]  the reference on every single image: per-image rows
  batched      [9]  calc_2d_depth_metrics_batched with ``batch_size`` (the scene's result)
The inputs of M2d_d (256 x 320 -> 480 x 640) are not stored: they are seeded (``metrics2d_oracle.scene``) and the fixture holds
their SHA-256.  Every reference output is asserted finite: no fixture rests on what the reference does with a masked non-finite
term.  Every fixture has at least a quarter of its pixels in the mask, one image with an empty mask and one with exactly one
pixel in it.

  M2d_a   n = 4,   6 x 8 -> 12 x 16,       batch_size 3
  M2d_b   n = 3,   33 x 130 (identity),    batch_size 100
  M2d_c   n = 101, 8 x 8 (identity),       batch_size 100 (weights 100 and 1)
  M2d_d   n = 3,   256 x 320 -> 480 x 640, batch_size 2
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import metrics2d_oracle as oracle  # noqa: E402

REF = _ref_import.reference().metrics
CASES = {'M2d_a': (4, 12, 16, 6, 8, 3, 21, True), 'M2d_b': (3, 33, 130, 33, 130, 100, 22, True),
         'M2d_c': (101, 8, 8, 8, 8, 100, 23, True), 'M2d_d': (3, 480, 640, 256, 320, 2, 24, False)}
BUDGET = 500 * 1024           # all M2d_* fixtures together


def row(d):
    assert list(d) == [k for k in oracle.COLUMNS if k in d]            # the reference's key order
    v = np.array([d[k] for k in d], dtype=np.float64)
    assert np.all(np.isfinite(v)), d
    return v


def case(name, n, H, W, hp, wp, batch_size, seed, store):
    pred_np, gt_mm = oracle.scene(n, H, W, hp, wp, seed)
    with torch.no_grad():
        depth_gt = torch.from_numpy(gt_mm.astype(float) / 1000.)                                  # load_gt_depth, :55
        depth_preds = torch.from_numpy(pred_np)
        lg = F.interpolate(depth_preds.unsqueeze(1), depth_gt.shape[-2:], mode='nearest').squeeze(1)    # :162
        valid = (lg != 0.) & (~torch.isinf(lg))                                                   # :163
        batch = row(REF.calc_2d_depth_metrics(lg, depth_gt, valid, True))
        nomask = row(REF.calc_2d_depth_metrics(lg, depth_gt, None, True))
        rows = np.stack([row(REF.calc_2d_depth_metrics(lg[i:i + 1], depth_gt[i:i + 1], valid[i:i + 1], True)) for i in range(n)])
        batched = row(REF.calc_2d_depth_metrics_batched(lg, depth_gt, pred_valid=valid, batch_size=batch_size))   # :164
    mask = valid.numpy() & (depth_gt.numpy() >= 0.5) & (depth_gt.numpy() < 65.)
    per = mask.reshape(n, -1).sum(1)
    assert mask.mean() >= 0.25, mask.mean()
    assert (per == 0).any() and (per == 1).any(), per
    arrays = dict(shape=np.asarray([n, H, W, hp, wp], dtype=np.int64), batch_size=np.int64(batch_size), seed=np.int64(seed),
                  pred_sha=np.str_(oracle.digest(pred_np)), gt_sha=np.str_(oracle.digest(gt_mm)), batch=batch, batch_nomask=nomask,
                  rows=rows, batched=batched, n_mask=per.astype(np.int64), n_pred_valid=valid.numpy().reshape(n, -1).sum(1))
    if store:
        arrays.update(pred=pred_np, gt_mm=gt_mm)
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%.1f KB): %.0f %% of the pixels in the mask, abs_rel %.6f' % (path, os.path.getsize(path) / 1024,
                                                                                  100 * mask.mean(), batched[1]))
    return os.path.getsize(path)


def main():
    total = sum(case(name, *args) for name, args in CASES.items())
    assert total <= BUDGET, total
    print('total %.1f KB' % (total / 1024))


if __name__ == '__main__':
    main()
