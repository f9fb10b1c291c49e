#!/usr/bin/env python3
"""Golden vectors of the depth supervision: the REFERENCE's own ``MAELoss.forward`` (``mv3d/loss.py:6-20``) and
``calc_2d_depth_metrics`` (``mv3d/eval/metricfunctions.py:26-67``) executed on CPU torch from where they lie, through the import
stand-ins of _ref_import.py, on the seeded inputs of tests/supervision_oracle.py, the way ``PL3DVNet.forward`` reaches them
(``mv3d/lightningmodel.py:58-60``): the ground truth first reduced to the prediction's size with ``F.interpolate(mode='nearest')``.
Nothing of the reference's text is written to disk.

Run in the build container only:  python tests/golden/make_golden_supervision.py
Outputs tests/golden/S_sup_*.npz (committed) -- data only.

Every case is run twice:
  ref32   on the fp32 tensors, the reference's own types;
  ref64   with the ground truth widened to float64.  The prediction stays the float32 tensor it is in the reference (torch
          promotes it wherever it meets the ground truth; ``1. / depth_pred`` is its one fp32 operation, as include/v3d.h pins it),
          and the interval is the fp32 number the reference's fp32 division sees, widened.
Every fixture holds, for predictions ``pred`` [n, h, w] and ground truth ``gt`` [n, H, W], both float32, nine columns (the eight
keys of calc_2d_depth_metrics without a mask in its order, then the loss):
  ref32_batch, ref64_batch  [9]     the reference on the whole batch
  ref32_rows, ref64_rows    [n, 9]  the reference on every single image
  n_mask, n_loss            [n]     pixels in the metrics' mask (0.5 <= gt < 65) and in the loss's (gt != 0)
Inputs of more than 4 KB are not stored: they are seeded (``supervision_oracle.scene``) and the fixture holds their SHA-256.
Every reference output is asserted finite.  Every fixture has at least a quarter of its pixels in the metrics' mask, one image
with no ground truth at all, one with exactly one valid pixel, pixels with 0 < gt < 0.5 and pixels with gt >= 65: the last two
kinds count in the loss and not in the metrics.

  S_sup_a   n = 4,   6 x 8 <- 12 x 16,        interval 0.05
  S_sup_b   n = 3,   7 x 5 (identity),        interval 0.6
  S_sup_c   n = 4,   96 x 100 <- 192 x 200,   interval 0.05
  S_sup_d   n = 257, 4 x 4 (identity),        interval 0.025
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
import supervision_oracle as oracle  # noqa: E402

REF = _ref_import.reference().metrics
from mv3d.loss import MAELoss  # noqa: E402  (the reference's, importable once the stand-ins are installed)

CASES = {'S_sup_a': (4, 12, 16, 6, 8, 0.05, 31), 'S_sup_b': (3, 7, 5, 7, 5, 0.6, 32),
         'S_sup_c': (4, 192, 200, 96, 100, 0.05, 33), 'S_sup_d': (257, 4, 4, 4, 4, 0.025, 34)}
BUDGET = 500 * 1024           # all S_sup_* fixtures together
STORE_BELOW = 4 * 1024        # bytes of pred + gt


def row(pred, gt, interval):
    """the reference on one batch -> [9] float64: the eight metrics in the reference's key order, then the loss"""
    d = REF.calc_2d_depth_metrics(pred, gt)
    assert tuple(d) == oracle.METRIC_KEYS                              # the reference's key order
    v = np.array([float(d[k]) for k in d] + [float(MAELoss()(pred, gt, interval))], dtype=np.float64)
    assert np.all(np.isfinite(v)), v
    return v


def case(name, n, H, W, h, w, interval, seed):
    pred_np, gt_np = oracle.scene(n, H, W, h, w, seed)
    with torch.no_grad():
        pred, gt = torch.from_numpy(pred_np), torch.from_numpy(gt_np)
        gt_sm = F.interpolate(gt.unsqueeze(1), pred.shape[-2:], mode='nearest').squeeze(1)        # lightningmodel.py:58
        assert np.array_equal(gt_sm.numpy(), oracle.reduce_gt(gt_np, h, w))
        gt64, interval64 = gt_sm.double(), float(np.float32(interval))
        ref32_batch, ref64_batch = row(pred, gt_sm, interval), row(pred, gt64, interval64)
        ref32_rows = np.stack([row(pred[i:i + 1], gt_sm[i:i + 1], interval) for i in range(n)])
        ref64_rows = np.stack([row(pred[i:i + 1], gt64[i:i + 1], interval64) for i in range(n)])
    g = gt_sm.numpy()
    mask = (g >= 0.5) & (g < 65.)
    n_mask, n_loss = mask.reshape(n, -1).sum(1), (g != 0).reshape(n, -1).sum(1)
    assert mask.mean() >= 0.25, mask.mean()
    assert (n_loss == 0).any(), n_loss                                 # an image with no ground truth at all
    assert ((n_mask == 1) & (n_loss == 1)).any(), (n_mask, n_loss)     # an image with exactly one valid pixel
    assert ((g > 0) & (g < 0.5)).any() and (g >= 65.).any()            # in the loss, not in the metrics
    arrays = dict(shape=np.asarray([n, H, W, h, w], dtype=np.int64), seed=np.int64(seed), interval=np.float64(interval),
                  pred_sha=np.str_(oracle.digest(pred_np)), gt_sha=np.str_(oracle.digest(gt_np)), ref32_batch=ref32_batch,
                  ref64_batch=ref64_batch, ref32_rows=ref32_rows, ref64_rows=ref64_rows, n_mask=n_mask.astype(np.int64),
                  n_loss=n_loss.astype(np.int64))
    if pred_np.nbytes + gt_np.nbytes <= STORE_BELOW:
        arrays.update(pred=pred_np, gt=gt_np)
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrays)
    print('wrote %s (%.1f KB): %.0f %% of the pixels in the metrics\' mask, %d in the loss only; loss %.6f (fp32) %.6f (fp64)'
          % (path, os.path.getsize(path) / 1024, 100 * mask.mean(), int(((g != 0) & ~mask).sum()), ref32_batch[8], ref64_batch[8]))
    return os.path.getsize(path)


def main():
    total = sum(case(name, *args) for name, args in CASES.items())
    assert total <= BUDGET, total
    print('total %.1f KB' % (total / 1024))


if __name__ == '__main__':
    main()
