"""Depth supervision on the device: the reference's ``MAELoss`` (``mv3d/loss.py:6-20``) and, in the same pass, the 2D depth metrics
that ``PL3DVNet.forward`` takes beside it at every supervised depth map (``mv3d/lightningmodel.py:57-119``:
``calc_2d_depth_metrics`` without a mask against the ground truth reduced to the prediction's size).  The arithmetic is
``csrc/supervision.hip`` (on ``csrc/depth2d.h``, which it shares with the 2D metrics) behind ``v3d_depth_supervision_f32``
(include/v3d.h states the rule): one pass over the prediction, the ground truth gathered through the index tables of the nearest
resize, no temporary.  This module is the plumbing:

  * ``supervise``   device tensors in, a record of device tensors out (counts, per-image rows, mean; ``mean[9]`` is the loss);
  * ``MAELoss``     the reference's module and ``forward`` signature -> the loss as a 0-dim float64 device tensor.

There is no backward pass and no CPU fallback: without the library or a HIP device every computing entry raises
``V3DLibraryError``.
"""
import collections

import torch
import torch.nn as nn

from . import _lib, metrics2d

COLUMNS = metrics2d.COLUMNS + ('loss_2d',)                   # per_image, mean
COUNTS = metrics2d.COUNTS + ('n_loss',)
METRIC_KEYS = metrics2d.COLUMNS[1:]                          # calc_2d_depth_metrics without a mask, in its order
LOSS = COLUMNS.index('loss_2d')
Supervision = collections.namedtuple('Supervision', ('counts', 'per_image', 'mean'))
resize_tables = metrics2d.resize_tables      # (src_h, src_w, dst_h, dst_w, device): here the source is the ground truth


def supervise(depth_pred, depth_gt, depth_interval):
    """depth_pred [n, h, w] fp32, depth_gt [n, H, W] fp32 metres, both on a HIP device -> ``Supervision(counts [n, 6] int32,
    per_image [n, 10] float64, mean [10] float64)`` on that device (columns: ``COUNTS``, ``COLUMNS``).  Ground truth of another
    size is read through the index tables of ``F.interpolate(mode='nearest')``, as the reference reduces it.  Reads nothing back."""
    lib = _lib.load()
    dev = metrics2d._on_device(depth_pred, 'supervise')
    metrics2d._on_device(depth_gt, 'supervise(depth_gt)')
    if depth_pred.dim() != 3 or depth_gt.dim() != 3 or depth_pred.shape[0] != depth_gt.shape[0] or depth_pred.shape[0] == 0:
        raise ValueError('supervise: [n, h, w] and [n, H, W] with n > 0 expected, got %s and %s'
                         % (tuple(depth_pred.shape), tuple(depth_gt.shape)))
    if depth_pred.dtype != torch.float32 or depth_gt.dtype != torch.float32:
        raise ValueError('supervise: fp32 predictions and ground truth expected, got %s and %s' % (depth_pred.dtype, depth_gt.dtype))
    depth_pred, depth_gt = depth_pred.contiguous(), depth_gt.contiguous()
    n, h, w = depth_pred.shape
    H, W = depth_gt.shape[1:]
    rows, cols = (None, None) if (H, W) == (h, w) else resize_tables(H, W, h, w, dev)
    counts = torch.empty((n, len(COUNTS)), dtype=torch.int32, device=dev)
    per_image = torch.empty((n, len(COLUMNS)), dtype=torch.float64, device=dev)
    mean = torch.empty(len(COLUMNS), dtype=torch.float64, device=dev)
    ws = torch.empty(max(int(lib.v3d_depth_supervision_workspace_bytes(n, h, w)), 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.v3d_depth_supervision_f32(depth_pred.data_ptr(), n, h, w, depth_gt.data_ptr(), H, W, _lib.ptr(rows),
                                                 _lib.ptr(cols), float(depth_interval), counts.data_ptr(), per_image.data_ptr(),
                                                 mean.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)),
                   'v3d_depth_supervision_f32')
    return Supervision(counts, per_image, mean)


def metrics_dict(sup):
    """The eight keys of the reference's ``calc_2d_depth_metrics`` without a mask, in its order, as 0-dim float64 device
    tensors (views of ``sup.mean``)."""
    return {k: sup.mean[COLUMNS.index(k)] for k in METRIC_KEYS}


class MAELoss(nn.Module):
    """Reference ``MAELoss`` (loss.py:6-20): the mean over the images of ``(sum |pred - gt| over gt != 0) / depth_interval /
    (count + 1e-7)``, the ground truth reduced to the prediction's size when the shapes differ.  -> 0-dim float64 device tensor."""

    def forward(self, pred_depth_image, gt_depth_image, depth_interval):
        return supervise(pred_depth_image, gt_depth_image, depth_interval).mean[LOSS]
