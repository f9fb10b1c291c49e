"""2D depth metrics of predicted depth maps on the device: the reference's ``calc_2d_depth_metrics`` /
``calc_2d_depth_metrics_batched`` (``mv3d/eval/metricfunctions.py:6-67``) and ``process_scene_2d_metrics``
(``mv3d/eval/processresults.py:153-169``).  The arithmetic is ``csrc/depthmetrics.hip`` (on ``csrc/depth2d.h``, which it shares
with the depth supervision) behind ``v3d_depth_metrics_2d`` (include/v3d.h states the rule): one pass over the ground truth, the predictions gathered through the index tables of the
nearest resize, no temporary of the image size.  This module is the plumbing:

  * ``depth_metrics``                      device tensors in, a record of device tensors out (counts, per-image rows, mean);
  * ``calc_2d_depth_metrics`` / ``calc_2d_depth_metrics_batched``   the reference's names, arguments, keys and key order;
  * ``process_scene_2d_metrics``           a ``preds.npz`` record + ground-truth depth -> the dict of ``metrics_2d.json``;
  * ``per_image_metrics``                  the [N, 9] table of per-view values, which the reference does not have.

Where a masked pixel's term is not finite (an infinite prediction, a NaN ground truth) the reference returns NaN; this module
returns the metric over the valid pixels.

There is no CPU fallback: without the library or a HIP device every computing entry raises ``V3DLibraryError``.
"""
import collections
import json

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, fusion

COLUMNS = ('perc_valid', 'abs_rel', 'abs_diff', 'abs_inv', 'sq_rel', 'rmse', 'd_125', 'd_125_2', 'd_125_3')    # per_image, mean
COUNTS = ('n_pred_valid', 'n_mask', 'c_125', 'c_125_2', 'c_125_3')
DepthMetrics = collections.namedtuple('DepthMetrics', ('counts', 'per_image', 'mean'))
_GT_TYPES = {torch.uint16: 0, torch.int16: 0, torch.float32: 1, torch.float64: 2}       # int16: the bits of a uint16
_tables = {}


def nearest_index(in_size, out_size):
    """Host int32 [out_size]: the source index ``F.interpolate(mode='nearest')`` reads for every output index -- by running
    it on an ``arange``, so it is torch's own rule by construction."""
    src = torch.arange(in_size, dtype=torch.float32).view(1, 1, in_size, 1)
    return F.interpolate(src, (out_size, 1), mode='nearest').view(-1).to(torch.int32)


def resize_tables(src_h, src_w, dst_h, dst_w, device):
    """(row_src [dst_h], col_src [dst_w]) int32 on ``device``: the row / column of a src_h x src_w image that
    ``F.interpolate(image, (dst_h, dst_w), mode='nearest')`` reads for every row / column of its result; cached.  The metrics
    read an hp x wp prediction on the ground truth's H x W grid with them, the supervision (``loss.resize_tables`` is this
    function) H x W ground truth on the prediction's h x w grid."""
    key = (src_h, src_w, dst_h, dst_w, str(device))
    if key not in _tables:
        _tables[key] = (nearest_index(src_h, dst_h).to(device), nearest_index(src_w, dst_w).to(device))
    return _tables[key]


def _on_device(t, what):
    if not torch.cuda.is_available() or not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.V3DLibraryError('%s: tensors must live on a HIP device (no CPU fallback)' % what)
    return t.device


def depth_metrics(depth_pred, depth_gt, pred_valid=None, derive_valid=False):
    """depth_pred [n, hp, wp] fp32, depth_gt [n, H, W] uint16 millimetres (or int16 holding those bits), fp32 or fp64 metres,
    both on a HIP device -> ``DepthMetrics(counts [n, 5] int32, per_image [n, 9] float64, mean [9] float64)`` on that device
    (columns: ``COUNTS``, ``COLUMNS``).  A prediction of another size is scored through the index tables of
    ``F.interpolate(mode='nearest')``.  ``pred_valid`` [n, H, W] (bool or uint8) is the reference's mask; ``derive_valid``
    derives it as ``pred != 0 & ~isinf(pred)`` inside the kernel instead.  Without either every prediction counts (and
    ``perc_valid`` is 1).  Reads nothing back."""
    lib = _lib.load()
    dev = _on_device(depth_pred, 'depth_metrics')
    _on_device(depth_gt, 'depth_metrics(depth_gt)')
    if depth_pred.dim() != 3 or depth_gt.dim() != 3 or depth_pred.shape[0] != depth_gt.shape[0] or depth_pred.shape[0] == 0:
        raise ValueError('depth_metrics: [n, hp, wp] and [n, H, W] with n > 0 expected, got %s and %s'
                         % (tuple(depth_pred.shape), tuple(depth_gt.shape)))
    if depth_pred.dtype != torch.float32:
        raise ValueError('depth_metrics: fp32 predictions expected, got %s' % depth_pred.dtype)
    if depth_gt.dtype not in _GT_TYPES:
        raise ValueError('depth_metrics: ground truth must be uint16, fp32 or fp64, got %s' % depth_gt.dtype)
    if pred_valid is not None and derive_valid:
        raise ValueError('depth_metrics: pred_valid and derive_valid exclude each other')
    depth_pred, depth_gt = depth_pred.contiguous(), depth_gt.contiguous()
    n, hp, wp = depth_pred.shape
    H, W = depth_gt.shape[1:]
    mode = 2 if derive_valid else 0
    if pred_valid is not None:
        _on_device(pred_valid, 'depth_metrics(pred_valid)')
        if tuple(pred_valid.shape) != (n, H, W) or pred_valid.dtype not in (torch.bool, torch.uint8):
            raise ValueError('depth_metrics: pred_valid must be bool or uint8 %s, got %s %s'
                             % ((n, H, W), pred_valid.dtype, tuple(pred_valid.shape)))
        pred_valid = pred_valid.contiguous().view(torch.uint8)
        mode = 1
    rows, cols = (None, None) if (hp, wp) == (H, W) else resize_tables(hp, wp, H, W, dev)
    counts = torch.empty((n, 5), dtype=torch.int32, device=dev)
    per_image = torch.empty((n, 9), dtype=torch.float64, device=dev)
    mean = torch.empty(9, dtype=torch.float64, device=dev)
    ws = torch.empty(max(int(lib.v3d_depth_metrics_workspace_bytes(n, H, W)), 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.v3d_depth_metrics_2d(depth_pred.data_ptr(), hp, wp, _lib.ptr(rows), _lib.ptr(cols), depth_gt.data_ptr(),
                                            _GT_TYPES[depth_gt.dtype], _lib.ptr(pred_valid), mode, n, H, W, counts.data_ptr(),
                                            per_image.data_ptr(), mean.data_ptr(), ws.data_ptr(), ws.numel(),
                                            _lib.stream_ptr(dev)), 'v3d_depth_metrics_2d')
    return DepthMetrics(counts, per_image, mean)


def _keys(with_valid):
    return COLUMNS if with_valid else COLUMNS[1:]


def calc_2d_depth_metrics(depth_pred, depth_gt, pred_valid=None, convert_to_cpu=False):
    """The reference's ``calc_2d_depth_metrics`` (metricfunctions.py:26-67): its keys in its order (``perc_valid`` first, and
    only with a mask), as float64 device scalars, or Python floats with ``convert_to_cpu``."""
    mean = depth_metrics(depth_pred, depth_gt, pred_valid).mean
    with_valid = pred_valid is not None
    if convert_to_cpu:
        vals = mean.cpu().tolist()
        return {k: vals[COLUMNS.index(k)] for k in _keys(with_valid)}
    return {k: mean[COLUMNS.index(k)] for k in _keys(with_valid)}


def _batched(depth_pred, depth_gt, pred_valid, derive_valid, batch_size):
    """-> (records per batch, view counts per batch)"""
    n_imgs = depth_pred.shape[0]
    recs, n = [], []
    for start in range(0, n_imgs, batch_size):
        end = start + batch_size
        valid = None if pred_valid is None else pred_valid[start:end]
        recs.append(depth_metrics(depth_pred[start:end], depth_gt[start:end], valid, derive_valid))
        n.append(recs[-1].counts.shape[0])
    return recs, n


def _weighted(recs, n, with_valid):
    means = torch.stack([r.mean for r in recs]).cpu().numpy()             # the one read-back
    n_sum = float(np.sum(n))
    return {k: float(np.sum([n[j] * means[j, COLUMNS.index(k)] for j in range(len(n))]) / n_sum) for k in _keys(with_valid)}


def calc_2d_depth_metrics_batched(depth_pred, depth_gt, pred_valid=None, batch_size=100):
    """The reference's ``calc_2d_depth_metrics_batched`` (metricfunctions.py:6-23): batches of ``batch_size`` views, averaged
    with the batches' view counts as weights -> Python floats.  One read-back, of the batches' means."""
    recs, n = _batched(depth_pred, depth_gt, pred_valid, False, batch_size)
    return _weighted(recs, n, pred_valid is not None)


def _scene_tensors(preds, depth_gt, device):
    dev = fusion._device(device)
    _lib.load()
    if isinstance(preds, (str, bytes)) or hasattr(preds, '__fspath__'):
        with np.load(preds) as f:
            depth_preds = f['depth_preds']
    else:
        depth_preds = preds['depth_preds']
    if not torch.is_tensor(depth_preds):
        depth_preds = torch.from_numpy(np.ascontiguousarray(np.asarray(depth_preds, dtype=np.float32)))
    if not torch.is_tensor(depth_gt):
        depth_gt = torch.from_numpy(np.ascontiguousarray(depth_gt))
    return depth_preds.float().to(dev), depth_gt.to(dev)


def process_scene_2d_metrics(preds, depth_gt, batch_size=100, out_path=None, device=None):
    """The reference's ``process_scene_2d_metrics`` (processresults.py:153-169) without its files: ``preds`` is a
    ``preds.npz`` path or a mapping as ``results.write_preds`` writes it, ``depth_gt`` [N, H, W] the sensor depth as uint16
    millimetres, fp32 or fp64 metres, host or device.  The predictions are scored at the ground truth's size (nearest), valid
    where they are neither 0 nor infinite, in batches of ``batch_size`` views.  -> the dict of ``metrics_2d.json`` (the nine
    metrics as Python floats and ``'n'``), which ``results.average_metrics`` takes as it is; written to ``out_path`` when
    given."""
    depth_preds, depth_gt = _scene_tensors(preds, depth_gt, device)
    recs, n = _batched(depth_preds, depth_gt, None, True, batch_size)
    metrics = _weighted(recs, n, True)
    metrics['n'] = int(depth_preds.shape[0])
    if out_path is not None:
        with open(out_path, 'w') as f:
            json.dump(metrics, f)
    return metrics


def per_image_metrics(depth_pred, depth_gt, pred_valid=None, derive_valid=False, batch_size=100):
    """The per-view values behind the means -> ``(table [N, 9] float64 NumPy array, COLUMNS)``: what one looks at first when
    a scene scores badly.  Device tensors in; one read-back."""
    recs, _ = _batched(depth_pred, depth_gt, pred_valid, derive_valid, batch_size)
    return torch.cat([r.per_image for r in recs]).cpu().numpy(), COLUMNS
