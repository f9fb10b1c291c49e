"""3D metrics of a fused point cloud on the device: what the reference does with the cloud after fusion
(``mv3d/eval/processresults.py:283-295``, ``mv3d/eval/metricfunctions.py:70-124``) -- ``voxel_down_sample`` of the
predicted and the ground-truth cloud, ``nn_correspondance`` in both directions, ``eval_mesh``.  The arithmetic is
``csrc/cloudmetrics.hip`` behind ``v3d_cloud_downsample_f32`` / ``v3d_nn_query_f32`` / ``v3d_cloud_metrics_f64``; this
module is the plumbing:

  * ``voxel_down_sample`` / ``nearest_neighbors`` / ``eval_clouds``   device tensors in, device tensors out;
  * ``nn_correspondance`` / ``eval_mesh``   the reference's names, argument order and return values (arrays, tensors or
                                            any object with ``.points``);
  * ``depth_3d_metrics``                    a ``preds.npz`` record + ground-truth points -> the metrics dict, without the
                                            points leaving the device.

The down-sample restates Open3D's documented ``VoxelDownSample`` (not pinned against the package).  Output
order is ascending cell key x 2^42 + y 2^21 + z (Open3D's is hash-map order).

There is no CPU fallback: without the library or a HIP device every computing entry raises ``V3DLibraryError``.
"""
import ctypes

import numpy as np
import torch

from . import _lib, fusion, meshtodepth

KEYS = ('acc', 'comp', 'prec', 'recal', 'fscore')
_STATUS = {1: 'the cloud holds a non-finite coordinate', 2: 'extent / voxel_size reaches 2^21 cells on an axis',
           4: 'voxel_size must be positive and finite'}


def _device_of(t, what):
    if not torch.cuda.is_available() or not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.V3DLibraryError('%s: tensors must live on a HIP device (no CPU fallback)' % what)
    return t.device


def _cloud(t, what):
    if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
        raise ValueError('%s: fp32 [n, 3] expected, got %s %s' % (what, t.dtype, tuple(t.shape)))
    return t.contiguous()


def _workspace(nbytes, dev):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


def _raise_status(code):
    raise _lib.V3DLibraryError('voxel_down_sample failed: ' + '; '.join(m for b, m in _STATUS.items() if code & b))


def voxel_down_sample(pts, voxel_size, attr=None, count=None, trim=False):
    """pts [n, 3] fp32 (and attr [n, k] fp32, e.g. colours) on a HIP device -> ``(out_pts, out_attr | None, out_count)``:
    one row per occupied cell of edge ``voxel_size`` = the double-precision mean of its member rows (original row order)
    rounded once to fp32, in ascending cell-key order; ``out_count`` is their number as a device int32 word.  ``count``
    (a device int32 word, e.g. the one ``fusion.fuse_depth_maps(trim=False)`` returns) limits the input to its first rows.
    ``trim=False`` reads nothing back: the outputs hold n rows (rows >= out_count are unspecified) and an error shows as a
    NEGATIVE out_count; ``trim=True`` reads status and count back once, raises on an error and returns out_count rows."""
    lib = _lib.load()
    dev = _device_of(pts, 'voxel_down_sample')
    pts = _cloud(pts, 'voxel_down_sample')
    n = pts.shape[0]
    k = 0
    if attr is not None:
        _device_of(attr, 'voxel_down_sample(attr)')
        if attr.dim() != 2 or attr.shape[0] != n or attr.dtype != torch.float32:
            raise ValueError('voxel_down_sample: attr must be fp32 [n, k], got %s %s' % (attr.dtype, tuple(attr.shape)))
        attr = attr.contiguous()
        k = int(attr.shape[1])
    if count is not None:
        _device_of(count, 'voxel_down_sample(count)')
        if count.dtype != torch.int32 or count.numel() != 1:
            raise ValueError('voxel_down_sample: count must be one int32 word on the device')
    ws_bytes = int(lib.v3d_cloud_downsample_workspace_bytes(n))
    ws = _workspace(ws_bytes, dev)
    out_pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    out_attr = None if attr is None else torch.empty((n, k), dtype=torch.float32, device=dev)
    out_count = torch.empty((), dtype=torch.int32, device=dev)
    stream = _lib.stream_ptr(dev)
    with torch.cuda.device(dev):
        _lib.check(lib.v3d_cloud_downsample_f32(pts.data_ptr(), _lib.ptr(attr), k, n, _lib.ptr(count), float(voxel_size),
                                                out_pts.data_ptr(), _lib.ptr(out_attr), out_count.data_ptr(), ws.data_ptr(),
                                                ws.numel(), stream), 'v3d_cloud_downsample_f32')
        if trim:
            m = ctypes.c_int(0)
            _lib.check(lib.v3d_cloud_status(ws.data_ptr(), ws.numel(), ctypes.byref(m), stream), 'v3d_cloud_status')
            out_pts, out_attr = out_pts[:m.value], (None if out_attr is None else out_attr[:m.value])
    return out_pts, out_attr, out_count


def nearest_neighbors(target, query):
    """For every row of ``query`` [m, 3] its nearest row of ``target`` [n, 3] (fp32, HIP device) -> ``(idx [m] int32, dist
    [m] fp32)``: the index in the target's own row order and the fp32 Euclidean distance.  Exact; among equal fp32
    distances the lowest index wins.  An empty target gives idx -1, dist inf."""
    lib = _lib.load()
    dev = _device_of(target, 'nearest_neighbors')
    _device_of(query, 'nearest_neighbors')
    target, query = _cloud(target, 'nearest_neighbors(target)'), _cloud(query, 'nearest_neighbors(query)')
    n, m = target.shape[0], query.shape[0]
    idx = torch.empty(m, dtype=torch.int32, device=dev)
    dist = torch.empty(m, dtype=torch.float32, device=dev)
    ws = _workspace(lib.v3d_nn_workspace_bytes(n, m), dev)
    with torch.cuda.device(dev):
        _lib.check(lib.v3d_nn_query_f32(target.data_ptr(), n, query.data_ptr(), m, idx.data_ptr(), dist.data_ptr(),
                                        ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)), 'v3d_nn_query_f32')
    return idx, dist


def cloud_metrics(dist_pred, dist_target, threshold):
    """Distances pred -> target and target -> pred (fp32, device) -> the [5] float64 device record (acc, comp, prec,
    recal, fscore)."""
    lib = _lib.load()
    dev = _device_of(dist_pred, 'cloud_metrics')
    _device_of(dist_target, 'cloud_metrics')
    if dist_pred.dtype != torch.float32 or dist_target.dtype != torch.float32:
        raise ValueError('cloud_metrics: fp32 distances expected')
    dist_pred, dist_target = dist_pred.contiguous().reshape(-1), dist_target.contiguous().reshape(-1)
    out = torch.empty(5, dtype=torch.float64, device=dev)
    ws = _workspace(lib.v3d_cloud_metrics_workspace_bytes(), dev)
    with torch.cuda.device(dev):
        _lib.check(lib.v3d_cloud_metrics_f64(dist_pred.data_ptr(), dist_pred.numel(), dist_target.data_ptr(),
                                             dist_target.numel(), float(threshold), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                             _lib.stream_ptr(dev)), 'v3d_cloud_metrics_f64')
    return out


def eval_clouds(pred, target, threshold=.05):
    """Predicted and target cloud (fp32 [n, 3], device) -> the [5] float64 device record (acc, comp, prec, recal, fscore).
    Reads nothing back."""
    _, d_pred = nearest_neighbors(target, pred)           # metricfunctions.py:84: dist1, per predicted vertex
    _, d_trgt = nearest_neighbors(pred, target)           # :85: dist2, per target vertex
    return cloud_metrics(d_pred, d_trgt, threshold)


def _points(pcd):
    """Array, tensor or any object with ``.points`` -> fp32 [n, 3] tensor (where it lives)."""
    p = pcd.points if hasattr(pcd, 'points') else pcd
    if not torch.is_tensor(p):
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(p, dtype=np.float32)).reshape(-1, 3))
    return p.float().reshape(-1, 3)


def _to_device(p, device):
    if p.is_cuda:
        return p
    if not torch.cuda.is_available():
        raise _lib.V3DLibraryError('3D metrics need a HIP device (no CPU fallback)')
    return p.to(fusion._device(device))


def nn_correspondance(pcd1, pcd2, device=None):
    """The reference's ``nn_correspondance`` (metricfunctions.py:102-124): for each vertex of ``pcd2`` its nearest vertex
    of ``pcd1`` -> ``(indices, distances)`` lists; empty lists when either cloud is empty."""
    p1, p2 = _points(pcd1), _points(pcd2)
    if p1.shape[0] == 0 or p2.shape[0] == 0:
        return [], []
    _lib.load()
    idx, dist = nearest_neighbors(_to_device(p1, device), _to_device(p2, device))
    return idx.cpu().tolist(), dist.cpu().tolist()


def eval_mesh(pcd_pred, pcd_trgt, threshold=.05, device=None):
    """The reference's ``eval_mesh`` (metricfunctions.py:70-99) -> dict of Python floats with its five keys.  An empty
    cloud gives what NumPy gives the reference for empty arrays (nan); no kernel is launched then."""
    pred, trgt = _points(pcd_pred), _points(pcd_trgt)
    if pred.shape[0] == 0 or trgt.shape[0] == 0:
        return {k: float('nan') for k in KEYS}
    _lib.load()
    rec = eval_clouds(_to_device(pred, device), _to_device(trgt, device), threshold)
    return dict(zip(KEYS, rec.cpu().tolist()))


def depth_3d_metrics(preds, images, gt_points, z_thresh, n_consistent_thresh=3, voxel_downsample=0.02, dist_thresh=0.05,
                     out_size=None, device=None, gt_mesh=None):
    """The chain of processresults.py:218-291 without files or fusibile: ``fusion.prepare_preds`` (-> with ``gt_mesh``, the
    depths zeroed where that mesh, rendered from the same cameras at the fused size, is not seen: :262-266) ->
    ``fuse_depth_maps(trim=False)`` -> down-sample of the fused cloud (colours / 255 as attributes) and of ``gt_points``
    -> nearest neighbours in both directions -> metrics.  ``preds`` is a ``preds.npz`` path or mapping, ``images``
    [N, H, W, 3] at the fused size, ``gt_points`` [n, 3].  -> dict of the five metrics and ``'n'`` (the number of views).

    The points never leave the device.  Read-backs: 3 -- the two down-sampled counts (4 bytes each, they size the
    neighbour searches) and the final 40-byte record; with ``gt_mesh`` the renderer's status word as well."""
    _lib.load()
    dev = fusion._device(device)
    depths, poses, K = fusion.prepare_preds(preds, out_size)
    images = torch.as_tensor(images).to(dev)
    depths = torch.from_numpy(depths).to(dev)
    if gt_mesh is not None:
        depths = meshtodepth.mask_with_mesh(depths, gt_mesh, poses, K, device=dev)
    pts, rgb, _, count = fusion.fuse_depth_maps(depths, torch.from_numpy(poses),
                                                torch.from_numpy(K), images, z_thresh, n_consistent_thresh, trim=False)
    pred, _, n_pred = voxel_down_sample(pts, voxel_downsample, attr=rgb.float() / 255., count=count)
    gt = _to_device(_points(gt_points), dev)
    trgt, _, n_trgt = voxel_down_sample(gt, voxel_downsample)
    n_pred, n_trgt = int(n_pred.item()), int(n_trgt.item())
    for c in (n_pred, n_trgt):
        if c < 0:
            _raise_status(-c)
    out = {k: float('nan') for k in KEYS}
    if n_pred > 0 and n_trgt > 0:
        out = dict(zip(KEYS, eval_clouds(pred[:n_pred], trgt[:n_trgt], dist_thresh).cpu().tolist()))
    out['n'] = int(depths.shape[0])
    return out
