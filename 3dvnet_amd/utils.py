"""Host-side mirror of the hot-path helpers of ``mv3d/utils.py``.

``voxelize`` runs in ``lib3dvnet_hip.so`` (csrc/voxelize.hip): bounding box, voxel ids, radix sort +
unique, inverse map and decode are device kernels that restate ``utils.voxelize`` literally -- including
the reference's mix of a ceil-based grid size for decoding (utils.py:41) with torch_cluster's trunc+1
cell counts for encoding (``torch_geometric.nn.voxel_grid`` is an un-vendored third-party call).
"""
import ctypes

import torch

from . import _lib


def slice_edges(edges, index_start, index_end, slice_dim=0):
    """Row H1 (utils.py:32-35): keep edge columns whose ``edges[slice_dim]`` is in [start, end)."""
    keep = (edges[slice_dim] >= index_start) & (edges[slice_dim] < index_end)
    return edges[:, keep]


def sort_unique_u64(keys):
    """Ascending unique values of an int64 key tensor (device) -> int64 tensor [n_unique]."""
    lib = _lib.load()
    dev, n = keys.device, keys.shape[0]
    out = torch.empty(n, dtype=torch.int64, device=dev)
    nbytes = lib.v3d_sort_unique_workspace_bytes(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cnt = ctypes.c_int(0)
    rc = lib.v3d_sort_unique_u64(keys.data_ptr(), n, out.data_ptr(), ctypes.byref(cnt), ws.data_ptr(), nbytes,
                                 _lib.stream_ptr(dev))
    _lib.check(rc, 'v3d_sort_unique_u64')
    return out[:cnt.value]


def voxelize(pts, pts_batch, edge_len):
    """Row B3 (utils.py:38-64): -> (anchor_pts [Nv,3] f32, anchor_idx3d [Nv,3] int32,
    anchor_batch [Nv] int64, anchor_pts_edges [2,Np] int64)."""
    if not pts.is_cuda:
        raise _lib.V3DLibraryError('voxelize: tensors must live on a HIP device (no CPU fallback)')
    lib = _lib.load()
    dev, n = pts.device, pts.shape[0]
    stream = _lib.stream_ptr(dev)
    pts = pts.contiguous().float()
    pts_batch = pts_batch.contiguous().long()
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    wbytes = lib.v3d_voxelize_workspace_bytes()
    ws = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.v3d_voxel_keys(pts.data_ptr(), pts_batch.data_ptr(), n, float(edge_len), keys.data_ptr(),
                                  ws.data_ptr(), wbytes, stream), 'v3d_voxel_keys')
    uniq = sort_unique_u64(keys)                                              # torch.unique (:48)
    # range checks of the fixed-size device tables (batch ids, cells per axis); the stream is already synchronised
    _lib.check(lib.v3d_voxelize_status(ws.data_ptr(), wbytes, stream), 'voxelize')
    nv = uniq.shape[0]
    inv = torch.empty(n, dtype=torch.int64, device=dev)
    _lib.check(lib.v3d_lower_bound_u64(uniq.data_ptr(), nv, keys.data_ptr(), n, inv.data_ptr(), stream),
               'v3d_lower_bound_u64')
    anchor_pts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    anchor_idx3d = torch.empty((nv, 3), dtype=torch.int32, device=dev)
    anchor_batch = torch.empty(nv, dtype=torch.int64, device=dev)
    _lib.check(lib.v3d_voxel_decode(uniq.data_ptr(), nv, float(edge_len), float(edge_len / 2.),
                                    anchor_pts.data_ptr(), anchor_idx3d.data_ptr(), anchor_batch.data_ptr(),
                                    ws.data_ptr(), wbytes, stream), 'v3d_voxel_decode')
    anchor_pts_edges = torch.stack((inv, torch.arange(n, dtype=torch.long, device=dev)), dim=0)
    return anchor_pts, anchor_idx3d, anchor_batch, anchor_pts_edges


def _confidence_call(name, vol, depth_map, depth_start, depth_interval):
    if not (vol.is_cuda and depth_map.is_cuda):
        raise _lib.V3DLibraryError('%s: tensors must live on a HIP device (no CPU fallback)' % name)
    if vol.dim() != 4 or depth_map.dim() != 3 or (vol.shape[0],) + tuple(vol.shape[2:]) != tuple(depth_map.shape):
        raise ValueError('%s: a volume [n, D, h, w] and a depth map [n, h, w] are required, got %s and %s'
                         % (name, tuple(vol.shape), tuple(depth_map.shape)))
    lib = _lib.load()
    dev = vol.device
    vol = vol.detach().contiguous().float()
    depth_map = depth_map.detach().to(dev).contiguous().float()
    n, D, h, w = vol.shape
    prob = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(_lib.ptr(vol), _lib.ptr(depth_map), float(depth_start), float(depth_interval), n, D, h, w,
                                _lib.ptr(prob), _lib.stream_ptr(dev))
    _lib.check(rc, name)
    return prob


def get_propability_map(cv, depth_map, depth_start, depth_interval):
    """utils.py:111-145 (the reference's name and spelling): ``cv`` [n, D, h, w] holds probabilities, ``depth_map`` [n, h, w]
    depths on the grid ``depth_start + i * depth_interval`` -> [n, h, w], the sum of the two entries of ``cv`` that bracket the
    depth (the same entry twice where floor and ceil meet: up to 2 p).  One gather kernel (include/v3d.h,
    v3d_probability_map_f32), bit-identical to the reference on fp32 tensors; device tensors only."""
    return _confidence_call('v3d_probability_map_f32', cv, depth_map, depth_start, depth_interval)


def confidence_from_logits(x_reg, depth_map, depth_start, depth_interval):
    """``get_propability_map(softmax(-x_reg, dim=1), depth_map, ...)`` without the probability volume: ``x_reg`` [n, D, h, w]
    is the regulariser's output (``regularize_depth(return_reg=True)``), ``depth_map`` [n, h, w] any depths -- for instance the
    refined stage-2 depths, scored under the initial distribution.  One kernel (include/v3d.h, v3d_confidence_logits_f32); for
    the soft-argmin's own depth it gives the bits of ``regularize_depth(return_prob=True)``."""
    return _confidence_call('v3d_confidence_logits_f32', x_reg, depth_map, depth_start, depth_interval)


def soft_argmin(x_reg, depth_vals, return_prob=False, depth_start=None, depth_interval=None):
    """The last step of the cost-volume path on a regularised volume the caller holds (``x_reg`` [n, D, h, w], ``depth_vals``
    [D]): depth [n, h, w] = sum_d depth_vals[d] softmax(-x_reg)[d], by the kernel ``regularize_depth`` ends with (include/v3d.h,
    v3d_soft_argmin_f32); ``return_prob`` -> ``(depth, prob)`` by the kernel that also writes the confidence of that depth on
    the grid ``depth_start + i * depth_interval``."""
    if not x_reg.is_cuda:
        raise _lib.V3DLibraryError('soft_argmin: tensors must live on a HIP device (no CPU fallback)')
    if return_prob and (depth_start is None or depth_interval is None):
        raise ValueError('soft_argmin(return_prob=True) needs depth_start and depth_interval')
    lib = _lib.load()
    dev = x_reg.device
    x_reg = x_reg.detach().contiguous().float()
    n, D, h, w = x_reg.shape
    depth_vals = depth_vals.to(device=dev, dtype=torch.float32).contiguous()
    if depth_vals.shape != (D,):
        raise ValueError('soft_argmin: depth_vals must be [%d], got %s' % (D, tuple(depth_vals.shape)))
    depth = torch.empty((n, h, w), dtype=torch.float32, device=dev)
    prob = torch.empty_like(depth) if return_prob else None
    with torch.cuda.device(dev):
        rc = lib.v3d_soft_argmin_f32(_lib.ptr(x_reg), _lib.ptr(depth_vals), float(depth_start or 0.), float(depth_interval or 0.),
                                     n, D, h, w, _lib.ptr(depth), _lib.ptr(prob), _lib.stream_ptr(dev))
    _lib.check(rc, 'v3d_soft_argmin_f32')
    return (depth, prob) if return_prob else depth
