"""TSDF integration on the device: the depth maps ``results.write_preds`` leaves behind -> a truncated signed distance
volume with weights and colours (``mv3d/eval/tsdf_atlas.py``: ``TSDFFusion`` :341-463, ``TSDF`` :70-159, driven by the
``run_tsdf`` branch of ``mv3d/eval/processresults.py:297-383``).  The arithmetic is ``csrc/tsdf.hip`` behind
``v3d_tsdf_integrate_f32`` / ``v3d_tsdf_normalize_f32``; this module is the plumbing around it:

  * ``TSDFFusion``           the reference's constructor, ``reset`` / ``integrate`` / ``get_tsdf``, plus ``integrate_batch``
                             (N views in one launch; the same bits as N ``integrate`` calls);
  * ``TSDF``                 the holder with ``to`` / ``save`` / ``load`` and the reference's npz keys;
  * ``projection_matrices``  K [R | t] (processresults.py:19-24);
  * ``volume_bounds``        the scene's volume from the quantiles of the back-projected depths (:324-357);
  * ``volume_bounds_device`` the same volume without the points ever leaving the device or existing in memory
                             (``csrc/order_stats.hip`` behind ``v3d_backproject_order_stats_f32``: exact order statistics by
                             radix selection; 52 bytes per batch come back); ``cloud_order_stats`` /
                             ``backproject_order_stats`` are the thin wrappers.  The drivers take ``bounds='device'``;
  * ``fuse_preds_tsdf``      from a ``preds.npz`` record (path or mapping) to the ``TSDF``;
  * ``TSDF.get_mesh``        the volume -> a ``mesh.TriangleMesh`` on the device (``csrc/mesh.hip``: marching cubes with the
                             project's own case table and the reference's rules around it, tsdf_atlas.py:161-253);
  * ``TSDF.transform``       the volume resampled onto another grid and / or through a 3 x 4 transform (``csrc/tsdf_resample.hip``
                             behind ``v3d_tsdf_resample_f32`` / ``v3d_volume_resample_nearest``; tsdf_atlas.py:255-338);
  * ``eval_tsdf``            the volume metric (``mv3d/baselines/atlas/evaluation.py:24-96``): the prediction aligned to the
                             target's grid by ``transform``, then ``l1`` / ``l1_ns``;
  * ``tsdf_mesh_metrics``    the rest of the ``run_tsdf`` branch (:383-397): mesh -> vertices -> down-sample -> 3D metrics;
  * ``trim_mesh``            a mesh cut down to what given cameras saw (:71-150): rendered into every view
                             (``meshtodepth``), the renderings integrated into a fresh volume, that volume meshed;
  * ``mesh_3d_metrics``      the body of ``process_volume_3d_metrics`` (:172-200): trim, down-sample, 3D metrics.

``gt_mesh`` / ``mask_mesh`` arguments are the reference's ``MASK_USING_GT_MESH`` switch: depths are zeroed where a rendering of
that mesh sees nothing (``meshtodepth.mask_with_mesh``).

There is no CPU fallback: without the library or a HIP device every integrating, meshing, rendering or resampling entry raises
``V3DLibraryError``.  The label volume is not provided; ``transform`` carries integer and bool volumes that
arrive through the constructor or ``load``.
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from . import fusion as _fusion
from . import mesh as _mesh
from . import meshtodepth as _meshtodepth
from . import metrics3d as _metrics3d


def projection_matrices(K, poses):
    """[N, 3, 3] intrinsics, [N, 4, 4] world->camera poses -> [N, 3, 4] projections K [R | t]: the batched product of K with
    a zero fourth column and the pose, as the reference forms it, on the tensors' device."""
    K, poses = torch.as_tensor(K), torch.as_tensor(poses)
    if K.dim() != 3 or K.shape[1:] != (3, 3) or poses.shape != (K.shape[0], 4, 4):
        raise ValueError('projection_matrices: K [N, 3, 3] and poses [N, 4, 4] expected, got %s and %s'
                         % (tuple(K.shape), tuple(poses.shape)))
    K4 = torch.cat((K, torch.zeros((K.shape[0], 3, 1), dtype=K.dtype, device=K.device)), dim=2)
    return torch.bmm(K4, poses.to(K))


def _backproject(depths, P):
    """[n, h, w] depths, [n, 3, 4] projections -> [n, h w, 3] world points: P4^-1 [x, y, 1, 1 / d] de-homogenised.  A zero
    depth gives NaN rows."""
    n, h, w = depths.shape
    ys, xs = torch.meshgrid(torch.arange(h).type_as(depths), torch.arange(w).type_as(depths), indexing='ij')
    pix = torch.stack((xs, ys, torch.ones_like(xs)), dim=0)[None].repeat(n, 1, 1, 1)
    pix = torch.cat((pix, 1. / depths.unsqueeze(1)), dim=1)
    last = torch.tensor([[0, 0, 0, 1]]).type_as(P)[None].repeat(n, 1, 1)
    P_inv = torch.cat((P, last), dim=1).inverse()
    X = torch.bmm(P_inv, pix.view(n, 4, h * w))
    return (X[:, :3] / X[:, 3:]).transpose(2, 1)


def volume_bounds(depths, K, poses, vol_prcnt=.995, vol_margin=1.5, vox_res=.04, img_batch=100):
    """The reference's bounds rule (processresults.py:324-357).  Per batch of ``img_batch`` views the depths are
    back-projected, rows with a NaN dropped, and the per-axis quantiles at ``1 - vol_prcnt`` / ``vol_prcnt`` (NumPy's linear
    rule on the fp32 values, on the host, as the reference takes them) widened by ``vol_margin``; an empty batch is skipped;
    across batches the lower bound is a running minimum and the upper a running maximum.  ``depths`` [N, h, w] may live on
    the host or a device (the back-projection runs where they live); K and poses are host tensors / arrays.
    -> ``(origin [3] fp32, vol_max [3] fp32, vol_dim list of 3 ints)``, ``vol_dim = int((vol_max - origin) / vox_res)``.
    Once per scene, not a hot path: stock torch ops and one host quantile per batch."""
    depths = torch.as_tensor(depths)
    K, poses = torch.as_tensor(K).float().cpu(), torch.as_tensor(poses).float().cpu()
    n = depths.shape[0]
    origin = vol_max = None
    for start in range(0, n, int(img_batch)):
        d = depths[start:start + img_batch].float()
        P = projection_matrices(K[start:start + img_batch], poses[start:start + img_batch]).to(d.device)
        pts = _backproject(d, P).reshape(-1, 3)
        pts = pts[~torch.any(torch.isnan(pts), dim=1)].cpu().numpy()
        if pts.shape[0] == 0:
            continue
        lo = torch.as_tensor(np.quantile(pts, 1 - vol_prcnt, axis=0) - vol_margin).float()
        hi = torch.as_tensor(np.quantile(pts, vol_prcnt, axis=0) + vol_margin).float()
        origin = lo if origin is None else torch.minimum(origin, lo)
        vol_max = hi if vol_max is None else torch.maximum(vol_max, hi)
    if origin is None:
        raise ValueError('volume_bounds: no depth map has a usable pixel')
    vol_dim = ((vol_max - origin) / vox_res).int().tolist()
    return origin, vol_max, vol_dim


def _order_stats_args(qs, what):
    qs = [float(q) for q in np.atleast_1d(np.asarray(qs, dtype=np.float64))]
    if not 1 <= len(qs) <= 4 or not all(0.0 <= q <= 1.0 for q in qs):
        raise ValueError('%s: one to four quantiles within [0, 1] expected, got %r' % (what, qs))
    return qs, (ctypes.c_double * len(qs))(*qs)


def _order_stats_out(lib, n_q, dev):
    return (torch.empty(1, dtype=torch.int32, device=dev), torch.empty((n_q, 3, 2), dtype=torch.float32, device=dev),
            torch.empty(int(lib.v3d_order_stats_workspace_bytes(n_q)), dtype=torch.uint8, device=dev))


def cloud_order_stats(pts, qs):
    """Exact order statistics of a device cloud ``pts`` [N, 3] fp32 for the quantiles ``qs`` (one to four values in [0, 1]) ->
    ``(count, stats)`` device tensors: ``count`` [1] int32 = the rows without a NaN, ``stats`` [len(qs), 3, 2] fp32 = per
    quantile and axis the ``lo``-th and ``hi``-th smallest coordinate of the kept rows, ``lo = clamp(floor(q (N - 1)), 0,
    N - 1)``, ``hi = min(lo + 1, N - 1)`` (float64), as exact input bit patterns; NaN when no row is kept.  Asynchronous: nothing
    is read back (include/v3d.h: v3d_cloud_order_stats_f32).  No CPU fallback."""
    lib = _lib.load()
    pts = torch.as_tensor(pts)
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.dtype != torch.float32:
        raise ValueError('cloud_order_stats: pts must be [N, 3] fp32, got %s %s' % (tuple(pts.shape), pts.dtype))
    qs, q_host = _order_stats_args(qs, 'cloud_order_stats')
    if not torch.cuda.is_available() or not pts.is_cuda:
        raise _lib.V3DLibraryError('cloud_order_stats: the cloud must live on a HIP device (no CPU fallback)')
    pts = pts.contiguous()
    with torch.cuda.device(pts.device):
        count, stats, ws = _order_stats_out(lib, len(qs), pts.device)
        _lib.check(lib.v3d_cloud_order_stats_f32(_lib.ptr(pts), int(pts.shape[0]), q_host, len(qs), _lib.ptr(count), _lib.ptr(stats),
                                                 _lib.ptr(ws), ws.numel(), _lib.stream_ptr(pts.device)), 'v3d_cloud_order_stats_f32')
    return count, stats


def backproject_order_stats(depths, proj_inv, qs):
    """``cloud_order_stats`` of the points that ``depths`` [n, h, w] fp32 (device) back-project to through the inverse 4 x 4
    projections ``proj_inv`` [n, 4, 4] fp32, without the points being stored: pixel (x, y) with depth d becomes
    ``Pi [x, y, 1, 1 / d]`` de-homogenised, in individually rounded fp32 operations (include/v3d.h:
    v3d_backproject_order_stats_f32 pins the order).  A zero or NaN depth gives a NaN row, which is dropped.
    -> ``(count, stats)`` device tensors.  No CPU fallback."""
    lib = _lib.load()
    depths, proj_inv = torch.as_tensor(depths), torch.as_tensor(proj_inv)
    if depths.dim() != 3 or depths.dtype != torch.float32 or tuple(proj_inv.shape) != (depths.shape[0], 4, 4):
        raise ValueError('backproject_order_stats: depths [n, h, w] fp32 and proj_inv [n, 4, 4] expected, got %s %s and %s'
                         % (tuple(depths.shape), depths.dtype, tuple(proj_inv.shape)))
    qs, q_host = _order_stats_args(qs, 'backproject_order_stats')
    if not torch.cuda.is_available() or not depths.is_cuda:
        raise _lib.V3DLibraryError('backproject_order_stats: the depths must live on a HIP device (no CPU fallback)')
    dev = depths.device
    depths = depths.contiguous()
    proj_inv = proj_inv.to(dev, torch.float32).contiguous()
    n, h, w = (int(v) for v in depths.shape)
    with torch.cuda.device(dev):
        count, stats, ws = _order_stats_out(lib, len(qs), dev)
        _lib.check(lib.v3d_backproject_order_stats_f32(_lib.ptr(depths), _lib.ptr(proj_inv), n, h, w, q_host, len(qs), _lib.ptr(count),
                                                       _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)),
                   'v3d_backproject_order_stats_f32')
    return count, stats


def inverse_projections(K, poses):
    """[N, 3, 3], [N, 4, 4] host tensors -> the [N, 4, 4] fp32 inverses of [K [R | t]; 0 0 0 1], on the host as the reference
    takes them."""
    P = projection_matrices(K, poses)
    last = torch.tensor([[0, 0, 0, 1]]).type_as(P)[None].repeat(P.shape[0], 1, 1)
    return torch.cat((P, last), dim=1).inverse()


def quantile_from_order_stats(count, pair, q):
    """The pinned finish of a quantile from its two order statistics: ``t = q (N - 1) - lo`` with ``lo = clamp(floor(q (N - 1)),
    0, N - 1)`` in float64, then ``float32(a + (b - a) t)`` evaluated in float64 (``a`` itself when ``a == b``)."""
    vi = float(q) * float(count - 1)
    lo = min(max(np.floor(vi), 0.0), float(count - 1))
    a, b = np.float64(pair[0]), np.float64(pair[1])
    if a == b:
        return np.float32(a)
    return np.float32(a + (b - a) * np.float64(vi - lo))


def volume_bounds_device(depths, K, poses, vol_prcnt=.995, vol_margin=1.5, vox_res=.04, img_batch=100):
    """``volume_bounds`` with the quantiles taken on the device (same signature, same return triple): per batch of
    ``img_batch`` views one ``backproject_order_stats`` at ``1 - vol_prcnt`` and ``vol_prcnt`` -- the points are back-projected
    in registers and never stored -- and, after every batch is enqueued, ONE read-back of ``n_batches x (count + 12 floats)``
    for the whole scene.  The projections and their 4 x 4 fp32 inverses are formed on the host, as the reference forms them.
    On the host, per batch, axis and quantile: ``quantile_from_order_stats``, then ``-/+ vol_margin`` and ``.float()`` as the
    host path; a batch without a point is skipped; running minimum / maximum across batches; ``ValueError`` when no batch has
    a point.

    The interpolation rule is pinned here and not delegated to ``np.quantile``: NumPy 2.2 computes the virtual index
    ``q (N - 1)`` in the array's dtype, float32 -- above 2^24 points that rounds the index itself, and on small inputs it moves
    the result by about 1e-6 relative.  The device path takes the index in float64 and does not inherit that artefact, so its
    bounds may differ from ``volume_bounds`` in the last bits (the back-projection's rounding order differs from
    ``torch.bmm``'s as well).  ``depths`` [N, h, w] must live on a HIP device; K and poses are host tensors / arrays.  No CPU
    fallback: ``V3DLibraryError`` without the library or a device."""
    _lib.load()
    depths = torch.as_tensor(depths)
    if not torch.cuda.is_available() or not depths.is_cuda:
        raise _lib.V3DLibraryError('volume_bounds_device: the depths must live on a HIP device (no CPU fallback)')
    K, poses = torch.as_tensor(K).float().cpu(), torch.as_tensor(poses).float().cpu()
    qs = (1 - vol_prcnt, vol_prcnt)
    step = int(img_batch)
    out = []
    for start in range(0, depths.shape[0], step):
        Pi = inverse_projections(K[start:start + step], poses[start:start + step])
        count, stats = backproject_order_stats(depths[start:start + step].float(), Pi, qs)
        out.append(torch.cat((count, stats.reshape(-1).view(torch.int32))))         # bit patterns: 13 words per batch
    rec = torch.stack(out).cpu() if out else torch.empty((0, 13), dtype=torch.int32)
    counts, stats = rec[:, 0].tolist(), rec[:, 1:].contiguous().view(torch.float32).reshape(-1, 2, 3, 2).numpy()
    origin = vol_max = None
    for n_kept, st in zip(counts, stats):
        if n_kept == 0:
            continue
        lo = np.array([quantile_from_order_stats(n_kept, st[0, a], qs[0]) for a in range(3)], dtype=np.float32)
        hi = np.array([quantile_from_order_stats(n_kept, st[1, a], qs[1]) for a in range(3)], dtype=np.float32)
        lo, hi = torch.as_tensor(lo - vol_margin).float(), torch.as_tensor(hi + vol_margin).float()
        origin = lo if origin is None else torch.minimum(origin, lo)
        vol_max = hi if vol_max is None else torch.maximum(vol_max, hi)
    if origin is None:
        raise ValueError('volume_bounds_device: no depth map has a usable pixel')
    vol_dim = ((vol_max - origin) / vox_res).int().tolist()
    return origin, vol_max, vol_dim


def _bounds_fn(bounds, what):
    if bounds == 'host':
        return volume_bounds
    if bounds == 'device':
        return volume_bounds_device
    raise ValueError("%s: bounds must be 'host' or 'device', got %r" % (what, bounds))


class TSDF:
    """Holder of a TSDF volume with its metadata (tsdf_atlas.py:70-159): ``voxel_size``, ``origin`` [1, 3], ``tsdf_vol``
    [nx, ny, nz], ``attribute_vols`` (``'weight'`` [nx, ny, nz], ``'color'`` [3, nx, ny, nz]) and ``attributes``.

    ``save`` writes the reference's npz keys: ``origin``, ``voxel_size``, ``tsdf`` and one key per attribute volume /
    attribute.  ``load`` reads them back the way the reference does, including its placement of ``weight`` (and
    ``tsdf_point_cloud``) under ``attributes`` rather than ``attribute_vols``.  ``get_mesh`` and ``transform`` run on the
    device."""

    def __init__(self, voxel_size, origin, tsdf_vol, attribute_vols=None, attributes=None):
        self.voxel_size = voxel_size
        self.origin = origin
        self.tsdf_vol = tsdf_vol
        self.attribute_vols = attribute_vols if attribute_vols is not None else {}
        self.attributes = attributes if attributes is not None else {}
        self.device = tsdf_vol.device

    def save(self, fname):
        data = {'origin': self.origin.cpu().numpy(), 'voxel_size': self.voxel_size,
                'tsdf': self.tsdf_vol.detach().cpu().numpy()}
        for key, value in self.attribute_vols.items():
            data[key] = value.detach().cpu().numpy()
        for key, value in self.attributes.items():
            data[key] = value.cpu().numpy()
        np.savez_compressed(fname, **data)

    @classmethod
    def load(cls, fname, voxel_types=None):
        """``voxel_types``: which volumes to load besides the tsdf (e.g. ``['color']``); None = all."""
        with np.load(fname) as data:
            voxel_size = data['voxel_size'].item()
            origin = torch.as_tensor(data['origin']).view(1, 3)
            tsdf_vol = torch.as_tensor(data['tsdf'])
            attribute_vols, attributes = {}, {}
            for key in ('weight', 'tsdf_point_cloud'):
                if key in data:
                    attributes[key] = torch.as_tensor(data[key])
            if 'color' in data and (voxel_types is None or 'color' in voxel_types):
                attribute_vols['color'] = torch.as_tensor(data['color'])
            if 'instance' in data and (voxel_types is None or 'instance' in voxel_types or 'semseg' in voxel_types):
                attribute_vols['instance'] = torch.as_tensor(data['instance'])
        return cls(voxel_size, origin, tsdf_vol, attribute_vols, attributes)

    def to(self, device):
        self.origin = self.origin.to(device)
        self.tsdf_vol = self.tsdf_vol.to(device)
        self.attribute_vols = {key: value.to(device) for key, value in self.attribute_vols.items()}
        self.attributes = {key: value.to(device) for key, value in self.attributes.items()}
        self.device = device
        return self

    def get_mesh(self, attribute='color'):
        """The reference's ``get_mesh`` (tsdf_atlas.py:161-253) -> ``mesh.TriangleMesh`` on the volume's device: values
        clamped to [-1, 1]; an empty mesh when the clamped minimum is >= 0 or the maximum <= 0; one vertex per sign-changing
        grid edge; vertices at a -1 / +1 crossing removed together with their triangles and the rest renumbered in order;
        ``attribute='color'`` with a colour volume: ``color[:, round(vertex)]`` clamped to [0, 255] as bytes in channel order
        [2, 1, 0] (without a colour volume the mesh has no colours, where the reference fails).  The triangulation is this
        project's.  ``attribute='instance'`` (the label colouring) is not provided."""
        if attribute == 'instance':
            raise NotImplementedError('TSDF.get_mesh: the instance colouring needs the label volume, which is not provided')
        color = self.attribute_vols.get('color') if attribute == 'color' else None
        verts, colors, tris = _mesh.extract(self.tsdf_vol, color, self.voxel_size, self.origin, _mesh.MODE_MESH)
        return _mesh.TriangleMesh(verts, tris, colors)

    def transform(self, transform=None, voxel_dim=None, origin=None, align_corners=False):
        """The reference's ``transform`` (tsdf_atlas.py:255-338) -> a new ``TSDF`` on the same device, resampled onto the
        grid ``voxel_dim`` (default: this volume's) at ``origin`` (default: this volume's), with the same voxel size.
        ``transform`` [3, 4] or [4, 4] (host or device; read to the host once as 12 floats; None = identity) maps the world
        coordinates of the new grid to those of this volume.  ``align_corners`` is ``grid_sample``'s, default False as in
        the reference (``eval_tsdf`` passes True, with which an integer shift does not interpolate).

        tsdf: the nearest value; where that has magnitude < 1 the trilinear one; 1 where the voxel lies outside this
        volume (some normalised coordinate of magnitude >= 1 -- which includes this volume's border layer).  fp32 attribute
        volumes [nx, ny, nz] / [C, nx, ny, nz]: trilinear with zero padding.  Every other dtype (integer labels, bool masks,
        float64): nearest with zero padding, the element copied in its own type -- equal to the reference's route through
        fp32 for |value| < 2^24, a stated deviation beyond.  Outside, ``'semseg'`` becomes -1 and ``'mask_outside'`` True.
        ``attributes`` is passed through as the same dict.  The result's ``origin`` is [1, 3] fp32; shapes are
        [nx, ny, nz] / [C, nx, ny, nz] without the reference's ``.squeeze()`` (a difference only when a size is 1).
        One launch for the tsdf together with the first fp32 attribute volume, one per other attribute volume
        (csrc/tsdf_resample.hip; the arithmetic is pinned in include/v3d.h).  No CPU fallback."""
        lib = _lib.load()
        dev = self.tsdf_vol.device
        if self.tsdf_vol.dim() != 3 or self.tsdf_vol.dtype != torch.float32:
            raise ValueError('TSDF.transform: tsdf_vol must be [nx, ny, nz] fp32, got %s %s'
                             % (tuple(self.tsdf_vol.shape), self.tsdf_vol.dtype))
        src_dim = tuple(int(v) for v in self.tsdf_vol.shape)
        if min(src_dim) < 2:
            raise ValueError('TSDF.transform: the volume is %s; every size must be at least 2 (the coordinates are normalised '
                             'by size - 1)' % (src_dim,))
        if transform is None:
            mat = torch.eye(4)[:3]
        else:
            mat = torch.as_tensor(transform).detach().to('cpu', torch.float32)
            if tuple(mat.shape) not in ((3, 4), (4, 4)):
                raise ValueError('TSDF.transform: transform must be [3, 4] or [4, 4], got %s' % (tuple(mat.shape),))
            mat = mat[:3]
        if not bool(torch.isfinite(mat).all()):
            raise ValueError('TSDF.transform: transform is not finite')
        dim = src_dim if voxel_dim is None else tuple(int(v) for v in voxel_dim)
        if len(dim) != 3 or min(dim) < 1 or dim[0] * dim[1] * dim[2] >= 2 ** 31:
            raise ValueError('TSDF.transform: voxel_dim %r (three positive sizes, fewer than 2^31 voxels)' % (voxel_dim,))
        src_origin = torch.as_tensor(self.origin).detach().to('cpu', torch.float32).reshape(-1)
        new_origin = src_origin if origin is None else torch.as_tensor(origin).detach().to('cpu', torch.float32).reshape(-1)
        if src_origin.numel() != 3 or new_origin.numel() != 3:
            raise ValueError('TSDF.transform: an origin has three components')
        if not bool(torch.isfinite(src_origin).all() and torch.isfinite(new_origin).all()):
            raise ValueError('TSDF.transform: an origin is not finite')
        vs = float(self.voxel_size)
        if not (np.isfinite(vs) and vs > 0):
            raise ValueError('TSDF.transform: voxel_size=%r (positive and finite)' % (self.voxel_size,))
        vols = {}
        for key, value in self.attribute_vols.items():
            if value.dim() not in (3, 4) or tuple(value.shape[-3:]) != src_dim:
                raise ValueError('TSDF.transform: attribute volume %r is %s; [nx, ny, nz] or [C, nx, ny, nz] on the grid %s expected'
                                 % (key, tuple(value.shape), src_dim))
            if value.element_size() not in (1, 2, 4, 8) or value.is_complex():
                raise ValueError('TSDF.transform: attribute volume %r has dtype %s' % (key, value.dtype))
        if not torch.cuda.is_available() or not self.tsdf_vol.is_cuda:
            raise _lib.V3DLibraryError('TSDF.transform: the volume must live on a HIP device (no CPU fallback)')
        for key, value in self.attribute_vols.items():
            vols[key] = value.to(dev).contiguous()
        grid = (src_dim[0], src_dim[1], src_dim[2], vs, (ctypes.c_float * 3)(*src_origin.tolist()),
                (ctypes.c_float * 12)(*mat.reshape(-1).tolist()), 1 if align_corners else 0, dim[0], dim[1], dim[2],
                (ctypes.c_float * 3)(*new_origin.tolist()))
        tsdf_src = self.tsdf_vol.contiguous()
        tsdf_dst = torch.empty(dim, dtype=torch.float32, device=dev)
        out = {}
        fused = next((k for k, v in vols.items() if v.dtype == torch.float32), None)
        with torch.cuda.device(dev):
            stream = _lib.stream_ptr(dev)
            for key, value in vols.items():
                channels = 1 if value.dim() == 3 else int(value.shape[0])
                dst = torch.empty(tuple(value.shape[:-3]) + dim, dtype=value.dtype, device=dev)
                out[key] = dst
                if channels == 0:
                    continue
                if value.dtype == torch.float32:
                    with_tsdf = key == fused
                    _lib.check(lib.v3d_tsdf_resample_f32(_lib.ptr(tsdf_src) if with_tsdf else None, _lib.ptr(value), channels, *grid,
                                                         _lib.ptr(tsdf_dst) if with_tsdf else None, _lib.ptr(dst), stream),
                               'v3d_tsdf_resample_f32')
                else:
                    fill = {'semseg': -1, 'mask_outside': True}.get(key)
                    fill_bytes = None if fill is None else torch.tensor([fill]).to(value.dtype).numpy().tobytes()
                    _lib.check(lib.v3d_volume_resample_nearest(_lib.ptr(value), value.element_size(), channels, *grid,
                                                               0 if fill is None else 1, fill_bytes, _lib.ptr(dst), stream),
                               'v3d_volume_resample_nearest')
            if fused is None or out[fused].numel() == 0:
                _lib.check(lib.v3d_tsdf_resample_f32(_lib.ptr(tsdf_src), None, 0, *grid, _lib.ptr(tsdf_dst), None, stream),
                           'v3d_tsdf_resample_f32')
        return TSDF(self.voxel_size, new_origin.view(1, 3).to(dev), tsdf_dst, out, self.attributes)


def _masked_l1(pred, trgt, non_surface_only):
    """Mean |pred - trgt| over the target's observed voxels (``weight != 0``; with ``non_surface_only`` also ``trgt < 1``), as a
    float64 sum on the prediction's device; NaN for an empty mask, as ``F.l1_loss`` gives."""
    if float(pred.voxel_size) != float(trgt.voxel_size):
        raise ValueError('l1: voxel sizes %r and %r differ' % (pred.voxel_size, trgt.voxel_size))
    if tuple(pred.tsdf_vol.shape) != tuple(trgt.tsdf_vol.shape):
        raise ValueError('l1: volumes of %s and %s voxels are not aligned (eval_tsdf aligns them)'
                         % (tuple(pred.tsdf_vol.shape), tuple(trgt.tsdf_vol.shape)))
    dev = pred.tsdf_vol.device
    if not torch.equal(torch.as_tensor(pred.origin).reshape(-1).float().cpu(), torch.as_tensor(trgt.origin).reshape(-1).float().cpu()):
        raise ValueError('l1: the origins differ (eval_tsdf aligns the volumes)')
    weight = trgt.attributes.get('weight', trgt.attribute_vols.get('weight'))
    if weight is None:
        raise ValueError("l1: the target carries no 'weight' (which voxels were observed)")
    t = trgt.tsdf_vol.to(dev)
    mask = weight.to(dev).reshape(t.shape) != 0
    if non_surface_only:
        mask = mask & (t < 1.)
    diff = (pred.tsdf_vol.double() - t.double()).abs()
    return (diff[mask].sum() / mask.sum()).item()


def l1(pred, trgt):
    """The reference's ``l1`` (mv3d/baselines/atlas/evaluation.py:61-77) of two aligned ``TSDF``: the mean absolute difference
    over the voxels the target observed (``trgt.attributes['weight'] != 0``, as ``TSDF.load`` places it; a ``'weight'``
    attribute volume serves too)."""
    return _masked_l1(pred, trgt, False)


def l1_ns(pred, trgt):
    """The reference's ``l1_ns`` (:80-96): ``l1`` restricted further to ``trgt < 1``."""
    return _masked_l1(pred, trgt, True)


def eval_tsdf(pred, trgt, device=None):
    """The reference's volume metric (mv3d/baselines/atlas/evaluation.py:24-51) -> ``{'l1': ..., 'l1_ns': ...}``.  ``pred`` and
    ``trgt`` are ``TSDF`` objects or npz paths (read with ``TSDF.load`` and moved to ``device``, default the first HIP device).
    The prediction is brought onto the target's grid by ``transform(voxel_dim=..., origin=..., align_corners=True)``; the
    shift between the two origins must be a whole number of voxels (``torch.allclose``'s rule), else ``ValueError``.  The two
    means are stock torch ops with float64 sums: once per scene, not a hot path."""
    def get(v):
        if isinstance(v, TSDF):
            return v
        return TSDF.load(v).to(_fusion._device(device))
    pred, trgt = get(pred), get(trgt)
    shift = (torch.as_tensor(trgt.origin).float().cpu() - torch.as_tensor(pred.origin).float().cpu()) / trgt.voxel_size
    if not torch.allclose(shift, shift.round()):
        raise ValueError('eval_tsdf: the origins differ by %s voxels, not by a whole number' % (shift.reshape(-1).tolist(),))
    pred = pred.transform(voxel_dim=list(trgt.tsdf_vol.shape), origin=torch.as_tensor(trgt.origin).detach().cpu(),
                          align_corners=True)
    return {'l1': l1(pred, trgt), 'l1_ns': l1_ns(pred, trgt)}


class TSDFFusion:
    """Accumulates depth maps into a TSDF volume (tsdf_atlas.py:341-463) with the reference's constructor order.
    ``tsdf_vol`` holds the running SUM of truncated distances (fresh: -1, as the reference's constructor fills it and
    never-seen voxels keep it; after ``reset()``: +1, as the reference's ``reset`` fills it), ``weight_vol`` the number of
    views that saw a voxel, ``color_vol`` [3, n] the summed colours (None with ``color=False``).  ``device=None`` takes the
    first HIP device (the host when there is none: such an object can be built and reset, not integrated into)."""

    def __init__(self, voxel_dim=(128, 128, 128), voxel_size=.02, origin=(0, 0, 0), trunc_ratio=3, device=None,
                 color=True, label=False):
        if label:
            raise NotImplementedError('TSDFFusion: the label volume is not provided (the evaluation path passes label=False)')
        if device is None:
            device = torch.device('cuda:0' if torch.cuda.is_available() else 'cpu')
        device = torch.device(device)
        nx, ny, nz = (int(v) for v in voxel_dim)
        if min(nx, ny, nz) < 1 or nx * ny * nz >= 2 ** 31:
            raise ValueError('TSDFFusion: voxel_dim %r (positive, fewer than 2^31 voxels)' % (voxel_dim,))
        self.voxel_dim = voxel_dim
        self.voxel_size = voxel_size
        self.origin = torch.as_tensor(origin).detach().clone().to(dtype=torch.float, device=device).view(1, 3)
        self.trunc_margin = voxel_size * trunc_ratio
        self.device = device
        self._dims = (nx, ny, nz)
        self._origin_host = (ctypes.c_float * 3)(*[float(v) for v in self.origin.view(3).cpu()])
        self.tsdf_vol = -torch.ones(nx * ny * nz, device=device)
        self.weight_vol = torch.zeros(nx * ny * nz, device=device)
        self.color_vol = torch.zeros((3, nx * ny * nz), device=device) if color else None
        self.label_vol = None

    def reset(self):
        self.tsdf_vol.fill_(1)
        self.weight_vol.fill_(0)
        if self.color_vol is not None:
            self.color_vol.fill_(0)

    def _lib(self, what):
        lib = _lib.load()
        if not torch.cuda.is_available() or not self.tsdf_vol.is_cuda:
            raise _lib.V3DLibraryError('%s: the volume must live on a HIP device (no CPU fallback)' % what)
        return lib

    def integrate_batch(self, projections, depths, colors=None):
        """N views in ONE launch, applied in the given order: projections [N, 3, 4], depths [N, h, w], colors [N, 3, h, w]
        (required exactly when the volume carries colour).  Gives the bits of N ``integrate`` calls."""
        lib = self._lib('TSDFFusion.integrate_batch')
        projections, depths = torch.as_tensor(projections), torch.as_tensor(depths)
        if depths.dim() != 3 or projections.dim() != 3 or projections.shape != (depths.shape[0], 3, 4):
            raise ValueError('integrate_batch: projections [N, 3, 4] and depths [N, h, w] expected, got %s and %s'
                             % (tuple(projections.shape), tuple(depths.shape)))
        n, h, w = depths.shape
        if (colors is None) != (self.color_vol is None):
            raise ValueError('integrate_batch: colours are required exactly when the volume was built with color=True')
        P = projections.to(self.device, torch.float32).contiguous()
        d = depths.to(self.device, torch.float32).contiguous()
        img = None
        if colors is not None:
            if tuple(colors.shape) != (n, 3, h, w):
                raise ValueError('integrate_batch: colors must be [N, 3, h, w] = %s, got %s' % ((n, 3, h, w), tuple(colors.shape)))
            img = torch.as_tensor(colors).to(self.device, torch.float32).contiguous()
        nx, ny, nz = self._dims
        with torch.cuda.device(self.device):
            _lib.check(lib.v3d_tsdf_integrate_f32(_lib.ptr(self.tsdf_vol), _lib.ptr(self.weight_vol), _lib.ptr(self.color_vol),
                                                  nx, ny, nz, float(self.voxel_size), self._origin_host,
                                                  float(self.trunc_margin), _lib.ptr(P), _lib.ptr(d), _lib.ptr(img), n, h, w,
                                                  _lib.stream_ptr(self.device)), 'v3d_tsdf_integrate_f32')

    def integrate(self, projection, depth, color=None, label=None):
        """One view (tsdf_atlas.py:390): projection [3, 4], depth [h, w], color [3, h, w]."""
        if label is not None:
            raise NotImplementedError('TSDFFusion.integrate: the label volume is not provided')
        self._lib('TSDFFusion.integrate')
        self.integrate_batch(torch.as_tensor(projection)[None], torch.as_tensor(depth)[None],
                             None if color is None else torch.as_tensor(color)[None])

    def get_tsdf(self, point_cloud=False):
        """-> ``TSDF`` with the averaged distances [nx, ny, nz] (sum / weight where weight > 0, the fill value elsewhere),
        ``attribute_vols['weight']`` and, with colour, ``['color']`` [3, nx, ny, nz] averaged the same way.
        ``point_cloud=True`` with colour also attaches the reference's ``attribute_vols['tsdf_point_cloud']`` (:465-481):
        [V, 6] float64 on the device, world x y z of every marching-cubes vertex and floor(colour at round(vertex)) in
        channel order; the values are the kernel's fp32 / byte results.  Off by default: it costs a pass over the volume and
        one read-back, and ``save`` would write it."""
        lib = self._lib('TSDFFusion.get_tsdf')
        nx, ny, nz = self._dims
        tsdf_vol = torch.empty_like(self.tsdf_vol)
        color_vol = None if self.color_vol is None else torch.empty_like(self.color_vol)
        with torch.cuda.device(self.device):
            _lib.check(lib.v3d_tsdf_normalize_f32(_lib.ptr(self.tsdf_vol), _lib.ptr(self.weight_vol), _lib.ptr(self.color_vol),
                                                  nx * ny * nz, _lib.ptr(tsdf_vol), _lib.ptr(color_vol),
                                                  _lib.stream_ptr(self.device)), 'v3d_tsdf_normalize_f32')
        attribute_vols = {'weight': self.weight_vol.view(nx, ny, nz)}
        if color_vol is not None:
            attribute_vols['color'] = color_vol.view(3, nx, ny, nz)
            if point_cloud:
                verts, colors, _ = _mesh.extract(tsdf_vol.view(nx, ny, nz), attribute_vols['color'], self.voxel_size, self.origin,
                                                 _mesh.MODE_POINT_CLOUD)
                attribute_vols['tsdf_point_cloud'] = torch.cat((verts.double(), colors.double()), dim=1)
        return TSDF(self.voxel_size, self.origin, tsdf_vol.view(nx, ny, nz), attribute_vols)


def prepare_preds_tsdf(preds, images):
    """Host preparation of a ``preds.npz`` record (path or mapping) and the scene's images [N, H, W, 3] (RGB, any dtype) for
    the TSDF branch (processresults.py:306-320): poses from ``rotmats`` / ``tvecs``, images flipped to BGR, made float
    [N, 3, H, W] and bilinearly resized to the depth maps' size.  No probability masking: the reference's TSDF branch does
    none.  -> ``(depths [N, h, w], poses [N, 4, 4], K [N, 3, 3], images [N, 3, h, w])`` fp32 host tensors."""
    if isinstance(preds, (str, bytes)) or hasattr(preds, '__fspath__'):
        with np.load(preds) as f:
            preds = {k: f[k] for k in f.files}
    rec = {k: v for k, v in preds.items() if k not in ('init_prob', 'final_prob')}
    depths, poses, K = _fusion.prepare_preds(rec)
    images = torch.as_tensor(np.asarray(images))
    if images.dim() != 4 or images.shape[0] != depths.shape[0] or images.shape[-1] != 3:
        raise ValueError('prepare_preds_tsdf: images must be [N, H, W, 3] with N = %d, got %s'
                         % (depths.shape[0], tuple(images.shape)))
    images = images[..., [2, 1, 0]].permute(0, 3, 1, 2).float()
    images = F.interpolate(images, tuple(depths.shape[-2:]), mode='bilinear')
    return torch.from_numpy(depths), torch.from_numpy(poses), torch.from_numpy(K), images


def fuse_preds_tsdf(preds, images, vox_res=.04, trunc_ratio=3, vol_prcnt=.995, vol_margin=1.5, img_batch=100, color=True,
                    device=None, return_fusion=False, gt_mesh=None, bounds='host'):
    """The ``run_tsdf`` branch up to ``get_tsdf()``: bounds from ``volume_bounds`` (``bounds='device'``: from
    ``volume_bounds_device``), one ``integrate_batch`` per chunk of
    ``img_batch`` views, ``get_tsdf()``.  -> ``TSDF`` (on the device); ``return_fusion=True`` -> ``(TSDF, TSDFFusion)``.
    ``gt_mesh``: each chunk's depths are masked with that mesh rendered at the predictions' size before they are integrated
    (:368-371); the bounds are taken from the unmasked depths, as the reference takes them."""
    _lib.load()
    dev = _fusion._device(device)
    depths, poses, K, images = prepare_preds_tsdf(preds, images)
    origin, _, vol_dim = _bounds_fn(bounds, 'fuse_preds_tsdf')(depths.to(dev), K, poses, vol_prcnt, vol_margin, vox_res, img_batch)
    fus = TSDFFusion(vol_dim, vox_res, origin, trunc_ratio, dev, color=color, label=False)
    masker = None if gt_mesh is None else _meshtodepth.Renderer(gt_mesh, depths.shape[1], depths.shape[2], device=dev)
    for start in range(0, depths.shape[0], int(img_batch)):
        sl = slice(start, start + int(img_batch))
        d = depths[sl] if masker is None else _meshtodepth.mask_with_mesh(depths[sl], masker, poses[sl], K[sl])
        fus.integrate_batch(projection_matrices(K[sl], poses[sl]), d, images[sl] if color else None)
    tsdf = fus.get_tsdf()
    return (tsdf, fus) if return_fusion else tsdf


def _vertex_metrics(vertices, gt_points, voxel_downsample, dist_thresh, dev):
    """A mesh's vertices [V, 3] (device) against ``gt_points``: both down-sampled, then ``metrics3d.eval_clouds`` -> dict of
    the five metrics (NaN when either side is empty, as the reference's NumPy means give)."""
    out = {k: float('nan') for k in _metrics3d.KEYS}
    gt = _metrics3d._to_device(_metrics3d._points(gt_points), dev)
    if vertices.shape[0] > 0 and gt.shape[0] > 0:
        pred, _, n_pred = _metrics3d.voxel_down_sample(vertices, voxel_downsample)
        trgt, _, n_trgt = _metrics3d.voxel_down_sample(gt, voxel_downsample)
        n_pred, n_trgt = int(n_pred.item()), int(n_trgt.item())
        for c in (n_pred, n_trgt):
            if c < 0:
                _metrics3d._raise_status(-c)
        if n_pred > 0 and n_trgt > 0:
            out = dict(zip(_metrics3d.KEYS, _metrics3d.eval_clouds(pred[:n_pred], trgt[:n_trgt], dist_thresh).cpu().tolist()))
    return out


def tsdf_mesh_metrics(preds, images, gt_points, vox_res=.04, trunc_ratio=3, voxel_downsample=0.02, dist_thresh=0.05,
                      vol_prcnt=.995, vol_margin=1.5, img_batch=100, device=None, return_mesh=False, gt_mesh=None, bounds='host'):
    """The ``run_tsdf`` branch to its end (processresults.py:297-397) without files: ``fuse_preds_tsdf`` (with ``gt_mesh``: the
    predictions masked by that mesh) -> ``get_mesh`` -> the mesh's vertices through ``metrics3d.voxel_down_sample`` ->
    ``metrics3d.eval_clouds`` against the down-sampled ``gt_points`` [n, 3].  -> the dict of the five metrics and ``'n'`` (the
    number of views); ``return_mesh=True`` -> ``(dict, TriangleMesh)``.  An empty mesh or ground truth gives NaN metrics, as
    the reference's NumPy means do.  The vertices never leave the device; read-backs: the mesh's two counts, the two
    down-sampled counts and the final 40-byte record (and one status word per rendered chunk with ``gt_mesh``).
    ``bounds`` is ``fuse_preds_tsdf``'s."""
    _lib.load()
    dev = _fusion._device(device)
    if isinstance(preds, (str, bytes)) or hasattr(preds, '__fspath__'):
        with np.load(preds) as f:
            preds = {k: f[k] for k in f.files}
    n_views = int(np.asarray(preds['depth_preds']).shape[0])
    tsdf = fuse_preds_tsdf(preds, images, vox_res, trunc_ratio, vol_prcnt, vol_margin, img_batch, color=True, device=dev,
                           gt_mesh=gt_mesh, bounds=bounds)
    mesh = tsdf.get_mesh()
    out = _vertex_metrics(mesh.vertices, gt_points, voxel_downsample, dist_thresh, dev)
    out['n'] = n_views
    return (out, mesh) if return_mesh else out


def trim_mesh(mesh, poses, K, images=None, size=(480, 640), mask_mesh=None, vox_res=.04, trunc_ratio=3, vol_prcnt=.995,
              vol_margin=1.5, img_batch=100, device=None, bounds='host'):
    """The reference's ``trim_mesh`` (processresults.py:71-150) over given cameras -- ``poses`` [N, 4, 4] world -> camera, ``K``
    [N, 3, 3] at ``size``: (1) ``meshtodepth.process_scene`` renders the mesh into every view; (2) ``volume_bounds`` of those
    depths; (3) the depths -- with ``mask_mesh`` zeroed where a rendering of that mesh sees nothing (:134-137) -- go into a
    ``TSDFFusion`` in chunks of ``img_batch``, with ``images`` [N, 3, h, w] fp32 as colours (None: a volume without colour);
    (4) ``get_tsdf().get_mesh()``.  -> ``mesh.TriangleMesh`` on the device: the part of the surface the cameras saw.
    ``bounds='device'`` takes step (2) from ``volume_bounds_device``: the renderings stay on the device."""
    _lib.load()
    dev = _fusion._device(device)
    K, poses = torch.as_tensor(K).float().cpu(), torch.as_tensor(poses).float().cpu()
    n, step = int(poses.shape[0]), int(img_batch)
    if images is not None:
        images = torch.as_tensor(images)
        if tuple(images.shape) != (n, 3, int(size[0]), int(size[1])):
            raise ValueError('trim_mesh: images must be [N, 3, h, w] = %s, got %s'
                             % ((n, 3, int(size[0]), int(size[1])), tuple(images.shape)))
    renderer = _meshtodepth.Renderer(mesh, size[0], size[1], device=dev)
    depths = torch.cat([renderer.render(K[i:i + step], poses[i:i + step]) for i in range(0, n, step)], dim=0)
    origin, _, vol_dim = _bounds_fn(bounds, 'trim_mesh')(depths, K, poses, vol_prcnt, vol_margin, vox_res, img_batch)
    fus = TSDFFusion(vol_dim, vox_res, origin, trunc_ratio, dev, color=images is not None, label=False)
    masker = None if mask_mesh is None else _meshtodepth.Renderer(mask_mesh, size[0], size[1], device=dev)
    for i in range(0, n, step):
        sl = slice(i, i + step)
        d = depths[sl] if masker is None else _meshtodepth.mask_with_mesh(depths[sl], masker, poses[sl], K[sl])
        fus.integrate_batch(projection_matrices(K[sl], poses[sl]), d, None if images is None else images[sl])
    return fus.get_tsdf().get_mesh()


def mesh_3d_metrics(mesh, gt_points, poses, K, images=None, size=(480, 640), mask_mesh=None, vox_res=.04, trunc_ratio=3,
                    voxel_downsample=0.02, dist_thresh=0.05, vol_prcnt=.995, vol_margin=1.5, img_batch=100, device=None,
                    return_mesh=False, bounds='host'):
    """The body of ``process_volume_3d_metrics`` (processresults.py:172-200) without files: ``trim_mesh``, then the trimmed
    mesh's vertices and ``gt_points`` down-sampled and scored by ``metrics3d.eval_clouds``.  -> the dict of the five metrics;
    ``return_mesh=True`` -> ``(dict, trimmed TriangleMesh)``.  ``bounds`` is ``trim_mesh``'s."""
    dev = _fusion._device(device)
    trimmed = trim_mesh(mesh, poses, K, images, size, mask_mesh, vox_res, trunc_ratio, vol_prcnt, vol_margin, img_batch, dev, bounds)
    out = _vertex_metrics(trimmed.vertices, gt_points, voxel_downsample, dist_thresh, dev)
    return (out, trimmed) if return_mesh else out
