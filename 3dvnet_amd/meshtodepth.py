"""Depth maps of a triangle mesh on the device: ``mv3d/eval/meshtodepth.py`` (``Renderer``, ``process_scene``; there pyrender /
OpenGL) with the rasteriser of ``csrc/meshrender.hip`` behind ``v3d_mesh_render_depth_f32``.  This module is the plumbing:

  * ``Renderer``        the reference's class: built from a mesh, called with one camera -> ``(None, depth [h, w])``;
                        ``render`` takes all cameras of a scene in one launch;
  * ``process_scene``   mesh + poses + intrinsics -> depth maps [n, h, w] (fp32, on the device);
  * ``mask_with_mesh``  the reference's ``MASK_USING_GT_MESH`` step: predictions zeroed where the mesh is not seen.

Poses are world -> camera, as everywhere in the evaluation code (the reference inverts them to place pyrender's camera).  The
semantics are those of include/v3d.h: the nearest fragment's camera-axis depth, 0 where there is none, both sides of a triangle,
``znear`` / ``zfar`` = pyrender's ``IntrinsicsCamera`` defaults, pixel (r, c) sampled at ``(c + pixel_center, r + pixel_center)``
with OpenGL's 0.5 by default.  The differences from OpenGL (inclusive edges, no depth-buffer quantisation, a per-fragment clip,
fp32 device tensors) are listed in DESIGN.md §6.

There is no CPU fallback: without the library or a HIP device rendering raises ``V3DLibraryError``.
"""
import numpy as np
import torch

from . import _lib
from . import fusion as _fusion

STATUS_BAD_INDEX, STATUS_NON_FINITE = 1, 2          # V3D_RENDER_STATUS_* of include/v3d.h


def _projections(K, poses):
    """K [n, 3, 3], poses [n, 4, 4] -> [n, 3, 4] fp32: the batched product ``tsdf.projection_matrices`` forms."""
    K, poses = torch.as_tensor(K).float(), torch.as_tensor(poses).float()
    if K.dim() != 3 or K.shape[1:] != (3, 3) or poses.shape != (K.shape[0], 4, 4):
        raise ValueError('meshtodepth: K [n, 3, 3] and poses [n, 4, 4] expected, got %s and %s'
                         % (tuple(K.shape), tuple(poses.shape)))
    K4 = torch.cat((K, torch.zeros((K.shape[0], 3, 1), dtype=K.dtype, device=K.device)), dim=2)
    return torch.bmm(K4, poses.to(K.device))


class Renderer:
    """``mesh``: a ``mesh.TriangleMesh`` or any object with ``.vertices`` / ``.triangles`` (tensors or arrays, on the host or
    a device).  Host arrays are uploaded once, here."""

    def __init__(self, mesh, height=480, width=640, znear=.05, zfar=100., pixel_center=.5, device=None):
        _lib.load()
        if not torch.cuda.is_available():
            raise _lib.V3DLibraryError('meshtodepth.Renderer: rendering needs a HIP device (no CPU fallback)')
        v, f = mesh.vertices, mesh.triangles
        if not torch.is_tensor(v):
            v = torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32)))
        if not torch.is_tensor(f):
            f = np.asarray(f)
            if f.size and (f.min() < -2 ** 31 or f.max() >= 2 ** 31):
                raise ValueError('meshtodepth.Renderer: a triangle index does not fit in int32')
            f = torch.from_numpy(np.ascontiguousarray(f.astype(np.int32)))
        if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError('meshtodepth.Renderer: vertices [V, 3] and triangles [F, 3] expected, got %s and %s'
                             % (tuple(v.shape), tuple(f.shape)))
        if v.shape[0] >= 2 ** 31 or f.shape[0] >= 2 ** 31 - 256:
            raise ValueError('meshtodepth.Renderer: %d vertices and %d triangles do not fit the int32 counts of the C ABI'
                             % (v.shape[0], f.shape[0]))
        if f.is_floating_point():
            raise ValueError('meshtodepth.Renderer: triangles must be integers')
        dev = v.device if v.is_cuda else (f.device if f.is_cuda else _fusion._device(device))
        self.device = dev
        self.vertices = v.detach().to(dev, torch.float32).contiguous()
        self.triangles = f.detach().to(dev, torch.int32).contiguous()
        self.height, self.width = int(height), int(width)
        self.znear, self.zfar, self.pixel_center = float(znear), float(zfar), float(pixel_center)
        if self.height < 1 or self.width < 1:
            raise ValueError('meshtodepth.Renderer: image size %d x %d' % (self.height, self.width))

    def render(self, K, poses):
        """K [n, 3, 3], poses [n, 4, 4] (world -> camera) -> depth [n, h, w] fp32 on the device: every view in ONE launch.
        One 4-byte read-back, after the launch: the status word (``ValueError`` for a triangle index outside the vertex list
        or a non-finite vertex)."""
        return self.render_projections(_projections(K, poses))

    def render_projections(self, projections):
        """As ``render`` from the [n, 3, 4] matrices K [R | t] themselves."""
        lib = _lib.load()
        P = torch.as_tensor(projections)
        if P.dim() != 3 or P.shape[1:] != (3, 4):
            raise ValueError('meshtodepth: projections [n, 3, 4] expected, got %s' % (tuple(P.shape),))
        n, h, w = int(P.shape[0]), self.height, self.width
        if n * h * w >= 2 ** 31:
            raise ValueError('meshtodepth: %d x %d x %d pixels (fewer than 2^31 in one call)' % (n, h, w))
        dev = self.device
        if n == 0 or self.triangles.shape[0] == 0 or self.vertices.shape[0] == 0:
            return torch.zeros((n, h, w), dtype=torch.float32, device=dev)
        P = P.detach().to(dev, torch.float32).contiguous()
        depth = torch.empty((n, h, w), dtype=torch.float32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(lib.v3d_mesh_render_depth_f32(self.vertices.data_ptr(), int(self.vertices.shape[0]),
                                                     self.triangles.data_ptr(), int(self.triangles.shape[0]), P.data_ptr(), n,
                                                     h, w, self.pixel_center, self.znear, self.zfar, depth.data_ptr(),
                                                     status.data_ptr(), _lib.stream_ptr(dev)), 'v3d_mesh_render_depth_f32')
            code = int(status.item())
        if code:
            why = [m for b, m in ((STATUS_BAD_INDEX, 'a triangle index lies outside the vertex list'),
                                  (STATUS_NON_FINITE, 'a vertex coordinate is not finite')) if code & b]
            raise ValueError('meshtodepth: ' + '; '.join(why))
        return depth

    def __call__(self, intrinsics, pose):
        """One camera: intrinsics [3, 3], pose [4, 4] -> ``(None, depth [h, w])``, the reference's ``(colour, depth)``."""
        return None, self.render(torch.as_tensor(intrinsics)[None], torch.as_tensor(pose)[None])[0]

    def delete(self):
        """Nothing to release (the reference frees its OpenGL context here)."""


def process_scene(mesh, poses, K, render_size=(480, 640), znear=.05, zfar=100., pixel_center=.5, device=None):
    """The reference's ``process_scene``: depth maps [n, h, w] of ``mesh`` from the cameras ``poses`` [n, 4, 4] / ``K``
    [n, 3, 3] -- fp32 on the device, every view in one launch."""
    renderer = Renderer(mesh, render_size[0], render_size[1], znear, zfar, pixel_center, device)
    depths = renderer.render(K, poses)
    renderer.delete()
    return depths


def mask_with_mesh(depth_preds, mesh, poses, K, device=None):
    """``np.where(render == 0, 0, depth_preds)`` (processresults.py:263-266, :368-371) with the mesh rendered at the
    predictions' own size [n, h, w] -> fp32 [n, h, w] on the device.  ``mesh`` may be a ``Renderer`` of that size: a caller
    that masks a scene in chunks builds it once, so that a host mesh is uploaded once."""
    _lib.load()
    d = torch.as_tensor(depth_preds)
    if d.dim() != 3:
        raise ValueError('mask_with_mesh: depth_preds [n, h, w] expected, got %s' % (tuple(d.shape),))
    size = tuple(int(v) for v in d.shape[-2:])
    if isinstance(mesh, Renderer):
        if (mesh.height, mesh.width) != size:
            raise ValueError('mask_with_mesh: the renderer draws %d x %d, the predictions are %d x %d'
                             % ((mesh.height, mesh.width) + size))
        seen = mesh.render(K, poses)
    else:
        dev = d.device if d.is_cuda else _fusion._device(device)
        seen = process_scene(mesh, poses, K, size, device=dev)
    d = d.to(seen.device, torch.float32)
    return torch.where(seen == 0, torch.zeros_like(d), d)
