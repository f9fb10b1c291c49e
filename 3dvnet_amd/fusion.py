"""Multi-view depth fusion on the device: the depth maps ``process_scene`` / ``results.write_preds`` leave behind ->
one fused, coloured point cloud (``mv3d/eval/pointcloudfusion_custom.py``, called from
``mv3d/eval/processresults.py:203-281``).  The arithmetic is ``csrc/fusion.hip`` behind ``v3d_fuse_depths_f32`` /
``v3d_fusion_compact``; this module is the plumbing around it:

  * ``process_depth`` / ``process_scene``  the reference's signatures and return tuples (NumPy at the boundary);
  * ``fuse_depth_maps``                    device tensors in, device tensors out, optional source window / lists;
  * ``fuse_preds``                         from a ``preds.npz`` record (path or mapping); its host preparation is
                                           ``prepare_preds`` and needs no device.

There is no CPU fallback: without the library or a HIP device every fusing entry raises ``V3DLibraryError``.
"""
import ctypes

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib

CAM_FLOATS = 48      # camera block of include/v3d.h: K, K^-1, R, t, rows 0..2 of P^-1


def camera_blocks(poses, K):
    """[N, 4, 4] world->camera poses, [N, 3, 3] intrinsics -> [N, 48] fp32 blocks on the tensors' device.  The inverses are
    ``torch.inverse`` of the 3x3 / 4x4 matrices, as the reference takes them (pointcloudfusion_custom.py:22-24), not an
    analytic transpose: their last bits are part of the result."""
    poses = torch.as_tensor(poses).float()
    K = torch.as_tensor(K).float().to(poses.device)
    if poses.dim() != 3 or poses.shape[1:] != (4, 4) or K.shape != (poses.shape[0], 3, 3):
        raise ValueError('camera_blocks: poses [N, 4, 4] and K [N, 3, 3] expected, got %s and %s'
                         % (tuple(poses.shape), tuple(K.shape)))
    n = poses.shape[0]
    cam = torch.zeros((n, CAM_FLOATS), dtype=torch.float32, device=poses.device)
    cam[:, 0:9] = K.reshape(n, 9)
    cam[:, 9:18] = torch.inverse(K).reshape(n, 9)
    cam[:, 18:27] = poses[:, :3, :3].reshape(n, 9)
    cam[:, 27:30] = poses[:, :3, 3]
    cam[:, 30:42] = torch.inverse(poses)[:, :3, :].reshape(n, 12)
    return cam


def window_lists(n_img, src_window, ref_idx=None):
    """CSR source lists (edge_ofs [n_ref + 1], edge_src) of a +-k view window: reference r takes the images
    r - before .. r + after that exist, without r itself, in ascending order."""
    before, after = int(src_window[0]), int(src_window[1])
    if before < 0 or after < 0:
        raise ValueError('src_window must be (before >= 0, after >= 0), got %r' % (src_window,))
    refs = range(n_img) if ref_idx is None else [int(r) for r in ref_idx]
    ofs, src = [0], []
    for r in refs:
        src.extend(s for s in range(max(0, r - before), min(n_img, r + after + 1)) if s != r)
        ofs.append(len(src))
    return np.asarray(ofs, dtype=np.int32), np.asarray(src, dtype=np.int32)


def _int_array(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _require_device(t, what):
    if not torch.cuda.is_available() or not t.is_cuda:
        raise _lib.V3DLibraryError('%s: tensors must live on a HIP device (no CPU fallback)' % what)


def fuse_depth_maps(depths, poses, K, images=None, z_thresh=0.1, n_consistent_thresh=3, src_window=None,
                    src_lists=None, ref_idx=None, trim=False, return_dense=False):
    """Device-level fusion.  depths [N, h, w] fp32 on a HIP device; images [N, h, w, 3] of any dtype on the device, or
    None; poses [N, 4, 4] / K [N, 3, 3] on the host or the device.  Their inverses are taken where they live.  HOST poses
    and intrinsics are the path without any synchronisation, and the one whose inverses carry the bits of the host solver
    the reference-generated fixtures were made with (``process_scene`` / ``process_depth`` always take it); with DEVICE
    tensors ``torch.inverse`` runs the device solver, whose status check is a hidden read-back and whose last bits may
    differ.

    ``src_window=(before, after)`` or ``src_lists=(edge_ofs, edge_src)`` (host integer arrays, CSR per reference) choose
    the sources; default: every other image, ascending.  ``ref_idx`` (host integers) restricts the references.

    Returns ``(pts [M', 3] fp32, rgb [M', 3] | None, valid [n_ref, h, w] bool, count)``: the kept points in (view, pixel)
    order and ``count`` = their number M as a device int32 word.  With ``trim=False`` this function reads nothing back
    and M' is the worst case n_ref h w (rows >= M are unspecified); ``trim=True`` reads the one word back and returns M rows.
    ``return_dense=True`` appends the kernel's dense outputs ``(pts [n_ref, h w, 3], n_valid [n_ref, h w] int32)``.
    """
    lib = _lib.load()
    _require_device(depths, 'fuse_depth_maps')
    if depths.dim() != 3 or depths.dtype != torch.float32:
        raise ValueError('fuse_depth_maps: depths must be fp32 [N, h, w], got %s %s' % (depths.dtype, tuple(depths.shape)))
    if src_window is not None and src_lists is not None:
        raise ValueError('fuse_depth_maps: give src_window or src_lists, not both')
    dev = depths.device
    depths = depths.contiguous()
    n, h, w = depths.shape
    cams = camera_blocks(poses, K).to(dev).contiguous()
    if cams.shape[0] != n:
        raise ValueError('fuse_depth_maps: %d depth maps but %d cameras' % (n, cams.shape[0]))
    ref_arr, ref_p = (None, None) if ref_idx is None else _int_array(ref_idx)
    n_ref = n if ref_arr is None else int(ref_arr.shape[0])
    if src_window is not None:
        src_lists = window_lists(n, src_window, ref_arr)
    (ofs_arr, ofs_p), (src_arr, src_p) = ((None, None), (None, None)) if src_lists is None else \
        (_int_array(src_lists[0]), _int_array(src_lists[1]))
    if ofs_arr is not None and (ofs_arr.shape[0] != n_ref + 1 or int(ofs_arr[-1]) != src_arr.shape[0]):
        raise ValueError('fuse_depth_maps: edge_ofs must have n_ref + 1 entries ending at len(edge_src)')

    hw = h * w
    ws_bytes = max(int(lib.v3d_fusion_workspace_bytes(n, h, w)), 256)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    pts = torch.empty((n_ref, hw, 3), dtype=torch.float32, device=dev)
    n_valid = torch.empty((n_ref, hw), dtype=torch.int32, device=dev)
    stream = _lib.stream_ptr(dev)
    with torch.cuda.device(dev):
        _lib.check(lib.v3d_fuse_depths_f32(_lib.ptr(depths), _lib.ptr(cams), n, h, w, ref_p, n_ref, ofs_p, src_p,
                                           float(z_thresh), _lib.ptr(pts), _lib.ptr(n_valid), _lib.ptr(ws), ws_bytes,
                                           stream), 'v3d_fuse_depths_f32')
        img_b = None
        if images is not None:
            _require_device(images, 'fuse_depth_maps(images)')
            if tuple(images.shape) != (n, h, w, 3):
                raise ValueError('fuse_depth_maps: images must be [N, h, w, 3], got %s' % (tuple(images.shape),))
            if ref_arr is not None:
                images = images[torch.as_tensor(ref_arr, dtype=torch.long, device=dev)]
            img_b = images.contiguous().view(torch.uint8).reshape(n_ref, hw, -1)
        px = 0 if img_b is None else int(img_b.shape[-1])
        valid = torch.empty((n_ref, h, w), dtype=torch.uint8, device=dev)
        counts = torch.empty(2 * n_ref + 2, dtype=torch.int32, device=dev)     # view_count | view_ofs | total
        out_pts = torch.empty((n_ref * hw, 3), dtype=torch.float32, device=dev)
        out_rgb = None if img_b is None else torch.empty((n_ref * hw, px), dtype=torch.uint8, device=dev)
        _lib.check(lib.v3d_fusion_compact(_lib.ptr(n_valid), _lib.ptr(pts), _lib.ptr(img_b), px, n_ref, h, w,
                                          int(n_consistent_thresh), _lib.ptr(valid), counts.data_ptr(),
                                          counts.data_ptr() + 4 * n_ref, _lib.ptr(out_pts), _lib.ptr(out_rgb),
                                          counts.data_ptr() + 4 * (2 * n_ref + 1), _lib.ptr(ws), ws_bytes, stream),
                   'v3d_fusion_compact')
    count = counts[2 * n_ref + 1]
    rgb = None if out_rgb is None else out_rgb.view(images.dtype).reshape(n_ref * hw, 3)
    if trim:
        m = int(count.item())                       # the one 4-byte read-back
        out_pts, rgb = out_pts[:m], (None if rgb is None else rgb[:m])
    out = (out_pts, rgb, valid.view(torch.bool), count)
    return out + (pts, n_valid) if return_dense else out


def _device(device):
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.V3DLibraryError('depth fusion needs a HIP device (no CPU fallback)')
        device = torch.device('cuda:0')
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.V3DLibraryError('depth fusion needs a HIP device (no CPU fallback), got %s' % device)
    return device


def process_scene(depth_preds, images, poses, K, z_thresh, n_consistent_thresh, device=None):
    """The reference's ``process_scene`` (pointcloudfusion_custom.py:98-116): every view is a reference against all
    others.  Host tensors / arrays in, ``(fused_pts [M, 3] float32, fused_rgb [M, 3] image dtype, all_valid [N, h, w]
    bool)`` NumPy arrays out."""
    _lib.load()
    dev = _device(device)
    depths = torch.as_tensor(depth_preds).float()
    images = torch.as_tensor(images)
    pts, rgb, valid, _ = fuse_depth_maps(depths.to(dev), torch.as_tensor(poses).cpu(), torch.as_tensor(K).cpu(),
                                         images.to(dev), z_thresh, n_consistent_thresh, trim=True)
    return pts.cpu().numpy(), rgb.cpu().numpy(), valid.cpu().numpy()


def process_depth(ref_depth, ref_image, src_depths, src_images, ref_P, src_Ps, ref_K, src_Ks, z_thresh=0.1,
                  n_consistent_thresh=3, device=None):
    """The reference's ``process_depth`` (pointcloudfusion_custom.py:10-95): one reference view against an explicit
    source set, in the given order.  ``src_images`` is accepted for the signature's sake (the reference does not read it
    either).  -> ``(pts [M, 3], rgb [M, 3], valid [h, w] bool)`` NumPy arrays."""
    _lib.load()
    dev = _device(device)
    ref_depth, src_depths = torch.as_tensor(ref_depth).float(), torch.as_tensor(src_depths).float()
    n_src = int(src_depths.shape[0])
    depths = torch.cat((ref_depth[None], src_depths), 0)
    poses = torch.cat((torch.as_tensor(ref_P)[None], torch.as_tensor(src_Ps)), 0).cpu()
    Ks = torch.cat((torch.as_tensor(ref_K)[None], torch.as_tensor(src_Ks)), 0).cpu()
    ref_image = torch.as_tensor(ref_image)
    images = torch.zeros((n_src + 1,) + tuple(ref_image.shape), dtype=ref_image.dtype)
    images[0] = ref_image
    lists = (np.array([0, n_src], dtype=np.int32), np.arange(1, n_src + 1, dtype=np.int32))
    pts, rgb, valid, _ = fuse_depth_maps(depths.to(dev), poses, Ks, images.to(dev), z_thresh, n_consistent_thresh,
                                         src_lists=lists, ref_idx=[0], trim=True)
    return pts.cpu().numpy(), rgb.cpu().numpy(), valid[0].cpu().numpy()


def prepare_preds(preds, out_size=None, prob_resize=None):
    """Host preparation of a ``preds.npz`` record (``results.write_preds``) for fusion, after
    processresults.py:218-260: 4x4 poses from ``rotmats`` / ``tvecs``; depths zeroed where ``init_prob <= 0.2`` /
    ``final_prob <= 0.1`` when those maps are present; with ``out_size=(H, W)`` different from the depth maps' size the
    depths are nearest-resized and the rows of K rescaled.  ``preds`` is a path or a mapping.  Nothing here touches a
    device.  ``prob_resize``: what to do with a probability map whose size differs from the depth maps' (the plane-grid
    ``init_prob`` of ``eval_3dvnet.pred_func_with_prob`` beside full-resolution depths): ``None`` raises, ``'nearest'`` resizes
    it with ``F.interpolate(mode='nearest')`` (the reference uses OpenCV's Lanczos-4 there: DESIGN.md 6).
    -> ``(depths [N, H, W] float32, poses [N, 4, 4] float32, K [N, 3, 3] float32)`` NumPy arrays."""
    if isinstance(preds, (str, bytes)) or hasattr(preds, '__fspath__'):
        with np.load(preds) as f:
            preds = {k: f[k] for k in f.files}
    depths = np.array(preds['depth_preds'], dtype=np.float32)          # a copy: the masks write into it
    n = depths.shape[0]
    poses = np.repeat(np.eye(4, dtype=np.float32)[None], n, axis=0)
    poses[:, :3, :3] = np.asarray(preds['rotmats'], dtype=np.float32)
    poses[:, :3, 3] = np.asarray(preds['tvecs'], dtype=np.float32)
    K = np.array(preds['K'], dtype=np.float32)
    if prob_resize not in (None, 'nearest'):
        raise ValueError("prepare_preds: prob_resize must be None or 'nearest', got %r" % (prob_resize,))
    for key, thresh in (('init_prob', 0.2), ('final_prob', 0.1)):
        if key in preds and preds[key] is not None:
            p = np.asarray(preds[key])
            if p.shape != depths.shape and prob_resize == 'nearest' and p.ndim == 3 and p.shape[0] == n:
                p = F.interpolate(torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)).unsqueeze(1),
                                  tuple(depths.shape[-2:]), mode='nearest').squeeze(1).numpy()
            if p.shape != depths.shape:
                # the reference resizes such a map with OpenCV's Lanczos filter, which this package does not restate
                raise ValueError('prepare_preds: %s has shape %s, the depth maps %s; resize it before fusing'
                                 % (key, p.shape, depths.shape))
            depths = np.where(p > thresh, depths, np.float32(0.)).astype(np.float32)
    if out_size is not None and tuple(out_size) != depths.shape[-2:]:
        x_fact = out_size[1] / float(depths.shape[-1])
        y_fact = out_size[0] / float(depths.shape[-2])
        depths = F.interpolate(torch.from_numpy(depths).unsqueeze(1), tuple(out_size), mode='nearest').squeeze(1).numpy()
        K[:, 0, :] *= x_fact
        K[:, 1, :] *= y_fact
    return depths, poses, K


def fuse_preds(preds, images, z_thresh, n_consistent_thresh, out_size=None, device=None):
    """Fuse the record ``results.write_preds`` wrote (a path or a mapping) with the scene's images [N, H, W, 3] at the
    fused size.  -> the tuple of ``process_scene``."""
    _lib.load()
    dev = _device(device)
    depths, poses, K = prepare_preds(preds, out_size)
    return process_scene(depths, images, poses, K, z_thresh, n_consistent_thresh, device=dev)
