"""NumPy checker of scene preparation (3dvnet_amd/preprocess.py, csrc/prepare.hip) -- a checker, not a product path.

``register`` restates the pinned chain of include/v3d.h (v3d_register_colour_u8) with NumPy float32 arrays: every operation is one
float32 array operation, so each is rounded on its own and nothing is fused.  It equals the reference's ``process_color_image``
(data_preprocess/preprocess_scannet.py:36-70, torch on the CPU) bit for bit on every fixture of tests/golden/P_register_*.npz
(tests/test_preprocess_oracle.py), so the device kernel is compared with it for equality.

``lut`` is the reference's depth-unit conversion in the reference's own type (preprocess_icl_nuim.py:181-185 float64,
preprocess_tum_rgbd.py:177-180 float32) over all 65 536 inputs.

``raw_scene`` / ``MemoryFiles``: a synthetic raw scene whose image files live in a dict, for the scene drivers.
"""
import hashlib
import importlib
import os

import numpy as np

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# ScanNet's exported intrinsics of two scenes (intrinsic_color.txt / intrinsic_depth.txt: fx, fy, cx, cy), as published with the
# dataset: the second pair's colour camera sees less than the depth camera at the frame's edge
SCANNET_PAIRS = {
    'a': ((1169.621094, 1167.105103, 646.295044, 489.927032), (577.590698, 578.729797, 318.905426, 242.683609)),
    'b': ((1165.723022, 1165.738037, 649.094971, 484.765015), (574.540771, 577.583740, 322.522827, 238.558853)),
}


def kmat(fx, fy, cx, cy, skew=0.0):
    return np.array([[fx, skew, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]], dtype=np.float64)


def homography(K_color, K_depth):
    """float64 product with np.linalg.inv, cast once (preprocess_scannet.py:48-49)"""
    return np.asarray(K_color, dtype=np.float64).dot(np.linalg.inv(np.asarray(K_depth, dtype=np.float64))).astype(F32)


def sample_positions(H, Hc, Wc, h, w):
    """-> (jx, jy) float32 [h, w]: the rounded sample positions of the pinned chain (NaN / inf where it gives them)"""
    H = np.asarray(H, dtype=F32).reshape(3, 3)
    x = np.arange(w, dtype=F32)[None, :].repeat(h, 0)
    y = np.arange(h, dtype=F32)[:, None].repeat(w, 1)
    with np.errstate(all='ignore'):
        u = (H[0, 0] * x + H[0, 1] * y) + H[0, 2]
        v = (H[1, 0] * x + H[1, 1] * y) + H[1, 2]
        d = (H[2, 0] * x + H[2, 1] * y) + H[2, 2]
        d = d + F32(1e-8)
        u = u / d
        v = v / d
        half_w, half_h = F32(Wc / 2.0), F32(Hc / 2.0)
        gx = (u - half_w) / half_w
        gy = (v - half_h) / half_h
        ix = (gx + F32(1)) * (F32(Wc - 1) / F32(2))
        iy = (gy + F32(1)) * (F32(Hc - 1) / F32(2))
        assert all(a.dtype == F32 for a in (u, v, d, gx, gy, ix, iy))
        return np.rint(ix), np.rint(iy)                                            # half to even


def register(colour, depth_size, H):
    """colour uint8 [n, Hc, Wc, 3] (or [Hc, Wc, 3]), H float32 [3, 3] -> (uint8 [n, h, w, 3], outside bool [h, w])"""
    colour = np.asarray(colour)
    single = colour.ndim == 3
    if single:
        colour = colour[None]
    n, Hc, Wc, _ = colour.shape
    h, w = depth_size
    jx, jy = sample_positions(H, Hc, Wc, h, w)
    with np.errstate(all='ignore'):
        inside = (jx >= 0) & (jx <= Wc - 1) & (jy >= 0) & (jy <= Hc - 1)           # NaN and the infinities fail
    cx = np.where(inside, jx, 0).astype(np.int64)
    cy = np.where(inside, jy, 0).astype(np.int64)
    out = colour[:, cy, cx, :] * inside[None, :, :, None].astype(np.uint8)
    return (out[0] if single else out), ~inside


def random_colour(seed, n, Hc, Wc):
    return np.random.RandomState(seed).randint(0, 256, (n, Hc, Wc, 3)).astype(np.uint8)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fixture(name):
    with np.load(os.path.join(GOLDEN, 'P_%s.npz' % name)) as f:
        return {k: f[k] for k in f.files}


SMALL = ['register_down2', 'register_focal', 'register_skew', 'register_aligned', 'register_tie']
FULL = ['register_full_a', 'register_full_b']


def lut(kind):
    """the reference's expression over every uint16 value, in the reference's type"""
    raw = np.arange(65536, dtype=np.uint16)
    if kind == 'icl-nuim':
        depth = raw.astype(np.float64) / 5_000.
        depth[np.isnan(depth)] = 0.
        depth[np.isinf(depth)] = 0.
        return (depth * 1000).astype(np.uint16)
    if kind == 'tum-rgbd':
        depth = raw.astype(np.float32) / 5000.
        depth[np.isnan(depth)] = 0.
        depth[np.isinf(depth)] = 0.
        return (depth * 1000.).astype(np.uint16)
    raise ValueError(kind)


# ---- a raw scene in memory ------------------------------------------------------------------------------------------------------

class MemoryFiles:
    """``read_image`` / ``write_image`` / ``exists`` over a dict: path -> array.  ``reads`` / ``writes`` record the calls in order."""

    def __init__(self, files=None):
        self.files = dict(files or {})
        self.reads, self.writes = [], []

    def read_image(self, path, depth):
        self.reads.append((path, bool(depth)))
        return self.files[path]

    def write_image(self, path, array):
        self.writes.append(path)
        self.files[path] = np.array(array)

    def exists(self, path):
        return path in self.files


def room_frames(n=7, size=(24, 32), seed=31, zero_frame=6, K=None, sigma=0.03, scale=1.0):
    """The box room of tests/fusion_oracle.py as a prepared scene: colour uint8 [n, h, w, 3], depth_mm uint16 [n, h, w] (frame
    `zero_frame` all zero), K [3, 3] and poses [n, 4, 4] float64 camera -> world, as info.json holds them.  ``K``: other
    intrinsics (the depths are then the room's through those, without noise).  ``scale``: the room and the camera positions
    enlarged by that factor (depths past 4 m)."""
    import torch
    fo = importlib.import_module('fusion_oracle')
    syn = importlib.import_module('3dvnet_amd.synthetic')
    d, images, w2c, K_all = fo.scene(n, size, seed=seed, yaw_step_deg=6, sigma=sigma)
    if K is not None:
        K_all = torch.as_tensor(np.asarray(K, dtype=np.float32))[None].repeat(n, 1, 1)
        d = syn.ray_box_depth(w2c[:, :3, :3], w2c[:, :3, 3], K_all, size, size).float()
    depth_mm = np.clip(np.rint(d.numpy().astype(np.float64) * (1000.0 * scale)), 0, 65535).astype(np.uint16)
    if zero_frame is not None:
        depth_mm[zero_frame] = 0
    poses = np.linalg.inv(w2c.numpy().astype(np.float64))
    poses[:, :3, 3] *= scale
    return images.numpy().copy(), depth_mm, K_all[0].numpy().astype(np.float64), poses
