"""NumPy checker of the scene-batch front end (3dvnet_amd/dataset.py, csrc/frames.hip): the gather tables restated as scalar loops,
the linear blend in float64, the colour chain in fp32 (and in float64, for the unquantised bound), the depth rule, and the seeded
inputs the CPU tests, the GPU tests and tests/golden/make_golden_dataset.py share.  Nothing here imports the package."""
import hashlib
import math

import numpy as np

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


# ---- tables -------------------------------------------------------------------------------------------------------------------------

def linear_axis(dst, src, crop):
    """(i0, i1, w) of one axis, cell by cell: f = (d + 0.5) (n / dst) - 0.5 over the n = src - 2 crop inner cells."""
    n = src - 2 * crop
    i0, i1, w = [], [], []
    for d in range(dst):
        f = (d + 0.5) * (n / dst) - 0.5
        s = math.floor(f)
        t = f - s
        if s < 0:
            s, t = 0, 0.0
        if s >= n - 1:
            s, t = n - 1, 0.0
        i0.append(s + crop)
        i1.append(min(s + 1, n - 1) + crop)
        w.append(t)
    return np.asarray(i0, dtype=np.int32), np.asarray(i1, dtype=np.int32), np.asarray(w, dtype=np.float64).astype(np.float32)


def nearest_axis(out, mid, src, crop):
    """Composed nearest table of one axis: out <- mid (torch, fp32) <- the n = src - 2 crop inner cells (OpenCV, float64)."""
    n = src - 2 * crop
    inv = 1.0 / (mid / n)
    first = [min(math.floor(d * inv), n - 1) + crop for d in range(mid)]
    scale = np.float32(mid) / np.float32(out)
    second = [min(int(np.floor(np.float32(d) * scale)), mid - 1) for d in range(out)]
    return np.asarray([first[s] for s in second], dtype=np.int32)


def linear_tables(H, W, oh, ow, crop=(0, 0)):
    return linear_axis(oh, H, crop[0]) + linear_axis(ow, W, crop[1])


def nearest_tables(H, W, mid, out, crop=(0, 0)):
    return nearest_axis(out[0], mid[0], H, crop[0]), nearest_axis(out[1], mid[1], W, crop[1])


# ---- colour -------------------------------------------------------------------------------------------------------------------------

def blend64(frames, tables):
    """uint8 [n, H, W, 3] -> float64 [n, 3, oh, ow]: the bilinear blend with the fp32 weights widened, in float64 (exact to
    ~1e-13 grey levels; exact where the weights are dyadic)."""
    y0, y1, wy, x0, x1, wx = tables
    f = frames.astype(np.float64)
    wx64, wy64 = wx.astype(np.float64)[None, None, :, None], wy.astype(np.float64)[None, :, None, None]
    top = f[:, y0][:, :, x0] * (1 - wx64) + f[:, y0][:, :, x1] * wx64
    bot = f[:, y1][:, :, x0] * (1 - wx64) + f[:, y1][:, :, x1] * wx64
    return np.ascontiguousarray((top * (1 - wy64) + bot * wy64).transpose(0, 3, 1, 2))


def chain32(v, scale_rgb=255., mean=MEAN, std=STD):
    """The reference's normalisation (dataset.py:197, :202-205) on fp32 grey levels [n, 3, h, w], one rounded fp32 operation per
    step, constants rounded to fp32 once."""
    assert v.dtype == np.float32
    x = v / np.float32(255.0)
    x = x * np.float32(255.0)
    x = x / np.float32(scale_rgb)
    m = np.asarray(mean, dtype=np.float32)[None, :, None, None]
    s = np.asarray(std, dtype=np.float32)[None, :, None, None]
    x = (x - m) / s
    assert x.dtype == np.float32
    return x


def chain64(v, scale_rgb=255., mean=MEAN, std=STD):
    """The same chain in float64 with the SAME (fp32-rounded) constants: what the unquantised output is measured against."""
    m = np.asarray(mean, dtype=np.float32).astype(np.float64)[None, :, None, None]
    s = np.asarray(std, dtype=np.float32).astype(np.float64)[None, :, None, None]
    return (v.astype(np.float64) / 255.0 * 255.0 / np.float64(np.float32(scale_rgb)) - m) / s


def images_quantised(frames, tables, scale_rgb=255., mean=MEAN, std=STD):
    """-> (fp32 [n, 3, oh, ow], float64 blend): rint (half to even) of the float64 blend, then the fp32 chain."""
    v = blend64(frames, tables)
    return chain32(np.rint(v).astype(np.float32), scale_rgb, mean, std), v


def unquantised_bound(scale_rgb=255., mean=MEAN, std=STD):
    """13 fp32 roundings lie on the path of a value through the kernel (include/v3d.h: 4 per lerp, two lerps deep; 5 in the
    chain), each at most 2^-24 of its result, and no result exceeds the largest intermediate: 255 grey levels in the blend,
    255 / scale + max |mean| after the subtraction.  Taken all at that magnitude and carried through the division by the smallest
    std: 13 * 2^-24 * (255 / scale + max |mean|) / min std.  (The checker's own float64 error is 1e-9 of this.)"""
    return 13 * 2.0 ** -24 * (255.0 / scale_rgb + max(abs(m) for m in mean)) / min(std)


def near_tie(v64, margin=2e-3):
    """elements whose float64 grey level lies within `margin` of a half-integer"""
    return np.abs((v64 - np.floor(v64)) - 0.5) <= margin


# ---- depth --------------------------------------------------------------------------------------------------------------------------

def depths(depth_mm, tables):
    """uint16 [n, H, W] -> fp32 [n, oh, ow]: gather, / 1000 in fp32, > 65 -> 0"""
    ys, xs = tables
    d = depth_mm[:, ys][:, :, xs].astype(np.float32) / np.float32(1000.0)
    d[d > np.float32(65.0)] = 0
    return d


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------

def colour_frames(n, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)


def depth_frames(n, H, W, seed):
    """uint16 millimetres; a tenth of the pixels each hold 0, 65,000 (the largest valid depth), 65,001 and 65,535"""
    rng = np.random.default_rng(seed)
    d = rng.integers(300, 9000, size=(n, H, W), dtype=np.uint16)
    pick = rng.integers(0, 10, size=(n, H, W))
    for j, v in enumerate((0, 65000, 65001, 65535)):
        d[pick == j] = v
    return d


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _rodrigues(axis, angle):
    axis = axis / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


WALKS = {'gentle': (60, 11), 'jumps': (90, 12), 'short': (6, 13)}


def pose_walk(kind):
    """float64 [n, 4, 4] camera-to-world poses of a seeded random walk.  'gentle': ~3 cm and ~1.5 degrees a frame; 'jumps': the same
    with stalls of 12 frames (longer than the selectors' search_interval of 8 in the fixtures) and leaps of a metre; 'short': 6
    frames, fewer than the n_frames asked for."""
    n, seed = WALKS[kind]
    rng = np.random.default_rng(seed)
    poses = np.empty((n, 4, 4))
    P = np.eye(4)
    P[:3, :3] = _rodrigues(rng.normal(size=3), 0.7)
    P[:3, 3] = rng.normal(size=3)
    for i in range(n):
        poses[i] = P
        step, turn = 0.03, np.deg2rad(1.5)
        if kind == 'jumps':
            if 20 <= i < 32 or 60 <= i < 72:
                step, turn = 1e-4, 1e-5
            elif i in (40, 41, 75):
                step, turn = 1.0, np.deg2rad(25.)
        M = np.eye(4)
        M[:3, :3] = _rodrigues(rng.normal(size=3), turn * rng.uniform(0.5, 1.5))
        M[:3, 3] = rng.normal(size=3) * step
        P = P @ M
    return poses


SELECTORS = (('range', 'RangePoseDistSelector', (0.1, 0.3, 8)), ('best', 'BestPoseDistSelector', (0.225, 8)),
             ('next', 'NextPoseDistSelector', (0.15, 8)), ('neucon', 'NeuralReconSelector', (0.1, 15)),
             ('nth', 'EveryNthSelector', (3,)))


def selector_cases():
    """(key, walk, class name, constructor arguments, n_frames, seed_idx, np.random seed) of every selector fixture"""
    out = []
    for walk, (n, wseed) in WALKS.items():
        for tag, cls, args in SELECTORS:
            for n_frames in (4, 10, 100_000):
                for seed_idx in (None, 0, n // 2):
                    key = '%s_%s_%d_%s' % (walk, tag, n_frames, 'none' if seed_idx is None else seed_idx)
                    out.append((key, walk, cls, args, n_frames, seed_idx, 1000 + len(out)))
    return out


_K = np.array([[577.870605, 0., 319.5], [0., 577.870605, 239.5], [0., 0., 1.]])
# (key, H, W, new_h, new_w, crop)
PREPROCESS_CASES = (('a_crop', 480, 640, 256, 320, True), ('a_plain', 480, 640, 256, 320, False), ('b_plain', 480, 640, 240, 320, False),
                    ('b_crop', 480, 640, 240, 320, True), ('c_crop', 968, 1296, 480, 640, True), ('d_crop', 37, 53, 16, 24, True),
                    ('e_portrait', 640, 480, 256, 320, True), ('e_portrait_plain', 640, 480, 256, 320, False))


def intrinsics(H, W):
    """a ScanNet-like K scaled to an H x W frame (float64)"""
    K = _K.copy()
    K[0] *= W / 640.
    K[1] *= H / 480.
    return K


def transcribed_geometry(poses, img_idx, k):
    """The reference's lines for the edge window, the reference views and the camera tensors (dataset.py:130-137, :214-215),
    written as the loop they are: -> (ref_idx, ref_src_edges, rotmats, tvecs)."""
    import torch
    ref_idx = img_idx[k:-k]
    n_ref, per = ref_idx.shape[0], 2 * k + 1
    edges = torch.empty((2, n_ref * per), dtype=torch.long)
    for i in range(n_ref):
        edges[0, i * per:(i + 1) * per] = torch.ones(per) * (i + k)
        edges[1, i * per:(i + 1) * per] = torch.arange(i, i + per)
    rotmats = torch.from_numpy(poses[img_idx, :3, :3]).float().transpose(2, 1)
    tvecs = -torch.bmm(rotmats, torch.from_numpy(poses[img_idx, :3, 3, None]).float())[..., 0]
    return ref_idx, edges, rotmats @ torch.eye(3, dtype=torch.float32).T, tvecs
