"""NumPy restatement of the device's volume bounds (3dvnet_amd/tsdf.py: volume_bounds_device; csrc/order_stats.hip), written
from include/v3d.h and independent of the kernel: the pinned fp32 back-projection (every NumPy float32 operation is rounded on
its own, as the kernel's are), the NaN-row drop, ``np.sort`` per axis, the float64 rank rule and the pinned finish of a
quantile.  ``np.sort`` may place -0.0 and +0.0 in either order: callers compare zeros as values.
"""
import numpy as np
import torch


def inverse_projections(K, poses):
    """K [N, 3, 3], poses [N, 4, 4] -> [N, 4, 4] float32: the inverse of [K [R | t]; 0 0 0 1], formed on the host the way the
    reference forms it (torch.bmm of K with a zero column and the pose, a row appended, torch's inverse)."""
    K, poses = torch.as_tensor(np.asarray(K)).float(), torch.as_tensor(np.asarray(poses)).float()
    K4 = torch.cat((K, torch.zeros((K.shape[0], 3, 1))), dim=2)
    P = torch.bmm(K4, poses)
    last = torch.tensor([[[0., 0., 0., 1.]]]).repeat(K.shape[0], 1, 1)
    return torch.cat((P, last), dim=1).inverse().numpy()


def backproject(depths, proj_inv):
    """depths [n, h, w], proj_inv [n, 4, 4] -> [n h w, 3] float32, view-major then row-major: inv = 1 / d; X_r = ((Pi[r][0] x +
    Pi[r][1] y) + Pi[r][2]) + Pi[r][3] inv; p_a = X_a / X_3."""
    d = np.asarray(depths, dtype=np.float32)
    Pi = np.asarray(proj_inv, dtype=np.float32).reshape(d.shape[0], 4, 4)
    n, h, w = d.shape
    y, x = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing='ij')
    x, y = x[None], y[None]
    with np.errstate(all='ignore'):
        inv = np.float32(1) / d
        X = []
        for r in range(4):
            c = [Pi[:, r, k].reshape(n, 1, 1) for k in range(4)]
            X.append(((c[0] * x + c[1] * y) + c[2]) + c[3] * inv)
        pts = np.stack([X[a] / X[3] for a in range(3)], axis=-1)
    assert pts.dtype == np.float32
    return pts.reshape(-1, 3)


def ranks(count, q):
    """-> (lo, hi, vi): float64 rule of include/v3d.h."""
    last = np.float64(count - 1)
    vi = np.float64(q) * last
    lo = min(max(np.floor(vi), 0.0), last)
    return int(lo), int(min(lo + 1, last)), vi


def order_stats(pts, qs):
    """pts [N, 3] float32 -> (count, stats [len(qs), 3, 2] float32): rows with a NaN dropped, then per axis the lo-th and hi-th
    smallest values; NaN everywhere when no row is left."""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    kept = pts[~np.isnan(pts).any(axis=1)]
    count = int(kept.shape[0])
    stats = np.full((len(qs), 3, 2), np.nan, dtype=np.float32)
    if count:
        srt = np.sort(kept, axis=0)
        for j, q in enumerate(qs):
            lo, hi, _ = ranks(count, q)
            stats[j, :, 0] = srt[lo]
            stats[j, :, 1] = srt[hi]
    return count, stats


def finish(count, pair, q):
    """The quantile from its two order statistics: t = q (N - 1) - lo; float32(a + (b - a) t) in float64; a when a == b."""
    lo, _, vi = ranks(count, q)
    a, b = np.float64(pair[0]), np.float64(pair[1])
    if a == b:
        return np.float32(a)
    with np.errstate(all='ignore'):
        return np.float32(a + (b - a) * (vi - np.float64(lo)))


def batch_bounds(count, stats, qs, vol_margin):
    """One batch's (lower [3], upper [3]) float32 from its statistics at qs = (1 - vol_prcnt, vol_prcnt)."""
    lo = np.array([finish(count, stats[0, a], qs[0]) for a in range(3)], dtype=np.float32)
    hi = np.array([finish(count, stats[1, a], qs[1]) for a in range(3)], dtype=np.float32)
    return torch.as_tensor(lo - vol_margin).float(), torch.as_tensor(hi + vol_margin).float()


def volume_bounds(depths, K, poses, vol_prcnt=.995, vol_margin=1.5, vox_res=.04, img_batch=100):
    """-> (origin [3] fp32 tensor, vol_max [3], vol_dim list): per batch the statistics of the back-projected depths, the pinned
    finish, -/+ vol_margin; empty batches skipped; running minimum / maximum; ValueError when no batch has a point."""
    depths = np.asarray(depths, dtype=np.float32)
    qs = (1 - vol_prcnt, vol_prcnt)
    origin = vol_max = None
    step = int(img_batch)
    for s in range(0, depths.shape[0], step):
        Pi = inverse_projections(np.asarray(K)[s:s + step], np.asarray(poses)[s:s + step])
        count, stats = order_stats(backproject(depths[s:s + step], Pi), qs)
        if count == 0:
            continue
        lo, hi = batch_bounds(count, stats, qs, vol_margin)
        origin = lo if origin is None else torch.minimum(origin, lo)
        vol_max = hi if vol_max is None else torch.maximum(vol_max, hi)
    if origin is None:
        raise ValueError('no depth map has a usable pixel')
    return origin, vol_max, ((vol_max - origin) / vox_res).int().tolist()


def same_bits(got, want):
    """Bit-exact equality of two float32 arrays, except that zeros compare as values (-0.0 == +0.0)."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    return bool(np.all((got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0))))
