"""Float64 checker of TSDF integration (3dvnet_amd/tsdf.py, csrc/tsdf.hip) -- a checker, not a product path.

It restates the integration semantics with elementwise float64 torch ops on the SAME fp32 inputs.  It starts from the fp32
world coordinates fl(fl(i * voxel_size) + origin), which are specifiable bit for bit; everything after them is float64.

Per (voxel, view) pair the verdict "valid" is  px >= 0, py >= 0, px < w, py < h, c2 > 0,  d = depth[py, px] > 0  and
dist = min((d - c2) / trunc_margin, 1) > -1,  (px, py) = round-half-even(c0 / c2, c1 / c2).  A pair is UNCERTAIN when an
fp32 evaluation may legitimately decide it the other way or read another texel:
  * u or v within the coordinate margin of x.5 while the point lies inside the image or at its border (up to the margin
    outside the half-texel frame) and not behind the camera;
  * c2 within the depth margin of 0;
  * dist within the margin of -1, i.e. |d - c2 + trunc_margin| < depth margin, for a pair that passed the tests before it.
Margins are fusion_oracle.margins: depth = 16 fp32 ulps of the largest depth, coordinates = max(1e-4, 16 * 2^-23 * w) pixels.
A voxel with any uncertain pair is left out of value comparisons; its weight is only bracketed.

UNCERTAIN_CAP: at most 0.5 % of the voxels a volume touches (weight > 0) may be uncertain.
"""
import numpy as np
import torch

import fusion_oracle

UNCERTAIN_CAP = 0.005


def world_axes(voxel_dim, voxel_size, origin):
    """The fp32 world coordinate of every index along each axis: two roundings, multiply then add."""
    vs = np.float32(voxel_size)
    o = np.asarray(origin, dtype=np.float32).reshape(3)
    return [(np.arange(int(n), dtype=np.float32) * vs + o[a]).astype(np.float32) for a, n in enumerate(voxel_dim)]


def integrate(voxel_dim, voxel_size, origin, trunc_margin, projections, depths, images=None, order=None, fill=-1.0):
    """All views (or those of `order`) into a fresh volume.  fp32 inputs, float64 arithmetic.
    -> dict: weight [n_vox] int64, tsdf [n_vox] f64 sum (`fill` where weight == 0), color [3, n_vox] f64 sums | None,
    tsdf_avg / color_avg (get_tsdf), uncertain [n_vox] bool, n_pairs_uncertain."""
    nx, ny, nz = (int(v) for v in voxel_dim)
    P = torch.as_tensor(np.asarray(projections, dtype=np.float32)).double().reshape(-1, 3, 4)
    D32 = torch.as_tensor(np.asarray(depths, dtype=np.float32))
    n, h, w = D32.shape
    D = D32.double().reshape(n, h * w)
    I = None if images is None else torch.as_tensor(np.asarray(images, dtype=np.float32)).double().reshape(n, 3, h * w)
    finite = D32[torch.isfinite(D32)]
    dm, cm = fusion_oracle.margins(finite if finite.numel() else torch.ones(1), w)
    tm = float(np.float32(trunc_margin))
    ax = [torch.from_numpy(a).double() for a in world_axes((nx, ny, nz), voxel_size, origin)]
    X, Y, Z = torch.meshgrid(ax[0], ax[1], ax[2], indexing='ij')
    X, Y, Z = X.reshape(-1), Y.reshape(-1), Z.reshape(-1)
    n_vox = X.numel()
    weight = torch.zeros(n_vox, dtype=torch.int64)
    tsdf = torch.zeros(n_vox, dtype=torch.float64)
    color = None if I is None else torch.zeros((3, n_vox), dtype=torch.float64)
    uncertain = torch.zeros(n_vox, dtype=torch.bool)
    n_pairs = 0
    for k in (range(n) if order is None else order):
        c0 = P[k, 0, 0] * X + P[k, 0, 1] * Y + P[k, 0, 2] * Z + P[k, 0, 3]
        c1 = P[k, 1, 0] * X + P[k, 1, 1] * Y + P[k, 1, 2] * Z + P[k, 1, 3]
        c2 = P[k, 2, 0] * X + P[k, 2, 1] * Y + P[k, 2, 2] * Z + P[k, 2, 3]
        u, v = c0 / c2, c1 / c2
        ok_uv = torch.isfinite(u) & torch.isfinite(v)
        uc = torch.where(ok_uv, u, torch.full_like(u, -1e9)).clamp(-1e9, 1e9)
        vc = torch.where(ok_uv, v, torch.full_like(v, -1e9)).clamp(-1e9, 1e9)
        px, py = torch.round(uc), torch.round(vc)                      # torch.round = half to even
        inview = (px >= 0) & (py >= 0) & (px < w) & (py < h) & (c2 > 0)
        idx = (py.clamp(0, h - 1) * w + px.clamp(0, w - 1)).long()
        d = D[k][idx]
        has_d = inview & (d > 0)                                       # a NaN depth fails
        dist = ((d - c2) / tm).clamp(max=1.0)
        valid = has_d & (dist > -1)
        half_x = ((uc - torch.floor(uc)) - 0.5).abs() < cm
        half_y = ((vc - torch.floor(vc)) - 0.5).abs() < cm
        frame = (uc > -0.5 - cm) & (uc < w - 0.5 + cm) & (vc > -0.5 - cm) & (vc < h - 0.5 + cm) & (c2 > -dm)
        unc = ((half_x | half_y) & frame) | (c2.abs() < dm) | (has_d & ((d - c2 + tm).abs() < dm))
        uncertain |= unc
        n_pairs += int(unc.sum())
        dv = torch.where(valid, dist, torch.zeros_like(dist))
        tsdf += dv
        weight += valid
        if color is not None:
            color += torch.where(valid[None], I[k][:, idx], torch.zeros((), dtype=torch.float64))
    seen = weight > 0
    wd = weight.double().clamp(min=1)
    tsdf = torch.where(seen, tsdf, torch.full_like(tsdf, fill))
    return dict(weight=weight, tsdf=tsdf, color=color, tsdf_avg=torch.where(seen, tsdf / wd, tsdf),
                color_avg=None if color is None else color / wd[None], uncertain=uncertain, n_pairs_uncertain=n_pairs)


def uncertain_share(res, touched=None):
    """Share of uncertain voxels among the touched ones (weight > 0 in `touched`, default the checker's own weights)."""
    t = res['weight'] > 0 if touched is None else torch.as_tensor(touched).reshape(-1) > 0
    return float((res['uncertain'] & t).sum()) / max(1, int(t.sum()))


def errors(res, tsdf_sum, color_sum=None, tsdf_avg=None, color_avg=None):
    """Largest |fp32 volume - checker| over the voxels that are not uncertain -> dict of floats (keys as given)."""
    keep = ~res['uncertain']
    out = {}
    for key, got in (('tsdf', tsdf_sum), ('color', color_sum), ('tsdf_avg', tsdf_avg), ('color_avg', color_avg)):
        if got is None or res[key] is None:
            continue
        got = torch.as_tensor(np.asarray(got, dtype=np.float64)).reshape(res[key].shape)
        out[key] = float((got - res[key]).abs()[..., keep].max())
    return out


def weight_mismatches(res, weight):
    """Voxels outside the uncertain set whose weight differs from the checker's."""
    got = torch.as_tensor(np.asarray(weight, dtype=np.float64)).reshape(-1).long()
    return int(((got != res['weight']) & ~res['uncertain']).sum())
