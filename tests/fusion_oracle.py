"""Float64 checker of multi-view depth fusion (3dvnet_amd/fusion.py, csrc/fusion.hip) -- a checker, not a product path.

It restates the fusion semantics with elementwise float64 torch ops on the SAME fp32 inputs and, because the operation is a
chain of hard decisions, also says which decisions an fp32 evaluation may legitimately take the other way.

Per (pixel, source) pair the verdict "valid" is  z > 1e-4  and  0 <= u <= w-1  and  0 <= v <= h-1  and  |z - z_s| < z_thresh,
z_s = the texel at round-half-even(u, v).  A pair is UNCERTAIN when a quantity lies within a margin of the boundary that
decides it and the other side of that boundary would give the other verdict:
  * | |z - z_s| - z_thresh | < depth margin;
  * u or v within the coordinate margin of 0 / w-1 / h-1;
  * u or v within the coordinate margin of x.5 and the neighbouring texel's depth gives the other verdict;
  * z within the depth margin of 1e-4.
Margins: depth = 16 fp32 ulps of the scene's largest depth; coordinates = max(1e-4, 16 * 2^-23 * w) pixels (an fp32 chain of
this length is off by a few ulps of u; 16 leaves room).

Per pixel: n_lo <= n_valid <= n_hi = the counts without / with the uncertain pairs.  The MASK is ambiguous when
n_lo < n_consistent_thresh <= n_hi, the SOURCE SET when n_lo < n_hi.

One more flag, for the comparison of fused POINTS only: a pair that may be valid whose u or v lies within the coordinate
margin of x.5 while the neighbouring texel holds a different depth.  Its verdict can be certain (both texels pass) and yet
the sample it contributes depends on which texel an fp32 evaluation reads -- with 4 cm of noise that moves the fused point by
millimetres, not ulps.  Such pixels are `sample_amb`; the tests leave them out of the point comparison together with the
source-set-ambiguous ones, under the same cap.
"""
import importlib

import numpy as np
import torch

Z_MIN = float(np.float32(1e-4))


def margins(depths, w):
    dmax = float(torch.as_tensor(depths).max())
    return 16.0 * float(np.spacing(np.float32(dmax))), max(1e-4, 16.0 * 2.0 ** -23 * w)


def scene(n_img, size, seed, yaw_step_deg, sigma, zero_frac=0.03):
    """Seeded fusion inputs: ring cameras of 3dvnet_amd.synthetic, analytic box-room depths + N(0, sigma), a fraction of
    the pixels zeroed (masked predictions), blocky uint8 colours.  -> depths [N,h,w] f32, images [N,h,w,3] u8, poses, K."""
    syn = importlib.import_module('3dvnet_amd.synthetic')
    rot, tvec, K = syn.make_cameras(n_img, size, seed=seed, yaw_step_deg=yaw_step_deg)
    d = syn.ray_box_depth(rot, tvec, K, size, size)
    g = torch.Generator().manual_seed(seed + 1000)
    d = d + sigma * torch.randn(d.shape, generator=g)
    d = torch.where(torch.rand(d.shape, generator=g) < zero_frac, torch.zeros_like(d), d).float()
    poses = torch.eye(4).repeat(n_img, 1, 1)
    poses[:, :3, :3] = rot
    poses[:, :3, 3] = tvec
    yy, xx = torch.meshgrid(torch.arange(size[0]), torch.arange(size[1]), indexing='ij')
    bx, by = xx // 8, yy // 8                                  # 8 x 8 blocks of one colour: the fixture files stay small
    chan = [torch.stack([(bx * m0 + by * m1 + i * m2) % 256 for i in range(n_img)]) for m0, m1, m2 in
            ((37, 91, 53), (59, 17, 101), (7, 113, 29))]
    images = torch.stack(chan, -1).to(torch.uint8)
    return d, images, poses.float(), K.float()


def check_view(depths, poses, K, r, srcs, z_thresh, n_consistent_thresh, depth_margin=None, coord_margin=None):
    """Reference view `r` against the sources `srcs` (in order).  All inputs fp32 tensors; arithmetic float64.
    -> dict: pts [hw, 3] f64 (sources chosen by the float64 verdicts), n [hw], n_lo, n_hi, keep, mask_amb, set_amb,
    sample_amb (bool [hw])."""
    depths = torch.as_tensor(depths)
    n_img, h, w = depths.shape
    dm, cm = margins(depths, w)
    dm = dm if depth_margin is None else depth_margin
    cm = cm if coord_margin is None else coord_margin
    zt = float(np.float32(z_thresh))
    D = depths.double().reshape(n_img, h * w)
    P, Kd = torch.as_tensor(poses).double(), torch.as_tensor(K).double()
    Kinv, Pinv = torch.inverse(Kd), torch.inverse(P)

    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
    d = D[r]
    pix = torch.stack((xx.reshape(-1) * d, yy.reshape(-1) * d, d), 0)
    X = Pinv[r, :3, :3] @ (Kinv[r] @ pix) + Pinv[r, :3, 3:4]

    acc = X.clone()
    n = torch.zeros(h * w, dtype=torch.int64)
    n_lo, n_hi = n.clone(), n.clone()
    sample_amb = torch.zeros(h * w, dtype=torch.bool)
    for s in srcs:
        q = Kd[s] @ (P[s, :3, :3] @ X + P[s, :3, 3:4])
        z = q[2]
        u, v = q[0] / z, q[1] / z
        u = torch.where(torch.isfinite(u), u, torch.full_like(u, -1e9))
        v = torch.where(torch.isfinite(v), v, torch.full_like(v, -1e9))
        cz, near_z = z > Z_MIN, (z - Z_MIN).abs() < dm
        cx = (u >= 0) & (u <= w - 1)
        cy = (v >= 0) & (v <= h - 1)
        near_x = (u.abs() < cm) | ((u - (w - 1)).abs() < cm)
        near_y = (v.abs() < cm) | ((v - (h - 1)).abs() < cm)
        uc, vc = u.clamp(-2, w + 1), v.clamp(-2, h + 1)
        ix0, iy0 = torch.round(uc), torch.round(vc)               # torch.round = half to even
        half_x = ((uc - torch.floor(uc)) - 0.5).abs() < cm
        half_y = ((vc - torch.floor(vc)) - 0.5).abs() < cm
        ixa = torch.floor(uc) + torch.ceil(uc) - ix0              # the other neighbour (only used where half_x)
        iya = torch.floor(vc) + torch.ceil(vc) - iy0

        def texel(ix, iy):
            ok = (ix >= 0) & (ix <= w - 1) & (iy >= 0) & (iy <= h - 1)
            idx = (iy.clamp(0, h - 1) * w + ix.clamp(0, w - 1)).long()
            return torch.where(ok, D[s][idx], torch.zeros_like(z))

        zs = texel(ix0, iy0)
        cd = (z - zs).abs() < zt
        pt_d = cd | (((z - zs).abs() - zt).abs() < dm)          # the depth test may come out true
        pf_d = ~cd | (((z - zs).abs() - zt).abs() < dm)         # ... or false
        other = torch.zeros_like(cd)                              # a neighbouring texel with another depth is in reach
        for ix, iy, en in ((ixa, iy0, half_x), (ix0, iya, half_y), (ixa, iya, half_x & half_y)):
            za = texel(ix, iy)
            ca = (z - za).abs() < zt
            na = ((z - za).abs() - zt).abs() < dm
            pt_d = pt_d | (en & (ca | na))
            pf_d = pf_d | (en & (~ca | na))
            other = other | (en & (za != zs))
        valid = cz & cx & cy & cd
        may_true = (cz | near_z) & (cx | near_x) & (cy | near_y) & pt_d
        may_false = (~cz | near_z) | (~cx | near_x) | (~cy | near_y) | pf_d
        n += valid
        n_hi += may_true
        n_lo += ~may_false
        sample_amb |= may_true & other
        # X_s = R^T (K^-1 [u z_s, v z_s, z_s] - t)
        Xs = P[s, :3, :3].T @ (Kinv[s] @ torch.stack((u * zs, v * zs, zs), 0) - P[s, :3, 3:4])
        acc += torch.where(valid[None], Xs, torch.zeros_like(Xs))
    assert bool((n_lo <= n).all()) and bool((n <= n_hi).all())
    t = int(n_consistent_thresh)
    return dict(pts=(acc / (n + 1).double()[None]).T.contiguous(), n=n, n_lo=n_lo, n_hi=n_hi, keep=n >= t,
                mask_amb=(n_lo < t) & (t <= n_hi), set_amb=n_lo < n_hi, sample_amb=sample_amb)


def check_scene(depths, poses, K, z_thresh, n_consistent_thresh, refs=None, src_lists=None):
    """check_view for the references `refs` (default: all) against all other views (or src_lists[r]); results stacked
    along a leading reference axis."""
    n_img = torch.as_tensor(depths).shape[0]
    refs = list(range(n_img)) if refs is None else list(refs)
    out = []
    for k, r in enumerate(refs):
        srcs = [s for s in range(n_img) if s != r] if src_lists is None else list(src_lists[k])
        out.append(check_view(depths, poses, K, r, srcs, z_thresh, n_consistent_thresh))
    return {key: torch.stack([o[key] for o in out]) for key in out[0]}


def dense_from_compact(fused, all_valid, stride=1):
    """Rows of a (view, pixel)-ordered compact list (every `stride`-th row stored) -> (dense [n, hw, 3] float64 with NaN where
    nothing is stored, has [n, hw] bool)."""
    all_valid = np.asarray(all_valid)
    n = all_valid.shape[0]
    flat = np.flatnonzero(all_valid.reshape(-1))[::stride]
    dense = np.full((all_valid.size, 3), np.nan)
    dense[flat] = np.asarray(fused, dtype=np.float64)
    has = np.zeros(all_valid.size, dtype=bool)
    has[flat] = True
    return dense.reshape(n, -1, 3), has.reshape(n, -1)


def shares(res):
    """-> (share of mask-ambiguous pixels, share of pixels left out of the point / n_valid comparison)."""
    tot = float(res['n'].numel())
    return float(res['mask_amb'].sum()) / tot, float((res['set_amb'] | res['sample_amb']).sum()) / tot


MASK_CAP, SET_CAP = 0.02, 0.10
