"""Checkers of TSDF resampling (3dvnet_amd/tsdf.py: TSDF.transform, csrc/tsdf_resample.hip) -- checkers, not a product path.

Two evaluations of the arithmetic include/v3d.h pins, written once and run in two number formats:

  * ``plan(..., dtype=np.float32)``  the fp32 restatement: every operation rounded to fp32 on its own, the three rows of the
    transform as FMA chains (meshtodepth_oracle.fma32).  The device is compared with it bit for bit.
  * ``plan(..., dtype=np.float64)``  the float64 checker.  It starts from the fp32 world coordinates fl(fl(i * voxel_size) +
    origin), which are specifiable bit for bit, as tests/tsdf_oracle.py does; everything after them is float64.

An output voxel is UNCERTAIN when an fp32 route may legitimately decide otherwise than the float64 one:
  * some u_a within ``margin`` voxels of x.5 while the point lies inside the source volume or within half a voxel (plus the
    margin) of it: the nearest pick may differ;
  * some |g_a| within the margin (brought to voxels: (D_a - 1) / 2 per unit of g) of 1: the outside verdict may differ.
The trilinear value is continuous in the coordinate, so it makes no voxel uncertain.  MARGIN = 1e-4 voxels, far above the fp32
rounding of a coordinate (a few 1e-6 voxels at the tested sizes).  UNCERTAIN_CAP (tsdf_oracle): at most 0.5 % of the output
voxels.  A fixture whose every step up to g is exact (integer shift, power-of-two voxel size) is checked with margin 0: there
the verdicts are equal on every voxel.
"""
import numpy as np

from meshtodepth_oracle import fma32
from tsdf_oracle import UNCERTAIN_CAP, world_axes  # noqa: F401  (UNCERTAIN_CAP is part of this module's interface)

MARGIN = 1e-4


def _row(m, wx, wy, wz, dtype):
    """Row of the transform times [world; 1]: fp32 = fl(fma(m2, z, fma(m1, y, fl(m0 x))) + m3)."""
    if dtype == np.float32:
        acc = (m[0] * wx).astype(np.float32)
        acc = fma32(np.full_like(acc, m[1]), wy, acc)
        acc = fma32(np.full_like(acc, m[2]), wz, acc)
        return (acc + m[3]).astype(np.float32)
    return m[0] * wx + m[1] * wy + m[2] * wz + m[3]


def plan(src_dim, voxel_size, src_origin, matrix, align_corners, voxel_dim, dst_origin, dtype=np.float32, margin=MARGIN):
    """Where every output voxel reads.  -> dict: g, u [3, n] (dtype), outside [n] bool, nearest [n] int64 (flat source index,
    -1 out of bounds), tap_idx [8, n] int64 (-1 outside), tap_w [8, n] (dtype), uncertain [n] bool (float64 plans only)."""
    D = [int(v) for v in src_dim]
    T = dtype
    vs = T(np.float32(voxel_size))
    so = np.asarray(src_origin, dtype=np.float32).reshape(3).astype(T)
    M = np.asarray(matrix, dtype=np.float32).reshape(-1)[:12].reshape(3, 4).astype(T)
    ax = world_axes(voxel_dim, voxel_size, dst_origin)                # fp32, both plans start here
    W = [w.reshape(-1).astype(T) for w in np.meshgrid(ax[0], ax[1], ax[2], indexing='ij')]
    g, u = [], []
    with np.errstate(invalid='ignore', over='ignore'):
        for a in range(3):
            t = _row(M[a], W[0], W[1], W[2], T)
            c = (t - so[a]) / vs
            ga = (T(2) * c) / T(D[a] - 1) - T(1)
            g1 = ga + T(1)
            ua = (g1 / T(2)) * T(D[a] - 1) if align_corners else ((g1 * T(D[a])) - T(1)) / T(2)
            assert ga.dtype == T and ua.dtype == T
            g.append(ga)
            u.append(ua)
        outside = (np.abs(g[0]) >= 1) | (np.abs(g[1]) >= 1) | (np.abs(g[2]) >= 1)
        r = [np.rint(x) for x in u]                                    # half to even
        inb = np.ones(r[0].shape, dtype=bool)
        for a in range(3):
            inb &= (r[a] >= 0) & (r[a] <= D[a] - 1)
        ri = [np.where(inb, x, 0).astype(np.int64) for x in r]
        nearest = np.where(inb, (ri[0] * D[1] + ri[1]) * D[2] + ri[2], -1)
        w, p = [], []
        for a in range(3):
            f = np.floor(u[a])
            f1 = f + T(1)
            w.append(((f1 - u[a]).astype(T), (u[a] - f).astype(T)))
            ok0, ok1 = (f >= 0) & (f <= D[a] - 1), (f1 >= 0) & (f1 <= D[a] - 1)
            p.append((np.where(ok0, np.where(ok0, f, 0).astype(np.int64), -1), np.where(ok1, np.where(ok1, f1, 0).astype(np.int64), -1)))
        tap_idx, tap_w = [], []
        for k in range(8):
            bx, by, bz = k >> 2, (k >> 1) & 1, k & 1
            ok = (p[0][bx] >= 0) & (p[1][by] >= 0) & (p[2][bz] >= 0)
            tap_idx.append(np.where(ok, (p[0][bx] * D[1] + p[1][by]) * D[2] + p[2][bz], -1))
            tap_w.append(((w[2][bz] * w[1][by]).astype(T) * w[0][bx]).astype(T))
    out = dict(g=np.stack(g), u=np.stack(u), outside=outside, nearest=nearest, tap_idx=np.stack(tap_idx), tap_w=np.stack(tap_w),
               dtype=T, n=int(outside.size))
    if T == np.float64:
        frame = np.ones(outside.shape, dtype=bool)
        half = np.zeros(outside.shape, dtype=bool)
        edge = np.zeros(outside.shape, dtype=bool)
        for a in range(3):
            frame &= (u[a] > -0.5 - margin) & (u[a] < D[a] - 0.5 + margin)
            half |= np.abs((u[a] - np.floor(u[a])) - 0.5) < margin
            edge |= np.abs(np.abs(g[a]) - 1) * (D[a] - 1) / 2 < margin
        out['uncertain'] = (half & frame) | edge
    return out


def nearest(pl, vol):
    """[C, ...] or [...] source volume of any dtype -> [C, n] the nearest pick in the volume's own type, zero padding."""
    v = np.asarray(vol)
    v = v.reshape(-1, int(np.prod(v.shape[-3:])))
    got = v[:, np.maximum(pl['nearest'], 0)]
    return np.where(pl['nearest'][None] >= 0, got, np.zeros((), dtype=v.dtype))


def trilinear(pl, vol):
    """fp32 source volume -> [C, n] in the plan's dtype: the sum over the taps inside of fl(value * weight), in tap order, every
    addition rounded."""
    T = pl['dtype']
    v = np.asarray(vol, dtype=np.float32)
    v = v.reshape(-1, int(np.prod(v.shape[-3:]))).astype(T)
    acc = np.zeros((v.shape[0], pl['n']), dtype=T)
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(8):
            idx = pl['tap_idx'][k]
            term = (v[:, np.maximum(idx, 0)] * pl['tap_w'][k][None]).astype(T)
            acc = np.where(idx[None] >= 0, (acc + term).astype(T), acc)
    return acc


def tsdf(pl, vol):
    """The tsdf rule: the nearest value; where its magnitude is < 1 the trilinear one; 1 where the voxel is outside."""
    T = pl['dtype']
    v = nearest(pl, np.asarray(vol, dtype=np.float32))[0].astype(T)
    v = np.where(np.abs(v) < 1, trilinear(pl, vol)[0], v)
    return np.where(pl['outside'], T(1), v)


def fill_outside(pl, values, fill):
    """``values`` [C, n] with ``fill`` where the voxel is outside (the reference's semseg = -1, mask_outside = True)."""
    return np.where(pl['outside'][None], np.asarray(fill, dtype=values.dtype), values)


def uncertain_share(pl64):
    return float(pl64['uncertain'].sum()) / pl64['n']


def max_error(pl64, got, want):
    """Largest |got - want| over the voxels that are not uncertain; got / want [C, n] or [n]."""
    keep = ~pl64['uncertain']
    d = np.abs(np.asarray(got, dtype=np.float64).reshape(-1, pl64['n']) - np.asarray(want, dtype=np.float64).reshape(-1, pl64['n']))
    return float(d[:, keep].max()) if keep.any() else 0.0
