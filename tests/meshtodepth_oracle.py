"""NumPy checker of mesh rendering (3dvnet_amd/meshtodepth.py, csrc/meshrender.hip) -- a checker, not a product path.

Two evaluations of the semantics pinned in include/v3d.h (homogeneous rasterisation: q_i = P [X_i; 1]; A_0 = q_1 x q_2, A_1 =
q_2 x q_0, A_2 = q_0 x q_1; det = q_0 . A_0; per pixel e_i = A_i . (px, py, 1), s = e_0 + e_1 + e_2; a fragment iff the e_i
agree in sign (zero allowed) with s strictly of that sign and znear <= z = det / s <= zfar; depth = the smallest z, 0 for none):

``render32``   the fp32 restatement: explicit element-wise float32 operations in the stated order, one rounding each; the
               projection rows are FMA chains (``fma32``: exact product and sum in float64 brought to round-to-odd, then ONE
               rounding to float32 -- 53 >= 2 * 24 + 2 bits make that the correctly rounded fused result).  It tests EVERY
               triangle at EVERY pixel.  ``conservative=True`` adds the kernel's two rejections (a triangle wholly before the
               near plane; pixels outside the bounding box widened by one pixel of a triangle wholly behind it), which exact
               arithmetic implies; tests/test_meshtodepth_oracle.py asserts that they change no bit on any test input.

``render64``   float64 on the SAME fp32 inputs with a forward error bound on what an fp32 evaluation may return.  With u =
               2^-24 and g(k) = k u / (1 - k u), a value computed by k nested roundings differs from the exact one by at most
               g(k) times the same expression over absolute values (every leaf's contribution is multiplied by one (1 + d), |d|
               <= u, per rounding on its way to the root; in a product the two factors' counts add).  Counting roundings on
               the longest path:
                 q_i.c        mul, fma, fma, add                                  k = 4
                 A_i.c        two q (4 + 4), mul, sub                             k = 10
                 e_i          A_i.x (10), mul by px, add, add                     k = 13
                 s            e (13), add, add                                    k = 15
                 det          q_0.x (4) times A_0.x (10), mul, add, add           k = 17
               (px, py are the same fp32 numbers in both evaluations.)  Hence |e_i32 - e_i| <= be_i = g(13) eabs_i, |s32 - s| <=
               bs = g(15) sabs, |det32 - det| <= bd = g(17) detabs, and for the quotient, one more rounding,
                 |z32 - z| <= bz = (|det| + bd) / (|s| - bs) (1 + u) - |det| / |s|      (bs < |s|).
               The float64 evaluation's own error (2^-53 per operation) is covered by a factor 1 + 2^-20 on every bound.
               Underflow is not modelled: the test inputs stay far from the subnormal range.

A (pixel, triangle) pair is CERTAIN when it certainly has no fragment -- two edge values certainly of opposite strict sign, or
all three and s certainly of one strict sign with z certainly outside [znear, zfar] -- or certainly has one (all three and s
certainly of one strict sign, z certainly inside).  Any other pair is VAGUE: it may or may not have a fragment, at a depth within
bz of z when s is certainly non-zero.  A pixel is DECIDED when the nearest certain fragment is nearer than every other certain
or vague one by more than their two bounds (z_1 + bz_1 < z_k - bz_k) and no vague pair is without such a depth; a pixel with no
certain fragment is decided when it has no vague pair either.  A decided pixel's fp32 depth is 0 exactly when the checker's is,
and lies within bz_1 of it.  (A vague pair far behind the nearest fragment cannot change the minimum, which is why it does not
make the pixel undecided; every vague pair at or before it does.)

UNDECIDED_CAP: at most 2 % of the pixels of a test input may be undecided (a condition on the inputs, met by the checker alone).
"""
import numpy as np

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -20
UNDECIDED_CAP = 0.02


def g(k):
    return k * U / (1.0 - k * U) * SLACK


def fma32(a, b, c):
    """fmaf on float32 arrays: the exact product (48 bits) plus c in float64 with the sum brought to round-to-odd (TwoSum's error
    term says whether and in which direction the float64 sum is inexact), then one rounding to float32."""
    p = np.asarray(a, dtype=np.float32).astype(np.float64) * np.asarray(b, dtype=np.float32).astype(np.float64)
    c = np.asarray(c, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def project32(P, X):
    """P [3, 4], X [T, 3] fp32 -> q [T, 3] fp32: per row fl(fma(P2, Z, fma(P1, Y, fl(P0 X))) + P3)."""
    P = np.asarray(P, dtype=np.float32).reshape(3, 4)
    rows = []
    with np.errstate(invalid='ignore', over='ignore'):
        for r in range(3):
            acc = (P[r, 0] * X[:, 0]).astype(np.float32)
            acc = fma32(np.full_like(acc, P[r, 1]), X[:, 1], acc)
            acc = fma32(np.full_like(acc, P[r, 2]), X[:, 2], acc)
            rows.append((acc + P[r, 3]).astype(np.float32))
    return np.stack(rows, axis=1)


def cross(a, b):
    """Per component fl(fl(p) - fl(q)) in the arrays' own type."""
    return np.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), axis=1)


def cross_abs(a, b):
    """The expression of ``cross`` over absolute values: a b + c d."""
    return np.stack((a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]), axis=1)


def usable_triangles(verts, tris):
    """-> (mask of the triangles that are rendered, status word): index in [0, V) and finite vertices."""
    verts, tris = np.asarray(verts, dtype=np.float32).reshape(-1, 3), np.asarray(tris).reshape(-1, 3).astype(np.int64)
    in_range = ((tris >= 0) & (tris < verts.shape[0])).all(axis=1)
    finite = np.zeros(tris.shape[0], dtype=bool)
    finite[in_range] = np.isfinite(verts[tris[in_range]]).all(axis=(1, 2))
    return in_range & finite, (0 if in_range.all() else 1) | (0 if finite[in_range].all() else 2)


def pixel_grid(h, w, pixel_center):
    pc = np.float32(pixel_center)
    px = (np.arange(w, dtype=np.float32) + pc).astype(np.float32)
    py = (np.arange(h, dtype=np.float32) + pc).astype(np.float32)
    return np.tile(px, h)[None], np.repeat(py, w)[None]            # [1, h w] each, row major


def render32(verts, tris, projections, h, w, pixel_center=.5, znear=.05, zfar=100., conservative=False, chunk=2048):
    """-> depth [n, h, w] float32."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    tris = np.asarray(tris).reshape(-1, 3)
    P = np.asarray(projections, dtype=np.float32).reshape(-1, 3, 4)
    tris = tris[usable_triangles(verts, tris)[0]]
    zn, zf, pc = np.float32(znear), np.float32(zfar), np.float32(pixel_center)
    px, py = pixel_grid(h, w, pixel_center)
    col, row = np.tile(np.arange(w, dtype=np.float32), h)[None], np.repeat(np.arange(h, dtype=np.float32), w)[None]
    out = np.zeros((P.shape[0], h, w), dtype=np.float32)
    with np.errstate(all='ignore'):
        for k in range(P.shape[0]):
            best = np.full(h * w, np.inf, dtype=np.float32)
            for start in range(0, tris.shape[0], chunk):
                t = tris[start:start + chunk]
                q = [project32(P[k], verts[t[:, i]]) for i in range(3)]
                A = [cross(q[1], q[2]), cross(q[2], q[0]), cross(q[0], q[1])]
                det = ((q[0][:, 0] * A[0][:, 0] + q[0][:, 1] * A[0][:, 1]) + q[0][:, 2] * A[0][:, 2])[:, None]
                e = [((a[:, 0:1] * px + a[:, 1:2] * py) + a[:, 2:3]) for a in A]
                s = (e[0] + e[1]) + e[2]
                front = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0) & (s > 0)
                back = (e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0) & (s < 0)
                z = det / s
                frag = (front | back) & (z >= zn) & (z <= zf)
                if conservative:
                    near = np.stack([qi[:, 2] < zn for qi in q], axis=1)
                    finite = np.stack([np.isfinite(qi).all(axis=1) for qi in q], axis=1).all(axis=1)
                    culled = near.all(axis=1)
                    whole = near.any(axis=1) | ~finite
                    u = np.stack([qi[:, 0] / qi[:, 2] for qi in q], axis=1)
                    v = np.stack([qi[:, 1] / qi[:, 2] for qi in q], axis=1)
                    x0 = (np.floor(u.min(axis=1) - pc) - np.float32(1))[:, None]
                    x1 = (np.ceil(u.max(axis=1) - pc) + np.float32(1))[:, None]
                    y0 = (np.floor(v.min(axis=1) - pc) - np.float32(1))[:, None]
                    y1 = (np.ceil(v.max(axis=1) - pc) + np.float32(1))[:, None]
                    inbox = (col >= x0) & (col <= x1) & (row >= y0) & (row <= y1)
                    frag &= ~culled[:, None] & (whole[:, None] | inbox)
                best = np.minimum(best, np.where(frag, z, np.float32(np.inf)).min(axis=0, initial=np.float32(np.inf)))
            out[k] = np.where(np.isinf(best), np.float32(0), best).reshape(h, w)
    return out


def render64(verts, tris, projections, h, w, pixel_center=.5, znear=.05, zfar=100., chunk=2048):
    """-> dict: depth [n, h, w] float64 (0 for no fragment), bound [n, h, w] float64 (bz of the nearest fragment), decided
    [n, h, w] bool."""
    verts = np.asarray(verts, dtype=np.float32).reshape(-1, 3)
    tris = np.asarray(tris).reshape(-1, 3)
    P = np.asarray(projections, dtype=np.float32).reshape(-1, 3, 4).astype(np.float64)
    tris = tris[usable_triangles(verts, tris)[0]]
    zn, zf = float(np.float32(znear)), float(np.float32(zfar))
    px, py = (a.astype(np.float64) for a in pixel_grid(h, w, pixel_center))
    n = P.shape[0]
    depth, bound = np.zeros((n, h * w)), np.zeros((n, h * w))
    decided = np.zeros((n, h * w), dtype=bool)
    inf = np.inf
    with np.errstate(all='ignore'):
        for k in range(n):
            unsure = np.zeros(h * w, dtype=bool)
            best_z, best_b, best_low, second_low = (np.full(h * w, inf) for _ in range(4))
            for start in range(0, tris.shape[0], chunk):
                t = tris[start:start + chunk]
                X = [verts[t[:, i]].astype(np.float64) for i in range(3)]
                q = [x @ P[k, :, :3].T + P[k, :, 3] for x in X]
                qa = [np.abs(x) @ np.abs(P[k, :, :3]).T + np.abs(P[k, :, 3]) for x in X]
                A = [cross(q[1], q[2]), cross(q[2], q[0]), cross(q[0], q[1])]
                Aa = [cross_abs(qa[i], qa[j]) for i, j in ((1, 2), (2, 0), (0, 1))]
                det = (q[0] * A[0]).sum(axis=1)[:, None]
                bd = g(17) * (qa[0] * Aa[0]).sum(axis=1)[:, None]
                e = [a[:, 0:1] * px + a[:, 1:2] * py + a[:, 2:3] for a in A]
                ea = [a[:, 0:1] * np.abs(px) + a[:, 1:2] * np.abs(py) + a[:, 2:3] for a in Aa]
                pos = [e[i] > g(13) * ea[i] for i in range(3)]
                neg = [e[i] < -g(13) * ea[i] for i in range(3)]
                s = e[0] + e[1] + e[2]
                bs = g(15) * (ea[0] + ea[1] + ea[2])
                s_sure = np.abs(s) > bs
                one_sign = ((pos[0] & pos[1] & pos[2] & (s > 0)) | (neg[0] & neg[1] & neg[2] & (s < 0))) & s_sure
                mixed = (pos[0] | pos[1] | pos[2]) & (neg[0] | neg[1] | neg[2])
                z = det / s
                bz = np.where(s_sure, (np.abs(det) + bd) / (np.abs(s) - bs) * (1 + U) * SLACK - np.abs(z), inf)
                inside = one_sign & (z - bz >= zn) & (z + bz <= zf)
                outside = one_sign & ((z + bz < zn) | (z - bz > zf))
                vague = ~(inside | outside | mixed)
                unsure |= (vague & ~s_sure).any(axis=0)
                if t.shape[0] == 0:
                    continue
                zin = np.where(inside, z, inf)
                low = np.where(inside | vague, z - bz, inf)            # a vague pair counts as a fragment that may be there
                arg = zin.argmin(axis=0)
                cols = np.arange(h * w)
                cz = zin[arg, cols]
                got = np.isfinite(cz)                                  # the chunk has a certain fragment at the pixel
                cb, clow = np.where(got, bz[arg, cols], 0.0), np.where(got, low[arg, cols], inf)
                low[arg[got], cols[got]] = inf
                csec = low.min(axis=0)
                better = cz < best_z
                second_low = np.where(better, np.minimum(np.minimum(second_low, best_low), csec),
                                      np.minimum(np.minimum(second_low, clow), csec))
                best_z, best_b, best_low = np.where(better, cz, best_z), np.where(better, cb, best_b), np.where(better, clow, best_low)
            hit = np.isfinite(best_z)
            depth[k] = np.where(hit, best_z, 0.0)
            bound[k] = np.where(hit, best_b, 0.0)
            decided[k] = ~unsure & np.where(hit, best_z + best_b < second_low, np.isinf(second_low))
    return dict(depth=depth.reshape(n, h, w), bound=bound.reshape(n, h, w), decided=decided.reshape(n, h, w))


def undecided_share(res):
    return 1.0 - float(res['decided'].mean())


# ---------------------------------------------------------------------------------------------------------------------------
# geometry and cameras of the tests

def icosphere(level, radius=1.0, center=(0., 0., 0.)):
    """20 * 4^level triangles, no degenerate one -> (verts [V, 3] fp32, tris [F, 3] int32)."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = np.asarray(v) * radius + np.asarray(center, dtype=np.float64)
    return verts.astype(np.float32), np.asarray(f, dtype=np.int32)


def box(lo, hi):
    """Closed axis-aligned box, 12 triangles."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    v = np.asarray([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)])
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7),
         (1, 7, 3)]
    return v.astype(np.float32), np.asarray(f, dtype=np.int32)


def quad(p00, p10, p11, p01):
    return np.asarray([p00, p10, p11, p01], dtype=np.float32), np.asarray([(0, 1, 2), (0, 2, 3)], dtype=np.int32)


def merge(*meshes):
    verts, tris, base = [], [], 0
    for v, f in meshes:
        verts.append(v)
        tris.append(f + base)
        base += v.shape[0]
    return np.concatenate(verts).astype(np.float32), np.concatenate(tris).astype(np.int32)


def look_at(eye, target, up=(0., -1., 0.)):
    """World -> camera pose [4, 4] fp32 (camera looks along +z, x right, y down)."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(-up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack((x, y, z))
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R, -R @ eye
    return pose.astype(np.float32)


def intrinsics(fx, fy, cx, cy):
    return np.asarray([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)


def floor_case():
    """A floor at y = 1 under an identity camera, running from behind the camera (z = -5) over z = 0 exactly and z = 0.02 <
    znear to z = 20: three quads.  K puts the horizon at py = cy = 10.25, between two sample rows."""
    rows = [-5.0, 0.0, 0.02, 20.0]
    v = np.asarray([[x, 1.0, z] for z in rows for x in (-10.0, 10.0)], dtype=np.float32)
    f = []
    for i in range(3):
        a, b, c, d = 2 * i, 2 * i + 1, 2 * i + 3, 2 * i + 2
        f += [(a, b, c), (a, c, d)]
    return v, np.asarray(f, dtype=np.int32), intrinsics(30., 30., 15.75, 10.25)[None], np.eye(4, dtype=np.float32)[None], 24, 32


def orbit(n, radius, target=(0., 0., 0.), tilt=0.35, phase=0.4):
    return np.stack([look_at((target[0] + radius * np.cos(phase + 2.1 * i) * np.cos(tilt), target[1] - radius * np.sin(tilt) * (1 + .3 * i),
                              target[2] + radius * np.sin(phase + 2.1 * i) * np.cos(tilt)), target) for i in range(n)])


def gpu_cases():
    """name -> dict(verts, tris, K [n, 3, 3], poses [n, 4, 4], h, w): the inputs of tests/test_meshtodepth_gpu.py (cases 1-4)."""
    cases = {}
    for tag, (h, w) in (('24x32', (24, 32)), ('17x41', (17, 41))):
        K = np.repeat(intrinsics(0.9 * w, 0.85 * w, w / 2 - 0.3, h / 2 + 0.2)[None], 3, axis=0)
        v, f = icosphere(2, 1.0, (0.1, -0.05, 0.2))
        cases['icosphere_' + tag] = dict(verts=v, tris=f, K=K, poses=orbit(3, 3.0, (0.1, -0.05, 0.2)), h=h, w=w)
        v, f = box((-0.7, -0.5, -0.6), (0.6, 0.8, 0.5))
        cases['cube_' + tag] = dict(verts=v, tris=f, K=K, poses=orbit(3, 3.2, tilt=0.5, phase=0.9), h=h, w=w)
    # two triangles that fill the image (a wall of 2000 m at z = 4) and a small tetrahedron in front of it; the second camera
    # stands 7 cm before the wall, every corner behind its near plane, with a focal length of 2 * 10^5 pixels: the corners
    # project some 3 * 10^9 pixels outside the image, beyond what an int holds, so only a clamp taken in float keeps the box
    wall = quad((-1000.3, -1000.1, 4.0), (1000.2, -1000.4, 4.0), (1000.1, 1000.3, 4.0), (-1000.2, 1000.2, 4.0))
    tet = (np.asarray([(0.0, 0.0, 2.0), (0.5, 0.1, 2.2), (0.1, 0.6, 2.1), (0.3, 0.3, 1.7)], dtype=np.float32),
           np.asarray([(0, 1, 2), (0, 1, 3), (1, 2, 3), (0, 2, 3)], dtype=np.int32))
    v, f = merge(wall, tet)
    close = np.eye(4, dtype=np.float32)                       # faces the wall squarely: all four corners 7 cm before the camera plane
    close[:3, 3] = (-0.3, 0.2, -3.93)
    poses = np.stack([look_at((0.2, 0.1, 0.0), (0.25, 0.2, 4.0)), close, look_at((-1.0, 0.5, 0.5), (0.2, 0.3, 2.0))])
    K = np.stack([intrinsics(60., 58., 31.7, 24.4), intrinsics(2.0e5, 1.9e5, 31.7, 24.4), intrinsics(60., 58., 31.7, 24.4)])
    cases['wall_48x64'] = dict(verts=v, tris=f, K=K, poses=poses, h=48, w=64)
    v, f, K, poses, h, w = floor_case()
    cases['floor_24x32'] = dict(verts=v, tris=f, K=K, poses=poses, h=h, w=w)
    # 20 480 triangles seen from 15 cm before the surface by two cameras that only turn about their own centre (no translation: the
    # absolute-value expressions of the bound stay close to the values).  The near cap fills the image with triangles of a few
    # pixels; the far hemisphere lies behind it with triangles far below a pixel, most of which cover no sample.
    v, f = icosphere(5, 1.0, (0.05, -0.03, 1.15))
    turn = np.eye(4, dtype=np.float32)
    turn[0, 0] = turn[2, 2] = np.float32(np.cos(0.25))
    turn[0, 2], turn[2, 0] = np.float32(np.sin(0.25)), -np.float32(np.sin(0.25))
    cases['sphere20480_16x20'] = dict(verts=v, tris=f, K=np.repeat(intrinsics(10., 9.5, 9.8, 8.3)[None], 2, axis=0),
                                      poses=np.stack([np.eye(4, dtype=np.float32), turn]), h=16, w=20)
    return cases
