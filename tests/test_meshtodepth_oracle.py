"""CPU: the NumPy checker of mesh rendering (tests/meshtodepth_oracle.py) against analysis, the condition on the inputs of
tests/test_meshtodepth_gpu.py (at most 2 % undecided pixels; the kernel's two rejections change no bit), and
mesh.read_triangle_mesh."""
import os

import numpy as np
import pytest
import torch

import meshtodepth_oracle as mo
from conftest import v3d

_cache = {}


def projections(K, poses):
    return v3d('tsdf').projection_matrices(torch.from_numpy(np.asarray(K, dtype=np.float32)),
                                           torch.from_numpy(np.asarray(poses, dtype=np.float32))).numpy()


def case_results(name, pixel_center=.5):
    """(case, P, fp32 restatement, float64 evaluation) of a GPU case, computed once per process."""
    key = (name, pixel_center)
    if key not in _cache:
        c = mo.gpu_cases()[name]
        P = projections(c['K'], c['poses'])
        _cache[key] = (c, P, mo.render32(c['verts'], c['tris'], P, c['h'], c['w'], pixel_center),
                       mo.render64(c['verts'], c['tris'], P, c['h'], c['w'], pixel_center))
    return _cache[key]


def agree(d32, r64):
    """The fp32 restatement against the float64 evaluation at decided pixels: coverage equal, depth within the bound."""
    d = r64['decided']
    assert ((d32 == 0) == (r64['depth'] == 0))[d].all()
    assert (np.abs(d32.astype(np.float64) - r64['depth']) <= r64['bound'])[d].all()


IDENT = np.eye(4, dtype=np.float32)[None]


def test_fma32_is_the_fused_operation():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(20000).astype(np.float32), rng.standard_normal(20000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.standard_normal(20000) * 1e-7)).astype(np.float32)
    got = mo.fma32(a, b, c)
    from fractions import Fraction
    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        err = abs(Fraction(float(got[i])) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)
    # a sum that lands on a float32 tie only after the float64 rounding: 1 + 2^-24 + 2^-60 must round up
    assert mo.fma32(np.float32([1.0]), np.float32([1.0 + 2.0 ** -23]), np.float32([0]))[0] == np.float32(1.0 + 2.0 ** -23)
    x = mo.fma32(np.float32([2.0 ** -30]), np.float32([2.0 ** -30]), np.float32([1.0 + 2.0 ** -23]) * np.float32(1))  # 1 + 2^-23 + 2^-60
    assert x[0] == np.float32(1.0 + 2.0 ** -23)
    tie = mo.fma32(np.float32([2.0 ** -12]), np.float32([2.0 ** -12]), np.float32([1.0]))                              # 1 + 2^-24: tie, to even
    assert tie[0] == np.float32(1.0)
    above = mo.fma32(np.float32([2.0 ** -12 + 2.0 ** -35]), np.float32([2.0 ** -12]), np.float32([1.0]))               # 1 + 2^-24 + 2^-47
    assert above[0] == np.float32(1.0 + 2.0 ** -23)


def test_fronto_parallel_quad():
    z0, K = 2.5, mo.intrinsics(20., 20., 16.3, 12.2)
    v, f = mo.quad((-0.5, -0.4, z0), (0.45, -0.4, z0), (0.45, 0.35, z0), (-0.5, 0.35, z0))
    P = projections(K[None], IDENT)
    d32, r64 = mo.render32(v, f, P, 24, 32), mo.render64(v, f, P, 24, 32)
    agree(d32, r64)
    u0, u1, v0, v1 = 20 * -0.5 / z0 + 16.3, 20 * 0.45 / z0 + 16.3, 20 * -0.4 / z0 + 12.2, 20 * 0.35 / z0 + 12.2
    px, py = np.meshgrid(np.arange(32) + .5, np.arange(24) + .5)
    inside = (px > u0 + 1e-3) & (px < u1 - 1e-3) & (py > v0 + 1e-3) & (py < v1 - 1e-3)
    outside = (px < u0 - 1e-3) | (px > u1 + 1e-3) | (py < v0 - 1e-3) | (py > v1 + 1e-3)
    assert inside.sum() > 20 and (d32[0][inside] > 0).all() and (d32[0][outside] == 0).all()      # no crack, the diagonal included
    hit = d32[0] > 0
    assert (np.abs(d32[0][hit].astype(np.float64) - z0) <= np.maximum(r64['bound'][0][hit], 2.0 ** -22 * z0)).all()
    # a square whose diagonal runs exactly through sample points: every sample on it is covered
    v, f = mo.quad((-1., -1., 2.), (1., -1., 2.), (1., 1., 2.), (-1., 1., 2.))
    d = mo.render32(v, f, projections(mo.intrinsics(16., 16., 8., 8.)[None], IDENT), 16, 16)[0]
    assert (np.diag(d)[1:-1] == 2.0).all() and (d[1:-1, 1:-1] == 2.0).all()


def test_tilted_plane_closed_form():
    # plane z = 3 + 0.5 x - 0.25 y; the ray through (px, py) is ((px - cx) / f, (py - cy) / f, 1) t
    f_, cx, cy = 25., 15.6, 11.9
    corners = [(x, y, 3 + 0.5 * x - 0.25 * y) for x, y in ((-3, -3), (3, -3), (3, 3), (-3, 3))]
    v, f = mo.quad(*corners)
    P = projections(mo.intrinsics(f_, f_, cx, cy)[None], IDENT)
    d32, r64 = mo.render32(v, f, P, 24, 32), mo.render64(v, f, P, 24, 32)
    agree(d32, r64)
    px, py = np.meshgrid(np.arange(32) + .5, np.arange(24) + .5)
    want = 3.0 / (1 - 0.5 * (px - cx) / f_ + 0.25 * (py - cy) / f_)
    X, Y = (px - cx) / f_ * want, (py - cy) / f_ * want
    inside = (np.abs(X) < 3 - 1e-3) & (np.abs(Y) < 3 - 1e-3)
    outside = (np.abs(X) > 3 + 1e-3) | (np.abs(Y) > 3 + 1e-3)
    assert inside.sum() > 400 and outside.sum() > 4
    assert (d32[0][inside] > 0).all() and (d32[0][outside] == 0).all()
    assert np.abs(r64['depth'][0] - want)[inside].max() < 1e-5           # the corners are fp32 numbers: not the exact plane
    assert np.abs(d32[0] - want)[inside].max() < 1e-5


def test_sphere_against_ray_intersection():
    c, r = np.array([0.1, -0.05, 3.0]), 1.0
    v, f = mo.icosphere(3, r, c)
    f_, cx, cy = 30., 16.2, 12.1
    P = projections(mo.intrinsics(f_, f_, cx, cy)[None], IDENT)
    d32, r64 = mo.render32(v, f, P, 24, 32), mo.render64(v, f, P, 24, 32)
    agree(d32, r64)
    px, py = np.meshgrid(np.arange(32) + .5, np.arange(24) + .5)
    ray = np.stack(((px - cx) / f_, (py - cy) / f_, np.ones_like(px)), axis=-1)
    a, b, cc = (ray * ray).sum(-1), -2 * (ray @ c), c @ c - r * r
    disc = b * b - 4 * a * cc
    t = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)                     # depth along z = t (the ray has z = 1)
    # the inscribed mesh lies inside the sphere by at most the sagitta of its longest edge
    edge = np.linalg.norm(v[f[:, 0]].astype(np.float64) - v[f[:, 1]], axis=1).max()
    sag = r - np.sqrt(r * r - edge * edge / 3)                            # circumradius of a triangle <= edge / sqrt(3)
    cosine = np.sqrt(np.maximum(disc, 0)) / (2 * a) / (r / np.sqrt(a))    # cos of the incidence angle at the sphere
    hit = d32[0] > 0
    well_inside = disc > 0.2 * b * b * 0 + 4 * a * 0.15                   # chord half-length^2 a > 0.15: away from the silhouette
    assert hit[well_inside].all() and (~hit[disc < 0]).all() and well_inside.sum() > 150
    err = d32[0].astype(np.float64) - t
    assert (err[well_inside] >= -1e-6).all()
    assert (err[well_inside] <= 1.05 * sag / np.maximum(cosine[well_inside], 1e-9) / np.sqrt(a[well_inside]) + 1e-6).all()


@pytest.mark.parametrize('pc,covered,empty', [(.5, 10, 9), (0., 11, 10)])
def test_pixel_center_convention(pc, covered, empty):
    """A quad whose left edge projects to u = 10.25: with samples at c + 0.5 column 10 (10.5) is the first covered one and
    column 9 (9.5) is empty; with samples at c the first is column 11 and column 10 (10.0) is empty."""
    z0 = 2.0
    x0 = (10.25 - 16.0) * z0 / 16.0
    v, f = mo.quad((x0, -5., z0), (5., -5., z0), (5., 5., z0), (x0, 5., z0))
    P = projections(mo.intrinsics(16., 16., 16., 12.)[None], IDENT)
    d = mo.render32(v, f, P, 24, 32, pixel_center=pc)[0]
    assert (d[:, covered:] == z0).all() and (d[:, :empty + 1] == 0).all()
    agree(mo.render32(v, f, P, 24, 32, pixel_center=pc), mo.render64(v, f, P, 24, 32, pixel_center=pc))


def test_floor_running_behind_the_camera():
    c, P, d32, r64 = case_results('floor_24x32')
    agree(d32, r64)
    fy, cy, fx, cx = 30., 10.25, 30., 15.75
    px, py = np.meshgrid(np.arange(32) + .5, np.arange(24) + .5)
    want = np.where(py > cy, fy / np.maximum(py - cy, 1e-9), 0.0)        # y = 1 at depth z: py = fy / z + cy
    seen = (want >= .05) & (want <= 20.0) & (np.abs((px - cx) / fx * want) < 10.0 - 1e-3)
    gone = (py < cy) | (want > 100.0) | (np.abs((px - cx) / fx * want) > 10.0 + 1e-3)
    assert seen.sum() > 300 and gone.sum() > 300
    assert (d32[0][gone] == 0).all()                                     # nothing above the horizon
    assert (np.abs(d32[0][seen] - want[seen]) <= 1e-5 * want[seen]).all()


def test_closed_box_from_inside():
    v, f = mo.box((-1.2, -0.9, -1.1), (1.3, 1.0, 1.4))
    poses = np.stack([mo.look_at((0.1, 0.05, -0.1), (1.0, 0.3, 0.9)), mo.look_at((0.2, -0.1, 0.3), (-1.0, -0.8, -0.2))])
    P = projections(np.repeat(mo.intrinsics(14., 13., 15.8, 12.3)[None], 2, axis=0), poses)
    d32, r64 = mo.render32(v, f, P, 24, 32), mo.render64(v, f, P, 24, 32)
    agree(d32, r64)
    assert (d32 > 0).all() and d32.max() < 3.5


@pytest.mark.parametrize('name', list(mo.gpu_cases()))
@pytest.mark.parametrize('pc', [.5, 0.])
def test_gpu_case_inputs_are_decidable(name, pc):
    """The condition on the inputs of the GPU tests: at most 2 % undecided pixels per case; the fp32 restatement agrees with the
    float64 evaluation where it is decided; and the kernel's two rejections (near-plane cull, widened bounding box) change no
    bit of the pure predicate's image."""
    c, P, d32, r64 = case_results(name, pc)
    share = mo.undecided_share(r64)
    print('%s pixel_center %.1f: undecided %.4f, covered %.3f' % (name, pc, share, float((d32 > 0).mean())))
    assert share <= mo.UNDECIDED_CAP
    agree(d32, r64)
    assert (d32 > 0).any()
    cons = mo.render32(c['verts'], c['tris'], P, c['h'], c['w'], pc, conservative=True)
    assert np.array_equal(cons.view(np.uint32), d32.view(np.uint32))


def test_skipped_triangles_and_status():
    v, f = mo.icosphere(1)
    bad = np.concatenate((f, [[0, 1, v.shape[0]], [2, -1, 3]])).astype(np.int32)
    keep, status = mo.usable_triangles(v, bad)
    assert status == 1 and keep.sum() == f.shape[0] and not keep[-2:].any()
    v2 = v.copy()
    v2[5, 1] = np.nan
    keep, status = mo.usable_triangles(v2, f)
    assert status == 2 and (~keep).sum() == (f == 5).any(axis=1).sum()
    P = projections(mo.intrinsics(20., 20., 16., 12.)[None], mo.look_at((0, 0, -3.), (0, 0, 0))[None])
    assert np.array_equal(mo.render32(v, bad, P, 24, 32), mo.render32(v, f, P, 24, 32))


def test_read_triangle_mesh(tmp_path):
    mesh = v3d('mesh')
    rng = np.random.default_rng(4)
    # the ScanNet layout, written by hand: float x y z, uchar red green blue alpha, faces of uchar count + int indices
    n_v, n_f = 9, 5
    rows = np.zeros(n_v, dtype=[('x', '<f4'), ('y', '<f4'), ('z', '<f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1'), ('alpha', 'u1')])
    for k in 'xyz':
        rows[k] = rng.standard_normal(n_v).astype(np.float32)
    for k in ('red', 'green', 'blue', 'alpha'):
        rows[k] = rng.integers(0, 256, n_v)
    faces = np.zeros(n_f, dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    faces['n'], faces['i'] = 3, rng.integers(0, n_v, (n_f, 3))
    head = ('ply\nformat binary_little_endian 1.0\ncomment VCGLIB generated\nelement vertex %d\nproperty float x\nproperty float y\n'
            'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nelement face %d\n'
            'property list uchar int vertex_indices\nend_header\n' % (n_v, n_f)).encode()
    path = os.path.join(str(tmp_path), 'scan_vh_clean_2.ply')
    with open(path, 'wb') as out:
        out.write(head + rows.tobytes() + faces.tobytes())
    m = mesh.read_triangle_mesh(path)
    assert isinstance(m, mesh.TriangleMesh) and not m.vertices.is_cuda
    assert m.vertices.dtype == torch.float32 and m.triangles.dtype == torch.int32 and m.vertex_colors_u8.dtype == torch.uint8
    assert np.array_equal(m.vertices.numpy(), np.stack((rows['x'], rows['y'], rows['z']), axis=1))
    assert np.array_equal(m.triangles.numpy(), faces['i'])
    assert np.array_equal(m.vertex_colors_u8.numpy(), np.stack((rows['red'], rows['green'], rows['blue']), axis=1))
    # a file of write_ply: the same as read_ply
    own = mesh.TriangleMesh(torch.from_numpy(rng.standard_normal((7, 3)).astype(np.float32)),
                            torch.from_numpy(rng.integers(0, 7, (4, 3)).astype(np.int32)),
                            torch.from_numpy(rng.integers(0, 256, (7, 3)).astype(np.uint8)))
    for tag, colours in (('c', own.vertex_colors_u8), ('n', None)):
        p2 = os.path.join(str(tmp_path), 'own_%s.ply' % tag)
        mesh.TriangleMesh(own.vertices, own.triangles, colours).write_ply(p2)
        verts, cols, tris = mesh.read_ply(p2)
        got = mesh.read_triangle_mesh(p2)
        assert np.array_equal(got.vertices.numpy().astype(np.float64), verts) and np.array_equal(got.triangles.numpy(), tris)
        assert (got.vertex_colors_u8 is None) == (cols is None)
        if cols is not None:
            assert np.array_equal(got.vertex_colors_u8.numpy(), cols)
    # what is not read says why
    for change, why in ((lambda b: b.replace(b'binary_little_endian', b'ascii'), 'binary_little_endian'),
                        (lambda b: b.replace(b'property float x', b'property int x'), 'float or double'),
                        (lambda b: b.replace(b'uchar int vertex_indices', b'uchar short vertex_indices'), 'indices'),
                        (lambda b: b[:-3], 'truncated'),
                        (lambda b: b.replace(b'ply\n', b'plx\n', 1), 'not a PLY')):
        p3 = os.path.join(str(tmp_path), 'bad.ply')
        with open(p3, 'wb') as out:
            out.write(change(head + rows.tobytes() + faces.tobytes()))
        with pytest.raises(ValueError, match=why):
            mesh.read_triangle_mesh(p3)
    quadf = faces.copy()
    quadf['n'][2] = 4
    with open(p3, 'wb') as out:
        out.write(head + rows.tobytes() + quadf.tobytes())
    with pytest.raises(ValueError, match='not a triangle'):
        mesh.read_triangle_mesh(p3)


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        return                                  # with a device the calls succeed: tests/test_meshtodepth_gpu.py
    lib_mod, m2d = v3d('_lib'), v3d('meshtodepth')
    v, f = mo.icosphere(0)
    holder = v3d('mesh').TriangleMesh(torch.from_numpy(v), torch.from_numpy(f))
    with pytest.raises(lib_mod.V3DLibraryError):
        m2d.Renderer(holder, 8, 8)
    with pytest.raises(lib_mod.V3DLibraryError):
        m2d.process_scene(holder, np.eye(4)[None], np.eye(3)[None], (8, 8))
    with pytest.raises(lib_mod.V3DLibraryError):
        m2d.mask_with_mesh(torch.zeros(1, 8, 8), holder, np.eye(4)[None], np.eye(3)[None])
