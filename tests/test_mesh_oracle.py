"""CPU: the marching-cubes case table (3dvnet_amd/csrc/mc_table.h against the rule of scripts/gen_mc_table.py), the NumPy checker
of mesh extraction (tests/mesh_oracle.py) against the reference-written fixtures (tests/golden/G_mesh_*.npz, written by
tests/golden/make_golden_mesh.py) bit for bit, the invariants of the checker's meshes, the PLY round trip and the host side
of the two C entry points.

Sphere (24^3, radius 8.3 about (11.3, 11.3, 11.3)): the checker's mesh encloses 2374.31 against 4/3 pi r^3 = 2395.10, a
deviation of 0.868 % (chords of a convex surface lie inside it); the test allows twice that, 1.74 %.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import mesh_oracle as mo
from conftest import ROOT, v3d

SPHERE_DEVIATION = 8.68e-3          # measured on the checker, see the module docstring
_cache = {}


def generator():
    if 'gen' not in _cache:
        spec = importlib.util.spec_from_file_location('gen_mc_table', os.path.join(ROOT, 'scripts', 'gen_mc_table.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cache['gen'] = mod
    return _cache['gen']


def golden(name):
    if name not in _cache:
        with np.load(os.path.join(ROOT, 'tests', 'golden', 'G_mesh_%s.npz' % name)) as f:
            _cache[name] = {k: f[k] for k in f.files}
    return _cache[name]


def sphere(n=24, r=8.3, c=11.3):
    g = np.mgrid[0:n, 0:n, 0:n].astype(np.float64)
    return (np.sqrt(((g - c) ** 2).sum(0)) - r).astype(np.float32)


def noise(shape=(9, 8, 7), seed=5):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_committed_table_is_the_generated_one():
    gen = generator()
    assert open(mo.HEADER).read() == gen.render()
    assert np.array_equal(mo.parse_header(), np.asarray(gen.rows()))


def test_table_cases_close_and_use_every_crossing_edge_once():
    gen = generator()
    edges = gen.cell_edges()
    ntri, tris = mo.table()
    total = 0
    for case in range(256):
        crossing = sorted(e for e, (p, q) in edges.items() if ((case >> p) & 1) != ((case >> q) & 1))
        loops = gen.loops(case)                                   # raises when a chain of segments does not close
        used = [e for L in loops for e in L]
        assert sorted(used) == crossing, case                     # every crossing edge exactly once, nothing else
        assert all(len(L) >= 3 and L[0] == min(L) for L in loops), case
        n = int(ntri[case])
        assert n == sum(len(L) - 2 for L in loops) <= 5, case
        assert (tris[case, :n] >= 0).all() and (tris[case, n:] == -1).all(), case
        assert sorted(set(tris[case, :n].reshape(-1).tolist())) == crossing, case
        total += n
    assert ntri[0] == 0 and ntri[255] == 0
    assert total == 820


@pytest.mark.parametrize('name', ['a', 'b'])
def test_checker_reproduces_the_reference_bit_for_bit(name):
    g = golden(name)
    out = mo.get_mesh(g['tsdf'], g['color'], float(g['voxel_size']), g['origin'])
    removed = np.setdiff1d(np.arange(out['n_all']), out['kept'])
    print('fixture %s: %d vertices, %d removed, %d triangles' % (name, out['n_all'], removed.shape[0], out['triangles'].shape[0]))
    assert removed.shape[0] > 0 and out['kept'].shape[0] > 0
    assert np.array_equal(removed, g['removed'])
    assert np.array_equal(out['triangles'], g['triangles'])
    assert np.array_equal(out['colors'], g['colors'])
    assert np.array_equal(bits(out['vertices']), bits(g['vertices']))
    # float64 second opinion on the positions, in index space: one subtraction without cancellation, one division, one add
    x64 = mo.marching_cubes(mo.clamp(g['tsdf']), np.float64)[0][out['kept']]
    x32 = mo.marching_cubes(mo.clamp(g['tsdf']))[0][out['kept']].astype(np.float64)
    assert (np.abs(x32 - x64) <= 2.0 ** -24 * (3 + np.abs(x64))).all()


def test_checker_point_cloud_reproduces_the_reference():
    g = golden('a')
    xyz, rgb = mo.point_cloud(g['tsdf'], g['color'], float(g['voxel_size']), g['origin'])
    assert xyz.shape == g['pc_xyz'].shape and np.array_equal(bits(xyz), bits(g['pc_xyz']))
    assert np.array_equal(rgb, g['pc_rgb'])


def test_checker_empty_mesh_rule():
    g = golden('c')
    for tag in ('pos', 'neg'):
        out = mo.get_mesh(g[tag + '_tsdf'], g[tag + '_color'], float(g['voxel_size']), g['origin'])
        assert out['vertices'].shape == (0, 3) and out['triangles'].shape == (0, 3) and out['colors'].shape == (0, 3)
        assert g[tag + '_vertices'].shape == (0, 3) and g[tag + '_triangles'].shape == (0, 3)
    assert mo.n_crossing_edges(g['neg_tsdf']) > 0                # the sign rule alone would emit vertices
    assert mo.point_cloud(g['neg_tsdf'], g['neg_color'], 0.05, g['origin'])[0].shape[0] == mo.n_crossing_edges(g['neg_tsdf'])


def test_sphere_is_a_closed_manifold_with_outward_normals():
    vol = sphere()
    v, f = mo.marching_cubes(vol)
    assert v.shape[0] == mo.n_crossing_edges(vol) and np.array_equal(np.unique(f), np.arange(v.shape[0]))
    assert mo.unbalanced_edges(f).shape[0] == 0 and mo.repeated_edges(f) == 0
    assert mo.euler_characteristic(v.shape[0], f) == 2
    vol_mesh, vol_true = mo.signed_volume(v, f), 4. / 3. * np.pi * 8.3 ** 3
    dev = abs(vol_mesh - vol_true) / vol_true
    print('sphere: %d vertices, %d triangles, volume %.2f against %.2f (deviation %.3e)' % (v.shape[0], f.shape[0], vol_mesh, vol_true, dev))
    assert vol_mesh > 0                                           # normals point towards positive values = outwards
    assert dev <= 2 * SPHERE_DEVIATION


def all_cases_volume(seed=9):
    """32 x 32 x 2 voxels: the cell at (2 i, 2 j, 0) has case 16 j + i, magnitudes are Gaussian noise.  (The 336 cells of a
    9 x 8 x 7 noise volume cannot hold all 256 cases: about 187 distinct ones are expected, 191 occur with the seed used here.)"""
    mag = np.abs(np.random.default_rng(seed).standard_normal((32, 32, 2))).astype(np.float32) + np.float32(0.01)
    vol = mag.copy()
    for case in range(256):
        i, j = case % 16, case // 16
        for c in range(8):
            if (case >> c) & 1:
                vol[2 * i + (c & 1), 2 * j + ((c >> 1) & 1), (c >> 2) & 1] *= -1
    return vol


def cases_of(vol):
    nx, ny, nz = vol.shape
    inside = vol < 0
    case = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int64)
    for c in range(8):
        ox, oy, oz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= inside[ox:nx - 1 + ox, oy:ny - 1 + oy, oz:nz - 1 + oz].astype(np.int64) << c
    return case


@pytest.mark.parametrize('which', ['noise', 'all_cases'])
def test_noise_is_closed_inside_and_every_case_occurs(which):
    vol = noise() if which == 'noise' else all_cases_volume()
    case = cases_of(vol)
    print('%s: %d distinct cases in %d cells' % (which, np.unique(case).shape[0], case.size))
    if which == 'all_cases':
        assert np.unique(case).shape[0] == 256
    v, f = mo.marching_cubes(vol)
    assert v.shape[0] == mo.n_crossing_edges(vol) and np.array_equal(np.unique(f), np.arange(v.shape[0]))
    open_edges = mo.unbalanced_edges(f)
    assert open_edges.shape[0] > 0 and mo.on_boundary_face(v, open_edges, vol.shape).all()
    assert f.shape[0] == int(mo.table()[0][case].sum())


def test_tilted_plane_is_open_only_on_boundary_faces():
    g = np.mgrid[0:12, 0:11, 0:10].astype(np.float64)
    vol = (g[0] * 0.3 + g[1] * 0.5 - g[2] * 0.81 - 1.234).astype(np.float32)
    v, f = mo.marching_cubes(vol)
    open_edges = mo.unbalanced_edges(f)
    assert f.shape[0] > 100 and open_edges.shape[0] > 0
    assert mo.on_boundary_face(v, open_edges, vol.shape).all()
    assert mo.repeated_edges(f) == 0
    # normals point towards positive values: along the gradient (0.3, 0.5, -0.81)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    assert (n @ np.array([0.3, 0.5, -0.81]) > 0).all()


def test_dimension_one_gives_vertices_but_no_cells():
    vol = noise((1, 9, 9), 6)
    v, f = mo.marching_cubes(vol)
    assert v.shape[0] == mo.n_crossing_edges(vol) > 0 and f.shape == (0, 3)


def test_ply_round_trip(tmp_path):
    mesh = v3d('mesh')
    g = golden('b')
    m = mesh.TriangleMesh(torch.from_numpy(g['vertices']), torch.from_numpy(g['triangles']), torch.from_numpy(g['colors']))
    assert torch.equal(m.vertex_colors, torch.from_numpy(g['colors']).float() / 255.) and m.points is m.vertices
    path = str(tmp_path / 'mesh.ply')
    m.write_ply(path)
    head = open(path, 'rb').read(400).split(b'end_header\n')[0].decode().split('\n')
    assert head[:3] == ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % g['vertices'].shape[0]]
    assert 'property double x' in head and 'property uchar red' in head and 'property list uchar int vertex_indices' in head
    v, c, f = mesh.read_ply(path)
    assert v.dtype == np.float64 and np.array_equal(v, g['vertices'].astype(np.float64))
    assert np.array_equal(c, g['colors']) and np.array_equal(f, g['triangles'])
    assert np.array_equal(mesh.read_ply_points(path), v)
    # no colours, no faces, no vertices
    plain = str(tmp_path / 'plain.ply')
    mesh.TriangleMesh(torch.from_numpy(g['vertices'])).write_ply(plain)
    v, c, f = mesh.read_ply(plain)
    assert np.array_equal(v, g['vertices'].astype(np.float64)) and c is None and f.shape == (0, 3)
    mesh.TriangleMesh().write_ply(plain)
    assert mesh.read_ply_points(plain).shape == (0, 3)
    with open(plain, 'wb') as out:
        out.write(b'ply\nformat ascii 1.0\nend_header\n')
    with pytest.raises(ValueError):
        mesh.read_ply(plain)


def test_no_cpu_fallback_and_no_instance_colouring():
    tsdf, lib_mod = v3d('tsdf'), v3d('_lib')
    t = tsdf.TSDF(0.04, torch.zeros(1, 3), torch.from_numpy(noise((4, 3, 2))))
    with pytest.raises(NotImplementedError):
        t.get_mesh(attribute='instance')
    with pytest.raises(lib_mod.V3DLibraryError):
        t.get_mesh()
    with pytest.raises(lib_mod.V3DLibraryError):
        v3d('mesh').extract(t.tsdf_vol, None, 0.04, [0., 0., 0.])


def test_host_validation_of_the_c_abi():
    """Errors that return before anything touches the device."""
    lib = v3d('_lib').load()
    one = ctypes.c_void_p(256)                            # never dereferenced: every call below fails first
    org = (ctypes.c_float * 3)(0., 0., 0.)
    count, extract, size = lib.v3d_mesh_count_f32, lib.v3d_mesh_extract_f32, lib.v3d_mesh_workspace_bytes
    big = 1 << 40
    need = size(4, 3, 2)
    assert need > 24 * 10 and size(0, 3, 2) == 0 and size(2048, 1024, 1024) == 0
    assert size(150, 128, 128) >= 150 * 128 * 128 * 10
    assert count(None, 4, 3, 2, 0, one, one, big, None) == -2 and b'null' in lib.v3d_last_error()
    assert count(one, 4, 3, 2, 0, None, one, big, None) == -2
    assert count(one, 4, 3, 2, 0, one, None, big, None) == -2
    assert count(one, 4, 3, 2, 2, one, one, big, None) == -2
    for dims in ((0, 3, 2), (4, -1, 2), (4, 3, 0), (2048, 1024, 1024), (65536, 65536, 1)):
        assert count(one, dims[0], dims[1], dims[2], 0, one, one, big, None) == -1, dims
    assert count(one, 4, 3, 2, 0, one, one, need - 1, None) == -3
    ok = lambda **kw: [kw.get(k, v) for k, v in (('tsdf', one), ('color', None), ('nx', 4), ('ny', 3), ('nz', 2), ('vs', 0.04),
                                                  ('org', org), ('mode', 0), ('verts', one), ('colors', None), ('v_cap', 5),
                                                  ('tris', one), ('f_cap', 5), ('ws', one), ('bytes', big), ('s', None))]
    assert extract(*ok(tsdf=None)) == -2
    assert extract(*ok(org=None)) == -2
    assert extract(*ok(ws=None)) == -2
    assert extract(*ok(verts=None)) == -2
    assert extract(*ok(tris=None)) == -2
    assert extract(*ok(mode=7)) == -2
    assert extract(*ok(color=one)) == -2 and b'together' in lib.v3d_last_error()
    assert extract(*ok(colors=one)) == -2
    for vs in (0.0, -0.04, float('nan'), float('inf')):
        assert extract(*ok(vs=vs)) == -2, vs
    assert extract(*ok(nz=0)) == -1
    assert extract(*ok(nx=65536, ny=65536)) == -1
    assert extract(*ok(v_cap=-1)) == -1
    assert extract(*ok(f_cap=-1)) == -1
    assert extract(*ok(bytes=need - 1)) == -3
    assert lib.v3d_version() == 9
