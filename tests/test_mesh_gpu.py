"""GPU: mesh extraction (3dvnet_amd/tsdf.py TSDF.get_mesh / get_tsdf(point_cloud=True) / tsdf_mesh_metrics -> 3dvnet_amd/mesh.py ->
v3d_mesh_count_f32 / v3d_mesh_extract_f32, csrc/mesh.hip) against the reference-written fixtures (tests/golden/G_mesh_*.npz)
and the NumPy checker (tests/mesh_oracle.py).  Every test runs the HIP path through the C ABI.

Counts, triangle indices, colours and the kept / removed sets are compared for equality.  Positions: the arithmetic is pinned
(include/v3d.h), so the bits are expected to equal the checker's / the reference's; the hard bound behind that expectation is,
in index space, |x - x64| <= 2^-24 (3 + |x64|) (one subtraction without cancellation, one division, one addition: half an ulp
each of a quotient <= 1 and a sum <= |x64| + 1) and in world space the two further half-ulps of the multiply and the add.

Measured on one MI355X: no position differs in bits from the fp32 restatement or the reference's arrays in any test (fixtures a, b,
the six noise volumes raw and scaled, two spheres: 42 716 vertices / 85 428 triangles); largest error / hard bound 0.83.  Wall time
of the module's 14 tests: 5.4 s.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import mesh_oracle as mo
from conftest import ROOT, v3d
from test_mesh_oracle import all_cases_volume, bits, golden, noise

pytestmark = pytest.mark.gpu
H = 2.0 ** -24
_cache = {}


def tsdf_case_a():
    """The inputs of tests/golden/T_tsdf_a.npz and the colours the TSDF branch feeds."""
    if 'tsdf_a' not in _cache:
        with np.load(os.path.join(ROOT, 'tests', 'golden', 'T_tsdf_a.npz')) as f:
            t = {k: f[k] for k in f.files}
        _cache['tsdf_a'] = (t, torch.from_numpy(t['images'])[..., [2, 1, 0]].permute(0, 3, 1, 2).float().contiguous())
    return _cache['tsdf_a']


def device_mesh(dev, vol, color, voxel_size, origin):
    tsdf = v3d('tsdf')
    vols = {} if color is None else {'color': torch.from_numpy(np.ascontiguousarray(color)).to(dev)}
    t = tsdf.TSDF(voxel_size, torch.as_tensor(origin, dtype=torch.float32).view(1, 3).to(dev),
                  torch.from_numpy(np.ascontiguousarray(vol)).to(dev), vols)
    m = t.get_mesh()
    assert isinstance(m, v3d('mesh').TriangleMesh) and m.vertices.is_cuda and m.triangles.dtype == torch.int32
    return (m.vertices.cpu().numpy(), m.triangles.cpu().numpy(), None if m.vertex_colors_u8 is None else m.vertex_colors_u8.cpu().numpy())


def check_positions(tag, got, want32, vol, kept, voxel_size, origin):
    """Prints the number of rows whose bits differ from the fp32 restatement, asserts the hard bound against float64, then
    bit equality."""
    x64 = mo.marching_cubes(mo.clamp(vol), np.float64)[0][kept]
    vs = float(np.float32(voxel_size))
    org = np.asarray(origin, dtype=np.float32).astype(np.float64).reshape(1, 3)
    w64 = x64 * vs + org
    bound = (H * (3 + np.abs(x64)) * vs + H * np.abs(x64 * vs) + H * np.abs(w64)) * (1 + 2.0 ** -20)
    err = np.abs(got.astype(np.float64) - w64)
    differ = int((bits(got) != bits(want32)).any(axis=1).sum())
    print('%s: %d vertices, %d rows differ in bits from the fp32 restatement, largest error / bound %.3f'
          % (tag, got.shape[0], differ, float((err / bound).max()) if got.shape[0] else 0.0))
    assert (err <= bound).all()
    assert differ == 0


@pytest.mark.parametrize('name', ['a', 'b'])
def test_fixtures_through_get_mesh(cuda, name):
    g = golden(name)
    vs, org = float(g['voxel_size']), g['origin']
    v, f, c = device_mesh(cuda, g['tsdf'], g['color'], vs, org)
    n_all = g['vertices'].shape[0] + g['removed'].shape[0]
    kept = np.setdiff1d(np.arange(n_all), g['removed'])
    print('fixture %s: %d of %d vertices kept, %d triangles' % (name, v.shape[0], n_all, f.shape[0]))
    assert v.shape == g['vertices'].shape and f.shape == g['triangles'].shape
    assert np.array_equal(f, g['triangles'])
    assert np.array_equal(c, g['colors'])
    check_positions('fixture %s' % name, v, g['vertices'], g['tsdf'], kept, vs, org)
    # the kept / removed sets: every vertex (point-cloud mode removes none) at the kept rows is the mesh's vertex list
    every, _, _ = v3d('mesh').extract(torch.from_numpy(g['tsdf']).to(cuda), None, vs, org, v3d('mesh').MODE_POINT_CLOUD)
    every = every.cpu().numpy()
    assert every.shape[0] == n_all and np.array_equal(bits(every[kept]), bits(v))
    # without a colour volume: the same geometry, no colours
    v2, f2, c2 = device_mesh(cuda, g['tsdf'], None, vs, org)
    assert c2 is None and np.array_equal(bits(v2), bits(v)) and np.array_equal(f2, f)


def test_fixture_c_empty_mesh_rule(cuda):
    g = golden('c')
    for tag in ('pos', 'neg'):
        v, f, c = device_mesh(cuda, g[tag + '_tsdf'], g[tag + '_color'], float(g['voxel_size']), g['origin'])
        assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)
    # point-cloud mode knows no empty-mesh rule
    xyz, rgb, tri = v3d('mesh').extract(torch.from_numpy(g['neg_tsdf']).to(cuda), torch.from_numpy(g['neg_color']).to(cuda),
                                        float(g['voxel_size']), g['origin'], v3d('mesh').MODE_POINT_CLOUD)
    want_xyz, want_rgb = mo.point_cloud(g['neg_tsdf'], g['neg_color'], float(g['voxel_size']), g['origin'])
    assert want_xyz.shape[0] > 0 and tri.shape == (0, 3)
    assert np.array_equal(bits(xyz.cpu().numpy()), bits(want_xyz)) and np.array_equal(rgb.cpu().numpy(), want_rgb)


VOLUMES = {'9x8x7': lambda: noise((9, 8, 7), 5), '5x4x131': lambda: noise((5, 4, 131), 11), '2x2x2': lambda: noise((2, 2, 2), 12),
           '1x9x9': lambda: noise((1, 9, 9), 6), '9x1x1': lambda: noise((9, 1, 1), 13), 'all_cases': all_cases_volume}


@pytest.mark.parametrize('which', list(VOLUMES))
def test_noise_volumes_against_the_checker(cuda, which):
    """Raw Gaussian noise (values beyond +-1: the clamp makes -1 / +1 neighbours, so the bad-vertex rule removes vertices) and
    the same noise scaled into (-0.9, 0.9) (nothing is removed: the invariants of a marching-cubes mesh hold on the device
    output)."""
    raw = VOLUMES[which]()
    rng = np.random.default_rng(3)
    color = rng.uniform(-30, 290, (3,) + raw.shape).astype(np.float32)
    vs, org = 0.04, [0.25, -1.5, 3.0]
    for tag, vol in (('raw', raw), ('scaled', np.clip(raw * np.float32(0.3), -0.9, 0.9).astype(np.float32))):
        want = mo.get_mesh(vol, color, vs, org)
        v, f, c = device_mesh(cuda, vol, color, vs, org)
        print('%s %s: %d of %d vertices kept, %d triangles' % (which, tag, v.shape[0], want['n_all'], f.shape[0]))
        assert v.shape == want['vertices'].shape and f.shape == want['triangles'].shape
        assert np.array_equal(f, want['triangles']) and np.array_equal(c, want['colors'])
        check_positions('%s %s' % (which, tag), v, want['vertices'], vol, want['kept'], vs, org)
        if min(raw.shape) == 1:
            assert f.shape == (0, 3)
        if tag == 'scaled':
            assert v.shape[0] == mo.n_crossing_edges(vol) == want['n_all']
            if f.shape[0]:
                assert np.array_equal(np.unique(f), np.arange(v.shape[0]))           # every vertex is used
                idx = (v.astype(np.float64) - np.asarray(org, dtype=np.float32).astype(np.float64)) / float(np.float32(vs))
                open_edges = mo.unbalanced_edges(f)
                on_face = (np.abs(idx[open_edges[:, 0]] - idx[open_edges[:, 1]]) < 1e-4) & \
                          ((np.abs(idx[open_edges[:, 0]]) < 1e-4) | (np.abs(idx[open_edges[:, 0]] - (np.asarray(vol.shape) - 1)) < 1e-4))
                assert on_face.any(axis=1).all()                                     # open only in boundary faces of the volume


def test_nan_and_negative_zero_are_outside(cuda):
    vol = np.clip(noise((6, 5, 7), 21) * np.float32(0.3), -0.9, 0.9).astype(np.float32)
    vol[2, 2, 3] = np.nan
    vol[3, 1, 4] = -0.0
    vol[4, 3, 2] = 0.0
    want = mo.get_mesh(vol, None, 0.05, [0., 0., 0.])
    v, f, _ = device_mesh(cuda, vol, None, 0.05, [0., 0., 0.])
    assert want['n_all'] == mo.n_crossing_edges(vol) and np.isnan(want['vertices']).any()
    assert np.array_equal(f, want['triangles'])
    assert np.array_equal(v, want['vertices'], equal_nan=True)


def test_point_cloud_mode_and_get_tsdf_attribute(cuda):
    mesh, tsdf = v3d('mesh'), v3d('tsdf')
    g = golden('a')
    vs, org = float(g['voxel_size']), g['origin']
    xyz, rgb, tri = mesh.extract(torch.from_numpy(g['tsdf']).to(cuda), torch.from_numpy(g['color']).to(cuda), vs, org,
                                 mesh.MODE_POINT_CLOUD)
    want_xyz, want_rgb = mo.point_cloud(g['tsdf'], g['color'], vs, org)
    assert tri.shape == (0, 3) and xyz.shape == g['pc_xyz'].shape
    assert np.array_equal(bits(xyz.cpu().numpy()), bits(want_xyz)) and np.array_equal(rgb.cpu().numpy(), want_rgb)
    assert np.array_equal(bits(xyz.cpu().numpy()), bits(g['pc_xyz'])) and np.array_equal(rgb.cpu().numpy(), g['pc_rgb'])   # the reference's
    # get_tsdf(point_cloud=True) from the inputs of T_tsdf_a: the reference's key and shape; the default is unchanged
    t, cols = tsdf_case_a()
    fus = tsdf.TSDFFusion([int(v) for v in t['voxel_dim']], float(t['voxel_size']), t['origin'].tolist(), float(t['trunc_ratio']), cuda)
    fus.integrate_batch(t['projections'], t['depths'], cols)
    plain = fus.get_tsdf()
    assert sorted(plain.attribute_vols) == ['color', 'weight'] and plain.attributes == {}
    out = fus.get_tsdf(point_cloud=True)
    assert sorted(out.attribute_vols) == ['color', 'tsdf_point_cloud', 'weight']
    assert torch.equal(out.tsdf_vol, plain.tsdf_vol) and torch.equal(out.attribute_vols['color'], plain.attribute_vols['color'])
    pc = out.attribute_vols['tsdf_point_cloud']
    w_xyz, w_rgb = mo.point_cloud(out.tsdf_vol.cpu().numpy(), out.attribute_vols['color'].cpu().numpy(), float(t['voxel_size']), t['origin'])
    assert pc.dim() == 2 and pc.shape == (w_xyz.shape[0], 6) and pc.dtype == torch.float64 and pc.shape[0] > 1000
    assert abs(pc.shape[0] - g['pc_xyz'].shape[0]) <= 0.05 * g['pc_xyz'].shape[0]
    pc = pc.cpu().numpy()
    assert np.array_equal(pc[:, :3], w_xyz.astype(np.float64)) and np.array_equal(pc[:, 3:], w_rgb.astype(np.float64))
    # a volume without colour attaches nothing, as the reference's does
    nc = tsdf.TSDFFusion((4, 3, 2), 0.1, (0., 0., 0.), 3, cuda, color=False)
    assert sorted(nc.get_tsdf(point_cloud=True).attribute_vols) == ['weight']


def two_spheres():
    x = np.arange(150, dtype=np.float32)[:, None, None]
    y = np.arange(128, dtype=np.float32)[None, :, None]
    z = np.arange(128, dtype=np.float32)[None, None, :]
    d1 = np.sqrt((x - 60.3) ** 2 + (y - 61.7) ** 2 + (z - 58.9) ** 2) - 41.2
    d2 = np.sqrt((x - 97.6) ** 2 + (y - 70.2) ** 2 + (z - 71.4) ** 2) - 35.7
    return (np.minimum(d1, d2) * np.float32(0.125)).astype(np.float32)


def test_two_spheres_scan_across_many_workgroups(cuda):
    """150 x 128 x 128 voxels (9 600 workgroups; the scans span many rocPRIM blocks): every vertex and triangle against the
    checker, closed and manifold, and ten launches with identical bits."""
    mesh = v3d('mesh')
    vol = two_spheres()
    vs, org = 0.04, [0.5, -1.0, 2.0]
    want = mo.get_mesh(vol, None, vs, org)
    dvol = torch.from_numpy(vol).to(cuda)
    v, _, f = mesh.extract(dvol, None, vs, org)
    vh, fh = v.cpu().numpy(), f.cpu().numpy()
    print('two spheres: %d vertices, %d triangles' % (vh.shape[0], fh.shape[0]))
    assert want['n_all'] == want['kept'].shape[0] > 40000
    assert np.array_equal(fh, want['triangles'])
    check_positions('two spheres', vh, want['vertices'], vol, want['kept'], vs, org)
    assert mo.unbalanced_edges(fh).shape[0] == 0 and mo.repeated_edges(fh) == 0
    assert mo.euler_characteristic(vh.shape[0], fh) == 2
    assert mo.signed_volume(vh, fh) > 0
    for _ in range(10):
        v2, _, f2 = mesh.extract(dvol, None, vs, org)
        assert torch.equal(v2.view(torch.int32), v.view(torch.int32)) and torch.equal(f2, f)


def test_error_codes_and_capacities(cuda):
    lib_mod = v3d('_lib')
    lib = lib_mod.load()
    g = golden('b')
    nx, ny, nz = g['tsdf'].shape
    vol = torch.from_numpy(g['tsdf']).to(cuda)
    col = torch.from_numpy(g['color']).to(cuda)
    org = (ctypes.c_float * 3)(*[float(x) for x in g['origin']])
    s = lib_mod.stream_ptr(cuda)
    need = lib.v3d_mesh_workspace_bytes(nx, ny, nz)
    ws = torch.zeros(need, dtype=torch.uint8, device=cuda)
    counts = torch.full((2,), -7, dtype=torch.int32, device=cuda)
    count = lib.v3d_mesh_count_f32
    assert count(vol.data_ptr(), nx, ny, nz, 0, counts.data_ptr(), ws.data_ptr(), need - 1, s) == -3
    assert count(None, nx, ny, nz, 0, counts.data_ptr(), ws.data_ptr(), need, s) == -2
    assert count(vol.data_ptr(), nx, ny, nz, 0, None, ws.data_ptr(), need, s) == -2
    assert count(vol.data_ptr(), nx, ny, nz, 0, counts.data_ptr(), None, need, s) == -2
    assert count(vol.data_ptr(), nx, ny, nz, 3, counts.data_ptr(), ws.data_ptr(), need, s) == -2
    assert count(vol.data_ptr(), 0, ny, nz, 0, counts.data_ptr(), ws.data_ptr(), need, s) == -1
    assert count(vol.data_ptr(), 65536, 65536, 1, 0, counts.data_ptr(), ws.data_ptr(), need, s) == -1
    with pytest.raises(lib_mod.V3DLibraryError, match='V3D_ERR_WORKSPACE_TOO_SMALL'):
        lib_mod.check(count(vol.data_ptr(), nx, ny, nz, 0, counts.data_ptr(), ws.data_ptr(), 16, s), 'v3d_mesh_count_f32')
    torch.cuda.synchronize()
    assert counts.tolist() == [-7, -7] and int(ws.sum()) == 0             # none of the refused calls touched anything
    assert count(vol.data_ptr(), nx, ny, nz, 0, counts.data_ptr(), ws.data_ptr(), need, s) == 0
    n_v, n_f = counts.tolist()
    assert (n_v, n_f) == (g['vertices'].shape[0], g['triangles'].shape[0])
    # capacities below the counts: the rows that fit are written, nothing behind them
    cap_v, cap_f = n_v - 5, n_f - 7
    verts = torch.full((n_v, 3), -5.0, device=cuda)
    cols = torch.full((n_v, 3), 77, dtype=torch.uint8, device=cuda)
    tris = torch.full((n_f, 3), -9, dtype=torch.int32, device=cuda)
    extract = lambda **kw: lib.v3d_mesh_extract_f32(*[kw.get(k, d) for k, d in (
        ('tsdf', vol.data_ptr()), ('color', col.data_ptr()), ('nx', nx), ('ny', ny), ('nz', nz), ('vs', float(g['voxel_size'])), ('org', org),
        ('mode', 0), ('verts', verts.data_ptr()), ('colors', cols.data_ptr()), ('v_cap', cap_v), ('tris', tris.data_ptr()),
        ('f_cap', cap_f), ('ws', ws.data_ptr()), ('bytes', need), ('s', s))])
    assert extract(bytes=need - 1) == -3
    assert extract(tsdf=None) == -2 and extract(verts=None) == -2 and extract(tris=None) == -2 and extract(colors=None) == -2
    assert extract(vs=0.0) == -2 and extract(nz=-1) == -1 and extract(v_cap=-1) == -1
    torch.cuda.synchronize()
    assert bool((verts == -5.0).all()) and bool((tris == -9).all())
    assert extract() == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(verts[:cap_v].cpu().numpy()), bits(g['vertices'][:cap_v])) and bool((verts[cap_v:] == -5.0).all())
    assert np.array_equal(cols[:cap_v].cpu().numpy(), g['colors'][:cap_v]) and bool((cols[cap_v:] == 77).all())
    assert np.array_equal(tris[:cap_f].cpu().numpy(), g['triangles'][:cap_f]) and bool((tris[cap_f:] == -9).all())
    with pytest.raises(NotImplementedError):
        v3d('tsdf').TSDF(0.04, torch.zeros(1, 3), vol).get_mesh(attribute='instance')


def test_tsdf_mesh_metrics_end_to_end(cuda):
    """From the inputs of T_tsdf_a to the metrics record.  The ground truth is the checker's mesh of the device's volume moved
    by a fixed offset; the expected record is metrics3d.eval_clouds on the checker's vertices, compared for equality as
    tests/test_metrics3d_gpu.py compares depth_3d_metrics."""
    tsdf, m3 = v3d('tsdf'), v3d('metrics3d')
    t = tsdf_case_a()[0]
    rec = dict(depth_preds=t['depths'], rotmats=t['poses'][:, :3, :3], tvecs=t['poses'][:, :3, 3], K=t['K'])
    kw = dict(vox_res=float(t['voxel_size']), trunc_ratio=float(t['trunc_ratio']), vol_prcnt=float(t['bounds_vol_prcnt']),
              vol_margin=float(t['bounds_vol_margin']), img_batch=int(t['bounds_img_batch']))
    vol = tsdf.fuse_preds_tsdf(rec, t['images'], device=cuda, **kw)
    want = mo.get_mesh(vol.tsdf_vol.cpu().numpy(), vol.attribute_vols['color'].cpu().numpy(), vol.voxel_size, vol.origin.cpu().numpy())
    assert 1000 < want['vertices'].shape[0] < want['n_all']
    gt = want['vertices'] + np.array([[0.01, -0.02, 0.015]], dtype=np.float32)
    pred, _, n_pred = m3.voxel_down_sample(torch.from_numpy(want['vertices']).to(cuda), 0.02)
    trgt, _, n_trgt = m3.voxel_down_sample(torch.from_numpy(gt).to(cuda), 0.02)
    expect = dict(zip(m3.KEYS, m3.eval_clouds(pred[:int(n_pred)], trgt[:int(n_trgt)], 0.05).cpu().tolist()), n=6)
    got, mesh = tsdf.tsdf_mesh_metrics(rec, t['images'], gt, return_mesh=True, device=cuda, **kw)
    print('tsdf_mesh_metrics: %s' % got)
    assert got == expect and list(got) == list(m3.KEYS) + ['n']
    assert 0 < got['acc'] < 0.05 and got['prec'] > 0.9
    assert np.array_equal(bits(mesh.vertices.cpu().numpy()), bits(want['vertices']))
    assert np.array_equal(mesh.triangles.cpu().numpy(), want['triangles'])
    assert np.array_equal(mesh.vertex_colors_u8.cpu().numpy(), want['colors'])
    # an empty ground truth gives the reference's NaN record
    none = tsdf.tsdf_mesh_metrics(rec, t['images'], np.zeros((0, 3), np.float32), device=cuda, **kw)
    assert none['n'] == 6 and all(np.isnan(none[k]) for k in m3.KEYS)
