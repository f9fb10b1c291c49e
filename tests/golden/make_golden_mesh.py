#!/usr/bin/env python3
"""Golden vectors of mesh extraction: the REFERENCE's own ``TSDF.get_mesh`` (``mv3d/eval/tsdf_atlas.py:161-253``) and the
``tsdf_point_cloud`` attribute of its ``TSDFFusion.get_tsdf`` (:465-481), executed from the source file in memory by the
route of make_golden_tsdf.py (the same single in-memory change to the two aliased mask writes of ``integrate``).  Nothing of
the reference's text is written to disk.

Stand-ins for what is absent here:
  * ``skimage.measure.marching_cubes`` / ``marching_cubes_lewiner`` := the checker's ``marching_cubes`` (tests/mesh_oracle.py,
    the project's case table), returning float32 vertices as skimage does.  The triangulation is therefore the project's;
    everything the reference does AROUND the call -- clamp, empty-mesh rule, the -1 / +1 bad-vertex rule, the colour lookup at
    round(verts), the world transform, the removal of bad vertices -- is the reference's own NumPy.
  * ``open3d`` := a minimal ``geometry.TriangleMesh`` / ``utility.Vector3dVector`` / ``Vector3iVector``;
    ``remove_vertices_by_index`` follows Open3D's documented semantics: the listed vertices are removed, every triangle that
    references one is removed, the remaining vertices are renumbered in order.
  * ``np.int`` := ``int`` (the reference was written for an older NumPy).

Run in the build container only:  python tests/golden/make_golden_mesh.py
Outputs tests/golden/G_mesh_{a,b,c}.npz (committed) -- data only: the input volumes and the reference's output vertices,
triangles, colours and removed-vertex list.
  a  the volume the reference's own TSDFFusion builds from the inputs of T_tsdf_a (20 x 52 x 34 voxels, colour): many -1 / +1
     crossings at the truncation band, so the bad-vertex rule removes a large share; also its tsdf_point_cloud attribute
  b  a hand-built 7 x 6 x 5 volume: edges with t exactly 0.5 at an even and an odd voxel (half-to-even both ways), corners
     holding exactly 0 on either end of an edge (t = 1 moves floor to the next voxel), values beyond +-1 (the clamp makes
     them +-1: bad vertices), colours below 0 and above 255
  c  two volumes for the empty-mesh rule: all >= 0, and zeros with negatives (where the sign rule alone would emit vertices)
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import  # noqa: E402
import mesh_oracle  # noqa: E402

LIMIT = 587073          # bytes of tests/golden/C_decoder_net.npz, the largest golden there is


class _Mesh:
    """Minimal stand-in for open3d.geometry.TriangleMesh."""
    last_removed = None

    def __init__(self):
        self.vertices = np.zeros((0, 3), dtype=np.float64)
        self.triangles = np.zeros((0, 3), dtype=np.int32)
        self.vertex_colors = np.zeros((0, 3), dtype=np.float64)

    def remove_vertices_by_index(self, idx):
        idx = np.asarray(idx, dtype=np.int64)
        _Mesh.last_removed = idx.copy()
        n = self.vertices.shape[0]
        keep = np.ones(n, dtype=bool)
        keep[idx] = False
        new = np.cumsum(keep) - 1
        tri = np.asarray(self.triangles, dtype=np.int64)
        tri = tri[keep[tri].all(axis=1)] if tri.shape[0] else tri
        self.triangles = new[tri].astype(np.int32).reshape(-1, 3)
        self.vertices = self.vertices[keep]
        if self.vertex_colors.shape[0] == n:
            self.vertex_colors = self.vertex_colors[keep]


def load_reference():
    _ref_import.install_stubs()

    def mc(vol, level=0):
        assert level == 0
        verts, faces = mesh_oracle.marching_cubes(np.asarray(vol, dtype=np.float32))
        return verts.astype(np.float32), faces, None, None

    measure = types.ModuleType('skimage.measure')
    measure.marching_cubes = mc
    measure.marching_cubes_lewiner = mc
    sk = types.ModuleType('skimage')
    sk.measure = measure
    sys.modules['skimage'], sys.modules['skimage.measure'] = sk, measure
    o3d = types.ModuleType('open3d')
    o3d.geometry = types.SimpleNamespace(TriangleMesh=_Mesh)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.array(a, dtype=np.float64).reshape(-1, 3),
                                        Vector3iVector=lambda a: np.array(a, dtype=np.int32).reshape(-1, 3))
    sys.modules['open3d'] = o3d
    try:
        import matplotlib.cm as cm
    except ImportError:
        cm = types.ModuleType('matplotlib.cm')
        mpl = types.ModuleType('matplotlib')
        mpl.cm = cm
        sys.modules['matplotlib'], sys.modules['matplotlib.cm'] = mpl, cm
    if not hasattr(cm, 'get_cmap'):
        cm.get_cmap = lambda *a, **k: None
    if not hasattr(np, 'int'):
        np.int = int
    path = os.path.join(_ref_import.REFERENCE_ROOT, 'mv3d', 'eval', 'tsdf_atlas.py')
    src = open(path).read()
    assert src.count('valid[valid] *=') == 2
    src = src.replace('valid[valid] *=', 'valid[valid.clone()] *=')
    atlas = types.ModuleType('tsdf_atlas_reference')
    atlas.__file__ = path
    exec(compile(src, path, 'exec'), atlas.__dict__)
    return atlas


ATLAS = load_reference()


def ref_mesh(vol, color, voxel_size, origin):
    """The reference's get_mesh on a volume -> dict of recorded arrays (prefix-free)."""
    attribute_vols = {} if color is None else {'color': torch.from_numpy(color)}
    t = ATLAS.TSDF(voxel_size, torch.tensor(origin, dtype=torch.float).view(1, 3), torch.from_numpy(vol), attribute_vols)
    _Mesh.last_removed = None
    m = t.get_mesh()
    verts = np.asarray(m.vertices)
    v32 = verts.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), verts)                 # the reference's world positions are float32 values
    cols = np.asarray(m.vertex_colors)
    c8 = np.rint(cols * 255.).astype(np.uint8)
    assert np.array_equal(c8 / 255., cols)
    removed = np.zeros(0, dtype=np.int64) if _Mesh.last_removed is None else _Mesh.last_removed
    return dict(vertices=v32, triangles=np.asarray(m.triangles, dtype=np.int32).reshape(-1, 3), colors=c8.reshape(-1, 3),
                removed=removed.astype(np.int32))


def save(name, **arrays):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= LIMIT, (path, os.path.getsize(path))
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def case_a():
    with np.load(os.path.join(HERE, 'T_tsdf_a.npz')) as f:
        g = {k: f[k] for k in f.files}
    dim, vs, origin = [int(v) for v in g['voxel_dim']], float(g['voxel_size']), g['origin'].tolist()
    cols = torch.from_numpy(g['images'])[..., [2, 1, 0]].permute(0, 3, 1, 2).float().contiguous()
    fus = ATLAS.TSDFFusion(dim, vs, origin, float(g['trunc_ratio']), torch.device('cpu'), color=True, label=False)
    with torch.no_grad():
        for i in range(g['depths'].shape[0]):
            fus.integrate(torch.from_numpy(g['projections'][i]), torch.from_numpy(g['depths'][i]), cols[i])
        tsdf = fus.get_tsdf()
    vol = tsdf.tsdf_vol.numpy().copy()
    color = tsdf.attribute_vols['color'].numpy().copy()
    pc = tsdf.attribute_vols['tsdf_point_cloud']
    print('a: the reference\'s tsdf_point_cloud is %s %s' % (pc.dtype, tuple(pc.shape)))
    pc = pc.numpy()
    pc_xyz, pc_rgb = pc[:, :3].astype(np.float32), pc[:, 3:].astype(np.uint8)
    assert np.array_equal(pc_xyz.astype(pc.dtype), pc[:, :3]) and np.array_equal(pc_rgb.astype(pc.dtype), pc[:, 3:])
    out = ref_mesh(vol, color, vs, origin)
    n_all = out['vertices'].shape[0] + out['removed'].shape[0]
    print('a: %d marching-cubes vertices, %d removed, %d triangles left' % (n_all, out['removed'].shape[0], out['triangles'].shape[0]))
    assert out['vertices'].shape[0] > 0 and out['removed'].shape[0] > 0 and pc.shape[0] == n_all
    save('G_mesh_a', tsdf=vol, color=color, voxel_size=np.float64(vs), origin=np.asarray(origin, dtype=np.float32),
         pc_xyz=pc_xyz, pc_rgb=pc_rgb, pc_dtype=np.asarray(str(pc.dtype)), **out)


def case_b():
    rng = np.random.default_rng(77)
    g = np.mgrid[0:7, 0:6, 0:5].astype(np.float64)
    vol = (0.21 * g[0] + 0.13 * g[1] - 0.33 * g[2] - 0.37 + 0.15 * rng.standard_normal((7, 6, 5))).astype(np.float32)
    vol[2, 2, 2], vol[3, 2, 2] = -0.25, 0.25          # t = 0.5 at x = 2.5: rounds to 2
    vol[3, 3, 1], vol[4, 3, 1] = 0.375, -0.375        # t = 0.5 at x = 3.5: rounds to 4
    vol[1, 1, 1], vol[1, 2, 1] = -0.125, 0.125        # t = 0.5 at y = 1.5: rounds to 2
    vol[5, 2, 2], vol[5, 2, 3] = 0.5, -0.5            # t = 0.5 at z = 2.5: rounds to 2
    vol[1, 4, 3], vol[1, 5, 3] = -0.5, 0.0            # vb = 0: t = 1, the vertex sits on the next voxel
    vol[4, 1, 3], vol[5, 1, 3] = 0.0, -0.75           # va = 0: t = 0
    vol[0, 0, 4], vol[1, 0, 4] = -2.5, 1.75           # beyond the clamp: -1 next to +1, a bad vertex
    vol[6, 5, 0], vol[6, 4, 0] = 3.0, -1.0
    vol[3, 0, 0] = -7.0
    color = rng.uniform(-60, 320, (3, 7, 6, 5)).astype(np.float32)
    color[:, 2, 2, 2] = [12.9, -0.5, 255.9]
    color[:, 4, 3, 1] = [300.0, 254.999, 0.0]
    vs, origin = 0.04, [-1.25, 0.3, 2.0]
    out = ref_mesh(vol, color, vs, origin)
    print('b: %d vertices kept, %d removed, %d triangles left' % (out['vertices'].shape[0], out['removed'].shape[0],
                                                                  out['triangles'].shape[0]))
    assert out['vertices'].shape[0] > 0 and out['removed'].shape[0] > 0 and out['triangles'].shape[0] > 0
    assert (color < 0).any() and (color > 255).any()
    save('G_mesh_b', tsdf=vol, color=color, voxel_size=np.float64(vs), origin=np.asarray(origin, dtype=np.float32), **out)


def case_c():
    rng = np.random.default_rng(78)
    pos = np.abs(rng.standard_normal((5, 4, 6))).astype(np.float32)
    pos[1, 2, 3] = 0.0
    neg = -np.abs(rng.standard_normal((4, 5, 3))).astype(np.float32)
    neg[rng.random((4, 5, 3)) < 0.4] = 0.0
    assert (neg == 0).any() and (neg < 0).any() and mesh_oracle.n_crossing_edges(neg) > 0
    arrays = {}
    for tag, vol in (('pos', pos), ('neg', neg)):
        color = rng.uniform(0, 255, (3,) + vol.shape).astype(np.float32)
        out = ref_mesh(vol, color, 0.05, [0., 0., 0.])
        assert out['vertices'].shape[0] == 0 and out['triangles'].shape[0] == 0
        arrays.update({tag + '_tsdf': vol, tag + '_color': color})
        arrays.update({tag + '_' + k: v for k, v in out.items()})
    save('G_mesh_c', voxel_size=np.float64(0.05), origin=np.zeros(3, dtype=np.float32), **arrays)


if __name__ == '__main__':
    case_a()
    case_b()
    case_c()
