#!/usr/bin/env python3
"""Golden vectors of TSDF integration: the REFERENCE's own ``mv3d/eval/tsdf_atlas.py`` (``TSDFFusion.integrate`` /
``get_tsdf``) run on the CPU from where it lies, and ``get_projection_matrices`` / ``depth_projection_batched`` of
``mv3d/eval/processresults.py`` (executed from the source file by the ast route of make_golden_metrics3d.py, because that
module's import chain does not import here).

``tsdf_atlas.py`` is executed from its source file with ONE in-memory change: current torch refuses its two
``valid[valid] *= ...`` writes because the index mask aliases the written tensor, so exactly those two masks are cloned
(``valid[valid.clone()] *= ...``; the script asserts that two occurrences were replaced).  Nothing of the reference's text
is written to disk.  Stand-ins: the stubs of _ref_import.py, ``skimage.measure`` (a marching-cubes stub that returns no
vertices: ``get_tsdf`` calls it for its ``tsdf_point_cloud`` attribute, which is not recorded) and
``matplotlib.cm.get_cmap`` (imported by the module, never called here).

Run in the build container only:  python tests/golden/make_golden_tsdf.py
Outputs tests/golden/T_tsdf_*.npz (committed) -- data only: seeded inputs (tests/fusion_oracle.scene), the projections the
reference formed, its ``tsdf_vol`` / ``weight_vol`` / ``color_vol`` sums and its ``get_tsdf()`` volumes on the touched
voxels (weight > 0; every other voxel is asserted to hold -1 / 0 / 0), its volume bounds, and the reference's own fp32 error
against the float64 checker (tests/tsdf_oracle.py), which is the yardstick of the GPU tests.
"""
import ast
import math
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
import fusion_oracle  # noqa: E402
import tsdf_oracle  # noqa: E402

LIMIT = 587073          # bytes of tests/golden/C_decoder_net.npz, the largest golden there is


def load_reference():
    _ref_import.install_stubs()
    measure = types.ModuleType('skimage.measure')
    measure.marching_cubes_lewiner = lambda vol, level=0: (np.zeros((0, 3)), np.zeros((0, 3), dtype=int), None, None)
    sk = types.ModuleType('skimage')
    sk.measure = measure
    sys.modules['skimage'], sys.modules['skimage.measure'] = sk, measure
    try:
        import matplotlib.cm as cm
    except ImportError:
        cm = types.ModuleType('matplotlib.cm')
        mpl = types.ModuleType('matplotlib')
        mpl.cm = cm
        sys.modules['matplotlib'], sys.modules['matplotlib.cm'] = mpl, cm
    if not hasattr(cm, 'get_cmap'):
        cm.get_cmap = lambda *a, **k: None
    path = os.path.join(_ref_import.REFERENCE_ROOT, 'mv3d', 'eval', 'tsdf_atlas.py')
    src = open(path).read()
    assert src.count('valid[valid] *=') == 2
    src = src.replace('valid[valid] *=', 'valid[valid.clone()] *=')
    atlas = types.ModuleType('tsdf_atlas_reference')
    atlas.__file__ = path
    exec(compile(src, path, 'exec'), atlas.__dict__)

    path = os.path.join(_ref_import.REFERENCE_ROOT, 'mv3d', 'eval', 'processresults.py')
    tree = ast.parse(open(path).read())
    want = ('get_projection_matrices', 'depth_projection_batched')
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(fns) == 2
    ns = dict(torch=torch, np=np)
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, 'exec'), ns)
    return atlas, ns['get_projection_matrices'], ns['depth_projection_batched']


ATLAS, REF_PROJ, REF_BACKPROJECT = load_reference()


def colors_of(images_u8):
    """[N, h, w, 3] RGB bytes -> what the TSDF branch feeds: BGR, [N, 3, h, w] float (the images already have the depth
    maps' size, so its bilinear resize is the identity and is left out)."""
    return images_u8[..., [2, 1, 0]].permute(0, 3, 1, 2).float().contiguous()


def ref_bounds(depths, K, poses, vol_prcnt, vol_margin, vox_res, img_batch):
    """The bounds loop of the run_tsdf branch, driven through the reference's own two functions."""
    origin = vol_max = None
    n = depths.shape[0]
    for i in range((n - 1) // img_batch + 1):
        sl = slice(i * img_batch, (i + 1) * img_batch)
        P = REF_PROJ(K[sl], poses[sl])
        pts = REF_BACKPROJECT(depths[sl].float(), P).reshape(-1, 3)
        pts = pts[~torch.any(torch.isnan(pts), dim=1)].numpy()
        if pts.shape[0] == 0:
            continue
        lo = torch.as_tensor(np.quantile(pts, 1 - vol_prcnt, axis=0) - vol_margin).float()
        hi = torch.as_tensor(np.quantile(pts, vol_prcnt, axis=0) + vol_margin).float()
        origin = lo if origin is None else torch.min(torch.stack((origin, lo), dim=0), dim=0)[0]
        vol_max = hi if vol_max is None else torch.max(torch.stack((vol_max, hi), dim=0), dim=0)[0]
    return origin, vol_max, ((vol_max - origin) / vox_res).int().tolist()


def sparse(prefix, fus, tsdf, color):
    """State of a reference TSDFFusion (and its get_tsdf volumes) on the touched voxels."""
    w = fus.weight_vol
    idx = torch.nonzero(w > 0).reshape(-1)
    rest = w == 0
    assert bool((fus.tsdf_vol[rest] == -1).all()) and bool((tsdf.tsdf_vol.reshape(-1)[rest] == -1).all())
    assert float(w.max()) < 65536 and bool((w == w.round()).all())
    out = {prefix + 'idx': idx.numpy().astype(np.int32), prefix + 'weight': w[idx].numpy().astype(np.uint16),
           prefix + 'tsdf_sum': fus.tsdf_vol[idx].numpy(), prefix + 'tsdf_avg': tsdf.tsdf_vol.reshape(-1)[idx].numpy()}
    if color:
        assert bool((fus.color_vol[:, rest] == 0).all())
        out[prefix + 'color_sum'] = fus.color_vol[:, idx].numpy()
        out[prefix + 'color_avg'] = tsdf.attribute_vols['color'].reshape(3, -1)[:, idx].numpy()
    return out


def case(name, depths, images_u8, poses, K, voxel_dim, voxel_size, origin, trunc_ratio, color, mid=None, bounds=None):
    P = REF_PROJ(K, poses)
    cols = colors_of(images_u8) if color else None
    n = depths.shape[0]
    fus = ATLAS.TSDFFusion(voxel_dim, voxel_size, origin, trunc_ratio, torch.device('cpu'), color=color, label=False)
    arrays = {}
    with torch.no_grad():
        for i in range(n):
            fus.integrate(P[i], depths[i], None if cols is None else cols[i])
            if mid is not None and i + 1 == mid:
                arrays.update(sparse('mid_', fus, fus.get_tsdf(), color))
        tsdf = fus.get_tsdf()
    arrays.update(sparse('', fus, tsdf, color))
    assert torch.equal(tsdf.attribute_vols['weight'].reshape(-1), fus.weight_vol)

    # the reference's own fp32 error against the float64 checker on the same inputs
    res = tsdf_oracle.integrate(voxel_dim, voxel_size, origin, voxel_size * trunc_ratio, P, depths, cols)
    share = tsdf_oracle.uncertain_share(res, fus.weight_vol)
    mism = tsdf_oracle.weight_mismatches(res, fus.weight_vol)
    err = tsdf_oracle.errors(res, fus.tsdf_vol, fus.color_vol, tsdf.tsdf_vol, tsdf.attribute_vols.get('color'))
    touched = int((fus.weight_vol > 0).sum())
    print('%s: %s voxels, %d touched, uncertain %.4f %% of them (%d pairs), %d weight mismatches outside, reference fp32 '
          'error %s' % (name, 'x'.join(str(int(v)) for v in voxel_dim), touched, 100 * share, res['n_pairs_uncertain'], mism,
                        {k: '%.3g' % v for k, v in err.items()}))
    assert touched > 0 and mism == 0 and share <= tsdf_oracle.UNCERTAIN_CAP
    arrays.update({'ref_err_' + k: np.float64(v) for k, v in err.items()})
    if bounds is not None:
        o, m, dim = ref_bounds(depths, K, poses, **bounds)
        arrays.update(bounds_origin=o.numpy(), bounds_max=m.numpy(), bounds_dim=np.asarray(dim, dtype=np.int64),
                      **{'bounds_' + k: np.float64(v) for k, v in bounds.items()})
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, depths=depths.numpy(), images=images_u8.numpy(), poses=poses.numpy(), K=K.numpy(),
                        projections=P.numpy(), voxel_dim=np.asarray([int(v) for v in voxel_dim], dtype=np.int64),
                        voxel_size=np.float64(voxel_size), origin=np.asarray(origin, dtype=np.float32),
                        trunc_ratio=np.float64(trunc_ratio), color=np.bool_(color),
                        mid=np.int64(0 if mid is None else mid), **arrays)
    assert os.path.getsize(path) <= LIMIT, (path, os.path.getsize(path))
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def turn_about_y(poses, i, ang):
    c, s = math.cos(ang), math.sin(ang)
    turn = torch.tensor([[c, 0., s], [0., 1., 0.], [-s, 0., c]])
    R = turn @ poses[i, :3, :3]
    centre = -poses[i, :3, :3].T @ poses[i, :3, 3]
    poses[i, :3, :3] = R
    poses[i, :3, 3] = -R @ centre


def main():
    # (a) 6 views of 48 x 64 with colour; the volume from the reference's bounds rule with a small margin, two batches
    d, img, poses, K = fusion_oracle.scene(6, (48, 64), seed=21, yaw_step_deg=6, sigma=0.04)
    bounds = dict(vol_prcnt=.995, vol_margin=0.25, vox_res=VOX_A, img_batch=4)
    origin, _, dim = ref_bounds(d, K, poses, **bounds)
    case('T_tsdf_a', d, img, poses, K, dim, VOX_A, origin.tolist(), 3, True, bounds=bounds)
    # (c) the same views and volume, with the state after the first three views recorded too
    case('T_tsdf_c', d, img, poses, K, dim, VOX_A, origin.tolist(), 3, True, mid=3)
    # (b) no colour, 37 x 29 x 23 voxels of 35 cm: far larger than the room, voxels behind cameras and outside every frustum
    d, img, poses, K = fusion_oracle.scene(8, (30, 40), seed=22, yaw_step_deg=40, sigma=0.03)
    case('T_tsdf_b', d, img, poses, K, (37, 29, 23), 0.35, (-3.4, -2.6, -2.55), 3, False)
    # (d) edge cases: 17 x 41 images, 5 x 3 x 2 voxels next to the wall the views look at, trunc_ratio = 1, view 1 all zero, view 3
    # facing away, +inf and NaN depth pixels in views 0 and 2
    d, img, poses, K = fusion_oracle.scene(5, (17, 41), seed=23, yaw_step_deg=4, sigma=0.02)
    d[1] = 0
    turn_about_y(poses, 3, math.pi)
    d[0, 3:6, 10:20] = float('inf')
    d[0, 9:12, 22:30] = float('nan')
    d[2, 5:9, 5:15] = float('nan')
    d[2, 10:14, 25:35] = float('inf')
    case('T_tsdf_d', d, img, poses, K, (5, 3, 2), 0.3, (4.8, 2.0, 1.2), 1, True)


VOX_A = 0.08

if __name__ == '__main__':
    main()
