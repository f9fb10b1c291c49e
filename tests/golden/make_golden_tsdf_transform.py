#!/usr/bin/env python3
"""Golden vectors of TSDF resampling: the REFERENCE's own ``TSDF.transform`` (``mv3d/eval/tsdf_atlas.py:255-338``) run on the CPU
from where it lies, through the loader of make_golden_tsdf.py (``ATLAS``), with fp32, int64 and bool attribute volumes; and the
reference's ``l1`` / ``l1_ns`` (``mv3d/baselines/atlas/evaluation.py:61-96``) taken by the ast route with a no-op stand-in for
its ``check_tsdf`` (which, as written, raises on an attribute typo).  Nothing of the reference's text is written to disk.

Run in the build container only:  python tests/golden/make_golden_tsdf_transform.py
Outputs tests/golden/R_resample_*.npz (committed) -- data only: the seeded inputs, the reference's outputs, its outside mask
(read off a second run whose ``mask_outside`` volume is all False: the output is True exactly where the reference's mask is),
the reference's own fp32 error against the float64 checker (tests/tsdf_transform_oracle.py) outside the uncertain set -- the
yardstick of the GPU tests -- and the uncertain share, asserted <= 0.5 % here.

  a  exact integer shift, align_corners=True, 12 x 9 x 7 -> 10 x 11 x 8 (cropped on one side, padded on the other), voxel size
     0.0625 and origins that are multiples of it: every step up to g is exact, so the checker runs with margin 0 and the
     verdicts are equal on every voxel.  Also the reference's l1 / l1_ns of the aligned volume against a seeded target, and the
     float64 value of the same masked means.
  b  Rz(17 deg) Ry(-8 deg) about the volume's centre plus a sub-voxel translation, 13 x 10 x 9 -> 15 x 12 x 11, align_corners=False
  c  the same with align_corners=True
"""
import ast
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import tsdf_transform_oracle as oracle  # noqa: E402
from make_golden_tsdf import ATLAS, LIMIT  # noqa: E402


def load_metrics():
    path = os.path.join(_ref_import.REFERENCE_ROOT, 'mv3d', 'baselines', 'atlas', 'evaluation.py')
    tree = ast.parse(open(path).read())
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ('l1', 'l1_ns')]
    assert len(fns) == 2
    ns = dict(torch=torch, np=np, F=torch.nn.functional, check_tsdf=lambda pred, trgt: None)
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, 'exec'), ns)
    return ns['l1'], ns['l1_ns']


REF_L1, REF_L1_NS = load_metrics()
FP32_KEYS, OTHER_KEYS = ('weight', 'color'), ('instance', 'semseg', 'mask_outside')


def volumes(dim, seed):
    """A seeded volume that exercises every branch: a tilted wavy surface through the middle with a truncation band of about
    three voxels (so both |v| < 1 and the saturated -1 / +1 regions occur), and attribute volumes of every kind."""
    rng = np.random.RandomState(seed)
    nx, ny, nz = dim
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing='ij')
    d = (z - nz / 2.0) + 0.35 * (x - nx / 2.0) - 0.2 * (y - ny / 2.0) + 0.8 * np.sin(0.9 * x + 0.5 * y)
    tsdf = np.clip(d / 3.0 + 0.02 * rng.randn(nx, ny, nz), -1, 1).astype(np.float32)
    weight = (rng.randint(0, 6, size=dim) * (rng.rand(*dim) > 0.25)).astype(np.float32)
    color = (rng.rand(3, *dim) * 255).astype(np.float32)
    instance = rng.randint(-1, 7, size=dim).astype(np.int64)
    semseg = rng.randint(-1, 12, size=dim).astype(np.int64)
    mask_outside = rng.rand(*dim) > 0.6
    return dict(tsdf=tsdf, weight=weight, color=color, instance=instance, semseg=semseg, mask_outside=mask_outside)


def rotation(dim, voxel_size, origin, shift):
    """Rz(17 deg) Ry(-8 deg) about the centre of the volume, then a translation: [3, 4] fp32."""
    a, b = math.radians(17), math.radians(-8)
    Rz = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    R = Rz @ Ry
    c = np.asarray(origin, dtype=np.float64) + 0.5 * voxel_size * (np.asarray(dim) - 1)
    t = c - R @ c + np.asarray(shift, dtype=np.float64)
    return np.concatenate((R, t[:, None]), axis=1).astype(np.float32)


def run_reference(v, voxel_size, src_origin, matrix, voxel_dim, dst_origin, align):
    def ref(mask):
        vols = {k: torch.from_numpy(v[k].copy()) for k in FP32_KEYS + OTHER_KEYS if k != 'mask_outside'}
        vols['mask_outside'] = torch.from_numpy(mask.copy())
        t = ATLAS.TSDF(voxel_size, torch.tensor(src_origin, dtype=torch.float).view(1, 3), torch.from_numpy(v['tsdf'].copy()), vols)
        M = torch.cat((torch.from_numpy(matrix), torch.tensor([[0., 0., 0., 1.]])), dim=0)
        with torch.no_grad():
            return t.transform(M, [int(d) for d in voxel_dim], [float(o) for o in dst_origin], align_corners=align)
    out = ref(v['mask_outside'])
    probe = ref(np.zeros_like(v['mask_outside']))
    return out, probe.attribute_vols['mask_outside'].numpy().copy()


def case(name, src_dim, voxel_dim, voxel_size, src_origin, dst_origin, matrix, align, seed, margin, metrics=False):
    v = volumes(src_dim, seed)
    out, ref_outside = run_reference(v, voxel_size, src_origin, matrix, voxel_dim, dst_origin, align)
    assert tuple(out.tsdf_vol.shape) == tuple(voxel_dim) and out.attribute_vols['instance'].dtype == torch.int64
    assert out.attribute_vols['mask_outside'].dtype == torch.bool
    pl = oracle.plan(src_dim, voxel_size, src_origin, matrix, align, voxel_dim, dst_origin, np.float64, margin)
    keep = ~pl['uncertain']
    share = oracle.uncertain_share(pl)
    assert share <= oracle.UNCERTAIN_CAP, share
    assert np.array_equal(ref_outside.reshape(-1)[keep], pl['outside'][keep])
    want_tsdf = oracle.tsdf(pl, v['tsdf'])
    interp = (~pl['outside']) & (np.abs(oracle.nearest(pl, v['tsdf'])[0]) < 1)
    arrays = {'in_' + k: a for k, a in v.items()}
    arrays.update(out_tsdf=out.tsdf_vol.numpy(), ref_outside=ref_outside, uncertain_share=np.float64(share),
                  ref_err_tsdf=np.float64(oracle.max_error(pl, out.tsdf_vol.numpy(), want_tsdf)))
    for k in FP32_KEYS:
        got = out.attribute_vols[k].numpy()
        arrays['out_' + k] = got
        arrays['ref_err_' + k] = np.float64(oracle.max_error(pl, got, oracle.trilinear(pl, v[k])))
    for k in OTHER_KEYS:
        got = out.attribute_vols[k].numpy()
        want = oracle.nearest(pl, v[k])
        if k in ('semseg', 'mask_outside'):
            want = oracle.fill_outside(pl, want, -1 if k == 'semseg' else True)
        assert np.array_equal(got.reshape(-1)[keep], want[0][keep]), k
        arrays['out_' + k] = got
    print('%s: %s -> %s align_corners=%s: outside %.1f %%, interpolated %.1f %%, uncertain %.3f %%; reference fp32 error tsdf %.3g '
          'weight %.3g color %.3g' % (name, 'x'.join(map(str, src_dim)), 'x'.join(map(str, voxel_dim)), align,
                                      100 * pl['outside'].mean(), 100 * interp.mean(), 100 * share, arrays['ref_err_tsdf'],
                                      arrays['ref_err_weight'], arrays['ref_err_color']))
    if metrics:
        # the reference's l1 / l1_ns of its aligned volume against a seeded target on the output grid, whose weight lies under
        # `attributes` as TSDF.load places it
        rng = np.random.RandomState(seed + 1000)
        trgt_tsdf = np.clip(out.tsdf_vol.numpy() + 0.1 * rng.randn(*voxel_dim), -1, 1).astype(np.float32)
        trgt_weight = (rng.randint(0, 4, size=voxel_dim) * (rng.rand(*voxel_dim) > 0.3)).astype(np.float32)
        trgt = ATLAS.TSDF(voxel_size, out.origin, torch.from_numpy(trgt_tsdf), {}, {'weight': torch.from_numpy(trgt_weight)})
        ref_l1, ref_l1_ns = REF_L1(out, trgt), REF_L1_NS(out, trgt)
        diff = np.abs(want_tsdf.reshape(voxel_dim) - trgt_tsdf.astype(np.float64))
        m1 = trgt_weight != 0
        m2 = m1 & (trgt_tsdf < 1)
        f64_l1, f64_l1_ns = float(diff[m1].mean()), float(diff[m2].mean())
        print('%s: l1 %.9g (float64 %.9g), l1_ns %.9g (float64 %.9g) over %d / %d voxels'
              % (name, ref_l1, f64_l1, ref_l1_ns, f64_l1_ns, m1.sum(), m2.sum()))
        arrays.update(trgt_tsdf=trgt_tsdf, trgt_weight=trgt_weight, ref_l1=np.float64(ref_l1), ref_l1_ns=np.float64(ref_l1_ns),
                      f64_l1=np.float64(f64_l1), f64_l1_ns=np.float64(f64_l1_ns))
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, voxel_size=np.float64(voxel_size), src_origin=np.asarray(src_origin, dtype=np.float32),
                        dst_origin=np.asarray(dst_origin, dtype=np.float32), matrix=matrix,
                        voxel_dim=np.asarray(voxel_dim, dtype=np.int64), align_corners=np.bool_(align),
                        margin=np.float64(margin), **arrays)
    assert os.path.getsize(path) <= LIMIT, (path, os.path.getsize(path))
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def main():
    eye = np.eye(4, dtype=np.float32)[:3]
    # (a) shift by (+3, -1, 0) voxels: x is cropped below and runs past the source above, y starts one voxel before the source
    case('R_resample_a', (12, 9, 7), (10, 11, 8), 0.0625, (1.0, -0.5, 0.25), (1.1875, -0.5625, 0.25), eye, True, 41, 0.0, metrics=True)
    src_origin, dst_origin = (0.3, -1.1, 0.7), (0.26, -1.13, 0.68)
    M = rotation((13, 10, 9), 0.04, src_origin, (0.013, -0.009, 0.017))
    case('R_resample_b', (13, 10, 9), (15, 12, 11), 0.04, src_origin, dst_origin, M, False, 42, oracle.MARGIN)
    case('R_resample_c', (13, 10, 9), (15, 12, 11), 0.04, src_origin, dst_origin, M, True, 42, oracle.MARGIN)


if __name__ == '__main__':
    main()
