"""GPU: exact order statistics by radix selection (3dvnet_amd/tsdf.py: cloud_order_stats / backproject_order_stats ->
csrc/order_stats.hip) and the volume bounds built on them (volume_bounds_device, the drivers' ``bounds='device'``) against the
NumPy checker (tests/order_stats_oracle.py).  Every comparison of ``count`` and ``stats`` is bit-exact (zeros compare as
values: the sort of the checker may order -0.0 and +0.0 either way); there is no tolerance.  The bounds are compared with the
reference's recorded ones at the 1e-5 the host path is held to on the same fixture, and with the checker's exactly.

Measured on one MI355X: every count and statistic identical to the checker's in all 28 cases x 3 quantile sets; device bounds on
the fixture 9.5e-7 from the reference's (bound 1e-5), dims equal, identical to the checker's.  Wall time of the module's 30 tests:
2.9 s.
"""
import numpy as np
import pytest
import torch

import fusion_oracle as fo
import order_stats_oracle as oo
from conftest import v3d
from test_order_stats_oracle import fixture_a

pytestmark = pytest.mark.gpu

TILE = 2048                                   # points per workgroup tile (include/v3d.h)
QS_SETS = ((0.0, 1 - .995, .5, .995), (1 - .995, .995, 1.0), (1 - .995, .995))
_rng = np.random.default_rng(20240611)


def _rand(n, scale=3.0):
    return (_rng.standard_normal((n, 3)) * scale).astype(np.float32)


def _bits(base, field):
    return (np.uint32(base) + field.astype(np.uint32)).view(np.float32)


def _clouds():
    c = {}
    for n in (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1):
        c['n%d' % n] = _rand(n)
    c['all_equal'] = np.tile(np.array([[1.5, -2.25, 0.0]], np.float32), (300, 1))
    # 100 + 100 rows: q = .5 has lo = 99 (the last of the lower value) and hi = 100 (the first of the upper one)
    two = np.concatenate((np.tile(np.array([[-1.0, 2.0, 1e-3]], np.float32), (100, 1)),
                          np.tile(np.array([[3.0, 2.5, 2e-3]], np.float32), (100, 1))))
    c['two_values_on_the_boundary'] = two[_rng.permutation(200)]
    n = 1500
    c['last_digit_only'] = np.stack((_bits(0x40490000, _rng.integers(0, 1024, n)), _bits(0xC0490000, _rng.integers(0, 1024, n)),
                                     _bits(0x00000000, _rng.integers(0, 1024, n))), axis=1)
    c['middle_digit_only'] = np.stack((_bits(0x40400155, _rng.integers(0, 2048, n) << 10), _bits(0xC0400155, _rng.integers(0, 2048, n) << 10),
                                       _bits(0x3F800000, _rng.integers(0, 2048, n) << 10)), axis=1)
    signs = _rng.choice(np.array([-1.0, -0.0, 0.0, 1.0, -1e-3, 1e-3, -1e-40, 1e-40], np.float32), (700, 3))
    signs[::7] = _rand(100, 0.5)
    c['mixed_signs_and_zeros'] = signs
    inf = _rand(900)
    inf[_rng.integers(0, 900, 40), _rng.integers(0, 3, 40)] = np.inf
    inf[_rng.integers(0, 900, 40), _rng.integers(0, 3, 40)] = -np.inf
    c['infinities'] = inf
    nan = _rand(TILE + 300)
    nan[_rng.integers(0, nan.shape[0], 200), _rng.integers(0, 3, 200)] = np.nan
    c['nan_rows'] = nan
    c['all_nan'] = np.where(np.arange(3)[None] == _rng.integers(0, 3, (70, 1)), np.float32(np.nan), _rand(70))
    return c


CLOUDS = _clouds()


def _scene():
    d, _, poses, K = fo.scene(3, (37, 53), seed=77, yaw_step_deg=None, sigma=0.04)
    return d.numpy().copy(), K.numpy(), poses.numpy()


def _fused_cases():
    g, _ = fixture_a()
    c = {'golden_batch0': (g['depths'][:4], g['K'][:4], g['poses'][:4]), 'golden_batch1': (g['depths'][4:], g['K'][4:], g['poses'][4:])}
    d, K, poses = _scene()
    c['scene_37x53'] = (d, K, poses)
    z = d.copy()
    z[1] = 0
    c['one_zero_view'] = (z, K, poses)
    c['all_zero'] = (np.zeros_like(d), K, poses)
    inf = d.copy()
    inf[0, 5, 7] = np.inf
    inf[2, 30, 50] = np.inf
    c['inf_depth'] = (inf, K, poses)
    neg = d.copy()
    neg[1, 10:14, 20:30] = -neg[1, 10:14, 20:30]
    c['negative_depth'] = (neg, K, poses)
    c['one_pixel'] = (np.array([[[2.5]]], np.float32), K[:1], poses[:1])
    return c


FUSED = _fused_cases()


def check(tag, got, want, qs):
    (count, stats), (want_n, want_stats) = got, want
    torch.cuda.synchronize()
    n, st = int(count.cpu().item()), stats.cpu().numpy()
    ok = oo.same_bits(st, want_stats)
    print('%s qs=%s: count %d (checker %d), statistics %s' % (tag, qs, n, want_n, 'identical' if ok else 'DIFFER'))
    assert count.dtype == torch.int32 and stats.dtype == torch.float32 and st.shape == (len(qs), 3, 2)
    assert n == want_n
    assert ok, (st, want_stats)
    if want_n == 0:
        assert np.isnan(st).all()


@pytest.mark.parametrize('case', list(CLOUDS))
def test_cloud_entry_point(cuda, case):
    tsdf = v3d('tsdf')
    pts = CLOUDS[case]
    dev_pts = torch.from_numpy(pts).to(cuda)
    for qs in QS_SETS:
        check(case, tsdf.cloud_order_stats(dev_pts, qs), oo.order_stats(pts, qs), qs)


@pytest.mark.parametrize('case', list(FUSED))
def test_fused_entry_point(cuda, case):
    tsdf = v3d('tsdf')
    d, K, poses = FUSED[case]
    Pi = oo.inverse_projections(K, poses)
    want_pts = oo.backproject(d, Pi)
    dd, pp = torch.from_numpy(np.ascontiguousarray(d)).to(cuda), torch.from_numpy(Pi).to(cuda)
    for qs in QS_SETS:
        check(case, tsdf.backproject_order_stats(dd, pp, qs), oo.order_stats(want_pts, qs), qs)
    if case == 'inf_depth':
        assert np.isinf(want_pts[~np.isnan(want_pts).any(axis=1)]).any()          # the case holds what it is named for


def test_fused_entry_point_uses_the_whole_matrix(cuda):
    """A projective last row and small views that share waves (several views per wave, a matrix per view)."""
    tsdf = v3d('tsdf')
    rng = np.random.default_rng(9)
    Pi = (np.eye(4) + 0.05 * rng.standard_normal((9, 4, 4))).astype(np.float32)
    d = (1 + rng.random((9, 5, 7))).astype(np.float32)
    qs = (1 - .995, .5, .995)
    check('general matrices', tsdf.backproject_order_stats(torch.from_numpy(d).to(cuda), torch.from_numpy(Pi).to(cuda), qs),
          oo.order_stats(oo.backproject(d, Pi), qs), qs)


def test_volume_bounds_device(cuda):
    tsdf = v3d('tsdf')
    g, kw = fixture_a()
    depths = torch.from_numpy(g['depths']).to(cuda)
    origin, vol_max, dim = tsdf.volume_bounds_device(depths, g['K'], g['poses'], **kw)
    print('device bounds: origin %s max %s dim %s; largest difference to the reference %.3g'
          % (origin.tolist(), vol_max.tolist(), dim, max(float(np.abs(origin.numpy() - g['bounds_origin']).max()),
                                                        float(np.abs(vol_max.numpy() - g['bounds_max']).max()))))
    assert origin.dtype == torch.float32 and origin.shape == (3,) and vol_max.shape == (3,) and not origin.is_cuda
    np.testing.assert_allclose(origin.numpy(), g['bounds_origin'], rtol=0, atol=1e-5)
    np.testing.assert_allclose(vol_max.numpy(), g['bounds_max'], rtol=0, atol=1e-5)
    assert dim == g['bounds_dim'].tolist()
    want = oo.volume_bounds(g['depths'], g['K'], g['poses'], **kw)
    assert torch.equal(origin, want[0]) and torch.equal(vol_max, want[1]) and dim == want[2]
    # two batches (4 + 2 views): the element-wise minimum / maximum of the single-batch calls
    one = [tsdf.volume_bounds_device(depths[s], g['K'][s], g['poses'][s], **kw) for s in (slice(0, 4), slice(4, 6))]
    assert torch.equal(origin, torch.minimum(one[0][0], one[1][0])) and torch.equal(vol_max, torch.maximum(one[0][1], one[1][1]))
    # an empty batch is skipped; a scene without a point is an error
    d = depths.clone()
    d[4:] = 0
    o2, m2, _ = tsdf.volume_bounds_device(d, g['K'], g['poses'], **kw)
    assert torch.equal(o2, one[0][0]) and torch.equal(m2, one[0][1])
    with pytest.raises(ValueError):
        tsdf.volume_bounds_device(torch.zeros_like(d), g['K'], g['poses'], **kw)


def test_fuse_preds_tsdf_with_device_bounds(cuda):
    tsdf = v3d('tsdf')
    g, kw = fixture_a()
    rec = dict(depth_preds=g['depths'], rotmats=g['poses'][:, :3, :3], tvecs=g['poses'][:, :3, 3], K=g['K'])
    out, fus = tsdf.fuse_preds_tsdf(rec, g['images'], trunc_ratio=float(g['trunc_ratio']), return_fusion=True, bounds='device',
                                    vol_prcnt=kw['vol_prcnt'], vol_margin=kw['vol_margin'], vox_res=kw['vox_res'],
                                    img_batch=kw['img_batch'])
    assert tuple(out.tsdf_vol.shape) == tuple(g['bounds_dim'].tolist()) and list(fus.voxel_dim) == g['voxel_dim'].tolist()
    np.testing.assert_allclose(fus.origin.cpu().numpy().reshape(3), g['bounds_origin'], rtol=0, atol=1e-5)
    assert int((fus.weight_vol > 0).sum()) > 0
    with pytest.raises(ValueError):
        tsdf.fuse_preds_tsdf(rec, g['images'], bounds='elsewhere')


def test_ten_launches_are_bit_identical(cuda):
    tsdf = v3d('tsdf')
    pts = torch.from_numpy(CLOUDS['n%d' % (3 * TILE + 1)]).to(cuda)
    qs = QS_SETS[0]
    runs = [tsdf.cloud_order_stats(pts, qs) for _ in range(10)]
    torch.cuda.synchronize()
    first = (runs[0][0].cpu(), runs[0][1].cpu().view(torch.int32))
    for c, s in runs[1:]:
        assert torch.equal(c.cpu(), first[0]) and torch.equal(s.cpu().view(torch.int32), first[1])
    d, K, poses = FUSED['scene_37x53']
    dd, pp = torch.from_numpy(d).to(cuda), torch.from_numpy(oo.inverse_projections(K, poses)).to(cuda)
    runs = [tsdf.backproject_order_stats(dd, pp, qs) for _ in range(10)]
    torch.cuda.synchronize()
    for c, s in runs[1:]:
        assert torch.equal(c, runs[0][0]) and torch.equal(s.view(torch.int32), runs[0][1].view(torch.int32))


def test_errors(cuda):
    tsdf, lib_mod = v3d('tsdf'), v3d('_lib')
    lib = lib_mod.load()
    import ctypes
    pts = torch.zeros(8, 3, device=cuda)
    count, stats = torch.zeros(1, dtype=torch.int32, device=cuda), torch.zeros(24, device=cuda)
    ws = torch.zeros(int(lib.v3d_order_stats_workspace_bytes(4)), dtype=torch.uint8, device=cuda)
    q2 = (ctypes.c_double * 2)(0.005, 0.995)
    args = (count.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert lib.v3d_cloud_order_stats_f32(pts.data_ptr(), 0, q2, 2, *args) == -1                    # BAD_SHAPE
    assert lib.v3d_backproject_order_stats_f32(pts.data_ptr(), pts.data_ptr(), 2048, 1024, 1024, q2, 2, *args) == -1
    assert lib.v3d_cloud_order_stats_f32(pts.data_ptr(), 8, q2, 5, *args) == -2                    # BAD_ARG
    assert lib.v3d_cloud_order_stats_f32(pts.data_ptr(), 8, (ctypes.c_double * 2)(0.5, 1.5), 2, *args) == -2
    assert lib.v3d_backproject_order_stats_f32(pts.data_ptr(), pts.data_ptr(), 1, 2, 2, q2, 0, *args) == -2
    torch.cuda.synchronize()
    assert int(count.item()) == 0 and bool((stats == 0).all())                                     # nothing was enqueued
    with pytest.raises(ValueError):
        tsdf.cloud_order_stats(pts, (0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError):
        tsdf.backproject_order_stats(torch.ones(2, 4, 4, device=cuda), torch.eye(4)[None], (0.5,))
    with pytest.raises(lib_mod.V3DLibraryError):
        tsdf.volume_bounds_device(torch.ones(1, 4, 4), np.eye(3)[None], np.eye(4)[None])
