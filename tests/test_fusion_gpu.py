"""GPU: multi-view depth fusion (3dvnet_amd/fusion.py -> v3d_fuse_depths_f32 / v3d_fusion_compact, csrc/fusion.hip) against the
reference's outputs (tests/golden/F_fusion_*.npz), against the float64 checker (tests/fusion_oracle.py) at small and at full
size, and its own invariants.  Every test runs the HIP path through the C ABI.

Bound on fused points: 4 x the reference's own fp32 error against the float64 checker (the project's rule for fp32 routes),
per golden case the figure recorded in tests/test_fusion_oracle.py; where no reference output exists (properties, full
size) the largest of those figures, 1.426e-6 m -- the scenes share the room, the depth range and hence the ulp of a
coordinate.  Masks and counts: see tests/fusion_oracle.py (caps: 2 % mask-ambiguous, 10 % left out of point comparisons).

Wall time on one MI355X: 10 s for the module's 14 tests (the float64 checker on the CPU dominates: 8 reference views against
all 63 sources at 256 x 320 and 480 x 640 take 2.6 s and 3.7 s).
"""
import numpy as np
import pytest
import torch

import fusion_oracle as fo
from conftest import v3d
from test_fusion_oracle import CASES, REF_ERR, load_case

pytestmark = pytest.mark.gpu
YARDSTICK = max(REF_ERR.values())


def run_dense(dev, depths, poses, K, images=None, z_thresh=0.1, n_thresh=3, **kw):
    fusion = v3d('fusion')
    out = fusion.fuse_depth_maps(torch.as_tensor(depths).to(dev), torch.as_tensor(poses), torch.as_tensor(K),
                                 None if images is None else torch.as_tensor(images).to(dev), z_thresh, n_thresh,
                                 return_dense=True, **kw)
    torch.cuda.synchronize()
    return out


def compare(tag, res, pts, n_valid, valid, bound):
    """Dense device outputs of the references in `res` against the checker; prints every figure before asserting."""
    pts, n_valid, valid = pts.cpu().double(), n_valid.cpu().long(), valid.cpu().reshape(n_valid.shape)
    mask_share, pts_share = fo.shares(res)
    keep, mask_amb, set_amb = res['keep'], res['mask_amb'], res['set_amb']
    differ = int(((valid != keep) & mask_amb).sum())
    ok = keep & valid & ~(set_amb | res['sample_amb'])
    err = float((pts - res['pts']).abs().amax(-1)[ok].max())
    print('%s: mask-ambiguous %.4f %% (%d of them differ), left out of point comparison %.4f %%, max point error %.4g m '
          '= %.2f x the reference\'s own (bound %.1f x), %d points compared'
          % (tag, 100 * mask_share, differ, 100 * pts_share, err, err / (bound / 4), 4.0, int(ok.sum())))
    assert mask_share <= fo.MASK_CAP and pts_share <= fo.SET_CAP
    assert torch.equal(valid[~mask_amb], keep[~mask_amb])
    assert bool((res['n_lo'] <= n_valid).all()) and bool((n_valid <= res['n_hi']).all())
    assert torch.equal(n_valid[~set_amb], res['n'][~set_amb])
    assert int(ok.sum()) > 0 and err <= bound
    return err


@pytest.mark.parametrize('case', CASES)
def test_goldens(cuda, case):
    """Mask, counts, points, order and colours against the reference's outputs and the float64 checker.  Measured on MI355X:
    point error / the reference's own error = a 1.03, b 1.18, c 0.95, d 1.29 (bound 4); no mask pixel differs from the
    reference's; largest |HIP - reference| 1.9e-6 m (a, b), 9.5e-7 m (c), 1.4e-6 m (d)."""
    fusion = v3d('fusion')
    g, res, refs, lists = load_case(case)
    zt, nt = float(g['z_thresh']), int(g['n_consistent_thresh'])
    if refs is None:
        fused = fusion.process_scene(g['depths'], g['images'], g['poses'], g['K'], zt, nt)
        dense = run_dense(cuda, g['depths'], g['poses'], g['K'], g['images'], zt, nt)
    else:
        r, s = refs[0], lists[0]
        fused = fusion.process_depth(g['depths'][r], g['images'][r], g['depths'][s], g['images'][s], g['poses'][r],
                                     g['poses'][s], g['K'][r], g['K'][s], zt, nt)
        fused = (fused[0], fused[1], fused[2][None])
        ofs, src = np.array([0, len(s)]), np.array(s)
        dense = run_dense(cuda, g['depths'], g['poses'], g['K'], g['images'], zt, nt, src_lists=(ofs, src), ref_idx=[r])
    pts_c, rgb_c, valid, count, pts, n_valid = dense
    compare('golden %s' % case, res, pts, n_valid, valid, 4 * REF_ERR[case])
    f_pts, f_rgb, f_valid = fused
    assert f_pts.dtype == np.float32 and f_rgb.dtype == g['images'].dtype and f_valid.dtype == np.bool_
    assert np.array_equal(f_valid, valid.cpu().numpy()) and f_pts.shape[0] == int(count) == int(f_valid.sum())
    assert np.array_equal(f_pts, pts_c[:int(count)].cpu().numpy())
    if np.array_equal(f_valid, g['all_valid']):
        # same mask -> same order: row i of the output is row i of the reference's
        stride = int(g['pts_stride'])
        assert np.array_equal(f_rgb, g['fused_rgb'])
        amb = (res['set_amb'] | res['sample_amb']).numpy().reshape(f_valid.shape)[f_valid][::stride]
        d = np.abs(f_pts[::stride].astype(np.float64) - g['fused_pts'])[~amb]
        print('golden %s: max |HIP - reference| %.4g m over %d rows' % (case, d.max(), d.shape[0]))
        assert d.max() <= 5 * REF_ERR[case]          # both within their bound of the float64 point
    else:
        same = f_valid == g['all_valid']
        print('golden %s: %d mask pixels differ from the reference (all ambiguous)' % (case, int((~same).sum())))
        assert bool(res['mask_amb'].numpy().reshape(same.shape)[~same].all())


def _clean_scene(n, size, yaw=5):
    return fo.scene(n, size, seed=11, yaw_step_deg=yaw, sigma=0.0, zero_frac=0.0)


@pytest.mark.parametrize('size', [(17, 41), (34, 82)])
def test_noise_free_scene_keeps_what_three_views_see(cuda, size):
    """Noise-free analytic depths.  (1) Every pixel whose point at least 3 other views see consistently is kept: that is
    `compare`'s mask check against the float64 checker, on every mask-unambiguous pixel.  (2) The fused point is the
    back-projected point X up to the nearest-texel offset.  This deviates from the issue, which asks for equality within the
    fp32 bound (6e-6 m): that cannot hold, because a source contributes the back-projection of (u, v) with the depth of the
    NEAREST TEXEL, up to half a texel away on a slanted wall.  X and the sample lie on the same source ray, so they are
    |z_s - z| * |K^-1 (u, v, 1)| apart, and on a noise-free map |z_s - z| <= (Gx + Gy) / 2 with Gx, Gy the largest depth
    difference of horizontally / vertically neighbouring texels.  The bound below is that product with the longest ray of
    the image; it halves with the texel size (6.3 cm at 17 x 41, 3.2 cm at 34 x 82; z_thresh is 10 cm).  Measured on
    MI355X: 2.47 cm and 1.38 cm."""
    d, img, poses, K = _clean_scene(8, size)
    res = fo.check_scene(d, poses, K, 0.1, 3)
    _, _, valid, _, pts, n_valid = run_dense(cuda, d, poses, K, img, 0.1, 3)
    compare('noise-free %dx%d' % size, res, pts, n_valid, valid, 4 * YARDSTICK)
    X = fo.check_scene(d, poses, K, 0.1, 3, src_lists=[[]] * 8)['pts']          # no sources: pts = X / 1
    h, w = size
    corners = torch.tensor([[0., 0., 1.], [w - 1., 0., 1.], [0., h - 1., 1.], [w - 1., h - 1., 1.]]).double().T
    ray = float((torch.inverse(K[0].double()) @ corners).norm(dim=0).max())
    gx, gy = float((d[:, :, 1:] - d[:, :, :-1]).abs().max()), float((d[:, 1:] - d[:, :-1]).abs().max())
    bound = 0.5 * (gx + gy) * ray
    kept = valid.cpu().reshape(8, -1)
    dev = float((pts.cpu().double() - X).norm(dim=-1)[kept].max())
    print('noise-free %dx%d: max |fused - back-projected| %.4g m on %d kept pixels, half-texel bound %.4g m'
          % (size + (dev, int(kept.sum()), bound)))
    assert int(kept.sum()) > 0 and bound < 0.1 and dev <= bound


def test_zero_source_map_never_counts(cuda):
    d, img, poses, K = _clean_scene(5, (12, 16))
    _, _, _, _, _, n0 = run_dense(cuda, d, poses, K, None, 0.1, 1)
    d2 = d.clone()
    d2[2] = 0
    _, _, _, _, _, n1 = run_dense(cuda, d2, poses, K, None, 0.1, 1)
    lists = ([0, 3, 6, 9, 12], [1, 3, 4, 0, 3, 4, 0, 1, 4, 0, 1, 3])            # the same scene without view 2 as a source
    _, _, _, _, _, n2 = run_dense(cuda, d, poses, K, None, 0.1, 1, src_lists=lists, ref_idx=[0, 1, 3, 4])
    assert torch.equal(n1[[0, 1, 3, 4]], n2) and bool((n1 <= n0).all()) and int(n0.sum()) > int(n1.sum())


@pytest.mark.parametrize('thresh', [1, 'n-1'])
def test_consistency_threshold_extremes(cuda, thresh):
    d, img, poses, K = fo.scene(6, (12, 16), seed=12, yaw_step_deg=2, sigma=0.01)
    t = 5 if thresh == 'n-1' else 1
    pts_c, rgb_c, valid, count, pts, n_valid = run_dense(cuda, d, poses, K, img, 0.1, t)
    want = n_valid.reshape(6, 12, 16) >= t
    assert torch.equal(valid, want) and int(count) == int(want.sum())
    assert 0 < int(count) < want.numel() or t == 1
    sel = want.reshape(6, -1)
    assert torch.equal(pts_c[:int(count)], pts[sel]) and torch.equal(rgb_c[:int(count)], img.to(cuda).reshape(6, -1, 3)[sel])
    compare('threshold %s' % thresh, fo.check_scene(d, poses, K, 0.1, t), pts, n_valid, valid, 4 * YARDSTICK)


def test_window_equals_explicit_lists_and_process_depth_equals_scene_slice(cuda):
    fusion = v3d('fusion')
    d, img, poses, K = fo.scene(7, (17, 41), seed=13, yaw_step_deg=3, sigma=0.02)
    a = run_dense(cuda, d, poses, K, img, 0.1, 2, src_window=(2, 1))
    ofs, src = fusion.window_lists(7, (2, 1))
    b = run_dense(cuda, d, poses, K, img, 0.1, 2, src_lists=(ofs, src))
    m = int(a[3])
    assert m == int(b[3]) and torch.equal(a[0][:m], b[0][:m]) and torch.equal(a[1][:m], b[1][:m])       # rows >= m are unspecified
    for x, y in zip(a[2:], b[2:]):
        assert torch.equal(x, y)
    full = run_dense(cuda, d, poses, K, img, 0.1, 2)
    assert not torch.equal(a[5], full[5])                      # the window really drops sources
    s_pts, s_rgb, s_valid = fusion.process_scene(d, img, poses, K, 0.1, 2)
    first = 0
    for r in range(7):
        srcs = [s for s in range(7) if s != r]
        p, c, v = fusion.process_depth(d[r], img[r], d[srcs], img[srcs], poses[r], poses[srcs], K[r], K[srcs], 0.1, 2)
        m = int(v.sum())
        assert np.array_equal(v, s_valid[r]) and np.array_equal(p, s_pts[first:first + m])
        assert np.array_equal(c, s_rgb[first:first + m])
        first += m
    assert first == s_pts.shape[0]


def test_smallest_and_odd_sizes(cuda):
    for size in ((2, 3), (17, 41)):
        d, img, poses, K = fo.scene(4, size, seed=14, yaw_step_deg=1, sigma=0.005)
        res = fo.check_scene(d, poses, K, 0.1, 2)
        _, _, valid, _, pts, n_valid = run_dense(cuda, d, poses, K, img.float(), 0.1, 2)        # fp32 colours: 12-byte pixels
        compare('size %dx%d' % size, res, pts, n_valid, valid, 4 * YARDSTICK)


def test_error_codes(cuda):
    fusion, lib_mod = v3d('fusion'), v3d('_lib')
    d, img, poses, K = _clean_scene(3, (4, 6))
    with pytest.raises(lib_mod.V3DLibraryError, match='V3D_ERR_BAD_SHAPE'):
        fusion.fuse_depth_maps(d[:, :1].to(cuda), poses, K)
    with pytest.raises(lib_mod.V3DLibraryError, match='V3D_ERR_BAD_SHAPE'):
        fusion.fuse_depth_maps(d[:, :, :1].contiguous().to(cuda), poses, K)
    with pytest.raises(lib_mod.V3DLibraryError, match='source index 3'):
        fusion.fuse_depth_maps(d.to(cuda), poses, K, src_lists=([0, 1, 2, 3], [1, 3, 0]))
    with pytest.raises(lib_mod.V3DLibraryError, match='reference index'):
        fusion.fuse_depth_maps(d.to(cuda), poses, K, ref_idx=[0, 7])


@pytest.mark.parametrize('size', [(256, 320), (480, 640)])
def test_full_size_scene(cuda, size):
    """64 views (the cfg3 ring, sigma = 4 cm, 3 % zeroed pixels): every output element of 8 evenly spaced reference views
    against all 63 sources is compared with the float64 checker of the same fp32 inputs; then ten launches beside a GEMM on
    a second stream are bit-identical.  Shares of ambiguous pixels of the float64 checker ALONE on these inputs (measured on
    the CPU before any GPU run, sigma = 4 cm): 256 x 320 mask-ambiguous 0.011 %, left out of the point comparison 1.49 %
    (source-set-ambiguous 0.28 %); 480 x 640: 0.025 %, 2.98 % (0.54 %) -- inside the 2 % / 10 % caps, no lower sigma needed.
    Measured on MI355X: point error 1.20 x (256 x 320) and 1.31 x (480 x 640) the reference's own fp32 error (bound 4 x); 0 and 19
    of the mask-ambiguous pixels differ from the float64 mask."""
    d, img, poses, K = fo.scene(64, size, seed=1237, yaw_step_deg=None, sigma=0.04)
    refs = list(range(0, 64, 8))
    res = fo.check_scene(d, poses, K, 0.1, 3, refs)
    dev_d, dev_img = d.to(cuda), img.to(cuda)
    fusion = v3d('fusion')
    out = fusion.fuse_depth_maps(dev_d, poses, K, dev_img, 0.1, 3, return_dense=True)
    torch.cuda.synchronize()
    pts_c, rgb_c, valid, count, pts, n_valid = out
    compare('full size %dx%d' % size, res, pts[refs], n_valid[refs], valid[refs], 4 * YARDSTICK)
    m = int(count)
    assert m == int(valid.sum()) and torch.equal(pts_c[:m], pts[valid.reshape(64, -1)])
    assert torch.equal(rgb_c[:m], dev_img.reshape(64, -1, 3)[valid.reshape(64, -1)])
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=cuda)
    for _ in range(10):
        with torch.cuda.stream(side):
            for _ in range(4):
                a @ a
        again = fusion.fuse_depth_maps(dev_d, poses, K, dev_img, 0.1, 3, return_dense=True)
        torch.cuda.synchronize()
        assert int(again[3]) == m
        assert torch.equal(again[0][:m], pts_c[:m]) and torch.equal(again[1][:m], rgb_c[:m])
        assert torch.equal(again[2], valid) and torch.equal(again[4], pts) and torch.equal(again[5], n_valid)
