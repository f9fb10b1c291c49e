"""CPU: the float64 fusion checker (tests/fusion_oracle.py) against the reference's own outputs (tests/golden/F_fusion_*.npz,
written by tests/golden/make_golden_fusion.py), the host preparation of ``fusion.fuse_preds``, and the no-fallback rule."""
import numpy as np
import pytest
import torch

import fusion_oracle as fo
from conftest import ROOT, v3d

CASES = ('a', 'b', 'c', 'd')
# max |reference fp32 - float64 checker| over the compared points, metres (test_checker_reproduces_the_reference prints them)
REF_ERR = {'a': 1.372e-6, 'b': 1.426e-6, 'c': 9.06e-7, 'd': 8.18e-7}


def load_case(c):
    g = np.load('%s/tests/golden/F_fusion_%s.npz' % (ROOT, c))
    g = {k: g[k] for k in g.files}
    refs, lists = (None, None) if 'ref' not in g else ([int(g['ref'])], [[int(s) for s in g['srcs']]])
    res = fo.check_scene(torch.from_numpy(g['depths']), torch.from_numpy(g['poses']), torch.from_numpy(g['K']),
                         float(g['z_thresh']), int(g['n_consistent_thresh']), refs, lists)
    return g, res, refs, lists


@pytest.mark.parametrize('case', CASES)
def test_checker_reproduces_the_reference(case):
    """The checker's mask equals the reference's ``all_valid`` on every mask-unambiguous pixel, the ambiguous shares stay
    under the caps (2 % mask, 10 % source set / sample), and the reference's fused points agree with the float64 points on
    the kept, unambiguous pixels.  Measured reference-vs-float64 maximum error (the yardstick of the GPU tests):
    a 1.372e-6 m, b 1.426e-6 m, c 9.06e-7 m, d 8.18e-7 m; shares of ambiguous pixels (mask, points): a 0 / 0.26 %,
    b 0.012 % / 0.41 %, c 0 / 0.17 %, d 0 / 0.13 %.  Without the `sample_amb` rule of the checker case b holds a pixel where
    the reference itself is 6.9 mm from the float64 point (it read the neighbouring texel)."""
    g, res, _, _ = load_case(case)
    n_ref = res['keep'].shape[0]
    gold = g['all_valid'].reshape(n_ref, -1)
    keep, mask_amb = res['keep'].numpy(), res['mask_amb'].numpy()
    mask_share, pts_share = fo.shares(res)
    print('case %s: mask-ambiguous %.4f %%, left out of the point comparison %.4f %%' % (case, 100 * mask_share, 100 * pts_share))
    assert mask_share <= fo.MASK_CAP and pts_share <= fo.SET_CAP
    assert int(g['n_fused']) == int(gold.sum())
    assert np.array_equal(keep[~mask_amb], gold[~mask_amb])
    dense, has = fo.dense_from_compact(g['fused_pts'], g['all_valid'], int(g['pts_stride']))
    ok = has & keep & ~(res['set_amb'] | res['sample_amb']).numpy()
    assert ok.sum() > 0.5 * has.sum()
    err = np.abs(dense - res['pts'].numpy()).max(-1)[ok].max()
    print('case %s: reference vs float64 max error %.4g m over %d points' % (case, err, ok.sum()))
    assert err <= 1.05 * REF_ERR[case]          # the recorded yardstick is what this reference run gives
    assert err < 1e-5                           # ~ 20 ulps of a 6 m coordinate


def test_checker_flags_boundary_pairs():
    """A pair exactly on a decision boundary is uncertain; far from every boundary it is certain."""
    d = torch.full((2, 4, 4), 2.0)
    poses = torch.eye(4).repeat(2, 1, 1)
    K = torch.tensor([[4., 0., 1.5], [0., 4., 1.5], [0., 0., 1.]]).repeat(2, 1, 1)
    res = fo.check_view(d, poses, K, 0, [1], 0.1, 1)
    inner = torch.tensor([5, 6, 9, 10])                      # the border pixels project exactly onto u = 0 / w-1: uncertain
    assert bool((res['n'] == 1).all()) and not bool(res['set_amb'][inner].any()) and bool(res['set_amb'][0])
    d[1] = 2.1                                               # |z - z_s| sits on z_thresh
    res = fo.check_view(d, poses, K, 0, [1], 0.1, 1)
    assert bool(res['set_amb'].all()) and bool(res['mask_amb'].all())
    assert bool((res['n_lo'] == 0).all()) and bool((res['n_hi'] == 1).all())


def _record():
    n, h, w = 3, 4, 6
    rng = np.random.RandomState(0)
    return dict(depth_preds=rng.rand(n, h, w).astype(np.float32) + 1, rotmats=rng.rand(n, 3, 3).astype(np.float32),
                tvecs=rng.rand(n, 3).astype(np.float32),
                K=np.tile(np.array([[5., 0., 3.], [0., 6., 2.], [0., 0., 1.]], dtype=np.float32), (n, 1, 1)),
                init_prob=rng.rand(n, h, w).astype(np.float32), final_prob=rng.rand(n, h, w).astype(np.float32))


def test_prepare_preds_host_logic(tmp_path):
    fusion = v3d('fusion')
    rec = _record()
    keep0 = rec['depth_preds'].copy()
    depths, poses, K = fusion.prepare_preds(rec)
    assert np.array_equal(rec['depth_preds'], keep0), 'the record must not be written to'
    assert np.array_equal(poses[:, :3, :3], rec['rotmats']) and np.array_equal(poses[:, :3, 3], rec['tvecs'])
    assert np.array_equal(poses[:, 3], np.tile(np.array([0, 0, 0, 1], dtype=np.float32), (3, 1)))
    want = np.where((rec['init_prob'] > 0.2) & (rec['final_prob'] > 0.1), rec['depth_preds'], 0).astype(np.float32)
    assert np.array_equal(depths, want) and (depths == 0).any() and (depths != 0).any()
    assert np.array_equal(K, rec['K'])
    # nearest resize to (8, 9): rows doubled, columns by floor(x * 6 / 9); K rows rescaled by 9/6 and 8/4
    d2, _, K2 = fusion.prepare_preds(rec, out_size=(8, 9))
    cols = np.floor(np.arange(9) * 6 / 9.).astype(int)
    assert d2.shape == (3, 8, 9) and np.array_equal(d2, want[:, np.arange(8) // 2][:, :, cols])
    assert np.allclose(K2[:, 0], rec['K'][:, 0] * 1.5) and np.allclose(K2[:, 1], rec['K'][:, 1] * 2.0)
    assert np.array_equal(K2[:, 2], rec['K'][:, 2]) and np.array_equal(rec['K'][0, 0], [5., 0., 3.])
    # the same record from a file; without the probability maps nothing is masked
    path = str(tmp_path / 'preds.npz')
    np.savez(path, **rec)
    d3, p3, K3 = fusion.prepare_preds(path)
    assert np.array_equal(d3, depths) and np.array_equal(p3, poses) and np.array_equal(K3, K)
    del rec['init_prob'], rec['final_prob']
    assert np.array_equal(fusion.prepare_preds(rec)[0], keep0)
    rec['init_prob'] = np.ones((3, 2, 3), dtype=np.float32)
    with pytest.raises(ValueError, match='init_prob'):
        fusion.prepare_preds(rec)


def test_camera_blocks_and_window_lists():
    fusion = v3d('fusion')
    _, _, poses, K = fo.scene(4, (6, 8), seed=1, yaw_step_deg=5, sigma=0.0)
    cam = fusion.camera_blocks(poses, K)
    assert cam.shape == (4, 48) and cam.dtype == torch.float32
    assert torch.equal(cam[:, 9:18].reshape(4, 3, 3), torch.inverse(K))
    assert torch.equal(cam[:, 30:42].reshape(4, 3, 4), torch.inverse(poses)[:, :3])
    assert torch.equal(cam[:, 18:27].reshape(4, 3, 3), poses[:, :3, :3]) and torch.equal(cam[:, 27:30], poses[:, :3, 3])
    ofs, src = fusion.window_lists(5, (1, 2))
    assert ofs.tolist() == [0, 2, 5, 8, 10, 11] and src.tolist() == [1, 2, 0, 2, 3, 1, 3, 4, 2, 4, 3]
    ofs, src = fusion.window_lists(5, (1, 0), ref_idx=[0, 3])
    assert ofs.tolist() == [0, 0, 1] and src.tolist() == [2]


def test_no_cpu_fallback():
    fusion, lib_mod = v3d('fusion'), v3d('_lib')
    d, img, poses, K = fo.scene(3, (4, 6), seed=1, yaw_step_deg=5, sigma=0.0)
    with pytest.raises(lib_mod.V3DLibraryError):
        fusion.fuse_depth_maps(d, poses, K)                  # host tensors are never computed on
    with pytest.raises(lib_mod.V3DLibraryError):
        fusion.process_scene(d, img, poses, K, 0.1, 1, device='cpu')
    if torch.cuda.is_available():
        return                                               # with a device the remaining entries run (tests/test_fusion_gpu.py)
    with pytest.raises(lib_mod.V3DLibraryError):
        fusion.process_scene(d, img, poses, K, 0.1, 1)
    with pytest.raises(lib_mod.V3DLibraryError):
        fusion.process_depth(d[0], img[0], d[1:], img[1:], poses[0], poses[1:], K[0], K[1:])
    with pytest.raises(lib_mod.V3DLibraryError):
        fusion.fuse_preds(dict(depth_preds=d.numpy(), rotmats=poses[:, :3, :3].numpy(), tvecs=poses[:, :3, 3].numpy(),
                               K=K.numpy()), img, 0.1, 1)


def test_host_side_argument_validation():
    """Error paths of the C ABI that return before touching the device."""
    import ctypes
    lib_mod = v3d('_lib')
    lib = lib_mod.load()
    assert lib.v3d_fusion_workspace_bytes(4, 1, 8) == 0 and lib.v3d_fusion_workspace_bytes(4, 8, 1) == 0
    assert lib.v3d_fusion_workspace_bytes(64, 256, 320) >= (64 * 2 + 1 + 64 * 64) * 4 + 2 * 64 * 320 * 4
    buf = (ctypes.c_int * 64)()
    p = ctypes.addressof(buf)
    ip = p
    assert lib.v3d_fuse_depths_f32(p, p, 4, 1, 8, None, 4, None, None, 0.1, p, p, p, 1 << 20, None) == -1
    assert b'h=1' in lib.v3d_last_error()
    assert lib.v3d_fuse_depths_f32(p, p, 4, 8, 1, None, 4, None, None, 0.1, p, p, p, 1 << 20, None) == -1
    assert lib.v3d_fuse_depths_f32(None, p, 4, 8, 8, None, 4, None, None, 0.1, p, p, p, 1 << 20, None) == -2
    assert lib.v3d_fuse_depths_f32(p, p, 4, 8, 8, None, 4, None, None, 0.1, p, p, p, 16, None) == -3
    ofs = (ctypes.c_int * 5)(0, 1, 2, 3, 4)
    src = (ctypes.c_int * 4)(1, 0, 4, 2)                       # 4 is not an image of a 4-image stack
    assert lib.v3d_fuse_depths_f32(p, p, 4, 8, 8, None, 4, ofs, src, 0.1, p, p, p, 1 << 20, None) == -2
    assert b'source index 4' in lib.v3d_last_error()
    assert lib.v3d_fuse_depths_f32(p, p, 4, 8, 8, None, 2, None, None, 0.1, p, p, p, 1 << 20, None) == -2    # n_ref != n_img, no list
    assert lib.v3d_fusion_compact(p, p, None, 0, 4, 1, 8, 3, p, ip, ip, p, None, ip, p, 1 << 20, None) == -1
    assert lib.v3d_fusion_compact(p, p, p, 3, 4, 8, 8, 3, p, ip, ip, p, None, ip, p, 1 << 20, None) == -2
