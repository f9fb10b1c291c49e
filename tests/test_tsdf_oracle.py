"""CPU: the float64 checker of TSDF integration (tests/tsdf_oracle.py) against the reference's recorded volumes
(tests/golden/T_tsdf_*.npz, written by tests/golden/make_golden_tsdf.py), the host side of 3dvnet_amd/tsdf.py (projection
matrices, volume bounds, the TSDF holder's save / load, validation, the no-fallback rule) and the host-side error codes of the
two C entry points.

Recorded with the fixtures (the reference's own fp32 volumes against the checker, outside the uncertain set; REF_ERR below
is read from the files): largest error of the tsdf sum a 8.47e-6, b 6.43e-7, c 8.47e-6, d 8.17e-7; of the averaged tsdf
a 2.68e-6, b 6.16e-7, d 5.91e-7; colour sums exact (integers), averaged colours a 6.1e-6, d 5.09e-6.  Uncertain share of the
touched voxels: a / c 0.217 %, b 0.058 %, d 0 (cap 0.5 %); no weight differs outside the set.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import tsdf_oracle as to
from conftest import ROOT, v3d

CASES = ['a', 'b', 'c', 'd']
EPS32 = 2.0 ** -23
_cache = {}


def colors_of(images_u8):
    """What the TSDF branch feeds: BGR, [N, 3, h, w] float."""
    return torch.as_tensor(images_u8)[..., [2, 1, 0]].permute(0, 3, 1, 2).float().contiguous()


def dense(g, prefix=''):
    """The recorded sparse state -> dense fp32 volumes dict(weight, tsdf_sum, tsdf_avg, color_sum, color_avg)."""
    n_vox = int(np.prod(g['voxel_dim']))
    idx = g[prefix + 'idx'].astype(np.int64)
    out = {}
    for key, fill in (('weight', 0.), ('tsdf_sum', -1.), ('tsdf_avg', -1.)):
        vol = np.full(n_vox, fill, dtype=np.float32)
        vol[idx] = g[prefix + key].astype(np.float32)
        out[key] = vol
    for key in ('color_sum', 'color_avg'):
        out[key] = None
        if prefix + key in g:
            vol = np.zeros((3, n_vox), dtype=np.float32)
            vol[:, idx] = g[prefix + key]
            out[key] = vol
    return out


def load_case(case):
    """-> (fixture dict, dense reference volumes, checker result, colours fed | None); computed once, shared, not modified."""
    if case not in _cache:
        with np.load(os.path.join(ROOT, 'tests', 'golden', 'T_tsdf_%s.npz' % case)) as f:
            g = {k: f[k] for k in f.files}
        cols = colors_of(g['images']) if bool(g['color']) else None
        res = to.integrate(g['voxel_dim'], float(g['voxel_size']), g['origin'], float(g['voxel_size']) * float(g['trunc_ratio']),
                           g['projections'], g['depths'], cols)
        _cache[case] = (g, dense(g), res, cols)
    return _cache[case]


def ref_err(case):
    g = load_case(case)[0]
    return {k[8:]: float(g[k]) for k in g if k.startswith('ref_err_')}


def value_bound(g):
    """What an fp32 evaluation of the sum may be off by, from the formats alone: per view the camera depth c2 is a 4-term
    chain (each rounding at most an ulp of the largest partial sum, |row| . |world| + |t|), the subtraction and the division
    add an ulp of the quotient (<= 1 in magnitude where it counts), and each of the n additions an ulp of a sum <= n."""
    P = g['projections'].astype(np.float64)
    ax = to.world_axes(g['voxel_dim'], float(g['voxel_size']), g['origin'])
    far = np.array([np.abs(a).max() for a in ax], dtype=np.float64)
    scale = float((np.abs(P[:, 2, :3]) @ far + np.abs(P[:, 2, 3])).max())
    n = P.shape[0]
    tm = float(g['voxel_size']) * float(g['trunc_ratio'])
    return n * (4 * EPS32 * scale / tm + 2 * EPS32 + EPS32 * n)


@pytest.mark.parametrize('case', CASES)
def test_checker_reproduces_the_reference(case):
    g, ref, res, cols = load_case(case)
    touched = ref['weight'] > 0
    share = to.uncertain_share(res, ref['weight'])
    mism = to.weight_mismatches(res, ref['weight'])
    err = to.errors(res, ref['tsdf_sum'], ref['color_sum'], ref['tsdf_avg'], ref['color_avg'])
    bound = value_bound(g)
    print('case %s: %d touched voxels, uncertain %.4f %%, %d weight mismatches outside, reference errors %s, bound %.3g'
          % (case, int(touched.sum()), 100 * share, mism, err, bound))
    assert int(touched.sum()) > 0 and share <= to.UNCERTAIN_CAP
    assert mism == 0
    assert err['tsdf'] <= bound and err['tsdf_avg'] <= bound
    if cols is not None:
        assert err['color'] == 0.0                                      # sums of small integers are exact in fp32
        assert err['color_avg'] <= 255 * EPS32
    rec = ref_err(case)
    assert set(rec) == set(err)
    for k in err:
        assert err[k] == pytest.approx(rec[k], rel=1e-6, abs=1e-12), k
    # the intermediate state of case c: the first three views alone
    if int(g['mid']):
        m = int(g['mid'])
        mid = dense(g, 'mid_')
        res3 = to.integrate(g['voxel_dim'], float(g['voxel_size']), g['origin'], float(g['voxel_size']) * float(g['trunc_ratio']),
                            g['projections'][:m], g['depths'][:m], cols[:m])
        assert to.weight_mismatches(res3, mid['weight']) == 0
        assert to.errors(res3, mid['tsdf_sum'])['tsdf'] <= bound


def test_checker_properties():
    """Never-seen voxels keep the fill value, an all-zero view adds nothing, the order of the views leaves the weights."""
    g, ref, res, cols = load_case('d')
    args = (g['voxel_dim'], float(g['voxel_size']), g['origin'], float(g['voxel_size']), g['projections'], g['depths'], cols)
    assert bool((g['depths'][1] == 0).all())
    no1 = to.integrate(*args, order=[0, 2, 3, 4])
    assert torch.equal(no1['weight'], res['weight']) and torch.equal(no1['tsdf'], res['tsdf'])
    rev = to.integrate(*args, order=[4, 3, 2, 1, 0])
    assert torch.equal(rev['weight'], res['weight'])
    gb, refb, resb, _ = load_case('b')
    unseen = resb['weight'] == 0
    assert int(unseen.sum()) > 0 and bool((resb['tsdf'][unseen] == -1).all())
    plus = to.integrate(gb['voxel_dim'], float(gb['voxel_size']), gb['origin'], 3 * float(gb['voxel_size']), gb['projections'],
                        gb['depths'], fill=1.0)
    assert bool((plus['tsdf'][unseen] == 1).all()) and torch.equal(plus['tsdf'][~unseen], resb['tsdf'][~unseen])


def test_projection_matrices_and_volume_bounds():
    tsdf = v3d('tsdf')
    g = load_case('a')[0]
    P = tsdf.projection_matrices(torch.from_numpy(g['K']), torch.from_numpy(g['poses']))
    assert P.shape == (6, 3, 4) and P.dtype == torch.float32
    np.testing.assert_allclose(P.numpy(), g['projections'], rtol=1e-6, atol=1e-6)
    want = g['K'][2].astype(np.float64) @ g['poses'][2][:3].astype(np.float64)
    np.testing.assert_allclose(P[2].numpy(), want, rtol=1e-5, atol=1e-5)
    kw = dict(vol_prcnt=float(g['bounds_vol_prcnt']), vol_margin=float(g['bounds_vol_margin']),
              vox_res=float(g['bounds_vox_res']), img_batch=int(g['bounds_img_batch']))
    origin, vol_max, dim = tsdf.volume_bounds(g['depths'], g['K'], g['poses'], **kw)
    assert origin.dtype == torch.float32 and origin.shape == (3,) and vol_max.shape == (3,)
    np.testing.assert_allclose(origin.numpy(), g['bounds_origin'], rtol=0, atol=1e-5)
    np.testing.assert_allclose(vol_max.numpy(), g['bounds_max'], rtol=0, atol=1e-5)
    assert dim == g['bounds_dim'].tolist() == g['voxel_dim'].tolist()
    # two batches (4 + 2 views) take the running minimum / maximum of the per-batch bounds
    lo = [tsdf.volume_bounds(g['depths'][s], g['K'][s], g['poses'][s], **kw) for s in (slice(0, 4), slice(4, 6))]
    assert torch.equal(origin, torch.minimum(lo[0][0], lo[1][0])) and torch.equal(vol_max, torch.maximum(lo[0][1], lo[1][1]))
    # a batch without a usable pixel is skipped; a scene without any is an error
    d = g['depths'].copy()
    d[4:] = 0
    o2, m2, _ = tsdf.volume_bounds(d, g['K'], g['poses'], **kw)
    assert torch.equal(o2, lo[0][0]) and torch.equal(m2, lo[0][1])
    with pytest.raises(ValueError):
        tsdf.volume_bounds(np.zeros_like(d), g['K'], g['poses'], **kw)
    with pytest.raises(ValueError):
        tsdf.projection_matrices(torch.eye(3)[None], torch.eye(4).repeat(2, 1, 1))


def test_tsdf_save_load_round_trip(tmp_path):
    tsdf = v3d('tsdf')
    vol = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4) / 24 - 0.5
    t = tsdf.TSDF(0.04, torch.tensor([[1., 2., 3.]]), vol, {'weight': torch.ones(2, 3, 4), 'color': torch.rand(3, 2, 3, 4)})
    path = str(tmp_path / 'tsdf.npz')
    t.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ['color', 'origin', 'tsdf', 'voxel_size', 'weight']        # the reference's keys
        assert f['origin'].shape == (1, 3) and float(f['voxel_size']) == 0.04
    back = tsdf.TSDF.load(path)
    assert back.voxel_size == 0.04 and torch.equal(back.origin, t.origin) and torch.equal(back.tsdf_vol, vol)
    assert torch.equal(back.attribute_vols['color'], t.attribute_vols['color'])
    assert torch.equal(back.attributes['weight'], t.attribute_vols['weight'])               # where the reference's load puts it
    only = tsdf.TSDF.load(path, voxel_types=['tsdf'])
    assert 'color' not in only.attribute_vols
    assert back.to('cpu') is back and back.device == 'cpu'
    assert tsdf.TSDF(0.04, t.origin, vol).attribute_vols == {}


def test_host_validation_of_the_c_abi():
    """Errors that return before anything touches the device."""
    lib = v3d('_lib').load()
    one = ctypes.c_void_p(256)                            # never dereferenced: every call below fails first
    org = (ctypes.c_float * 3)(0., 0., 0.)
    integ, norm = lib.v3d_tsdf_integrate_f32, lib.v3d_tsdf_normalize_f32
    assert integ(None, one, None, 4, 4, 4, 0.04, org, 0.12, one, one, None, 1, 4, 4, None) == -2
    assert b'null' in lib.v3d_last_error()
    assert integ(one, None, None, 4, 4, 4, 0.04, org, 0.12, one, one, None, 1, 4, 4, None) == -2
    assert integ(one, one, None, 4, 4, 4, 0.04, None, 0.12, one, one, None, 1, 4, 4, None) == -2
    assert integ(one, one, None, 4, 4, 4, 0.04, org, 0.12, None, one, None, 1, 4, 4, None) == -2
    assert integ(one, one, None, 4, 4, 4, 0.04, org, 0.12, one, None, None, 1, 4, 4, None) == -2
    for vs, tm in ((0.0, 0.12), (-0.04, 0.12), (float('nan'), 0.12), (float('inf'), 0.12), (0.04, 0.0), (0.04, -1.0),
                   (0.04, float('nan')), (0.04, float('inf'))):
        assert integ(one, one, None, 4, 4, 4, vs, org, tm, one, one, None, 1, 4, 4, None) == -2, (vs, tm)
    assert integ(one, one, None, 4, 4, 4, 0.04, org, 0.12, one, one, one, 1, 4, 4, None) == -2       # images, no colour volume
    assert b'together' in lib.v3d_last_error()
    assert integ(one, one, one, 4, 4, 4, 0.04, org, 0.12, one, one, None, 1, 4, 4, None) == -2       # colour volume, no images
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (2048, 1024, 1024), (65536, 65536, 1)):
        assert integ(one, one, None, dims[0], dims[1], dims[2], 0.04, org, 0.12, one, one, None, 1, 4, 4, None) == -1, dims
    assert integ(one, one, None, 4, 4, 4, 0.04, org, 0.12, one, one, None, -1, 4, 4, None) == -1
    assert integ(one, one, None, 4, 4, 4, 0.04, org, 0.12, one, one, None, 1, 0, 4, None) == -1
    assert integ(one, one, None, 4, 4, 4, 0.04, org, 0.12, one, one, None, 1, 4, -3, None) == -1
    assert integ(one, one, None, 4, 4, 4, 0.04, org, 0.12, one, one, None, 0, 4, 4, None) == 0        # no views: nothing to do
    assert integ(one, one, one, 4, 4, 4, 0.04, org, 0.12, None, None, None, 0, 0, 0, None) == 0
    assert norm(None, one, None, 8, one, None, None) == -2 and b'null' in lib.v3d_last_error()
    assert norm(one, None, None, 8, one, None, None) == -2
    assert norm(one, one, None, 8, None, None, None) == -2
    assert norm(one, one, one, 8, one, None, None) == -2
    assert norm(one, one, None, 8, one, one, None) == -2
    assert norm(one, one, None, 0, one, None, None) == -1
    assert norm(one, one, None, -5, one, None, None) == -1
    assert lib.v3d_version() == 9


def test_no_cpu_fallback_and_no_labels():
    tsdf, lib_mod = v3d('tsdf'), v3d('_lib')
    fus = tsdf.TSDFFusion((4, 3, 2), 0.1, (0., 0., 0.), device='cpu')
    assert fus.tsdf_vol.shape == (24,) and bool((fus.tsdf_vol == -1).all()) and bool((fus.weight_vol == 0).all())
    assert fus.color_vol.shape == (3, 24) and fus.origin.shape == (1, 3) and fus.trunc_margin == pytest.approx(0.3)
    assert fus.voxel_dim == (4, 3, 2)
    fus.reset()
    assert bool((fus.tsdf_vol == 1).all())
    P, d, c = torch.zeros(3, 4), torch.ones(5, 6), torch.zeros(3, 5, 6)
    with pytest.raises(lib_mod.V3DLibraryError):
        fus.integrate(P, d, c)
    with pytest.raises(lib_mod.V3DLibraryError):
        fus.integrate_batch(P[None], d[None], c[None])
    with pytest.raises(lib_mod.V3DLibraryError):
        fus.get_tsdf()
    assert tsdf.TSDFFusion((4, 3, 2), 0.1, (0., 0., 0.), device='cpu', color=False).color_vol is None
    with pytest.raises(NotImplementedError):
        tsdf.TSDFFusion((4, 3, 2), 0.1, (0., 0., 0.), device='cpu', label=True)
    with pytest.raises(NotImplementedError):
        fus.integrate(P, d, c, label=torch.zeros(5, 6))
    if not torch.cuda.is_available():
        rec = dict(depth_preds=np.ones((2, 5, 6), np.float32), rotmats=np.eye(3, dtype=np.float32)[None].repeat(2, 0),
                   tvecs=np.zeros((2, 3), np.float32), K=np.eye(3, dtype=np.float32)[None].repeat(2, 0))
        with pytest.raises(lib_mod.V3DLibraryError):
            tsdf.fuse_preds_tsdf(rec, np.zeros((2, 5, 6, 3), np.uint8))


def test_prepare_preds_tsdf_host_work():
    """Poses from rotmats / tvecs, BGR flip, bilinear resize to the depth size, and no probability masking."""
    tsdf = v3d('tsdf')
    rng = np.random.default_rng(3)
    rec = dict(depth_preds=rng.random((2, 6, 8)).astype(np.float32) + 1, rotmats=np.eye(3, dtype=np.float32)[None].repeat(2, 0),
               tvecs=rng.random((2, 3)).astype(np.float32), K=np.eye(3, dtype=np.float32)[None].repeat(2, 0),
               init_prob=np.zeros((2, 6, 8), np.float32), final_prob=np.zeros((2, 6, 8), np.float32))
    img = rng.integers(0, 256, (2, 12, 16, 3)).astype(np.uint8)
    d, poses, K, cols = tsdf.prepare_preds_tsdf(rec, img)
    assert np.array_equal(d.numpy(), rec['depth_preds'])                 # zero probabilities mask nothing here
    assert np.array_equal(poses[:, :3, 3].numpy(), rec['tvecs']) and bool((poses[:, 3] == torch.tensor([0., 0, 0, 1])).all())
    want = torch.nn.functional.interpolate(torch.from_numpy(img[..., ::-1].copy()).permute(0, 3, 1, 2).float(), (6, 8),
                                           mode='bilinear')
    assert cols.shape == (2, 3, 6, 8) and torch.equal(cols, want)
    with pytest.raises(ValueError):
        tsdf.prepare_preds_tsdf(rec, img[:1])
