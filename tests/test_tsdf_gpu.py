"""GPU: TSDF integration (3dvnet_amd/tsdf.py -> v3d_tsdf_integrate_f32 / v3d_tsdf_normalize_f32, csrc/tsdf.hip) against the
reference's recorded volumes (tests/golden/T_tsdf_*.npz), against the float64 checker (tests/tsdf_oracle.py) at small and
at larger size, and its own invariants.  Every test runs the HIP path through the C ABI.

Two rules (tests/tsdf_oracle.py): the weight equals the reference's / the checker's on every voxel outside the uncertain set,
which may hold at most 0.5 % of the touched voxels; the tsdf sum, the colour sums and the averaged volumes on those voxels
lie within 4 x the reference's own fp32 error against the checker on the same fixture (the project's rule for fp32 routes:
same products, possibly another contraction).  The reference's errors are recorded in the fixtures (figures in
tests/test_tsdf_oracle.py).  Where no reference output exists (the larger case) the yardstick is derived from fixture a: same
room, same depth range, same voxel size and truncation margin, so the same error per view; the error of a sum of n views
grows at most linearly in n, hence ref_err(a) * n / 6.

Measured on one MI355X: error / the reference's own fp32 error (bound 4): tsdf sum a 1.00, b 1.00, c 1.00, d 1.00 (on all four the
HIP sums equal the reference's CPU sums bit for bit outside the uncertain set), averaged tsdf 1.00, colour sums exact, averaged
colours 1.00; case c after three views 0.55.  Uncertain share of the touched voxels: a / c 0.217 %, b 0.058 %, d 0, larger case
0.205 % (cap 0.5 %); no weight differs outside the set anywhere.  Larger case: tsdf sum 4.93e-6 = 0.22 x its yardstick, averaged tsdf
3.07e-6 = 0.43 x.  Wall time of the module's 10 tests: 4.2 s (the float64 checker of the larger case on the CPU: 1.8 s).
"""
import numpy as np
import pytest
import torch

import fusion_oracle as fo
import tsdf_oracle as to
from conftest import v3d
from test_tsdf_oracle import CASES, colors_of, dense, load_case, ref_err

pytestmark = pytest.mark.gpu


def make(dev, g, color=None):
    tsdf = v3d('tsdf')
    color = bool(g['color']) if color is None else color
    return tsdf.TSDFFusion([int(v) for v in g['voxel_dim']], float(g['voxel_size']), g['origin'].tolist(),
                           float(g['trunc_ratio']), dev, color=color)


def state(fus):
    torch.cuda.synchronize()
    return (fus.tsdf_vol.cpu().clone(), fus.weight_vol.cpu().clone(), None if fus.color_vol is None else fus.color_vol.cpu().clone())


def same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def compare(tag, res, fus, bounds, ref=None):
    """Device volumes against the checker (and the reference's weights); prints every figure before asserting."""
    t = fus.get_tsdf()
    tsdf_sum, weight, color_sum = state(fus)
    share = to.uncertain_share(res, weight if ref is None else ref['weight'])
    mism = to.weight_mismatches(res, weight)
    err = to.errors(res, tsdf_sum, color_sum, t.tsdf_vol.cpu(), None if color_sum is None else t.attribute_vols['color'].cpu())
    ratios = {k: (err[k] / (bounds[k] / 4) if bounds[k] > 0 else (0.0 if err[k] == 0 else float('inf'))) for k in err}
    print('%s: uncertain %.4f %% of the touched voxels, %d weight mismatches outside; error %s = %s x the reference\'s own '
          '(bound 4 x)' % (tag, 100 * share, mism, {k: '%.3g' % v for k, v in err.items()},
                           {k: '%.2f' % v for k, v in ratios.items()}))
    assert share <= to.UNCERTAIN_CAP
    assert mism == 0
    if ref is not None:
        keep = ~res['uncertain']
        assert torch.equal(weight[keep], torch.from_numpy(ref['weight'])[keep])
    for k in err:
        assert err[k] <= bounds[k], k
    return err


@pytest.mark.parametrize('case', CASES)
def test_goldens(cuda, case):
    """One launch over all views of a fixture against the reference's volumes and the float64 checker; case c also as 3 + 3
    (with the reference's state after three views) and one view per call."""
    g, ref, res, cols = load_case(case)
    fus = make(cuda, g)
    fus.integrate_batch(g['projections'], g['depths'], cols)
    bounds = {k: 4 * v for k, v in ref_err(case).items()}
    compare('golden %s' % case, res, fus, bounds, ref)
    # the reference's own values, outside the uncertain set: both within their bound of the float64 value
    keep = ~res['uncertain']
    d = (fus.tsdf_vol.cpu().double() - torch.from_numpy(ref['tsdf_sum']).double()).abs()[keep].max()
    print('golden %s: max |HIP - reference| of the tsdf sum %.4g' % (case, float(d)))
    assert float(d) <= 5 * ref_err(case)['tsdf']
    if int(g['mid']):
        m = int(g['mid'])
        whole = state(fus)
        two = make(cuda, g)
        two.integrate_batch(g['projections'][:m], g['depths'][:m], cols[:m])
        mid = dense(g, 'mid_')
        res3 = to.integrate(g['voxel_dim'], float(g['voxel_size']), g['origin'], float(g['voxel_size']) * float(g['trunc_ratio']),
                            g['projections'][:m], g['depths'][:m], cols[:m])
        compare('golden %s after %d views' % (case, m), res3, two, bounds, mid)
        two.integrate_batch(g['projections'][m:], g['depths'][m:], cols[m:])
        single = make(cuda, g)
        for i in range(g['depths'].shape[0]):
            single.integrate(torch.from_numpy(g['projections'][i]), torch.from_numpy(g['depths'][i]), cols[i])
        assert same(state(two), whole) and same(state(single), whole)


def _scene(n=6, size=(24, 32), seed=31):
    d, img, poses, K = fo.scene(n, size, seed=seed, yaw_step_deg=6, sigma=0.03)
    P = v3d('tsdf').projection_matrices(K, poses)
    return d, colors_of(img), P


# 29 x 37 x 23 voxels of 20 cm from (1.0, -1.5, -1.0): dimensions that are no multiple of the tile, about 96 workgroups; the slab
# y < 0 lies outside the room (y in [0, 5.01]) beyond the truncation margin, so no view touches it
DIM, VOX, ORG = (29, 37, 23), 0.2, (1.0, -1.5, -1.0)


def test_batch_equals_single_views_bit_for_bit_and_launches_repeat(cuda):
    tsdf = v3d('tsdf')
    d, cols, P = _scene()
    a = tsdf.TSDFFusion(DIM, VOX, ORG, 3, cuda)
    a.integrate_batch(P, d, cols)
    whole = state(a)
    assert int((whole[1] > 0).sum()) > 1000
    b = tsdf.TSDFFusion(DIM, VOX, ORG, 3, cuda)
    for i in range(6):
        b.integrate(P[i], d[i], cols[i])
    c = tsdf.TSDFFusion(DIM, VOX, ORG, 3, cuda)
    c.integrate_batch(P[:3], d[:3], cols[:3])
    c.integrate_batch(P[3:], d[3:], cols[3:])
    assert same(state(b), whole) and same(state(c), whole)
    dev = [t.to(cuda) for t in (P, d, cols)]
    for _ in range(10):
        again = tsdf.TSDFFusion(DIM, VOX, ORG, 3, cuda)
        again.integrate_batch(*dev)
        assert same(state(again), whole)


def test_unseen_voxels_reset_zero_maps_and_order(cuda):
    tsdf = v3d('tsdf')
    d, cols, P = _scene()
    fus = tsdf.TSDFFusion(DIM, VOX, ORG, 3, cuda)
    fus.integrate_batch(P, d, cols)
    t0, w0, c0 = state(fus)
    unseen = w0 == 0
    slab = torch.zeros(DIM, dtype=torch.bool)
    slab[:, :4] = True                                        # y < -0.7: more than the 0.6 m margin outside the room
    assert bool(unseen[slab.reshape(-1)].all()) and 0 < int(unseen.sum()) < unseen.numel()
    assert bool((t0[unseen] == -1).all()) and bool((c0[:, unseen] == 0).all())
    assert bool((w0 == w0.round()).all()) and float(w0.max()) <= 6
    # after reset() the never-seen voxels hold +1, the others the same values
    fus.reset()
    fus.integrate_batch(P, d, cols)
    t1, w1, c1 = state(fus)
    assert bool((t1[unseen] == 1).all()) and torch.equal(t1[~unseen], t0[~unseen]) and torch.equal(w1, w0) and torch.equal(c1, c0)
    # an all-zero depth map changes nothing
    fus.integrate(P[2], torch.zeros_like(d[2]), cols[2])
    assert same(state(fus), (t1, w1, c1))
    dz, colsz, Pz = (torch.cat((x[:3], x[2:3], x[3:])) for x in (d, cols, P))
    dz[3] = 0
    z = tsdf.TSDFFusion(DIM, VOX, ORG, 3, cuda)
    z.integrate_batch(Pz, dz, colsz)
    assert same(state(z), (t0, w0, c0))
    # permuting the views leaves the weights (and the integer colour sums)
    perm = [4, 0, 5, 2, 1, 3]
    p = tsdf.TSDFFusion(DIM, VOX, ORG, 3, cuda)
    p.integrate_batch(P[perm], d[perm], cols[perm])
    tp, wp, cp = state(p)
    assert torch.equal(wp, w0) and torch.equal(cp, c0)
    # the sums differ by rounding only: |sum| <= 6, so each of the at most 5 additions of either order is off by <= 2^-22
    assert float((tp - t0).abs().max()) <= 10 * 2.0 ** -22


def test_get_tsdf_and_colourless_volume(cuda):
    tsdf = v3d('tsdf')
    d, cols, P = _scene()
    fus = tsdf.TSDFFusion(DIM, VOX, ORG, 3, cuda)
    fus.integrate_batch(P, d, cols)
    t, w, c = state(fus)
    out = fus.get_tsdf()
    assert isinstance(out, tsdf.TSDF) and out.voxel_size == VOX and out.origin.shape == (1, 3)
    assert out.tsdf_vol.shape == DIM and out.attribute_vols['weight'].shape == DIM and out.attribute_vols['color'].shape == (3,) + DIM
    assert sorted(out.attribute_vols) == ['color', 'weight'] and out.attributes == {}
    seen = w > 0
    want = torch.where(seen, t / w.clamp(min=1), t)
    assert torch.equal(out.tsdf_vol.cpu().reshape(-1), want)
    assert torch.equal(out.attribute_vols['color'].cpu().reshape(3, -1), torch.where(seen[None], c / w.clamp(min=1)[None], c))
    assert torch.equal(out.attribute_vols['weight'].cpu().reshape(-1), w)
    assert same(state(fus), (t, w, c))                       # get_tsdf leaves the sums alone
    plain = tsdf.TSDFFusion(DIM, VOX, ORG, 3, cuda, color=False)
    plain.integrate_batch(P, d)
    tp, wp, cp = state(plain)
    assert cp is None and plain.color_vol is None and torch.equal(tp, t) and torch.equal(wp, w)
    po = plain.get_tsdf()
    assert sorted(po.attribute_vols) == ['weight'] and torch.equal(po.tsdf_vol.cpu().reshape(-1), want)


def test_error_codes(cuda):
    tsdf, lib_mod = v3d('tsdf'), v3d('_lib')
    lib = lib_mod.load()
    d, cols, P = _scene(2, (6, 8))
    fus = tsdf.TSDFFusion((4, 3, 2), 0.1, (0., 0., 0.), 3, cuda)
    with pytest.raises(ValueError):
        fus.integrate_batch(P, d)                            # a colour volume needs colours
    with pytest.raises(ValueError):
        fus.integrate_batch(P[:1], d, cols)
    before = state(fus)
    Pd, dd, cd = (x.to(cuda).contiguous() for x in (P, d, cols))
    import ctypes
    org = (ctypes.c_float * 3)(0., 0., 0.)
    s = lib_mod.stream_ptr(cuda)
    args = lambda **kw: [kw.get(k, v) for k, v in (('tsdf', fus.tsdf_vol.data_ptr()), ('weight', fus.weight_vol.data_ptr()),
                                                    ('color', fus.color_vol.data_ptr()), ('nx', 4), ('ny', 3), ('nz', 2), ('vs', 0.1),
                                                    ('org', org), ('tm', 0.3), ('P', Pd.data_ptr()), ('d', dd.data_ptr()),
                                                    ('img', cd.data_ptr()), ('n', 2), ('h', 6), ('w', 8), ('s', s))]
    assert lib.v3d_tsdf_integrate_f32(*args(img=None)) == -2
    assert lib.v3d_tsdf_integrate_f32(*args(color=None)) == -2
    assert lib.v3d_tsdf_integrate_f32(*args(tm=0.0)) == -2
    assert lib.v3d_tsdf_integrate_f32(*args(vs=float('nan'))) == -2
    assert lib.v3d_tsdf_integrate_f32(*args(nz=0)) == -1
    assert lib.v3d_tsdf_integrate_f32(*args(h=0)) == -1
    assert lib.v3d_tsdf_integrate_f32(*args(n=-2)) == -1
    assert lib.v3d_tsdf_integrate_f32(*args(n=0)) == 0
    with pytest.raises(lib_mod.V3DLibraryError, match='V3D_ERR_BAD_ARG'):
        lib_mod.check(lib.v3d_tsdf_integrate_f32(*args(P=None)), 'v3d_tsdf_integrate_f32')
    assert lib.v3d_tsdf_normalize_f32(fus.tsdf_vol.data_ptr(), fus.weight_vol.data_ptr(), fus.color_vol.data_ptr(), 24,
                                      fus.tsdf_vol.data_ptr(), None, s) == -2
    assert lib.v3d_tsdf_normalize_f32(fus.tsdf_vol.data_ptr(), fus.weight_vol.data_ptr(), None, 0, fus.tsdf_vol.data_ptr(), None, s) == -1
    assert same(state(fus), before)                          # none of the refused calls touched the volume
    with pytest.raises(lib_mod.V3DLibraryError):
        tsdf.TSDFFusion((4, 3, 2), 0.1, (0., 0., 0.), 3, 'cpu').integrate(P[0], d[0], cols[0])


def test_larger_volume_every_voxel(cuda):
    """16 views of 96 x 128 into 160 x 160 x 96 voxels of 8 cm (2.46 M voxels, more than the device holds resident threads):
    every voxel against the float64 checker under the two rules.  Yardstick: ref_err(a) * 16 / 6 (module docstring)."""
    tsdf = v3d('tsdf')
    d, img, poses, K = fo.scene(16, (96, 128), seed=37, yaw_step_deg=20, sigma=0.04)
    cols, P = colors_of(img), tsdf.projection_matrices(K, poses)
    dim, vox, org = (160, 160, 96), 0.08, (-3.4, -3.9, -2.4)
    res = to.integrate(dim, vox, org, vox * 3, P, d, cols)
    fus = tsdf.TSDFFusion(dim, vox, org, 3, cuda)
    fus.integrate_batch(P, d, cols)
    ra = ref_err('a')
    # colour sums are sums of byte values (exact); an averaged colour is one rounding of a quotient <= 255 whatever n is
    bounds = dict(tsdf=4 * ra['tsdf'] * 16 / 6, tsdf_avg=4 * ra['tsdf_avg'] * 16 / 6, color=0.0, color_avg=4 * ra['color_avg'])
    compare('larger volume', res, fus, bounds)
    assert int((res['weight'] > 0).sum()) > 50000


def test_fuse_preds_tsdf_from_a_written_record(cuda, tmp_path):
    tsdf, results = v3d('tsdf'), v3d('results')
    Batch = v3d('batch').Batch
    d, img, poses, K = fo.scene(5, (24, 32), seed=41, yaw_step_deg=6, sigma=0.03)
    full = torch.from_numpy(np.repeat(np.repeat(img.numpy(), 2, axis=1), 2, axis=2))          # [5, 48, 64, 3] scene images
    K_full = K.clone()
    K_full[:, :2] *= 2
    b = Batch(torch.zeros(5, 3, 48, 64), poses[:, :3, :3].contiguous(), poses[:, :3, 3].contiguous(), K_full, None, None)
    path = str(tmp_path / 'preds.npz')
    results.write_preds(path, '/data/scene0000_00', d.numpy(), b, list(range(5)), np.arange(5))
    kw = dict(vol_prcnt=.995, vol_margin=0.3, img_batch=2)
    out, fus = tsdf.fuse_preds_tsdf(path, full.numpy(), vox_res=0.1, trunc_ratio=3, return_fusion=True, **kw)
    dd, pp, KK, cc = tsdf.prepare_preds_tsdf(path, full.numpy())
    assert torch.equal(dd, d) and cc.shape == (5, 3, 24, 32)
    origin, vol_max, dim = tsdf.volume_bounds(dd.to(cuda), KK, pp, vox_res=0.1, **kw)
    assert torch.equal(fus.origin.cpu().reshape(3), origin) and list(fus.voxel_dim) == dim and min(dim) > 4
    assert out.tsdf_vol.shape == tuple(dim) and out.voxel_size == 0.1
    mine = tsdf.TSDFFusion(dim, 0.1, origin, 3, cuda)
    mine.integrate_batch(tsdf.projection_matrices(KK, pp), dd, cc)
    assert same(state(mine), state(fus)) and int((fus.weight_vol > 0).sum()) > 100
    assert torch.equal(mine.get_tsdf().tsdf_vol, out.tsdf_vol)
    assert torch.equal(mine.get_tsdf().attribute_vols['color'], out.attribute_vols['color'])
