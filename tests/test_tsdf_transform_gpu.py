"""GPU: TSDF resampling (3dvnet_amd/tsdf.py: TSDF.transform / eval_tsdf -> v3d_tsdf_resample_f32 / v3d_volume_resample_nearest,
csrc/tsdf_resample.hip) against the reference's recorded volumes (tests/golden/R_resample_*.npz), the float64 checker and the
fp32 restatement (tests/tsdf_transform_oracle.py), and its own invariants.  Every test runs the HIP path through the C ABI.

Rules: outside the uncertain set (at most 0.5 % of the output voxels; fixture a is compared on every voxel) the outside mask and
every integer / bool volume equal the reference's; the tsdf and the fp32 attribute volumes lie within 4 x the reference's own
recorded fp32 error against the checker (equality where that error is 0).  Bit identity: the device equals the fp32
restatement of include/v3d.h bit for bit -- no step is allowed to contract.

Measured on one MI355X: error / the reference's own fp32 error (bound 4): tsdf 1.00, weight 1.00, colour 1.00 on each of a, b and
c (errors a 5.96e-8 / 5.96e-7 / 3.05e-5, b 2.73e-6 / 1.89e-5 / 9.28e-4, c 9.68e-7 / 1.75e-5 / 7.35e-4: the reference's own to every
printed digit).  Uncertain share: a 0 (margin 0), b and c 0 of 1 980 voxels, the 29 x 37 x 23 -> 31 x 33 x 27 case 0.022 %
(align_corners=False) and 0.018 % (True); cap 0.5 %.  Elements that differ from the fp32 restatement: 0 in every volume of every
case (tsdf, fp32 channels, 1-, 2-, 4- and 8-byte nearest volumes).  Identity: 344 border voxels become 1, 110 of the 168 interior
voxels have an exact round trip and keep their bits.  eval_tsdf on a: l1 0.05135607227 and l1_ns 0.07553344396, 4.8e-10 and 7.0e-10
from the float64 means (tolerances 6.7e-9 and 4.3e-9).  Wall time of the module's 13 tests: 3.2 s.
"""
import numpy as np
import pytest
import torch

import tsdf_transform_oracle as oracle
from conftest import v3d
from test_tsdf_transform_oracle import CASES, FILL, FP32_KEYS, OTHER_KEYS, bound, load_case, metric_tolerance

pytestmark = pytest.mark.gpu


def make(dev, voxel_size, origin, tsdf_vol, vols):
    tsdf = v3d('tsdf')
    return tsdf.TSDF(float(voxel_size), torch.as_tensor(np.asarray(origin, dtype=np.float32)).view(1, 3).to(dev),
                     torch.as_tensor(tsdf_vol).to(dev), {k: torch.as_tensor(v).to(dev) for k, v in vols.items()})


def fixture_volume(dev, g, keys=FP32_KEYS + OTHER_KEYS):
    return make(dev, g['voxel_size'], g['src_origin'], g['in_tsdf'], {k: g['in_' + k] for k in keys})


def run(vol, g):
    out = vol.transform(torch.from_numpy(g['matrix']), [int(v) for v in g['voxel_dim']], g['dst_origin'].tolist(),
                        align_corners=bool(g['align_corners']))
    torch.cuda.synchronize()
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.itemsize]) if a.dtype.kind == 'f' else a


def assert_equals_restatement(tag, out, p32, tsdf_vol, vols):
    """Bit identity of everything a transform returned with the fp32 restatement."""
    n_diff = {'tsdf': int((bits(out.tsdf_vol.cpu().numpy().reshape(-1)) != bits(oracle.tsdf(p32, tsdf_vol))).sum())}
    for k, v in vols.items():
        v = np.asarray(v)
        if v.dtype == np.float32:
            want = oracle.trilinear(p32, v)
        else:
            want = oracle.nearest(p32, v)
            if k in FILL:
                want = oracle.fill_outside(p32, want, FILL[k])
        got = out.attribute_vols[k].cpu().numpy()
        assert got.dtype == v.dtype and got.shape == v.shape[:-3] + tuple(out.tsdf_vol.shape), k
        n_diff[k] = int((bits(got.reshape(want.shape)) != bits(want)).sum())
    print('%s: elements that differ from the fp32 restatement: %s' % (tag, n_diff))
    assert not any(n_diff.values())


@pytest.mark.parametrize('case', CASES)
def test_goldens(cuda, case):
    g, p64, p32 = load_case(case)
    out = run(fixture_volume(cuda, g), g)
    assert tuple(out.origin.shape) == (1, 3) and out.origin.dtype == torch.float32 and out.origin.device.type == 'cuda'
    assert np.array_equal(out.origin.cpu().numpy().reshape(-1), g['dst_origin'])
    probe = run(make(cuda, g['voxel_size'], g['src_origin'], g['in_tsdf'], {'mask_outside': np.zeros_like(g['in_mask_outside'])}), g)
    outside = probe.attribute_vols['mask_outside'].cpu().numpy().reshape(-1)
    keep = ~p64['uncertain']
    share = oracle.uncertain_share(p64)
    print('golden %s: uncertain %.4f %% of the output voxels, outside %.1f %%' % (case, 100 * share, 100 * outside.mean()))
    assert share <= oracle.UNCERTAIN_CAP
    if case == 'a':
        assert keep.all()                                    # verdicts and integer volumes equal on every voxel
    assert np.array_equal(outside[keep], g['ref_outside'].reshape(-1)[keep])
    for k in OTHER_KEYS:
        got = out.attribute_vols[k].cpu().numpy()
        assert got.dtype == g['out_' + k].dtype and got.shape == g['out_' + k].shape
        assert np.array_equal(got.reshape(-1)[keep], g['out_' + k].reshape(-1)[keep]), k
    want = {'tsdf': oracle.tsdf(p64, g['in_tsdf'])}
    got = {'tsdf': out.tsdf_vol.cpu().numpy()}
    for k in FP32_KEYS:
        want[k], got[k] = oracle.trilinear(p64, g['in_' + k]), out.attribute_vols[k].cpu().numpy()
        assert got[k].shape == g['out_' + k].shape and got[k].dtype == np.float32
    for k in want:
        err, ref = oracle.max_error(p64, got[k], want[k]), float(g['ref_err_' + k])
        print('golden %s: %s error %.4g = %s x the reference\'s own %.4g (bound 4 x)'
              % (case, k, err, ('%.2f' % (err / ref)) if ref > 0 else ('0' if err == 0 else 'inf'), ref))
        assert err <= bound(ref), k
    assert_equals_restatement('golden %s' % case, out, p32, g['in_tsdf'], {k: g['in_' + k] for k in FP32_KEYS + OTHER_KEYS})


def seeded(dim, seed):
    rng = np.random.RandomState(seed)
    nx, ny, nz = dim
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing='ij')
    d = (z - nz / 2.0) + 0.3 * (x - nx / 2.0) - 0.25 * (y - ny / 2.0) + np.sin(0.7 * x + 0.4 * y)
    tsdf_vol = np.clip(d / 3.0 + 0.02 * rng.randn(nx, ny, nz), -1, 1).astype(np.float32)
    vols = dict(weight=rng.randint(0, 6, size=dim).astype(np.float32), color=(rng.rand(3, *dim) * 255).astype(np.float32),
                instance=rng.randint(-1, 7, size=dim).astype(np.int64), semseg=rng.randint(-1, 12, size=dim).astype(np.int32),
                mask_outside=rng.rand(*dim) > 0.6, label16=rng.randint(-5, 300, size=(2,) + tuple(dim)).astype(np.int16),
                fine=rng.randn(*dim).astype(np.float64))
    return tsdf_vol, vols


def rotation(dim, voxel_size, origin, shift):
    a, b = np.radians(17), np.radians(-8)
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    R = Rz @ Ry
    c = np.asarray(origin, dtype=np.float64) + 0.5 * voxel_size * (np.asarray(dim) - 1)
    return np.concatenate((R, (c - R @ c + np.asarray(shift))[:, None]), axis=1).astype(np.float32)


# 29 x 37 x 23 -> 31 x 33 x 27 = 27 621 voxels: no multiple of the 256-thread tile, 108 workgroups (13 or 14 per XCD)
SRC, DST, VOX, SRC_ORG, DST_ORG = (29, 37, 23), (31, 33, 27), 0.04, (0.3, -1.1, 0.7), (0.24, -1.02, 0.62)


@pytest.mark.parametrize('align', [False, True])
def test_bit_identity_over_many_workgroups(cuda, align):
    """Every element size of the nearest kernel (1, 2, 4, 8 bytes, a two-channel volume among them), float64 copied in its own
    type, and the fused fp32 launch, against the fp32 restatement."""
    tsdf_vol, vols = seeded(SRC, 7)
    M = rotation(SRC, VOX, SRC_ORG, (0.013, -0.009, 0.017))
    out = make(cuda, VOX, SRC_ORG, tsdf_vol, vols).transform(M, DST, DST_ORG, align_corners=align)
    torch.cuda.synchronize()
    p32 = oracle.plan(SRC, VOX, SRC_ORG, M, align, DST, DST_ORG, np.float32)
    p64 = oracle.plan(SRC, VOX, SRC_ORG, M, align, DST, DST_ORG, np.float64)
    interp = (~p32['outside']) & (np.abs(oracle.nearest(p32, tsdf_vol)[0]) < 1)
    print('align_corners=%s: outside %.1f %%, interpolated %.1f %%, uncertain %.3f %%'
          % (align, 100 * p32['outside'].mean(), 100 * interp.mean(), 100 * oracle.uncertain_share(p64)))
    assert 0.1 < p32['outside'].mean() < 0.9 and interp.mean() > 0.1
    assert oracle.uncertain_share(p64) <= oracle.UNCERTAIN_CAP
    assert_equals_restatement('29x37x23 -> 31x33x27 align_corners=%s' % align, out, p32, tsdf_vol, vols)


def test_identity_keeps_the_interior_and_marks_the_border(cuda):
    """Identity transform onto the same grid, align_corners=True, power-of-two sizes, voxel size and origin: every step up to g is
    exact.  The border layer has |g| = 1 on some axis, which the reference's rule turns into 1 (asserted as that rule); every
    interior voxel whose round trip returns its own integer coordinate keeps its value bit for bit."""
    dim, vs, org = (16, 8, 4), 0.0625, (0.5, -0.25, 1.0)
    tsdf_vol, vols = seeded(dim, 11)
    vols = {k: vols[k] for k in ('color', 'instance')}
    src = make(cuda, vs, org, tsdf_vol, vols)
    out = src.transform(align_corners=True)
    torch.cuda.synchronize()
    p32 = oracle.plan(dim, vs, org, np.eye(4)[:3], True, dim, org, np.float32)
    idx = np.stack(np.meshgrid(*[np.arange(n) for n in dim], indexing='ij')).reshape(3, -1)
    border = ((idx == 0) | (idx == np.asarray(dim)[:, None] - 1)).any(0)
    assert np.array_equal(p32['outside'], border)            # the reference's |g| >= 1 rule, nothing else
    got = out.tsdf_vol.cpu().numpy().reshape(-1)
    assert (got[border] == 1).all()
    exact = (~border) & (p32['u'] == idx).all(0)
    print('identity: %d border voxels, %d of %d interior voxels with an exact round trip' % (border.sum(), exact.sum(), (~border).sum()))
    assert exact.sum() * 2 > (~border).sum()
    assert np.array_equal(bits(got[exact]), bits(tsdf_vol.reshape(-1)[exact]))
    col = out.attribute_vols['color'].cpu().numpy().reshape(3, -1)
    assert np.array_equal(bits(col[:, exact]), bits(vols['color'].reshape(3, -1)[:, exact]))
    # nearest volumes keep every voxel, the border included: nothing but semseg / mask_outside is overwritten
    assert np.array_equal(out.attribute_vols['instance'].cpu().numpy(), vols['instance'])
    assert out.attributes is src.attributes


def test_fused_equals_separate_repeats_and_source_unchanged(cuda):
    g, _, _ = load_case('b')
    tsdf_mod = v3d('tsdf')
    both = make(cuda, g['voxel_size'], g['src_origin'], g['in_tsdf'], {'color': g['in_color'], 'again': g['in_color'].copy()})
    before = (both.tsdf_vol.clone(), both.attribute_vols['color'].clone())
    first = run(both, g)
    alone = run(make(cuda, g['voxel_size'], g['src_origin'], g['in_tsdf'], {}), g)
    assert isinstance(first, tsdf_mod.TSDF) and alone.attribute_vols == {}
    # 'color' rode with the tsdf in one launch, 'again' had a launch of its own, `alone` is the tsdf without channels
    assert torch.equal(first.tsdf_vol, alone.tsdf_vol)
    assert torch.equal(first.attribute_vols['color'], first.attribute_vols['again'])
    for _ in range(10):
        again = run(both, g)
        assert torch.equal(again.tsdf_vol, first.tsdf_vol)
        assert all(torch.equal(again.attribute_vols[k], first.attribute_vols[k]) for k in first.attribute_vols)
    assert torch.equal(both.tsdf_vol, before[0]) and torch.equal(both.attribute_vols['color'], before[1])
    assert first.tsdf_vol.data_ptr() != both.tsdf_vol.data_ptr()


@pytest.mark.parametrize('src,dst', [((5, 4, 3), (6, 1, 4)), ((5, 4, 3), (1, 1, 1)), ((2, 2, 2), (3, 4, 3)), ((2, 7, 2), (4, 1, 5))])
def test_sizes_of_one_and_two(cuda, src, dst):
    """An output size of 1 (kept as a dimension: no squeeze) and source sizes of 2 (the smallest the normalisation allows)."""
    tsdf_vol, vols = seeded(src, 5)
    vols = {k: vols[k] for k in ('color', 'semseg', 'mask_outside')}
    org, dorg = (0., 0., 0.), (0.01, -0.005, 0.002)
    M = rotation(src, 0.04, org, (0.004, 0.002, -0.003))
    for align in (False, True):
        out = make(cuda, 0.04, org, tsdf_vol, vols).transform(M, dst, dorg, align_corners=align)
        torch.cuda.synchronize()
        assert tuple(out.tsdf_vol.shape) == dst and tuple(out.attribute_vols['color'].shape) == (3,) + dst
        p32 = oracle.plan(src, 0.04, org, M, align, dst, dorg, np.float32)
        assert_equals_restatement('%s -> %s align_corners=%s' % (src, dst, align), out, p32, tsdf_vol, vols)


def test_matrix_forms_agree(cuda):
    g, _, _ = load_case('c')
    vol = fixture_volume(cuda, g, ('color', 'semseg'))
    host = run(vol, g)
    M4 = torch.cat((torch.from_numpy(g['matrix']), torch.tensor([[0., 0., 0., 1.]])), dim=0).to(cuda)
    dev = vol.transform(M4, tuple(int(v) for v in g['voxel_dim']), torch.from_numpy(g['dst_origin']).to(cuda), align_corners=True)
    assert torch.equal(dev.tsdf_vol, host.tsdf_vol) and torch.equal(dev.origin, host.origin)
    assert all(torch.equal(dev.attribute_vols[k], host.attribute_vols[k]) for k in host.attribute_vols)
    # None = identity, the input's grid and origin
    same = vol.transform(align_corners=True)
    eye = vol.transform(torch.eye(4), list(vol.tsdf_vol.shape), vol.origin, align_corners=True)
    assert torch.equal(same.tsdf_vol, eye.tsdf_vol) and torch.equal(same.origin, vol.origin)


def test_eval_tsdf(cuda, tmp_path):
    """Fixture a: the prediction on its own grid against the seeded target on the shifted grid, as objects and as npz files."""
    tsdf = v3d('tsdf')
    g, _, _ = load_case('a')
    pred = fixture_volume(cuda, g, ('color',))
    trgt = tsdf.TSDF(float(g['voxel_size']), torch.from_numpy(g['dst_origin'].copy()).view(1, 3), torch.from_numpy(g['trgt_tsdf'].copy()),
                     {}, {'weight': torch.from_numpy(g['trgt_weight'].copy())})
    trgt.save(str(tmp_path / 'trgt.npz'))
    pred.save(str(tmp_path / 'pred.npz'))
    got = tsdf.eval_tsdf(pred, trgt.to(cuda))
    from_files = tsdf.eval_tsdf(str(tmp_path / 'pred.npz'), str(tmp_path / 'trgt.npz'))
    assert sorted(got) == ['l1', 'l1_ns'] and got == from_files
    for key in ('l1', 'l1_ns'):
        tol = metric_tolerance(g, key)
        print('eval_tsdf %s: %.10g, reference %.10g, float64 %.10g: distance %.3g, tolerance %.3g'
              % (key, got[key], float(g['ref_' + key]), float(g['f64_' + key]), abs(got[key] - float(g['f64_' + key])), tol))
        assert abs(got[key] - float(g['f64_' + key])) <= tol
    off = tsdf.TSDF(trgt.voxel_size, trgt.origin + 0.02, trgt.tsdf_vol, {}, trgt.attributes)
    with pytest.raises(ValueError, match='whole number'):
        tsdf.eval_tsdf(pred, off)
