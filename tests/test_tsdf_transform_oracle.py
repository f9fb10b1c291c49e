"""CPU: the checkers of TSDF resampling (tests/tsdf_transform_oracle.py) against the reference-written fixtures
(tests/golden/R_resample_*.npz, written by tests/golden/make_golden_tsdf_transform.py), the host-side validation of the two C
entry points, and the behaviour of ``TSDF.transform`` / ``eval_tsdf`` without a device.

Recorded in the fixtures (the reference's own fp32 error against the float64 checker outside the uncertain set; the yardstick of
tests/test_tsdf_transform_gpu.py): a (integer shift, margin 0) tsdf 5.96e-8, weight 5.96e-7, colour 3.05e-5; b (rotation,
align_corners=False) 2.73e-6 / 1.89e-5 / 9.28e-4; c (rotation, align_corners=True) 9.68e-7 / 1.75e-5 / 7.35e-4.  Uncertain
share at a margin of 1e-4 voxels: 0 of the 1 980 output voxels of b and c (cap 0.5 %); a is compared on every voxel.  Outside
the source volume: 68 % (a), 56 % (b, c) of the voxels; interpolated: 29 % / 27 % / 30 %.  Reference l1 / l1_ns on a:
0.0513560735 / 0.0755334422 against the float64 means 0.0513560718 / 0.0755334433.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import tsdf_transform_oracle as oracle
from conftest import ROOT, v3d

CASES = ('a', 'b', 'c')
FP32_KEYS, OTHER_KEYS = ('weight', 'color'), ('instance', 'semseg', 'mask_outside')
FILL = {'semseg': -1, 'mask_outside': True}


@functools.lru_cache(maxsize=None)
def load_case(case):
    """-> (fixture dict, float64 plan, fp32 plan); computed once and shared (treat as read-only)."""
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'R_resample_%s.npz' % case)) as f:
        g = {k: f[k] for k in f.files}
    args = (g['in_tsdf'].shape, float(g['voxel_size']), g['src_origin'], g['matrix'], bool(g['align_corners']),
            [int(v) for v in g['voxel_dim']], g['dst_origin'])
    return g, oracle.plan(*args, np.float64, float(g['margin'])), oracle.plan(*args, np.float32)


def bound(err):
    """The project's rule for fp32 routes: 4 x the reference's own fp32 error (same products, possibly another contraction)."""
    return 4 * float(err)


def tsdf_of(g):
    tsdf = v3d('tsdf')
    vols = {k: torch.from_numpy(g['in_' + k].copy()) for k in FP32_KEYS + OTHER_KEYS}
    return tsdf.TSDF(float(g['voxel_size']), torch.from_numpy(g['src_origin'].copy()).view(1, 3), torch.from_numpy(g['in_tsdf'].copy()),
                     vols)


@pytest.mark.parametrize('case', CASES)
def test_checker_reproduces_the_recorded_yardsticks(case):
    g, p64, _ = load_case(case)
    keep = ~p64['uncertain']
    share = oracle.uncertain_share(p64)
    assert share <= oracle.UNCERTAIN_CAP and share == float(g['uncertain_share'])
    if case == 'a':
        assert not p64['uncertain'].any()                    # margin 0: every voxel is compared
    assert np.array_equal(g['ref_outside'].reshape(-1)[keep], p64['outside'][keep])
    assert 0.2 < p64['outside'].mean() < 0.8                 # both verdicts are well represented
    assert oracle.max_error(p64, g['out_tsdf'], oracle.tsdf(p64, g['in_tsdf'])) == float(g['ref_err_tsdf'])
    for k in FP32_KEYS:
        assert oracle.max_error(p64, g['out_' + k], oracle.trilinear(p64, g['in_' + k])) == float(g['ref_err_' + k])
    for k in OTHER_KEYS:
        want = oracle.nearest(p64, g['in_' + k])
        if k in FILL:
            want = oracle.fill_outside(p64, want, FILL[k])
        assert want.dtype == g['out_' + k].dtype
        assert np.array_equal(g['out_' + k].reshape(-1)[keep], want[0][keep])
    assert (g['in_instance'] == -1).any() and (g['in_semseg'] == -1).any()


@pytest.mark.parametrize('case', CASES)
def test_fp32_restatement_against_reference_and_checker(case):
    """The pinned fp32 arithmetic: verdicts and integer volumes equal the reference's outside the uncertain set (on a: on every
    voxel); values within 4 x the reference's own error of the float64 checker."""
    g, p64, p32 = load_case(case)
    keep = ~p64['uncertain']
    assert np.array_equal(p32['outside'][keep], g['ref_outside'].reshape(-1)[keep])
    for k in OTHER_KEYS:
        got = oracle.nearest(p32, g['in_' + k])
        if k in FILL:
            got = oracle.fill_outside(p32, got, FILL[k])
        assert np.array_equal(got[0][keep], g['out_' + k].reshape(-1)[keep])
    err = {'tsdf': oracle.max_error(p64, oracle.tsdf(p32, g['in_tsdf']), oracle.tsdf(p64, g['in_tsdf']))}
    for k in FP32_KEYS:
        err[k] = oracle.max_error(p64, oracle.trilinear(p32, g['in_' + k]), oracle.trilinear(p64, g['in_' + k]))
    print('restatement %s: error %s; the reference\'s own %s' % (case, err, {k: float(g['ref_err_' + k]) for k in err}))
    for k, e in err.items():
        assert e <= bound(g['ref_err_' + k]), k


def test_l1_metrics_on_the_reference_aligned_volume():
    """``l1`` / ``l1_ns`` are stock torch ops and run where the volumes live: on the reference's aligned volume of fixture a
    they give the reference's scalars within 4 x the reference's own distance from the float64 means."""
    tsdf = v3d('tsdf')
    g, _, _ = load_case('a')
    origin = torch.from_numpy(g['dst_origin'].copy()).view(1, 3)
    pred = tsdf.TSDF(float(g['voxel_size']), origin, torch.from_numpy(g['out_tsdf'].copy()))
    trgt = tsdf.TSDF(float(g['voxel_size']), origin, torch.from_numpy(g['trgt_tsdf'].copy()), {},
                     {'weight': torch.from_numpy(g['trgt_weight'].copy())})
    for fn, key in ((tsdf.l1, 'l1'), (tsdf.l1_ns, 'l1_ns')):
        tol = metric_tolerance(g, key)
        got = fn(pred, trgt)
        print('%s: %.10g, reference %.10g, float64 %.10g, tolerance %.3g' % (key, got, float(g['ref_' + key]), float(g['f64_' + key]), tol))
        assert abs(got - float(g['f64_' + key])) <= tol
    empty = tsdf.TSDF(float(g['voxel_size']), origin, torch.from_numpy(g['trgt_tsdf'].copy()), {},
                      {'weight': torch.zeros(g['trgt_weight'].shape)})
    assert np.isnan(tsdf.l1(pred, empty)) and np.isnan(tsdf.l1_ns(pred, empty))
    with pytest.raises(ValueError, match='aligned'):
        tsdf.l1(tsdf.TSDF(float(g['voxel_size']), origin, torch.zeros(3, 3, 3)), trgt)


def metric_tolerance(g, key):
    """4 x |reference scalar - float64 value of the same masked mean|; one fp32 ulp of the value where that is 0."""
    d = abs(float(g['ref_' + key]) - float(g['f64_' + key]))
    return 4 * d if d > 0 else float(np.spacing(np.float32(g['f64_' + key])))


def _grid_args(sx=4, sy=4, sz=4, vs=0.1, src_origin=(0, 0, 0), matrix=None, align=1, nx=3, ny=3, nz=3, dst_origin=(0, 0, 0)):
    m = np.eye(4, dtype=np.float32)[:3].reshape(-1) if matrix is None else np.asarray(matrix, dtype=np.float32).reshape(-1)
    return [sx, sy, sz, vs, (ctypes.c_float * 3)(*src_origin), (ctypes.c_float * 12)(*m.tolist()), align, nx, ny, nz,
            (ctypes.c_float * 3)(*dst_origin)]


def test_host_validation_returns_before_any_launch():
    """Every stated error of the two entry points comes back with the project's code and a message; the pointers are host buffers
    and this machine may have no device at all, so a code other than BAD_ARG / BAD_SHAPE would mean a launch was attempted."""
    lib_mod = v3d('_lib')
    lib = lib_mod.load()
    assert lib.v3d_version() == 9
    BAD_SHAPE, BAD_ARG = -1, -2
    src = np.zeros(4 * 4 * 4 * 3, dtype=np.float32)
    dst = np.zeros(4 * 4 * 4 * 3, dtype=np.float32)
    s, d = src.ctypes.data, dst.ctypes.data
    nan, inf = float('nan'), float('inf')
    bad_m = np.eye(4, dtype=np.float32)[:3].copy()
    bad_m[1, 2] = np.nan
    grids = [
        (dict(sx=1), BAD_SHAPE, b'at least 2'), (dict(sy=1), BAD_SHAPE, b'at least 2'), (dict(sz=0), BAD_SHAPE, b'at least 2'),
        (dict(nx=0), BAD_SHAPE, b'output volume'), (dict(ny=-1), BAD_SHAPE, b'output volume'), (dict(nz=0), BAD_SHAPE, b'output volume'),
        (dict(sx=2048, sy=2048, sz=512), BAD_SHAPE, b'2^31'), (dict(nx=2048, ny=2048, nz=512), BAD_SHAPE, b'2^31'),
        (dict(vs=0.0), BAD_ARG, b'voxel_size'), (dict(vs=-1.0), BAD_ARG, b'voxel_size'), (dict(vs=nan), BAD_ARG, b'voxel_size'),
        (dict(vs=inf), BAD_ARG, b'voxel_size'), (dict(vs=1e-60), BAD_ARG, b'voxel_size'),
        (dict(src_origin=(0, nan, 0)), BAD_ARG, b'origin'), (dict(dst_origin=(inf, 0, 0)), BAD_ARG, b'origin'),
        (dict(matrix=bad_m), BAD_ARG, b'transform'),
    ]

    def f32(tsdf_src, attr_src, channels, grid, tsdf_dst, attr_dst):
        return lib.v3d_tsdf_resample_f32(tsdf_src, attr_src, channels, *grid, tsdf_dst, attr_dst, None)

    def near(src_, elem, channels, grid, fill_on, fill, dst_):
        return lib.v3d_volume_resample_nearest(src_, elem, channels, *grid, fill_on, fill, dst_, None)

    def expect(rc, code, word):
        msg = lib.v3d_last_error()
        assert rc == code and word in msg, (rc, code, word, msg)

    for kw, code, word in grids:
        expect(f32(s, None, 0, _grid_args(**kw), d, None), code, word)
        expect(near(s, 8, 1, _grid_args(**kw), 0, None, d), code, word)
    ok = _grid_args()
    # null pointers and halves of pairs
    expect(f32(None, None, 0, ok, None, None), BAD_ARG, b'null')
    expect(f32(s, None, 0, ok, None, None), BAD_ARG, b'null')
    expect(f32(None, None, 0, ok, d, None), BAD_ARG, b'null')
    expect(f32(None, s, 3, ok, None, None), BAD_ARG, b'null')
    expect(f32(None, None, 3, ok, None, d), BAD_ARG, b'null')
    expect(f32(None, s, 0, ok, None, d), BAD_ARG, b'null')
    expect(f32(s, None, -1, ok, d, None), BAD_SHAPE, b'channels')
    for k in (4, 5, 10):                                     # the three host arrays: source origin, matrix, output origin
        bad = list(ok)
        bad[k] = None
        expect(f32(s, None, 0, bad, d, None), BAD_ARG, b'null')
        expect(near(s, 4, 1, bad, 0, None, d), BAD_ARG, b'null')
    expect(near(None, 4, 1, ok, 0, None, d), BAD_ARG, b'null')
    expect(near(s, 4, 1, ok, 0, None, None), BAD_ARG, b'null')
    expect(near(s, 4, 1, ok, 1, None, d), BAD_ARG, b'null')
    expect(near(s, 3, 1, ok, 0, None, d), BAD_ARG, b'elem_bytes')
    expect(near(s, 16, 1, ok, 0, None, d), BAD_ARG, b'elem_bytes')
    expect(near(s, 4, 1, ok, 2, b'\0' * 8, d), BAD_ARG, b'fill_outside')
    expect(near(s, 4, 0, ok, 0, None, d), BAD_SHAPE, b'channels')
    # overlap: the same buffer, a destination that starts inside the source, a source that starts inside the destination
    expect(f32(s, None, 0, ok, s, None), BAD_ARG, b'overlap')
    expect(f32(s, None, 0, ok, s + 4 * 63, None), BAD_ARG, b'overlap')
    expect(f32(s + 4 * 26, None, 0, ok, s, None), BAD_ARG, b'overlap')
    expect(f32(d, s, 3, ok, d + 4 * 64, s + 4 * 100), BAD_ARG, b'overlap')
    expect(f32(s, d, 1, ok, d + 4 * 64, d + 4 * 90), BAD_ARG, b'overlap')       # the two destinations overlap
    expect(near(s, 8, 1, ok, 0, None, s + 8), BAD_ARG, b'overlap')
    with pytest.raises(lib_mod.V3DLibraryError, match='overlap'):
        lib_mod.check(near(s, 1, 1, ok, 0, None, s + 63), 'v3d_volume_resample_nearest')


def test_no_cpu_fallback_and_argument_errors():
    tsdf, lib_mod = v3d('tsdf'), v3d('_lib')
    g, _, _ = load_case('a')
    vol = tsdf_of(g)
    with pytest.raises(lib_mod.V3DLibraryError, match='no CPU fallback'):
        vol.transform()
    with pytest.raises(lib_mod.V3DLibraryError):
        tsdf.eval_tsdf(vol, vol)
    with pytest.raises(ValueError, match=r'\[3, 4\] or \[4, 4\]'):
        vol.transform(torch.eye(3))
    with pytest.raises(ValueError, match='not finite'):
        vol.transform(torch.full((3, 4), float('nan')))
    with pytest.raises(ValueError, match='voxel_dim'):
        vol.transform(voxel_dim=[4, 0, 4])
    with pytest.raises(ValueError, match='voxel_dim'):
        vol.transform(voxel_dim=[4, 4])
    with pytest.raises(ValueError, match='origin'):
        vol.transform(origin=[0., float('inf'), 0.])
    with pytest.raises(ValueError, match='origin'):
        vol.transform(origin=[0., 1.])
    with pytest.raises(ValueError, match='at least 2'):
        tsdf.TSDF(0.04, torch.zeros(1, 3), torch.zeros(5, 1, 5)).transform()
    with pytest.raises(ValueError, match="'color'"):
        tsdf.TSDF(0.04, torch.zeros(1, 3), torch.zeros(5, 4, 5), {'color': torch.zeros(3, 5, 4, 4)}).transform()
    with pytest.raises(ValueError, match='fp32'):
        tsdf.TSDF(0.04, torch.zeros(1, 3), torch.zeros(5, 4, 5, dtype=torch.float64)).transform()
    # eval_tsdf: a shift of half a voxel between the origins is refused before anything runs
    a = tsdf.TSDF(0.04, torch.zeros(1, 3), torch.zeros(4, 4, 4))
    b = tsdf.TSDF(0.04, torch.tensor([[0.02, 0., 0.]]), torch.zeros(4, 4, 4), {}, {'weight': torch.ones(4, 4, 4)})
    with pytest.raises(ValueError, match='whole number'):
        tsdf.eval_tsdf(a, b)
