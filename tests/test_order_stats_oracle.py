"""CPU: the NumPy checker of the device's volume bounds (tests/order_stats_oracle.py) against the bounds the reference's own
functions wrote into tests/golden/T_tsdf_a.npz (6 views of 48 x 64, two batches of 4 + 2) and against a brute-force sort; the
host side of the new entry points (the no-fallback rule, the header, the host-side error codes).

The checker's bounds on that fixture: largest difference to the reference's 4.8e-7 (bound 1e-5, the one tests/test_tsdf_oracle.py
uses for the host path on the same fixture), dims equal; the fractional parts of (max - origin) / vox_res are .48, .54, .89, so
no dim sits near a flip.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import order_stats_oracle as oo
from conftest import ROOT, v3d

QS = (0.0, 1 - .995, .5, .995, 1.0)
_cache = {}


def fixture_a():
    """-> (fixture dict, keyword arguments of the bounds); loaded once, not modified."""
    if 'a' not in _cache:
        with np.load(os.path.join(ROOT, 'tests', 'golden', 'T_tsdf_a.npz')) as f:
            g = {k: f[k] for k in f.files}
        kw = dict(vol_prcnt=float(g['bounds_vol_prcnt']), vol_margin=float(g['bounds_vol_margin']),
                  vox_res=float(g['bounds_vox_res']), img_batch=int(g['bounds_img_batch']))
        _cache['a'] = (g, kw)
    return _cache['a']


def test_checker_reproduces_the_reference_bounds():
    g, kw = fixture_a()
    origin, vol_max, dim = oo.volume_bounds(g['depths'], g['K'], g['poses'], **kw)
    diff = max(float(np.abs(origin.numpy() - g['bounds_origin']).max()), float(np.abs(vol_max.numpy() - g['bounds_max']).max()))
    frac = ((vol_max - origin) / kw['vox_res']).numpy() % 1
    print('checker against the reference: largest difference %.3g, dims %s, fractional parts %s' % (diff, dim, frac))
    assert origin.dtype == torch.float32 and vol_max.dtype == torch.float32
    np.testing.assert_allclose(origin.numpy(), g['bounds_origin'], rtol=0, atol=1e-5)
    np.testing.assert_allclose(vol_max.numpy(), g['bounds_max'], rtol=0, atol=1e-5)
    assert dim == g['bounds_dim'].tolist()
    # two batches: the running minimum / maximum of the single-batch bounds
    one = [oo.volume_bounds(g['depths'][s], g['K'][s], g['poses'][s], **kw) for s in (slice(0, 4), slice(4, 6))]
    assert torch.equal(origin, torch.minimum(one[0][0], one[1][0])) and torch.equal(vol_max, torch.maximum(one[0][1], one[1][1]))
    d = g['depths'].copy()
    d[4:] = 0
    o2, m2, _ = oo.volume_bounds(d, g['K'], g['poses'], **kw)
    assert torch.equal(o2, one[0][0]) and torch.equal(m2, one[0][1])
    with pytest.raises(ValueError):
        oo.volume_bounds(np.zeros_like(d), g['K'], g['poses'], **kw)


def brute(pts, qs):
    rows = [tuple(float(v) for v in r) for r in pts if not any(v != v for v in r)]
    n = len(rows)
    out = np.full((len(qs), 3, 2), np.nan, dtype=np.float32)
    for a in range(3):
        col = sorted(r[a] for r in rows)
        for j, q in enumerate(qs):
            if n:
                lo = int(min(max(np.floor(q * (n - 1)), 0), n - 1))
                out[j, a] = (col[lo], col[min(lo + 1, n - 1)])
    return n, out


@pytest.mark.parametrize('n', [1, 2, 7, 200, 201])
def test_checker_statistics_match_a_brute_force_sort(n):
    rng = np.random.default_rng(100 + n)
    pts = rng.integers(-4, 5, (n, 3)).astype(np.float32) / 2            # many duplicates
    if n > 2:
        pts[rng.integers(0, n, 3), rng.integers(0, 3, 3)] = np.inf
        pts[rng.integers(0, n, 3), rng.integers(0, 3, 3)] = -np.inf
        pts[rng.integers(0, n, 2), rng.integers(0, 3, 2)] = np.nan
    count, stats = oo.order_stats(pts, QS)
    want_n, want = brute(pts, QS)
    assert count == want_n and oo.same_bits(stats, want)
    for j, q in enumerate(QS):                                          # the pinned finish lies between its two statistics
        for a in range(3):
            v = oo.finish(count, stats[j, a], q)
            if np.isfinite(stats[j, a]).all():
                assert stats[j, a, 0] <= v <= stats[j, a, 1]
    assert oo.order_stats(np.full((5, 3), np.nan, np.float32), QS)[0] == 0


def test_backprojection_of_the_checker_is_the_plain_formula():
    """On a matrix with a general last row, against float64: every point within a few fp32 roundings of its scale."""
    rng = np.random.default_rng(5)
    Pi = (np.eye(4) + 0.1 * rng.standard_normal((2, 4, 4))).astype(np.float32)
    d = (1 + rng.random((2, 3, 5))).astype(np.float32)
    d[0, 1, 2] = 0
    got = oo.backproject(d, Pi).reshape(2, 3, 5, 3)
    assert np.isnan(got[0, 1, 2]).all()
    for i, y, x in ((0, 0, 0), (1, 2, 4), (0, 2, 3)):
        X = Pi[i].astype(np.float64) @ np.array([x, y, 1, 1 / np.float64(d[i, y, x])])
        np.testing.assert_allclose(got[i, y, x], X[:3] / X[3], rtol=1e-5)


def test_no_cpu_fallback():
    tsdf, lib_mod = v3d('tsdf'), v3d('_lib')
    g, kw = fixture_a()
    with pytest.raises(lib_mod.V3DLibraryError):
        tsdf.volume_bounds_device(torch.from_numpy(g['depths']), g['K'], g['poses'], **kw)
    with pytest.raises(lib_mod.V3DLibraryError):
        tsdf.cloud_order_stats(torch.zeros(4, 3), (0.5,))
    with pytest.raises(lib_mod.V3DLibraryError):
        tsdf.backproject_order_stats(torch.ones(1, 2, 2), torch.eye(4)[None], (0.5,))
    with pytest.raises(ValueError):
        tsdf.cloud_order_stats(torch.zeros(4, 3), (0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError):
        tsdf.cloud_order_stats(torch.zeros(4, 3), (1.5,))
    with pytest.raises(ValueError):
        tsdf._bounds_fn('somewhere', 'trim_mesh')
    # the pinned finish of the package equals the checker's
    for count, pair, q in ((10, (1.0, 2.0), .995), (3, (-1.5, -1.5), .5), (1 << 25, (0.25, 0.75), 1 - .995)):
        pair = np.array(pair, dtype=np.float32)
        assert tsdf.quantile_from_order_stats(count, pair, q) == oo.finish(count, pair, q)


def test_header_declares_the_three_symbols():
    src = open(os.path.join(ROOT, 'include', 'v3d.h')).read()
    for name in ('v3d_order_stats_workspace_bytes', 'v3d_backproject_order_stats_f32', 'v3d_cloud_order_stats_f32'):
        assert name + '(' in src, name
        assert name in v3d('_lib').SIGNATURES


def test_host_validation_of_the_c_abi():
    """Errors that return before anything touches the device."""
    lib = v3d('_lib').load()
    one = ctypes.c_void_p(256)                            # never dereferenced: every call below fails first
    q2 = (ctypes.c_double * 2)(0.005, 0.995)
    size = lib.v3d_order_stats_workspace_bytes
    assert size(0) == 0 and size(5) == 0 and 0 < size(1) < size(2) < size(4)
    # header + 3 top-digit histograms + per target one 2048-bin and one 1024-bin histogram
    assert size(2) == 1024 + 4 * (3 * 2048 + 12 * 2048 + 12 * 1024)
    cloud, fused = lib.v3d_cloud_order_stats_f32, lib.v3d_backproject_order_stats_f32
    big = size(4)
    assert cloud(None, 8, q2, 2, one, one, one, big, None) == -2 and b'null' in lib.v3d_last_error()
    assert cloud(one, 8, q2, 2, None, one, one, big, None) == -2
    assert cloud(one, 8, q2, 2, one, None, one, big, None) == -2
    assert cloud(one, 8, q2, 2, one, one, None, big, None) == -2
    assert cloud(one, 8, None, 2, one, one, one, big, None) == -2
    assert cloud(one, 0, q2, 2, one, one, one, big, None) == -1
    assert cloud(one, -3, q2, 2, one, one, one, big, None) == -1
    assert cloud(one, 8, q2, 0, one, one, one, big, None) == -2
    assert cloud(one, 8, (ctypes.c_double * 5)(), 5, one, one, one, big, None) == -2
    for bad in (-0.01, 1.01, float('nan'), float('inf')):
        assert cloud(one, 8, (ctypes.c_double * 2)(0.5, bad), 2, one, one, one, big, None) == -2, bad
    assert cloud(one, 8, q2, 2, one, one, one, size(2) - 1, None) == -3
    assert cloud(one, 8, q2, 2, one, one, ctypes.c_void_p(260), big, None) == -2 and b'aligned' in lib.v3d_last_error()
    assert fused(None, one, 1, 4, 4, q2, 2, one, one, one, big, None) == -2
    assert fused(one, None, 1, 4, 4, q2, 2, one, one, one, big, None) == -2
    for n, h, w in ((0, 4, 4), (1, -1, 4), (1, 4, 0), (2048, 1024, 1024), (1, 65536, 32768), (3, 32768, 32768)):
        assert fused(one, one, n, h, w, q2, 2, one, one, one, big, None) == -1, (n, h, w)
    assert fused(one, one, 1, 4, 4, q2, 7, one, one, one, big, None) == -2
    assert fused(one, one, 1, 4, 4, (ctypes.c_double * 1)(2.0), 1, one, one, one, big, None) == -2
    assert fused(one, one, 1, 4, 4, q2, 2, one, one, one, 16, None) == -3
    assert lib.v3d_version() == 9
