"""CPU: the yardsticks of the confidence-map tests (tests/confidence_oracle.py) against the reference-written fixtures
(tests/golden/P_conf_*.npz, made by tests/golden/make_golden_confidence.py from the reference's own get_propability_map):
the fp32 restatement equals the reference bit for bit in gather mode, the float64 checker agrees with it outside the
uncertain set, and the hand-computed edge cases of the chain."""
import os

import numpy as np
import pytest

import confidence_oracle as oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
F32 = np.float32


def load(name):
    with np.load(os.path.join(GOLDEN, name + '.npz')) as f:
        return {k: f[k] for k in f.files}


def fixture_logits(g):
    x = g['x'] if 'x' in g else oracle.logits(tuple(int(v) for v in g['shape']), float(g['scale']), int(g['seed']))
    assert oracle.digest(x) == str(g['x_sha'])          # the seeded generator still gives the bits the reference saw
    return x


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_restatement_equals_the_reference_in_gather_mode():
    g = load('P_conf_gather')
    ds, di = float(g['depth_start']), float(g['depth_interval'])
    seen_D, seen_hw, seen_n = set(), set(), set()
    for i, (n, D, h, w) in enumerate(g['cases']):
        cv = oracle.volume((n, D, h, w), 100 + i)
        assert oracle.digest(cv) == str(g['cv_sha_%d' % i])
        got = oracle.gather_f32(cv, g['depth_%d' % i], ds, di)
        assert np.array_equal(bits(got), bits(g['prob_%d' % i])), (n, D, h, w)
        seen_D.add(int(D)), seen_hw.add(int(h)), seen_n.add(int(n))
    assert seen_D == {1, 7, 8, 9, 96} and seen_hw == {8, 24, 56} and seen_n == {1, 3}


@pytest.mark.parametrize('name', ['P_conf_a', 'P_conf_b', 'P_conf_c'])
def test_restatement_and_checker_on_the_logit_fixtures(name):
    g = load(name)
    x = fixture_logits(g)
    ds, di, D = float(g['depth_start']), float(g['depth_interval']), x.shape[1]
    p64 = oracle.softmax64(x)
    # given depth: the planes of the fp32 chain; the reference's values lie within its recorded error of the checker, and the
    # NumPy restatement of the tail (another exp) within a few ulp of the largest value
    lr = oracle.indices_f32(g['depth_given'], ds, di, D)
    want = oracle.check(p64, g['depth_given'], ds, di, indices=lr)['prob']
    assert oracle.max_error(g['prob_given'], want) == float(g['ref_err_given'])
    assert oracle.max_error(oracle.logits_f32(x, g['depth_given'], ds, di), want) <= 16 * np.finfo(F32).eps * want.max()
    if 'prob_own' not in g:
        return
    # its own depth: outside the uncertain set the reference's planes are the checker's
    own = oracle.check(p64, oracle.expectation64(p64, g['depth_vals']), ds, di)
    keep = ~own['uncertain']
    assert own['uncertain'].mean() == float(g['uncertain_share']) <= oracle.UNCERTAIN_CAP
    l, r = oracle.indices_f32(g['depth'], ds, di, D)
    assert np.array_equal(l[keep], own['l'][keep]) and np.array_equal(r[keep], own['r'][keep])
    assert oracle.max_error(g['prob_own'], own['prob'], keep) == float(g['ref_err_own'])
    assert float(g['ref_err_own']) < 1e-6


def test_hand_computed_cases():
    ds, di = 0.5, 0.05
    # D = 1: both planes are plane 0 wherever the depth lies: 2 p = 2 for a probability volume
    one = np.ones((1, 1, 2, 2), dtype=F32)
    depth = np.array([[[0.5, 0.7], [0.0, 9.0]]], dtype=F32)
    assert np.array_equal(oracle.gather_f32(one, depth, ds, di), np.full((1, 2, 2), 2, dtype=F32))
    assert np.array_equal(oracle.check(one.astype(np.float64), depth, ds, di)['prob'], np.full((1, 2, 2), 2.))
    # D = 4, p = (0.1, 0.2, 0.3, 0.4) at every pixel
    p = np.array([0.1, 0.2, 0.3, 0.4], dtype=F32)
    cv = np.broadcast_to(p[None, :, None, None], (1, 4, 1, 6)).copy()
    depth = np.array([[[0.3, 0.9, 0.0, 0.575, np.nan, np.inf]]], dtype=F32)
    want = np.array([[[p[0] + p[0],          # below the first plane: 2 p[0]
                       p[3] + p[3],          # above the last plane: 2 p[D - 1]
                       p[0] + p[0],          # depth 0, a masked pixel: far below the grid
                       p[1] + p[2],          # between planes 1 and 2
                       p[0] + p[0],          # NaN: pinned to plane 0
                       p[0] + p[0]]]], dtype=F32)      # +inf: pinned to plane 0
    assert np.array_equal(bits(oracle.gather_f32(cv, depth, ds, di)), bits(want))
    l, r = oracle.indices_f32(np.array([-np.inf, 1e30, -1e30], dtype=F32), ds, di, 4)
    assert l.tolist() == [0, 3, 0] and r.tolist() == [0, 3, 0]          # -inf pinned; enormous finite depths clamp
    chk = oracle.check(cv.astype(np.float64), depth, ds, di)
    assert np.allclose(chk['prob'], want.astype(np.float64), rtol=0, atol=1e-7)


def test_on_plane_quirk():
    """The fp32 coordinate of a plane's own depth is not always that plane's integer: of linspace(0.5, 5.25, 96), 68 planes land
    on it (l == r: the plane's value twice), 9 above (the plane and the next), 19 below (the previous plane and the plane).
    The reference's map of the fixture whose depths start with those planes must be exactly that."""
    g = load('P_conf_gather')
    ds, di = float(g['depth_start']), float(g['depth_interval'])
    i = [k for k, c in enumerate(g['cases']) if tuple(c) == (3, 96, 24, 24)][0]
    planes = oracle.plane_depths(ds, di, 96)
    depth = g['depth_%d' % i].reshape(-1)
    assert np.array_equal(depth[5:5 + 96], planes)
    d = oracle.coordinate_f32(planes, ds, di)
    k = np.arange(96)
    exact, above, below = d == k, d > k, d < k
    assert (int(exact.sum()), int(above.sum()), int(below.sum())) == (68, 9, 19)
    assert np.all(np.abs(d - k) < 1e-4)
    cv = oracle.volume((3, 96, 24, 24), 100 + i)
    col = np.stack([cv[0, :, (5 + j) // 24, (5 + j) % 24] for j in range(96)])          # col[j] = the column of pixel 5 + j
    up, down = np.minimum(k + 1, 95), np.maximum(k - 1, 0)
    want = np.where(exact, col[k, k] + col[k, k], np.where(above, col[k, k] + col[k, up], col[k, down] + col[k, k])).astype(F32)
    ref = g['prob_%d' % i].reshape(-1)[5:5 + 96]
    assert np.array_equal(bits(ref), bits(want))
    assert np.array_equal(bits(oracle.gather_f32(cv, g['depth_%d' % i], ds, di).reshape(-1)[5:5 + 96]), bits(want))
