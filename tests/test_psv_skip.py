"""scripts/psv_skip_share.py groups samples as the window warp kernel does -- 8 consecutive flat pixels x 8 consecutive planes x 1
edge, lanes beyond the last pixel / plane counting as zero -- checked here against a loop over the passes on a tiny ragged shape."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _share_module():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import psv_skip_share as ss
    finally:
        sys.path.pop(0)
    return ss


def _brute(zero):
    E, D, P = zero.shape
    nd, nt = (D + 7) // 8, (P + 7) // 8
    cnt = np.zeros((E, nd, nt), dtype=np.int64)
    steps = []
    for e in range(E):
        for d in range(D):
            for t in range(nt):
                steps.append(all(zero[e, d, p] for p in range(8 * t, min(8 * t + 8, P))))
            for p in range(P):
                cnt[e, d // 8, p // 8] += 0 if zero[e, d, p] else 1
    return cnt, float(np.mean(steps))


def test_grouping_against_a_loop_over_the_passes():
    ss = _share_module()
    rng = np.random.RandomState(0)
    E, D, P = 3, 13, 35                     # partial last plane chunk, partial last pixel tile
    zero = rng.rand(E, D, P) < 0.6
    zero[0] = True                          # a wholly skipped edge
    zero[1, :8, 8:16] = True                # one skipped pass
    zero[1, 8:, 32:] = True                 # a skipped pass made of dead lanes and zeros
    zero[2, :8, 16:24] = True
    zero[2, 3, 17] = False                  # a near miss: one sample inside the image
    cnt, step_share = _brute(zero)
    got = ss.pass_live_counts(zero)
    assert got.shape == (E, 2, 5) and np.array_equal(got, cnt)
    assert (got[0] == 0).all() and got[1, 0, 1] == 0 and got[1, 1, 4] == 0 and got[2, 0, 2] == 1
    s = ss.shares(zero)
    assert s[0] == float(zero.mean())
    assert abs(s[1] - step_share) < 1e-12
    assert s[2] == float((cnt == 0).mean())


def test_zero_rule_is_exact_at_the_image_border():
    ss = _share_module()
    Hf, Wf = 4, 6
    ix = np.array([-1.0, np.nextafter(-1.0, 0.0), -0.5, 0.0, 5.0, 5.5, np.nextafter(6.0, 0.0), 6.0, np.nan, 2.0, 2.0, 2.0])
    iy = np.array([1.0] * 9 + [-1.0, 4.0, np.nextafter(4.0, 0.0)])
    want = [True, False, False, False, False, False, False, True, True, True, True, False]
    assert ss.zero_mask(ix, iy, (Hf, Wf)).tolist() == want


def test_positions_of_the_self_edge_are_the_pixel_grid():
    ss = _share_module()
    K = np.array([[[100.0, 0, 40.0], [0, 100.0, 30.0], [0, 0, 1]]])
    ix, iy = ss.sample_positions(np.eye(3)[None], np.zeros((1, 3)), K, np.array([[0], [0]]), 1.0, 0.5, 3, (61, 81), (16, 21), (4, 5))
    assert ix.shape == (1, 3, 20)
    np.testing.assert_allclose(ix[0, 2].reshape(4, 5)[1], np.linspace(0, 20, 5), atol=1e-5)
    np.testing.assert_allclose(iy[0, 0].reshape(4, 5)[:, 3], np.linspace(0, 15, 4), atol=1e-5)
