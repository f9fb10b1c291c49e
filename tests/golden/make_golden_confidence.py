#!/usr/bin/env python3
"""Golden vectors of the photometric confidence maps: the REFERENCE's own ``get_propability_map`` (``mv3d/utils.py:111-145``)
executed on CPU torch from where it lies, through the import stand-ins of _ref_import.py (``cv2`` and the other packages its
module imports at the top); softmax and expectation are the three stock calls of ``mvsnet.py:220-227``.  Nothing of the
reference's text is written to disk.

Run in the build container only:  python tests/golden/make_golden_confidence.py
Outputs tests/golden/P_conf_*.npz (committed) -- data only.  Large inputs are not stored: they are seeded
(tests/confidence_oracle.py: ``logits`` / ``volume``) and the fixture holds their SHA-256.

  P_conf_gather  gather mode: for each case a seeded volume [n, D, h, w] (uniform values: gather mode asks nothing of them), a
                 depth map that visits every branch (0, far outside on both sides, just outside either end, every plane's own
                 depth, uniform depths around the grid) and the reference's map.  Cases: every D of {1, 7, 8, 9, 96}, every
                 h x w of {8 x 8, 24 x 24, 56 x 56}, n of {1, 3}.
  P_conf_a       logits [2, 96, 56, 56] = randn * 1 (seeded, not stored); depth_start 0.5, depth_interval 0.05
  P_conf_b       logits [3, 8, 8, 8] = randn * 3 (stored)
                 Both: the reference's fp32 probability volume is not stored; stored are its depth (the expectation), its map of
                 that depth, a given depth map and its map of that, and the reference's own fp32 error against the float64
                 checker -- the yardstick of the GPU tests: for its own depth outside the uncertain set (share asserted <= 3 %),
                 for the given depth over all pixels with the planes of the fp32 chain.
  P_conf_c       logits [3, 8, 8, 8] = randn * 30, near one-hot: given-depth mode only (half of the own-depth pixels would be
                 uncertain)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import confidence_oracle as oracle  # noqa: E402

LIMIT = 587073          # bytes of tests/golden/C_decoder_net.npz, the largest golden there is
REF = _ref_import.reference().utils.get_propability_map
DEPTH_START, DEPTH_INTERVAL = 0.5, 0.05
GATHER_CASES = [(1, 1, 8, 8), (3, 1, 56, 56), (3, 7, 24, 24), (1, 8, 24, 24), (3, 9, 8, 8), (1, 96, 8, 8), (3, 96, 24, 24),
                (1, 96, 56, 56)]          # (n, D, h, w)


def save(name, arrays):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= LIMIT, (path, os.path.getsize(path))
    print('wrote %s (%.1f KB)' % (path, os.path.getsize(path) / 1024))


def gather():
    arrays = dict(cases=np.asarray(GATHER_CASES, dtype=np.int64), depth_start=np.float64(DEPTH_START),
                  depth_interval=np.float64(DEPTH_INTERVAL))
    for i, (n, D, h, w) in enumerate(GATHER_CASES):
        cv = oracle.volume((n, D, h, w), 100 + i)
        depth = oracle.special_depths(DEPTH_START, DEPTH_INTERVAL, D, n * h * w, 200 + i).reshape(n, h, w)
        with torch.no_grad():
            ref = REF(torch.from_numpy(cv), torch.from_numpy(depth), DEPTH_START, DEPTH_INTERVAL).numpy()
        assert ref.dtype == np.float32 and ref.shape == (n, h, w)
        arrays.update({'cv_sha_%d' % i: np.str_(oracle.digest(cv)), 'depth_%d' % i: depth, 'prob_%d' % i: ref})
    save('P_conf_gather', arrays)


def logits_case(name, shape, scale, seed, store_x, own):
    n, D, h, w = shape
    x = oracle.logits(shape, scale, seed)
    vals = torch.linspace(DEPTH_START, DEPTH_START + DEPTH_INTERVAL * (D - 1), D)
    with torch.no_grad():
        xt = torch.from_numpy(x)
        x_prob = F.softmax(-xt, dim=1)                                          # mvsnet.py:220
        depth_volume = vals.unsqueeze(0).repeat(n, 1).view(n, D, 1, 1).expand(x_prob.shape)      # :224-225
        depth_img = torch.sum(depth_volume * x_prob, dim=1)                     # :227
        given = torch.from_numpy(oracle.special_depths(DEPTH_START, DEPTH_INTERVAL, D, n * h * w, seed + 1).reshape(n, h, w))
        prob_own = REF(x_prob, depth_img, DEPTH_START, DEPTH_INTERVAL).numpy()
        prob_given = REF(x_prob, given, DEPTH_START, DEPTH_INTERVAL).numpy()
    p64 = oracle.softmax64(x)
    # given depth: the planes of the fp32 chain, the values in float64
    lr = oracle.indices_f32(given.numpy(), DEPTH_START, DEPTH_INTERVAL, D)
    want_given = oracle.check(p64, given.numpy(), DEPTH_START, DEPTH_INTERVAL, indices=lr)['prob']
    arrays = dict(shape=np.asarray(shape, dtype=np.int64), scale=np.float64(scale), seed=np.int64(seed),
                  x_sha=np.str_(oracle.digest(x)), depth_start=np.float64(DEPTH_START), depth_interval=np.float64(DEPTH_INTERVAL),
                  depth_vals=vals.numpy(), depth_given=given.numpy(), prob_given=prob_given,
                  ref_err_given=np.float64(oracle.max_error(prob_given, want_given)))
    msg = '%s: %s x %g: reference fp32 error given-depth %.3g' % (name, 'x'.join(map(str, shape)), scale, arrays['ref_err_given'])
    if store_x:
        arrays['x'] = x
    # its own depth: planes and values in float64 from the float64 expectation; outside the uncertain set the reference's
    # planes must be the checker's
    depth64 = oracle.expectation64(p64, vals.numpy())
    own64 = oracle.check(p64, depth64, DEPTH_START, DEPTH_INTERVAL)
    share = float(own64['uncertain'].mean())
    if own:
        assert share <= oracle.UNCERTAIN_CAP, share
        keep = ~own64['uncertain']
        l, r = oracle.indices_f32(depth_img.numpy(), DEPTH_START, DEPTH_INTERVAL, D)
        assert np.array_equal(l[keep], own64['l'][keep]) and np.array_equal(r[keep], own64['r'][keep])
        arrays.update(depth=depth_img.numpy(), prob_own=prob_own, uncertain_share=np.float64(share),
                      ref_err_own=np.float64(oracle.max_error(prob_own, own64['prob'], keep)),
                      ref_err_depth=np.float64(oracle.max_error(depth_img.numpy(), depth64)))
        msg += ', own depth %.3g (depth %.3g)' % (arrays['ref_err_own'], arrays['ref_err_depth'])
    print(msg + '; uncertain %.2f %%' % (100 * share))
    save(name, arrays)


def main():
    gather()
    logits_case('P_conf_a', (2, 96, 56, 56), 1.0, 11, store_x=False, own=True)
    logits_case('P_conf_b', (3, 8, 8, 8), 3.0, 12, store_x=True, own=True)
    logits_case('P_conf_c', (3, 8, 8, 8), 30.0, 13, store_x=True, own=False)


if __name__ == '__main__':
    main()
