#!/usr/bin/env python3
"""How much of the window warp kernel's work the pass skip (csrc/psv_window.hip, developer option psv_skip) can leave out at
a given shape: the share of samples that fall wholly beside their source image, of (8 pixels, plane, edge) steps made of such
samples only, and of (8 pixels, 8 planes, edge) passes made of such samples only -- the passes the kernel skips.  CPU only.

    python scripts/psv_skip_share.py [--config cfg2] [--views 16] [--seed N]

A sample is zero when its position in feature cells is not inside (-1, Wf) x (-1, Hf) (NaN counts as zero): every cell of its
2 x 2 footprint is then zero padding or carries the weight 0.  Samples are grouped as the kernel groups them: 8 consecutive
flat pixels of the plane grid x 8 consecutive planes x 1 edge; lanes beyond the last pixel / the last plane count as zero.
The positions are worked out here in float64 from the cameras (the kernel's float32 positions differ in the last bits, which
moves a share by a sample or two; tests/test_psv_skip_gpu.py applies the same rule to the device's own positions)."""
import argparse
import importlib
import os
import sys

import numpy as np

PIX, PLANES = 8, 8       # kRPix, kRDB of csrc/psv_kernels.h


def sample_positions(rotmats, tvecs, K, edges, depth_start, depth_interval, n_planes, img_size, feat_size, plane_size):
    """-> (ix, iy) float64 [E, D, h*w] in feature cells, edge e = column e of `edges` ([2, E]: reference, source)."""
    R, t, K = (np.asarray(x, dtype=np.float64) for x in (rotmats, tvecs, K))
    edges = np.asarray(edges)
    (H, W), (Hf, Wf), (h, w) = img_size, feat_size, plane_size
    xs, ys = np.linspace(0, W - 1, w), np.linspace(0, H - 1, h)
    z = depth_start + depth_interval * np.arange(n_planes)
    xx, yy = np.meshgrid(xs, ys)
    pix = np.stack((xx.ravel(), yy.ravel(), np.ones(h * w)))                       # [3, P]
    cam = (pix[:, None, :] * z[None, :, None]).reshape(3, -1)                      # [3, D * P]
    ix = np.empty((edges.shape[1], n_planes, h * w))
    iy = np.empty_like(ix)
    for e, (ref, src) in enumerate(edges.T):
        world = R[ref].T @ (np.linalg.inv(K[ref]) @ cam - t[ref][:, None])
        q = K[src] @ (R[src] @ world + t[src][:, None])
        zb = np.abs(q[2]) + 1e-8
        gx, gy = q[0] / zb / (W - 1) * 2 - 1, q[1] / zb / (H - 1) * 2 - 1          # normalised with the IMAGE size
        ix[e] = ((gx + 1) * 0.5 * (Wf - 1)).reshape(n_planes, -1)
        iy[e] = ((gy + 1) * 0.5 * (Hf - 1)).reshape(n_planes, -1)
    return ix, iy


def zero_mask(ix, iy, feat_size):
    """The kernel's rule, on unclamped positions: zero unless -1 < ix < Wf and -1 < iy < Hf (a NaN is zero)."""
    Hf, Wf = feat_size
    return ~((ix > -1) & (ix < Wf) & (iy > -1) & (iy < Hf))


def pass_live_counts(zero):
    """zero [E, D, P] bool -> int [E, ceil(D / 8), ceil(P / 8)]: non-zero samples per pass."""
    E, D, P = zero.shape
    nd, nt = -(-D // PLANES), -(-P // PIX)
    live = np.zeros((E, nd * PLANES, nt * PIX), dtype=np.int64)
    live[:, :D, :P] = ~zero
    return live.reshape(E, nd, PLANES, nt, PIX).sum(axis=(2, 4))


def shares(zero):
    """zero [E, D, P] bool -> (share of samples, of (8 px, plane, edge) steps, of (8 px, 8 planes, edge) passes) that are zero."""
    E, D, P = zero.shape
    nt = -(-P // PIX)
    step = np.ones((E, D, nt * PIX), dtype=bool)
    step[:, :, :P] = zero
    step = step.reshape(E, D, nt, PIX).all(axis=3)
    return float(zero.mean()), float(step.mean()), float((pass_live_counts(zero) == 0).mean())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--config', default='cfg2')
    ap.add_argument('--views', type=int, default=16, help='reference views of the sliding-window batch')
    ap.add_argument('--seed', type=int, default=None, help='default: the config\'s own seed')
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    syn = importlib.import_module('3dvnet_amd.synthetic')
    c = syn.make_costvolume_inputs(a.config, a.views, seed=a.seed)
    d0, dd, D = c['depth']
    ix, iy = sample_positions(c['rotmats'].numpy(), c['tvecs'].numpy(), c['K'].numpy(), c['edges'].numpy(), d0, dd, D,
                              c['img_size'], c['feat_size'], c['plane_size'])
    zero = zero_mask(ix, iy, c['feat_size'])
    s = shares(zero)
    print('%s, %d views, %d edges: samples zero %.1f %%, (8 px, plane, edge) steps all zero %.1f %%, passes all zero %.1f %%'
          % (a.config, a.views, zero.shape[0], 100 * s[0], 100 * s[1], 100 * s[2]))
    per = c['edges'].shape[1] // a.views
    print('zero samples per edge slot of a reference (%%): %s'
          % ' '.join('%.0f' % (100 * zero[k::per].mean()) for k in range(per)))


if __name__ == '__main__':
    main()
