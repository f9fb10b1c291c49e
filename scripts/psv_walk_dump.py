#!/usr/bin/env python3
"""Developer check of the window warp kernel's depth walk (developer option psv_walk): writes the variance volumes of a few small
seeded cases -- fp32, split and fp32 channel-last (cl8) output -- to an .npz, one run per option set, for a bit-for-bit comparison
(tests/test_psv_walk_gpu.py).

    python scripts/psv_walk_dump.py OUT.npz [--option=psv_walk=N] [--option=psv_kernel=1]

Cases: feature maps 32 x 16 x 20, image 64 x 80; plane grids 7 x 9 (partial pixel tile) and 8 x 8; D in 6, 13, 24, 40 (one partial
chunk, a partial last chunk, exact chunks, 5 chunks); ragged, unsorted edge lists with 1, 3, 7 and 10 sources (7: the division
path of the mean, 10: more than the 8 camera blocks held in LDS); the zoomed / rolled / far-off camera pairs of
scripts/psv_hash.py (out-of-window path); the D = 40 case twice (run-to-run identity) and its last chunk as a launch of its own."""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
syn = importlib.import_module('3dvnet_amd.synthetic')
mvs = importlib.import_module('3dvnet_amd.mvsnet')
IMG, FEAT = (64, 80), (16, 20)
D0, DD = 0.5, 0.3


def ragged_case():
    R, tv, K = syn.make_cameras(12, IMG, seed=3)
    feat = syn.make_features(12, 32, *FEAT, seed=3)
    refs = [4] + [7] * 3 + [5] * 7 + [2] * 10
    srcs = [4] + [6, 7, 8] + [0, 1, 2, 3, 6, 7, 8] + list(range(0, 10))
    perm = torch.randperm(len(refs), generator=torch.Generator().manual_seed(0))
    return feat, R, tv, K, torch.tensor([refs, srcs])[:, perm]


def exotic_case():
    R, tv, K = syn.make_exotic_cameras(IMG, seed=9)      # shared with scripts/psv_hash.py
    feat = syn.make_features(6, 32, *FEAT, seed=9)
    return feat, R, tv, K, torch.tensor([[0] * 5 + [4] * 3, [0, 1, 2, 3, 5, 4, 1, 2]])


def leak_case():
    """one view with a single edge and one with 10, in the same launch"""
    feat, R, tv, K, _ = ragged_case()
    return feat, R, tv, K, torch.tensor([[4] + [2] * 10, [6] + list(range(0, 10))])


def main():
    out, opts = sys.argv[1], [a for a in sys.argv[2:] if a.startswith('--option=')]
    reuse = False
    for a in opts:
        name, val = a[len('--option='):].split('=')
        importlib.import_module('3dvnet_amd._lib').set_option(name, int(val))
        reuse = reuse or (name == 'psv_kernel' and int(val) != 0)
    dev = torch.device('cuda:0')
    res = {}

    def run(tag, case, d0, D, plane):
        feat, R, tv, K, edges = case
        for kind in ('f32', 'split') + (() if reuse else ('cl8',)):      # only the window kernel writes cl8
            v = mvs.plane_sweep_variance(feat.to(dev), R, tv, K, edges.to(dev), d0, DD, D, IMG, plane,
                                         split=kind == 'split', cl8=kind == 'cl8')
            torch.cuda.synchronize()
            data = v if kind == 'f32' else v.data
            res['%s_%s' % (tag, kind)] = data.contiguous().view(torch.uint8).cpu().numpy().copy()

    rc, ec, lc = ragged_case(), exotic_case(), leak_case()
    for D in (6, 13, 24, 40):
        for plane in ((7, 9), (8, 8)):
            run('ragged_D%d_%dx%d' % (D, *plane), rc, D0, D, plane)
    for D in (13, 40):
        run('exotic_D%d' % D, ec, 0.4, D, (15, 19))
    run('again_D40', rc, D0, 40, (7, 9))
    run('leak_D40', lc, D0, 40, (7, 9))
    run('leak_last8', lc, D0 + 32 * DD, 8, (7, 9))
    np.savez(out, **res)


if __name__ == '__main__':
    main()
