#!/usr/bin/env python3
"""Developer check of the window warp kernel's pass skip (developer option psv_skip): writes the variance volumes of a few small
seeded cases in which whole passes miss their source image -- fp32, split and fp32 channel-last (cl8) output -- and the sample
positions the device works with to an .npz, one run per option set, for a bit-for-bit comparison (tests/test_psv_skip_gpu.py).

    python scripts/psv_skip_dump.py OUT.npz [--option=psv_skip=0] [--option=psv_kernel=1] [--option=psv_walk=N]

Cases: images 128 x 160, feature maps 32 x 32 x 40 of signed values with a few exact -0.0 and denormal entries; cameras 9 degrees
apart on a circle (make_cameras), so that sources five or more images from their reference are wholly out of view.
  a  window (5, 5) = 11 edges per reference, 2 references, D = 24, plane grid 7 x 9
  b  window (6, 6) = 13 edges: more edges than the 8 camera blocks held in LDS, a ragged second camera load
  c  b with each reference's edges permuted: the wholly skipped sources at slots 6, 7, 8, 9, either side of the camera reload
  d  hand-built: a reference with sources [far, far, far, self], one with far sources only (variance +0 everywhere), an ordinary one
  e  the geometry of a with plane grid 5 x 7 (last pixel tile partly dead) and D = 13 (last plane chunk partly dead)
  f  the zoomed / rolled / far-off camera pairs of make_exotic_cameras, D = 13: the out-of-window path beside skipped passes"""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
syn = importlib.import_module('3dvnet_amd.synthetic')
IMG, FEAT = (128, 160), (32, 40)
D0, DD = 0.5, 0.05
YAW = 9.0
FAR = 5                    # sources this many images (or more) from their reference see nothing of its plane sweep at YAW degrees
C_SLOTS = (6, 7, 8, 9)     # case c: where the wholly skipped sources of a reference sit in its edge list


def make_signed_features(n_img, seed):
    """randn features with a few exact -0.0 and denormal entries (the skip's exactness argument is about signed zeros)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((n_img, 32) + FEAT, generator=g, dtype=torch.float32)
    flat = f.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:96]
    flat[idx[:32]] = -0.0
    flat[idx[32:64]] = 1e-41           # denormal
    flat[idx[64:]] = -3e-42
    # the first and last cell of every image, where a footprint half outside the image lands
    f[:, :, 0, 0] = -0.0
    f[:, 0, -1, -1] = 1e-41
    return f


def window_case(nb, na, n_ref=2, seed=5):
    edges, n_img = syn.make_edges(n_ref, nb, na)
    R, tv, K = syn.make_cameras(n_img, IMG, seed=seed, yaw_step_deg=YAW)
    return make_signed_features(n_img, seed), R, tv, K, edges


def case_a():
    return window_case(5, 5)


def case_b():
    return window_case(6, 6)


def case_c():
    """b, the edges of each reference reordered: sources FAR or more images away at C_SLOTS (edges_to_csr keeps the order of the
    edge list within a reference)."""
    feat, R, tv, K, edges = case_b()
    cols = []
    for ref in torch.unique(edges[0]).tolist():
        mine = [i for i in range(edges.shape[1]) if int(edges[0, i]) == ref]
        far = [i for i in mine if abs(int(edges[1, i]) - ref) >= FAR]
        near = [i for i in mine if abs(int(edges[1, i]) - ref) < FAR]
        assert len(far) == len(C_SLOTS)
        near = near[::-1]                                   # not the sorted order either
        order, fi, ni = [], 0, 0
        for slot in range(len(mine)):
            if slot in C_SLOTS:
                order.append(far[fi]); fi += 1
            else:
                order.append(near[ni]); ni += 1
        cols += order
    return feat, R, tv, K, edges[:, cols]


D_REFS = dict(far_self=0, far_only=13, ordinary=6)


def case_d():
    feat, R, tv, K, _ = case_b()                            # 14 images
    refs = [0] * 4 + [13] * 3 + [6] * 5
    srcs = [5, 6, 7, 0] + [8, 7, 6] + [4, 5, 6, 7, 8]
    return feat, R, tv, K, torch.tensor([refs, srcs])


def case_f():
    R, tv, K = syn.make_exotic_cameras(IMG, seed=9)
    return make_signed_features(6, 9), R, tv, K, torch.tensor([[0] * 5 + [4] * 3, [0, 1, 2, 3, 5, 4, 1, 2]])


# tag -> (case, depth_start, D, plane grid)
CASES = {
    'a': (case_a, D0, 24, (7, 9)),
    'b': (case_b, D0, 24, (7, 9)),
    'c': (case_c, D0, 24, (7, 9)),
    'd': (case_d, D0, 24, (7, 9)),
    'e': (case_a, D0, 13, (5, 7)),
    'f': (case_f, 0.4, 13, (15, 19)),
}


def main():
    mvs = importlib.import_module('3dvnet_amd.mvsnet')
    out, opts = sys.argv[1], [a for a in sys.argv[2:] if a.startswith('--option=')]
    reuse = False
    for a in opts:
        name, val = a[len('--option='):].split('=')
        importlib.import_module('3dvnet_amd._lib').set_option(name, int(val))
        reuse = reuse or (name == 'psv_kernel' and int(val) != 0)
    dev = torch.device('cuda:0')
    res = {}
    for tag, (case, d0, D, plane) in CASES.items():
        feat, R, tv, K, edges = case()
        for kind in ('f32', 'split') + (() if reuse else ('cl8',)):      # only the window kernel writes cl8
            v = mvs.plane_sweep_variance(feat.to(dev), R, tv, K, edges.to(dev), d0, DD, D, IMG, plane,
                                         split=kind == 'split', cl8=kind == 'cl8')
            torch.cuda.synchronize()
            data = v if kind == 'f32' else v.data
            res['%s_%s' % (tag, kind)] = data.contiguous().view(torch.uint8).cpu().numpy().copy()
        # the positions the kernels sample at, [E, D * h * w, 2] in CSR edge order, and that order's sources
        pos, _, csr = mvs.plane_sweep_sample_positions(R, tv, K, edges, d0, DD, D, IMG, FEAT, plane, dev)
        res[tag + '_pos'] = pos.cpu().numpy()
        res[tag + '_ref'] = csr[1].cpu().numpy()
        res[tag + '_ofs'] = csr[2].cpu().numpy()
        res[tag + '_src'] = csr[3].cpu().numpy()
    np.savez(out, **res)


if __name__ == '__main__':
    main()
