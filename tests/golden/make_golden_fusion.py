#!/usr/bin/env python3
"""Golden vectors of multi-view depth fusion: the REFERENCE's own ``mv3d/eval/pointcloudfusion_custom.py`` run on the CPU,
unmodified, from where it lies (imported with the stubs of _ref_import.py; ``torch.Tensor.cuda`` is made a no-op so that
its ``.cuda()`` calls stay on the host).

Run in the build container only:  python tests/golden/make_golden_fusion.py
Outputs tests/golden/F_fusion_*.npz (committed): seeded inputs, thresholds and the reference's outputs -- data only.
Every file stays at or below the largest golden there was before (C_decoder_net.npz): when the fused points would not
fit, every `pts_stride`-th row is stored (the full count, mask and colours always are).
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import  # noqa: E402
import fusion_oracle  # noqa: E402

LIMIT = 587073          # bytes of tests/golden/C_decoder_net.npz

_ref_import.install_stubs()
torch.Tensor.cuda = lambda self, *a, **k: self
from mv3d.eval import pointcloudfusion_custom as ref_fusion  # noqa: E402


def save(name, pts, **arrays):
    path = os.path.join(HERE, name + '.npz')
    stride = 1
    while True:
        np.savez_compressed(path, fused_pts=pts[::stride], pts_stride=np.int64(stride), n_fused=np.int64(pts.shape[0]),
                            **arrays)
        if os.path.getsize(path) <= LIMIT:
            break
        stride += 1
        assert stride <= 64, 'the inputs of %s alone exceed the size limit' % name
    print('wrote %s (%.1f KB, %d points, every %d stored)' % (path, os.path.getsize(path) / 1024, pts.shape[0], stride))


def scene_case(name, depths, images, poses, K, z_thresh, n_thresh):
    with torch.no_grad():
        pts, rgb, valid = ref_fusion.process_scene(depths.clone(), images.clone(), poses.clone(), K.clone(), z_thresh, n_thresh)
    save(name, pts, depths=depths.numpy(), images=images.numpy(), poses=poses.numpy(), K=K.numpy(),
         z_thresh=np.float64(z_thresh), n_consistent_thresh=np.int64(n_thresh), fused_rgb=rgb, all_valid=valid)


def main():
    # (a) 12 views of 48 x 64, 6 degrees apart, 4 cm noise, 3 % of the pixels zeroed
    scene_case('F_fusion_a', *fusion_oracle.scene(12, (48, 64), seed=3, yaw_step_deg=6, sigma=0.04), 0.1, 3)
    # (b) 16 views of 60 x 80, 4 degrees apart, 5 cm noise
    scene_case('F_fusion_b', *fusion_oracle.scene(16, (60, 80), seed=4, yaw_step_deg=4, sigma=0.05), 0.1, 3)
    # (c) tiny, with one camera turned away (points behind it: z <= 1e-4) and one turned by a quarter (samples outside the image)
    d, img, poses, K = fusion_oracle.scene(6, (12, 16), seed=5, yaw_step_deg=5, sigma=0.02)
    for i, ang in ((2, math.pi), (4, math.pi / 2)):
        c, s = math.cos(ang), math.sin(ang)
        turn = torch.tensor([[c, 0., s], [0., 1., 0.], [-s, 0., c]])            # about the camera's y axis
        R = turn @ poses[i, :3, :3]
        centre = -poses[i, :3, :3].T @ poses[i, :3, 3]
        poses[i, :3, :3] = R
        poses[i, :3, 3] = -R @ centre
    scene_case('F_fusion_c', d, img, poses, K, 0.1, 2)
    # (d) process_depth with an explicit source subset (reference 2; sources 0, 1, 4, 5, 6 of 7 views)
    d, img, poses, K = fusion_oracle.scene(7, (24, 32), seed=6, yaw_step_deg=5, sigma=0.03)
    ref, srcs = 2, [0, 1, 4, 5, 6]
    with torch.no_grad():
        pts, rgb, valid = ref_fusion.process_depth(d[ref].clone(), img[ref].clone(), d[srcs].clone(), img[srcs].clone(),
                                                   poses[ref].clone(), poses[srcs].clone(), K[ref].clone(), K[srcs].clone(),
                                                   z_thresh=0.08, n_consistent_thresh=2)
    save('F_fusion_d', pts, depths=d.numpy(), images=img.numpy(), poses=poses.numpy(), K=K.numpy(), ref=np.int64(ref),
         srcs=np.asarray(srcs), z_thresh=np.float64(0.08), n_consistent_thresh=np.int64(2), fused_rgb=rgb,
         all_valid=valid[None])


if __name__ == '__main__':
    main()
