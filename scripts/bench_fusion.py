#!/usr/bin/env python3
"""Depth fusion on the device: the HIP path (3dvnet_amd/fusion.py: v3d_fuse_depths_f32 + v3d_fusion_compact) against the
same algorithm in stock torch ops on the same GPU -- what a user has today -- in one run.

    python scripts/bench_fusion.py [--size 256x320,480x640] [--views 64] [--repeats 20] [--warmup 3] [--profile]

Scenes: the 64-view ring of synthetic.make_cameras (cfg3), analytic box-room depths + N(0, 4 cm), 3 % of the pixels zeroed.
Timing: HIP events around the whole device-level call (camera blocks, the two library calls, no read-back) and, with the
library's own event brackets, around fuse_depths_kernel alone; the torch restatement is timed the same way around one whole
scene (all views as references, sources in batches).  One JSON line per run.  `--profile` runs only the HIP path a few
times (for rocprofv3).

Measured on one MI355X (profiles/r09_bench_fusion.json; 64 views, 20 timed repeats of each route):
  256 x 320: HIP call 0.593 ms (fuse_depths_kernel 0.387 ms = 0.65 of it, compaction 0.080 ms), torch 125.2 ms: 211 x
  480 x 640: HIP call 1.812 ms (fuse_depths_kernel 1.335 ms = 0.74 of it, compaction 0.319 ms), torch 347.5 ms: 192 x
The two routes' masks differ on 2 / 8 pixels (the torch route sums a batch of sources at once: another order).
"""
import argparse
import importlib
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def torch_fusion(depths, poses, K, Kinv, Pinv, z_thresh, n_thresh, batch=16):
    """The fusion semantics in stock torch ops on the device (written for this script): per reference view, batches of
    source views as [B, 3, h w] tensors; the inverses are given (taken once, outside the timed region).
    -> (points [M, 3], keep [N, h, w])."""
    n, h, w = depths.shape
    R, t = poses[:, :3, :3], poses[:, :3, 3:4]
    ys, xs = torch.meshgrid(torch.arange(h, device=depths.device, dtype=torch.float32),
                            torch.arange(w, device=depths.device, dtype=torch.float32), indexing='ij')
    pix = torch.stack((xs, ys, torch.ones_like(xs)), 0).reshape(3, -1)
    all_pts, all_keep = [], []
    for r in range(n):
        X = Pinv[r, :3, :3] @ (Kinv[r] @ (pix * depths[r].reshape(1, -1))) + Pinv[r, :3, 3:4]
        src = torch.tensor([s for s in range(n) if s != r], device=depths.device)
        acc, cnt = X.clone(), torch.zeros(h * w, device=depths.device)
        for b in range(0, n - 1, batch):
            s = src[b:b + batch]
            q = K[s] @ (R[s] @ X[None] + t[s])
            z = q[:, 2]
            uv = q[:, :2] / z[:, None]
            ok = (z > 1e-4) & (uv[:, 0] >= 0) & (uv[:, 0] <= w - 1) & (uv[:, 1] >= 0) & (uv[:, 1] <= h - 1)
            grid = torch.stack((uv[:, 0] / (w - 1) * 2 - 1, uv[:, 1] / (h - 1) * 2 - 1), -1)[:, :, None]
            zs = F.grid_sample(depths[s][:, None], grid, mode='nearest', align_corners=True, padding_mode='zeros')[:, 0, :, 0]
            ok = ok & ((z - zs).abs() < z_thresh)
            Xs = R[s].transpose(1, 2) @ (Kinv[s] @ torch.cat((uv * zs[:, None], zs[:, None]), 1) - t[s])
            acc = acc + torch.where(ok[:, None], Xs, torch.zeros_like(Xs)).sum(0)
            cnt = cnt + ok.sum(0)
        keep = cnt >= n_thresh
        all_pts.append((acc / (cnt + 1)).T[keep])
        all_keep.append(keep.reshape(h, w))
    return torch.cat(all_pts), torch.stack(all_keep)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='256x320,480x640')
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-repeats', type=int, default=20)
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_fusion.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    fusion = importlib.import_module('3dvnet_amd.fusion')
    lib = importlib.import_module('3dvnet_amd._lib')
    import fusion_oracle as fo
    for size in [tuple(int(v) for v in s.split('x')) for s in args.size.split(',')]:
        d, img, poses, K = fo.scene(args.views, size, seed=1237, yaw_step_deg=None, sigma=0.04)
        Kinv_d, Pinv_d = torch.inverse(K).to(dev), torch.inverse(poses).to(dev)
        d, img, poses_d, K_d = d.to(dev), img.to(dev), poses.to(dev), K.to(dev)

        def hip():
            return fusion.fuse_depth_maps(d, poses, K, img, 0.1, 3)

        if args.profile:
            for _ in range(5):
                hip()
            torch.cuda.synchronize()
            continue
        hip_ms = timed(hip, args.warmup, args.repeats)
        lib.timing_enable(True)
        for _ in range(args.repeats):
            hip()
        spans = lib.timing_collect()
        lib.timing_enable(False)
        kern_ms = spans['fuse_depths'][0] / spans['fuse_depths'][1]
        compact_ms = spans['fusion_compact'][0] / spans['fusion_compact'][1]
        tor_ms = timed(lambda: torch_fusion(d, poses_d, K_d, Kinv_d, Pinv_d, 0.1, 3), 1, args.torch_repeats)
        # same answer: the kept masks of the two routes (they may differ on the few boundary pixels of the checker's rule)
        _, _, valid, count = hip()
        t_pts, t_keep = torch_fusion(d, poses_d, K_d, Kinv_d, Pinv_d, 0.1, 3)
        pairs = args.views * (args.views - 1) * size[0] * size[1]
        print(json.dumps(dict(
            bench='fusion', views=args.views, size=list(size), pairs=pairs, hip_call_ms=round(hip_ms[0], 4),
            hip_call_ms_min_max=[round(hip_ms[1], 4), round(hip_ms[2], 4)], fuse_depths_kernel_ms=round(kern_ms, 4),
            compact_ms=round(compact_ms, 4), kernel_share_of_call=round(kern_ms / hip_ms[0], 3),
            torch_ms=round(tor_ms[0], 3), torch_ms_min_max=[round(tor_ms[1], 3), round(tor_ms[2], 3)],
            ratio_torch_over_hip=round(tor_ms[0] / hip_ms[0], 1), gpairs_per_s=round(pairs / kern_ms / 1e6, 2),
            points=int(count), mask_pixels_differing_from_torch=int((valid != t_keep).sum()),
            repeats=args.repeats, torch_repeats=args.torch_repeats)), flush=True)


if __name__ == '__main__':
    main()
