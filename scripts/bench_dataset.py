#!/usr/bin/env python3
"""Decoded frames -> the images and depth maps of a scene batch: the two frame kernels (3dvnet_amd/dataset.py ->
v3d_frames_to_images_f32 / v3d_frames_to_depths_f32, csrc/frames.hip) against the same result by stock torch ops on the device
and against the reference's per-image route on the host.  One process, every shape warmed, medians.

    python scripts/bench_dataset.py [--frames 71] [--sizes 256x320,240x320] [--repeats 50] [--warmup 5] [--host-repeats 3] [--out FILE]

Workload: `--frames` colour frames of 480x640 uint8 and frames - 2 depth frames of uint16 (the reference views of a window of one
source view on either side), to each of `--sizes` and to 56x56 depth maps, quantised as Dataset does by default.
Per size one JSON line with
  (a) kernels_*      the two kernels on device-resident frames: kernel time (the library's event brackets, mean of `repeats`
                     launches) and call time (host clock between two synchronisations, median)
  (b) upload_*       the same including the copy of the frames from pinned host memory
  (c) torch_device_* the same result by stock torch ops on the device: cast, permute, crop, F.interpolate(bilinear), round, the
                     normalisation chain; index gathers, a division and a mask for the depths
  (d) host_torch_*   the reference's route on the host, one image at a time (dataset.py:159-219) with F.interpolate in place of
                     cv2.resize; host_cv2_* the same with OpenCV where it imports
  byte_model_*       the bytes the colour kernel has to move (frames read once, images written once), the time they take at
                     6.3 TB/s, and the share of it the kernel time reaches
  max_abs_diff_*     the kernels' images against (c) and (d): the three routes compute the same thing
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12          # achievable HBM bandwidth of an MI355X
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DEPTH_SIZE = (56, 56)
FRAME = (480, 640)


def timed(fn, warmup, repeats):
    """Wall-clock milliseconds of fn() between two device synchronisations -> (median, min, max)."""
    import torch
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms.sort()
    return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)]


def torch_device_route(frames, depth_mm, pre, size, ys, xs):
    """(c): stock torch ops on the device."""
    import torch
    import torch.nn.functional as F
    H, W = frames.shape[1:3]
    x = frames[:, pre.crop_y:H - pre.crop_y, pre.crop_x:W - pre.crop_x].permute(0, 3, 1, 2).float()
    x = torch.round(F.interpolate(x, size, mode='bilinear', align_corners=False))
    x = ((x / 255.0) * 255.0) / 255.
    mean = torch.tensor(MEAN, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(STD, device=x.device).view(1, 3, 1, 1)
    x = (x - mean) / std
    d = depth_mm[:, ys][:, :, xs].int().bitwise_and(0xFFFF).float() / 1000.0          # the int16 tensor holds uint16 bits
    d = torch.where(d > 65., torch.zeros_like(d), d)
    return x, d


def host_route(colour, depth_mm, pre, size, resize):
    """(d): one image at a time on the host, as the reference (dataset.py:159-219)."""
    import torch
    import torch.nn.functional as F
    H, W = colour.shape[1:3]
    images, depths = [], []
    for i in range(colour.shape[0]):
        image = resize(colour[i, pre.crop_y:H - pre.crop_y, pre.crop_x:W - pre.crop_x], size)
        image = torch.from_numpy(np.transpose(image, (2, 0, 1)).astype(np.float32))
        image = image / 255.0
        image = (image * 255.0) / 255.
        for c in range(3):
            image[c] = (image[c] - MEAN[c]) / STD[c]
        images.append(image)
    for i in range(depth_mm.shape[0]):
        d = depth_mm[i].astype(np.float32) / 1000.0
        d[d > 65.] = 0
        d = torch.from_numpy(d[pre.crop_y:H - pre.crop_y, pre.crop_x:W - pre.crop_x])[None, None]
        depths.append(F.interpolate(F.interpolate(d, size, mode='nearest'), DEPTH_SIZE, mode='nearest')[0, 0])
    return torch.stack(images), torch.stack(depths)


def torch_resize(image, size):
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(image.astype(np.float32)).permute(2, 0, 1)[None]
    return torch.round(F.interpolate(x, size, mode='bilinear', align_corners=False))[0].permute(1, 2, 0).numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=71)
    ap.add_argument('--sizes', default='256x320,240x320')
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_dataset.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    ds = importlib.import_module('3dvnet_amd.dataset')
    lib = importlib.import_module('3dvnet_amd._lib')
    try:
        import cv2
    except ImportError:
        cv2 = None
    rng = np.random.default_rng(18)
    n, (H, W) = args.frames, FRAME
    colour = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    depth_mm = rng.integers(300, 9000, size=(n - 2, H, W), dtype=np.uint16)
    depth_mm[:, ::7, ::5] = 65535
    K = np.array([[577.87, 0., 319.5], [0., 577.87, 239.5], [0., 0., 1.]])
    pin_c = torch.from_numpy(colour).pin_memory()
    pin_d = torch.from_numpy(depth_mm.view(np.int16)).pin_memory()
    dev_c, dev_d = pin_c.to(dev), pin_d.to(dev)
    lines = []
    for size in [tuple(int(v) for v in s.split('x')) for s in args.sizes.split(',')]:
        pre = ds.PreprocessImage(K, W, H, size[1], size[0], 0, False)
        linear = [torch.from_numpy(t).to(dev) for t in pre.linear_tables()]
        nearest = [torch.from_numpy(t).to(dev) for t in pre.nearest_tables(DEPTH_SIZE)]
        ys, xs = nearest[0].long(), nearest[1].long()
        images = torch.empty((n, 3) + size, dtype=torch.float32, device=dev)
        depths = torch.empty((n - 2,) + DEPTH_SIZE, dtype=torch.float32, device=dev)

        def kernels(c=dev_c, d=dev_d):
            ds.images_from_frames(c, linear, out=images)
            ds.depths_from_frames(d, nearest, out=depths)

        def with_upload():
            kernels(pin_c.to(dev, non_blocking=True), pin_d.to(dev, non_blocking=True))

        rec = dict(bench='dataset', frames=n, frame_size=[H, W], img_size=list(size), depth_size=list(DEPTH_SIZE), repeats=args.repeats)
        rec['kernels_call_ms'] = timed(kernels, args.warmup, args.repeats)
        lib.timing_enable(True)
        for _ in range(args.repeats):
            kernels()
        spans = lib.timing_collect()
        lib.timing_enable(False)
        rec['kernels_kernel_ms'] = {k: round(v[0] / v[1], 5) for k, v in sorted(spans.items()) if k.startswith('frames_to_')}
        rec['upload_call_ms'] = timed(with_upload, args.warmup, args.repeats)
        rec['torch_device_call_ms'] = timed(lambda: torch_device_route(dev_c, dev_d, pre, size, ys, xs), args.warmup, args.repeats)
        rec['host_torch_call_ms'] = timed(lambda: host_route(colour, depth_mm, pre, size, torch_resize), 1, args.host_repeats)
        if cv2 is not None:
            rec['host_cv2_call_ms'] = timed(lambda: host_route(colour, depth_mm, pre, size, lambda im, s: cv2.resize(
                im, (s[1], s[0]), interpolation=cv2.INTER_LINEAR)), 1, args.host_repeats)
        else:
            rec['host_cv2_call_ms'] = None                                         # OpenCV does not import here: not measured
        moved = colour.nbytes + images.numel() * 4
        rec['byte_model_bytes'] = moved
        rec['byte_model_ms'] = round(moved / HBM_BYTES_PER_S * 1e3, 5)
        rec['byte_model_share'] = round(rec['byte_model_ms'] / rec['kernels_kernel_ms']['frames_to_images'], 4)
        kernels()
        tx, td = torch_device_route(dev_c, dev_d, pre, size, ys, xs)
        hx, hd = host_route(colour, depth_mm, pre, size, torch_resize)
        rec['max_abs_diff_torch_device'] = [float((images - tx).abs().max()), float((depths - td).abs().max())]
        rec['max_abs_diff_host_torch'] = [float((images.cpu() - hx).abs().max()), float((depths.cpu() - hd).abs().max())]
        rec['kernels_faster_than_torch_device'] = rec['kernels_call_ms'][0] < rec['torch_device_call_ms'][0]
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
