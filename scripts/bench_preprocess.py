#!/usr/bin/env python3
"""Scene preparation on the device (3dvnet_amd/preprocess.py, csrc/prepare.hip): the colour registration against the same
resampling by F.grid_sample on the device and against the reference's per-frame route on the host, and the ground-truth mesh of a
synthetic scene end to end against the per-view stock-torch integration that scripts/bench_tsdf.py has as its comparator.  One
process, every shape warmed, medians.

    python scripts/bench_preprocess.py [--frames 71] [--views 200] [--vox-res 0.02] [--repeats 30] [--warmup 3] [--host-repeats 3]
                                       [--mesh-repeats 3] [--skip-mesh] [--out FILE]

One JSON line per part.
  register   `--frames` colour frames of 968 x 1296 -> 480 x 640 through a ScanNet intrinsics pair:
               kernel_ms          v3d_register_colour_u8 alone (the library's event brackets, mean of `repeats` launches)
               call_ms            register_colour on device-resident frames (host clock between two synchronisations; median, min, max)
               grid_sample_ms     the same pixels by stock torch on the device: the float image, the warp grid, F.grid_sample(nearest),
                                  the cast back -- in chunks of 8 frames (the float copy of 71 frames is 1 GB)
               host_ms            the reference's route: one frame at a time on the host, F.grid_sample on the CPU
               byte_model_*       the bytes the kernel must move at least (the output written once, each sampled source pixel read
                                  once) at 6.3 TB/s, and the share of that rate the kernel reaches
               equal_*            whether the three routes give the same bytes
  gt_mesh    gt_mesh_from_frames on `--views` synthetic frames of 480 x 640 (ring cameras in the box room) at `--vox-res`:
               total_s and the stages upload / bounds / fusion / mesh (host clock, each closed by a synchronisation), for
               bounds='host' and bounds='device'; torch_fusion_s: the fusion stage alone by whole-volume torch ops, one view after the
               other (bench_tsdf.torch_tsdf) on the same volume and inputs
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
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

HBM_BYTES_PER_S = 6.3e12          # achievable HBM bandwidth of an MI355X
K_COLOR = np.array([[1165.723022, 0., 649.094971], [0., 1165.738037, 484.765015], [0., 0., 1.]])
K_DEPTH = np.array([[574.540771, 0., 322.522827], [0., 577.583740, 238.558853], [0., 0., 1.]])
COLOUR_SIZE, DEPTH_SIZE = (968, 1296), (480, 640)


def timed(fn, warmup, repeats):
    """Wall-clock milliseconds of fn() between two device synchronisations -> [median, min, max]."""
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


def warp_grid(H, colour_size, depth_size, device):
    """The normalised sampling grid [1, h, w, 2] of the registration in stock torch ops (the reference's normalisers)."""
    import torch
    Hc, Wc = colour_size
    h, w = depth_size
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float32, device=device), torch.arange(w, dtype=torch.float32, device=device),
                            indexing='ij')
    pix = torch.stack((xs, ys, torch.ones_like(xs)), dim=0).reshape(3, -1)
    warped = torch.as_tensor(H, device=device) @ pix
    uv = warped[:2] / (warped[2:] + 1e-8)
    gx = (uv[0] - Wc / 2.0) / (Wc / 2.0)
    gy = (uv[1] - Hc / 2.0) / (Hc / 2.0)
    return torch.stack((gx, gy), dim=-1).reshape(1, h, w, 2)


def grid_sample_route(frames, H, depth_size, chunk):
    """uint8 [n, Hc, Wc, 3] on any device -> uint8 [n, h, w, 3] by F.grid_sample, `chunk` frames at a time."""
    import torch
    import torch.nn.functional as F
    grid = warp_grid(H, frames.shape[1:3], depth_size, frames.device)
    out = []
    for i in range(0, frames.shape[0], chunk):
        x = frames[i:i + chunk].permute(0, 3, 1, 2).float()
        y = F.grid_sample(x, grid.expand(x.shape[0], -1, -1, -1), mode='nearest', padding_mode='zeros', align_corners=True)
        out.append(y.to(torch.uint8).permute(0, 2, 3, 1))
    return torch.cat(out).contiguous()


def bench_register(args, dev):
    import torch
    pre = importlib.import_module('3dvnet_amd.preprocess')
    lib = importlib.import_module('3dvnet_amd._lib')
    n = args.frames
    colour = np.random.default_rng(23).integers(0, 256, size=(n,) + COLOUR_SIZE + (3,), dtype=np.uint8)
    dev_c = torch.from_numpy(colour).to(dev)
    out = torch.empty((n,) + DEPTH_SIZE + (3,), dtype=torch.uint8, device=dev)
    H = pre.colour_to_depth_homography(K_COLOR, K_DEPTH)

    def kernel():
        pre.register_colour(dev_c, DEPTH_SIZE, K_COLOR, K_DEPTH, out=out)

    rec = dict(bench='preprocess', part='register', frames=n, colour_size=list(COLOUR_SIZE), depth_size=list(DEPTH_SIZE), repeats=args.repeats)
    rec['call_ms'] = timed(kernel, args.warmup, args.repeats)
    lib.timing_enable(True)
    for _ in range(args.repeats):
        kernel()
    spans = lib.timing_collect()
    lib.timing_enable(False)
    rec['kernel_ms'] = round(spans['register_colour'][0] / spans['register_colour'][1], 5)
    rec['grid_sample_ms'] = timed(lambda: grid_sample_route(dev_c, H, DEPTH_SIZE, 8), args.warmup, args.repeats)
    rec['host_ms'] = timed(lambda: [grid_sample_route(torch.from_numpy(colour[i:i + 1]), H, DEPTH_SIZE, 1) for i in range(n)], 0, args.host_repeats)
    moved = 2 * out.numel()                                                        # every output byte written, its source byte read
    rec['byte_model_bytes'] = moved
    rec['byte_model_ms'] = round(moved / HBM_BYTES_PER_S * 1e3, 5)
    rec['byte_model_share'] = round(rec['byte_model_ms'] / rec['kernel_ms'], 4)
    kernel()
    rec['equal_grid_sample_device'] = bool(torch.equal(out, grid_sample_route(dev_c, H, DEPTH_SIZE, 8)))
    rec['pixels_differing_from_grid_sample_device'] = int((out != grid_sample_route(dev_c, H, DEPTH_SIZE, 8)).any(dim=-1).sum())
    host = torch.cat([grid_sample_route(torch.from_numpy(colour[i:i + 1]), H, DEPTH_SIZE, 1) for i in range(min(n, 4))])
    rec['equal_host_first_frames'] = bool(torch.equal(out[:host.shape[0]].cpu(), host))
    rec['kernel_faster_than_grid_sample'] = rec['call_ms'][0] < rec['grid_sample_ms'][0]
    return rec


def bench_gt_mesh(args, dev):
    import torch
    import fusion_oracle as fo
    from bench_tsdf import torch_tsdf
    pre = importlib.import_module('3dvnet_amd.preprocess')
    tsdf = importlib.import_module('3dvnet_amd.tsdf')
    ds = importlib.import_module('3dvnet_amd.dataset')
    n, size = args.views, DEPTH_SIZE
    d, img, w2c, K = fo.scene(n, size, seed=1237, yaw_step_deg=None, sigma=0.01)
    colour = img.numpy()
    depth_mm = np.clip(np.rint(d.numpy().astype(np.float64) * 1000.0), 0, 65535).astype(np.uint16)
    poses = np.linalg.inv(w2c.numpy().astype(np.float64))
    K0 = K[0].numpy().astype(np.float64)
    rec = dict(bench='preprocess', part='gt_mesh', views=n, size=list(size), vox_res=args.vox_res, img_batch=20, repeats=args.mesh_repeats)
    for bounds in ('host', 'device'):
        runs = []
        for _ in range(args.mesh_repeats + 1):                                     # the first run warms every shape
            stages = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh = pre.gt_mesh_from_frames(colour, depth_mm, K0, poses, vox_res=args.vox_res, bounds=bounds, device=dev, stages=stages)
            torch.cuda.synchronize()
            stages['total'] = time.perf_counter() - t0
            runs.append(stages)
        runs = runs[1:]
        med = {k: round(sorted(r[k] for r in runs)[len(runs) // 2], 4) for k in ('total', 'upload', 'bounds', 'fusion', 'mesh')}
        rec['bounds_%s_s' % bounds] = med
        rec['voxel_dim'] = runs[0]['voxel_dim']
        rec['vertices'], rec['triangles'] = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
        del mesh
    # the comparator of the fusion stage: the same volume and inputs, whole-volume torch ops per view
    geo = ds.scene_geometry(K0, poses, np.arange(n), size, size, False, 0)
    pose32 = torch.eye(4).repeat(n, 1, 1)
    pose32[:, :3, :3], pose32[:, :3, 3] = geo['rotmats'], geo['tvecs']
    depths = torch.from_numpy(depth_mm.astype(np.float32) / np.float32(1000.)).to(dev)
    origin, _, dim = tsdf.volume_bounds_device(depths, geo['K'], pose32, vox_res=args.vox_res, img_batch=20)
    P = tsdf.projection_matrices(geo['K'].contiguous(), pose32).to(dev)
    cols = torch.from_numpy(colour).to(dev).permute(0, 3, 1, 2).float().contiguous()
    org, tm = [float(v) for v in origin], float(torch.tensor(args.vox_res * 3, dtype=torch.float32))
    runs = []
    for _ in range(2):                                                             # the first run warms the allocator
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_tsdf(dim, args.vox_res, org, tm, P, depths, cols)
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    rec['torch_fusion_s'] = round(runs[-1], 4)
    rec['torch_fusion_voxel_dim'] = dim
    rec['fusion_faster_than_torch'] = rec['bounds_device_s']['fusion'] < rec['torch_fusion_s']
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=71)
    ap.add_argument('--views', type=int, default=200)
    ap.add_argument('--vox-res', type=float, default=0.02)
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--mesh-repeats', type=int, default=3)
    ap.add_argument('--skip-mesh', action='store_true')
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_preprocess.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    lines = []
    for part in [bench_register] + ([] if args.skip_mesh else [bench_gt_mesh]):
        line = json.dumps(part(args, dev))
        print(line, flush=True)
        lines.append(line)
        if args.out:                                                               # after every part: a later part's failure loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
