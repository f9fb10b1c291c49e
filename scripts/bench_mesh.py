#!/usr/bin/env python3
"""Mesh extraction on the device: ``TSDF.get_mesh`` (3dvnet_amd/mesh.py: v3d_mesh_count_f32 + v3d_mesh_extract_f32, one 8-byte
read-back between them) on the volume scripts/bench_tsdf.py builds -- 64 views of 256 x 320 integrated into about 6.0 M voxels
of 4 cm -- against the host route the reference takes: copy the volume and its colours to the host, then mesh there.  The host
mesher is this project's NumPy checker (tests/mesh_oracle.py; skimage is not available), which computes the same arrays.

    python scripts/bench_mesh.py [--size 256x320] [--views 64] [--repeats 50] [--warmup 5] [--host-repeats 3] [--out DIR]

Without --step this is a driver: the measuring step runs as a child process of its own under `timeout`.
  --step hip   device events around get_mesh (count + read-back + extract) and, with the library's own event brackets, around
               the two C calls; then the host route by a host clock that ends in a synchronise: volume + colour copy, checker.
               The device mesh is compared with the checker's (equal arrays) before anything is printed.  One JSON line.
Bytes are a model computed from the shapes (n = voxels, V = vertices, F = triangles), not counters: the passes read 19 n
(volume twice, the status / count bytes and the two offset arrays) and write 10 n (two byte arrays, two offset arrays) plus
15 V + 12 F of output.  The JSON line lands in OUT/bench_mesh.json.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(fn, warmup, repeats):
    import torch
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


def step(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_mesh.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    tsdf = importlib.import_module('3dvnet_amd.tsdf')
    lib = importlib.import_module('3dvnet_amd._lib')
    import fusion_oracle as fo
    import mesh_oracle as mo
    size = tuple(int(v) for v in args.size.split('x'))
    d, img, poses, K = fo.scene(args.views, size, seed=1237, yaw_step_deg=None, sigma=0.04)
    cols = img[..., [2, 1, 0]].permute(0, 3, 1, 2).float().contiguous().to(dev)
    d = d.to(dev)
    origin, _, dim = tsdf.volume_bounds(d, K, poses)
    fus = tsdf.TSDFFusion(dim, 0.04, origin, 3, dev)
    fus.integrate_batch(tsdf.projection_matrices(K, poses).to(dev), d, cols)
    vol = fus.get_tsdf()
    n_vox = dim[0] * dim[1] * dim[2]

    mesh = vol.get_mesh()
    torch.cuda.synchronize()
    n_v, n_f = int(mesh.vertices.shape[0]), int(mesh.triangles.shape[0])
    hip_ms = timed(vol.get_mesh, args.warmup, args.repeats)
    lib.timing_enable(True)
    for _ in range(args.repeats):
        vol.get_mesh()
    spans = lib.timing_collect()
    lib.timing_enable(False)
    count_ms = spans['mesh_count'][0] / spans['mesh_count'][1]
    extract_ms = spans['mesh_extract'][0] / spans['mesh_extract'][1]

    copy_s, host_s = [], []
    for _ in range(args.host_repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tv, cv = vol.tsdf_vol.cpu().numpy(), vol.attribute_vols['color'].cpu().numpy()
        t1 = time.perf_counter()
        want = mo.get_mesh(tv, cv, vol.voxel_size, vol.origin.cpu().numpy())
        t2 = time.perf_counter()
        copy_s.append(t1 - t0)
        host_s.append(t2 - t1)
    same = (np.array_equal(mesh.vertices.cpu().numpy().view(np.uint32), want['vertices'].view(np.uint32))
            and np.array_equal(mesh.triangles.cpu().numpy(), want['triangles'])
            and np.array_equal(mesh.vertex_colors_u8.cpu().numpy(), want['colors']))
    if not same:
        sys.exit('bench_mesh.py: the device mesh differs from the checker\'s; no figure is reported')
    read_b, write_b = 19 * n_vox, 10 * n_vox + 15 * n_v + 12 * n_f
    kern_ms = count_ms + extract_ms
    print(json.dumps(dict(bench='mesh', views=args.views, size=list(size), voxel_dim=dim, voxels=n_vox, vertices=n_v, triangles=n_f,
                          vertices_before_removal=int(want['n_all']),
                          get_mesh_ms=round(hip_ms[0], 4), get_mesh_ms_min_max=[round(hip_ms[1], 4), round(hip_ms[2], 4)],
                          mesh_count_ms=round(count_ms, 4), mesh_extract_ms=round(extract_ms, 4),
                          model_bytes_read=read_b, model_bytes_written=write_b,
                          model_gb_per_s=round((read_b + write_b) / kern_ms / 1e6, 1),
                          host_copy_ms=round(1e3 * min(copy_s), 2), host_checker_ms=round(1e3 * min(host_s), 2),
                          host_route_ms=round(1e3 * min(c + h for c, h in zip(copy_s, host_s)), 2),
                          host_route_over_get_mesh=round(1e3 * min(c + h for c, h in zip(copy_s, host_s)) / hip_ms[0], 1),
                          equal_to_checker=True, repeats=args.repeats, host_repeats=args.host_repeats)), flush=True)


def driver(args):
    out = args.out or os.path.join(ROOT, 'build', 'bench_mesh')
    os.makedirs(out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), '--size', args.size, '--views', str(args.views), '--repeats', str(args.repeats),
           '--warmup', str(args.warmup), '--host-repeats', str(args.host_repeats), '--step', 'hip']
    p = subprocess.run(['timeout', '-k', '10', '400'] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        sys.exit('bench_mesh.py: the measuring step ended with status %d' % p.returncode)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    for ln in lines:
        print(ln, flush=True)
    with open(os.path.join(out, 'bench_mesh.json'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='256x320')
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--step', choices=['hip'])
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.step:
        step(args)
    else:
        driver(args)


if __name__ == '__main__':
    main()
