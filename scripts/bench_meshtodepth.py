#!/usr/bin/env python3
"""Mesh rendering on the device: ``meshtodepth.Renderer.render`` (3dvnet_amd/meshtodepth.py: v3d_mesh_render_depth_f32, one
4-byte read-back) on the mesh of the volume scripts/bench_mesh.py builds -- 64 views of 256 x 320 fused into about 6.0 M voxels
of 4 cm, about 97 k triangles -- rendered back into its own 64 cameras, against the host route: copy mesh and cameras to the
host and render ONE view there with this project's NumPy checker (tests/meshtodepth_oracle.py; pyrender is not available; the
checker is timed on a 64-row image).

    python scripts/bench_meshtodepth.py [--size 256x320] [--views 64] [--repeats 50] [--warmup 5] [--coop N[,N...]] [--out DIR]

Without --step this is a driver: the measuring step runs as a child process of its own under `timeout`.
  --step hip   three workloads, each as milliseconds PER VIEW = the whole ``render`` call (fill, raster, resolve, status
               read-back: wall time by a host clock that ends with the call's own synchronisation, median of --repeats after
               --warmup) / views:
                 a   the mesh into its cameras at --size;
                 a2  the same mesh and cameras at 480 x 640;
                 b   the mesh subdivided to about 2 M triangles, the size of a ScanNet ground-truth mesh (each triangle into
                     four, twice, then as many as it takes into three at their centroids) at --size.
               Per workload also: the share of (view, triangle) pairs whose box goes to the cooperative path (the kernel's box
               rule restated in NumPy for view 0), the share of time in that path (view 0 rendered from the cooperative
               triangles alone and from the others alone), and achieved bytes / s against the byte model below.  With --coop the
               first workloads are timed again at each listed "render_coop" threshold.  The device image of view 0 of workload
               a at 64 x 80 is compared with the checker's fp32 restatement (equal bits) before anything is printed.
Bytes are a model from the shapes, not counters: per view every triangle's three indices (12 F) and nine coordinates (36 F) and
the three image passes (fill 4, resolve 4 read + up to 4 written: 12 h w); atomics are not counted.  The JSON lines land in
OUT/bench_meshtodepth.json.
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


def wall_ms(fn, warmup, repeats):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()                                   # ends with the status read-back: the call synchronises itself
        ms.append(1e3 * (time.perf_counter() - t0))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def subdivide(verts, tris):
    """Each triangle into four (edge midpoints, shared between neighbours) on the device."""
    import torch
    e = torch.cat((tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]), dim=0).long()
    key = torch.minimum(e[:, 0], e[:, 1]) * verts.shape[0] + torch.maximum(e[:, 0], e[:, 1])
    uniq, inv = torch.unique(key, return_inverse=True)
    mid = (verts[uniq // verts.shape[0]] + verts[uniq % verts.shape[0]]) * 0.5
    F = tris.shape[0]
    m = (inv + verts.shape[0]).view(3, F).t().to(torch.int32)             # midpoints of edges 01, 12, 20
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    new = torch.cat((torch.stack((a, m[:, 0], m[:, 2]), 1), torch.stack((b, m[:, 1], m[:, 0]), 1),
                     torch.stack((c, m[:, 2], m[:, 1]), 1), m), dim=0)
    return torch.cat((verts, mid), dim=0).contiguous(), new.contiguous()


def split_at_centroids(verts, tris, count):
    """The first `count` triangles into three each (a new vertex at the centroid: no edge is cut, so no crack opens)."""
    import torch
    count = max(0, min(int(count), int(tris.shape[0])))
    t = tris[:count].long()
    cen = (verts[t[:, 0]] + verts[t[:, 1]] + verts[t[:, 2]]) / 3.0
    c = (torch.arange(count, device=tris.device) + verts.shape[0]).to(torch.int32)
    a, b, d = tris[:count, 0], tris[:count, 1], tris[:count, 2]
    new = torch.cat((torch.stack((a, b, c), 1), torch.stack((b, d, c), 1), torch.stack((d, a, c), 1), tris[count:]), dim=0)
    return torch.cat((verts, cen), dim=0).contiguous(), new.contiguous()


def coop_mask(verts, tris, P, h, w, pc, znear, coop):
    """The kernel's box rule for one view in NumPy -> (live [F] bool, cooperative [F] bool)."""
    import numpy as np
    import meshtodepth_oracle as mo
    pc32 = np.float32(pc)
    with np.errstate(all='ignore'):
        q = [mo.project32(P, verts[tris[:, i]]) for i in range(3)]
        near = np.stack([qi[:, 2] < np.float32(znear) for qi in q], axis=1)
        whole = near.any(axis=1)
        u = np.stack([qi[:, 0] / qi[:, 2] for qi in q], axis=1)
        v = np.stack([qi[:, 1] / qi[:, 2] for qi in q], axis=1)
        x0, x1 = np.floor(u.min(1) - pc32) - 1, np.ceil(u.max(1) - pc32) + 1
        y0, y1 = np.floor(v.min(1) - pc32) - 1, np.ceil(v.max(1) - pc32) + 1
        beside = (x1 < 0) | (y1 < 0) | (x0 > w - 1) | (y0 > h - 1)
        area = (np.clip(x1, 0, w - 1) - np.clip(x0, 0, w - 1) + 1) * (np.clip(y1, 0, h - 1) - np.clip(y0, 0, h - 1) + 1)
    live = ~near.all(axis=1) & (whole | ~beside)
    return live, live & (whole | (area > coop))


def step(args):
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_meshtodepth.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    tsdf = importlib.import_module('3dvnet_amd.tsdf')
    m2d = importlib.import_module('3dvnet_amd.meshtodepth')
    mesh_mod = importlib.import_module('3dvnet_amd.mesh')
    lib = importlib.import_module('3dvnet_amd._lib')
    import fusion_oracle as fo
    import meshtodepth_oracle as mo
    size = tuple(int(v) for v in args.size.split('x'))
    d, img, poses, K = fo.scene(args.views, size, seed=1237, yaw_step_deg=None, sigma=0.04)
    cols = img[..., [2, 1, 0]].permute(0, 3, 1, 2).float().contiguous().to(dev)
    origin, _, dim = tsdf.volume_bounds(d.to(dev), K, poses)
    fus = tsdf.TSDFFusion(dim, 0.04, origin, 3, dev)
    fus.integrate_batch(tsdf.projection_matrices(K, poses).to(dev), d.to(dev), cols)
    mesh = fus.get_tsdf().get_mesh()
    K, poses = torch.as_tensor(K).float(), torch.as_tensor(poses).float()
    default = lib.set_option('render_coop', 0)
    lib.set_option('render_coop', default)

    # equality with the checker on a small image before any figure
    Ks = K[:1].clone()
    Ks[:, :2] *= 64.0 / size[0]
    small = m2d.Renderer(mesh, 64, int(round(size[1] * 64.0 / size[0]))).render(Ks, poses[:1])
    vh, fh = mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy()
    t0 = time.perf_counter()
    want = mo.render32(vh, fh, tsdf.projection_matrices(Ks, poses[:1]).numpy(), small.shape[1], small.shape[2])
    checker_small_s = time.perf_counter() - t0
    if not np.array_equal(small.cpu().numpy().view(np.uint32), want.view(np.uint32)):
        sys.exit('bench_meshtodepth.py: the device image differs from the checker\'s; no figure is reported')

    big_v, big_f = subdivide(*subdivide(mesh.vertices, mesh.triangles))
    big_v, big_f = split_at_centroids(big_v, big_f, (2000000 - int(big_f.shape[0])) // 2)
    K2 = K.clone()
    K2[:, 0] *= 640.0 / size[1]
    K2[:, 1] *= 480.0 / size[0]
    loads = [('a', mesh.vertices, mesh.triangles, K, size), ('a2', mesh.vertices, mesh.triangles, K2, (480, 640)),
             ('b', big_v, big_f, K, size)]
    for name, v, f, Kw, (h, w) in loads:
        holder = mesh_mod.TriangleMesh(v, f)
        r = m2d.Renderer(holder, h, w)
        P = tsdf.projection_matrices(Kw, poses)
        n, F = int(P.shape[0]), int(f.shape[0])
        med, lo, hi = wall_ms(lambda: r.render_projections(P), args.warmup, args.repeats)
        vh, fh = v.cpu().numpy(), f.cpu().numpy()
        live, coop = coop_mask(vh, fh, P[0].numpy(), h, w, .5, .05, default)
        parts = {}
        for tag, sel in (('coop', coop), ('own', live & ~coop)):
            if sel.any():
                rp = m2d.Renderer(mesh_mod.TriangleMesh(v, f[torch.from_numpy(sel).to(dev)].contiguous()), h, w)
                parts[tag] = wall_ms(lambda: rp.render_projections(P[:1]), args.warmup, args.repeats)[0]
            else:
                parts[tag] = 0.0
        empty = m2d.Renderer(mesh_mod.TriangleMesh(v, f[:1].contiguous()), h, w)
        floor_ms = wall_ms(lambda: empty.render_projections(P[:1]), args.warmup, args.repeats)[0]     # launches + read-back
        t_coop, t_own = max(parts['coop'] - floor_ms, 0.0), max(parts['own'] - floor_ms, 0.0)
        model = n * (48 * F + 12 * h * w)
        rec = dict(bench='meshtodepth', workload=name, views=n, size=[h, w], vertices=int(v.shape[0]), triangles=F,
                   render_coop=default, ms_per_view=round(med / n, 5), call_ms=round(med, 4), call_ms_min_max=[round(lo, 4), round(hi, 4)],
                   coop_share_of_live_triangles_view0=round(float(coop.sum()) / max(int(live.sum()), 1), 4),
                   live_share_of_triangles_view0=round(float(live.mean()), 4),
                   coop_share_of_time_view0=round(t_coop / (t_coop + t_own), 3) if t_coop + t_own > 0 else None,
                   one_view_call_floor_ms=round(floor_ms, 4), model_bytes=model, model_gb_per_s=round(model / med / 1e6, 1),
                   equal_to_checker=True, repeats=args.repeats)
        if name == 'a':
            # the host route: mesh and cameras to the host, one view by the checker.  The checker tests every triangle at every
            # pixel, so it is timed at 64 rows (the image compared above) and that time is scaled by the
            # pixel ratio for the comparison at the workload's size
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh.vertices.cpu().numpy(), mesh.triangles.cpu().numpy(), P[:1].cpu().numpy()
            t1 = time.perf_counter()
            scale = float(h * w) / float(small.shape[1] * small.shape[2])
            rec.update(host_copy_ms=round(1e3 * (t1 - t0), 2), host_checker_one_view_ms=round(1e3 * checker_small_s, 1),
                       host_checker_size=[int(small.shape[1]), int(small.shape[2])],
                       host_checker_one_view_ms_scaled_to_size=round(1e3 * checker_small_s * scale, 0),
                       host_route_over_device_per_view=round(1e3 * (t1 - t0 + checker_small_s * scale) / (med / n), 0))
        print(json.dumps(rec), flush=True)
        for value in [int(x) for x in args.coop.split(',') if x] if name in ('a', 'a2') else []:
            lib.set_option('render_coop', value)
            try:
                m = wall_ms(lambda: r.render_projections(P), args.warmup, args.repeats)[0]
            finally:
                lib.set_option('render_coop', default)
            print(json.dumps(dict(bench='meshtodepth', workload=name, render_coop=value, ms_per_view=round(m / n, 5))), flush=True)


def driver(args):
    out = args.out or os.path.join(ROOT, 'build', 'bench_meshtodepth')
    os.makedirs(out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), '--size', args.size, '--views', str(args.views), '--repeats', str(args.repeats),
           '--warmup', str(args.warmup), '--coop', args.coop, '--step', 'hip']
    p = subprocess.run(['timeout', '-k', '10', '400'] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        sys.exit('bench_meshtodepth.py: the measuring step ended with status %d' % p.returncode)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    for ln in lines:
        print(ln, flush=True)
    with open(os.path.join(out, 'bench_meshtodepth.json'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='256x320')
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--coop', default='', help='further render_coop thresholds to time workloads a and a2 at')
    ap.add_argument('--step', choices=['hip'])
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.step:
        step(args)
    else:
        driver(args)


if __name__ == '__main__':
    main()
