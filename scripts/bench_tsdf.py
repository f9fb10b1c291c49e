#!/usr/bin/env python3
"""TSDF integration on the device: the HIP path (3dvnet_amd/tsdf.py: v3d_tsdf_integrate_f32, one launch for all views) against
the same algorithm in stock torch ops on the same GPU -- what a user has today -- and the profiler passes of the kernel.

    python scripts/bench_tsdf.py [--size 256x320,480x640] [--views 64] [--repeats 20] [--warmup 3] [--out DIR] [--rocprof]

Scenes: the 64-view ring of synthetic.make_cameras, analytic box-room depths + N(0, 4 cm), 3 % of the pixels zeroed, blocky
colours; the volume from tsdf.volume_bounds with the reference's constants (VOX_RES 0.04, VOL_MARGIN 1.5, VOL_PRCNT 0.995).

Without --step this is a driver: every GPU step runs as a child process of its own under `timeout`, in sequence, and the
first step that fails ends the run.
  --step hip      HIP events around integrate_batch (all views, one launch) and, with the library's own event brackets, around
                  tsdf_integrate_kernel alone; get_tsdf() separately.  One JSON line per size.
  --step torch    the same per-voxel algorithm as whole-volume torch ops, one view after the other (written for this script;
                  masks by torch.where, so without the boolean-index writes that synchronise the reference's version).
  --step profile  a few un-timed HIP launches per size (the program rocprofv3 runs).
--rocprof adds two profiler passes over `--step profile`: `rocprofv3 --kernel-trace --stats` and, as a run of its own,
`rocprofv3 --pmc ...` (SQ counters; a pass with the FETCH_SIZE / WRITE_SIZE traffic counters aborted inside the profiler on
the one attempt made and is not part of the script); their tables are reduced to OUT/kernel_stats_tsdf.csv and
OUT/pmc_tsdf.csv.  The JSON lines land in OUT/bench_tsdf.json.
"""
import argparse
import csv
import glob
import importlib
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PMC = ['SQ_WAVES', 'SQ_INSTS_VALU', 'SQ_INSTS_SALU', 'SQ_INSTS_VMEM_RD', 'SQ_BUSY_CYCLES', 'SQ_WAIT_INST_ANY', 'SQ_ACTIVE_INST_VALU']


def torch_tsdf(dim, voxel_size, origin, trunc_margin, P, depths, colors):
    """TSDF integration in stock torch ops on the device (written for this script): the world grid once, then per view a
    handful of whole-volume elementwise ops and two gathers.  -> (tsdf sum, weight, colour sums)."""
    import torch
    dev = depths.device
    nx, ny, nz = dim
    ax = [torch.arange(n, device=dev, dtype=torch.float32) * voxel_size + origin[a] for a, n in enumerate(dim)]
    X, Y, Z = (t.reshape(-1) for t in torch.meshgrid(*ax, indexing='ij'))
    world = torch.stack((X, Y, Z, torch.ones_like(X)), 0)
    n, h, w = depths.shape
    tsdf = -torch.ones(nx * ny * nz, device=dev)
    weight = torch.zeros(nx * ny * nz, device=dev)
    color = torch.zeros((3, nx * ny * nz), device=dev)
    for k in range(n):
        cam = P[k] @ world
        pz = cam[2]
        px, py = (cam[0] / pz).round(), (cam[1] / pz).round()
        valid = (px >= 0) & (py >= 0) & (px < w) & (py < h) & (pz > 0)
        idx = (py.clamp(0, h - 1) * w + px.clamp(0, w - 1)).long()
        idx = torch.where(valid, idx, torch.zeros_like(idx))
        d = depths[k].reshape(-1)[idx]
        dist = ((d - pz) / trunc_margin).clamp(max=1)
        valid = valid & (d > 0) & (dist > -1)
        tsdf = torch.where(valid, torch.where(weight == 0, dist, tsdf + dist), tsdf)
        weight = weight + valid
        color = color + torch.where(valid[None], colors[k].reshape(3, -1)[:, idx], torch.zeros((), device=dev))
    return tsdf, weight, color


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
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_tsdf.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    tsdf = importlib.import_module('3dvnet_amd.tsdf')
    lib = importlib.import_module('3dvnet_amd._lib')
    import fusion_oracle as fo
    for size in [tuple(int(v) for v in s.split('x')) for s in args.size.split(',')]:
        d, img, poses, K = fo.scene(args.views, size, seed=1237, yaw_step_deg=None, sigma=0.04)
        cols = img[..., [2, 1, 0]].permute(0, 3, 1, 2).float().contiguous().to(dev)
        d = d.to(dev)
        origin, _, dim = tsdf.volume_bounds(d, K, poses)
        P = tsdf.projection_matrices(K, poses).to(dev)
        fus = tsdf.TSDFFusion(dim, 0.04, origin, 3, dev)
        n_vox = dim[0] * dim[1] * dim[2]

        def hip():
            fus.integrate_batch(P, d, cols)

        if args.step == 'profile':
            for _ in range(5):
                hip()
            torch.cuda.synchronize()
            continue
        base = dict(bench='tsdf', step=args.step, views=args.views, size=list(size), voxel_dim=dim, voxels=n_vox)
        if args.step == 'hip':
            hip_ms = timed(hip, args.warmup, args.repeats)
            norm_ms = timed(fus.get_tsdf, args.warmup, args.repeats)
            lib.timing_enable(True)
            for _ in range(args.repeats):
                hip()
            spans = lib.timing_collect()
            lib.timing_enable(False)
            kern_ms = spans['tsdf_integrate'][0] / spans['tsdf_integrate'][1]
            fresh = tsdf.TSDFFusion(dim, 0.04, origin, 3, dev)
            fresh.integrate_batch(P, d, cols)
            torch.cuda.synchronize()
            print(json.dumps(dict(base, hip_call_ms=round(hip_ms[0], 4), hip_call_ms_min_max=[round(hip_ms[1], 4), round(hip_ms[2], 4)],
                                  tsdf_integrate_kernel_ms=round(kern_ms, 4), get_tsdf_ms=round(norm_ms[0], 4),
                                  gpairs_per_s=round(n_vox * args.views / kern_ms / 1e6, 2),
                                  volume_bytes_per_launch=40 * n_vox, volume_gb_per_s=round(40 * n_vox / kern_ms / 1e6, 1),
                                  touched_voxels=int((fresh.weight_vol > 0).sum()), weight_sum=float(fresh.weight_vol.sum()),
                                  repeats=args.repeats)), flush=True)
        else:
            org = [float(v) for v in origin]
            tm = float(torch.tensor(0.04 * 3, dtype=torch.float32))
            tor_ms = timed(lambda: torch_tsdf(dim, 0.04, org, tm, P, d, cols), 1, args.torch_repeats)
            t, wt, c = torch_tsdf(dim, 0.04, org, tm, P, d, cols)
            fresh = tsdf.TSDFFusion(dim, 0.04, origin, 3, dev)
            fresh.integrate_batch(P, d, cols)
            torch.cuda.synchronize()
            print(json.dumps(dict(base, torch_ms=round(tor_ms[0], 3), torch_ms_min_max=[round(tor_ms[1], 3), round(tor_ms[2], 3)],
                                  torch_repeats=args.torch_repeats, weights_differing_from_hip=int((wt != fresh.weight_vol).sum()),
                                  max_tsdf_difference_where_weights_agree=float(
                                      (t - fresh.tsdf_vol).abs()[wt == fresh.weight_vol].max()))), flush=True)


def reduce_tables(tmp, out):
    """rocprofv3's tables -> two small CSVs (kernel statistics as they are; counters as means per launch and kernel)."""
    stats = sorted(glob.glob(os.path.join(tmp, 'kt', '**', '*kernel_stats.csv'), recursive=True))
    if stats:
        shutil.copy(stats[0], os.path.join(out, 'kernel_stats_tsdf.csv'))
    acc = {}
    for name in ('pmc',):
        for path in glob.glob(os.path.join(tmp, name, '**', '*counter_collection.csv'), recursive=True):
            for row in csv.DictReader(open(path)):
                key = (row.get('Kernel_Name', '')[:80], row.get('Counter_Name', ''))
                s = acc.setdefault(key, [0.0, set()])
                s[0] += float(row.get('Counter_Value', 0) or 0)
                s[1].add(row.get('Dispatch_Id', ''))
    if acc:
        with open(os.path.join(out, 'pmc_tsdf.csv'), 'w', newline='') as f:
            wr = csv.writer(f)
            wr.writerow(['kernel', 'counter', 'launches', 'mean_per_launch'])
            for (kern, ctr), (total, ids) in sorted(acc.items()):
                wr.writerow([kern, ctr, len(ids), '%.6g' % (total / max(1, len(ids)))])


def driver(args):
    out = args.out or os.path.join(ROOT, 'build', 'bench_tsdf')
    os.makedirs(out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), '--size', args.size, '--views', str(args.views), '--repeats',
          str(args.repeats), '--warmup', str(args.warmup), '--torch-repeats', str(args.torch_repeats)]
    lines = []

    def run(cmd, limit, keep=False):
        p = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-4000:])
            sys.exit('bench_tsdf.py: `%s` ended with status %d; nothing more is started' % (' '.join(cmd[:6]), p.returncode))
        if keep:
            for ln in p.stdout.splitlines():
                if ln.startswith('{'):
                    print(ln, flush=True)
                    lines.append(ln)

    run(me + ['--step', 'hip'], 300, keep=True)
    run(me + ['--step', 'torch'], 420, keep=True)
    with open(os.path.join(out, 'bench_tsdf.json'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    if args.rocprof:
        tmp = tempfile.mkdtemp(prefix='bench_tsdf_')
        prof = me + ['--step', 'profile']
        run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', os.path.join(tmp, 'kt'), '-o', 'r', '--'] + prof, 300)
        reduce_tables(tmp, out)
        small = prof[:3] + [args.size.split(',')[0]] + prof[4:]
        run(['rocprofv3', '--pmc'] + PMC + ['--output-format', 'csv', '-d', os.path.join(tmp, 'pmc'), '-o', 'r', '--'] + small, 300)
        reduce_tables(tmp, out)
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='256x320,480x640')
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-repeats', type=int, default=5)
    ap.add_argument('--step', choices=['hip', 'torch', 'profile'])
    ap.add_argument('--out')
    ap.add_argument('--rocprof', action='store_true')
    args = ap.parse_args()
    if args.step:
        step(args)
    else:
        driver(args)


if __name__ == '__main__':
    main()
