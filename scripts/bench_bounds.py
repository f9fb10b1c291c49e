#!/usr/bin/env python3
"""Volume bounds of a scene: the device path (3dvnet_amd/tsdf.py: volume_bounds_device -> v3d_backproject_order_stats_f32, exact
order statistics by radix selection, 52 bytes read back per batch) against the host path (tsdf.volume_bounds with the depths
already on the device: back-projection in stock torch ops, the cloud copied to the host, np.quantile there).

    python scripts/bench_bounds.py [--scenes 64x256x320,100x480x640] [--repeats 10] [--warmup 2] [--out DIR]

Scenes: the ring of synthetic.make_cameras, analytic box-room depths + N(0, 4 cm), 3 % of the pixels zeroed; the reference's
constants (VOL_PRCNT 0.995, VOL_MARGIN 1.5, VOX_RES 0.04, batches of 100 views).

Without --step this is a driver: every GPU step runs as a child process of its own under `timeout`, in sequence, and the
first step that fails ends the run.
  --step device   wall time of volume_bounds_device end to end (enqueue, the one read-back, the host finish), the per-pass kernel
                  times from the library's own event brackets, and the result compared with the NumPy checker
                  (tests/order_stats_oracle.py), which must be identical.
  --step host     wall time of volume_bounds end to end, depths on the device.
One JSON line per scene and step; they land in OUT/bench_bounds.json.  The driver ends with an error when the device path's
median is not below the host path's fastest repeat.
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

KW = dict(vol_prcnt=.995, vol_margin=1.5, vox_res=.04, img_batch=100)


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
    return ms[len(ms) // 2], ms[0], ms[-1]


def step(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_bounds.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    tsdf = importlib.import_module('3dvnet_amd.tsdf')
    lib = importlib.import_module('3dvnet_amd._lib')
    import fusion_oracle as fo
    import order_stats_oracle as oo
    for views, h, w in [tuple(int(v) for v in s.split('x')) for s in args.scenes.split(',')]:
        d, _, poses, K = fo.scene(views, (h, w), seed=1237, yaw_step_deg=None, sigma=0.04)
        dd = d.to(dev)
        n_batches = -(-views // KW['img_batch'])
        base = dict(bench='bounds', step=args.step, views=views, size=[h, w], pixels=views * h * w, batches=n_batches,
                    repeats=args.repeats)
        if args.step == 'device':
            med, lo, hi = timed(lambda: tsdf.volume_bounds_device(dd, K, poses, **KW), args.warmup, args.repeats)
            origin, vol_max, dim = tsdf.volume_bounds_device(dd, K, poses, **KW)
            lib.timing_enable(True)
            for _ in range(args.repeats):
                tsdf.volume_bounds_device(dd, K, poses, **KW)
            spans = lib.timing_collect()
            lib.timing_enable(False)
            passes = {k: round(v[0] / v[1], 4) for k, v in sorted(spans.items()) if k.startswith('order_stats')}
            want = oo.volume_bounds(d.numpy(), K.numpy(), poses.numpy(), **KW)
            same = bool(torch.equal(origin, want[0]) and torch.equal(vol_max, want[1]) and dim == want[2])
            print(json.dumps(dict(base, device_ms=round(med, 4), device_ms_min_max=[round(lo, 4), round(hi, 4)],
                                  pass_kernel_ms=passes, bytes_to_host=n_batches * 13 * 4, origin=origin.tolist(),
                                  vol_max=vol_max.tolist(), vol_dim=dim, identical_to_checker=same)), flush=True)
            if not same:
                sys.exit('bench_bounds.py: the device bounds differ from the checker: %s %s %s against %s %s %s'
                         % (origin.tolist(), vol_max.tolist(), dim, want[0].tolist(), want[1].tolist(), want[2]))
        else:
            med, lo, hi = timed(lambda: tsdf.volume_bounds(dd, K, poses, **KW), min(args.warmup, 1), args.host_repeats)
            origin, vol_max, dim = tsdf.volume_bounds(dd, K, poses, **KW)
            kept = int((d > 0).sum())                                   # rows that survive the NaN drop and cross to the host
            print(json.dumps(dict(base, repeats=args.host_repeats, host_ms=round(med, 3), host_ms_min_max=[round(lo, 3), round(hi, 3)],
                                  bytes_to_host=kept * 12, origin=origin.tolist(), vol_max=vol_max.tolist(), vol_dim=dim)),
                  flush=True)


def driver(args):
    out = args.out or os.path.join(ROOT, 'build', 'bench_bounds')
    os.makedirs(out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), '--scenes', args.scenes, '--repeats', str(args.repeats), '--warmup',
          str(args.warmup), '--host-repeats', str(args.host_repeats)]
    lines = []

    def run(cmd, limit):
        p = subprocess.run(['timeout', '-k', '10', str(limit)] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for ln in p.stdout.splitlines():
            if ln.startswith('{'):
                print(ln, flush=True)
                lines.append(ln)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-4000:])
            sys.exit('bench_bounds.py: `%s` ended with status %d; nothing more is started' % (' '.join(cmd[:6]), p.returncode))

    run(me + ['--step', 'device'], 300)
    run(me + ['--step', 'host'], 420)
    with open(os.path.join(out, 'bench_bounds.json'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    rec = [json.loads(ln) for ln in lines]
    slow = []
    for dv in (r for r in rec if r['step'] == 'device'):
        ho = next(r for r in rec if r['step'] == 'host' and r['views'] == dv['views'] and r['size'] == dv['size'])
        print('%d views of %d x %d: device %.3f ms (median), host %.1f ms (fastest of %d): %.0f x; %d against %d bytes to the host'
              % (dv['views'], dv['size'][0], dv['size'][1], dv['device_ms'], ho['host_ms_min_max'][0], ho['repeats'],
                 ho['host_ms_min_max'][0] / dv['device_ms'], dv['bytes_to_host'], ho['bytes_to_host']), flush=True)
        if not dv['device_ms'] < ho['host_ms_min_max'][0]:
            slow.append(dv['size'])
    if slow:
        sys.exit('bench_bounds.py: the device path is not faster than the host path at %s' % slow)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--scenes', default='64x256x320,100x480x640')
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--step', choices=['device', 'host'])
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.step:
        step(args)
    else:
        driver(args)


if __name__ == '__main__':
    main()
