#!/usr/bin/env python3
"""2D depth metrics on the device (3dvnet_amd/metrics2d.py; csrc/depthmetrics.hip) on the evaluation's own workload: 100 views
of 256 x 320 predictions scored against 480 x 640 sensor depth (seeded: tests/metrics2d_oracle.py's makers), validity derived
from the prediction:

  (a) ``metrics2d.depth_metrics`` with the ground truth as uint16 millimetres;
  (b) the same with the ground truth as float64 metres;
  (c) the stock-torch route on the same GPU: ``F.interpolate(mode='nearest')``, ``pred != 0 & ~isinf(pred)``,
      ``results.depth_metrics_2d`` on the float64 ground truth.

    python scripts/bench_metrics2d.py [--repeats 50] [--warmup 5] [--views 100] [--out DIR]

Without --step this is a driver: the measuring step runs as a child process of its own under `timeout`.  Device events around
each call (median of --repeats, with minimum and maximum), the library's own event brackets around the two kernels, the peak of
``torch.cuda.max_memory_allocated`` above the inputs for (a) and (c), and the agreement of the three.  Bytes are a model from the
shapes: n H W (2 | 8) of ground truth + the predictions once.  The JSON line lands in OUT/bench_metrics2d.json.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

H, W, HP, WP = 480, 640, 256, 320
COLUMNS = ('perc_valid', 'abs_rel', 'abs_diff', 'abs_inv', 'sq_rel', 'rmse', 'd_125', 'd_125_2', 'd_125_3')


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
    return [round(ms[len(ms) // 2], 4), round(ms[0], 4), round(ms[-1], 4)]


def peak_above_inputs(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def step(args):
    import numpy as np
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        sys.exit('bench_metrics2d.py measures on a HIP device; none is visible')
    import metrics2d_oracle as oracle
    dev = torch.device('cuda:0')
    m2d = importlib.import_module('3dvnet_amd.metrics2d')
    results = importlib.import_module('3dvnet_amd.results')
    lib = importlib.import_module('3dvnet_amd._lib')
    n = args.views
    # two views at a time: the maker empties the last two images of a batch of three or more, a scene has no such views
    gt_mm = np.concatenate([oracle.gt_millimetres(min(2, n - s), H, W, 900 + s) for s in range(0, n, 2)])
    pred = torch.from_numpy(oracle.predictions(gt_mm, HP, WP, 901)).to(dev)
    gt16 = torch.from_numpy(gt_mm).to(dev)
    gt64 = torch.from_numpy(gt_mm.astype(np.float64) / 1000.0).to(dev)
    del gt_mm

    def new16():
        return m2d.depth_metrics(pred, gt16, derive_valid=True)

    def new64():
        return m2d.depth_metrics(pred, gt64, derive_valid=True)

    def stock():
        big = F.interpolate(pred.unsqueeze(1), (H, W), mode='nearest').squeeze(1)
        valid = (big != 0.) & (~torch.isinf(big))
        return results.depth_metrics_2d(big, gt64, valid)
    a, b, c = new16(), new64(), stock()
    torch.cuda.synchronize()
    mean_c = np.array([float(c[k]) for k in COLUMNS])
    mean_a = a.mean.cpu().numpy()
    rel = np.abs(mean_a - mean_c) / np.abs(mean_c)
    agree = dict(u16_and_fp64_records_bit_equal=bool(torch.equal(a.counts, b.counts) and torch.equal(a.per_image, b.per_image) and
                                                     torch.equal(a.mean, b.mean)),
                 max_rel_difference_to_stock_fp64_keys=float(rel[[1, 2, 3, 4, 5]].max()),
                 max_rel_difference_to_stock_fp32_keys=float(rel[[0, 6, 7, 8]].max()),
                 abs_rel=float(mean_a[1]), abs_rel_stock=float(mean_c[1]))
    del a, b, c
    peak = {k: peak_above_inputs(f) for k, f in (('new_u16', new16), ('stock', stock))}
    t = {k: timed(f, args.warmup, args.repeats) for k, f in (('new_u16', new16), ('new_fp64', new64), ('stock', stock))}
    spans = {}
    for k, f in (('u16', new16), ('fp64', new64)):
        lib.timing_enable(True)
        for _ in range(args.repeats):
            f()
        got = lib.timing_collect()
        lib.timing_enable(False)
        spans[k] = {name: round(v[0] / args.repeats, 4) for name, v in got.items()}
    npix = n * H * W
    model = {'u16': npix * 2 + n * HP * WP * 4, 'fp64': npix * 8 + n * HP * WP * 4}
    print(json.dumps(dict(bench='metrics2d', views=n, pred=[HP, WP], gt=[H, W], repeats=args.repeats,
                          new_u16_ms_med_min_max=t['new_u16'], new_fp64_ms_med_min_max=t['new_fp64'], stock_ms_med_min_max=t['stock'],
                          kernels_ms_u16=spans['u16'], kernels_ms_fp64=spans['fp64'],
                          stock_over_new_u16=round(t['stock'][0] / t['new_u16'][0], 2),
                          stock_over_new_fp64=round(t['stock'][0] / t['new_fp64'][0], 2),
                          model_bytes_u16=model['u16'], model_bytes_fp64=model['fp64'],
                          model_tb_per_s_u16=round(model['u16'] / spans['u16']['depth_metrics_slices'] / 1e9, 3),
                          model_tb_per_s_fp64=round(model['fp64'] / spans['fp64']['depth_metrics_slices'] / 1e9, 3),
                          pixels_per_ns_u16=round(npix / spans['u16']['depth_metrics_slices'] / 1e6, 2),
                          pixels_per_ns_fp64=round(npix / spans['fp64']['depth_metrics_slices'] / 1e6, 2),
                          peak_bytes_above_inputs_new_u16=peak['new_u16'], peak_bytes_above_inputs_stock=peak['stock'],
                          agreement=agree)), flush=True)


def driver(args):
    out = args.out or os.path.join(ROOT, 'build', 'bench_metrics2d')
    os.makedirs(out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), '--repeats', str(args.repeats), '--warmup', str(args.warmup), '--views',
           str(args.views), '--step', 'hip']
    p = subprocess.run(['timeout', '-k', '10', '300'] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        sys.exit('bench_metrics2d.py: the measuring step ended with status %d' % p.returncode)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    for ln in lines:
        print(ln, flush=True)
    with open(os.path.join(out, 'bench_metrics2d.json'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--views', type=int, default=100)
    ap.add_argument('--step', choices=['hip'])
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.step:
        step(args)
    else:
        driver(args)


if __name__ == '__main__':
    main()
