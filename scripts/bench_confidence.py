#!/usr/bin/env python3
"""Photometric confidence maps on the device (3dvnet_amd/utils.py: soft_argmin / get_propability_map; csrc/confidence.hip) on
random logits of the cfg2 shape (64 views x 96 planes x 56 x 56) and the cfg5 shape (8 views x 192 planes x 120 x 160):

  (a) today's soft-argmin kernel alone (``utils.soft_argmin``: soft_argmin_kernel, the last launch of ``regularize_depth``);
  (b) the fused depth + confidence kernel (``utils.soft_argmin(return_prob=True)``: soft_argmin_prob_kernel);
  (c) the stock-torch route on the device: ``softmax(-x_reg, dim=1)``, the expectation as the reference writes it, and the
      reference's five-index gather (``stock_route`` below, restated from the description of get_propability_map).

    python scripts/bench_confidence.py [--repeats 50] [--warmup 5] [--out DIR]

Without --step this is a driver: the measuring step runs as a child process of its own under `timeout`.  Per shape: device
events around each call (median of --repeats, with minimum and maximum), the library's own event brackets around the two
kernels, and the agreement of (b) with (c).  Bytes are a model from the shapes: D loads per pixel for (a); D + 2 loads and one
more 4-byte store per pixel for (b).  The JSON lines land in OUT/bench_confidence.json.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {'cfg2': (64, 96, 56, 56, 0.5, 0.05), 'cfg5': (8, 192, 120, 160, 0.5, 0.025)}


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


def stock_route(x_reg, vals, depth_start, depth_interval):
    """softmax, expectation and the gather with stock torch ops -> (depth, prob)."""
    import torch
    n, D, h, w = x_reg.shape
    p = torch.softmax(-x_reg, dim=1)
    depth = torch.sum(vals.view(1, D, 1, 1).expand(p.shape) * p, dim=1)
    dev = x_reg.device
    b = torch.arange(n, device=dev).view(n, 1, 1).expand(n, h, w).reshape(-1)
    y = torch.arange(h, device=dev).view(1, h, 1).expand(n, h, w).reshape(-1)
    x = torch.arange(w, device=dev).view(1, 1, w).expand(n, h, w).reshape(-1)
    d = ((depth - depth_start) / depth_interval).view(-1)
    left = torch.clamp(d.floor().long(), 0, D - 1)
    right = torch.clamp(d.ceil().long(), 0, D - 1)
    return depth, (p[b, left, y, x] + p[b, right, y, x]).view(n, h, w)


def step(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_confidence.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    utils = importlib.import_module('3dvnet_amd.utils')
    lib = importlib.import_module('3dvnet_amd._lib')
    for name, (n, D, h, w, ds, di) in SHAPES.items():
        x = torch.randn((n, D, h, w), generator=torch.Generator().manual_seed(1)).to(dev)
        vals = torch.linspace(ds, ds + di * (D - 1), D).to(dev)

        def plain():
            return utils.soft_argmin(x, vals)

        def fused():
            return utils.soft_argmin(x, vals, return_prob=True, depth_start=ds, depth_interval=di)

        def stock():
            return stock_route(x, vals, ds, di)
        depth_a = plain()
        depth_b, prob_b = fused()
        depth_c, prob_c = stock()
        torch.cuda.synchronize()
        same_planes = (prob_b - prob_c).abs() <= 1e-5          # elsewhere the stock depth's last bits chose another plane
        t = {k: timed(f, args.warmup, args.repeats) for k, f in (('plain', plain), ('fused', fused), ('stock', stock))}
        lib.timing_enable(True)
        for _ in range(args.repeats):
            plain()
            fused()
        spans = lib.timing_collect()
        lib.timing_enable(False)
        npix = n * h * w
        print(json.dumps(dict(bench='confidence', shape=name, n=n, D=D, h=h, w=w, pixels=npix,
                              soft_argmin_ms=round(t['plain'][0], 4), soft_argmin_ms_min_max=[round(v, 4) for v in t['plain'][1:]],
                              fused_ms=round(t['fused'][0], 4), fused_ms_min_max=[round(v, 4) for v in t['fused'][1:]],
                              stock_ms=round(t['stock'][0], 4), stock_ms_min_max=[round(v, 4) for v in t['stock'][1:]],
                              soft_argmin_kernel_ms=round(spans['soft_argmin'][0] / args.repeats, 4),
                              fused_kernel_ms=round(spans['soft_argmin_prob'][0] / args.repeats, 4),
                              fused_over_soft_argmin=round(t['fused'][0] / t['plain'][0], 3),
                              stock_over_fused=round(t['stock'][0] / t['fused'][0], 2),
                              model_bytes_soft_argmin=4 * npix * (D + 1), model_bytes_fused=4 * npix * (D + 4),
                              fused_model_gb_per_s=round(4 * npix * (D + 4) / (spans['soft_argmin_prob'][0] / args.repeats) / 1e6, 1),
                              depth_bits_equal=bool(torch.equal(depth_a, depth_b)),
                              max_abs_depth_difference_to_stock=float((depth_b - depth_c).abs().max()),
                              pixels_with_another_plane_than_stock=int((~same_planes).sum()),
                              max_abs_prob_difference_elsewhere=float((prob_b - prob_c).abs()[same_planes].max()),
                              repeats=args.repeats)), flush=True)
        del x, depth_a, depth_b, depth_c, prob_b, prob_c


def driver(args):
    out = args.out or os.path.join(ROOT, 'build', 'bench_confidence')
    os.makedirs(out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), '--repeats', str(args.repeats), '--warmup', str(args.warmup), '--step', 'hip']
    p = subprocess.run(['timeout', '-k', '10', '300'] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        sys.exit('bench_confidence.py: the measuring step ended with status %d' % p.returncode)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    for ln in lines:
        print(ln, flush=True)
    with open(os.path.join(out, 'bench_confidence.json'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--step', choices=['hip'])
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.step:
        step(args)
    else:
        driver(args)


if __name__ == '__main__':
    main()
