#!/usr/bin/env python3
"""3D scoring of a fused scene on the device: the HIP path (3dvnet_amd/metrics3d.py: v3d_cloud_downsample_f32,
v3d_nn_query_f32, v3d_cloud_metrics_f64) against the same job in stock torch ops on the same GPU, in one run.

    python scripts/bench_metrics3d.py [--size 256x320,480x640] [--views 64] [--repeats 10] [--warmup 2] [--torch-repeats 1]
                                      [--out profiles/r10_bench_metrics3d.json] [--profile]

Scenes: the 64-view ring of tests/fusion_oracle.py (analytic box-room depths + N(0, 4 cm), 3 % of the pixels zeroed), fused on
the device; ground truth: 3 M samples of the room's noise-free surfaces.  Both clouds are down-sampled at 2 cm and scored at
5 cm, as mv3d/eval/processresults.py:283-295 does.  Each stage is timed with HIP events (median of the repeats): down-sample
of the fused cloud (count taken from the device word), down-sample of the ground truth, the two neighbour searches, the metric
reduction.  The stock-torch route does the same job with torch.unique + index_add_ in float64 for the down-sample and a
chunked float64 brute-force minimum for the neighbours.  One JSON line per size, appended to --out as well.  `--profile` runs
only the HIP stages a few times (for rocprofv3).
"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def torch_down_sample(p, voxel):
    p64 = p.double()
    vmin = p64.min(0).values - 0.5 * voxel
    c = torch.floor((p64 - vmin) / voxel).long()
    key = (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]
    uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
    s = torch.zeros((uniq.shape[0], 3), dtype=torch.float64, device=p.device).index_add_(0, inv, p64)
    return (s / cnt[:, None]).float()


def torch_nearest(target, query, chunk_elems=1 << 28):
    t, q = target.double(), query.double()
    tx, ty, tz = t[:, 0][None], t[:, 1][None], t[:, 2][None]
    chunk = max(1, chunk_elems // t.shape[0])
    idx = torch.empty(q.shape[0], dtype=torch.long, device=q.device)
    dist = torch.empty(q.shape[0], dtype=torch.float64, device=q.device)
    for a in range(0, q.shape[0], chunk):
        qq = q[a:a + chunk]
        s = (qq[:, 0:1] - tx) ** 2
        s += (qq[:, 1:2] - ty) ** 2
        s += (qq[:, 2:3] - tz) ** 2
        best, arg = s.min(dim=1)
        idx[a:a + chunk], dist[a:a + chunk] = arg, best.sqrt()
    return idx, dist


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
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', default='256x320,480x640')
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--torch-repeats', type=int, default=1)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_metrics3d.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    fusion = importlib.import_module('3dvnet_amd.fusion')
    m3 = importlib.import_module('3dvnet_amd.metrics3d')
    syn = importlib.import_module('3dvnet_amd.synthetic')
    import cloud_oracle as co
    import fusion_oracle as fo
    gt_raw = torch.as_tensor(co.room(3000000, 0.0, 81, dims=syn.ROOM)).to(dev)
    for size in [tuple(int(v) for v in s.split('x')) for s in args.size.split(',')]:
        d, img, poses, K = fo.scene(args.views, size, seed=1237, yaw_step_deg=None, sigma=0.04)
        pts, rgb, _, count = fusion.fuse_depth_maps(d.to(dev), poses, K, img.to(dev), 0.1, 3)
        col = rgb.float() / 255.
        pred, _, n_pred = m3.voxel_down_sample(pts, 0.02, attr=col, count=count)
        trgt, _, n_trgt = m3.voxel_down_sample(gt_raw, 0.02)
        n_fused, n_pred, n_trgt = int(count), int(n_pred), int(n_trgt)
        pred, trgt = pred[:n_pred].contiguous(), trgt[:n_trgt].contiguous()
        _, d_pred = m3.nearest_neighbors(trgt, pred)
        _, d_trgt = m3.nearest_neighbors(pred, trgt)
        stages = {
            'downsample_pred_ms': lambda: m3.voxel_down_sample(pts, 0.02, attr=col, count=count),
            'downsample_gt_ms': lambda: m3.voxel_down_sample(gt_raw, 0.02),
            'nn_pred_to_target_ms': lambda: m3.nearest_neighbors(trgt, pred),
            'nn_target_to_pred_ms': lambda: m3.nearest_neighbors(pred, trgt),
            'metrics_ms': lambda: m3.cloud_metrics(d_pred, d_trgt, 0.05),
        }
        if args.profile:
            for _ in range(3):
                for fn in stages.values():
                    fn()
            torch.cuda.synchronize()
            continue
        hip = {k: round(timed(fn, args.warmup, args.repeats), 4) for k, fn in stages.items()}
        lib = importlib.import_module('3dvnet_amd._lib')
        lib.timing_enable(True)
        for _ in range(args.repeats):
            stages['nn_pred_to_target_ms']()
        spans = lib.timing_collect()
        lib.timing_enable(False)
        query_ms = spans['nn_query'][0] / spans['nn_query'][1]
        build_ms = spans['nn_build'][0] / spans['nn_build'][1]
        fused = pts[:n_fused].contiguous()
        tor = {
            'downsample_pred_ms': timed(lambda: torch_down_sample(fused, 0.02), 1, args.torch_repeats),
            'downsample_gt_ms': timed(lambda: torch_down_sample(gt_raw, 0.02), 1, args.torch_repeats),
            'nn_pred_to_target_ms': timed(lambda: torch_nearest(trgt, pred), 0, args.torch_repeats),
            'nn_target_to_pred_ms': timed(lambda: torch_nearest(pred, trgt), 0, args.torch_repeats),
        }
        tor = {k: round(v, 2) for k, v in tor.items()}
        # same answer: the brute-force distances against the HIP ones
        _, t_pred = torch_nearest(trgt, pred)
        worst = float(((d_pred.double() - t_pred).abs() / t_pred.clamp_min(1e-30)).max()) / 2.0 ** -24
        rec = dict(zip(m3.KEYS, m3.cloud_metrics(d_pred, d_trgt, 0.05).cpu().tolist()))
        hip_total = sum(hip.values())
        tor_total = sum(tor.values())
        line = json.dumps(dict(
            bench='metrics3d', views=args.views, size=list(size), fused_rows=n_fused, pred_rows=n_pred, target_rows=n_trgt,
            hip_ms=hip, hip_total_ms=round(hip_total, 3), nn_pred_to_target_build_ms=round(build_ms, 4),
            nn_pred_to_target_query_span_ms=round(query_ms, 4), torch_ms=tor, torch_total_ms=round(tor_total, 1),
            ratio_torch_over_hip=round(tor_total / hip_total, 1),
            ratio_nn_torch_over_hip=round((tor['nn_pred_to_target_ms'] + tor['nn_target_to_pred_ms']) /
                                          (hip['nn_pred_to_target_ms'] + hip['nn_target_to_pred_ms']), 1),
            max_rel_err_vs_float64_brute_force_u=round(worst, 2), metrics=rec, repeats=args.repeats,
            torch_repeats=args.torch_repeats))
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')


if __name__ == '__main__':
    main()
