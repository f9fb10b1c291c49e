#!/usr/bin/env python3
"""``PL3DVNet.forward`` (3dvnet_amd/lightningmodel.py) on one cfg3-shaped validation batch -- 16 reference views with a (4, 3)
window = 23 images of 256 x 320, synthetic features at 64 x 80 and 128 x 160, stage 1 on 56 x 56 with 96 planes, offsets
[0.05, 0.05, 0.025] x 2 iterations, 4 cm voxels -- and, on the ten depth maps it supervises, the ten ``loss.supervise`` calls
(csrc/supervision.hip) against the same ten points in stock torch ops on the same GPU.  The stock version is the reference's
formulas (mv3d/loss.py:6-20, mv3d/eval/metricfunctions.py:26-67, the ``F.interpolate`` of mv3d/lightningmodel.py:58) restated here.

    python scripts/bench_forward.py [--repeats 30] [--warmup 3] [--refs 16] [--out DIR]

Without --step this is a driver: the measuring step runs as a child process of its own under `timeout`.  Device events around
each call (median of --repeats, with minimum and maximum).  Launches: two per point for ``supervise`` (the library's own event
brackets count them); for the stock version the number of aten operators dispatched on device tensors per point, which is a lower
bound of its launches (a reduction may take two).  Shares are of the median time of one ``forward``.  The JSON line lands in
OUT/bench_forward.json.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OFFSETS, N_ITERS = [0.05, 0.05, 0.025], 2


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


def stock_point(pred, gt, interval):
    """one supervised point in stock torch ops: the reference's resize, loss and metrics -> [9] (eight metrics, the loss)"""
    import torch
    import torch.nn.functional as F
    if gt.shape != pred.shape:
        gt = F.interpolate(gt.unsqueeze(1), pred.shape[-2:], mode='nearest').squeeze(1)
    mask = (~torch.eq(gt, 0.0)).type(torch.float)
    denom = torch.sum(mask, dim=(1, 2)) + 1e-7
    loss = torch.mean((torch.sum(mask * torch.abs(pred - gt), dim=(1, 2)) / interval) / denom)
    valid = ((gt >= 0.5) & (gt < 65.)).type(torch.float)
    denom = torch.sum(valid, dim=(1, 2)) + 1e-7
    abs_diff = torch.abs(pred - gt)
    abs_inv = torch.abs(1. / pred - 1. / gt)
    abs_inv[torch.isinf(abs_inv)] = 0.
    abs_inv[torch.isnan(abs_inv)] = 0.
    abs_rel = torch.mean(torch.sum((abs_diff / (gt + 1e-7)) * valid, dim=(1, 2)) / denom)
    sq_rel = torch.mean(torch.sum((abs_diff ** 2 / (gt + 1e-7)) * valid, dim=(1, 2)) / denom)
    rmse = torch.mean(torch.sqrt(torch.sum(abs_diff ** 2 * valid, dim=(1, 2)) / denom))
    abs_diff = torch.mean(torch.sum(abs_diff * valid, dim=(1, 2)) / denom)
    abs_inv = torch.mean(torch.sum(abs_inv * valid, dim=(1, 2)) / denom)
    r1, r2 = (pred / gt).unsqueeze(-1), (gt / pred).unsqueeze(-1)
    rel_max = torch.max(torch.cat((r1, r2), dim=-1), dim=-1)[0]
    d = [torch.mean(torch.sum((rel_max < 1.25 ** k) * valid, dim=(1, 2)) / denom) for k in (1, 2, 3)]
    return torch.stack([abs_rel, abs_diff, abs_inv, sq_rel, rmse] + d + [loss])


def count_aten_ops(fn):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Counter(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Counter.n += 1
            return func(*args, **(kwargs or {}))
    with Counter():
        fn()
    return Counter.n


def step(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_forward.py measures on a HIP device; none is visible')
    syn = importlib.import_module('3dvnet_amd.synthetic')
    lm = importlib.import_module('3dvnet_amd.lightningmodel')
    drv = importlib.import_module('3dvnet_amd.eval_3dvnet')
    loss_mod = importlib.import_module('3dvnet_amd.loss')
    lib = importlib.import_module('3dvnet_amd._lib')
    Batch = importlib.import_module('3dvnet_amd.batch').Batch
    dev = torch.device('cuda:0')
    cfg = syn.CONFIGS['cfg3']
    img, (hq, wq) = cfg['img_size'], cfg['feat_size']
    nb, na = cfg['window']
    edges, n_img = syn.make_edges(args.refs, nb, na)
    rot, tv, K = syn.make_cameras(n_img, img, seed=1237)
    gt = syn.ray_box_depth(rot[nb:nb + args.refs], tv[nb:nb + args.refs], K[nb:nb + args.refs], img, img).float()
    gt[torch.rand(gt.shape, generator=torch.Generator().manual_seed(11)) < 0.1] = 0.0            # 10 % holes
    b = Batch(syn.make_images(n_img, img, seed=1239), rot, tv, K, gt.contiguous(), edges)
    b.features_quarter = syn.make_features(n_img, 32, hq, wq, seed=1237)
    b.features_half = syn.make_features(n_img, 32, 2 * hq, 2 * wq, seed=1238)
    b.images_batch = torch.zeros(n_img, dtype=torch.long)
    b = b.to(dev)
    net = lm.PL3DVNet(None, dict(drv.DEPTH_CONFIG), cfg['edge_len'], feat_dim=32, img_size=img).eval()
    net.mvsnet.cnn_3d.load_state_dict(syn.costregnet_weights(seed=0, sharpen=200.0), strict=False)
    net.pointnet.load_state_dict(syn.pointnet_weights())
    net.sparse_conv.load_state_dict(syn.sparse_unet_weights())
    net.decoder.load_state_dict(syn.decoder_weights(sharpen=50.0), strict=False)
    for m, seed, cin in zip((net.refine_quarter, net.refine_half, net.refine_full), (5, 6, 7), (33, 33, 4)):
        m.load_state_dict(syn.propagation_weights(cin, 32, seed), strict=False)
    net = net.to(dev)
    interval = drv.DEPTH_CONFIG['depth_interval']
    with torch.no_grad():
        out = net(b, OFFSETS, N_ITERS, return_depths=True)
        depths = out['depths']
        gt_dev = b.depth_images

        def forward():
            return net(b, OFFSETS, N_ITERS)

        def new_points():
            return [loss_mod.supervise(d, gt_dev, interval).mean for d in depths]

        def stock_points():
            return [stock_point(d, gt_dev, interval) for d in depths]
        a = torch.stack(new_points())[:, 1:].cpu()
        c = torch.stack(stock_points()).double().cpu()
        rel = ((a - c).abs() / c.abs().clamp_min(1e-30)).max(0).values
        t = {k: timed(f, args.warmup, args.repeats) for k, f in (('forward', forward), ('new', new_points), ('stock', stock_points))}
        per_size = {}
        for name, k in (('56x56', 0), ('64x80', 7), ('128x160', 8), ('256x320', 9)):
            per_size[name] = dict(new_ms=timed(lambda: loss_mod.supervise(depths[k], gt_dev, interval), args.warmup, args.repeats)[0],
                                  stock_ms=timed(lambda: stock_point(depths[k], gt_dev, interval), args.warmup, args.repeats)[0])
        lib.timing_enable(True)
        new_points()
        spans = {name: (round(v[0], 4), v[1]) for name, v in lib.timing_collect().items() if name.startswith('depth_supervision')}
        lib.timing_enable(False)
        stock_ops = count_aten_ops(stock_points)
    n_points = len(depths)
    print(json.dumps(dict(bench='forward', refs=args.refs, images=n_img, img=list(img), points=n_points, repeats=args.repeats,
                          forward_ms_med_min_max=t['forward'], supervise_10_points_ms_med_min_max=t['new'],
                          stock_10_points_ms_med_min_max=t['stock'],
                          supervise_ms_per_point=round(t['new'][0] / n_points, 4), stock_ms_per_point=round(t['stock'][0] / n_points, 4),
                          stock_over_supervise=round(t['stock'][0] / t['new'][0], 2),
                          supervise_share_of_forward=round(t['new'][0] / t['forward'][0], 4),
                          stock_share_of_forward_if_it_replaced_supervise=round(t['stock'][0] / (t['forward'][0] - t['new'][0] + t['stock'][0]), 4),
                          supervise_launches_per_point=sum(v[1] for v in spans.values()) / n_points, supervise_kernels_ms_10_points=spans,
                          stock_aten_ops_per_point=stock_ops / n_points, per_size_ms=per_size,
                          loss=float(out['loss']), max_rel_difference_to_stock_fp32=[float(v) for v in rel])), flush=True)


def driver(args):
    out = args.out or os.path.join(ROOT, 'build', 'bench_forward')
    os.makedirs(out, exist_ok=True)
    cmd = [sys.executable, os.path.abspath(__file__), '--repeats', str(args.repeats), '--warmup', str(args.warmup), '--refs',
           str(args.refs), '--step', 'hip']
    p = subprocess.run(['timeout', '-k', '10', '400'] + cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-4000:])
        sys.exit('bench_forward.py: the measuring step ended with status %d' % p.returncode)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    for ln in lines:
        print(ln, flush=True)
    with open(os.path.join(out, 'bench_forward.json'), 'w') as f:
        f.write('\n'.join(lines) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--refs', type=int, default=16)
    ap.add_argument('--step', choices=['hip'])
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.step:
        step(args)
    else:
        driver(args)


if __name__ == '__main__':
    main()
