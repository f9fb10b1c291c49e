#!/usr/bin/env python3
"""Backward of the plane-sweep variance: the HIP kernel (3dvnet_amd/training.py: PlaneSweepVariance ->
v3d_psv_variance_backward_f32) against the same gradient through stock torch ops on the device (F.grid_sample + an index_add_
mean, as oracle/costvolume.py restates mvsnet.py:209-216; the sampling positions come from the library's diagnostic twin of the
warp kernels' projection, so both routes sample the same points).

    python scripts/bench_psv_backward.py [--cfg cfg2] [--views 14,64] [--feat-dim 32] [--repeats 10] [--warmup 2] [--out DIR]

Without --step this is a driver: every GPU step runs as a child process of its own under `timeout`, in sequence, and the
first step that fails ends the run.
  --step hip     median wall time of the backward alone (autograd.grad of the Function, forward done before), peak memory
                 (torch.cuda.max_memory_allocated) over forward + backward, and the atomic bytes the kernel issues, COUNTED
                 from the sample positions: one 4 C-byte add per in-image tap of every sample without the on-chip combining,
                 one per in-image tap of every footprint run (consecutive planes of a 16-plane segment in one footprint) with it.
  --step torch   the same two figures for the stock route (backward alone; the peak includes the activations autograd saves:
                 the warped volume, its square, the grid), and the largest difference between the two gradients.
One JSON line per view count and step; they land in OUT/bench_psv_backward.json.  A record, no gate.
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

SEG = 16          # planes a wave of the backward kernel walks (csrc/psv_backward.hip: kBDS, the S of variance_backward.h's walk)


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


def atomic_bytes(pos, D, Hf, Wf, C):
    """pos [E, D*P, 2] sample positions in feature pixels -> (bytes without combining, bytes with combining)."""
    import torch
    E = pos.shape[0]
    x0 = torch.floor(torch.nan_to_num(pos[..., 0], nan=-1.0).clamp(-1, Wf)).view(E, D, -1)
    y0 = torch.floor(torch.nan_to_num(pos[..., 1], nan=-1.0).clamp(-1, Hf)).view(E, D, -1)
    nx = ((x0 >= 0) & (x0 < Wf)).long() + (x0 + 1 < Wf).long()
    ny = ((y0 >= 0) & (y0 < Hf)).long() + (y0 + 1 < Hf).long()
    taps = nx * ny
    new = torch.ones_like(taps, dtype=torch.bool)
    new[:, 1:] = (x0[:, 1:] != x0[:, :-1]) | (y0[:, 1:] != y0[:, :-1])
    new[:, ::SEG] = True
    return int(taps.sum()) * 4 * C, int((taps * new).sum()) * 4 * C


def step(args):
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        sys.exit('bench_psv_backward.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    syn = importlib.import_module('3dvnet_amd.synthetic')
    mvs = importlib.import_module('3dvnet_amd.mvsnet')
    tr = importlib.import_module('3dvnet_amd.training')
    for n_ref in [int(v) for v in args.views.split(',')]:
        inp = syn.make_costvolume_inputs(args.cfg, n_ref, feat_dim=args.feat_dim)
        start, interval, D = inp['depth']
        (Hf, Wf), (h, w), C = inp['feat_size'], inp['plane_size'], inp['feat'].shape[1]
        geom = (start, interval, D, inp['img_size'], inp['plane_size'])
        feat = inp['feat'].to(dev).requires_grad_(True)
        edges = inp['edges'].to(dev)
        gv = torch.randn((n_ref, C, D, h, w), generator=torch.Generator().manual_seed(7)).to(dev)
        base = dict(bench='psv_backward', step=args.step, cfg=args.cfg, views=n_ref, edges=int(edges.shape[1]), C=C,
                    voxels_per_view=D * h * w, repeats=args.repeats)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        var = tr.plane_sweep_variance(feat, inp['rotmats'], inp['tvecs'], inp['K'], edges, *geom)
        g_hip = torch.autograd.grad(var, feat, grad_outputs=gv, retain_graph=True)[0]
        torch.cuda.synchronize()
        hip_peak = torch.cuda.max_memory_allocated(dev) - before
        if args.step == 'hip':
            med, lo, hi = timed(lambda: torch.autograd.grad(var, feat, grad_outputs=gv, retain_graph=True), args.warmup, args.repeats)
            pos, _, _ = mvs.plane_sweep_sample_positions(inp['rotmats'], inp['tvecs'], inp['K'], edges, start, interval, D,
                                                         inp['img_size'], (Hf, Wf), (h, w), dev)
            plain, combined = atomic_bytes(pos, D, Hf, Wf, C)
            print(json.dumps(dict(base, hip_backward_ms=round(med, 4), hip_backward_ms_min_max=[round(lo, 4), round(hi, 4)],
                                  hip_peak_bytes_forward_backward=hip_peak, atomic_bytes_uncombined=plain,
                                  atomic_bytes_issued=combined, atomic_gb_per_s=round(combined / med / 1e6, 1))), flush=True)
            continue
        del var
        pos, _, csr = mvs.plane_sweep_sample_positions(inp['rotmats'], inp['tvecs'], inp['K'], edges, start, interval, D,
                                                       inp['img_size'], (Hf, Wf), (h, w), dev)
        _, _, edge_ofs, edge_src = csr
        counts = (edge_ofs[1:] - edge_ofs[:-1]).long()
        gather = torch.repeat_interleave(torch.arange(n_ref, device=dev), counts)
        grid = torch.stack((pos[..., 0] / (Wf - 1) * 2 - 1, pos[..., 1] / (Hf - 1) * 2 - 1), dim=-1).unsqueeze(2)
        del pos

        def forward():
            x = F.grid_sample(feat[edge_src.long()], grid, mode='bilinear', align_corners=True)
            x = x.squeeze(3).view(-1, C, D, h, w)
            cnt = counts.clamp(min=1).view(-1, 1, 1, 1, 1).float()
            avg = torch.zeros((n_ref, C, D, h, w), device=dev).index_add_(0, gather, x) / cnt
            avg_sq = torch.zeros((n_ref, C, D, h, w), device=dev).index_add_(0, gather, x ** 2) / cnt
            return avg_sq - avg ** 2
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        var_t = forward()
        g_torch = torch.autograd.grad(var_t, feat, grad_outputs=gv, retain_graph=True)[0]
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - before
        med, lo, hi = timed(lambda: torch.autograd.grad(var_t, feat, grad_outputs=gv, retain_graph=True), args.warmup, args.repeats)
        diff = float((g_torch - g_hip).abs().max()) / float(g_torch.abs().max())
        print(json.dumps(dict(base, torch_backward_ms=round(med, 3), torch_backward_ms_min_max=[round(lo, 3), round(hi, 3)],
                              torch_peak_bytes_forward_backward=peak, hip_peak_bytes_forward_backward=hip_peak,
                              max_abs_diff_over_max_abs=diff)), flush=True)
        del var_t, g_torch, grid


def driver(args):
    out = args.out or os.path.join(ROOT, 'build', 'bench_psv_backward')
    os.makedirs(out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), '--cfg', args.cfg, '--views', args.views, '--repeats', str(args.repeats),
          '--warmup', str(args.warmup), '--feat-dim', str(args.feat_dim)]
    lines = []
    for name, limit in (('hip', 240), ('torch', 420)):
        cmd = ['timeout', '-k', '10', str(limit)] + me + ['--step', name]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for ln in p.stdout.splitlines():
            if ln.startswith('{'):
                print(ln, flush=True)
                lines.append(ln)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-4000:])
            sys.exit('bench_psv_backward.py: step %s ended with status %d; nothing more is started' % (name, p.returncode))
    with open(os.path.join(out, 'bench_psv_backward.json'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    rec = [json.loads(ln) for ln in lines]
    for hp in (r for r in rec if r['step'] == 'hip'):
        to = next(r for r in rec if r['step'] == 'torch' and r['views'] == hp['views'])
        print('%s, %d views: HIP backward %.3f ms, stock torch %.1f ms (%.0f x); peak %.0f MB against %.0f MB; atomic bytes %.2f GB '
              'issued, %.2f GB without combining' % (hp['cfg'], hp['views'], hp['hip_backward_ms'], to['torch_backward_ms'],
                                                     to['torch_backward_ms'] / hp['hip_backward_ms'],
                                                     hp['hip_peak_bytes_forward_backward'] / 2 ** 20,
                                                     to['torch_peak_bytes_forward_backward'] / 2 ** 20,
                                                     hp['atomic_bytes_issued'] / 1e9, hp['atomic_bytes_uncombined'] / 1e9), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default='cfg2')
    ap.add_argument('--views', default='14,64')
    ap.add_argument('--feat-dim', type=int, default=32, choices=[16, 32])
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--step', choices=['hip', 'torch'])
    ap.add_argument('--out')
    args = ap.parse_args()
    if args.step:
        step(args)
    else:
        driver(args)


if __name__ == '__main__':
    main()
