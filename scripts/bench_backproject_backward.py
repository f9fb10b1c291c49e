#!/usr/bin/env python3
"""Backward of the back-projected variance: the HIP route (3dvnet_amd/training.py: BackprojectVariance ->
v3d_backproject_variance_backward_f32) against the same gradients through stock torch ops on the device (the sampling grid built
as lightningmodel.py:152-160 does and detached, F.grid_sample + an index_add_ mean; for n = 0 the points R^T (K^-1 (p d) - t) by
torch.bmm).  Both routes sample at the world points the forward kernel wrote.

    python scripts/bench_backproject_backward.py [--cfg cfg2] [--views 14,64] [--feat-dims 32,16] [--ns 0,3] [--offset 0.05]
                                                 [--repeats 10] [--warmup 2] [--out DIR]

Without --step this is a driver: every GPU step runs as a child process of its own under `timeout`, in sequence, and the first
step that fails ends the run.
  --step hip     median wall time of the whole Function.backward (autograd.grad with the forward done before; n = 0: both
                 gradients, n > 0: the feature gradient), peak memory (torch.cuda.max_memory_allocated) over forward + backward,
                 and the atomic bytes the kernel issues, COUNTED from the sample positions: one 4 C-byte add per in-image tap of
                 every sample without the on-chip combining, one per in-image tap of every footprint run (consecutive hypotheses
                 of a segment in one footprint) with it.
  --step torch   the same two figures for the stock route (the peak includes what autograd saves: the gathered features, the
                 samples, their squares), and the largest difference between the two routes' gradients.
One JSON line per shape and step; they land in OUT/bench_backproject_backward.json.  A record, no gate.
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


def sample_grid(pts, rot, tv, K, edges_ref_row, edge_src, img_size):
    """World points [n_ref, S, 3] -> grid_sample coordinates [E, S, 1, 2] (lightningmodel.py:152-160), no gradient."""
    import torch
    with torch.no_grad():
        P = torch.bmm(K[edge_src], torch.cat((rot[edge_src], tv[edge_src].unsqueeze(2)), dim=2))          # [E, 3, 4]
        X = pts[edges_ref_row].transpose(1, 2)                                                        # [E, 3, S]
        q = torch.bmm(P[:, :, :3], X) + P[:, :, 3:]
        uv = q[:, :2] / (q[:, 2:3].abs() + 1e-8)
        gx = uv[:, 0] / (img_size[1] - 1) * 2 - 1
        gy = uv[:, 1] / (img_size[0] - 1) * 2 - 1
        return torch.stack((gx, gy), dim=-1).unsqueeze(2)


def atomic_bytes(grid, n_hyp, seg, Hf, Wf, C):
    """grid [E, P * n_hyp, 1, 2] -> (bytes without combining, bytes with combining along the hypotheses of a segment)."""
    import torch
    E = grid.shape[0]
    ix = (grid[:, :, 0, 0] + 1) * 0.5 * (Wf - 1)
    iy = (grid[:, :, 0, 1] + 1) * 0.5 * (Hf - 1)
    x0 = torch.floor(torch.nan_to_num(ix, nan=-1.0).clamp(-1, Wf)).view(E, -1, n_hyp)
    y0 = torch.floor(torch.nan_to_num(iy, nan=-1.0).clamp(-1, Hf)).view(E, -1, n_hyp)
    nx = ((x0 >= 0) & (x0 < Wf)).long() + (x0 + 1 < Wf).long()
    ny = ((y0 >= 0) & (y0 < Hf)).long() + (y0 + 1 < Hf).long()
    taps = nx * ny
    new = torch.ones_like(taps, dtype=torch.bool)
    new[:, :, 1:] = (x0[:, :, 1:] != x0[:, :, :-1]) | (y0[:, :, 1:] != y0[:, :, :-1])
    new[:, :, ::seg] = True
    return int(taps.sum()) * 4 * C, int((taps * new).sum()) * 4 * C


def step(args):
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        sys.exit('bench_backproject_backward.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    syn = importlib.import_module('3dvnet_amd.synthetic')
    mvs = importlib.import_module('3dvnet_amd.mvsnet')
    tr = importlib.import_module('3dvnet_amd.training')
    shapes = [(v, C, n) for v in map(int, args.views.split(',')) for C in map(int, args.feat_dims.split(','))
              for n in map(int, args.ns.split(','))]
    for n_ref, C, n in shapes:
        inp = syn.make_costvolume_inputs(args.cfg, n_ref, feat_dim=C)
        (Hf, Wf), (h, w), img_size = inp['feat_size'], inp['plane_size'], inp['img_size']
        n_hyp, S = 2 * n + 1, h * w * (2 * n + 1)
        edges = inp['edges'].to(dev)
        csr = mvs.edges_to_csr(edges)
        ref_idx, _, edge_ofs, edge_src = csr
        refs = ref_idx.cpu().long()
        rot, tv, K = (x.to(dev) for x in (inp['rotmats'], inp['tvecs'], inp['K']))
        depth0 = syn.ray_box_depth(inp['rotmats'][refs], inp['tvecs'][refs], inp['K'][refs], img_size, (h, w)).to(dev)
        feat = inp['feat'].to(dev).requires_grad_(True)
        depth = depth0.clone().requires_grad_(n == 0)
        g = torch.Generator().manual_seed(7)
        gv = torch.randn((n_ref * h * w, n_hyp, C), generator=g).to(dev)
        gp = torch.randn((n_ref * h * w, n_hyp, 3), generator=g).to(dev)
        base = dict(bench='backproject_backward', step=args.step, cfg=args.cfg, views=n_ref, edges=int(edges.shape[1]), C=C, n=n,
                    offset=args.offset, samples_per_view=S, repeats=args.repeats)
        outs = lambda pts, var: ([var, pts], [feat, depth], [gv, gp]) if n == 0 else ([var], [feat], [gv])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        pts, var = tr.backproject_variance(depth, feat, rot, tv, K, edges, img_size, offset=args.offset, n=n, csr=csr)
        o, i, go = outs(pts, var)
        g_hip = torch.autograd.grad(o, i, grad_outputs=go, retain_graph=True)
        torch.cuda.synchronize()
        hip_peak = torch.cuda.max_memory_allocated(dev) - before
        counts = (edge_ofs[1:] - edge_ofs[:-1]).long()
        gather = torch.repeat_interleave(torch.arange(n_ref, device=dev), counts)
        grid = sample_grid(pts.detach().view(n_ref, S, 3), rot, tv, K, gather, edge_src.long(), img_size)
        if args.step == 'hip':
            med, lo, hi = timed(lambda: torch.autograd.grad(o, i, grad_outputs=go, retain_graph=True), args.warmup, args.repeats)
            plain, combined = atomic_bytes(grid, n_hyp, 1 if n == 0 else 8, Hf, Wf, C)
            print(json.dumps(dict(base, hip_backward_ms=round(med, 4), hip_backward_ms_min_max=[round(lo, 4), round(hi, 4)],
                                  hip_peak_bytes_forward_backward=hip_peak, atomic_bytes_uncombined=plain,
                                  atomic_bytes_issued=combined)), flush=True)
            continue
        del pts, var, o

        def forward():
            x = F.grid_sample(feat[edge_src.long()], grid, mode='bilinear', align_corners=True).squeeze(3)       # [E, C, S]
            cnt = counts.clamp(min=1).view(-1, 1, 1).float()
            avg = torch.zeros((n_ref, C, S), device=dev).index_add_(0, gather, x) / cnt
            avg_sq = torch.zeros((n_ref, C, S), device=dev).index_add_(0, gather, x ** 2) / cnt
            var_t = (avg_sq - avg ** 2).view(n_ref, C, h * w, n_hyp).permute(0, 2, 3, 1).reshape(n_ref * h * w, n_hyp, C)
            if n > 0:
                return None, var_t
            xs = torch.linspace(0, img_size[1] - 1, w, device=dev)
            ys = torch.linspace(0, img_size[0] - 1, h, device=dev)
            yy, xx = torch.meshgrid(ys, xs, indexing='ij')
            p = torch.stack((xx, yy, torch.ones_like(xx)), 0).reshape(1, 3, -1)
            cam = torch.bmm(torch.inverse(K[ref_idx.long()]), p * depth.view(n_ref, 1, -1)) - tv[ref_idx.long()].unsqueeze(2)
            return torch.bmm(rot[ref_idx.long()].transpose(1, 2), cam).transpose(1, 2).reshape(n_ref * h * w, 1, 3), var_t
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        pts_t, var_t = forward()
        o, i, go = outs(pts_t, var_t)
        g_torch = torch.autograd.grad(o, i, grad_outputs=go, retain_graph=True)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - before
        med, lo, hi = timed(lambda: torch.autograd.grad(o, i, grad_outputs=go, retain_graph=True), args.warmup, args.repeats)
        diff = [float((a - b).abs().max()) / float(a.abs().max()) for a, b in zip(g_torch, g_hip)]
        print(json.dumps(dict(base, torch_backward_ms=round(med, 3), torch_backward_ms_min_max=[round(lo, 3), round(hi, 3)],
                              torch_peak_bytes_forward_backward=peak, hip_peak_bytes_forward_backward=hip_peak,
                              max_abs_diff_over_max_abs=diff)), flush=True)
        del pts_t, var_t, o, g_torch, grid


def driver(args):
    out = args.out or os.path.join(ROOT, 'build', 'bench_backproject_backward')
    os.makedirs(out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), '--cfg', args.cfg, '--views', args.views, '--repeats', str(args.repeats),
          '--warmup', str(args.warmup), '--feat-dims', args.feat_dims, '--ns', args.ns, '--offset', str(args.offset)]
    lines = []
    for name, limit in (('hip', 200), ('torch', 300)):
        cmd = ['timeout', '-k', '10', str(limit)] + me + ['--step', name]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for ln in p.stdout.splitlines():
            if ln.startswith('{'):
                print(ln, flush=True)
                lines.append(ln)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-4000:])
            sys.exit('bench_backproject_backward.py: step %s ended with status %d; nothing more is started' % (name, p.returncode))
    with open(os.path.join(out, 'bench_backproject_backward.json'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    rec = [json.loads(ln) for ln in lines]
    key = lambda r: (r['views'], r['C'], r['n'])
    for hp in (r for r in rec if r['step'] == 'hip'):
        to = next(r for r in rec if r['step'] == 'torch' and key(r) == key(hp))
        print('%s, %d views, C = %d, n = %d: HIP backward %.3f ms, stock torch %.3f ms (%.1f x); peak %.1f MB against %.1f MB; atomic '
              'bytes %.1f MB issued, %.1f MB without combining'
              % (hp['cfg'], hp['views'], hp['C'], hp['n'], hp['hip_backward_ms'], to['torch_backward_ms'],
                 to['torch_backward_ms'] / hp['hip_backward_ms'], hp['hip_peak_bytes_forward_backward'] / 2 ** 20,
                 to['torch_peak_bytes_forward_backward'] / 2 ** 20, hp['atomic_bytes_issued'] / 1e6,
                 hp['atomic_bytes_uncombined'] / 1e6), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default='cfg2')
    ap.add_argument('--views', default='14,64')
    ap.add_argument('--feat-dims', default='32,16')
    ap.add_argument('--ns', default='0,3')
    ap.add_argument('--offset', type=float, default=0.05)
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
