#!/usr/bin/env python3
"""Backward of the sparse trilinear interpolation: the HIP route (3dvnet_amd/training.py: SparseInterpolate ->
v3d_sparse_interp_backward_f32) against the same gradient through stock torch ops on the device: the corner table out of the
forward's workspace, feats[rows] gathered into [nq, 8, C], weighted, summed, and autograd (an index_put backward) from there.

    python scripts/bench_sparse_interp_backward.py [--cfg cfg2] [--views 14,64] [--ns 0,3] [--offset 0.05] [--edge-len M]
                                                   [--repeats 10] [--warmup 2] [--out DIR]

The levels are those of the project's own SparseUNet on a synthetic scene (cfg cameras and edges, analytic wall depth + 2 cm noise
at the cfg's depth size, synthetic PointNet / U-Net weights); the queries are the hypothesis points of
training.pointflow_hypotheses (n = 0: one per pixel, n = 3: seven).

Without --step this is a driver: every GPU step runs as a child process of its own under `timeout`, in sequence, and the first
step that fails ends the run.
  --step hip     per level and n: median wall time of the whole Function.backward (autograd.grad with the forward done before),
                 peak memory (torch.cuda.max_memory_allocated) over forward + backward, and the contribution lists COUNTED from
                 the corner table: median and maximum list length per row, rows with an empty list, rows cut into chunks
                 (lists longer than 512) and the number of chunks -- the figures the split rule depends on.
  --step torch   time and peak memory of the stock route, and the largest difference between the two routes' gradients.
Every timed sample is ONE call between two device synchronisations: at a few tenths of a millisecond it includes the launches of
the call's dozen kernels, its two allocations and the synchronisation itself, not kernel time alone.
One JSON line per shape and step; they land in OUT/bench_sparse_interp_backward.json.  A record, no gate.
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
CHUNK = 512                   # kInterpBwdChunk of csrc/sparse_interp.hip


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


def corner_table(libm, x, pts, pts_batch, min_pts):
    """(rows int64 [nq, 8] (-1 absent), w float32 [nq, 8]) out of the workspace of v3d_sparse_interp_f32"""
    import torch
    lib = libm.load()
    dev = pts.device
    n_pts, n_hyp = pts.shape[:2]
    nq, C = n_pts * n_hyp, x['feats'].shape[1]
    ws = torch.empty(lib.v3d_sparse_interp_workspace_bytes(n_pts, n_hyp), dtype=torch.uint8, device=dev)
    out = torch.empty((nq, C), dtype=torch.float32, device=dev)
    f = x['feats'].contiguous()
    libm.check(lib.v3d_sparse_interp_f32(x['sparse'].table.data_ptr(), x['sparse'].n, f.data_ptr(), C, int(x['stride']),
                                         pts.data_ptr(), pts_batch.data_ptr(), n_pts, n_hyp, min_pts.data_ptr(), float(x['res']),
                                         out.data_ptr(), C, 0, ws.data_ptr(), ws.numel(), libm.stream_ptr(dev)),
               'v3d_sparse_interp_f32')
    half = (nq * 32 + 255) // 256 * 256
    rows = ws[:nq * 32].view(torch.int32).view(nq, 8).long()
    w = ws[half:half + nq * 32].view(torch.float32).view(nq, 8).clone()
    return rows, w


def step(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_sparse_interp_backward.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    syn = importlib.import_module('3dvnet_amd.synthetic')
    lm = importlib.import_module('3dvnet_amd.lightningmodel')
    tr = importlib.import_module('3dvnet_amd.training')
    libm = importlib.import_module('3dvnet_amd._lib')
    for n_ref in map(int, args.views.split(',')):
        inp = syn.make_costvolume_inputs(args.cfg, n_ref, feat_dim=32)
        (h, w), img_size = inp['plane_size'], inp['img_size']
        edge_len = args.edge_len or inp['edge_len']
        refs = torch.unique(inp['edges'][0])
        depth = syn.ray_box_depth(inp['rotmats'][refs], inp['tvecs'][refs], inp['K'][refs], img_size, (h, w))
        depth = (depth + 0.02 * torch.randn(depth.shape, generator=torch.Generator().manual_seed(7))).to(dev).contiguous()
        net = lm.PL3DVNet(None, {'depth_start': .5, 'depth_interval': .05, 'n_intervals': 96, 'size': (h, w)}, edge_len,
                          feat_dim=32, img_size=img_size).eval()
        net.pointnet.load_state_dict(syn.pointnet_weights())
        net.sparse_conv.load_state_dict(syn.sparse_unet_weights())
        net = net.to(dev)
        rot, tv, K, edges, feat = (inp[k].to(dev) for k in ('rotmats', 'tvecs', 'K', 'edges', 'feat'))
        depth_batch = torch.zeros(n_ref, dtype=torch.long, device=dev)
        with torch.no_grad():
            xs = net.model_scene(depth, depth_batch, feat, rot, tv, K, edges)
        for n in map(int, args.ns.split(',')):
            with torch.no_grad():
                pts, _, pts_batch = tr.pointflow_hypotheses(depth, depth_batch, feat, rot, tv, K, edges, args.offset, n, img_size)
            pts, pts_batch = pts.contiguous(), pts_batch.contiguous()
            n_pts, n_hyp = pts.shape[:2]
            out = out_t = g_hip = g_torch = rows = wgt = feats = g = None
            for x in xs:
                # nothing of the previous shape is alive when the baseline of the peak is read
                out = out_t = g_hip = g_torch = rows = wgt = feats = g = None
                N, C = x['feats'].shape
                base = dict(bench='sparse_interp_backward', step=args.step, cfg=args.cfg, views=n_ref, n_hyp=n_hyp, queries=n_pts * n_hyp,
                            stride=int(x['stride']), rows=N, C=C, edge_len=edge_len, repeats=args.repeats)
                feats = x['feats'].detach().clone().requires_grad_(True)
                g = torch.randn((n_pts, n_hyp, C), generator=torch.Generator().manual_seed(11)).to(dev)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                before = torch.cuda.memory_allocated(dev)
                out = tr.sparse_interpolate(x, pts, pts_batch, feats)
                (g_hip,) = torch.autograd.grad(out, feats, g, retain_graph=True)
                torch.cuda.synchronize()
                hip_peak = torch.cuda.max_memory_allocated(dev) - before
                rows, wgt = corner_table(libm, x, pts, pts_batch, tr._level_min_pts(x).contiguous())
                if args.step == 'hip':
                    med, lo, hi = timed(lambda: torch.autograd.grad(out, feats, g, retain_graph=True), args.warmup, args.repeats)
                    cnt = torch.bincount(rows[rows >= 0], minlength=N)
                    chunks = torch.where(cnt > CHUNK, (cnt + CHUNK - 1) // CHUNK, torch.ones_like(cnt))
                    print(json.dumps(dict(base, hip_backward_ms=round(med, 4), hip_backward_ms_min_max=[round(lo, 4), round(hi, 4)],
                                          hip_peak_bytes_forward_backward=hip_peak, list_len_median=int(cnt.median()),
                                          list_len_max=int(cnt.max()), rows_empty=int((cnt == 0).sum()),
                                          rows_chunked=int((cnt > CHUNK).sum()), chunks=int(chunks.sum()),
                                          chunk_bound=n_pts * n_hyp * 8 // CHUNK + N, present_slots=int(cnt.sum()))), flush=True)
                    continue
                out = None

                def forward():
                    gathered = feats[rows.clamp(min=0)] * (rows >= 0).float().unsqueeze(-1)          # [nq, 8, C]
                    return (gathered * wgt.unsqueeze(-1)).sum(dim=1).view(n_pts, n_hyp, C)
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats(dev)
                before = torch.cuda.memory_allocated(dev)
                out_t = forward()
                (g_torch,) = torch.autograd.grad(out_t, feats, g, retain_graph=True)
                torch.cuda.synchronize()
                peak = torch.cuda.max_memory_allocated(dev) - before
                med, lo, hi = timed(lambda: torch.autograd.grad(out_t, feats, g, retain_graph=True), args.warmup, args.repeats)
                diff = float((g_torch - g_hip).abs().max()) / float(g_torch.abs().max())
                print(json.dumps(dict(base, torch_backward_ms=round(med, 3), torch_backward_ms_min_max=[round(lo, 3), round(hi, 3)],
                                      torch_peak_bytes_forward_backward=peak, hip_peak_bytes_forward_backward=hip_peak,
                                      max_abs_diff_over_max_abs=diff)), flush=True)
                out_t = g_torch = None


def driver(args):
    out = args.out or os.path.join(ROOT, 'build', 'bench_sparse_interp_backward')
    os.makedirs(out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), '--cfg', args.cfg, '--views', args.views, '--repeats', str(args.repeats),
          '--warmup', str(args.warmup), '--ns', args.ns, '--offset', str(args.offset)] + \
        (['--edge-len', str(args.edge_len)] if args.edge_len else [])
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
            sys.exit('bench_sparse_interp_backward.py: step %s ended with status %d; nothing more is started' % (name, p.returncode))
    with open(os.path.join(out, 'bench_sparse_interp_backward.json'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    rec = [json.loads(ln) for ln in lines]
    key = lambda r: (r['views'], r['n_hyp'], r['stride'])
    for hp in (r for r in rec if r['step'] == 'hip'):
        to = next(r for r in rec if r['step'] == 'torch' and key(r) == key(hp))
        print('%d views, n_hyp %d, stride %d (%d rows, C = %d): HIP backward %.3f ms, stock torch %.3f ms (%.1f x); peak %.1f MB against '
              '%.1f MB; lists median %d max %d, %d rows in %d chunks'
              % (hp['views'], hp['n_hyp'], hp['stride'], hp['rows'], hp['C'], hp['hip_backward_ms'], to['torch_backward_ms'],
                 to['torch_backward_ms'] / hp['hip_backward_ms'], hp['hip_peak_bytes_forward_backward'] / 2 ** 20,
                 to['torch_peak_bytes_forward_backward'] / 2 ** 20, hp['list_len_median'], hp['list_len_max'], hp['rows_chunked'],
                 hp['chunks']), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default='cfg2')
    ap.add_argument('--views', default='14,64')
    ap.add_argument('--ns', default='0,3')
    ap.add_argument('--offset', type=float, default=0.05)
    ap.add_argument('--edge-len', type=float, help="voxel size of the scene model (default: the cfg's)")
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
