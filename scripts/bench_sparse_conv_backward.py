#!/usr/bin/env python3
"""Backward of the sparse convolutions: the HIP route (3dvnet_amd/training.py: SparseConv -> v3d_sparse_conv_weight_grad_f32 for
the kernel, v3d_sparse_conv_f32 over the inverse table for the input) against the same gradients through stock torch ops on the
device: 27 x index_select + matmul per convolution and autograd from there (which keeps the 27 gathered copies).

    python scripts/bench_sparse_conv_backward.py [--cfg cfg3] [--views 64] [--repeats 10] [--warmup 2] [--out DIR]

The levels are those of the project's own SparseUNet on a synthetic scene (cfg cameras and edges, analytic wall depth + 2 cm noise
at the cfg's depth size, synthetic PointNet / U-Net weights): about 60 k x 64, 13 k x 128 and 2.7 k x 128 rows for cfg3 with 64 views.

Without --step this is a driver: every GPU step runs as a child process of its own under `timeout`, in sequence, and the first
step that fails ends the run.
  --step hip     per level, for a same-level convolution C -> C: median wall time of the weight-gradient call (dW), of the
                 input-gradient call with the transposed pack built before (dx), of both packings (the host round trip of the
                 kernel: PackedGemm of the kernel and of its transpose), of the whole Function.backward (packing included) and the
                 peak memory over forward + backward; the present share of the table.  Then the whole training.sparse_unet forward
                 + backward: time, peak memory, the time of packing all its kernels both ways (what a step pays on the host), and
                 the time of the same in precision 'fp32'; the dW call again with developer option wgrad_compact = 0.
  --step torch   the same figures of the stock float32 route, and the largest difference between the two routes' gradients.
Every timed sample is ONE call between two device synchronisations: it includes the launches and the synchronisation itself, not
kernel time alone.  One JSON line per shape and step; they land in OUT/bench_sparse_conv_backward.json.  A record, no gate.
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


def stock_conv(x, kernel, nbr):
    import torch
    xp = torch.cat((x.new_zeros((1, x.shape[1])), x), dim=0)                  # row 0: the zero row of an absent neighbour
    return sum(xp.index_select(0, nbr[k].long() + 1) @ kernel[k] for k in range(nbr.shape[0]))


def stock_unet(unet, feats, xs):
    """training.sparse_unet with stock_conv in place of SparseConv"""
    import torch
    import torch.nn.functional as F
    levels = [x['sparse'] for x in xs][::-1]
    n_lv = len(levels)
    same = [lv.neighbors(lv.coords, lv.stride) for lv in levels]
    down = [None] + [levels[i - 1].neighbors(levels[i].coords, levels[i - 1].stride) for i in range(1, n_lv)]
    up = [None] + [levels[i].neighbors(levels[i - 1].coords, -levels[i - 1].stride) for i in range(1, n_lv)]
    gn = lambda m, y: F.group_norm(y, m.gn.num_groups, m.gn.weight, m.gn.bias, m.gn.eps)
    layer = lambda seq, x, nbr: F.relu(gn(seq[1], stock_conv(x, seq[0].kernel, nbr)))

    def residual(blk, x, nbr):
        y = F.relu(gn(blk.n1, stock_conv(x, blk.conv1.kernel, nbr)))
        return F.relu(gn(blk.n2, stock_conv(y, blk.conv2.kernel, nbr)) + x)
    x, skips = feats, []
    for i in range(n_lv):
        if i > 0:
            x = layer(unet.down[i - 1], x, down[i])
        for blk in unet.res_down[i]:
            x = residual(blk, x, same[i])
        skips.append(x)
    out = [x]
    for j in range(n_lv - 1):
        i = n_lv - 1 - j
        u = layer(unet.up[j], x, up[i])
        adj = unet.feat_adj[j]
        x = F.relu(gn(adj[1], torch.cat((u, skips[i - 1]), dim=1) @ adj[0].kernel))
        for blk in unet.res_up[j]:
            x = residual(blk, x, same[i - 1])
        out.append(x)
    return out


def step(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_sparse_conv_backward.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    syn = importlib.import_module('3dvnet_amd.synthetic')
    lm = importlib.import_module('3dvnet_amd.lightningmodel')
    tr = importlib.import_module('3dvnet_amd.training')
    sm = importlib.import_module('3dvnet_amd.scenemodeling')
    libm = importlib.import_module('3dvnet_amd._lib')
    lib = libm.load()
    n_ref = args.views
    inp = syn.make_costvolume_inputs(args.cfg, n_ref, feat_dim=32)
    (h, w), img_size = inp['plane_size'], inp['img_size']
    refs = torch.unique(inp['edges'][0])
    depth = syn.ray_box_depth(inp['rotmats'][refs], inp['tvecs'][refs], inp['K'][refs], img_size, (h, w))
    depth = (depth + 0.02 * torch.randn(depth.shape, generator=torch.Generator().manual_seed(7))).to(dev).contiguous()
    net = lm.PL3DVNet(None, {'depth_start': .5, 'depth_interval': .05, 'n_intervals': 96, 'size': (h, w)}, inp['edge_len'],
                      feat_dim=32, img_size=img_size).eval()
    net.pointnet.load_state_dict(syn.pointnet_weights())
    net.sparse_conv.load_state_dict(syn.sparse_unet_weights())
    net = net.to(dev)
    unet = net.sparse_conv
    rot, tv, K, edges, feat = (inp[k].to(dev) for k in ('rotmats', 'tvecs', 'K', 'edges', 'feat'))
    seen = {}
    hook = unet.register_forward_pre_hook(lambda mod, a: seen.update(F=a[0]))
    with torch.no_grad():
        xs = net.model_scene(depth, torch.zeros(n_ref, dtype=torch.long, device=dev), feat, rot, tv, K, edges)
    hook.remove()
    gen = torch.Generator().manual_seed(11)
    prec = unet.precision
    common = dict(bench='sparse_conv_backward', step=args.step, cfg=args.cfg, views=n_ref, repeats=args.repeats, precision=prec)
    for x in xs[::-1]:
        lv = x['sparse']
        M, C = x['feats'].shape
        nbr = lv.neighbors(lv.coords, lv.stride)
        inv = nbr.flip(0).contiguous()
        base = dict(common, rows=M, C=C, stride=int(x['stride']), present_share=round(float((nbr >= 0).float().mean()), 4))
        xin = x['feats'].detach().clone().requires_grad_(True)
        kernel = (torch.randn((27, C, C), generator=gen) / (27 * C) ** 0.5).to(dev).requires_grad_(True)
        g = torch.randn((M, C), generator=gen).to(dev)
        y = gx = gw = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        if args.step == 'hip':
            y = tr.sparse_conv(xin, kernel, nbr, inv, prec)
        else:
            y = stock_conv(xin, kernel, nbr)
        gx, gw = torch.autograd.grad(y, (xin, kernel), g, retain_graph=True)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated(dev) - before
        both, lo, hi = timed(lambda: torch.autograd.grad(y, (xin, kernel), g, retain_graph=True), args.warmup, args.repeats)
        rec = dict(base, backward_ms=round(both, 4), backward_ms_min_max=[round(lo, 4), round(hi, 4)], peak_bytes_forward_backward=peak)
        if args.step == 'hip':
            xc = xin.detach()
            nbytes = lib.v3d_sparse_conv_weight_grad_workspace_bytes(M, 27, C, C)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            dw = torch.empty((27, C, C), device=dev)
            s = libm.stream_ptr(dev)
            dw_ms = timed(lambda: libm.check(lib.v3d_sparse_conv_weight_grad_f32(xc.data_ptr(), C, nbr.data_ptr(), M, 27, g.data_ptr(), C, M, C, C,
                                                                                 dw.data_ptr(), ws.data_ptr(), nbytes, s), 'dW'),
                          args.warmup, args.repeats)
            pack_t = sm.PackedGemm(kernel.detach(), C * C, C, 1, 27, C, C, device=dev)
            dx = torch.empty((M, C), device=dev)
            dx_ms = timed(lambda: libm.check(lib.v3d_sparse_conv_f32(pack_t.handle, M, g.data_ptr(), C, inv.data_ptr(), M, 0, 0.0, None, 0, 0,
                                                                     dx.data_ptr(), C, libm.precision_code(prec), s), 'dx'),
                          args.warmup, args.repeats)
            pack_ms = timed(lambda: (sm.PackedGemm(kernel.detach(), C * C, 1, C, 27, C, C, device=dev),
                                     sm.PackedGemm(kernel.detach(), C * C, C, 1, 27, C, C, device=dev)), args.warmup, args.repeats)
            libm.set_option('wgrad_compact', 0)                       # the same call with every row staged, absent ones as zeros
            try:
                nc_ms = timed(lambda: libm.check(lib.v3d_sparse_conv_weight_grad_f32(xc.data_ptr(), C, nbr.data_ptr(), M, 27, g.data_ptr(), C, M,
                                                                                     C, C, dw.data_ptr(), ws.data_ptr(), nbytes, s), 'dW'),
                              args.warmup, args.repeats)
            finally:
                libm.set_option('wgrad_compact', 1)
            rec.update(dw_no_compaction_ms=round(nc_ms[0], 4), dw_no_compaction_ms_min_max=[round(nc_ms[1], 4), round(nc_ms[2], 4)])
            rec.update(dw_ms=round(dw_ms[0], 4), dw_ms_min_max=[round(dw_ms[1], 4), round(dw_ms[2], 4)], dx_ms=round(dx_ms[0], 4),
                       dx_ms_min_max=[round(dx_ms[1], 4), round(dx_ms[2], 4)], pack_both_ms=round(pack_ms[0], 4),
                       dw_workspace_bytes=nbytes, dw_gflop=round(2 * 27 * M * C * C * base['present_share'] / 1e9, 3))
        else:
            hx, hw = torch.autograd.grad(tr.sparse_conv(xin, kernel, nbr, inv, prec), (xin, kernel), g)
            rec.update(max_abs_diff_over_max_abs_dx=float((hx - gx).abs().max() / gx.abs().max()),
                       max_abs_diff_over_max_abs_dw=float((hw - gw).abs().max() / gw.abs().max()))
            hx = hw = None
        print(json.dumps(rec), flush=True)
        y = gx = gw = None
    # ---- the whole U-Net, forward + backward ---------------------------------------------------------------------------------------
    feats = seen['F'].detach().clone().requires_grad_(True)
    params = list(unet.parameters())
    fn = (lambda: tr.sparse_unet(unet, feats, xs)) if args.step == 'hip' else (lambda: stock_unet(unet, feats, xs))

    def fwd_bwd():
        level = fn()
        loss = sum(f.square().mean() for f in level)
        return torch.autograd.grad(loss, [feats] + params)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    fwd_bwd()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    med, lo, hi = timed(fwd_bwd, args.warmup, args.repeats)
    rec = dict(common, what='sparse_unet forward + backward', rows=[int(x['feats'].shape[0]) for x in xs], unet_ms=round(med, 3),
               unet_ms_min_max=[round(lo, 3), round(hi, 3)], peak_bytes=peak)
    if args.step == 'hip':
        kernels = [p for n, p in unet.named_parameters() if n.endswith('kernel') and p.dim() == 3]

        def pack_all():
            for k in kernels:
                _, ci, co = k.shape
                sm.PackedGemm(k.detach(), ci * co, 1, co, 27, co, ci, device=dev)
                sm.PackedGemm(k.detach(), ci * co, co, 1, 27, ci, co, device=dev)
        pk = timed(pack_all, args.warmup, args.repeats)
        rec.update(pack_all_ms=round(pk[0], 3), pack_all_ms_min_max=[round(pk[1], 3), round(pk[2], 3)], n_kernels=len(kernels))
    if args.step == 'hip' and prec != 'fp32':
        # the exact mode: the forward of a convolution is nine calls of three offsets (training.SparseConv)
        unet.precision = 'fp32'
        try:
            med, lo, hi = timed(fwd_bwd, args.warmup, args.repeats)
        finally:
            unet.precision = prec
        rec.update(unet_fp32_ms=round(med, 3), unet_fp32_ms_min_max=[round(lo, 3), round(hi, 3)])
    print(json.dumps(rec), flush=True)


def driver(args):
    out = args.out or os.path.join(ROOT, 'build', 'bench_sparse_conv_backward')
    os.makedirs(out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__), '--cfg', args.cfg, '--views', str(args.views), '--repeats', str(args.repeats),
          '--warmup', str(args.warmup), '--out', out]
    lines = []
    for name, limit in (('hip', 240), ('torch', 300)):
        cmd = ['timeout', '-k', '10', str(limit)] + me + ['--step', name]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        for ln in p.stdout.splitlines():
            if ln.startswith('{'):
                print(ln, flush=True)
                lines.append(ln)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-4000:])
            sys.exit('bench_sparse_conv_backward.py: step %s ended with status %d; nothing more is started' % (name, p.returncode))
    with open(os.path.join(out, 'bench_sparse_conv_backward.json'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    for r in [json.loads(ln) for ln in lines]:
        if 'what' in r:
            print('%s, %s: %.1f ms, peak %.0f MB%s' % (r['what'], r['step'], r['unet_ms'], r['peak_bytes'] / 2 ** 20,
                                                      ', packing all kernels both ways %.1f ms, precision fp32 %.1f ms' % (r['pack_all_ms'], r.get('unet_fp32_ms', float('nan'))) if 'pack_all_ms' in r else ''))
        else:
            print('%s: %d rows x %d: backward %.3f ms, peak %.1f MB%s' % (
                r['step'], r['rows'], r['C'], r['backward_ms'], r['peak_bytes_forward_backward'] / 2 ** 20,
                ' (dW %.3f ms, without compaction %.3f ms, dx %.3f ms, packing %.3f ms)' % (r['dw_ms'], r['dw_no_compaction_ms'], r['dx_ms'], r['pack_both_ms']) if 'dw_ms' in r else ''))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default='cfg3')
    ap.add_argument('--views', type=int, default=64)
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
