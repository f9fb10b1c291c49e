#!/usr/bin/env python3
"""Forward + backward of PointNet: the HIP route (3dvnet_amd/training.py: pointnet -> v3d_segment_max_arg_f32, v3d_segment_sum_f32,
v3d_pointnet_pool_backward_f32 beside torch.mm) against the stock graph on the device (scatter_reduce('amax') + cat + F.linear and
autograd from there, which keeps cat(x, pool[idx]) [Np, 2H] three times and sums the pooled gradients with index_add atomics), and
each of the three kernels against its stock-op equivalent.

    python scripts/bench_pointnet_backward.py [--cfg cfg3] [--views 64] [--repeats 10] [--warmup 2] [--out DIR]

The input is the PointNet input of the project's own scene model on a synthetic scene (cfg cameras and edges, analytic wall depth +
2 cm noise at the cfg's depth size, synthetic weights): 200 704 points x 35 columns at cfg3 with 64 views, hidden width 128.

Every figure is the median over three runs that alternate between the two routes (HIP, stock, HIP, stock, ...), each run the
median of --repeats samples; a sample is ONE call between two device synchronisations (launches and synchronisation included).
The spread is the smallest and the largest of the three run medians.  Peak memory is torch.cuda.max_memory_allocated over one
forward + backward, above what was allocated before.  One JSON line per measurement; they land in OUT/bench_pointnet_backward.json.
A record, no gate.
"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, repeats):
    """median wall-clock milliseconds of fn() between two device synchronisations"""
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
    return sorted(ms)[len(ms) // 2]


def alternating(fns, warmup, repeats, runs=3):
    """{name: fn} -> {name: (median, min, max) of the run medians}, the routes taking turns"""
    got = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            got[k].append(timed(fn, warmup, repeats))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in got.items()}


def peak_bytes(fn, dev):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    del out
    return peak


def stock_pointnet(pn, x, idx, n_idx):
    """scenemodeling.py:127-144 as the reference writes it, torch's scatter_reduce in place of torch_scatter's"""
    import torch
    import torch.nn.functional as F
    e = idx.view(-1, 1).expand(-1, pn.hidden_dim)
    pool = lambda t: t.new_zeros((n_idx, t.shape[1])).scatter_reduce(0, e, t, 'amax', include_self=False)
    y = pn.fc1(F.relu(pn.fc_pos(x)))
    for fc in (pn.fc2, pn.fc3, pn.fc4):
        y = fc(F.relu(torch.cat((y, pool(y)[idx]), dim=1)))
    return pn.fc_out(F.relu(pool(y)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cfg', default='cfg3')
    ap.add_argument('--views', type=int, default=64)
    ap.add_argument('--repeats', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('bench_pointnet_backward.py measures on a HIP device; none is visible')
    dev = torch.device('cuda:0')
    syn = importlib.import_module('3dvnet_amd.synthetic')
    lm = importlib.import_module('3dvnet_amd.lightningmodel')
    tr = importlib.import_module('3dvnet_amd.training')
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
    pn = net.pointnet
    rot, tv, K, edges, feat = (inp[k].to(dev) for k in ('rotmats', 'tvecs', 'K', 'edges', 'feat'))
    seen = {}
    hook = pn.register_forward_pre_hook(lambda mod, a: seen.update(x=a[0], idx=a[1], n_idx=a[2]))
    with torch.no_grad():
        net.model_scene(depth, torch.zeros(n_ref, dtype=torch.long, device=dev), feat, rot, tv, K, edges)
    hook.remove()
    x = seen['x'].detach().clone().requires_grad_(True)
    idx, n_idx = seen['idx'].contiguous(), int(seen['n_idx'])
    Np, H = x.shape[0], pn.hidden_dim
    counts = torch.bincount(idx, minlength=n_idx)
    common = dict(bench='pointnet_backward', cfg=args.cfg, views=n_ref, repeats=args.repeats, precision=pn.precision, points=Np,
                  voxels=n_idx, hidden=H, points_per_voxel_median=float(counts.float().median()), points_per_voxel_max=int(counts.max()))
    lines = []

    def emit(**rec):
        lines.append(json.dumps(dict(common, **rec)))
        print(lines[-1], flush=True)

    # ---- the whole function ------------------------------------------------------------------------------------------------------
    params = list(pn.parameters())
    routes = {'hip': lambda: tr.pointnet(pn, x, idx, n_idx), 'stock': lambda: stock_pointnet(pn, x, idx, n_idx)}
    fwd_bwd = {k: (lambda f=f: torch.autograd.grad(f().square().mean(), [x] + params)) for k, f in routes.items()}
    peaks = {k: peak_bytes(f, dev) for k, f in fwd_bwd.items()}
    # how far the two routes' gradients lie apart (largest max-norm relative difference over the 13).  They are two different
    # functions wherever a ReLU argument or a winner / runner-up gap lies within the forward's rounding: 'split_bf16' carries 2^-16
    # per product, so that is measured in precision 'fp32' as well
    def route_difference():
        g_hip, g_stock = fwd_bwd['hip'](), fwd_bwd['stock']()
        return max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(g_hip, g_stock))
    diff = route_difference()
    prec = pn.precision
    pn.precision = 'fp32'
    try:
        diff_fp32 = route_difference()
    finally:
        pn.precision = prec
    for k, (med, lo, hi) in alternating(fwd_bwd, args.warmup, args.repeats).items():
        emit(what='pointnet forward + backward', route=k, ms=round(med, 3), ms_min_max=[round(lo, 3), round(hi, 3)], peak_bytes=peaks[k],
             max_gradient_difference_between_the_routes=diff, max_gradient_difference_in_precision_fp32=diff_fp32)

    # ---- the three kernels against their stock-op equivalents ---------------------------------------------------------------------
    gen = torch.Generator().manual_seed(11)
    st = libm.stream_ptr(dev)
    idx32 = idx.to(torch.int32).contiguous()
    perm = torch.empty(Np, dtype=torch.int32, device=dev)
    offs = torch.empty(n_idx + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.v3d_segment_csr_workspace_bytes(Np), dtype=torch.uint8, device=dev)
    libm.check(lib.v3d_segment_csr(idx32.data_ptr(), Np, n_idx, perm.data_ptr(), offs.data_ptr(), ws.data_ptr(), ws.numel(), st), 'csr')
    act = torch.randn((Np, H), generator=gen).to(dev)
    g_lin = torch.randn((Np, H), generator=gen).to(dev)
    g_pool = torch.randn((n_idx, H), generator=gen).to(dev)
    pool = torch.empty((n_idx, H), device=dev)
    arg = torch.empty((n_idx, H), dtype=torch.int32, device=dev)
    out_rows = torch.empty((Np, H), device=dev)
    e = idx.view(-1, 1).expand(-1, H)

    def max_arg():
        libm.check(lib.v3d_segment_max_arg_f32(act.data_ptr(), H, perm.data_ptr(), offs.data_ptr(), n_idx, H, pool.data_ptr(), H,
                                               arg.data_ptr(), H, st), 'v3d_segment_max_arg_f32')

    def max_only():
        libm.check(lib.v3d_segment_max_f32(act.data_ptr(), H, perm.data_ptr(), offs.data_ptr(), n_idx, H, pool.data_ptr(), H, st),
                   'v3d_segment_max_f32')

    def seg_sum():
        libm.check(lib.v3d_segment_sum_f32(act.data_ptr(), H, perm.data_ptr(), offs.data_ptr(), n_idx, H, pool.data_ptr(), H, st),
                   'v3d_segment_sum_f32')

    def pool_bwd():
        libm.check(lib.v3d_pointnet_pool_backward_f32(g_lin.data_ptr(), H, act.data_ptr(), H, idx32.data_ptr(), g_pool.data_ptr(), H,
                                                      arg.data_ptr(), H, Np, H, out_rows.data_ptr(), H, st),
                   'v3d_pointnet_pool_backward_f32')
    max_arg()
    arg64 = arg.long().clamp(min=0)                                            # (every voxel of a scene holds a point)
    pairs = {
        'segment_max_arg': {'hip': max_arg, 'hip_max_without_arg': max_only,
                            'stock': lambda: torch.zeros((n_idx, H), device=dev).scatter_reduce(0, e, act, 'amax', include_self=False)},
        'segment_sum': {'hip': seg_sum, 'stock': lambda: torch.zeros((n_idx, H), device=dev).index_add_(0, idx, act)},
        'pool_backward': {'hip': pool_bwd,
                          'stock': lambda: (g_lin * (act > 0)).scatter_add_(0, arg64, g_pool)},
    }
    for name, fns in pairs.items():
        for k, (med, lo, hi) in alternating(fns, args.warmup, args.repeats).items():
            emit(what=name, route=k, ms=round(med, 4), ms_min_max=[round(lo, 4), round(hi, 4)])
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'bench_pointnet_backward.json'), 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
