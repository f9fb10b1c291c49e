#!/usr/bin/env python3
"""Developer check: SHA-256 of the gather-GEMM's outputs for seeded inputs, one line per case -- run on two builds (before and
after a change that must not move a bit: a refactor of csrc/gemm_*.hip) and compare.  Only PackedGemm, v3d_sparse_conv_f32 and
set_option are used, so the file runs unchanged on older trees.  The cases reach every kernel of the family and every
instantiation the kernel choice has:
  sparse   27 offsets over one source (v3d_sparse_conv_f32), GroupNorm + residual + ReLU, one offset wholly absent, ragged last
           tile; each shape on the pipeline, the rounds and the one-step kernel (gemm_rounds / gemm_pipe); M around the 8192-row
           switch to 64-row tiles; K = 96 (three K chunks); N = 32 with 8-channel groups
  dense    identity + gathered segment with -1 rows, ReLU-in, bias, GroupNorm, scatter-max (the generic epilogue); N = 20; a row
           stride that is no multiple of 4 (scalar gather); exact fp32; 131 072 rows x K = 35 (128-row tiles)
  conv1d   groups of 7 rows: N = 20, groups straddling 32-row tiles, the 64- and 128-row tiles of large M, and a source view
           that is not 16-byte aligned (falls back to the one-step kernel)

    python scripts/gemm_hash.py [--json OUT]
"""
import hashlib
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sm = importlib.import_module('3dvnet_amd.scenemodeling')
libm = importlib.import_module('3dvnet_amd._lib')
lib = libm.load()
dev = torch.device('cuda:0')
hashes = {}


def record(name, *tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for x in tensors:
        h.update(x.cpu().numpy().tobytes())
    hashes[name] = h.hexdigest()
    print(name, hashes[name][:16], float(tensors[0].double().abs().sum()))


# ---- sparse convolutions ------------------------------------------------------------------------------------------------------
for M, C, N in ((33, 64, 32), (777, 32, 128), (8191, 128, 128), (8192, 64, 64), (8200, 96, 64)):
    g = torch.Generator().manual_seed(M)
    gn = 8 if N == 32 else 16
    pk = sm.PackedGemm(torch.randn(27, C, N, generator=g) * 0.05, C * N, 1, N, 27, N, C, gn_w=torch.rand(N, generator=g) + 0.5,
                       gn_b=torch.randn(N, generator=g) * 0.1, gn_group=gn)
    x = torch.randn(M, C, generator=g).to(dev)
    nbr = (torch.arange(M)[None, :] + torch.randint(-50, 51, (27, M), generator=g)).clamp_(0, M - 1)
    nbr[torch.rand(27, M, generator=g) < 0.6] = -1
    nbr[5] = -1                                    # an offset no row of any tile has
    nbr[13] = torch.arange(M)
    nbr = nbr.to(torch.int32).to(dev).contiguous()
    res = torch.randn(M, N, generator=g).to(dev)
    for rounds, pipe in ((1, 1), (1, 0), (0, 0)):
        old, old_p = libm.set_option('gemm_rounds', rounds), libm.set_option('gemm_pipe', pipe)
        out = torch.empty(M, N, device=dev)
        rc = lib.v3d_sparse_conv_f32(pk.handle, M, x.data_ptr(), C, nbr.data_ptr(), M, gn, 1e-5, res.data_ptr(), N, 1, out.data_ptr(),
                                     N, libm.precision_code('split_bf16'), libm.stream_ptr(dev))
        libm.set_option('gemm_rounds', old), libm.set_option('gemm_pipe', old_p)
        libm.check(rc, 'v3d_sparse_conv_f32')
        record('sparse M=%d K=%d N=%d gn=%d rounds=%d pipe=%d' % (M, C, N, gn, rounds, pipe), out)


# ---- dense, one-step kernel ------------------------------------------------------------------------------------------------------
def dense(name, M, K, N, R, seed, use_gn=True, ld0=None, precision='split_bf16', pooled=True):
    g = torch.Generator().manual_seed(seed)
    ld0 = ld0 or K
    x0 = torch.randn(M, ld0, generator=g).to(dev)                    # the identity segment reads columns 0..K-1 of rows of ld0 floats
    x1 = torch.randn(R, K, generator=g).to(dev)
    idx = torch.randint(-1, R, (M,), generator=g).int().to(dev)
    W = torch.randn(N, 2 * K, generator=g) * 0.2
    bias = torch.randn(N, generator=g)
    gw, gb = (torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)) if use_gn else (None, None)
    pk = sm.PackedGemm(W, K, 2 * K, 1, 2, N, K, bias=bias, gn_w=gw, gn_b=gb)
    pool = torch.full((17, N), float('-inf'), device=dev) if pooled else None
    pidx = torch.randint(0, 17, (M,), generator=g).int().to(dev) if pooled else None
    out = pk(M, [x0, x1], idxs=[None, idx], lds=[ld0, K], relu_in=True, use_gn=use_gn, relu_out=True, pool=pool, pool_idx=pidx,
             precision=precision)
    record(name, out, *([pool] if pooled else []))


dense('dense M=333 K=48 N=64', 333, 48, 64, 200, 0)
dense('dense M=333 K=48 N=20', 333, 48, 20, 200, 1, use_gn=False)               # GroupNorm needs N % 16 == 0
dense('dense M=333 K=48 N=64 ld=50', 333, 48, 64, 200, 2, ld0=50)
dense('dense M=333 K=48 N=64 fp32', 333, 48, 64, 200, 3, precision='fp32')
dense('dense M=131072 K=35 N=128', 131072, 35, 128, 5000, 4, use_gn=False, pooled=False)


# ---- conv1d over groups of 7 rows -------------------------------------------------------------------------------------------------
def conv1d(name, M, K, N, seed, misalign=False):
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(M * K + 1, generator=g).to(dev)
    x = flat[1:].view(M, K) if misalign else flat[:M * K].view(M, K)          # [1:]: 4 bytes off a 16-byte boundary
    pk = sm.PackedGemm(torch.randn(N, K, 3, generator=g) * 0.2, 1, 3 * K, 3, 3, N, K, bias=torch.randn(N, generator=g))
    record(name, pk(M, [x, x, x], group_len=7, relu_out=True))


conv1d('conv1d M=35 K=48 N=20', 35, 48, 20, 10)
conv1d('conv1d M=259 K=128 N=128', 7 * 37, 128, 128, 11)
conv1d('conv1d M=131075 K=64 N=128', 131075 - 131075 % 7, 64, 128, 12)
conv1d('conv1d M=131075 K=64 N=64', 131075 - 131075 % 7, 64, 64, 13)
conv1d('conv1d M=259 K=128 N=128 misaligned', 7 * 37, 128, 128, 14, misalign=True)

if '--json' in sys.argv:
    with open(sys.argv[sys.argv.index('--json') + 1], 'w') as f:
        json.dump(hashes, f, indent=1)
