"""The gather-GEMM family (csrc/gemm_*.hip) at small sizes against a float64 torch reference, for the paths that the parity tests
only reach inside a network or kernel against kernel: 8-channel GroupNorm groups, the scalar gather of a source whose row stride
is no multiple of 4, the exact-fp32 matrix path, and the conv1d kernel with row groups straddling its 32-row tiles.

Tolerance: 1e-5 * max|ref|, the bound of test_scene_gpu.py::test_gather_gemm_unit for this family at these K (split-bf16 products
carry 16 mantissa bits per operand, ~7e-6 relative layer error)."""
import numpy as np
import pytest
import torch

from conftest import v3d

pytestmark = pytest.mark.gpu


def _close(a, b, rel):
    a, b = np.asarray(a), np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=0, atol=rel * max(float(np.abs(b).max()), 1e-12))


def test_sparse_conv_with_8_channel_groupnorm_groups(cuda):
    """27 offsets, N = 32 with use_gn = 8 (SparseUNet's first level), absent neighbours, one offset wholly absent, a ragged 32-row
    tile, residual + ReLU."""
    sm = v3d('scenemodeling')
    M, C, N = 33, 64, 32
    g = torch.Generator().manual_seed(33)
    w = torch.randn(27, C, N, generator=g) * 0.05
    gn_w, gn_b = torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g) * 0.1
    x = torch.randn(M, C, generator=g)
    nbr = torch.randint(0, M, (27, M), generator=g)
    nbr[torch.rand(27, M, generator=g) < 0.6] = -1
    nbr[5] = -1
    nbr[13] = torch.arange(M)
    res = torch.randn(M, N, generator=g)
    y = torch.zeros(M, N, dtype=torch.float64)
    for k in range(27):
        rows = torch.where((nbr[k] >= 0).unsqueeze(1), x.double()[nbr[k].clamp(min=0)], torch.zeros(M, C, dtype=torch.float64))
        y += rows @ w[k].double()
    y = torch.relu(torch.nn.functional.group_norm(y, N // 8, gn_w.double(), gn_b.double(), 1e-5) + res.double())
    pk = sm.PackedGemm(w, C * N, 1, N, 27, N, C, gn_w=gn_w, gn_b=gn_b, gn_group=8)
    nbr_d = nbr.to(torch.int32).to(cuda).contiguous()
    out = pk(M, [x.to(cuda)] * 27, idxs=[nbr_d[k] for k in range(27)], use_gn=True, residual=res.to(cuda), relu_out=True)
    _close(out.cpu(), y, rel=1e-5)


@pytest.mark.parametrize('ld0,precision', [(50, 'split_bf16'), (48, 'fp32')], ids=['unaligned_stride', 'fp32'])
def test_dense_two_segments(ld0, precision, cuda):
    """Identity + gathered segment with -1 rows, ReLU-in, bias, GroupNorm, ReLU, scatter-max: with a row stride of 50 floats (no
    16-byte loads: the scalar gather) and on the exact-fp32 matrix instructions."""
    sm = v3d('scenemodeling')
    M, K, N, R = 333, 48, 64, 200
    g = torch.Generator().manual_seed(ld0)
    x0 = torch.randn(M, ld0, generator=g)
    x1 = torch.randn(R, K, generator=g)
    idx = torch.randint(-1, R, (M,), generator=g).int()
    W = torch.randn(N, 2 * K, generator=g) * 0.2
    bias, gw, gb = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5, torch.randn(N, generator=g)
    pidx = torch.randint(0, 17, (M,), generator=g).int()
    gathered = torch.where((idx >= 0).unsqueeze(1), x1[idx.clamp(min=0).long()], torch.zeros(M, K))
    y = torch.relu(torch.cat((x0[:, :K], gathered), 1).double()) @ W.double().t() + bias.double()
    y = torch.relu(torch.nn.functional.group_norm(y, N // 16, gw.double(), gb.double(), 1e-5))
    pool_ref = torch.full((17, N), float('-inf'), dtype=torch.float64).scatter_reduce_(0, pidx.long().view(-1, 1).expand(-1, N), y, 'amax')
    pk = sm.PackedGemm(W, K, 2 * K, 1, 2, N, K, bias=bias, gn_w=gw, gn_b=gb)
    pool = torch.full((17, N), float('-inf'), device=cuda)
    out = pk(M, [x0.to(cuda), x1.to(cuda)], idxs=[None, idx.to(cuda)], lds=[ld0, K], relu_in=True, use_gn=True, relu_out=True,
             pool=pool, pool_idx=pidx.to(cuda), precision=precision)
    _close(out.cpu(), y, rel=1e-5)
    _close(pool.cpu(), pool_ref, rel=1e-5)


def test_conv1d_groups_straddle_the_tiles(cuda):
    """Conv1d(k = 3, pad 1) over 37 groups of 7 rows, K = N = 128: 32-row tiles, so groups start and end inside tiles and the
    halo rows of a tile belong to a neighbouring group or tile."""
    sm = v3d('scenemodeling')
    K = N = 128
    g = torch.Generator().manual_seed(7)
    Wc = torch.randn(N, K, 3, generator=g) * 0.2
    bias = torch.randn(N, generator=g)
    xin = torch.randn(7 * 37, K, generator=g)
    yref = torch.nn.functional.conv1d(xin.double().view(37, 7, K).transpose(2, 1), Wc.double(), bias.double(), 1, 1)
    yref = yref.transpose(2, 1).reshape(7 * 37, N)
    pk = sm.PackedGemm(Wc, 1, 3 * K, 3, 3, N, K, bias=bias)
    xg = xin.to(cuda)
    _close(pk(7 * 37, [xg, xg, xg], group_len=7).cpu(), yref, rel=1e-5)
