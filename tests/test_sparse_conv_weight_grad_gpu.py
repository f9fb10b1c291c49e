"""GPU: v3d_sparse_conv_weight_grad_f32 (csrc/gemm_wgrad.hip) through the C ABI, per element against
tests/sparse_conv_backward_oracle.py (float64 sums over the tables of tests/sparse_oracle.py; pinned on the CPU by
tests/test_sparse_conv_backward_oracle.py):

  * sizes M = 2 R + 37 (three chunks, the last one ragged), 1 and 0 with R = 512 rows per chunk (restated from the source line
    cited below) x the channel pairs (16, 16), (16, 32), (32, 16), (64, 128), (128, 128) on a same-level table of a random two-batch
    occupancy map; a down and an up table (n_in != n_out) of the same map;
  * a map of isolated voxels on a stride-3 lattice: only offset 13 is present, the 26 other slabs are +0 bit for bit;
  * every case runs with ld_src > K and ld_grad > N, NaN in the unused columns and in every src row no table entry names, into a
    NaN-filled grad_w and a 0xFF-filled workspace: every element is finite and within (cnt_k + 32) * 2^-24 * S of the float64 sum;
  * two calls (workspaces of 0xFF and of 0x00) give the same bits; contiguous rows give the bits of the wide rows;
  * developer option wgrad_compact = 0 (no compaction) meets the same bound;
  * K = 24, N = 144, n_seg = 28, M > 2^30, a workspace one byte short, a null pointer, ld_src < K, ld_grad < N and nbr_stride < M each return
    their error code and leave grad_w untouched.

The worst ratio to the bound is printed per case; DESIGN.md 4.1e records the values measured on an MI355X.  No number here comes
from the kernel under test.
"""
import os

import numpy as np
import pytest
import torch

import sparse_conv_backward_oracle as sco
from conftest import ROOT, v3d

pytestmark = pytest.mark.gpu

OK, BAD_SHAPE, BAD_ARG, WS_SMALL = 0, -1, -2, -3                              # include/v3d.h
ROWS_LINE = ('constexpr int kWgradRows = 512;', 'gemm_wgrad.hip:23')
R = 512
M_BIG = 2 * R + 37
PAIRS = [(16, 16), (16, 32), (32, 16), (64, 128), (128, 128)]
PAD_SRC, PAD_GRAD = 12, 8

_maps = {}


def tables(kind):
    """(nbr [27, M], n_in) of the shared maps, computed once."""
    if kind not in _maps:
        if kind == 'isolated':
            c = sco.occupancy_map(M_BIG, 9, 3, lattice=3)
            nbr = sco.table('same', c)[0]
            assert (nbr[13] == np.arange(M_BIG)).all() and (np.delete(nbr, 13, axis=0) == -1).all()
            _maps[kind] = (nbr, M_BIG)
        elif kind == 'same':
            nbr, _, n_in, _ = sco.table('same', sco.occupancy_map(M_BIG, 9, 0))
            _maps[kind] = (nbr, n_in)
        else:
            # 'up': M_BIG fine rows gather from the coarse map; 'down': the coarse rows gather from M_BIG fine rows
            nbr, _, n_in, m = sco.table(kind, sco.occupancy_map(M_BIG, 9, 0))
            assert n_in != m
            _maps[kind] = (nbr, n_in)
    return _maps[kind]


def _to(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda).contiguous()


def call(cuda, case, poison=0xFF, expect=OK, ws_short=0, null=None, **over):
    """One call into a NaN-filled grad_w -> the array.  `over`: arguments replaced (K, N, n_seg, ld_src, ld_grad, nbr_stride, M)."""
    libm = v3d('_lib')
    lib = libm.load()
    a = dict(M=case['M'], K=case['K'], N=case['N'], n_seg=case['nbr'].shape[0], ld_src=case['ld_src'], ld_grad=case['ld_grad'],
             nbr_stride=case['nbr'].shape[1])
    a.update(over)
    src, nbr, g = _to(case['src'], cuda), _to(case['nbr'], cuda), _to(case['grad_out'], cuda)
    out = torch.full((case['nbr'].shape[0], case['K'], case['N']), float('nan'), dtype=torch.float32, device=cuda)
    nbytes = lib.v3d_sparse_conv_weight_grad_workspace_bytes(case['M'], case['nbr'].shape[0], case['K'], case['N'])
    assert nbytes == sco.chunks(case['M'])[0] * out.numel() * 4
    ws = torch.full((max(nbytes, 16),), poison, dtype=torch.uint8, device=cuda)
    ptrs = dict(src=src.data_ptr(), nbr=nbr.data_ptr(), g=g.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr())
    if null:
        ptrs[null] = None
    rc = lib.v3d_sparse_conv_weight_grad_f32(ptrs['src'], a['ld_src'], ptrs['nbr'], a['nbr_stride'], a['n_seg'], ptrs['g'], a['ld_grad'],
                                             a['M'], a['K'], a['N'], ptrs['out'], ptrs['ws'], nbytes - ws_short,
                                             libm.stream_ptr(cuda))
    torch.cuda.synchronize(cuda)
    assert rc == expect, (rc, lib.v3d_last_error())
    return out.cpu().numpy()


def make(kind, M, K, N, seed=11):
    nbr, n_in = tables(kind)
    # fewer rows: the first M columns of the table, which keeps its row stride
    case = sco.make_case(nbr[:, :M], n_in, K, N, seed, pad_src=PAD_SRC, pad_grad=PAD_GRAD)
    case['nbr'] = np.ascontiguousarray(nbr, dtype=np.int32)
    return case


def check(name, case, got):
    M = case['M']
    orc = sco.weight_grad(case['x'], case['nbr'][:, :M].astype(np.int64), case['g'])
    assert np.isfinite(got).all(), '%s: %d elements are not finite' % (name, (~np.isfinite(got)).sum())
    bad, worst, worst_zero = sco.violations(got, orc)
    print('%s: worst |dW - dW64| / bound = %.4f over %d elements (%d with S = 0), outside: %d'
          % (name, worst, got.size, (orc['S'] == 0).sum(), bad))
    assert bad == 0 and worst_zero == 0.0
    return orc, worst


def test_restated_constant_is_on_the_source_line_cited():
    fname, line = ROWS_LINE[1].rsplit(':', 1)
    lines = open(os.path.join(ROOT, '3dvnet_amd', 'csrc', fname)).read().split('\n')
    assert ROWS_LINE[0] in lines[int(line) - 1], lines[int(line) - 1][:120]
    assert sco.ROWS == R and sco.chunks(M_BIG) == (3, R)


@pytest.mark.parametrize('K,N', PAIRS, ids=lambda v: str(v))
@pytest.mark.parametrize('M', [M_BIG, 1, 0])
def test_sizes_and_channel_pairs(M, K, N, cuda):
    case = make('same', M, K, N)
    assert np.isnan(case['src'][:, K:]).all() and np.isnan(case['grad_out'][:, N:]).all()
    got = call(cuda, case)
    orc, worst = check('same M=%d K=%d N=%d' % (M, K, N), case, got)
    if M == 0:
        assert (got.view(np.int32) == 0).all()
    elif M == 1:
        assert np.isnan(case['src']).all(axis=1).sum() >= case['n_in'] - 27            # the rows nobody names are poison
        one = np.outer(case['x'][0].astype(np.float64), case['g'][0].astype(np.float64)).astype(np.float32)
        assert np.array_equal(got[13], one)                                             # one product, rounded once: exact
    else:
        assert worst > 0 and (orc['S'] > 0).all()                                       # fp32 sums of random data do round


@pytest.mark.parametrize('K,N', [(32, 16), (128, 128)], ids=lambda v: str(v))
@pytest.mark.parametrize('kind', ['down', 'up'])
def test_down_and_up_tables(kind, K, N, cuda):
    nbr, n_in = tables(kind)
    case = make(kind, nbr.shape[1], K, N)
    assert case['n_in'] != case['M'] and (nbr >= 0).any(axis=1).all()
    check('%s M=%d n_in=%d K=%d N=%d' % (kind, case['M'], n_in, K, N), case, call(cuda, case))


def test_empty_slabs_are_exactly_zero(cuda):
    case = make('isolated', M_BIG, 32, 16)
    got = call(cuda, case)
    orc, _ = check('isolated', case, got)
    assert list(np.nonzero(orc['cnt'])[0]) == [13]
    assert (np.delete(got, 13, axis=0).view(np.int32) == 0).all() and np.abs(got[13]).min() > 0


@pytest.mark.parametrize('K,N', [(16, 32), (128, 128)], ids=lambda v: str(v))
def test_two_calls_agree_and_strides_do_not_matter(K, N, cuda):
    case = make('same', M_BIG, K, N)
    first = call(cuda, case)
    assert np.array_equal(call(cuda, case, poison=0x00).view(np.int32), first.view(np.int32))
    assert np.array_equal(call(cuda, case).view(np.int32), first.view(np.int32))
    tight = dict(case, src=np.where(np.isnan(case['src'][:, :K]), 0, case['src'][:, :K]), grad_out=case['g'], ld_src=K, ld_grad=N)
    assert np.array_equal(call(cuda, tight).view(np.int32), first.view(np.int32))


@pytest.mark.parametrize('K,N', [(16, 32), (128, 128)], ids=lambda v: str(v))
def test_without_compaction_the_same_bound_holds(K, N, cuda):
    """Developer option wgrad_compact = 0 (every row staged, absent ones as zero rows): the same terms, so the same bound; the
    empty slabs of the isolated map stay +0."""
    libm = v3d('_lib')
    old = libm.set_option('wgrad_compact', 0)
    try:
        case = make('same', M_BIG, K, N)
        check('no compaction, same M=%d K=%d N=%d' % (M_BIG, K, N), case, call(cuda, case))
        iso = make('isolated', M_BIG, K, N)
        got = call(cuda, iso)
        check('no compaction, isolated', iso, got)
        assert (np.delete(got, 13, axis=0).view(np.int32) == 0).all()
    finally:
        libm.set_option('wgrad_compact', old)
    assert old == 1


def test_refusals_leave_grad_w_untouched(cuda):
    case = make('same', M_BIG, 32, 16)
    refusals = [(dict(K=24), BAD_SHAPE), (dict(N=144), BAD_SHAPE), (dict(n_seg=28), BAD_SHAPE), (dict(K=0), BAD_SHAPE),
                (dict(M=-1), BAD_SHAPE), (dict(M=2 ** 30 + 1, nbr_stride=2 ** 30 + 1), BAD_SHAPE), (dict(ws_short=1), WS_SMALL), (dict(ld_src=31), BAD_SHAPE), (dict(ld_grad=15), BAD_SHAPE),
                (dict(nbr_stride=M_BIG - 1), BAD_SHAPE), (dict(ld_src=46), BAD_ARG)]
    refusals += [(dict(null=n), BAD_ARG) for n in ('src', 'nbr', 'g', 'out', 'ws')]
    for kw, code in refusals:
        assert np.isnan(call(cuda, case, expect=code, **kw)).all(), kw
    check('after the refusals', case, call(cuda, case))                                # and the same call, complete, works
