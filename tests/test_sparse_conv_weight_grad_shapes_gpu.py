"""GPU: every tile shape and every chunking of v3d_sparse_conv_weight_grad_f32 (csrc/gemm_wgrad.hip) through the C ABI, per element
against tests/sparse_conv_backward_oracle.py at the bound of tests/test_sparse_conv_weight_grad_gpu.py, (cnt_k + 32) * 2^-24 * S,
with that file's call (wide rows, NaN behind K / N and in every source row no table entry names, a NaN-filled grad_w, a
0xFF-filled workspace, the size function held to the oracle's chunking):

  * the 64 channel pairs of {16, 32, ..., 128}^2 on the same-level table at M = 2 * 512 + 37: each of the 16 instantiations
    sparse_conv_wgrad_kernel<KBW, NBW> is launched (the mapping is restated from the dispatch line cited below), and the widths
    48, 80 and 112, at which a wave owns real blocks and one behind K / 16 or N / 16;
  * a down and an up table at (64, 128), (128, 64), (48, 80) and (96, 112);
  * tables without a coordinate map (sparse_conv_backward_oracle.synthetic_table, one slab per pattern, n_seg = 11): every row, no
    row, only p = 0, only p = M - 1, one wave of one half of every 512-row block, empty blocks between full ones, 31 / 32 / 33
    present rows per block, a random half; at M = 511, 512, 513, 65 536 (128 one-block chunks), 65 537 (65 two-block chunks, the
    last of one row) and 131 077 (three-block chunks, the last ragged) x (16, 16) and (48, 80): the loop over the blocks of a chunk
    runs two and three times, with blocks of no present row between others.  The empty slab is +0 bit for bit, the one-row slabs
    equal the float32-rounded outer product;
  * the same-level table of a 66 597-voxel map (66 chunks of two blocks) at K = N = 64 on the offsets 0, 4, 13, 22, 26, with
    compaction and (developer option wgrad_compact = 0) without;
  * at M = 65 537 and 131 077 two calls (workspaces of 0xFF and of 0x00) give the same bits, and contiguous rows the bits of wide ones.

The worst ratio to the bound is printed per case; DESIGN.md 4.1e records the values measured on an MI355X.  No number here comes
from the kernel under test.  Wall time of the file on an MI355X: 8.4 s for its 90 GPU tests, 5 s of them the table and the float64
sums of the large map, computed once.
"""
import os

import numpy as np
import pytest

import sparse_conv_backward_oracle as sco
from conftest import ROOT, v3d
from test_sparse_conv_weight_grad_gpu import M_BIG, PAD_GRAD, PAD_SRC, call, check, make, tables

gpu = pytest.mark.gpu

DISPATCH_LINE = ('WgradKernel kern = wgrad_kernel((K / 16 + 1) / 2, (N / 16 + 1) / 2);', 'gemm_wgrad.hip:237')
TEMPLATE_LINE = ('for (int i = 0; i < KBW; ++i) acol[i] = (wr * KBW + i < nkb ? wr * KBW + i : 0) * 16 + jn;', 'gemm_wgrad.hip:68')
WIDTHS = list(range(16, 129, 16))
BLOCKS_PER_WAVE = {16: 1, 32: 1, 48: 2, 64: 2, 80: 3, 96: 3, 112: 4, 128: 4}       # what the dispatch line gives, width by width
ALL_PAIRS = [(K, N) for K in WIDTHS for N in WIDTHS]
SYNTH_M = [511, 512, 513, 128 * 512, 128 * 512 + 1, 131077]
BIG = 130 * 512 + 37                                                          # 66 597 voxels of a side-33 grid
BIG_OFFSETS = [0, 4, 13, 22, 26]


def instantiation(K, N):
    """(KBW, NBW) of the kernel a call with these widths launches: the dispatch line, restated."""
    return (K // 16 + 1) // 2, (N // 16 + 1) // 2


def phantom_blocks(K):
    """16-column blocks behind K / 16 that the two wave rows own: they recompute block 0 and store nothing."""
    return 2 * instantiation(K, K)[0] - K // 16


def test_restated_dispatch_is_on_the_source_lines_cited():
    for text, where in (DISPATCH_LINE, TEMPLATE_LINE):
        fname, line = where.rsplit(':', 1)
        lines = open(os.path.join(ROOT, '3dvnet_amd', 'csrc', fname)).read().split('\n')
        assert text in lines[int(line) - 1], '%r is not on line %s of %s: %r' % (text, line, fname, lines[int(line) - 1][:120])


def test_the_64_pairs_reach_all_16_instantiations():
    reached = {}
    for K, N in ALL_PAIRS:
        reached.setdefault(instantiation(K, N), []).append((K, N))
    print('instantiations reached by the sweep: %d of 16' % len(reached))
    assert sorted(reached) == [(a, b) for a in (1, 2, 3, 4) for b in (1, 2, 3, 4)] and all(len(v) == 4 for v in reached.values())
    assert all(instantiation(K, N) == (BLOCKS_PER_WAVE[K], BLOCKS_PER_WAVE[N]) for K, N in ALL_PAIRS)
    assert instantiation(64, 64) == (2, 2) and instantiation(128, 64) == (4, 2) and instantiation(64, 128) == (2, 4)
    assert instantiation(80, 96) == (3, 3) and instantiation(96, 80) == (3, 3)
    # a wave with real blocks AND one behind the width: 48, 80, 112; 16 is the degenerate form (a whole wave row idle)
    assert [K for K in WIDTHS if phantom_blocks(K) and instantiation(K, K)[0] > 1] == [48, 80, 112] and phantom_blocks(16) == 1
    # the sweep's M: three one-block chunks, the last ragged
    assert sco.chunks(M_BIG) == (3, 512)


@gpu
@pytest.mark.parametrize('K,N', ALL_PAIRS, ids=lambda v: str(v))
def test_every_instantiation(K, N, cuda):
    assert instantiation(K, N) == (BLOCKS_PER_WAVE[K], BLOCKS_PER_WAVE[N])
    case = make('same', M_BIG, K, N)
    assert case['ld_src'] == K + PAD_SRC and np.isnan(case['src'][:, K:]).all() and np.isnan(case['grad_out'][:, N:]).all()
    got = call(cuda, case)
    orc, worst = check('<%d, %d> same M=%d K=%d N=%d' % (instantiation(K, N) + (M_BIG, K, N)), case, got)
    assert worst > 0 and (orc['S'] > 0).all()


@gpu
@pytest.mark.parametrize('K,N', [(64, 128), (128, 64), (48, 80), (96, 112)], ids=lambda v: str(v))
@pytest.mark.parametrize('kind', ['down', 'up'])
def test_down_and_up_tables(kind, K, N, cuda):
    nbr, n_in = tables(kind)
    case = make(kind, nbr.shape[1], K, N)
    assert case['n_in'] != case['M'] and (nbr >= 0).any(axis=1).all() and (nbr < 0).any(axis=1).all()
    check('<%d, %d> %s M=%d n_in=%d K=%d N=%d' % (instantiation(K, N) + (kind, case['M'], n_in, K, N)), case, call(cuda, case))


def synthetic_case(M, K, N):
    """One slab per pattern; 40 source rows more than table rows, so that some source rows are named by no entry of some slab and a
    few by none at all (they hold NaN)."""
    pats = sco.ALL_PATTERNS
    nbr = sco.synthetic_table(M, M + 40, pats, seed=M)
    return pats, sco.make_case(nbr, M + 40, K, N, seed=M + K, pad_src=PAD_SRC, pad_grad=PAD_GRAD)


@gpu
@pytest.mark.parametrize('K,N', [(16, 16), (48, 80)], ids=lambda v: str(v))
@pytest.mark.parametrize('M', SYNTH_M)
def test_sizes_and_compaction_patterns(M, K, N, cuda):
    pats, case = synthetic_case(M, K, N)
    n_chunks, rows = sco.chunks(M)
    assert (n_chunks, rows // 512) == {511: (1, 1), 512: (1, 1), 513: (2, 1), 65536: (128, 1), 65537: (65, 2), 131077: (86, 3)}[M]
    assert len(pats) == 11 != 27 and case['nbr'].shape == (11, M)
    libm = v3d('_lib')
    assert libm.load().v3d_sparse_conv_weight_grad_workspace_bytes(M, len(pats), K, N) == n_chunks * len(pats) * K * N * 4
    got = call(cuda, case)
    orc, _ = check('patterns M=%d (%d chunks of %d blocks) K=%d N=%d' % (M, n_chunks, rows // 512, K, N), case, got)
    cnt = dict(zip(pats, orc['cnt']))
    assert cnt['every'] == M and cnt['none'] == 0 and cnt['first'] == 1 and cnt['last'] == 1 and cnt['wave0'] >= 64
    assert (got[pats.index('none')].view(np.int32) == 0).all()                          # +0 bit for bit
    nbr, x, g = case['nbr'], case['x'].astype(np.float64), case['g'].astype(np.float64)
    for name, p in (('first', 0), ('last', M - 1)):
        k = pats.index(name)
        one = np.outer(x[nbr[k, p]], g[p]).astype(np.float32)                           # one product, rounded once: exact
        assert np.array_equal(got[k], one) and np.abs(one).min() > 0, name
    if M > 512:
        b = np.arange(M) // 512
        for name in ('odd_blocks', 'tile_edge'):
            per_block = np.bincount(b, weights=(nbr[pats.index(name)] >= 0), minlength=b[-1] + 1).astype(np.int64)
            if name == 'odd_blocks':
                assert (per_block[0::2] == 0).all() and (per_block[1:-1:2] == 512).all()
            elif M >= 3 * 512:
                assert list(per_block[:3]) == [31, 32, 33]


_big = []


def big_case():
    """(case, oracle) of the large map, computed once and left unchanged."""
    if not _big:
        case = _make_big_case()
        _big.append((case, sco.weight_grad(case['x'], case['nbr'].astype(np.int64), case['g'])))
    return _big[0]


def _make_big_case():
    nbr, _, n_in, m, _ = sco.map_tables('same', BIG, 33, 0)
    sub = np.ascontiguousarray(nbr[BIG_OFFSETS])
    blocks = (sub[0, :m // 512 * 512].reshape(-1, 512) >= 0).sum(axis=1)
    assert m == BIG and sco.chunks(m) == (66, 1024) and (blocks == 0).sum() >= 3 and (blocks > 0).sum() >= 100, (blocks == 0).sum()
    return sco.make_case(sub, n_in, 64, 64, seed=5, pad_src=PAD_SRC, pad_grad=PAD_GRAD)


@gpu
@pytest.mark.parametrize('compact', [1, 0], ids=['compacted', 'every row staged'])
def test_a_realistic_large_map(compact, cuda):
    case, orc = big_case()
    libm = v3d('_lib')
    old = libm.set_option('wgrad_compact', compact)
    try:
        got = call(cuda, case)
    finally:
        libm.set_option('wgrad_compact', old)
    assert old == 1
    assert np.isfinite(got).all()
    bad, worst, worst_zero = sco.violations(got, orc)
    print('66 597 voxels, offsets %s, K=N=64, wgrad_compact=%d: worst |dW - dW64| / bound = %.3g over %d elements, outside: %d'
          % (BIG_OFFSETS, compact, worst, got.size, bad))
    assert bad == 0 and worst_zero == 0.0
    assert worst > 0 and (orc['S'] > 0).all() and orc['cnt'][2] == BIG and orc['cnt'][0] < BIG


@gpu
@pytest.mark.parametrize('M', [128 * 512 + 1, 131077])
def test_two_calls_agree_and_strides_do_not_matter_in_multi_block_chunks(M, cuda):
    K, N = 48, 80
    _, case = synthetic_case(M, K, N)
    first = call(cuda, case)
    assert np.isfinite(first).all()
    assert np.array_equal(call(cuda, case, poison=0x00).view(np.int32), first.view(np.int32))
    tight = dict(case, src=np.where(np.isnan(case['src'][:, :K]), 0, case['src'][:, :K]), grad_out=case['g'], ld_src=K, ld_grad=N)
    assert np.array_equal(call(cuda, tight).view(np.int32), first.view(np.int32))


@gpu
@pytest.mark.parametrize('M', [128 * 512 + 1, 131077])
def test_small_integer_inputs_are_summed_exactly(M, cuda):
    """Values in {-3, ..., 3}: every product and every partial sum is an integer below 2^24, so no order of summation rounds and
    grad_w equals the float64 sum bit for bit.  At these M the bound above is thousands of terms wide; this is the check that no
    single row of a multi-block chunk is dropped, doubled or gathered from the wrong place."""
    K, N = 48, 80
    pats, case = synthetic_case(M, K, N)
    q = lambda a: np.clip(np.rint(1.5 * a), -3, 3).astype(np.float32)                  # NaN stays NaN
    case = dict(case, src=q(case['src']), grad_out=q(case['grad_out']), x=q(case['x']))
    case['g'] = case['grad_out'][:, :N]
    assert np.isnan(case['src'][:, K:]).all() and np.isnan(case['grad_out'][:, N:]).all() and np.abs(case['x']).max() == 3
    got = call(cuda, case)
    orc = sco.weight_grad(case['x'], case['nbr'].astype(np.int64), case['g'])
    assert orc['S'].max() < 2 ** 24 and np.array_equal(orc['dW'], np.rint(orc['dW'])) and np.abs(orc['dW'][pats.index('every')]).max() > 100
    assert np.array_equal(got.astype(np.float64), orc['dW'])
    assert not np.signbit(got[pats.index('none')]).any()
