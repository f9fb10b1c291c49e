"""GPU: ``training.sparse_conv`` (3dvnet_amd/training.py: SparseConv) through ``torch.autograd.grad`` at the production widths, per
element against the float64 sums of tests/sparse_conv_backward_oracle.py, in both precisions:

  y   against ``forward``      within ``input_grad_bound(..., forward=True)``
  dx  against ``input_grad``   within ``input_grad_bound``: (n + 32) u S in 'fp32', (2^-16 + (n + 32) u) S in 'split_bf16'
  dW  against ``weight_grad``  within (cnt_k + 32) u S (the kernel is exact fp32 in both precisions)

with n = present offsets of the row x contracted width, S the sum of the absolute terms, u = 2^-24; an element with S = 0 must be
exactly zero, so a row with no neighbour at all is +0 in y and in dx.  The bounds are derived in the oracle's docstring; none is
fitted to a kernel.

The tables come from ``sco.table`` on seeded maps, go to the device as int32 and are compared ONCE with what
``SparseLevel.neighbors`` returns for the same coordinates, so the Function is fed what ``training.sparse_unet`` feeds it:

  map A  66 597 voxels of a side-33 grid; its stride-2 map has 9 826 rows: both sides of the down and the up convolution exceed
         the 8 192 rows from which the gather-GEMM takes 64-row tiles with 8 loader waves;
  map B  9 000 voxels of a side-21 grid (same-level, tall tiles);
  map C  the 1 061 voxels of tests/test_sparse_conv_weight_grad_gpu.py (32-row tiles).

Cases: down 64 -> 128 on A (its input gradient runs over the up table), up 128 -> 64 on A, same 128 -> 128 and 64 -> 64 on B, same
48 -> 80 on C (K not a multiple of 32), and 48 -> 80 on C's table with one row in a hundred cut out of either side (a legal table
of the header's contract, though no map gives it: a real table has no row without a neighbour): those output rows are +0 in y,
those input rows +0 in dx, and the rows no entry names hold NaN in x and in grad_out.  Every case takes grad_out once contiguous
and once as a column window of a wider NaN-filled tensor (through ``torch.cat``); the two give equal bits.

The worst ratios are printed per case; DESIGN.md 4.1e records the values measured on an MI355X.  Wall time of the file there:
9.5 s for its 19 tests, 6 s of them the down and up tables of map A on the CPU, built once.
"""
import numpy as np
import pytest
import torch

import sparse_conv_backward_oracle as sco
from conftest import v3d

pytestmark = pytest.mark.gpu

MAPS = {'A': (130 * 512 + 37, 33, 0), 'B': (9000, 21, 0), 'C': (2 * 512 + 37, 9, 0)}
CASES = {                                                                     # name: (kind, map, Ci, Co, pruned)
    'down 64 -> 128 on A': ('down', 'A', 64, 128, False),
    'up 128 -> 64 on A': ('up', 'A', 128, 64, False),
    'same 128 -> 128 on B': ('same', 'B', 128, 128, False),
    'same 64 -> 64 on B': ('same', 'B', 64, 64, False),
    'same 48 -> 80 on C': ('same', 'C', 48, 80, False),
    'pruned 48 -> 80 on C': ('same', 'C', 48, 80, True),
}
TALL = 8192                                                                   # rows from which choose_gemm_kernel takes 64-row tiles

_oracles, _device, _checked = {}, {}, set()


def invert(nbr, n_in):
    """The inverse of any table with injective rows: inv[k, nbr[k, p]] = p."""
    inv = np.full((nbr.shape[0], n_in), -1, dtype=np.int64)
    k, p = np.nonzero(nbr >= 0)
    inv[k, nbr[k, p]] = p
    return inv


def host_tables(name):
    """(nbr int64 [27, M], inv int64 [27, n_in]) of a case"""
    kind, m, _, _, pruned = CASES[name]
    nbr, inv, n_in, _ = sco.map_tables(kind, *MAPS[m])[:4]
    if pruned:
        rng = np.random.default_rng(17)
        assert np.array_equal(invert(nbr, n_in), inv)
        nbr = nbr.copy()
        nbr[:, rng.choice(nbr.shape[1], nbr.shape[1] // 100, replace=False)] = -1
        nbr[np.isin(nbr, rng.choice(n_in, n_in // 100, replace=False))] = -1
        inv = invert(nbr, n_in)
    return nbr, inv


def oracle(name):
    """Seeded inputs and the float64 results of a case, computed once and left unchanged."""
    if name not in _oracles:
        _, _, ci, co, _ = CASES[name]
        nbr, inv = host_tables(name)
        n_in, m = inv.shape[1], nbr.shape[1]
        rng = np.random.default_rng(len(name) + ci)
        x = rng.standard_normal((n_in, ci)).astype(np.float32)
        w = (0.2 * rng.standard_normal((27, ci, co))).astype(np.float32)
        g = rng.standard_normal((m, co)).astype(np.float32)
        x_used, g_used = (inv >= 0).any(axis=0), (nbr >= 0).any(axis=0)          # a row some entry names
        x0, g0 = np.where(x_used[:, None], x, 0), np.where(g_used[:, None], g, 0)
        x[~x_used], g[~g_used] = np.nan, np.nan                                  # nobody may read the others
        o = dict(x=x, w=w, g=g, x_used=x_used, g_used=g_used, y=sco.forward(x0, w, nbr), dx=sco.input_grad(w, inv, g0),
                 dW=sco.weight_grad(x0, nbr, g0), y_sums=sco.term_sums(w, nbr, x0, forward=True), dx_sums=sco.term_sums(w, inv, g0))
        # the comparison is not vacuous: terms on more than 95 % of the rows, a present and an absent entry in every table row
        assert (o['y_sums'][1] > 0).all(axis=1).mean() > 0.95 and (o['dx_sums'][1] > 0).all(axis=1).mean() > 0.95
        # (the centre offset of an unpruned same-level table is the identity: no absent entry there)
        identity = CASES[name][0] == 'same' and not CASES[name][4]
        for t in (nbr, inv):
            absent = (t < 0).any(axis=1)
            assert (t >= 0).any(axis=1).all() and absent[np.arange(27) != 13].all()
            assert absent[13] or (identity and np.array_equal(t[13], np.arange(t.shape[1])))
        _oracles[name] = o
    return _oracles[name]


def device_tables(name, cuda):
    """(nbr, inv) int32 on the device; the unpruned tables of each (kind, map) are compared once with SparseLevel.neighbors."""
    if name not in _device:
        kind, m, _, _, pruned = CASES[name]
        nbr, inv = host_tables(name)
        dev = tuple(torch.from_numpy(t.astype(np.int32)).to(cuda).contiguous() for t in (nbr, inv))
        if (kind, m) not in _checked and not pruned:
            sm = v3d('scenemodeling')
            res = sco.map_tables(kind, *MAPS[m])
            coords = lambda c: torch.from_numpy(np.ascontiguousarray(c, dtype=np.int32)).to(cuda)
            fine = sm.SparseLevel(coords(res[4]), 1).check()
            if kind == 'same':
                same = fine.neighbors(fine.coords, 1)
                assert torch.equal(same, dev[0]) and torch.equal(same.flip(0), dev[1])
            else:
                coarse = sm.SparseLevel(coords(res[5]), 2).check()
                down, up = fine.neighbors(coarse.coords, 1), coarse.neighbors(fine.coords, -1)   # as training.sparse_unet forms them
                assert torch.equal(down, dev[0] if kind == 'down' else dev[1]) and torch.equal(up, dev[1] if kind == 'down' else dev[0])
            _checked.add((kind, m))
        _device[name] = dev
    return _device[name]


def gradients(name, precision, cuda, windowed):
    tr = v3d('training')
    o = oracle(name)
    nbr, inv = device_tables(name, cuda)
    x = torch.from_numpy(o['x']).to(cuda).requires_grad_(True)
    w = torch.from_numpy(o['w']).to(cuda).requires_grad_(True)
    gy = torch.from_numpy(o['g']).to(cuda)
    y = tr.sparse_conv(x, w, nbr, inv, precision)
    if windowed:                                                              # the gradient of `y` is a view with row stride Co + 16 at column 16
        other = torch.zeros((y.shape[0], 16), device=cuda, requires_grad=True)
        wide = torch.full((y.shape[0], y.shape[1] + 16), float('nan'), device=cuda)
        wide[:, 16:] = gy
        dx, dw = torch.autograd.grad(torch.cat((other, y), dim=1), (x, w), wide)
    else:
        dx, dw = torch.autograd.grad(y, (x, w), gy)
    torch.cuda.synchronize(cuda)
    return y.detach().cpu().numpy(), dx.cpu().numpy(), dw.cpu().numpy()


def test_the_maps_reach_both_tile_heights():
    rows = {name: tuple(t.shape[1] for t in host_tables(name)) for name in CASES}
    assert rows['down 64 -> 128 on A'] == (9826, 66597) and rows['up 128 -> 64 on A'] == (66597, 9826)
    assert min(rows['down 64 -> 128 on A']) >= TALL and rows['same 128 -> 128 on B'] == (9000, 9000) and 9000 >= TALL
    assert rows['same 48 -> 80 on C'] == (1061, 1061) and 1061 < TALL
    nbr, inv = host_tables('pruned 48 -> 80 on C')
    assert 5 <= (~(nbr >= 0).any(axis=0)).sum() <= 30 and 5 <= (~(inv >= 0).any(axis=0)).sum() <= 30
    for name in CASES:
        if not CASES[name][4]:
            assert (host_tables(name)[0] >= 0).any(axis=0).all()              # a real table has no row without a neighbour


@pytest.mark.parametrize('precision', ['fp32', 'split_bf16'])
@pytest.mark.parametrize('name', list(CASES))
def test_forward_and_both_gradients_per_element(name, precision, cuda):
    o = oracle(name)
    nbr, inv = host_tables(name)
    y, dx, dw = gradients(name, precision, cuda, windowed=False)
    assert y.shape == o['y'].shape and dx.shape == o['dx'].shape and dw.shape == o['dW']['dW'].shape
    assert np.isfinite(y).all() and np.isfinite(dx).all() and np.isfinite(dw).all()
    report = []
    for what, got, ref, bnd in (('y', y, o['y'], sco.input_grad_bound(o['w'], nbr, None, precision, forward=True, sums=o['y_sums'])),
                                ('dx', dx, o['dx'], sco.input_grad_bound(o['w'], inv, None, precision, sums=o['dx_sums']))):
        bad, worst, worst_zero = sco.outside(got, ref, bnd)
        report.append((what, bad, worst, worst_zero, int((bnd == 0).sum())))
    bad, worst, worst_zero = sco.violations(dw, o['dW'])
    report.append(('dW', bad, worst, worst_zero, int((o['dW']['S'] == 0).sum())))
    print('%s, %s: ' % (name, precision) + '; '.join('%s worst ratio %.3g, outside %d, S = 0 on %d elements (largest |.| there %g)'
                                                    % (what, worst, bad, nz, wz) for what, bad, worst, wz, nz in report))
    assert all(bad == 0 and wz == 0.0 and worst > 0 for _, bad, worst, wz, _ in report), report
    # rows with no neighbour at all: +0 bit for bit
    assert (y[~o['g_used']].view(np.int32) == 0).all() and (dx[~o['x_used']].view(np.int32) == 0).all()
    if CASES[name][4]:
        assert (~o['g_used']).sum() >= 5 and (~o['x_used']).sum() >= 5 and np.isnan(o['x'][~o['x_used']]).all() and np.isnan(o['g'][~o['g_used']]).all()
    # grad_out as a column window of a wider NaN-filled tensor: the same bits
    y2, dx2, dw2 = gradients(name, precision, cuda, windowed=True)
    for a, b in ((y, y2), (dx, dx2), (dw, dw2)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize('precision', ['fp32', 'split_bf16'])
@pytest.mark.parametrize('name', ['down 64 -> 128 on A', 'up 128 -> 64 on A', 'pruned 48 -> 80 on C'])
def test_small_integer_inputs_give_the_float64_sums_exactly(name, precision, cuda):
    """Values in {-2, ..., 2}: bf16 holds them (the low halves of the split are zero), every product and partial sum is an integer
    below 2^24, so y, dx and dW equal the float64 sums bit for bit in both precisions, whatever the order.  The bounds above are
    relative to S; this is the check that no single row of the 64-row tiles is gathered from the wrong place."""
    o = oracle(name)
    key = name + ' / integers'
    if key not in _oracles:
        nbr, inv = host_tables(name)
        q = lambda a: np.clip(np.rint(a), -2, 2).astype(np.float32)                   # NaN stays NaN
        x, w, g = q(o['x']), q(5 * o['w']), q(o['g'])
        x0, g0 = np.where(o['x_used'][:, None], x, 0), np.where(o['g_used'][:, None], g, 0)
        _oracles[key] = dict(o, x=x, w=w, g=g, y=sco.forward(x0, w, nbr), dx=sco.input_grad(w, inv, g0), dW=sco.weight_grad(x0, nbr, g0))
        _device[key] = device_tables(name, cuda)
    oi = _oracles[key]
    assert np.abs(oi['w']).max() == 2 and oi['dW']['S'].max() < 2 ** 24 and np.abs(oi['y']).max() > 20 and np.abs(oi['dx']).max() > 20
    y, dx, dw = gradients(key, precision, cuda, windowed=False)
    assert np.array_equal(y.astype(np.float64), oi['y']) and np.array_equal(dx.astype(np.float64), oi['dx'])
    assert np.array_equal(dw.astype(np.float64), oi['dW']['dW'])
