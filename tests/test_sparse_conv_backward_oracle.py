"""CPU tests of tests/sparse_conv_backward_oracle.py: the inverse-table formulation of the input gradient is the scatter-add
definition, the table relations DESIGN.md 4.1e states hold, and the weight-gradient bound rejects the mistakes a kernel can make.

Seed 0 is the first one tried; every wrong variant reaches the floor with it, none had to be rejected.
"""
import numpy as np
import pytest

import sparse_conv_backward_oracle as sco
import sparse_oracle as so

FLOOR = 0.70            # share of the elements a bug can change that it must push outside the bound (test_backproject_backward_oracle.py)
SEED = 0
M = 2 * sco.ROWS + 37   # three chunks, the last one ragged
K = 16


@pytest.fixture(scope='module')
def coords():
    return sco.occupancy_map(M, 9, SEED)


@pytest.mark.parametrize('kind,ts', [('same', 1), ('same', 2), ('down', 1), ('up', 1)])
def test_input_gradient_is_the_scatter_add(kind, ts):
    c = sco.occupancy_map(400, 7, SEED + 1, lattice=ts)
    nbr, inv, n_in, m = sco.table(kind, c, ts)
    assert (nbr >= 0).any() and (nbr < 0).any() and nbr.shape == (27, m) and inv.shape == (27, n_in)
    if kind != 'same':
        assert n_in != m
    rng = np.random.default_rng(SEED)
    w, g = rng.standard_normal((27, 16, 32)), rng.standard_normal((m, 32))
    a, b = sco.input_grad(w, inv, g), sco.input_grad_scatter(w, nbr, g, n_in)
    assert np.abs(b).max() > 0
    # the same products; only the order of the (at most 27) additions per element differs
    assert np.abs(a - b).max() <= 27 * 2.0 ** -52 * np.abs(b).max() * 32
    # and it is the adjoint of the forward: <y(x), g> is linear in x with gradient dx
    x = rng.standard_normal((n_in, 16))
    assert abs((sco.forward(x, w, nbr) * g).sum() - (x * a).sum()) <= 1e-9 * np.abs(x).sum()
    orc = sco.weight_grad(x, nbr, g)
    assert abs((sco.forward(x, w, nbr) * g).sum() - (w * orc['dW']).sum()) <= 1e-9 * np.abs(w).sum()


def test_table_relations(coords):
    nbr, inv, _, _ = sco.table('same', coords)
    assert np.array_equal(inv, nbr[::-1])                                     # o_{26 - k} = -o_k
    assert np.array_equal(so.offsets()[::-1], -so.offsets())
    down, up, n_fine, n_coarse = sco.table('down', coords)
    up2, down2, _, _ = sco.table('up', coords)
    assert np.array_equal(down, down2) and np.array_equal(up, up2) and down.shape == (27, n_coarse) and up.shape == (27, n_fine)
    k, p = np.nonzero(down >= 0)
    assert np.array_equal(up[k, down[k, p]], p)                               # nbr[k, p] = a  <=>  inv[k, a] = p
    assert (up >= 0).sum() == (down >= 0).sum()


def test_chunks_depend_on_m_only():
    assert sco.chunks(0) == (0, 0) and sco.chunks(1) == (1, 512) and sco.chunks(M) == (3, 512)
    assert sco.chunks(128 * 512) == (128, 512) and sco.chunks(128 * 512 + 1) == (65, 1024)


def _case(coords, pad=0):
    nbr, _, n_in, _ = sco.table('same', coords)
    rng = np.random.default_rng(SEED + 7)
    case = sco.make_case(nbr, n_in, K, K, SEED, pad_src=pad, pad_grad=pad, poison=0.0)
    if pad:                                                                   # finite values: a NaN would be rejected whatever it is
        case['src'][:, K:] = rng.standard_normal((n_in, pad)).astype(np.float32)
        case['grad_out'][:, K:] = rng.standard_normal((M, pad)).astype(np.float32)
    return case


def _share_outside(wrong, orc, affected):
    out = ~(np.abs(wrong - orc['dW']) <= sco.bound(orc))
    return float((out & affected).sum()) / float(affected.sum()), int((out & ~affected).sum())


def test_bound_holds_a_float32_evaluation_and_is_not_vacuous(coords):
    case = _case(coords)
    orc = sco.weight_grad(case['x'], case['nbr'], case['g'])
    assert (orc['S'] > 0).all() and orc['cnt'].min() > 100 and orc['cnt'][13] == M
    d32 = np.stack([case['x'][n[n >= 0]].astype(np.float32).T @ case['g'][n >= 0] for n in case['nbr']])
    assert d32.dtype == np.float32
    bad, worst, _ = sco.violations(d32, orc)
    print('   float32 on the CPU: worst |d32 - d64| / bound = %.3f, outside: %d' % (worst, bad))
    assert bad == 0 and 0 < worst < 1
    # the bound is far below one term of the sum: a single present row dropped per offset (the first one) leaves it
    cut = case['nbr'].astype(np.int64)
    for k in range(27):
        cut[k, np.nonzero(cut[k] >= 0)[0][0]] = -1
    share, _ = _share_outside(sco.weight_grad(case['x'], cut, case['g'])['dW'], orc, np.ones_like(orc['S'], dtype=bool))
    print('   one row dropped per offset: %.3f of the elements outside the bound' % share)
    assert share >= FLOOR


def test_wrong_variants_leave_the_bound(coords):
    case = _case(coords)
    nbr, x, g = case['nbr'].astype(np.int64), case['x'], case['g']
    orc = sco.weight_grad(x, nbr, g)
    every = np.ones_like(orc['S'], dtype=bool)
    slabs = lambda mask: np.broadcast_to(np.asarray(mask)[:, None, None], orc['S'].shape)
    n_chunks, rows = sco.chunks(M)
    last = (n_chunks - 1) * rows
    variants = {}
    # the offset index 26 - k: every slab but the centre one
    variants['offset 26 - k'] = (orc['dW'][::-1], slabs(np.arange(27) != 13))
    # -1 read as row 0: the slabs with an absent row
    variants['-1 as row 0'] = (sco.weight_grad(x, np.where(nbr < 0, 0, nbr), g)['dW'], slabs((nbr < 0).any(axis=1)))
    # the last chunk dropped: the slabs with a present row in it
    variants['last chunk dropped'] = (sco.weight_grad(x, nbr[:, :last], g[:last])['dW'], slabs((nbr[:, last:] >= 0).any(axis=1)))
    # the ragged tail of the last chunk's present rows dropped (the last np % 32 of them, per offset)
    cut = nbr.copy()
    tails = np.zeros(27, dtype=np.int64)
    for k in range(27):
        present = last + np.nonzero(nbr[k, last:] >= 0)[0]
        tails[k] = present.size % sco.TILE
        if tails[k]:
            cut[k, present[-tails[k]:]] = -1
    variants['ragged tail dropped'] = (sco.weight_grad(x, cut, g)['dW'], slabs(tails > 0))
    # ci and co swapped (K = N)
    variants['ci / co swapped'] = (orc['dW'].transpose(0, 2, 1), every)
    # ld ignored: rows of K floats read from buffers whose rows are K + 12 floats wide
    wide = _case(coords, pad=12)
    flat = lambda a, n: a.reshape(-1)[:n * K].reshape(n, K)
    assert np.array_equal(wide['src'][:, :K], case['src'][:, :K])
    variants['ld ignored'] = (sco.weight_grad(flat(wide['src'], case['n_in']), nbr, flat(wide['grad_out'], M))['dW'], every)
    for name, (wrong, affected) in variants.items():
        assert affected.any(), name
        share, elsewhere = _share_outside(wrong, orc, affected)
        print('   %-22s %.3f of %d affected elements outside the bound' % (name, share, affected.sum()))
        assert share >= FLOOR, (name, share)
        assert elsewhere == 0, (name, elsewhere)
