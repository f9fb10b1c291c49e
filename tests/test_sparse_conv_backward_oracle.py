"""CPU tests of tests/sparse_conv_backward_oracle.py: the inverse-table formulation of the input gradient is the scatter-add
definition, the table relations DESIGN.md 4.1e states hold, and the weight-gradient bound rejects the mistakes a kernel can make,
those of a tile shape (K = 48) and of a multi-block chunk (M = 65 537) among them; `synthetic_table` is legal, injective per offset and
holds its patterns; `input_grad_bound` is the documented formula, holds a float32 evaluation and the three-product bf16 split on a
66 597-voxel map, and rejects four wrong input gradients.

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
    assert sco.chunks(66597) == (66, 1024) and sco.chunks(131077) == (86, 1536)
    # 131 077 rows are 257 blocks: 85 chunks of three and a ragged one (two blocks, the second of 5 rows)
    assert 131077 - 85 * 1536 == 512 + 5


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


# ---- synthetic tables ---------------------------------------------------------------------------------------------------------------

def test_synthetic_table_is_legal_injective_and_holds_its_patterns():
    R = sco.ROWS
    m, n_in = 6 * R + 5, 6 * R + 40
    pats = sco.ALL_PATTERNS
    t = sco.synthetic_table(m, n_in, pats, SEED)
    assert t.shape == (len(pats), m) and t.dtype == np.int64 and t.min() == -1 and t.max() < n_in
    assert np.array_equal(t, sco.synthetic_table(m, n_in, pats, SEED)) and not np.array_equal(t, sco.synthetic_table(m, n_in, pats, SEED + 1))
    present = dict(zip(pats, t >= 0))
    for row in t:                                                             # injective per offset
        assert np.unique(row[row >= 0]).size == (row >= 0).sum()
    assert present['every'].all() and not present['none'].any()
    assert list(np.nonzero(present['first'])[0]) == [0] and list(np.nonzero(present['last'])[0]) == [m - 1]
    for name, lo in (('wave0', 0), ('wave3', 192), ('wave4', 256), ('wave7', 448)):
        q = np.nonzero(present[name])[0] % R
        assert q.min() == lo and q.max() == lo + 63 and present[name][:6 * R].sum() == 6 * 64, name
    blocks = lambda mask: [int(mask[b * R:(b + 1) * R].sum()) for b in range(7)]
    assert blocks(present['odd_blocks']) == [0, R, 0, R, 0, R, 0]
    assert blocks(present['tile_edge']) == [31, 32, 33, 31, 32, 33, 1]               # the ragged block: 1 of its 5 rows
    # the 31 .. 33 rows of a block lie in every wave of both halves
    assert {int(q) // 64 for q in np.nonzero(present['tile_edge'][:R])[0]} == set(range(8))
    assert 0.45 < present['half'].mean() < 0.55
    # different offsets gather different source rows from the same p
    assert (t[pats.index('every')] != t[pats.index('half')])[present['half']].mean() > 0.99


def test_weight_gradient_variants_of_tile_shape_and_chunking_leave_the_bound():
    """The two mistakes the dispatch over tile shapes and the loop over the blocks of a chunk can make."""
    rng = np.random.default_rng(SEED + 3)
    # "ci block b >= 1 holds block 0's values", K = 48
    m, k48 = M, 48
    nbr = sco.synthetic_table(m, m, ('every', 'half', 'tile_edge'), SEED)
    x, g = rng.standard_normal((m, k48)).astype(np.float32), rng.standard_normal((m, 16)).astype(np.float32)
    orc = sco.weight_grad(x, nbr, g)
    wrong = orc['dW'].copy()
    wrong[:, 16:32], wrong[:, 32:48] = orc['dW'][:, :16], orc['dW'][:, :16]
    affected = np.zeros_like(orc['S'], dtype=bool)
    affected[:, 16:] = True
    share, elsewhere = _share_outside(wrong, orc, affected)
    print('   ci block b >= 1 = block 0, K = 48: %.3f of %d affected elements outside the bound' % (share, affected.sum()))
    assert share >= FLOOR and elsewhere == 0
    # "the second block of every two-block chunk dropped", M = 65 537: 65 chunks of 1024 rows
    m = 128 * sco.ROWS + 1
    assert sco.chunks(m) == (65, 2 * sco.ROWS)
    nbr = sco.synthetic_table(m, m, ('every', 'half', 'odd_blocks', 'wave4', 'last'), SEED)
    x, g = rng.standard_normal((m, K)).astype(np.float32), rng.standard_normal((m, K)).astype(np.float32)
    orc = sco.weight_grad(x, nbr, g)
    second = (np.arange(m) % (2 * sco.ROWS)) >= sco.ROWS
    cut = np.where(second[None], -1, nbr)
    has = ((nbr >= 0) & second[None]).any(axis=1)
    assert list(has) == [True, True, True, True, False]                       # the last row opens a chunk: it is a first block
    affected = np.broadcast_to(has[:, None, None], orc['S'].shape)
    share, elsewhere = _share_outside(sco.weight_grad(x, cut, g)['dW'], orc, affected)
    print('   second block of a chunk dropped, M = %d: %.3f of %d affected elements outside the bound' % (m, share, affected.sum()))
    assert share >= FLOOR and elsewhere == 0


# ---- the bound of the input gradient ---------------------------------------------------------------------------------------------------

BIG = 130 * sco.ROWS + 37       # 66 597 voxels of a side-33 grid: the map of the GPU tests


def _bf16(a):
    """float32 -> the float32 value of its bf16 rounding, to nearest even (csrc/bf16_split.h: bf16_rne)"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)).view(np.float32)


def _split(a):
    hi = _bf16(a)
    return hi.astype(np.float64), _bf16(np.asarray(a, dtype=np.float32) - hi).astype(np.float64)


@pytest.fixture(scope='module')
def big():
    nbr, inv, n_in, m = sco.table('same', sco.occupancy_map(BIG, 33, 0))
    assert n_in == m == BIG
    rng = np.random.default_rng(SEED + 5)
    w = (0.2 * rng.standard_normal((27, K, K))).astype(np.float32)
    g = rng.standard_normal((m, K)).astype(np.float32)
    return dict(nbr=nbr, inv=inv, w=w, g=g, dx=sco.input_grad(w, inv, g))


def test_input_grad_bound_holds_float32_and_the_three_product_split(big):
    w, inv, g, dx = big['w'], big['inv'], big['g'], big['dx']
    b32, bsp = sco.input_grad_bound(w, inv, g, 'fp32'), sco.input_grad_bound(w, inv, g, 'split_bf16')
    assert b32.shape == dx.shape and (b32 > 0).all() and (bsp > b32).all()
    # the bound is the documented one, on one element by hand
    a = 12345
    ks = np.nonzero(inv[:, a] >= 0)[0]
    S = sum(np.abs(g[inv[k, a]].astype(np.float64)) @ np.abs(w[k, 3].astype(np.float64)) for k in ks)
    assert 1 < ks.size < 27 and np.isclose(b32[a, 3], (ks.size * K + 32) * 2.0 ** -24 * S, rtol=1e-12)
    assert np.isclose(bsp[a, 3], (2.0 ** -16 + (ks.size * K + 32) * 2.0 ** -24) * S, rtol=1e-12)
    # a float32 evaluation
    d32 = np.zeros(dx.shape, dtype=np.float32)
    for k in range(27):
        sel = inv[k] >= 0
        d32[sel] += g[inv[k][sel]] @ w[k].T
    bad, worst, _ = sco.outside(d32, dx, b32)
    print('   float32 on the CPU: worst |d32 - d64| / fp32 bound = %.3f, outside: %d' % (worst, bad))
    assert d32.dtype == np.float32 and bad == 0 and 0 < worst < 1
    # hi hi' + hi lo' + lo hi' in float64: what the split leaves out, without any rounding of the sum
    (gh, gl), (wh, wl) = _split(g), _split(w)
    assert (np.abs(g - gh - gl) <= 2.0 ** -16 * np.abs(g)).all()              # (2^-8)^2: two roundings to 8 significant bits
    dsp = sco.input_grad(wh, inv, gh) + sco.input_grad(wl, inv, gh) + sco.input_grad(wh, inv, gl)
    bad, worst, _ = sco.outside(dsp, dx, bsp)
    print('   three-product split in float64: worst |dsp - d64| / split bound = %.3f, outside: %d' % (worst, bad))
    assert bad == 0 and 0 < worst < 1
    # the forward's bound is the same function with the roles exchanged: an element by hand
    x = g
    bf = sco.input_grad_bound(w, big['nbr'], x, 'fp32', forward=True)
    ks = np.nonzero(big['nbr'][:, a] >= 0)[0]
    S = sum(np.abs(x[big['nbr'][k, a]].astype(np.float64)) @ np.abs(w[k, :, 5].astype(np.float64)) for k in ks)
    assert np.isclose(bf[a, 5], (ks.size * K + 32) * 2.0 ** -24 * S, rtol=1e-12)


def test_wrong_input_gradients_leave_the_split_bound(big):
    w, inv, nbr, g, dx = big['w'], big['inv'], big['nbr'], big['g'], big['dx']
    bnd = sco.input_grad_bound(w, inv, g, 'split_bf16')
    rows = lambda mask: np.broadcast_to(np.asarray(mask)[:, None], dx.shape)
    off_centre = (np.delete(inv, 13, axis=0) >= 0).any(axis=0)
    variants = {
        'offset 26 - k': (sco.input_grad(w[::-1], inv, g), rows(off_centre)),
        '-1 as row 0': (sco.input_grad(w, np.where(inv < 0, 0, inv), g), rows((inv < 0).any(axis=0))),
        'forward table for the inverse': (sco.input_grad(w, nbr, g), rows(off_centre)),
        'slabs not transposed': (sco.input_grad(w.transpose(0, 2, 1), inv, g), rows(np.ones(BIG, dtype=bool))),
    }
    for name, (wrong, affected) in variants.items():
        out = ~(np.abs(wrong - dx) <= bnd)
        share, elsewhere = float((out & affected).sum()) / float(affected.sum()), int((out & ~affected).sum())
        print('   %-30s %.3f of %d affected elements outside the split bound' % (name, share, affected.sum()))
        assert share >= FLOOR and elsewhere == 0, (name, share, elsewhere)
