"""Plain checker of the backward of the sparse trilinear interpolation (csrc/sparse_interp.hip, v3d_sparse_interp_backward_f32) -- a
checker, not a product path.  NumPy only, built on tests/sparse_oracle.py, whose ``corner_table`` restates the forward's corner
rows and fp32 weights bit for bit.  The operation is the adjoint of the interpolation with respect to the level features:

    grad_feats[r, c] = sum over the corner slots (q, k) with row(q, k) == r of  w(q, k) * grad_out[q, col0 + c]

  * ``gradient(case)``  -> ``g64`` [N, C] the sums in float64, ``S`` [N, C] = sum |w * g_out|, ``cnt`` [N] the list lengths.
  * ``bound(orc)``      = (cnt + 2) * 2^-24 * S per element, no exemptions (u = 2^-24).  The weights are the checker's own fp32
                        numbers.  A row's sum is cnt products and cnt - 1 additions in SOME order (the first addition, to +0,
                        is exact).  Each product is rounded at most once (not at all inside a fused multiply-add) by at most
                        u |term|: u S in total.  Each addition rounds a partial sum of magnitude <= S (1 + cnt u) by at most u
                        times that: (cnt - 1) u S to first order.  Together cnt u S; the + 2 holds the second-order terms
                        (cnt^2 u^2 S < 2 u S for cnt < 5800; the longest list of these cases is below 2000 and asserted).
                        The chunked second pass needs no further term: a row of m chunks with cnt_1 .. cnt_m slots takes
                        sum_j (cnt_j - 1) additions inside its chunks and m - 1 additions of partial sums, cnt - 1 in all, each
                        of a partial sum of magnitude <= S -- it is one more summation order of the same cnt terms.
                        S == 0 (a row nobody touches, or only with zero gradients) demands exact zero.
  * exact cases         res = 2^-4, min_pts multiples of res, queries at min + (i + j/4) res, small integer gradients: every
                        weight is a multiple of 1/64, every product a multiple of 1/64 below 2^4 and every partial sum a
                        multiple of 1/64 below 2^15 -- exactly representable, whatever the order and whatever the compiler
                        contracts: bit equality with g64.
  * ``variant``         wrong backward passes for tests/test_sparse_interp_backward_oracle.py; never used for an expected value.

Cases (``CASES``; ``build(param)``): a map of about 200 rows in shuffled order over two batch elements with different min_pts whose
coordinates start at the -8 guard; a few thousand queries: inside the map, on its rim (some corners absent), wholly outside,
beyond the 60000 range guard, exactly on lattice points and at quarter-cell positions.  ``hot`` cases put 3 CHUNK + CHUNK / 3
queries into one cell, so that eight rows have lists of more than three full chunks beside rows with lists of 0 and 1;
``strided`` cases hold the gradient in rows of ld_grad > C floats from column col0 > 0 on, NaN elsewhere.
"""
import numpy as np

import sparse_oracle as so

U = 2.0 ** -24
CHUNK = 512                          # kInterpBwdChunk of csrc/sparse_interp.hip (test_sparse_interp_backward_oracle.py compares them)
RES = 0.0625
MIN_PTS = np.array([[-1.25, 0.5, 3.0], [2.0, -0.75, 0.0625]], dtype=np.float32)
SIDE = 5
N_HOT = 3 * CHUNK + CHUNK // 3

# (kind, C, tensor stride, n_hyp)
GENERIC_CASES = [('generic', C, ts, n_hyp) for C in (4, 64, 128) for ts in (1, 2, 4) for n_hyp in (1, 7)]
EXACT_CASES = [('exact', 64, 1, 7), ('exact', 4, 2, 1), ('exact', 128, 4, 7)]
HOT_CASES = [('hot', 128, 2, 1), ('hot_exact', 64, 1, 7)]
STRIDED_CASES = [('strided', 64, 2, 7), ('strided_vec', 128, 1, 1)]
CASES = GENERIC_CASES + EXACT_CASES + HOT_CASES + STRIDED_CASES
VARIANTS = ('one_minus_w', 'reversed_bits', 'clamp_absent', 'batch_by_query', 'col0_ignored', 'drop_last_chunk')


def case_id(param):
    return '%s-C%d-ts%d-h%d' % param


def is_exact(param):
    return param[0] in ('exact', 'hot_exact')


def _map(rng, ts):
    """~200 of the 2 * 5^3 lattice points of a block that starts at coordinate -8, in shuffled order."""
    lo = -so.GUARD // ts
    g = np.stack(np.meshgrid(np.arange(2), np.arange(SIDE), np.arange(SIDE), np.arange(SIDE), indexing='ij'), -1).reshape(-1, 4)
    coords = np.concatenate((g[:, :1], (g[:, 1:] + lo) * ts), axis=1).astype(np.int64)
    keep = rng.random(coords.shape[0]) < 0.8
    keep[[0, SIDE ** 3]] = True                                    # the corner at (-8, -8, -8) of both batch elements
    # two isolated rows away from every query but one: (lo + 12)^3 is never touched, (lo + 15)^3 by exactly one corner slot
    lone = np.array([[0] + [(lo + 12) * ts] * 3, [1] + [(lo + 15) * ts] * 3], dtype=np.int64)
    coords = np.concatenate((coords[keep], lone))
    return coords[rng.permutation(coords.shape[0])], lo


def build(param):
    kind, C, ts, n_hyp = param
    exact = is_exact(param)
    rng = np.random.default_rng(7000 + 97 * C + 13 * ts + n_hyp + 1000 * len(kind))
    coords, lo = _map(rng, ts)
    n_pts = (3000 if n_hyp == 1 else 600)
    n_each = n_pts // 10
    # positions in lattice units of the level (cells), relative to min_pts
    inside = rng.uniform(lo, lo + SIDE - 1, (5 * n_each, 3))
    rim = rng.uniform(lo - 1.5, lo + SIDE + 0.5, (2 * n_each, 3))
    rim[np.arange(rim.shape[0]), rng.integers(0, 3, rim.shape[0])] = rng.choice([lo - 0.5, lo + SIDE - 0.5], rim.shape[0])
    outside = rng.uniform(lo, lo + SIDE, (n_each, 3)) + rng.choice([-40.0, 30.0, 70000.0, 1e6], (n_each, 1)) * \
        np.eye(3)[rng.integers(0, 3, n_each)]
    lattice = rng.integers(lo - 1, lo + SIDE + 1, (n_each, 3)).astype(np.float64)
    quarter = rng.integers(4 * lo - 4, 4 * (lo + SIDE), (n_pts - 9 * n_each, 3)) / 4.0
    base = np.concatenate((inside, rim, outside, lattice, quarter))
    kinds = np.array(['inside'] * len(inside) + ['rim'] * len(rim) + ['outside'] * len(outside) + ['lattice'] * len(lattice) +
                     ['quarter'] * len(quarter))
    if kind.startswith('hot'):
        # N_HOT queries (points x hypotheses) in ONE cell whose 8 corners are all present, in batch element 0
        present = set(map(tuple, coords.tolist()))
        cell = next(c for c in coords[coords[:, 0] == 0].tolist()
                    if all((0, c[1] + dx * ts, c[2] + dy * ts, c[3] + dz * ts) in present for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)))
        n_hot_pts = -(-N_HOT // n_hyp)
        hot = np.array(cell[1:]) / ts + rng.uniform(0.05, 0.3, (n_hot_pts, 3))
        base = np.concatenate((hot, base))
        kinds = np.concatenate((np.array(['hot'] * n_hot_pts), kinds))
    if exact:
        base = np.round(base * 4) / 4
    base = np.concatenate((base, np.full((1, 3), lo + 15.0)))     # on the isolated lattice point; its other hypotheses step past it
    kinds = np.concatenate((kinds, np.array(['single'])))
    n_pts = base.shape[0]
    pts_batch = rng.integers(0, 2, n_pts)
    pts_batch[kinds == 'hot'] = 0
    pts_batch[kinds == 'single'] = 1
    step = rng.uniform(-0.2, 0.2, (n_pts, 1, 3))
    if exact:
        step = np.round(step * 4) / 4 + 0.25
    step[kinds == 'single'] = 3.0
    g = base[:, None, :] + step * np.arange(n_hyp)[None, :, None]
    if kind.startswith('hot'):
        g[kinds == 'hot'] = base[kinds == 'hot'][:, None, :] + (step[kinds == 'hot'] * 0.25 if not exact else 0.0) * np.arange(n_hyp)[None, :, None]
    p64 = MIN_PTS[pts_batch].astype(np.float64)[:, None, :] + g * RES
    pts = p64.astype(np.float32)
    nq = n_pts * n_hyp
    ld, col0 = {'strided': (C + 11, 5), 'strided_vec': (C + 12, 8)}.get(kind, (C, 0))
    grad = rng.integers(-8, 9, (nq, C)).astype(np.float32) if exact else rng.standard_normal((nq, C)).astype(np.float32)
    grad_out = np.full((nq, ld), np.nan, dtype=np.float32)
    grad_out[:, col0:col0 + C] = grad
    return dict(param=param, coords=coords, ts=ts, C=C, n_hyp=n_hyp, n_pts=n_pts, pts=pts, pts_batch=pts_batch.astype(np.int64),
                min_pts=MIN_PTS, res=RES, grad_out=grad_out, ld=ld, col0=col0, kinds=kinds, lattice_units=g, exact=exact)


def _reverse3(k):
    return ((k & 1) << 2) | (k & 2) | ((k >> 2) & 1)


def corner_lists(case, variant=None):
    """-> (rows int64 [nq, 8] (-1 absent), w float32 [nq, 8]) of the forward (or of a wrong variant)."""
    n_hyp, pts, pb = case['n_hyp'], case['pts'], case['pts_batch']
    if variant == 'batch_by_query':                              # pts_batch[q] (wrapped) instead of pts_batch[q // n_hyp]
        pb = pb[np.arange(case['n_pts'] * n_hyp) % case['n_pts']]
        pts, n_hyp = pts.reshape(-1, 1, 3), 1
    rows, w, _ = so.corner_table(case['coords'], case['ts'], pts, pb, n_hyp, case['min_pts'], case['res'])
    if variant == 'one_minus_w':
        w = np.float32(1) - w
    elif variant == 'reversed_bits':                             # the row of corner k with the weight of the bit-reversed corner
        w = w[:, [_reverse3(k) for k in range(8)]]
    elif variant == 'clamp_absent':
        rows = np.maximum(rows, 0)
    return rows, w


def gradient(case, variant=None):
    rows, w = corner_lists(case, variant)
    N, C, col0 = case['coords'].shape[0], case['C'], case['col0']
    if variant == 'col0_ignored':
        col0 = 0
    g = case['grad_out'][:, col0:col0 + C].astype(np.float64)
    flat_rows, flat_w = rows.reshape(-1), w.reshape(-1).astype(np.float64)      # slot order q * 8 + k: the list order of a row
    slot = np.arange(flat_rows.shape[0])
    keep = flat_rows >= 0
    if variant == 'drop_last_chunk':                             # rows of more than one chunk lose their last chunk
        order = np.argsort(np.where(keep, flat_rows, N), kind='stable')
        sorted_rows = np.where(keep, flat_rows, N)[order]
        start = np.searchsorted(sorted_rows, sorted_rows, side='left')
        pos = np.arange(order.shape[0]) - start
        cnt_sorted = np.bincount(sorted_rows, minlength=N + 1)[sorted_rows]
        last = (cnt_sorted > CHUNK) & (pos >= (cnt_sorted - 1) // CHUNK * CHUNK)
        keep = keep.copy()
        keep[order[last]] = False
    r, s = flat_rows[keep], slot[keep]
    term = flat_w[s][:, None] * g[s >> 3]
    g64 = np.zeros((N, C))
    S = np.zeros((N, C))
    np.add.at(g64, r, term)
    np.add.at(S, r, np.abs(term))
    cnt = np.bincount(r, minlength=N).astype(np.int64)
    return dict(g64=g64, S=S, cnt=cnt, rows=rows, w=w)


def bound(orc):
    return (orc['cnt'][:, None] + 2) * U * orc['S']


def violations(g, orc):
    """-> (elements outside the bound (NaN counts as outside), worst |g - g64| / bound where S > 0, worst |g| where S == 0)."""
    g = np.asarray(g, dtype=np.float64)
    err = np.abs(g - orc['g64'])
    b = bound(orc)
    bad = ~(err <= b)
    m = orc['S'] > 0
    with np.errstate(invalid='ignore'):
        worst = float(np.nanmax(err[m] / b[m])) if m.any() else 0.0
    worst_zero = float(np.abs(g[~m]).max()) if (~m).any() else 0.0
    return int(bad.sum()), worst, worst_zero
