"""NumPy float64 oracle of the sparse convolution's backward pass over tests/sparse_oracle.py's coordinate maps.

For a table nbr = A.neighbors(B.coords, step) ([27, n_B], rows of A or -1; sparse_oracle.neighbours(A, B, step)), a source x [n_A, K],
a kernel w [27, K, N] and the gradient g [n_B, N] of the output y[p] = sum_k [nbr[k, p] >= 0] x[nbr[k, p]] @ w[k]:

  weight gradient   dW[k, ci, co] = sum_p [nbr[k, p] >= 0] x[nbr[k, p], ci] g[p, co]                       (`weight_grad`)
  input gradient    dx[a]         = sum_k [inv[k, a] >= 0] g[inv[k, a]] @ w[k]^T,  inv = B.neighbors(A.coords, -step)   (`input_grad`)

The second line is the forward gather-GEMM run backwards: nbr[k, p] = a  <=>  A[a] = B[p] + step o_k  <=>  B[p] = A[a] - step o_k  <=>
inv[k, a] = p, with the SAME offset index k and every slab transposed.  `input_grad_scatter` is the definition (a scatter-add over the
forward table) the CPU test holds it to.  For a same-level table (A = B) the inverse is the table with its 27 rows reversed
(o_{26 - k} = -o_k); the inverse of a `down` table (A fine, B coarse, step = ts) is the `up` table coarse.neighbors(fine, -ts), and
the reverse.

Bound of the weight gradient, per element: with cnt_k the present rows of offset k and S = sum_p |x| |g| over them,

  |dW_kernel - dW_64| <= (cnt_k + 32) u S,   u = 2^-24,

cnt_k - 1 additions in any order are (cnt_k - 1) u S to first order; the 32 are tests/psv_backward_oracle.py's constant and hold the
product roundings, the additions of the chunk partials and the matrix instruction's internal order.  S = 0 demands exact zero.

Bound of the input gradient (`input_grad_bound`), and of the forward with (x, nbr) in place of (g, inv): per element, with
n = (present offsets of the row) x (contracted width) and S = sum |g| |w| over the same terms,

  'fp32'         |dx_kernel - dx_64| <= (n + 32) u S                     the same constant: n - 1 additions in any order
  'split_bf16'   |dx_kernel - dx_64| <= (2^-16 + (n + 32) u) S

The 2^-16 comes from csrc/bf16_split.h, not from a measurement: an operand a is carried as hi + lo with hi = RNE_bf16(a) and
lo = RNE_bf16(a - hi); the kernel forms hi hi' + hi lo' + lo hi' and drops lo lo'.  A product is off by the residual a - hi - lo of
either operand and by the dropped term: three terms.  With the mean rounding error of 8 significant bits, 2^-9 |a| per rounding,
each of the three is 2^-18 |a a'| and their sum is below 2^-16 |a a'|: that is the constant.  It is NOT the worst case of one
product: half an ulp of bf16 at the bottom of a binade is 2^-8 |a|, so a single operand can keep a residual of 2^-16 |a| and a single
product can be off by 3 * 2^-16 |a a'| (tests/test_sparse_conv_backward_oracle.py meets such operands in random data).  The bound
is on a sum over n >= 16 products whose residuals are independent in size and sign; the three-product split evaluated in float64 on
a 66 597-voxel map stays at 0.10 of it.  The bf16 products are exact in the fp32 accumulator and their additions are the
(n + 32) u S of the fp32 mode.  S = 0 demands exact zero.

`synthetic_table` builds tables without a coordinate map: the header makes entries in [-1, n_in) the caller's contract, so any such
table is legal, and the patterns put the present rows where the compaction of the weight-gradient kernel (two ballots per wave,
a prefix over eight wave counts, tiles of 32 present rows, blocks of 512 table entries) has its edges.
"""
import numpy as np

import sparse_oracle as so

U = 2.0 ** -24
C_BOUND = 32.0
ROWS = 512                  # rows per compaction block of the kernel; restated from gemm_wgrad.hip (the GPU test cites the line)
MAX_CHUNKS = 128
TILE = 32


def chunks(M):
    """(number of chunks, rows per chunk) of v3d_sparse_conv_weight_grad_f32: a function of M alone."""
    nblk = -(-M // ROWS)
    per = -(-nblk // MAX_CHUNKS)
    return (-(-nblk // per) if per else 0), per * ROWS


def _spread(q):
    """q = p % ROWS -> a permutation of [0, ROWS) (107 is odd; 107 * 67 = 1 mod 512): `_spread(q) < c` names the c rows 67 j mod 512,
    j < c, which for c >= 8 lie in every wave of both halves."""
    return (q * 107) % ROWS


# which rows p are present, as a rule on q = p % ROWS and b = p // ROWS (M: the number of rows)
PATTERNS = {
    'every':      lambda p, q, b, M: np.ones_like(p, dtype=bool),
    'none':       lambda p, q, b, M: np.zeros_like(p, dtype=bool),
    'first':      lambda p, q, b, M: p == 0,
    'last':       lambda p, q, b, M: p == M - 1,
    'wave0':      lambda p, q, b, M: q < 64,                                  # one wave of the first half ...
    'wave3':      lambda p, q, b, M: (q >= 192) & (q < 256),
    'wave4':      lambda p, q, b, M: (q >= 256) & (q < 320),                  # ... and of the second
    'wave7':      lambda p, q, b, M: q >= 448,
    'odd_blocks': lambda p, q, b, M: b % 2 == 1,                              # empty blocks between full ones
    'tile_edge':  lambda p, q, b, M: _spread(q) < 31 + b % 3,                 # 31, 32, 33 present rows in consecutive blocks
}
ALL_PATTERNS = tuple(PATTERNS) + ('half',)


def synthetic_table(M, n_in, patterns, seed):
    """A neighbour table without a coordinate map -> int64 [len(patterns), M], entries in [-1, n_in).  Row k holds the rows of
    `patterns[k]` (a key of PATTERNS, or 'half': a seeded random half); its present rows map to DISTINCT source rows through a
    seeded permutation of its own (injective per offset, as a real table is), so a gather of the wrong row changes the sum."""
    assert n_in >= M
    rng = np.random.default_rng(seed)
    p = np.arange(M, dtype=np.int64)
    nbr = np.full((len(patterns), M), -1, dtype=np.int64)
    for k, name in enumerate(patterns):
        present = rng.random(M) < 0.5 if name == 'half' else PATTERNS[name](p, p % ROWS, p // ROWS, M)
        rows = rng.permutation(n_in)[:M]
        nbr[k, present] = rows[present]
    return nbr


def occupancy_map(n, side, seed, lattice=1):
    """n voxels of a two-batch side^3 grid (coordinates from -2 on, times `lattice`), in lexicographic order.  -> int64 [n, 4]"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(2), np.arange(side), np.arange(side), np.arange(side), indexing='ij'), -1).reshape(-1, 4)
    c = g[np.sort(rng.choice(g.shape[0], n, replace=False))].astype(np.int64)
    c[:, 1:] = (c[:, 1:] - 2) * lattice
    return c


_tables = {}


def map_tables(kind, n, side, seed):
    """`table(kind, occupancy_map(n, side, seed))` and the coordinates, computed once per process and read-only: the large maps take
    seconds to build.  -> (nbr, inv, n_in, M, coords[, coarse coords])"""
    key = (kind, n, side, seed)
    if key not in _tables:
        c = occupancy_map(n, side, seed)
        res = table(kind, c) + (c,) + (() if kind == 'same' else (so.strided_coords(c, 1),))
        for a in res:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _tables[key] = res
    return _tables[key]


def table(kind, coords, ts=1):
    """-> (nbr int64 [27, M], inv int64 [27, n_in], n_in, M) of a 'same', 'down' or 'up' convolution on `coords` (tensor stride ts)."""
    if kind == 'same':
        nbr = so.neighbours(coords, coords, ts)
        return nbr, so.neighbours(coords, coords, -ts), coords.shape[0], coords.shape[0]
    coarse = so.strided_coords(coords, ts)
    down, up = so.neighbours(coords, coarse, ts), so.neighbours(coarse, coords, -ts)
    if kind == 'down':
        return down, up, coords.shape[0], coarse.shape[0]
    assert kind == 'up'
    return up, down, coarse.shape[0], coords.shape[0]


def weight_grad(x, nbr, g):
    """x [n_in, K], nbr [n_seg, M], g [M, N] (the valid columns only) -> dict(dW, S float64 [n_seg, K, N], cnt int64 [n_seg])."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    n_seg = nbr.shape[0]
    dW = np.zeros((n_seg, x.shape[1], g.shape[1]))
    S = np.zeros_like(dW)
    cnt = np.zeros(n_seg, dtype=np.int64)
    for k in range(n_seg):
        sel = nbr[k] >= 0
        cnt[k] = sel.sum()
        xk, gk = x[nbr[k][sel]], g[sel]
        dW[k] = xk.T @ gk
        S[k] = np.abs(xk).T @ np.abs(gk)
    return dict(dW=dW, S=S, cnt=cnt)


def bound(orc):
    return (orc['cnt'][:, None, None] + C_BOUND) * U * orc['S']


def violations(got, orc):
    """-> (elements outside the bound, worst |got - dW| / bound over S > 0, largest |got| over S == 0); a NaN is outside."""
    return outside(got, orc['dW'], bound(orc))


def input_grad(w, inv, g):
    """The gather formulation: w [27, K, N], inv [27, n_in] (rows of g or -1), g [M, N] -> dx float64 [n_in, K]."""
    w, g = np.asarray(w, dtype=np.float64), np.asarray(g, dtype=np.float64)
    dx = np.zeros((inv.shape[1], w.shape[1]))
    for k in range(inv.shape[0]):
        sel = inv[k] >= 0
        dx[sel] += g[inv[k][sel]] @ w[k].T
    return dx


def input_grad_scatter(w, nbr, g, n_in):
    """The definition: the adjoint of the forward's gather, a scatter-add over the forward table nbr [27, M] (rows of x or -1)."""
    w, g = np.asarray(w, dtype=np.float64), np.asarray(g, dtype=np.float64)
    dx = np.zeros((n_in, w.shape[1]))
    for k in range(nbr.shape[0]):
        sel = nbr[k] >= 0
        np.add.at(dx, nbr[k][sel], g[sel] @ w[k].T)
    return dx


def forward(x, w, nbr):
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    y = np.zeros((nbr.shape[1], w.shape[2]))
    for k in range(nbr.shape[0]):
        sel = nbr[k] >= 0
        y[sel] += x[nbr[k][sel]] @ w[k]
    return y


def term_sums(w, inv, g, forward=False):
    """-> (n int64 [rows, 1], S float64 [rows, width out]) of dx = input_grad(w, inv, g) (forward=True: of y = forward(x, w, nbr) with
    (x, nbr) passed as (g, inv)): n = present offsets of the row x contracted width, S = sum |g| |w| over the same terms."""
    w, g = np.abs(np.asarray(w, dtype=np.float64)), np.abs(np.asarray(g, dtype=np.float64))
    width = w.shape[1] if forward else w.shape[2]                             # the contracted width
    S = np.zeros((inv.shape[1], w.shape[2] if forward else w.shape[1]))
    for k in range(inv.shape[0]):
        sel = inv[k] >= 0
        S[sel] += g[inv[k][sel]] @ (w[k] if forward else w[k].T)
    return (inv >= 0).sum(axis=0)[:, None] * width, S


def input_grad_bound(w, inv, g, precision, forward=False, sums=None):
    """Per-element bound of dx = input_grad(w, inv, g) [n_in, K] for a kernel in `precision` ('fp32' or 'split_bf16'; the module
    docstring derives both).  forward=True: of y = forward(x, w, nbr) [M, N] with (x, nbr) passed as (g, inv).  `sums`: the result
    of term_sums on the same arguments, where it is at hand.  -> float64 array of the result's shape; 0 where no term is present
    (S = 0: exact zero is demanded)."""
    n, S = term_sums(w, inv, g, forward) if sums is None else sums
    rel = {'fp32': 0.0, 'split_bf16': 2.0 ** -16}[precision]
    return (rel + (n + C_BOUND) * U) * S


def outside(got, ref, bnd):
    """-> (elements outside the bound, worst |got - ref| / bound over bound > 0, largest |got| over bound == 0); a NaN is outside."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    pos = bnd > 0
    bad = int((~(err <= bnd)).sum())
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(pos, err / np.where(pos, bnd, 1.0), 0.0)
    worst = float(np.nanmax(ratio)) if pos.any() else 0.0
    zero = np.abs(got[~pos])
    return bad, worst, float(zero.max()) if zero.size else 0.0


def make_case(nbr, n_in, K, N, seed, pad_src=0, pad_grad=0, poison=np.nan):
    """Seeded inputs of one call: src [n_in, K + pad_src] and grad_out [M, N + pad_grad] float32, `poison` in the unused columns and
    in every src row no table entry names; nbr as int32.  -> dict(src, grad_out, nbr, x, g, M, n_in, K, N, ld_src, ld_grad)."""
    rng = np.random.default_rng(seed)
    M = nbr.shape[1]
    src = np.full((n_in, K + pad_src), poison, dtype=np.float32)
    src[:, :K] = rng.standard_normal((n_in, K)).astype(np.float32)
    used = np.zeros(n_in, dtype=bool)
    used[nbr[nbr >= 0]] = True
    src[~used] = poison
    grad = np.full((M, N + pad_grad), poison, dtype=np.float32)
    grad[:, :N] = rng.standard_normal((M, N)).astype(np.float32)
    x = np.where(used[:, None], src[:, :K], 0.0)                              # rows nobody names never enter a sum
    return dict(src=src, grad_out=grad, nbr=np.ascontiguousarray(nbr, dtype=np.int32), x=x, g=grad[:, :N], M=M, n_in=n_in, K=K, N=N,
                ld_src=K + pad_src, ld_grad=N + pad_grad)
