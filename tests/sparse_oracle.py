"""Plain checker of the sparse-structure layer (csrc/sparse_hash.h, csrc/sparse.hip, the key helpers of csrc/voxelize.hip and the
interpolation and the decoder's corner table of csrc/sparse_interp.hip) -- a checker, not a product path.  NumPy and Python only; it does not import the package.

  * ``lookup``          a Python dict over (b, x, y, z) tuples: row of each query coordinate, or -1.  No hashing of ours, no
                        packed keys: whatever the device table aliases, drops or fails to find shows as a difference.
  * ``neighbours``      [27, n_out], k = (ox+1) + 3 (oy+1) + 9 (oz+1): row of out + step * o_k.
  * ``strided_coords``  unique(floor(c / 2ts) * 2ts) in lexicographic (b, x, y, z) order, true floor for negative values.
  * ``interp``          sparse trilinear interpolation.  The coordinate chain is restated operation by operation in np.float32:
                            qc = ((p - min) / res) * ts,   c = floor(qc / ts) * ts (+ ts),   w = prod_d (1 - |qc - c| / ts)
                        (x, y, z order, starting from 1).  Every step is ONE IEEE operation on fp32 values (floor(.) * ts and the
                        added ts are exact for |c| < 2^24), so a fused multiply-add cannot change any of them: the corner rows and
                        the fp32 weights of a correct kernel are THESE, bit for bit.  A corner is absent when a coordinate leaves
                        [-8, 60000] (the kernels' range guard) or the dict does not hold it.  The value is sum_k w_k f_k over the
                        present corners in float64, not renormalised; S = sum_k |w_k f_k|.
  * ``pack_key``, ``hash_u64``, ``home_slot``   sparse_hash.h restated in uint64 arithmetic.  They CHOOSE INPUTS (coordinates whose
                        probe chain runs past the last slot); no expected result comes from them.

Bounds the tests use (u = 2^-24):
  * exact case: res a power of two, min_pts multiples of res, queries at min + (i + j/4) res, integer features: every weight is a
    multiple of 1/64, every product and partial sum an exactly representable number -> bit equality, whatever the compiler contracts.
  * generic case: the kernel's weights are the checker's; it rounds 8 products and 8 additions at most once each (a contracted
    multiply-add rounds once instead of twice), each by at most u times a partial sum of magnitude <= S (1 + 8u):
    |out - ref64| <= 9 u S to first order, for every element, no exemptions.  S = 0 (no corner present) demands exact zero.
"""
import numpy as np

U = 2.0 ** -24
INTERP_BOUND = 9 * U
GUARD = 8                      # coordinates may lie (and be probed) this far below zero
COORD_MAX = 65535 - 2 * GUARD  # largest coordinate the table stores
INTERP_MAX = 60000             # the interpolation kernels look no corner up beyond this


def _rows(coords):
    coords = np.asarray(coords).reshape(-1, 4)
    table = {}
    for i, c in enumerate(coords.tolist()):
        assert tuple(c) not in table, 'coordinate rows must be unique'
        table[tuple(c)] = i
    return table


def lookup(coords, queries, _table=None):
    """Row of every query (b, x, y, z) in ``coords`` (unique rows), or -1.  -> int64 [n_q]."""
    table = _rows(coords) if _table is None else _table
    q = np.asarray(queries).reshape(-1, 4)
    return np.fromiter((table.get(tuple(r), -1) for r in q.tolist()), dtype=np.int64, count=q.shape[0])


def offsets():
    """[27, 3] (ox, oy, oz), k = (ox+1) + 3 (oy+1) + 9 (oz+1): the first spatial axis runs fastest."""
    return np.array([(ox, oy, oz) for oz in (-1, 0, 1) for oy in (-1, 0, 1) for ox in (-1, 0, 1)], dtype=np.int64)


def neighbours(coords, out_coords, step):
    """-> int64 [27, n_out]: row of out_coords[p] + step * o_k in ``coords``, or -1."""
    table = _rows(coords)
    out = np.asarray(out_coords, dtype=np.int64).reshape(-1, 4)
    nbr = np.empty((27, out.shape[0]), dtype=np.int64)
    for k, o in enumerate(offsets()):
        q = out.copy()
        q[:, 1:] += step * o
        nbr[k] = lookup(None, q, table)
    return nbr


def strided_coords(coords, ts):
    """Output coordinate map of a stride-2 convolution on a map of tensor stride ts.  -> int64 [m, 4], lexicographic."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    out = set()
    for b, x, y, z in c.tolist():
        out.add((b,) + tuple((v // (2 * ts)) * (2 * ts) for v in (x, y, z)))       # Python's // is floor division
    return np.array(sorted(out), dtype=np.int64).reshape(-1, 4)


def query_coords(pts, pts_batch, n_hyp, min_pts, res, ts):
    """qc = ((p - min_pts[batch]) / res) * ts in np.float32, one operation at a time.  pts [n_pts, n_hyp, 3] (or [n_q, 3]),
    pts_batch [n_pts].  -> (b int64 [n_q], qc float32 [n_q, 3])."""
    p = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    b = np.repeat(np.asarray(pts_batch, dtype=np.int64).reshape(-1), n_hyp)
    assert b.shape[0] == p.shape[0]
    mn = np.asarray(min_pts, dtype=np.float32).reshape(-1, 3)
    assert b.min() >= 0 and b.max() < mn.shape[0]
    d = p - mn[b]
    assert d.dtype == np.float32
    q = d / np.float32(res)
    qc = q * np.float32(ts)
    assert qc.dtype == np.float32
    return b, qc


def corner_table(coords, ts, pts, pts_batch, n_hyp, min_pts, res):
    """-> (rows int64 [n_q, 8] (-1: absent), w float32 [n_q, 8], qc float32 [n_q, 3]); corner bit d set = upper corner on axis d."""
    table = _rows(coords)
    b, qc = query_coords(pts, pts_batch, n_hyp, min_pts, res, ts)
    tsf = np.float32(ts)
    lo = np.floor(qc / tsf) * tsf
    n = qc.shape[0]
    rows = np.full((n, 8), -1, dtype=np.int64)
    w = np.empty((n, 8), dtype=np.float32)
    for k in range(8):
        off = np.array([(k >> d) & 1 for d in range(3)], dtype=np.float32) * tsf
        c = lo + off
        wk = np.ones(n, dtype=np.float32)
        for d in range(3):
            wk = wk * (np.float32(1) - np.abs(qc[:, d] - c[:, d]) / tsf)
        assert c.dtype == np.float32 and wk.dtype == np.float32
        w[:, k] = wk
        with np.errstate(invalid='ignore'):
            ok = np.all((c >= -GUARD) & (c <= INTERP_MAX), axis=1)
        idx = np.nonzero(ok)[0]
        if idx.size:
            q = np.concatenate((b[idx, None], c[idx].astype(np.int64)), axis=1)
            rows[idx, k] = lookup(None, q, table)
    return rows, w, qc


def interp(coords, feats, ts, pts, pts_batch, n_hyp, min_pts, res):
    """-> (value float64 [n_q, C], S float64 [n_q, C]): sum_k w_k f_k and sum_k |w_k f_k| over the present corners."""
    rows, w, _ = corner_table(coords, ts, pts, pts_batch, n_hyp, min_pts, res)
    f = np.asarray(feats, dtype=np.float32).astype(np.float64)
    val = np.zeros((rows.shape[0], f.shape[1]))
    s = np.zeros_like(val)
    for k in range(8):
        m = rows[:, k] >= 0
        t = w[m, k].astype(np.float64)[:, None] * f[rows[m, k]]
        val[m] += t
        s[m] += np.abs(t)
    return val, s


# ---- sparse_hash.h restated: used to choose inputs only --------------------------------------------------------------------------

def pack_key(b, x, y, z):
    b, x, y, z = (np.asarray(v, dtype=np.int64) for v in (b, x, y, z))
    f = lambda v: (v & 0xffff).astype(np.uint64)
    return (f(b) << np.uint64(48)) | (f(x + GUARD) << np.uint64(32)) | (f(y + GUARD) << np.uint64(16)) | f(z + GUARD)


def hash_u64(key):
    """The 64-bit finaliser of sparse_hash.h (xor-shift 33, two odd multipliers), low 32 bits."""
    k = np.array(key, dtype=np.uint64, ndmin=1)
    s = np.uint64(33)
    with np.errstate(over='ignore'):
        k = k ^ (k >> s)
        k = k * np.uint64(0xff51afd7ed558ccd)
        k = k ^ (k >> s)
        k = k * np.uint64(0xc4ceb9fe1a85ec53)
        k = k ^ (k >> s)
    return k & np.uint64(0xffffffff)


def table_capacity(n):
    """Smallest power of two >= 4 n, at least 64."""
    cap = 64
    while cap < 4 * max(n, 1):
        cap *= 2
    return cap


def home_slot(coords, n):
    """Slot at which the probe chain of each coordinate row starts in the table of an n-row map."""
    c = np.asarray(coords, dtype=np.int64).reshape(-1, 4)
    return (hash_u64(pack_key(c[:, 0], c[:, 1], c[:, 2], c[:, 3])) & np.uint64(table_capacity(n) - 1)).astype(np.int64)
