"""Float64 checker of the 3D cloud metrics (3dvnet_amd/metrics3d.py, csrc/cloudmetrics.hip) -- a checker, not a product path.
NumPy / torch only (the GPU tests import it).

  * ``voxel_down_sample``  the specification of the down-sample, literally: vmin = double(min) - voxel / 2, cell =
                           floor((double(p) - vmin) / voxel), key = x 2^42 + y 2^21 + z, mean of the member rows summed in
                           double in original row order, divided by the count, rounded once to fp32; ascending key.
  * ``nearest``            chunked float64 brute force: index and distance of the nearest target row and the distance of the
                           second nearest (the gap decides where an fp32 evaluation may legitimately pick another row).
  * ``metrics``            acc / comp / prec / recal / fscore of two distance arrays (metricfunctions.py:84-98).

Bounds the tests use (u = 2^-24): an fp32 distance sqrt(dx^2 + dy^2 + dz^2) from fp32 differences carries one rounding per
difference (u each, 2u on the square), u per product, u per sum, all halved by the root, plus the root's own u: 3.5u to first
order; the bound is 4u.  Two neighbours closer than 8u d2 (twice that, relative to the farther one) can swap.
"""
import numpy as np
import torch

U = 2.0 ** -24
DIST_BOUND = 4 * U
GAP_BOUND = 8 * U
KEYS = ('acc', 'comp', 'prec', 'recal', 'fscore')


def room(n, noise, seed, outliers=0.0, dims=(6., 3., 5.)):
    """n seeded samples on the six faces of a box room + N(0, noise); the first ``outliers * n`` rows are displaced by
    N(0, 0.5 m).  -> float32 [n, 3]."""
    rng = np.random.default_rng(seed)
    dims = np.asarray(dims)
    f = rng.integers(0, 6, n)
    p = rng.random((n, 3)) * dims
    ax, side = f // 2, f % 2
    p[np.arange(n), ax] = side * dims[ax]
    p += rng.normal(0, noise, (n, 3))
    k = int(outliers * n)
    p[:k] += rng.normal(0, 0.5, (k, 3))
    return p.astype(np.float32)


def voxel_keys(p, voxel):
    p64 = np.asarray(p, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    vmin = p64.min(0) - 0.5 * voxel
    idx = np.floor((p64 - vmin) / voxel).astype(np.int64)
    assert idx.min() >= 0 and idx.max() < 2 ** 21
    return (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]


def voxel_down_sample(p, voxel, attr=None):
    """-> dict(pts f32 [m, 3], pts64, attr f32 [m, k] | None, attr64, keys [m] ascending, counts [m])."""
    p = np.asarray(p, dtype=np.float32).reshape(-1, 3)
    if p.shape[0] == 0:
        return dict(pts=p, pts64=p.astype(np.float64), attr=None, attr64=None, keys=np.zeros(0, np.int64), counts=np.zeros(0, np.int64))
    key = voxel_keys(p, voxel)
    keys, inv, counts = np.unique(key, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)

    def mean(x):
        s = np.zeros((len(keys), x.shape[1]))
        np.add.at(s, inv, x.astype(np.float64))            # unbuffered: adds in row order
        return s / counts[:, None].astype(np.float64)

    pts64 = mean(p)
    out = dict(pts=pts64.astype(np.float32), pts64=pts64, attr=None, attr64=None, keys=keys, counts=counts)
    if attr is not None:
        a64 = mean(np.asarray(attr, dtype=np.float32).reshape(p.shape[0], -1))
        out.update(attr=a64.astype(np.float32), attr64=a64)
    return out


def nearest(target, query, device='cpu', chunk_elems=1 << 25, distinct=False):
    """For every query row: (idx int64, d1, d2) of the nearest / the distance of the second nearest target row, float64,
    brute force in chunks.  Ties in float64 resolve to the lowest index.  d2 = inf for a single-row target.
    ``distinct=True`` (clouds with exact duplicate rows): the search runs over the distinct target rows, so d2 is the
    distance of the second nearest distinct POINT, and idx is the first row holding the nearest one -- exact duplicates
    have equal fp32 distances, among which the lowest row is the specified answer."""
    if distinct:
        tn = np.asarray(target.cpu() if torch.is_tensor(target) else target, dtype=np.float32).reshape(-1, 3)
        uniq, first = np.unique(tn, axis=0, return_index=True)
        idx, d1, d2 = nearest(uniq, query, device, chunk_elems)
        return torch.as_tensor(first).to(idx.device)[idx], d1, d2
    t = torch.as_tensor(np.asarray(target) if not torch.is_tensor(target) else target).to(device).double().reshape(-1, 3)
    q = torch.as_tensor(np.asarray(query) if not torch.is_tensor(query) else query).to(device).double().reshape(-1, 3)
    n, m = t.shape[0], q.shape[0]
    idx = torch.empty(m, dtype=torch.long, device=t.device)
    d1 = torch.empty(m, dtype=torch.float64, device=t.device)
    d2 = torch.full((m,), float('inf'), dtype=torch.float64, device=t.device)
    chunk = max(1, chunk_elems // max(n, 1))
    tx, ty, tz = t[:, 0][None], t[:, 1][None], t[:, 2][None]
    for a in range(0, m, chunk):
        qq = q[a:a + chunk]
        s = (qq[:, 0:1] - tx) ** 2
        s += (qq[:, 1:2] - ty) ** 2
        s += (qq[:, 2:3] - tz) ** 2
        best, arg = s.min(dim=1)
        # torch.min does not promise the first of equal minima: take the lowest index among them
        arg = torch.where(s == best[:, None], torch.arange(n, device=t.device)[None], n).min(dim=1).values
        idx[a:a + chunk], d1[a:a + chunk] = arg, best.sqrt()
        if n > 1:
            s.scatter_(1, arg[:, None], float('inf'))
            d2[a:a + chunk] = s.min(dim=1).values.sqrt()
    return idx, d1, d2


def metrics(dist_pred, dist_trgt, threshold):
    """The formulas of metricfunctions.py:84-98 on float64 distances -> dict of floats."""
    d1, d2 = np.asarray(dist_pred, dtype=np.float64), np.asarray(dist_trgt, dtype=np.float64)
    with np.errstate(all='ignore'):
        prec, recal = np.mean((d1 < threshold).astype('float')), np.mean((d2 < threshold).astype('float'))
        return dict(acc=float(np.mean(d1)), comp=float(np.mean(d2)), prec=float(prec), recal=float(recal),
                    fscore=float(2 * prec * recal / (prec + recal + 1e-8)))


def near_threshold(dist, threshold):
    """Number of float64 distances within 4u thr of the threshold: an fp32 distance may fall on the other side."""
    return int((np.abs(np.asarray(dist, dtype=np.float64) - threshold) <= DIST_BOUND * threshold).sum())


def clear_gap(d1, d2):
    """Where the second neighbour is farther than the nearest by more than 8u d2 (always, when there is no second one)."""
    d1, d2 = np.asarray(d1, dtype=np.float64), np.asarray(d2, dtype=np.float64)
    with np.errstate(invalid='ignore'):
        return np.isinf(d2) | ((d2 - d1) > GAP_BOUND * d2)


def check_nn(tag, target, query, idx, dist, ref, max_exempt=0.01):
    """Device result (idx, dist) against ``ref = nearest(target, query)``; all arguments NumPy / CPU tensors.  Prints every
    figure before asserting.  -> (largest relative distance error / u, exempt share)."""
    target, query = np.asarray(target, dtype=np.float64), np.asarray(query, dtype=np.float64)
    idx, dist = np.asarray(idx).astype(np.int64), np.asarray(dist).astype(np.float64)
    r_idx, d1, d2 = (np.asarray(x.cpu()) for x in ref)
    zero = d1 == 0
    rel = np.abs(dist - d1)[~zero] / d1[~zero]
    worst = float(rel.max()) / U if rel.size else 0.0
    clear = clear_gap(d1, d2)
    exempt = 1.0 - float(clear.mean())
    own = np.sqrt(((query - target[idx]) ** 2).sum(1))        # float64 distance to the row the device returned
    own_rel = np.abs(own - dist)[own > 0] / own[own > 0]
    print('%s: %d queries x %d targets, max |d - d64| / d64 = %.2f u (bound 4 u), %d zero distances, index-exempt share '
          '%.4g %% (cap %.2g %%), %d clear indices differ, returned row off its distance by at most %.2f u'
          % (tag, query.shape[0], target.shape[0], worst, int(zero.sum()), 100 * exempt, 100 * max_exempt,
             int((idx[clear] != r_idx[clear]).sum()), float(own_rel.max()) / U if own_rel.size else 0.0))
    assert idx.min() >= 0 and idx.max() < target.shape[0]
    assert np.all(dist[zero] == 0)
    assert worst <= 4.0
    assert exempt <= max_exempt
    assert np.array_equal(idx[clear], r_idx[clear])
    assert np.all(dist[own == 0] == 0) and (own_rel.size == 0 or float(own_rel.max()) <= DIST_BOUND)
    return worst, exempt


def check_metrics(tag, rec, d_pred64, d_trgt64, threshold):
    """Device record (5 floats) against the float64 distances of the checker."""
    rec = [float(x) for x in rec]
    want = metrics(d_pred64, d_trgt64, threshold)
    k1, k2 = near_threshold(d_pred64, threshold), near_threshold(d_trgt64, threshold)
    n1, n2 = len(d_pred64), len(d_trgt64)
    print('%s: device %s\n%s  checker %s; %d / %d distances within 4u of the threshold'
          % (tag, dict(zip(KEYS, rec)), ' ' * len(tag), want, k1, k2))
    assert abs(rec[0] - want['acc']) <= DIST_BOUND * want['acc']
    assert abs(rec[1] - want['comp']) <= DIST_BOUND * want['comp']
    assert abs(rec[2] - want['prec']) <= k1 / n1
    assert abs(rec[3] - want['recal']) <= k2 / n2
    assert abs(rec[4] - 2 * rec[2] * rec[3] / (rec[2] + rec[3] + 1e-8)) <= 1e-15
