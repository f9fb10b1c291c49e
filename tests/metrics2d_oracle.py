"""Float64 NumPy checker of the 2D depth metrics as include/v3d.h pins them (v3d_depth_metrics_2d), its seeded input makers and
the special pixels of the GPU tests.  Written from the rule, with NumPy only; it is the yardstick of tests/test_metrics2d_*.py
beside the reference-written fixtures tests/golden/M2d_*.npz.

The checker fixes no order of the float64 sums (NumPy's pairwise sum): the device's float64 columns are compared within H W
2^-53 relative, the bound for a float64 sum of non-negative terms in any order.  Counts and the fp32-typed columns
(perc_valid, d_125*) do not depend on the order and are compared bit for bit."""
import hashlib

import numpy as np

COLUMNS = ('perc_valid', 'abs_rel', 'abs_diff', 'abs_inv', 'sq_rel', 'rmse', 'd_125', 'd_125_2', 'd_125_3')
F32_COLUMNS = (0, 6, 7, 8)          # perc_valid, d_125, d_125_2, d_125_3: fp32 values, stored widened
F64_COLUMNS = (1, 2, 3, 4, 5)
F64_RTOL = 1e-10                    # H W 2^-53 = 3.4e-11 at 480 x 640


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def nearest_rule(in_size, out_size):
    """The index rule of a nearest resize: min(floor(dst * fl32(in / out)), in - 1), the product in fp32."""
    scale = np.float32(in_size) / np.float32(out_size)
    idx = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, in_size - 1)


def metres(gt):
    gt = np.asarray(gt)
    if gt.dtype == np.uint16:
        return gt.astype(np.float64) / 1000.0
    assert gt.dtype in (np.float32, np.float64), gt.dtype
    return gt.astype(np.float64)


def derived_valid(pred):
    return (pred != 0) & ~np.isinf(pred)            # a NaN prediction is "valid"


def check(pred, gt, pred_valid=None, derive_valid=False, rows=None, cols=None, drop=None):
    """pred [n, hp, wp] float32, gt [n, H, W] uint16 mm / float32 / float64 m -> dict(counts [n, 5] int32, per_image [n, 9],
    mean [9]).  rows / cols: the index tables (None: identity).  ``drop`` [n, H, W] bool: pixels taken out of the mask and of
    the count of valid predictions by hand (the tests of masked non-finite predictions)."""
    pred = np.asarray(pred)
    assert pred.dtype == np.float32
    g = metres(gt)
    n, H, W = g.shape
    if rows is not None:
        pred = pred[:, np.asarray(rows)][:, :, np.asarray(cols)]
    assert pred.shape == g.shape
    p = pred.astype(np.float64)
    if pred_valid is not None:
        pv = np.asarray(pred_valid) != 0
    elif derive_valid:
        pv = derived_valid(pred)
    else:
        pv = np.ones(g.shape, dtype=bool)
    if drop is not None:
        pv = pv & ~drop
    with np.errstate(all='ignore'):
        m = pv & (g >= 0.5) & (g < 65.0)
        e = np.abs(p - g)
        q = g + 1e-7
        t = np.abs((np.float32(1) / pred).astype(np.float64) - 1.0 / g)      # 1 / p is the one fp32 operation
        t = np.where(np.isfinite(t), t, 0.0)
        r1, r2 = p / g, g / p
        counts = np.zeros((n, 5), dtype=np.int32)
        per_image = np.zeros((n, 9))
        for i in range(n):
            k = m[i]
            c = [int(pv[i].sum()), int(k.sum())] + [int(((r1[i] < b) & (r2[i] < b) & k).sum()) for b in (1.25, 1.5625, 1.953125)]
            counts[i] = c
            denom32 = np.float32(c[1]) + np.float32(1e-7)
            denom = np.float64(denom32)
            ee = e[i][k] * e[i][k]
            sums = [np.sum((e[i][k] / q[i][k])), np.sum(e[i][k]), np.sum(t[i][k]), np.sum(ee / q[i][k]), np.sum(ee)]
            per_image[i] = [np.float32(c[0]) / np.float32(H * W), sums[0] / denom, sums[1] / denom, sums[2] / denom,
                            sums[3] / denom, np.sqrt(sums[4] / denom)] + [np.float32(v) / denom32 for v in c[2:]]
        mean = np.zeros(9)
        for i in range(n):                              # image order
            mean = mean + per_image[i]
        mean = mean / np.float64(n)
    return dict(counts=counts, per_image=per_image, mean=mean)


def weighted(means, ns, columns=range(9)):
    """The reference's average over batches: sum(n_j m_j) / sum(n_j) per column."""
    n_sum = float(np.sum(ns))
    return np.array([np.sum([ns[j] * means[j][k] for j in range(len(ns))]) / n_sum for k in columns])


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------
def gt_millimetres(n, H, W, seed):
    """Sensor depth as uint16 millimetres: a smooth-ish surface between 0.6 m and 6 m, 10 % holes (0), a few pixels below 0.5 m
    and a few at 65 m and beyond.  The last image is empty (all holes), the one before it holds exactly one pixel in range."""
    rng = np.random.default_rng(seed)
    mm = rng.integers(600, 6000, size=(n, H, W)).astype(np.uint16)
    u = rng.random((n, H, W))
    mm[u < 0.10] = 0
    mm[(u >= 0.10) & (u < 0.12)] = rng.integers(1, 500, size=int(((u >= 0.10) & (u < 0.12)).sum()))
    mm[(u >= 0.12) & (u < 0.13)] = rng.integers(65000, 65536, size=int(((u >= 0.12) & (u < 0.13)).sum()))
    if n >= 3:
        mm[n - 1] = 0
        mm[n - 2] = 0
        mm[n - 2, H // 2, W // 3] = 1234
    return mm


def predictions(gt_mm, hp, wp, seed):
    """float32 predictions [n, hp, wp]: the ground truth sampled at the coarse grid times 1 + 0.1 noise (holes filled with a
    depth of their own, so that a hole of the sensor is not a hole of the prediction), 5 % of them 0 (invalid)."""
    rng = np.random.default_rng(seed)
    n, H, W = gt_mm.shape
    rows = np.minimum((np.arange(hp) * H) // hp, H - 1)
    cols = np.minimum((np.arange(wp) * W) // wp, W - 1)
    g = gt_mm[:, rows][:, :, cols].astype(np.float64) / 1000.0
    g = np.where(g == 0, rng.uniform(0.6, 6.0, size=g.shape), g)
    p = (g * (1.0 + 0.1 * rng.standard_normal(g.shape))).astype(np.float32)
    p[rng.random(p.shape) < 0.05] = 0
    if n >= 3:                                         # the single pixel in range meets a valid prediction wherever it lands
        p[n - 2] = np.where(p[n - 2] == 0, np.float32(1.5), p[n - 2])
    return p


def scene(n, H, W, hp, wp, seed):
    gt = gt_millimetres(n, H, W, seed)
    return predictions(gt, hp, wp, seed + 1), gt


SPECIAL = dict(g_half=(2, 0, 0), g_65=(2, 0, 1), ratio_125=(2, 0, 2), p_zero=(2, 0, 3), p_negative=(2, 0, 4), spare_a=(2, 0, 5),
               spare_b=(2, 0, 6), single=(1, 7, 9))


def special_images():
    """(pred [3, 16, 16] float32, gt [3, 16, 16] uint16 mm): image 0 has an empty mask, image 1 exactly one pixel in range
    (SPECIAL['single']), image 2 is a random image whose first pixels are: g exactly 0.5 (in), g exactly 65.0 (out), p / g
    exactly 1.25 (not counted: the comparison is <), p = 0, a negative p, and two ordinary pixels the tests overwrite."""
    rng = np.random.default_rng(77)
    gt = rng.integers(600, 6000, size=(3, 16, 16)).astype(np.uint16)
    pred = (gt.astype(np.float64) / 1000.0 * (1.0 + 0.2 * rng.standard_normal(gt.shape))).astype(np.float32)
    gt[0] = 0
    gt[1] = 0
    gt[SPECIAL['single']] = 2500
    pred[SPECIAL['single']] = 2.25
    gt[SPECIAL['g_half']], pred[SPECIAL['g_half']] = 500, 0.55
    gt[SPECIAL['g_65']], pred[SPECIAL['g_65']] = 65000, 64.0
    gt[SPECIAL['ratio_125']], pred[SPECIAL['ratio_125']] = 2000, 2.5
    pred[SPECIAL['p_zero']] = 0.0
    pred[SPECIAL['p_negative']] = -1.75
    return pred, gt
