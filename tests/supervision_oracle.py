"""Float64 NumPy checker of the depth supervision as include/v3d.h pins it (v3d_depth_supervision_f32): the eight 2D depth metrics
without a mask and the masked MAE loss of predictions [n, h, w] against fp32 ground truth [n, H, W] that is read through the tables
of a nearest resize.  Written from the rule, with NumPy only; with the seeded input makers it is the yardstick of
tests/test_supervision_*.py and tests/test_forward_gpu.py beside the reference-written fixtures tests/golden/S_sup_*.npz.

Columns 0-8 and counts 0-4 are the rule of the 2D depth metrics with every prediction valid: tests/metrics2d_oracle.py computes
them here as well.  Column 9 is the loss, count 5 its mask's size:

    S_i = sum |p - g| over the pixels of image i with g != 0 (compared in fp32), in float64;   n_i their number;
    term_i = (S_i / float64(float32(depth_interval))) / float64(float32(n_i) + float32(1e-7));   loss = (sum_i term_i) / n.

The interval is an fp32 number (the C entry takes a float; the reference divides its float32 sums by it in fp32).  The loss's mask
(g != 0) is not the metrics' (0.5 <= g < 65): pixels with 0 < g < 0.5 or g >= 65 count in the loss only.

Like metrics2d_oracle.py the checker fixes no order of the float64 sums: the device's float64 columns and the loss are compared
within F64_RTOL, counts and the fp32-typed columns bit for bit."""
import numpy as np

import metrics2d_oracle as m2d

COLUMNS = m2d.COLUMNS + ('loss_2d',)
METRIC_KEYS = m2d.COLUMNS[1:]            # the keys of the reference's calc_2d_depth_metrics without a mask, in its order
F32_COLUMNS = m2d.F32_COLUMNS
F64_COLUMNS = m2d.F64_COLUMNS + (9,)     # the loss is a float64 column
F64_RTOL = m2d.F64_RTOL
LOSS = 9
digest = m2d.digest
nearest_rule = m2d.nearest_rule


def tables(H, W, h, w):
    """(rows [h], cols [w]): the ground-truth row / column a nearest resize H x W -> h x w reads; (None, None) for equal sizes"""
    return (None, None) if (H, W) == (h, w) else (nearest_rule(H, h), nearest_rule(W, w))


def reduce_gt(gt, h, w):
    """gt [n, H, W] -> [n, h, w] through the tables"""
    rows, cols = tables(gt.shape[1], gt.shape[2], h, w)
    return gt if rows is None else gt[:, rows][:, :, cols]


def check(pred, gt, depth_interval):
    """pred [n, h, w] float32, gt [n, H, W] float32 -> dict(counts [n, 6] int32, per_image [n, 10], mean [10])"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    assert pred.dtype == np.float32 and gt.dtype == np.float32
    n, h, w = pred.shape
    g32 = reduce_gt(gt, h, w)
    base = m2d.check(pred, g32)
    counts = np.zeros((n, 6), dtype=np.int32)
    per_image = np.zeros((n, 10))
    counts[:, :5], per_image[:, :9] = base['counts'], base['per_image']
    interval = np.float64(np.float32(depth_interval))
    with np.errstate(all='ignore'):
        for i in range(n):
            k = g32[i] != np.float32(0)
            counts[i, 5] = int(k.sum())
            s = np.sum(np.abs(pred[i][k].astype(np.float64) - g32[i][k].astype(np.float64)))
            per_image[i, 9] = (s / interval) / np.float64(np.float32(counts[i, 5]) + np.float32(1e-7))
        mean = np.zeros(10)
        for i in range(n):                              # image order
            mean = mean + per_image[i]
        mean = mean / np.float64(n)
    return dict(counts=counts, per_image=per_image, mean=mean)


def total_loss(losses, n_sweeps, lam):
    """PL3DVNet.forward's 'loss' from the ten (1 + n_sweeps + 3) supervised points' losses, in float64 and in its order"""
    total = np.float64(0.0) + np.float64(losses[0])
    for k in range(n_sweeps):
        total = total + np.float64(lam) * np.float64(losses[1 + k])
    for v in losses[1 + n_sweeps:]:
        total = total + np.float64(v)
    return total


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------
def scene(n, H, W, h, w, seed):
    """(pred [n, h, w] float32, gt [n, H, W] float32 metres): the seeded scene of the 2D-metric tests with the ground truth as
    the fp32 tensor a training batch carries.  10 % holes (0), 2 % of the pixels below 0.5 m and 1 % at 65 m and beyond; with
    n >= 3 the last image has no ground truth at all and the one before it exactly one pixel, which is in range and which the
    nearest resize to h x w reads.  The first image's last two pixels that the resize reads are 0.25 m and 65.5 m, so that
    the smallest scene has both kinds too."""
    pred, gt_mm = m2d.scene(n, H, W, h, w, seed)
    rows, cols = nearest_rule(H, h), nearest_rule(W, w)
    gt_mm[0, rows[h - 1], cols[w - 1]] = 250
    gt_mm[0, rows[h - 1], cols[w - 2]] = 65500
    if n >= 3:
        gt_mm[n - 2] = 0
        gt_mm[n - 2, rows[h // 2], cols[w // 3]] = 1234
    return pred, (gt_mm.astype(np.float64) / 1000.0).astype(np.float32)


def fixture_inputs(g):
    """The inputs of a fixture: stored, or seeded; checked against the stored digests either way."""
    n, H, W, h, w = (int(v) for v in g['shape'])
    pred, gt = (g['pred'], g['gt']) if 'pred' in g else scene(n, H, W, h, w, int(g['seed']))
    assert digest(pred) == str(g['pred_sha']) and digest(gt) == str(g['gt_sha'])
    return pred, gt
