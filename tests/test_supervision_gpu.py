"""GPU: depth supervision on the device (csrc/supervision.hip; include/v3d.h: v3d_depth_supervision_f32; 3dvnet_amd/loss.py) against
the float64 checker of tests/supervision_oracle.py and the reference-written fixtures tests/golden/S_sup_*.npz: counts and the
fp32-typed columns bit for bit, the float64 columns and the loss within h w 2^-53 relative (F64_RTOL = 1e-10), the fixtures by the
two rules of tests/test_supervision_oracle.py.

Cases (n, h x w <- H x W):
  S_sup_a   4,   6 x 8 <- 12 x 16        resize, tiny
  S_sup_b   3,   7 x 5 identity          w < 8, odd sizes, partial groups; its [1:] has bases that are not 16-byte aligned
  S_sup_c   4,   96 x 100 <- 192 x 200   9600 pixels are two slices, a row ends inside a group; its first two images alone as well
  S_sup_d   257, 4 x 4 identity          more images than threads of the finalising workgroup"""
import numpy as np
import pytest
import torch

import supervision_oracle as oracle
from conftest import v3d
from test_metrics2d_oracle import bits32
from test_supervision_oracle import FIXTURES, assert_against_fixture, load

pytestmark = pytest.mark.gpu
GUARD = 256


def record(rec):
    assert rec.counts.is_cuda and rec.per_image.is_cuda and rec.mean.is_cuda
    assert rec.counts.dtype == torch.int32 and rec.per_image.dtype == torch.float64 and rec.mean.dtype == torch.float64
    return dict(counts=rec.counts.cpu().numpy(), per_image=rec.per_image.cpu().numpy(), mean=rec.mean.cpu().numpy())


def run(cuda, pred, gt, interval):
    """NumPy in -> the device record as NumPy arrays (copies: fixtures are read-only)"""
    to = lambda a: torch.from_numpy(np.array(a)).to(cuda)    # noqa: E731
    return record(v3d('loss').supervise(to(pred), to(gt), interval))


def assert_record(got, want, what):
    """a device record against the checker"""
    assert got['counts'].shape == want['counts'].shape and got['per_image'].shape == want['per_image'].shape
    assert np.array_equal(got['counts'], want['counts']), what
    for c in oracle.F32_COLUMNS:
        assert np.array_equal(bits32(got['per_image'][:, c]), bits32(want['per_image'][:, c])), (what, oracle.COLUMNS[c])
    for c in oracle.F64_COLUMNS:
        np.testing.assert_allclose(got['per_image'][:, c], want['per_image'][:, c], rtol=oracle.F64_RTOL, atol=0,
                                   err_msg='%s %s' % (what, oracle.COLUMNS[c]))
    np.testing.assert_allclose(got['mean'], want['mean'], rtol=oracle.F64_RTOL, atol=0, err_msg=what)


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ('counts', 'per_image', 'mean'))


@pytest.mark.parametrize('name', FIXTURES)
def test_fixtures(cuda, name):
    g = load(name)
    got = run(cuda, g['pred'], g['gt'], g['interval'])
    assert_record(got, g['want'], name)
    assert np.array_equal(got['counts'][:, 1], g['n_mask']) and np.array_equal(got['counts'][:, 5], g['n_loss'])
    assert_against_fixture(got, g, name)
    for _ in range(2):                                                   # three launches, identical bits
        assert same_bits(got, run(cuda, g['pred'], g['gt'], g['interval']))


def test_two_images_of_two_slices(cuda):
    """2, 96 x 100 <- 192 x 200: the first two images of S_sup_c"""
    g = load('S_sup_c')
    pred, gt = g['pred'][:2], g['gt'][:2]
    got = run(cuda, pred, gt, g['interval'])
    assert_record(got, oracle.check(pred, gt, g['interval']), 'two of S_sup_c')
    assert_against_fixture(got, g, 'two of S_sup_c', images=slice(0, 2), batch=False)
    assert same_bits(got, run(cuda, pred, gt, g['interval']))


def test_unaligned_bases(cuda):
    """pred[1:] and gt[1:] of the 7 x 5 case: 35 floats in, 4-byte aligned only; the same images from fresh allocations give the
    same bits"""
    loss = v3d('loss')
    g = load('S_sup_b')
    pred_all, gt_all = torch.from_numpy(np.array(g['pred'])).to(cuda), torch.from_numpy(np.array(g['gt'])).to(cuda)
    pred, gt = pred_all[1:], gt_all[1:]
    assert pred.is_contiguous() and pred.data_ptr() % 16 != 0 and gt.data_ptr() % 16 != 0
    got = record(loss.supervise(pred, gt, g['interval']))
    assert_record(got, oracle.check(g['pred'][1:], g['gt'][1:], g['interval']), 'unaligned')
    assert_against_fixture(got, g, 'unaligned', images=slice(1, 3), batch=False)
    assert same_bits(got, run(cuda, g['pred'][1:], g['gt'][1:], g['interval']))


@pytest.mark.parametrize('H,W,unaligned', [(97, 131, False), (7, 5, False), (97, 131, True)],
                         ids=['97x131', '7x5', '97x131-unaligned'])
def test_metrics_columns_equal_the_2d_metrics_bit_for_bit(cuda, H, W, unaligned):
    """Equal sizes, fp32 ground truth, no validity: v3d_depth_metrics_2d walks the ground truth and v3d_depth_supervision_f32 the
    prediction, pixel for pixel the same lanes in the same order with the same rule (csrc/depth2d.h), so columns 0-8 and counts
    0-4 are the same bits.  3 images of 97 x 131 = 12 707 pixels: two slices, a partial last group, rows ending inside groups;
    7 x 5: W < 8; [1:] of a 4-image allocation: neither base is 16-byte aligned (12 707 floats in)."""
    loss, m2d = v3d('loss'), v3d('metrics2d')
    pred, gt = (torch.from_numpy(a).to(cuda) for a in oracle.scene(3, H, W, H, W, seed=H))
    if unaligned:
        pred, gt = (torch.cat((t[:1], t))[1:] for t in (pred, gt))
        assert pred.is_contiguous() and gt.is_contiguous() and pred.data_ptr() % 16 != 0 and gt.data_ptr() % 16 != 0
    sup, met = record(loss.supervise(pred, gt, 0.05)), record(m2d.depth_metrics(pred, gt))
    assert met['counts'].shape == (3, 5) and met['per_image'].shape == (3, 9) and sup['counts'][0, 1] > 0
    assert np.array_equal(sup['counts'][:, :5], met['counts'])
    assert np.array_equal(sup['per_image'][:, :9].view(np.uint64), met['per_image'].view(np.uint64))
    assert np.array_equal(sup['mean'][:9].view(np.uint64), met['mean'].view(np.uint64))


def test_resize_equals_the_reduced_ground_truth_through_the_identity_path(cuda):
    for name in ('S_sup_a', 'S_sup_c'):
        g = load(name)
        h, w = g['pred'].shape[1:]
        got = run(cuda, g['pred'], g['gt'], g['interval'])
        assert same_bits(got, run(cuda, g['pred'], np.ascontiguousarray(oracle.reduce_gt(g['gt'], h, w)), g['interval']))


def test_mae_loss_module_and_the_loss_only_pixels(cuda):
    loss = v3d('loss')
    g = load('S_sup_a')
    pred, gt = torch.from_numpy(np.array(g['pred'])).to(cuda), torch.from_numpy(np.array(g['gt'])).to(cuda)
    rec = loss.supervise(pred, gt, g['interval'])
    out = loss.MAELoss()(pred, gt, g['interval'])
    assert out.is_cuda and out.dim() == 0 and out.dtype == torch.float64 and torch.equal(out, rec.mean[9])
    d = loss.metrics_dict(rec)
    assert tuple(d) == oracle.METRIC_KEYS and all(torch.equal(d[k], rec.mean[oracle.COLUMNS.index(k)]) for k in d)
    # a pixel below 0.5 m moves the loss and leaves the metrics alone; a hole moves neither
    h, w = pred.shape[1:]
    rows, cols = oracle.tables(gt.shape[1], gt.shape[2], h, w)
    gt2 = gt.clone()
    gt2[0, int(rows[0]), int(cols[0])] = 0.25
    pred2 = pred.clone()
    pred2[0, 0, 0] += 1.0
    a, b = record(loss.supervise(pred, gt2, g['interval'])), record(loss.supervise(pred2, gt2, g['interval']))
    assert np.array_equal(a['per_image'][:, :9], b['per_image'][:, :9]) and b['per_image'][0, 9] != a['per_image'][0, 9]
    assert_record(b, oracle.check(pred2.cpu().numpy(), gt2.cpu().numpy(), g['interval']), 'below 0.5 m')
    gt2[0, int(rows[0]), int(cols[0])] = 0.0
    a, b = record(loss.supervise(pred, gt2, g['interval'])), record(loss.supervise(pred2, gt2, g['interval']))
    assert same_bits(a, b)


def test_non_finite_error_makes_the_loss_non_finite(cuda):
    g = load('S_sup_b')
    pred = np.array(g['pred'])
    k = np.argwhere(g['gt'][0] != 0)[0]
    pred[0, k[0], k[1]] = np.inf
    got = run(cuda, pred, g['gt'], g['interval'])
    assert np.isinf(got['per_image'][0, 9]) and np.isinf(got['mean'][9]) and np.all(np.isfinite(got['per_image'][1:, 9]))


def test_guard_bands_and_host_side_errors(cuda):
    lib_mod = v3d('_lib')
    lib = lib_mod.load()
    g = load('S_sup_a')
    n, H, W, h, w = (int(v) for v in g['shape'])
    pred, gt = torch.from_numpy(np.array(g['pred'])).to(cuda), torch.from_numpy(np.array(g['gt'])).to(cuda)
    rows, cols = (torch.from_numpy(t.astype(np.int32)).to(cuda) for t in oracle.tables(H, W, h, w))
    counts = torch.full((n * 6 + 2 * GUARD,), -777, dtype=torch.int32, device=cuda)
    per_image = torch.full((n * 10 + 2 * GUARD,), -777.0, dtype=torch.float64, device=cuda)
    mean = torch.full((10 + 2 * GUARD,), -777.0, dtype=torch.float64, device=cuda)
    ws_bytes = int(lib.v3d_depth_supervision_workspace_bytes(n, h, w))
    assert ws_bytes > 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=cuda)
    stream = lib_mod.stream_ptr(cuda)

    def call(pred_p=pred.data_ptr(), n_=n, h_=h, w_=w, gt_p=gt.data_ptr(), H_=H, W_=W, rows_p=rows.data_ptr(), cols_p=cols.data_ptr(),
             counts_p=counts.data_ptr() + 4 * GUARD, ws_p=ws.data_ptr(), ws_n=ws_bytes):
        return lib.v3d_depth_supervision_f32(pred_p, n_, h_, w_, gt_p, H_, W_, rows_p, cols_p, g['interval'], counts_p,
                                             per_image.data_ptr() + 8 * GUARD, mean.data_ptr() + 8 * GUARD, ws_p, ws_n, stream)

    BAD_SHAPE, BAD_ARG, TOO_SMALL = -1, -2, -3
    assert call(pred_p=None) == BAD_ARG and call(gt_p=None) == BAD_ARG and call(counts_p=None) == BAD_ARG and call(ws_p=None) == BAD_ARG
    assert call(rows_p=None) == BAD_ARG and call(cols_p=None) == BAD_ARG                          # tables given singly
    assert call(rows_p=None, cols_p=None) == BAD_SHAPE                                            # identity with unequal sizes
    assert call(n_=0) == BAD_SHAPE and call(h_=0) == BAD_SHAPE and call(w_=-1) == BAD_SHAPE and call(H_=0) == BAD_SHAPE
    assert call(W_=0) == BAD_SHAPE
    assert call(h_=4096, w_=4096) == BAD_SHAPE                                                    # h w = 2^24
    assert call(pred_p=pred.data_ptr() + 2) == BAD_ARG                                            # not aligned to its element
    assert call(ws_n=ws_bytes - 1) == TOO_SMALL
    assert lib.v3d_last_error()
    torch.cuda.synchronize()
    # nothing was enqueued: outputs and workspace are as they were
    assert bool((counts == -777).all()) and bool((per_image == -777.0).all()) and bool((mean == -777.0).all()) and bool((ws == 0).all())
    # the call itself: writes inside the bands only
    lib_mod.check(call(), 'v3d_depth_supervision_f32')
    torch.cuda.synchronize()
    for buf, k in ((counts, n * 6), (per_image, n * 10), (mean, 10)):
        out = buf.cpu().numpy()
        assert np.all(out[:GUARD] == -777) and np.all(out[GUARD + k:] == -777) and np.all(out[GUARD:GUARD + k] != -777)
    got = dict(counts=counts.cpu().numpy()[GUARD:GUARD + n * 6].reshape(n, 6),
               per_image=per_image.cpu().numpy()[GUARD:GUARD + n * 10].reshape(n, 10), mean=mean.cpu().numpy()[GUARD:GUARD + 10])
    assert_record(got, g['want'], 'C ABI')
    # table entries outside the ground truth are clamped: no read leaves the image
    wild_r, wild_c = rows.clone(), cols.clone()
    wild_r[0], wild_r[-1], wild_c[0], wild_c[-1] = -5, H + 100, -1, 1 << 30
    lib_mod.check(call(rows_p=wild_r.data_ptr(), cols_p=wild_c.data_ptr()), 'v3d_depth_supervision_f32')
    torch.cuda.synchronize()
    rr, cc = oracle.tables(H, W, h, w)
    rr, cc = rr.copy(), cc.copy()
    rr[0], rr[-1], cc[0], cc[-1] = 0, H - 1, 0, W - 1
    clamped = np.ascontiguousarray(g['gt'][:, rr][:, :, cc])
    got = dict(counts=counts.cpu().numpy()[GUARD:GUARD + n * 6].reshape(n, 6),
               per_image=per_image.cpu().numpy()[GUARD:GUARD + n * 10].reshape(n, 10), mean=mean.cpu().numpy()[GUARD:GUARD + 10])
    assert_record(got, oracle.check(g['pred'], clamped, g['interval']), 'clamped tables')


def test_argument_errors_of_the_python_entry(cuda):
    loss, lib_mod = v3d('loss'), v3d('_lib')
    g = load('S_sup_b')
    pred, gt = torch.from_numpy(np.array(g['pred'])).to(cuda), torch.from_numpy(np.array(g['gt'])).to(cuda)
    with pytest.raises(lib_mod.V3DLibraryError):
        loss.supervise(pred.cpu(), gt, 0.05)
    with pytest.raises(lib_mod.V3DLibraryError):
        loss.supervise(pred, gt.cpu(), 0.05)
    with pytest.raises(ValueError):
        loss.supervise(pred, gt[:2], 0.05)
    with pytest.raises(ValueError):
        loss.supervise(pred, gt.double(), 0.05)
