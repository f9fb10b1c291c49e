"""GPU: 2D depth metrics on the device (csrc/depthmetrics.hip; include/v3d.h: v3d_depth_metrics_2d; 3dvnet_amd/metrics2d.py)
against the reference-written fixtures tests/golden/M2d_*.npz and the float64 checker of tests/metrics2d_oracle.py: counts and
the fp32-typed columns bit for bit, the float64 columns within H W 2^-53 relative (1e-10), batch means of the fp32-typed keys
within n 2^-23 (the reference averages those in fp32)."""
import json
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics2d_oracle as oracle
from conftest import v3d
from test_metrics2d_oracle import FIXTURES, assert_means, assert_rows, batched_want, bits32, load

pytestmark = pytest.mark.gpu
GUARD = 256


def as_gt(gt_mm, kind):
    """uint16 millimetres -> the ground truth in one of the three types the kernel reads"""
    if kind == 'u16':
        return torch.from_numpy(np.ascontiguousarray(gt_mm))
    metres = gt_mm.astype(np.float64) / 1000.0
    return torch.from_numpy(metres.astype(np.float32) if kind == 'f32' else metres)


def run(cuda, pred, gt, pred_valid=None, derive_valid=False):
    """NumPy / tensors in -> the device record as NumPy arrays"""
    m2d = v3d('metrics2d')
    to = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(np.array(a))).to(cuda)    # noqa: E731  (a copy: fixtures are read-only)
    rec = m2d.depth_metrics(to(pred), to(gt), None if pred_valid is None else to(pred_valid), derive_valid)
    assert rec.counts.is_cuda and rec.per_image.is_cuda and rec.mean.is_cuda
    return dict(counts=rec.counts.cpu().numpy(), per_image=rec.per_image.cpu().numpy(), mean=rec.mean.cpu().numpy())


def assert_record(got, want, what):
    """a device record against the checker: counts and fp32-typed columns bit for bit, float64 columns within 1e-10; NaNs in
    the same places"""
    assert np.array_equal(got['counts'], want['counts']), what
    for c in oracle.F32_COLUMNS:
        assert np.array_equal(bits32(got['per_image'][:, c]), bits32(want['per_image'][:, c])), (what, oracle.COLUMNS[c])
    for c in oracle.F64_COLUMNS:
        np.testing.assert_allclose(got['per_image'][:, c], want['per_image'][:, c], rtol=oracle.F64_RTOL, atol=0,
                                   err_msg='%s %s' % (what, oracle.COLUMNS[c]))
    np.testing.assert_allclose(got['mean'], want['mean'], rtol=oracle.F64_RTOL, atol=0, err_msg=what)


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in ('counts', 'per_image', 'mean'))


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FIXTURES)
def test_fixtures(cuda, name):
    g = load(name)
    n = int(g['shape'][0])
    got = run(cuda, g['pred'], g['gt_mm'], derive_valid=True)
    assert np.array_equal(got['counts'][:, 0], g['n_pred_valid']) and np.array_equal(got['counts'][:, 1], g['n_mask'])
    assert_rows(got['per_image'], g['rows'], name)
    assert_means(got['mean'], g['batch'], n, name)
    assert_record(got, g['want'], name)
    nomask = run(cuda, g['pred'], g['gt_mm'])
    assert_means(nomask['mean'], np.concatenate([[1.0], g['batch_nomask']]), n, name + ' no mask')


def test_reference_named_functions_on_a_fixture(cuda):
    m2d = v3d('metrics2d')
    g = load('M2d_b')
    n = int(g['shape'][0])
    pred, gt = torch.from_numpy(g['pred']).to(cuda), as_gt(g['gt_mm'], 'f64').to(cuda)
    valid = (pred != 0) & ~torch.isinf(pred)
    out = m2d.calc_2d_depth_metrics(pred, gt, valid)
    assert list(out) == list(oracle.COLUMNS) and all(v.is_cuda and v.dim() == 0 for v in out.values())
    assert_means([float(v) for v in out.values()], g['batch'], n, 'calc_2d_depth_metrics')
    out = m2d.calc_2d_depth_metrics(pred, gt, convert_to_cpu=True)
    assert list(out) == list(oracle.COLUMNS[1:]) and all(isinstance(v, float) for v in out.values())
    assert_means([1.0] + list(out.values()), np.concatenate([[1.0], g['batch_nomask']]), n, 'calc_2d_depth_metrics, no mask')
    table, header = m2d.per_image_metrics(pred, gt, derive_valid=True, batch_size=2)
    assert header == oracle.COLUMNS and table.shape == (n, 9)
    assert_rows(table, g['rows'], 'per_image_metrics')


def test_batched_crosses_the_batch_of_100(cuda):
    """n = 101 views of 8 x 8: batches of 100 and 1, weights 100 and 1"""
    m2d = v3d('metrics2d')
    g = load('M2d_c')
    pred, gt = torch.from_numpy(g['pred']).to(cuda), as_gt(g['gt_mm'], 'f64').to(cuda)
    valid = (pred != 0) & ~torch.isinf(pred)
    out = m2d.calc_2d_depth_metrics_batched(pred, gt, pred_valid=valid, batch_size=100)
    assert list(out) == list(oracle.COLUMNS)
    assert_means(list(out.values()), g['batched'], 101, 'batched')
    assert_means(list(out.values()), batched_want(g), 101, 'batched against the checker')


@pytest.mark.parametrize('name', ['M2d_a', 'M2d_d'])
def test_chain_from_write_preds_to_the_scene_metrics(cuda, name, tmp_path):
    m2d, results = v3d('metrics2d'), v3d('results')
    g = load(name)
    n, H, W, hp, wp = (int(v) for v in g['shape'])
    batch = types.SimpleNamespace(images=torch.zeros(n, 3, H, W), K=torch.eye(3).repeat(n, 1, 1), rotmats=torch.eye(3).repeat(n, 1, 1),
                                  tvecs=torch.zeros(n, 3))
    path = str(tmp_path / 'preds.npz')
    results.write_preds(path, 'scene0000_00', g['pred'], batch, list(range(n)), np.arange(n))
    out_path = str(tmp_path / 'metrics_2d.json')
    out = m2d.process_scene_2d_metrics(path, g['gt_mm'], batch_size=int(g['batch_size']), out_path=out_path, device=cuda)
    assert list(out) == list(oracle.COLUMNS) + ['n'] and out['n'] == n
    assert_means([out[k] for k in oracle.COLUMNS], g['batched'], n, name + ' chain')
    assert json.load(open(out_path)) == out
    avg = results.average_metrics([out, out])
    assert avg['abs_rel'] == pytest.approx(out['abs_rel'], rel=1e-15)
    # a mapping with the ground truth as float64 metres already on the device gives the same numbers
    again = m2d.process_scene_2d_metrics(dict(depth_preds=g['pred']), as_gt(g['gt_mm'], 'f64').to(cuda), batch_size=int(g['batch_size']))
    assert again == out


# ---- addressing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(1, 1), (3, 5), (7, 9), (16, 64), (33, 130), (97, 131)])
@pytest.mark.parametrize('n', [1, 3])
def test_shapes_and_ground_truth_types(cuda, hw, n):
    """sizes below one vector, no multiple of a vector, rows ending inside a vector, one slice and (97 x 131 = 12707 pixels)
    two; the three ground-truth types; u16 and fp64(u16 / 1000) give the same bits"""
    H, W = hw
    pred, gt_mm = oracle.scene(n, H, W, H, W, 300 + H + n)
    recs = {}
    for kind in ('u16', 'f32', 'f64'):
        gt = as_gt(gt_mm, kind)
        recs[kind] = run(cuda, pred, gt, derive_valid=True)
        assert_record(recs[kind], oracle.check(pred, gt.numpy(), derive_valid=True), (hw, n, kind))
    assert same_bits(recs['u16'], recs['f64'])


@pytest.mark.parametrize('kind', ['u16', 'f32', 'f64'])
def test_unaligned_base(cuda, kind):
    """gt_all[1:] of 7 x 9 images: 63 elements in, the base is aligned to its element only (2 bytes for u16); the same views
    from a fresh allocation give the same bits"""
    pred, gt_mm = oracle.scene(4, 7, 9, 7, 9, 41)
    gt_all = as_gt(gt_mm, kind).to(cuda)
    valid_all = torch.from_numpy(oracle.derived_valid(pred)).to(cuda)
    m2d = v3d('metrics2d')
    view = gt_all[1:]
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    rec = m2d.depth_metrics(torch.from_numpy(pred[1:]).to(cuda), view, valid_all[1:])
    got = dict(counts=rec.counts.cpu().numpy(), per_image=rec.per_image.cpu().numpy(), mean=rec.mean.cpu().numpy())
    assert_record(got, oracle.check(pred[1:], as_gt(gt_mm[1:], kind).numpy(), derive_valid=True), kind)
    assert same_bits(got, run(cuda, pred[1:], as_gt(gt_mm[1:], kind), pred_valid=oracle.derived_valid(pred[1:])))


@pytest.mark.parametrize('sizes', [((6, 8), (11, 15)), ((10, 7), (7, 10)), ((5, 5), (5, 5)), ((256, 320), (480, 640))])
def test_resize_equals_the_enlarged_prediction_through_the_identity_path(cuda, sizes):
    (hp, wp), (H, W) = sizes
    if (H, W) == (480, 640):
        g = load('M2d_d')
        pred, gt_mm = g['pred'][:2], g['gt_mm'][:2]                      # two views
    else:
        pred, gt_mm = oracle.scene(3, H, W, hp, wp, 500 + H)
    got = run(cuda, pred, gt_mm, derive_valid=True)
    big = F.interpolate(torch.from_numpy(pred).unsqueeze(1), (H, W), mode='nearest').squeeze(1)
    assert same_bits(got, run(cuda, big, gt_mm, derive_valid=True))
    if (H, W) != (480, 640):
        assert_record(got, oracle.check(big.numpy(), gt_mm, derive_valid=True), sizes)


# ---- special pixels -----------------------------------------------------------------------------------------------------------
def test_special_pixels(cuda):
    pred, gt = oracle.special_images()
    want = oracle.check(pred, gt, derive_valid=True)
    got = run(cuda, pred, gt, derive_valid=True)
    assert_record(got, want, 'special')
    assert got['counts'][0, 1] == 0 and np.all(got['per_image'][0, 1:] == 0.0)            # empty mask: 0, not NaN
    assert got['counts'][1, 1] == 1 and got['per_image'][1, 2] == 0.25 / (1.0 + 2.0 ** -23)
    # one pixel at a time in an otherwise empty image 1: what each special pixel counts
    def single(g_mm, p, derive=True):
        gt1, pred1 = gt.copy(), pred.copy()
        gt1[oracle.SPECIAL['single']], pred1[oracle.SPECIAL['single']] = g_mm, p
        r = run(cuda, pred1, gt1, derive_valid=derive)
        assert_record(r, oracle.check(pred1, gt1, derive_valid=derive), (g_mm, p, derive))
        return r['counts'][1]
    assert list(single(500, 0.5)) == [256, 1, 1, 1, 1]                   # g exactly 0.5: in
    assert list(single(65000, 65.0)) == [256, 0, 0, 0, 0]                # g exactly 65.0: out
    assert list(single(2000, 2.5)) == [256, 1, 0, 1, 1]                  # p / g exactly 1.25: not below it
    assert list(single(2000, 0.0)) == [255, 0, 0, 0, 0]                  # p = 0 with the derived mask: not valid
    assert list(single(2000, 0.0, derive=False)) == [256, 1, 0, 0, 0]    # ... without a mask: in, g / p = inf, 1 / p - 1 / g = inf -> 0
    assert list(single(2000, -1.75)) == [256, 1, 1, 1, 1]                # a negative p: both ratios negative, below every bound


def test_masked_non_finite_predictions_contribute_nothing(cuda):
    """the stated deviation: the reference's 0 * inf is NaN; here the result is the checker's with those pixels dropped"""
    pred, gt = oracle.special_images()
    a, b = oracle.SPECIAL['spare_a'], oracle.SPECIAL['spare_b']
    pred[a], pred[b] = np.inf, np.nan
    valid = oracle.derived_valid(pred)
    valid[b] = False                                                     # mode 1: the caller masks the NaN; mode 2 masks the inf itself
    drop = np.zeros(gt.shape, dtype=bool)
    drop[a] = drop[b] = True
    got = run(cuda, pred, gt, pred_valid=valid)
    assert np.all(np.isfinite(got['per_image'])) and np.all(np.isfinite(got['mean']))
    assert_record(got, oracle.check(pred, gt, derive_valid=True, drop=drop), 'masked inf and NaN')


def test_unmasked_nan_prediction_propagates(cuda):
    pred, gt = oracle.special_images()
    pred[oracle.SPECIAL['spare_a']] = np.nan
    got = run(cuda, pred, gt, derive_valid=True)                          # a NaN prediction is "valid"
    want = oracle.check(pred, gt, derive_valid=True)
    assert np.array_equal(got['counts'], want['counts'])
    assert np.all(np.isnan(got['per_image'][2, [1, 2, 4, 5]])) and np.isfinite(got['per_image'][2, 3])    # 1 / p - 1 / g = NaN -> 0
    assert np.array_equal(np.isnan(got['per_image']), np.isnan(want['per_image']))
    assert np.array_equal(np.isnan(got['mean']), np.isnan(want['mean']))
    for c in oracle.F32_COLUMNS:
        assert np.array_equal(bits32(got['per_image'][:, c]), bits32(want['per_image'][:, c]))
    np.testing.assert_allclose(got['per_image'][:2], want['per_image'][:2], rtol=oracle.F64_RTOL, atol=0)


def test_validity_modes_agree(cuda):
    pred, gt_mm = oracle.scene(3, 33, 130, 33, 130, 61)
    derived = run(cuda, pred, gt_mm, derive_valid=True)
    valid = oracle.derived_valid(pred)
    assert same_bits(derived, run(cuda, pred, gt_mm, pred_valid=valid))
    assert same_bits(derived, run(cuda, pred, gt_mm, pred_valid=valid.astype(np.uint8) * 3))        # non-zero = valid
    none = run(cuda, pred, gt_mm)
    assert np.all(none['counts'][:, 0] == 33 * 130) and np.all(none['counts'][:, 1] >= derived['counts'][:, 1])
    assert_record(none, oracle.check(pred, gt_mm), 'mode 0')


def test_ten_launches_are_bit_identical(cuda):
    pred, gt_mm = oracle.scene(3, 33, 130, 33, 130, 62)
    first = run(cuda, pred, gt_mm, derive_valid=True)
    for _ in range(9):
        assert same_bits(first, run(cuda, pred, gt_mm, derive_valid=True))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_guard_bands_and_host_side_errors(cuda):
    lib_mod = v3d('_lib')
    lib = lib_mod.load()
    n, H, W = 3, 7, 9
    pred_np, gt_mm = oracle.scene(n, H, W, H, W, 63)
    pred, gt = torch.from_numpy(pred_np).to(cuda), torch.from_numpy(gt_mm).to(cuda)
    rows, cols = torch.arange(H, dtype=torch.int32, device=cuda), torch.arange(W, dtype=torch.int32, device=cuda)
    valid = torch.ones((n, H, W), dtype=torch.uint8, device=cuda)
    counts = torch.full((n * 5 + 2 * GUARD,), -777, dtype=torch.int32, device=cuda)
    per_image = torch.full((n * 9 + 2 * GUARD,), -777.0, dtype=torch.float64, device=cuda)
    mean = torch.full((9 + 2 * GUARD,), -777.0, dtype=torch.float64, device=cuda)
    ws_bytes = int(lib.v3d_depth_metrics_workspace_bytes(n, H, W))
    assert ws_bytes > 0 and lib.v3d_depth_metrics_workspace_bytes(0, H, W) == 0
    assert lib.v3d_depth_metrics_workspace_bytes(1, 4096, 4096) == 0
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=cuda)
    stream = lib_mod.stream_ptr(cuda)

    def call(pred_p=pred.data_ptr(), hp=H, wp=W, rows_p=None, cols_p=None, gt_p=gt.data_ptr(), gt_type=0, valid_p=None, mode=2,
             n_=n, H_=H, W_=W, counts_p=counts.data_ptr() + 4 * GUARD, ws_p=ws.data_ptr(), ws_n=ws_bytes):
        return lib.v3d_depth_metrics_2d(pred_p, hp, wp, rows_p, cols_p, gt_p, gt_type, valid_p, mode, n_, H_, W_, counts_p,
                                        per_image.data_ptr() + 8 * GUARD, mean.data_ptr() + 8 * GUARD, ws_p, ws_n, stream)

    BAD_SHAPE, BAD_ARG, TOO_SMALL = -1, -2, -3
    assert call(pred_p=None) == BAD_ARG and call(gt_p=None) == BAD_ARG and call(counts_p=None) == BAD_ARG and call(ws_p=None) == BAD_ARG
    assert call(rows_p=rows.data_ptr()) == BAD_ARG and call(cols_p=cols.data_ptr()) == BAD_ARG          # one table without the other
    assert call(hp=H - 1) == BAD_SHAPE and call(wp=W + 1) == BAD_SHAPE                                  # identity, other size
    assert call(n_=0) == BAD_SHAPE and call(H_=0) == BAD_SHAPE and call(W_=-1) == BAD_SHAPE and call(hp=0) == BAD_SHAPE
    assert call(H_=4096, W_=4096, hp=4096, wp=4096) == BAD_SHAPE                                        # H W = 2^24
    assert call(gt_type=3) == BAD_ARG and call(gt_type=-1) == BAD_ARG and call(mode=3) == BAD_ARG
    assert call(mode=1) == BAD_ARG                                                                      # mode 1 without a mask
    assert call(gt_p=gt.data_ptr() + 1) == BAD_ARG                                                      # not aligned to its element
    assert call(ws_n=ws_bytes - 1) == TOO_SMALL
    assert lib.v3d_last_error()
    torch.cuda.synchronize()
    # nothing was enqueued: outputs and workspace are as they were
    assert bool((counts == -777).all()) and bool((per_image == -777.0).all()) and bool((mean == -777.0).all()) and bool((ws == 0).all())
    # the call itself, through explicit identity tables and a mask of ones: writes inside the bands only
    lib_mod.check(call(rows_p=rows.data_ptr(), cols_p=cols.data_ptr(), valid_p=valid.data_ptr(), mode=1), 'v3d_depth_metrics_2d')
    torch.cuda.synchronize()
    for buf, k in ((counts, n * 5), (per_image, n * 9), (mean, 9)):
        out = buf.cpu().numpy()
        assert np.all(out[:GUARD] == -777) and np.all(out[GUARD + k:] == -777) and np.all(out[GUARD:GUARD + k] != -777)
    got = dict(counts=counts.cpu().numpy()[GUARD:GUARD + n * 5].reshape(n, 5), per_image=per_image.cpu().numpy()[GUARD:GUARD + n * 9].reshape(n, 9),
               mean=mean.cpu().numpy()[GUARD:GUARD + 9])
    assert_record(got, oracle.check(pred_np, gt_mm), 'C ABI')


# ---- against the stock-torch route ----------------------------------------------------------------------------------------------
def test_agrees_with_the_stock_torch_route_on_the_device(cuda):
    """results.depth_metrics_2d on the enlarged predictions and the float64 ground truth, as the reference's scene function
    hands them over"""
    results = v3d('results')
    g = load('M2d_a')
    n, H, W = (int(v) for v in g['shape'][:3])
    pred, gt = torch.from_numpy(g['pred']).to(cuda), as_gt(g['gt_mm'], 'f64').to(cuda)
    big = F.interpolate(pred.unsqueeze(1), (H, W), mode='nearest').squeeze(1)
    valid = (big != 0) & ~torch.isinf(big)
    stock = results.depth_metrics_2d(big, gt, valid)
    got = run(cuda, g['pred'], gt, derive_valid=True)
    assert_means(got['mean'], [float(stock[k]) for k in oracle.COLUMNS], n, 'stock route')
