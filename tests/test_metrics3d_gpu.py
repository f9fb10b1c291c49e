"""GPU: the 3D cloud metrics (3dvnet_amd/metrics3d.py -> v3d_cloud_downsample_f32 / v3d_nn_query_f32 / v3d_cloud_metrics_f64,
csrc/cloudmetrics.hip) against the reference's recorded outputs (tests/golden/M_metrics3d_*.npz), against the float64 checker
(tests/cloud_oracle.py) at small and at full size, and their own invariants.  Every test runs the HIP path through the C ABI.

Bounds (u = 2^-24; derivations in tests/cloud_oracle.py):
  distances   |d - d64| <= 4u d64, and d64 = 0 requires d = 0;
  indices     equal wherever the second-neighbour gap exceeds 8u d2; elsewhere the returned row must lie at the returned
              distance (within 4u); at most 1 % of the queries may be exempt -- a condition of the test, not a measurement.
              Clouds with exact duplicate rows are searched over their distinct rows (duplicates have equal fp32 distances
              and the lowest row is the specified answer);
  down-sample the same cells in the same order, points and attributes within 1 fp32 ulp of the checker (equality expected);
  metrics     acc / comp within 4u relative, |prec - prec64| <= k / n with k = checker distances within 4u thr of the
              threshold (same for recal), fscore = the formula on the device's own prec / recal to 1e-15.
"""
import math

import numpy as np
import pytest
import torch

import cloud_oracle as co
import fusion_oracle as fo
from conftest import v3d
from test_metrics3d_oracle import CASES, load_case

pytestmark = pytest.mark.gpu


def nn(cuda, target, query):
    m3 = v3d('metrics3d')
    idx, dist = m3.nearest_neighbors(torch.as_tensor(target).to(cuda), torch.as_tensor(query).to(cuda))
    torch.cuda.synchronize()
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32
    return idx.cpu().numpy(), dist.cpu().numpy()


def ulps(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))


@pytest.mark.parametrize('case', CASES)
def test_goldens(cuda, case):
    m3 = v3d('metrics3d')
    g = load_case(case)
    thr = float(g['threshold'])
    dists = {}
    for tgt, qry, tag in (('trgt', 'pred', 'pred'), ('pred', 'trgt', 'trgt')):
        idx, dist = nn(cuda, g[tgt], g[qry])
        ref = co.nearest(g[tgt], g[qry], distinct=(case == 'd'))
        co.check_nn('golden %s, %s rows' % (case, tag), g[tgt], g[qry], idx, dist, ref)
        # the reference's stored values under the same bounds
        stored = g['dist_' + tag]
        nz = stored > 0
        assert np.all(np.abs(dist - stored)[nz] <= co.DIST_BOUND * stored[nz]) and np.all(dist[~nz] == 0)
        clear = co.clear_gap(ref[1].numpy(), ref[2].numpy())
        assert np.array_equal(idx[clear], g['idx_' + tag][clear])
        dists[tag] = (dist, stored)
        # the reference's own entry point: lists, its argument order
        li, ld = m3.nn_correspondance(g[tgt], g[qry])
        assert isinstance(li, list) and li == idx.tolist() and ld == dist.tolist()
    rec = m3.cloud_metrics(torch.as_tensor(dists['pred'][0]).to(cuda), torch.as_tensor(dists['trgt'][0]).to(cuda), thr)
    co.check_metrics('golden %s' % case, rec.cpu().tolist(), dists['pred'][1], dists['trgt'][1], thr)
    m = m3.eval_mesh(g['pred'], g['trgt'], thr)
    assert list(m) == list(co.KEYS) and all(isinstance(v, float) for v in m.values())
    assert [m[k] for k in co.KEYS] == rec.cpu().tolist()
    for k in ('acc', 'comp'):
        assert abs(m[k] - float(g['m_' + k])) <= co.DIST_BOUND * float(g['m_' + k])
    assert abs(m['prec'] - float(g['m_prec'])) <= co.near_threshold(g['dist_pred'], thr) / len(g['dist_pred'])
    assert abs(m['recal'] - float(g['m_recal'])) <= co.near_threshold(g['dist_trgt'], thr) / len(g['dist_trgt'])


def _down(cuda, p, voxel, attr=None, count=None, trim=True):
    m3 = v3d('metrics3d')
    out = m3.voxel_down_sample(torch.as_tensor(p).to(cuda), voxel, None if attr is None else torch.as_tensor(attr).to(cuda),
                               None if count is None else torch.tensor(count, dtype=torch.int32, device=cuda), trim=trim)
    torch.cuda.synchronize()
    return out


def _compare_down(tag, out, ref):
    pts, attr, count = out
    m = int(count)
    assert m == len(ref['keys']) and pts.shape[0] >= m
    pts = pts[:m].cpu().numpy()
    e = float(ulps(pts, ref['pts']).max()) if m else 0.0
    same = bool(np.array_equal(pts, ref['pts']))
    ea = 0.0
    if ref['attr'] is not None:
        a = attr[:m].cpu().numpy()
        ea = float(ulps(a, ref['attr']).max())
        same = same and bool(np.array_equal(a, ref['attr']))
    print('%s: %d cells, points within %.2f ulp, attributes within %.2f ulp of the checker (bit-equal: %s)' % (tag, m, e, ea, same))
    assert e <= 1.0 and ea <= 1.0


def test_down_sample_faces_negative_coordinates_and_count_word(cuda):
    rng = np.random.default_rng(5)
    # (1) multiples of 1/8 in [-3, 3] with voxel 1/4: vmin = -3 - 1/8, so every odd multiple of 1/8 lies exactly on a cell face
    p = (rng.integers(-24, 25, (4000, 3)) / 8.0).astype(np.float32)
    p[0] = -3.0
    a = rng.random((4000, 3)).astype(np.float32)
    ref = co.voxel_down_sample(p, 0.25, a)
    assert len(ref['keys']) < 4000 and int((((p + 3.125) / 0.25) % 1 == 0).sum()) > 1000
    _compare_down('faces', _down(cuda, p, 0.25, a), ref)
    # (2) a noisy room moved to negative coordinates, 2 cm voxels, colours as attributes
    p = co.room(200000, 0.02, 41) - np.float32(7.5)
    a = rng.random((200000, 3)).astype(np.float32)
    ref = co.voxel_down_sample(p, 0.02, a)
    _compare_down('negative room', _down(cuda, p, 0.02, a), ref)
    # (3) the count as a device word smaller than the buffer; untrimmed outputs and the device count word
    ref = co.voxel_down_sample(p[:123457], 0.02, a[:123457])
    out = _down(cuda, p, 0.02, a, count=123457, trim=False)
    assert out[0].shape[0] == 200000 and out[2].dtype == torch.int32 and out[2].is_cuda
    _compare_down('count word', out, ref)
    _compare_down('count word 0', _down(cuda, p, 0.02, a, count=0, trim=False), co.voxel_down_sample(p[:0], 0.02))
    _compare_down('count word beyond the buffer', _down(cuda, p[:1000], 0.02, count=5000), co.voxel_down_sample(p[:1000], 0.02))
    # (4) repeated launches are bit-identical
    first = _down(cuda, p, 0.02, a)
    for _ in range(3):
        again = _down(cuda, p, 0.02, a)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]) and int(again[2]) == int(first[2])


def test_cloud_against_itself_and_translation(cuda):
    m3 = v3d('metrics3d')
    p = np.round(np.clip(co.room(30000, 0.02, 51, outliers=0.05).astype(np.float64), -7.5, 7.5) * 65536) / 65536
    p = np.unique(p.astype(np.float32), axis=0)                                # multiples of 2^-16 below 8: adding 8 or -64 is exact
    idx, dist = nn(cuda, p, p)
    assert np.array_equal(idx, np.arange(len(p))) and np.all(dist == 0)
    rec = m3.eval_clouds(torch.as_tensor(p).to(cuda), torch.as_tensor(p).to(cuda), 0.05).cpu().tolist()
    assert rec[:4] == [0.0, 0.0, 1.0, 1.0] and abs(rec[4] - 2 / (2 + 1e-8)) <= 1e-15
    q = np.round(co.room(20000, 0.0, 52).astype(np.float64) * 65536) / 65536
    q = q.astype(np.float32)
    ref = co.nearest(p, q)
    base = nn(cuda, p, q)
    co.check_nn('translation 0', p, q, base[0], base[1], ref)
    for shift in (8.0, -64.0):
        s = np.float32(shift)
        assert np.array_equal((p + s) - s, p) and np.array_equal((q + s) - s, q)
        idx, dist = nn(cuda, p + s, q + s)
        co.check_nn('translation %g' % shift, p, q, idx, dist, ref)
        # exact translation: the fp32 differences are the same numbers, so the results are the same bits
        assert np.array_equal(dist, base[1]) and np.array_equal(idx, base[0])


def test_permuting_the_queries_permutes_the_results(cuda):
    t, q = co.room(50000, 0.01, 61), co.room(40000, 0.02, 62, outliers=0.05)
    idx, dist = nn(cuda, t, q)
    perm = np.random.default_rng(63).permutation(len(q))
    idx_p, dist_p = nn(cuda, t, q[perm])
    assert np.array_equal(idx_p, idx[perm]) and np.array_equal(dist_p, dist[perm])
    perm_t = np.random.default_rng(64).permutation(len(t))                     # and permuting the target renames the rows
    idx_t, dist_t = nn(cuda, t[perm_t], q)
    assert np.array_equal(dist_t, dist)
    ref = co.nearest(t, q)
    clear = co.clear_gap(ref[1].numpy(), ref[2].numpy())
    assert np.array_equal(perm_t[idx_t][clear], idx[clear])


def test_single_point_far_queries_and_one_cell_targets(cuda):
    q = co.room(5000, 0.02, 71, outliers=0.05)
    one = np.array([[3.0, 1.5, 2.5]], dtype=np.float32)
    idx, dist = nn(cuda, one, q)
    co.check_nn('single-point target', one, q, idx, dist, co.nearest(one, q))
    assert np.all(idx == 0)
    t = co.room(20000, 0.01, 72)
    far = np.concatenate((q[:2000] + np.float32(1000.0), q[:2000] * np.float32(-50.0), q[:500] + np.array([0, 0, 40], np.float32)))
    idx, dist = nn(cuda, t, far)
    co.check_nn('queries far outside the target box', t, far, idx, dist, co.nearest(t, far))
    # all target rows in one fine cell (the cell edge follows the extent, so that means identical rows): the lowest row wins
    same = np.repeat(one, 300, axis=0)
    both = np.concatenate((q, one))
    idx, dist = nn(cuda, same, both)
    co.check_nn('identical target rows', same, both, idx, dist, co.nearest(same, both, distinct=True))
    assert np.all(idx == 0) and dist[-1] == 0


def test_empty_clouds(cuda):
    m3 = v3d('metrics3d')
    some, none = torch.rand(10, 3, device=cuda), torch.zeros(0, 3, device=cuda)
    idx, dist = m3.nearest_neighbors(none, some)
    assert idx.tolist() == [-1] * 10 and bool(torch.isinf(dist).all())
    idx, dist = m3.nearest_neighbors(some, none)
    assert idx.shape == (0,) and dist.shape == (0,)
    rec = m3.cloud_metrics(dist, torch.zeros(4, device=cuda), 0.05).cpu().tolist()
    assert math.isnan(rec[0]) and math.isnan(rec[2]) and rec[1] == 0.0 and rec[3] == 1.0 and math.isnan(rec[4])
    pts, attr, count = m3.voxel_down_sample(none, 0.02, trim=True)
    assert pts.shape == (0, 3) and attr is None and int(count) == 0
    assert m3.nn_correspondance(none, some) == ([], [])
    assert all(math.isnan(v) for v in m3.eval_mesh(some, none).values())


def test_error_codes(cuda):
    m3, lib_mod = v3d('metrics3d'), v3d('_lib')
    lib = lib_mod.load()
    p = torch.rand(100, 3, device=cuda)
    for vs in (0.0, -1.0, float('nan'), float('inf')):
        assert int(m3.voxel_down_sample(p, vs)[2]) == -4
        with pytest.raises(lib_mod.V3DLibraryError, match='V3D_ERR_BAD_ARG.*voxel_size'):
            m3.voxel_down_sample(p, vs, trim=True)
    for bad in (float('nan'), float('inf'), -float('inf')):
        b = p.clone()
        b[37, 1] = bad
        assert int(m3.voxel_down_sample(b, 0.02)[2]) == -1
        with pytest.raises(lib_mod.V3DLibraryError, match='non-finite'):
            m3.voxel_down_sample(b, 0.02, trim=True)
        assert int(m3.voxel_down_sample(b, 0.02, count=torch.tensor(37, dtype=torch.int32, device=cuda))[2]) > 0   # row 37 not in use
    # the rows lie in [0, 1): the farthest cell index is z / 0.02 + 0.5 - min / 0.02, i.e. up to 50 cells below z / 0.02
    wide = p.clone()
    wide[5, 2] = 0.02 * (2 ** 21 + 100)
    assert int(m3.voxel_down_sample(wide, 0.02)[2]) == -2
    with pytest.raises(lib_mod.V3DLibraryError, match='V3D_ERR_BAD_SHAPE.*2\\^21'):
        m3.voxel_down_sample(wide, 0.02, trim=True)
    wide[5, 2] = 0.02 * (2 ** 21 - 100)
    assert int(m3.voxel_down_sample(wide, 0.02)[2]) > 0
    d = torch.rand(10, device=cuda)
    for thr in (0.0, -0.05, float('nan')):
        with pytest.raises(lib_mod.V3DLibraryError, match='threshold'):
            m3.cloud_metrics(d, d, thr)
    ws = torch.empty(1024, dtype=torch.uint8, device=cuda)
    out = torch.empty(100, dtype=torch.int32, device=cuda)
    assert lib.v3d_nn_query_f32(p.data_ptr(), 100, p.data_ptr(), 100, out.data_ptr(), out.data_ptr(), ws.data_ptr(), 1024, None) == -3
    assert lib.v3d_cloud_downsample_f32(p.data_ptr(), None, 0, 100, None, 0.02, p.data_ptr(), None, out.data_ptr(), ws.data_ptr(),
                                        1024, None) == -3
    assert lib.v3d_cloud_downsample_f32(p.data_ptr(), None, 65, 100, None, 0.02, p.data_ptr(), None, out.data_ptr(), ws.data_ptr(),
                                        1024, None) == -1
    with pytest.raises(ValueError):
        m3.nearest_neighbors(p, p.double())
    with pytest.raises(lib_mod.V3DLibraryError):
        m3.nearest_neighbors(p, p.cpu())


def test_full_size_scene(cuda):
    """The 64-view 480 x 640 scene of tests/fusion_oracle.py (sigma = 4 cm, 3 % zeroed pixels), fused, down-sampled at 2 cm and
    scored against 3 M samples of the generator's noise-free room surfaces down-sampled the same way (>= 300 k rows); 5 % of the
    predicted rows are displaced by N(0, 0.5 m) so that the coarse levels of the search run.  Every distance of both directions
    is checked against a float64 brute force in stock torch ops on the same GPU; then ten launches are bit-identical, and
    depth_3d_metrics equals the staged calls bit for bit."""
    m3, fusion, syn = v3d('metrics3d'), v3d('fusion'), v3d('synthetic')
    d, img, poses, K = fo.scene(64, (480, 640), seed=1237, yaw_step_deg=None, sigma=0.04)
    dev_d, dev_img = d.to(cuda), img.to(cuda)
    pts, rgb, _, count = fusion.fuse_depth_maps(dev_d, poses, K, dev_img, 0.1, 3, trim=False)
    pred, col, n_pred = m3.voxel_down_sample(pts, 0.02, attr=rgb.float() / 255., count=count)
    gt_raw = torch.as_tensor(co.room(3000000, 0.0, 81, dims=syn.ROOM)).to(cuda)
    trgt, _, n_trgt = m3.voxel_down_sample(gt_raw, 0.02)
    n_pred, n_trgt = int(n_pred), int(n_trgt)
    print('full size: %d fused rows -> %d predicted rows, %d target rows' % (int(count), n_pred, n_trgt))
    assert n_trgt >= 300000 and n_pred > 100000
    pred, trgt = pred[:n_pred], trgt[:n_trgt]
    # the down-sample of the whole fused cloud against the checker (colours as attributes)
    m = int(count)
    ref = co.voxel_down_sample(pts[:m].cpu().numpy(), 0.02, (rgb[:m].float() / 255.).cpu().numpy())
    _compare_down('full size', (pred, col[:n_pred], n_pred), ref)

    g = torch.Generator().manual_seed(82)
    k = n_pred // 20
    rows = torch.randperm(n_pred, generator=g)[:k].to(cuda)
    moved = pred.clone()
    moved[rows] += (0.5 * torch.randn(k, 3, generator=g)).to(cuda)
    staged = {}
    for tgt, qry, tag in ((trgt, moved, 'pred'), (moved, trgt, 'trgt')):
        idx, dist = m3.nearest_neighbors(tgt, qry)
        torch.cuda.synchronize()
        ref = co.nearest(tgt, qry, device=cuda, chunk_elems=1 << 28)
        co.check_nn('full size, %s rows' % tag, tgt.cpu().numpy(), qry.cpu().numpy(), idx.cpu().numpy(), dist.cpu().numpy(), ref)
        staged[tag] = (idx, dist, ref[1].cpu().numpy())
    rec = m3.cloud_metrics(staged['pred'][1], staged['trgt'][1], 0.05)
    co.check_metrics('full size', rec.cpu().tolist(), staged['pred'][2], staged['trgt'][2], 0.05)
    share = float((staged['pred'][1] >= 0.0625).float().mean())
    print('full size: %.2f %% of the predicted rows are farther than 6.25 cm from the target' % (100 * share))
    assert share > 0.02                                           # the coarse levels did run

    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=cuda)
    for _ in range(10):
        with torch.cuda.stream(side):
            for _ in range(4):
                a @ a
        again = m3.voxel_down_sample(pts, 0.02, attr=rgb.float() / 255., count=count)
        assert int(again[2]) == n_pred and torch.equal(again[0][:n_pred], pred) and torch.equal(again[1][:n_pred], col[:n_pred])
        for tgt, qry, tag in ((trgt, moved, 'pred'), (moved, trgt, 'trgt')):
            idx, dist = m3.nearest_neighbors(tgt, qry)
            assert torch.equal(idx, staged[tag][0]) and torch.equal(dist, staged[tag][1])
        assert torch.equal(m3.eval_clouds(moved, trgt, 0.05), rec)

    want = dict(zip(co.KEYS, m3.eval_clouds(pred, trgt, 0.05).cpu().tolist()), n=64)
    preds = dict(depth_preds=d.numpy(), rotmats=poses[:, :3, :3].numpy(), tvecs=poses[:, :3, 3].numpy(), K=K.numpy())
    got = m3.depth_3d_metrics(preds, img, gt_raw, 0.1, 3, 0.02, 0.05)
    print('full size: depth_3d_metrics %s' % got)
    assert got == want and list(got) == list(co.KEYS) + ['n']
