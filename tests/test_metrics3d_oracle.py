"""CPU: the float64 checker of the 3D cloud metrics (tests/cloud_oracle.py) against the reference's recorded outputs
(tests/golden/M_metrics3d_*.npz, written by tests/golden/make_golden_metrics3d.py) and against scipy's KD-tree; the host
side of 3dvnet_amd/metrics3d.py (validation, empty clouds, no CPU fallback); results.average_metrics against the reference's
calc_avg_metrics."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import cloud_oracle as co
from conftest import ROOT, v3d

CASES = ['a', 'b', 'c', 'd']


def load_case(case):
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'M_metrics3d_%s.npz' % case)) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize('case', CASES)
def test_checker_reproduces_the_reference(case):
    """Same float64 arithmetic on the same inputs: distances equal to the last bits of the root, indices equal (both take
    the first of equal minima), metrics equal to rounding of the means."""
    g = load_case(case)
    for tgt, qry, tag in (('trgt', 'pred', 'pred'), ('pred', 'trgt', 'trgt')):
        idx, d1, _ = co.nearest(g[tgt], g[qry])
        assert np.array_equal(idx.numpy(), g['idx_' + tag])
        assert np.allclose(d1.numpy(), g['dist_' + tag], rtol=1e-14, atol=0)
    m = co.metrics(g['dist_pred'], g['dist_trgt'], float(g['threshold']))
    for k in co.KEYS:
        assert m[k] == pytest.approx(float(g['m_' + k]), rel=1e-13, abs=0), k
    assert set(k[2:] for k in g if k.startswith('m_')) == set(co.KEYS)


def test_checker_against_kdtree():
    spatial = pytest.importorskip('scipy.spatial')
    pred, trgt = co.room(6000, 0.02, 31, outliers=0.05), co.room(4000, 0.0, 32)
    for t, q in ((trgt, pred), (pred, trgt)):
        d, i = spatial.cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=2)
        idx, d1, d2 = co.nearest(t, q)
        assert np.allclose(d1.numpy(), d[:, 0], rtol=1e-14, atol=0) and np.allclose(d2.numpy(), d[:, 1], rtol=1e-14, atol=0)
        clear = d[:, 1] > d[:, 0]
        assert np.array_equal(idx.numpy()[clear], i[clear, 0])


def test_distinct_search_names_the_first_duplicate():
    t = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0], [5, 5, 5]], dtype=np.float32)
    q = np.array([[0.1, 0, 0], [0.9, 0, 0], [5, 5, 4]], dtype=np.float32)
    idx, d1, d2 = co.nearest(t, q, distinct=True)
    assert idx.tolist() == [0, 1, 4]
    assert np.allclose(d1.numpy(), [0.1, 0.1, 1.0], atol=1e-7) and np.allclose(d2.numpy()[:2], [0.9, 0.9], atol=1e-7)


def test_checker_down_sample_by_hand():
    """Cells of edge 1 from vmin = min - 0.5: rows on a cell face belong to the upper cell; means in row order."""
    p = np.array([[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [1.5, 0, 0], [-0.0, 0.5, 0], [0.4, 0.1, 0.2]], dtype=np.float32)
    a = np.arange(12, dtype=np.float32).reshape(6, 2)
    r = co.voxel_down_sample(p, 1.0, a)
    # x cells: [-0.5, 0.5) -> 0, 0.5 -> 1, 1.5 -> 2; y: 0.5 -> 1
    assert r['keys'].tolist() == [0, 1 << 21, 1 << 42, 2 << 42] and r['counts'].tolist() == [3, 1, 1, 1]
    assert np.array_equal(r['pts'][0], ((p[0].astype(np.float64) + p[1] + p[5]) / 3).astype(np.float32))
    assert np.array_equal(r['attr'][0], ((a[0].astype(np.float64) + a[1] + a[5]) / 3).astype(np.float32))
    assert np.array_equal(r['pts'][1], p[4]) and np.array_equal(r['pts'][2], p[2]) and np.array_equal(r['pts'][3], p[3])
    neg = co.voxel_down_sample(p - 7.5, 1.0)
    assert np.array_equal(neg['keys'], r['keys']) and np.array_equal(neg['counts'], r['counts'])


def test_empty_clouds_need_no_device():
    m3 = v3d('metrics3d')
    some, none = np.zeros((4, 3), np.float32), np.zeros((0, 3), np.float32)

    class Holder:
        points = none

    for a, b in ((some, none), (none, some), (Holder(), torch.zeros(2, 3)), (none, none)):
        assert m3.nn_correspondance(a, b) == ([], [])
        m = m3.eval_mesh(a, b)
        assert list(m) == ['acc', 'comp', 'prec', 'recal', 'fscore'] and all(math.isnan(v) for v in m.values())
    want = co.metrics([], [], 0.05)                       # what NumPy gives the reference
    assert all(math.isnan(v) for v in want.values())


def test_no_cpu_fallback():
    m3, lib_mod = v3d('metrics3d'), v3d('_lib')
    p = torch.zeros(5, 3)
    # host tensors are refused by the device-tensor entries wherever the test runs; the array entries move their input to
    # the device when there is one, so they are only expected to fail on a machine without
    calls = [lambda: m3.voxel_down_sample(p, 0.02), lambda: m3.nearest_neighbors(p, p), lambda: m3.eval_clouds(p, p),
             lambda: m3.cloud_metrics(p[:, 0], p[:, 0], 0.05)]
    if not torch.cuda.is_available():
        calls += [lambda: m3.nn_correspondance(p.numpy(), p.numpy()), lambda: m3.eval_mesh(p.numpy(), p.numpy()),
                  lambda: m3.depth_3d_metrics({}, p, p, 0.1)]
    for call in calls:
        with pytest.raises(lib_mod.V3DLibraryError):
            call()


def test_host_validation_of_the_c_abi():
    """Errors that return before anything touches the device."""
    lib_mod = v3d('_lib')
    lib = lib_mod.load()
    one = ctypes.c_void_p(256)                            # never dereferenced: every call below fails first
    assert lib.v3d_cloud_downsample_workspace_bytes(-1) == 0 and lib.v3d_nn_workspace_bytes(-1, 3) == 0
    assert lib.v3d_cloud_downsample_workspace_bytes(1000) > 1000 * 32
    assert lib.v3d_nn_workspace_bytes(1000, 10) > (1 << 18) * 4
    assert lib.v3d_cloud_downsample_f32(None, None, 0, 4, None, 0.02, None, None, None, None, 0, None) == -2
    assert b'null' in lib.v3d_last_error()
    assert lib.v3d_cloud_downsample_f32(one, None, 0, -1, None, 0.02, one, None, one, one, 1 << 30, None) == -1
    assert lib.v3d_cloud_downsample_f32(one, None, 3, 4, None, 0.02, one, None, one, one, 1 << 30, None) == -2
    assert lib.v3d_cloud_downsample_f32(one, None, 0, 4, None, 0.02, one, None, one, one, 16, None) == -3
    assert lib.v3d_nn_query_f32(one, -1, one, 4, one, one, one, 1 << 30, None) == -1
    assert lib.v3d_nn_query_f32(None, 4, one, 4, one, one, one, 1 << 30, None) == -2
    assert lib.v3d_nn_query_f32(one, 4, one, 4, one, one, one, 16, None) == -3
    assert lib.v3d_nn_query_f32(one, 4, None, 0, None, None, None, 0, None) == 0          # no queries: nothing to do
    assert lib.v3d_cloud_metrics_f64(None, 4, one, 4, 0.05, one, one, 1 << 20, None) == -2
    assert lib.v3d_cloud_metrics_f64(one, 4, one, 4, 0.0, one, one, 1 << 20, None) == -2 and b'threshold' in lib.v3d_last_error()
    assert lib.v3d_cloud_metrics_f64(one, 4, one, 4, float('nan'), one, one, 1 << 20, None) == -2
    assert lib.v3d_cloud_metrics_f64(one, 4, one, -4, 0.05, one, one, 1 << 20, None) == -1
    assert lib.v3d_cloud_metrics_f64(one, 4, one, 4, 0.05, one, one, 8, None) == -3
    assert lib.v3d_cloud_status(None, 0, None, None) == -2
    assert lib.v3d_version() == 9


def test_average_metrics_matches_the_reference():
    results = v3d('results')
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'M_metrics3d_avg.npz')) as f:
        scenes, avg = json.loads(str(f['scenes_json'])), json.loads(str(f['avg_json']))
    assert set(avg) == {'metrics_2d.json', 'metrics_3d.json'}
    for fname, want in avg.items():
        got = results.average_metrics([scenes[s][fname] for s in scenes])          # the reference walks os.listdir order
        assert set(got) == set(want)
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=1e-14, abs=0), (fname, k)
    only3d = results.average_metrics([{'acc': 1.0, 'fscore': 0.5}, {'acc': 2.0, 'fscore': 0.25}])      # no 'n' needed
    assert only3d == {'acc': 1.5, 'fscore': 0.375}
