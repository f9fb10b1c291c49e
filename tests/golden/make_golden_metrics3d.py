#!/usr/bin/env python3
"""Golden vectors of the 3D cloud metrics: the REFERENCE's own ``mv3d/eval/metricfunctions.py`` (nn_correspondance,
eval_mesh) and ``mv3d/eval/processresults.py`` (calc_avg_metrics), unmodified, from where they lie (imported with the stubs
of _ref_import.py).  Open3D is not available, so the two things the reference asks of it are stood in for here: a holder
with ``.points`` and a ``KDTreeFlann`` whose ``search_knn_vector_3d`` is an exact float64 brute-force search returning
squared distances (what the FLANN tree returns for k = 1, without its dependence on build order among exact ties: the
lowest index wins).

Run in the build container only:  python tests/golden/make_golden_metrics3d.py
Outputs tests/golden/M_metrics3d_*.npz (committed): seeded clouds, the reference's distances and indices in both
directions and its eval_mesh numbers; M_metrics3d_avg.npz: per-scene metric dicts and the reference's averages -- data only.
"""
import glob
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _ref_import  # noqa: E402
import cloud_oracle  # noqa: E402

LIMIT = 587073          # bytes of tests/golden/C_decoder_net.npz, the largest golden there is


class Cloud:
    """Stand-in of o3d.geometry.PointCloud as the reference uses it: ``.points`` (float64, as Vector3dVector holds them)."""

    def __init__(self, points):
        self.points = np.asarray(points, dtype=np.float64).reshape(-1, 3)


class KDTreeFlann:
    def __init__(self, pcd):
        self.pts = np.asarray(pcd.points, dtype=np.float64)

    def search_knn_vector_3d(self, vert, k):
        assert k == 1
        d = ((self.pts - np.asarray(vert, dtype=np.float64)[None]) ** 2).sum(1)
        i = int(np.argmin(d))                   # first of equal minima
        return 1, [i], [float(d[i])]


_ref_import.install_stubs()
sys.modules['open3d'].geometry = types.SimpleNamespace(KDTreeFlann=KDTreeFlann, PointCloud=Cloud)
for name in ('tqdm', 'PIL', 'PIL.Image'):
    if name not in sys.modules:
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
from mv3d.eval import metricfunctions as ref_metrics  # noqa: E402


def case(name, pred, trgt, threshold=0.05):
    pcd_pred, pcd_trgt = Cloud(pred), Cloud(trgt)
    idx1, dist1 = ref_metrics.nn_correspondance(pcd_trgt, pcd_pred)        # per predicted vertex (eval_mesh's dist1)
    idx2, dist2 = ref_metrics.nn_correspondance(pcd_pred, pcd_trgt)
    m = ref_metrics.eval_mesh(pcd_pred, pcd_trgt, threshold)
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, pred=pred, trgt=trgt, threshold=np.float64(threshold), idx_pred=np.asarray(idx1, dtype=np.int64),
                        dist_pred=np.asarray(dist1, dtype=np.float64), idx_trgt=np.asarray(idx2, dtype=np.int64),
                        dist_trgt=np.asarray(dist2, dtype=np.float64),
                        **{'m_' + k: np.float64(v) for k, v in m.items()})
    assert os.path.getsize(path) <= LIMIT, path
    print('wrote %s (%.1f KB): %s' % (path, os.path.getsize(path) / 1024, m))


def averages():
    """calc_avg_metrics on a temporary directory of per-scene json files (2D keys are n-weighted, 3D keys plain means)."""
    try:
        from mv3d.eval import processresults as ref_pr
        calc = ref_pr.calc_avg_metrics
    except Exception as e:                       # its import chain (datasets, cv2 ...) is not the function under test
        print('processresults does not import here (%s): executing its calc_avg_metrics from the source file' % e)
        import ast
        src = open(os.path.join(_ref_import.REFERENCE_ROOT, 'mv3d', 'eval', 'processresults.py')).read()
        fn = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == 'calc_avg_metrics'][0]
        ns = dict(os=os, glob=glob, json=json, np=np)
        exec(compile(ast.Module(body=[fn], type_ignores=[]), 'processresults.py', 'exec'), ns)
        calc = ns['calc_avg_metrics']
    rng = np.random.default_rng(7)
    scenes = {}
    for s, n in (('scene0000_00', 64), ('scene0001_00', 37), ('scene0002_01', 121)):
        scenes[s] = {
            'metrics_3d.json': dict({k: float(rng.random()) for k in cloud_oracle.KEYS}, n=n),
            'metrics_2d.json': dict({k: float(rng.random()) for k in ('abs_rel', 'abs_diff', 'rmse', 'd_125')}, n=n),
        }
    with tempfile.TemporaryDirectory() as tmp:
        for s, files in scenes.items():
            os.makedirs(os.path.join(tmp, 'scenes', s))
            for fname, rec in files.items():
                json.dump(rec, open(os.path.join(tmp, 'scenes', s, fname), 'w'))
        calc(tmp)
        avg = {os.path.basename(f): json.load(open(f)) for f in glob.glob(os.path.join(tmp, 'metrics*.json'))}
    path = os.path.join(HERE, 'M_metrics3d_avg.npz')
    np.savez_compressed(path, scenes_json=np.array(json.dumps(scenes)), avg_json=np.array(json.dumps(avg)))
    print('wrote %s: %s' % (path, avg))


def main():
    # (a) two noisy room clouds
    case('M_metrics3d_a', cloud_oracle.room(4000, 0.02, 21), cloud_oracle.room(3000, 0.005, 22))
    # (b) 5 % of the predicted rows far off (sigma 0.5 m)
    case('M_metrics3d_b', cloud_oracle.room(5000, 0.02, 23, outliers=0.05), cloud_oracle.room(3500, 0.0, 24))
    # (c) a single-point target
    case('M_metrics3d_c', cloud_oracle.room(1500, 0.02, 25), np.array([[3.0, 1.5, 2.5]], dtype=np.float32))
    # (d) exact duplicates: rows repeated inside each cloud and shared between the clouds (zero distances, index ties)
    a, b = cloud_oracle.room(1200, 0.02, 26), cloud_oracle.room(1000, 0.01, 27)
    pred = np.concatenate((a, a[:300], b[:200]))
    trgt = np.concatenate((b, b[100:400], a[500:600]))
    case('M_metrics3d_d', pred, trgt)
    averages()


if __name__ == '__main__':
    main()
