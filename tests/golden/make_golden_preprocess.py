#!/usr/bin/env python3
"""Golden vectors of scene preparation: the REFERENCE's own ``process_color_image`` (``data_preprocess/preprocess_scannet.py:36-70``)
executed from the source file in memory, and SciPy's quaternion matrices.  Nothing of the reference's text is written to disk.

``preprocess_scannet.py`` imports ``cv2`` and ``tqdm`` at its top, which are not needed by the function: the function's definition
is taken out of the parsed module by ``ast`` and executed with ``np`` and ``torch`` alone (as make_golden_mesh.py runs the reference
around a stand-in).

Run in the build container only:  python tests/golden/make_golden_preprocess.py
Outputs (committed, data only):
  P_register_down2     37 x 53 -> 19 x 27, n = 3: focal lengths and principal point doubled, the colour camera's principal point two
                       columns further right: the 19 pixels of the last column sample outside
  P_register_focal     the same sizes, focal ratio 2.55: 198 of the 513 pixels outside
  P_register_skew      the same sizes, a projective pair: every one of the nine terms of H is non-zero; 19 outside
  P_register_aligned   24 x 32 -> 12 x 16, n = 3: a width that is a multiple of four (the dword-store path)
  P_register_tie       6 x 6 arange -> 3 x 3, K_color = diag(3, 3, 1), K_depth = I: output pixel (1, 1) sits exactly on ix = iy =
                       2.5 and the reference returns colour[2, 2] (half to even)
  P_register_full_{a,b}   968 x 1296 -> 480 x 640 with two ScanNet intrinsics pairs: seed, intrinsics, the count of outside pixels
                       (0 and 2 077) and the SHA-256 of the reference's output
  P_quat               16 seeded quaternions, some not normalised, and SciPy's matrices
The generator refuses to write unless the NumPy checker (tests/preprocess_oracle.py) equals the reference on every case with 0
mismatching pixels and the outside counts are the ones above.
"""
import ast
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import preprocess_oracle as po  # noqa: E402

REFERENCE_FILE = os.path.join(_ref_import.REFERENCE_ROOT, 'data_preprocess', 'preprocess_scannet.py')
LIMIT = 64 * 1024          # bytes per fixture


def load_process_color_image():
    with open(REFERENCE_FILE) as f:
        tree = ast.parse(f.read())
    fn = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == 'process_color_image']
    assert len(fn) == 1
    ns = {'np': np, 'torch': torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), REFERENCE_FILE, 'exec'), ns)
    return ns['process_color_image']


def projective(f, skew, cx):
    K = po.kmat(f, f + 1.5, cx, 18.2, skew=skew)
    K[1, 0], K[2, 0], K[2, 1] = 0.8, 1e-3, -2e-3
    return K


SMALL = {
    # name: (seed, n, (Hc, Wc), (h, w), K_color, K_depth, outside)
    'register_down2': (11, 3, (37, 53), (19, 27), po.kmat(40, 40, 28, 18), po.kmat(20, 20, 13, 9), 19),
    'register_focal': (12, 3, (37, 53), (19, 27), po.kmat(51, 51, 26, 18), po.kmat(20, 20, 13, 9), 198),
    'register_skew': (13, 3, (37, 53), (19, 27), projective(38.5, 1.0, 24.3), po.kmat(20, 20.5, 13, 9, skew=0.7), 19),
    'register_aligned': (14, 3, (24, 32), (12, 16), po.kmat(32, 32, 16, 12), po.kmat(16, 16, 8, 6), 0),
    'register_tie': (None, 1, (6, 6), (3, 3), np.diag([3., 3., 1.]), np.eye(3), 0),
}
FULL = {'register_full_a': (21, 'a', 0), 'register_full_b': (22, 'b', 2077)}


def save(name, **arrays):
    path = os.path.join(HERE, 'P_%s.npz' % name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= LIMIT, '%s is %d bytes' % (path, size)
    print('%s: %d bytes' % (os.path.basename(path), size))


def main():
    ref = load_process_color_image()
    for name, (seed, n, (Hc, Wc), (h, w), Kc, Kd, outside) in SMALL.items():
        if seed is None:
            colour = (np.arange(Hc * Wc * 3) % 256).astype(np.uint8).reshape(1, Hc, Wc, 3)
        else:
            colour = po.random_colour(seed, n, Hc, Wc)
        want = np.stack([ref(colour[i], np.zeros((h, w)), Kc, Kd) for i in range(n)])
        got, out = po.register(colour, (h, w), po.homography(Kc, Kd))
        assert want.dtype == np.uint8 and np.array_equal(got, want), '%s: the checker differs from the reference' % name
        assert int(out.sum()) == outside, '%s: %d pixels outside, %d expected' % (name, int(out.sum()), outside)
        save(name, colour=colour, K_color=Kc, K_depth=Kd, depth_size=np.array([h, w]), expected=want, outside=np.int64(out.sum()))
    tie = np.load(os.path.join(HERE, 'P_register_tie.npz'))
    assert np.array_equal(tie['expected'][0, 1, 1], tie['colour'][0, 2, 2]) and not np.array_equal(tie['colour'][0, 2, 2], tie['colour'][0, 3, 3])
    for name, (seed, pair, outside) in FULL.items():
        Kc, Kd = (po.kmat(*v) for v in po.SCANNET_PAIRS[pair])
        colour = po.random_colour(seed, 1, 968, 1296)
        want = ref(colour[0], np.zeros((480, 640)), Kc, Kd)
        got, out = po.register(colour[0], (480, 640), po.homography(Kc, Kd))
        mism = int((got != want).any(axis=-1).sum())
        print('%s: %d mismatching pixels of %d, %d outside' % (name, mism, 480 * 640, int(out.sum())))
        assert mism == 0 and int(out.sum()) == outside
        save(name, seed=np.int64(seed), K_color=Kc, K_depth=Kd, colour_size=np.array([968, 1296]), depth_size=np.array([480, 640]),
             outside=np.int64(out.sum()), sha256=np.array(po.sha256(want)))
    from scipy.spatial.transform import Rotation
    q = np.random.RandomState(5).randn(16, 4)
    q[::3] *= 3.0                                                  # not normalised
    q[1::4] /= np.linalg.norm(q[1::4], axis=1, keepdims=True)      # normalised within a rounding
    save('quat', q=q, matrices=Rotation.from_quat(q).as_matrix())


if __name__ == '__main__':
    main()
