#!/usr/bin/env python3
"""Golden vectors of the scene-batch front end: the REFERENCE's own frame selectors (``mv3d/dsets/frameselector.py``) and
``PreprocessImage`` (``mv3d/dsets/dataset.py:21-96``: constructor and ``get_updated_intrinsics``) executed from where they lie,
through the import stand-ins of _ref_import.py, on the seeded inputs of tests/dataset_oracle.py.  Nothing of the reference's text
is written to disk.

Run in the build container only:  python tests/golden/make_golden_dataset.py
Outputs (committed, data only):
  Dset_selectors.npz    one int64 index array per case of dataset_oracle.selector_cases() (five selectors x three pose walks x
                        n_frames 4 / 10 / 100000 x seed_idx None / 0 / mid-sequence, ``np.random.seed`` fixed before each call),
                        and the SHA-256 of every pose walk
  Dset_preprocess.npz   per case of dataset_oracle.PREPROCESS_CASES: crop_x, crop_y (int64) and the 3 x 3 float64 intrinsics

``mv3d/dsets/dataset.py`` imports three names from kornia and subclasses ``torch_geometric.data.Dataset``; both are absent here and
the stand-ins of _ref_import.py do not carry them, so this script adds them to the stubbed modules before the import (its
``apply_rgb`` / ``apply_depth`` call OpenCV, which is absent as well: their outputs cannot be recorded here).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import _ref_import  # noqa: E402
import dataset_oracle as oracle  # noqa: E402

_ref_import.install_stubs()
for _name in ('adjust_brightness', 'adjust_gamma', 'adjust_contrast'):
    setattr(sys.modules['kornia'], _name, None)
sys.modules['torch_geometric.data'].Dataset = object

from mv3d.dsets import dataset as ref_dataset  # noqa: E402
from mv3d.dsets import frameselector as ref_selector  # noqa: E402


def selectors():
    out = {}
    walks = {w: oracle.pose_walk(w) for w in oracle.WALKS}
    for w, p in walks.items():
        out['sha_' + w] = np.str_(oracle.digest(p))
    for key, walk, cls, args, n_frames, seed_idx, np_seed in oracle.selector_cases():
        np.random.seed(np_seed)
        idx = getattr(ref_selector, cls)(*args).select_frames(walks[walk], n_frames, seed_idx)
        out[key] = np.asarray(idx, dtype=np.int64)
        assert out[key].ndim == 1 and len(out[key]) >= 1
    return out


def preprocess():
    out = {}
    for key, H, W, nh, nw, crop in oracle.PREPROCESS_CASES:
        p = ref_dataset.PreprocessImage(K=oracle.intrinsics(H, W), old_width=W, old_height=H, new_width=nw, new_height=nh,
                                        distortion_crop=0, perform_crop=crop)
        K = p.get_updated_intrinsics()
        assert K.dtype == np.float64
        out[key + '_crop'] = np.asarray([p.crop_x, p.crop_y], dtype=np.int64)
        out[key + '_K'] = K
    return out


def main():
    for name, arrays in (('Dset_selectors', selectors()), ('Dset_preprocess', preprocess())):
        path = os.path.join(HERE, name + '.npz')
        np.savez_compressed(path, **arrays)
        print('wrote %s (%.1f KB, %d arrays)' % (path, os.path.getsize(path) / 1024, len(arrays)))
        assert os.path.getsize(path) < 64 * 1024


if __name__ == '__main__':
    main()
