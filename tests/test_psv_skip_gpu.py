"""Pass skip of the window warp kernel (csrc/psv_window.hip; developer option psv_skip, default 1): a pass -- one edge, 8 planes,
8 pixels -- whose 64 samples all fall beside the source image adds exactly zero to the sums and is left out.  Every variant must
give the bits of psv_skip = 0, the kernel that never skips, and the reuse kernel (which has no skip) must give them too.

The cases (scripts/psv_skip_dump.py) are chosen so that the skip fires: each test works out the share of skipped passes from the
positions the device itself samples at (v3d_psv_sample_positions_f32), with the kernel's rule and grouping
(scripts/psv_skip_share.py), and fails if the case has gone vacuous.

The developer options are process-wide, so every variant writes its volumes in an interpreter of its own; the dumps are made once
per session and shared by the tests."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VAR_ATOL = 5e-7          # vs the pinned oracle, as tests/test_costvolume_gpu.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {'default': [], 'skip0': ['--option=psv_skip=0'], 'reuse': ['--option=psv_kernel=1'],
            'walk1': ['--option=psv_walk=1'], 'walk3': ['--option=psv_walk=3']}
TAGS = ('a', 'b', 'c', 'd', 'e', 'f')


def _scripts():
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import psv_skip_dump as pd
        import psv_skip_share as ss
    finally:
        sys.path.pop(0)
    return pd, ss


@pytest.fixture(scope='module')
def dumps(cuda, tmp_path_factory):
    td = tmp_path_factory.mktemp('psv_skip')
    res = {}
    for name, extra in VARIANTS.items():
        f = str(td / (name + '.npz'))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'psv_skip_dump.py'), f] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = dict(np.load(f))
    return res


@pytest.fixture(scope='module')
def passes(dumps):
    """tag -> non-zero samples per pass [E (CSR order), plane chunks, pixel tiles], from the device's own positions."""
    pd, ss = _scripts()
    out = {}
    for tag in TAGS:
        _, _, D, plane = pd.CASES[tag]
        pos = dumps['skip0'][tag + '_pos']
        assert np.array_equal(pos.view(np.uint32), dumps['default'][tag + '_pos'].view(np.uint32)), tag
        pos = pos.reshape(pos.shape[0], D, plane[0] * plane[1], 2)
        out[tag] = ss.pass_live_counts(ss.zero_mask(pos[..., 0], pos[..., 1], pd.FEAT))
    return out


@pytest.mark.parametrize('tag', TAGS)
def test_every_variant_gives_the_bits_of_the_kernel_that_never_skips(tag, dumps):
    base = dumps['skip0']
    for kind in ('f32', 'split', 'cl8'):
        key = '%s_%s' % (tag, kind)
        assert base[key].size > 0, key
        if kind != 'split':
            assert np.isfinite(base[key].view(np.float32)).all(), key
        for name in ('default', 'walk1', 'walk3'):
            assert np.array_equal(dumps[name][key].view(np.uint32), base[key].view(np.uint32)), (name, key)
        if kind != 'cl8':
            assert np.array_equal(dumps['reuse'][key].view(np.uint32), base[key].view(np.uint32)), ('reuse', key)
    # the volume is not trivially empty
    assert float(np.abs(base[tag + '_f32'].view(np.float32)).max()) > 1e-3


@pytest.mark.parametrize('tag', ['a', 'b', 'c', 'd'])
def test_the_skip_fires_in_the_case(tag, passes):
    cnt = passes[tag]
    share = float((cnt == 0).mean())
    print('case %s: %d of %d passes all zero (%.1f %%), %d passes with 1-8 non-zero samples'
          % (tag, int((cnt == 0).sum()), cnt.size, 100 * share, int(((cnt >= 1) & (cnt <= 8)).sum())))
    assert 0.10 <= share <= 0.90


def test_near_misses_exist_in_case_a(passes):
    cnt = passes['a']
    assert int(((cnt >= 1) & (cnt <= 8)).sum()) >= 1      # passes with a handful of samples inside the image: not skipped


def test_wholly_skipped_edges_sit_either_side_of_the_camera_reload_in_case_c(dumps, passes):
    pd, _ = _scripts()
    ofs, src, ref = dumps['skip0']['c_ofs'], dumps['skip0']['c_src'], dumps['skip0']['c_ref']
    cnt = passes['c']
    assert len(ref) == 2
    for r in range(len(ref)):
        ne = int(ofs[r + 1] - ofs[r])
        assert ne == 13                                       # more than the 8 camera blocks held in LDS
        whole = [s for s in range(ne) if (cnt[ofs[r] + s] == 0).all()]
        assert whole == list(pd.C_SLOTS), (r, whole)
        # the order of the edge list survives the CSR build
        assert all(abs(int(src[ofs[r] + s]) - int(ref[r])) >= pd.FAR for s in pd.C_SLOTS)


def test_far_sources_only_give_a_zero_volume_in_case_d(dumps, passes):
    pd, _ = _scripts()
    d = dumps['default']
    ofs, src, ref = d['d_ofs'], d['d_src'], d['d_ref'].tolist()
    cnt = passes['d']
    _, _, D, plane = pd.CASES['d']
    var = d['d_f32'].view(np.uint32).reshape(len(ref), 32, D, *plane)
    r_fs, r_fo, r_or = (ref.index(pd.D_REFS[k]) for k in ('far_self', 'far_only', 'ordinary'))
    # [far, far, far, self]: three wholly skipped edges, then one that contributes everywhere
    assert src[ofs[r_fs]:ofs[r_fs + 1]].tolist() == [5, 6, 7, 0]
    assert [bool((cnt[ofs[r_fs] + s] == 0).all()) for s in range(4)] == [True, True, True, False]
    assert (cnt[ofs[r_fs] + 3] > 0).all() and var[r_fs].any()
    # far sources only and no self edge: every pass skipped, the count is still ne -> +0 everywhere, all bytes zero
    assert ofs[r_fo + 1] - ofs[r_fo] == 3
    assert all((cnt[ofs[r_fo] + s] == 0).all() for s in range(3))
    assert not var[r_fo].any()
    for kind in ('split', 'cl8'):                             # slots [n][4][2][D][h][w][16 bytes]
        assert not d['d_' + kind].reshape(len(ref), -1)[r_fo].any(), kind
    # the ordinary reference
    assert not any((cnt[ofs[r_or] + s] == 0).all() for s in range(5)) and var[r_or].any()


def test_dead_lanes_neither_block_nor_cause_a_skip_in_case_e(passes):
    """Plane grid 5 x 7 and D = 13: the last pixel tile has 3 pixels, the last plane chunk 5 planes.  Partly dead passes are among
    the skipped ones (dead lanes do not block a skip) and among the others (they do not cause one); the bits are compared by
    test_every_variant_gives_the_bits_of_the_kernel_that_never_skips."""
    cnt = passes['e']
    assert cnt.shape[1:] == (2, 5)
    ragged = np.zeros(cnt.shape, dtype=bool)
    ragged[:, -1, :] = True
    ragged[:, :, -1] = True
    assert ((cnt == 0) & ragged).any() and ((cnt > 0) & ragged).any()
    assert ((cnt == 0) & ~ragged).any() and ((cnt > 0) & ~ragged).any()


def test_case_a_against_the_pinned_oracle(dumps):
    pd, _ = _scripts()
    from oracle import pinned
    feat, R, tv, K, edges = pd.case_a()
    _, d0, D, plane = pd.CASES['a']
    var_o = pinned.warp_variance(feat, R, tv, K, edges, d0, pd.DD, D, pd.IMG, plane)
    n = var_o.shape[0]
    var = torch.from_numpy(dumps['default']['a_f32'].view(np.float32).copy()).view(n, 32, D, *plane)
    print('case a: max |var - oracle| = %.3g' % float((var - var_o).abs().max()))
    np.testing.assert_allclose(var.numpy(), var_o.numpy(), rtol=0, atol=VAR_ATOL)
