"""CPU: the NumPy checker of the colour registration (tests/preprocess_oracle.py) against the reference's recorded outputs
(tests/golden/P_register_*.npz, written by tests/golden/make_golden_preprocess.py from the reference's own function), the host side
of 3dvnet_amd/preprocess.py (homography, the two depth tables, quaternions, fix_pose, the three scene drivers over a raw scene whose
images live in memory, with the pixel functions stubbed out), the host-side error codes of the two C entry points and the
no-fallback rule.

Recorded with the fixtures: the checker equals the reference with 0 mismatching pixels on every case; pixels that sample outside
the colour frame: down2 19, focal 198, skew 19 of 513; full size a 0, b 2 077 of 307 200.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import preprocess_oracle as po
from conftest import v3d


# ---- the checker against the reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', po.SMALL)
def test_checker_equals_the_reference_small(name):
    g = po.fixture(name)
    got, outside = po.register(g['colour'], tuple(g['depth_size']), po.homography(g['K_color'], g['K_depth']))
    assert got.dtype == np.uint8 and got.shape == g['expected'].shape
    assert np.array_equal(got, g['expected'])                                      # no tolerance, no exempt pixel
    assert int(outside.sum()) == int(g['outside'])
    assert not got[:, outside].any()                                               # zero padding
    assert int(g['outside']) == {'register_down2': 19, 'register_focal': 198, 'register_skew': 19}.get(name, 0)


def test_fixtures_cover_what_they_claim():
    skew = po.fixture('register_skew')
    assert (po.homography(skew['K_color'], skew['K_depth']) != 0).all()            # every term of H is used
    down = po.fixture('register_down2')
    _, outside = po.register(down['colour'], (19, 27), po.homography(down['K_color'], down['K_depth']))
    assert outside[:, -1].all() and not outside[:, :-1].any()                      # the last column, and nothing else
    tie = po.fixture('register_tie')
    jx, jy = po.sample_positions(po.homography(tie['K_color'], tie['K_depth']), 6, 6, 3, 3)
    H = po.homography(tie['K_color'], tie['K_depth'])
    assert np.array_equal(H, np.diag([3, 3, 1]).astype(np.float32))
    # pixel (1, 1): u = 3, ix = (3 / 3) * 2.5 = 2.5 exactly -> 2 (half to even), not 3
    assert jx[1, 1] == 2 and jy[1, 1] == 2
    assert np.array_equal(tie['expected'][0, 1, 1], tie['colour'][0, 2, 2])
    assert not np.array_equal(tie['colour'][0, 2, 2], tie['colour'][0, 3, 3])


@pytest.mark.parametrize('name', po.FULL)
def test_checker_equals_the_reference_full_size(name):
    g = po.fixture(name)
    Hc, Wc = (int(v) for v in g['colour_size'])
    colour = po.random_colour(int(g['seed']), 1, Hc, Wc)
    got, outside = po.register(colour[0], tuple(int(v) for v in g['depth_size']), po.homography(g['K_color'], g['K_depth']))
    assert int(outside.sum()) == int(g['outside']) == {'register_full_a': 0, 'register_full_b': 2077}[name]
    assert po.sha256(got) == str(g['sha256'])


def test_both_forms_of_the_unnormalisation_agree():
    """(g + 1) * ((S - 1) / 2), ATen's CPU form, and ((g + 1) / 2) * (S - 1), its device form, round to the same pixel on the
    fixtures' geometry."""
    F = np.float32
    for name in po.SMALL:
        g = po.fixture(name)
        Hc, Wc = g['colour'].shape[1:3]
        h, w = (int(v) for v in g['depth_size'])
        H = po.homography(g['K_color'], g['K_depth'])
        jx, jy = po.sample_positions(H, Hc, Wc, h, w)
        x = np.arange(w, dtype=F)[None, :].repeat(h, 0)
        y = np.arange(h, dtype=F)[:, None].repeat(w, 1)
        d = ((H[2, 0] * x + H[2, 1] * y) + H[2, 2]) + F(1e-8)
        u = ((H[0, 0] * x + H[0, 1] * y) + H[0, 2]) / d
        gx = (u - F(Wc / 2.0)) / F(Wc / 2.0)
        assert np.array_equal(np.rint(((gx + F(1)) / F(2)) * F(Wc - 1)), jx), name


def test_homography_is_the_float64_product_cast_once():
    pre = v3d('preprocess')
    for name in po.SMALL + po.FULL:
        g = po.fixture(name)
        H = pre.colour_to_depth_homography(g['K_color'], g['K_depth'])
        want = g['K_color'].astype(np.float64).dot(np.linalg.inv(g['K_depth'].astype(np.float64))).astype(np.float32)
        assert H.dtype == np.float32 and H.shape == (3, 3) and H.tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        pre.colour_to_depth_homography(np.eye(4), np.eye(3))


# ---- depth tables, quaternions, fix_pose ----------------------------------------------------------------------------------------

def test_depth_luts_are_the_references_expressions():
    pre = v3d('preprocess')
    icl, tum = pre.depth_lut('icl-nuim'), pre.depth_lut('tum-rgbd')
    for got, kind in ((icl, 'icl-nuim'), (tum, 'tum-rgbd')):
        assert got.dtype == np.uint16 and got.shape == (65536,) and np.array_equal(got, po.lut(kind))
    floor5 = (np.arange(65536) // 5).astype(np.uint16)
    assert int((icl != tum).sum()) == 144 and int((icl != floor5).sum()) == 95 and int((tum != floor5).sum()) == 91
    assert icl[1255] == 251 and tum[1255] == 250
    with pytest.raises(ValueError):
        pre.depth_lut('scannet')


def test_quat_to_matrix_against_scipy():
    pre = v3d('preprocess')
    g = po.fixture('quat')
    norms = np.linalg.norm(g['q'], axis=1)
    assert (np.abs(norms - 1) > 0.1).sum() >= 4 and (np.abs(norms - 1) < 1e-12).sum() >= 4
    got = pre.quat_to_matrix(g['q'])
    err = np.abs(got - g['matrices']).max()
    print('largest difference from SciPy: %.3g' % err)
    assert got.dtype == np.float64 and got.shape == (16, 3, 3) and err <= 1e-15
    assert np.array_equal(pre.quat_to_matrix(g['q'][3]), got[3])                   # a single quaternion -> [3, 3]
    assert np.isnan(pre.quat_to_matrix([np.nan, 0, 0, 1])).any()
    with pytest.raises(ValueError):
        pre.quat_to_matrix([0, 0, 0, 0])


def test_fix_pose_constants():
    pre = v3d('preprocess')
    c = np.float32(np.cos(np.float64(np.float32(np.pi / 2))))
    assert c == np.float32(-4.371139e-08) and pre.FIX_POSE_COS == c and pre.FIX_POSE_COS.dtype == np.float32
    assert pre.FIX_POSE_R.dtype == np.float32
    assert np.array_equal(pre.FIX_POSE_R, np.array([[1, 0, 0], [0, c, -1], [0, 1, c]], dtype=np.float32))
    P = np.eye(4)
    P[:3, 3] = (1., 2., 3.)
    got = pre.fix_pose(P)
    assert got.dtype == np.float64 and np.array_equal(got[3], [0, 0, 0, 1])
    assert np.array_equal(got[:3, 3], pre.FIX_POSE_R.astype(np.float64) @ np.array([1., 2., 3.]))
    assert np.array_equal(pre.K_ICL_NUIM, [[481.20, 0, 319.50], [0, -480.00, 239.50], [0, 0, 1]])
    assert np.array_equal(pre.K_TUM_RGBD, [[525.0, 0, 320.0], [0, 525.0, 240.0], [0, 0, 1]])


def test_closest_index_takes_the_first_of_ties_and_ignores_order():
    pre = v3d('preprocess')
    stamps = np.array([5.0, 1.0, 3.0, 9.0, 3.0])                                   # unsorted, with a gap and a repeat
    assert pre.get_closest_index(2.0, stamps) == 1                                 # 1.0 and 3.0 equally close: the first
    assert pre.get_closest_index(3.0, stamps) == 2 and pre.get_closest_index(100.0, stamps) == 3
    assert pre.get_closest_index(7.0, stamps) == 0                                 # 5.0 and 9.0: the first


# ---- scene drivers --------------------------------------------------------------------------------------------------------------

class Stubs:
    """the pixel functions replaced by recorders: the drivers' host halves run without a device"""

    def __init__(self, monkeypatch, pre):
        self.registered, self.converted, self.meshes = [], [], []
        monkeypatch.setattr(pre, '_dataset', type('D', (), {'_upload': staticmethod(lambda a, dev: torch.from_numpy(np.array(a).view(np.int16) if a.dtype == np.uint16 else np.array(a))),
                                                            '_device': staticmethod(lambda d: 'stub'),
                                                            'default_read_frame': None}))

        def register_colour(colour, depth_size, K_color, K_depth, out=None):
            self.registered.append((tuple(colour.shape), tuple(depth_size), np.array(K_color), np.array(K_depth)))
            return torch.full((1,) + tuple(depth_size) + (3,), 7, dtype=torch.uint8)

        def convert_depth(depth_raw, lut, out=None):
            self.converted.append(np.array(lut))
            return torch.from_numpy(np.asarray(lut).view(np.int16)[depth_raw.numpy().view(np.uint16).astype(np.int64)])

        class Mesh:
            def write_ply(_, path):
                with open(path, 'w') as f:
                    f.write('mesh %d' % len(self.meshes))

        def generate_gt_mesh(scene_dir, read_frame=None, **kw):
            self.meshes.append((scene_dir, read_frame, kw))
            return Mesh()
        monkeypatch.setattr(pre, 'register_colour', register_colour)
        monkeypatch.setattr(pre, 'convert_depth', convert_depth)
        monkeypatch.setattr(pre, 'generate_gt_mesh', generate_gt_mesh)


def _touch(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    open(path, 'w').close()


def test_process_scene_scannet(tmp_path, monkeypatch):
    pre = v3d('preprocess')
    stubs = Stubs(monkeypatch, pre)
    src, dst = str(tmp_path / 'src' / 'scene0000_00'), str(tmp_path / 'dst' / 'scene0000_00')
    Kc, Kd = (po.kmat(*v) for v in po.SCANNET_PAIRS['a'])
    os.makedirs(os.path.join(src, 'intrinsic'))
    os.makedirs(os.path.join(src, 'pose'))
    for name, K in (('intrinsic_color.txt', Kc), ('intrinsic_depth.txt', Kd)):
        K4 = np.eye(4)
        K4[:3, :3] = K
        np.savetxt(os.path.join(src, 'intrinsic', name), K4)
    with open(os.path.join(src, 'scene0000_00_vh_clean_2.ply'), 'w') as f:
        f.write('the mesh')
    files = po.MemoryFiles()
    ids = [0, 2, 10, 100, 1234567]                                                 # listed as strings they would sort 0, 10, 100, ...
    poses = {}
    for i in ids:
        _touch(os.path.join(src, 'color', '%d.jpg' % i))
        files.files[os.path.join(src, 'color', '%d.jpg' % i)] = np.full((8, 12, 3), i % 251, dtype=np.uint8)
        files.files[os.path.join(src, 'depth', '%d.png' % i)] = np.full((4, 6), i % 65521, dtype=np.uint16)
        poses[i] = np.eye(4) + i
        if i == 10:
            poses[i][1, 3] = -np.inf                                               # an invalid pose: the frame is skipped
        np.savetxt(os.path.join(src, 'pose', '%d.txt' % i), poses[i])
    _touch(os.path.join(src, 'color', 'notes.txt'))
    data = pre.process_scene_scannet(src, dst, read_image=files.read_image, write_image=files.write_image, exists=files.exists)
    with open(os.path.join(dst, 'info.json')) as f:
        info = json.load(f)
    assert info == data and list(info) == ['scene', 'path', 'frames', 'gt_mesh', 'intrinsics']
    assert info['scene'] == 'scene0000_00' and info['path'] == dst and np.array_equal(info['intrinsics'], Kd)
    assert info['gt_mesh'] == os.path.join(dst, 'scene0000_00_vh_clean_2.ply') and open(info['gt_mesh']).read() == 'the mesh'
    kept = [0, 2, 100, 1234567]
    # the reference pads the WHOLE name to nine characters: '0.jpg' -> '00000.jpg', and a long id is left alone
    names = ['00000', '00002', '00100', '1234567']
    assert [os.path.basename(f['filename_color']) for f in info['frames']] == [n + '.jpg' for n in names]
    assert [os.path.basename(f['filename_depth']) for f in info['frames']] == [n + '.png' for n in names]
    assert all(list(f) == ['filename_color', 'filename_depth', 'pose'] for f in info['frames'])
    for f, i in zip(info['frames'], kept):
        assert os.path.dirname(f['filename_color']) == os.path.join(dst, 'color') and np.array_equal(f['pose'], poses[i])
        assert (files.files[f['filename_color']] == 7).all() and files.files[f['filename_color']].shape == (4, 6, 3)
        assert np.array_equal(files.files[f['filename_depth']], files.files[os.path.join(src, 'depth', '%d.png' % i)])
    assert len(stubs.registered) == 4
    shape, size, K1, K2 = stubs.registered[0]
    assert shape == (8, 12, 3) and size == (4, 6) and np.array_equal(K1, Kc) and np.array_equal(K2, Kd)
    # a second run rewrites the registered colour frames (as the reference does) and leaves the depth frames that exist
    files.writes.clear()
    pre.process_scene_scannet(src, dst, read_image=files.read_image, write_image=files.write_image, exists=files.exists)
    assert sorted(files.writes) == sorted(f['filename_color'] for f in info['frames'])


def test_process_scene_scannet_does_not_register_frames_of_the_depth_size(tmp_path, monkeypatch):
    pre = v3d('preprocess')
    stubs = Stubs(monkeypatch, pre)
    src, dst = str(tmp_path / 'scene0001_00'), str(tmp_path / 'out')
    os.makedirs(os.path.join(src, 'intrinsic'))
    os.makedirs(os.path.join(src, 'pose'))
    for name in ('intrinsic_color.txt', 'intrinsic_depth.txt'):
        np.savetxt(os.path.join(src, 'intrinsic', name), np.eye(4))
    _touch(os.path.join(src, 'scene0001_00_vh_clean_2.ply'))
    _touch(os.path.join(src, 'color', '3.jpg'))
    np.savetxt(os.path.join(src, 'pose', '3.txt'), np.eye(4))
    colour = np.arange(4 * 6 * 3, dtype=np.uint8).reshape(4, 6, 3)
    files = po.MemoryFiles({os.path.join(src, 'color', '3.jpg'): colour, os.path.join(src, 'depth', '3.png'): np.ones((4, 6), dtype=np.uint16)})
    pre.process_scene_scannet(src, dst, read_image=files.read_image, write_image=files.write_image, exists=files.exists)
    assert stubs.registered == [] and np.array_equal(files.files[os.path.join(dst, 'color', '00003.jpg')], colour)
    files.writes.clear()
    pre.process_scene_scannet(src, dst, read_image=files.read_image, write_image=files.write_image, exists=files.exists)
    assert files.writes == []                                                      # both files exist: nothing is written again


def _icl_scene(tmp_path):
    scene = str(tmp_path / 'living_room_traj0')
    os.makedirs(scene)
    quats = {1: (0, 0, 0, 1), 2: (0, 0, 2, 2), 3: (np.nan, 0, 0, 1), 5: (1, 0, 0, 0)}          # frame 3: invalid; frame 4: no pose
    with open(os.path.join(scene, 'associations.txt'), 'w') as f:
        for i in (1, 2, 3, 4, 5):
            f.write('%d depth/%d.png %d rgb/%d.png\n' % (i, i, i, i))
    with open(os.path.join(scene, 'traj0.gt.freiburg'), 'w') as f:
        for i, q in quats.items():
            f.write('%d %g %g %g %s\n' % (i, 0.1 * i, 0.2 * i, 0.3 * i, ' '.join(repr(float(v)) for v in q)))
    files = po.MemoryFiles()
    for i in (1, 2, 3, 4, 5):
        files.files[os.path.join(scene, 'depth/%d.png' % i)] = (np.arange(24, dtype=np.uint16).reshape(4, 6) * 251 + 1255 * i).astype(np.uint16)
        files.files[os.path.join(scene, 'rgb/%d.png' % i)] = np.full((4, 6, 3), i, dtype=np.uint8)
    return scene, quats, files


def test_process_scene_icl_nuim(tmp_path, monkeypatch):
    pre = v3d('preprocess')
    stubs = Stubs(monkeypatch, pre)
    scene, quats, files = _icl_scene(tmp_path)
    io = dict(read_image=files.read_image, write_image=files.write_image, exists=files.exists)
    data = pre.process_scene_icl_nuim(scene, vox_res=0.08, **io)
    with open(os.path.join(scene, 'info.json')) as f:
        info = json.load(f)
    assert info == data and list(info) == ['scene', 'path', 'intrinsics', 'gt_mesh', 'frames']
    assert info['scene'] == 'living_room_traj0' and info['path'] == scene and info['gt_mesh'] == os.path.join(scene, 'gt_mesh.ply')
    assert np.array_equal(info['intrinsics'], pre.K_ICL_NUIM) and info['intrinsics'][1][1] == -480.0
    assert [os.path.basename(f['filename_depth']) for f in info['frames']] == ['1.png', '2.png', '5.png']
    lut = po.lut('icl-nuim')
    for f, i in zip(info['frames'], (1, 2, 5)):
        assert f['filename_color'] == os.path.join(scene, 'rgb/%d.png' % i)
        assert f['filename_depth'] == os.path.join(scene, 'depth_processed', '%d.png' % i)
        P = np.eye(4)
        P[:3, :3] = pre.quat_to_matrix(quats[i])
        P[:3, 3] = (0.1 * i, 0.2 * i, 0.3 * i)
        assert np.array_equal(f['pose'], pre.fix_pose(P))
        got = files.files[f['filename_depth']]
        assert got.dtype == np.uint16 and np.array_equal(got, lut[files.files[os.path.join(scene, 'depth/%d.png' % i)]])
    assert all(np.array_equal(t, lut) for t in stubs.converted) and len(stubs.converted) == 3
    assert open(info['gt_mesh']).read() == 'mesh 1' and stubs.meshes[0][0] == scene and stubs.meshes[0][2] == {'vox_res': 0.08}
    colour, depth = stubs.meshes[0][1](info['frames'][1])                          # the mesh pass reads through read_image
    assert (colour == 2).all() and np.array_equal(depth, files.files[info['frames'][1]['filename_depth']])
    # again: nothing is converted, no mesh is made; the flags bring each back
    files.writes.clear()
    pre.process_scene_icl_nuim(scene, **io)
    assert files.writes == [] and len(stubs.meshes) == 1 and len(stubs.converted) == 3
    pre.process_scene_icl_nuim(scene, overwrite_depth=True, **io)
    assert len(files.writes) == 3 and len(stubs.meshes) == 1
    pre.process_scene_icl_nuim(scene, overwrite_mesh=True, **io)
    assert len(files.writes) == 3 and len(stubs.meshes) == 2 and open(info['gt_mesh']).read() == 'mesh 2'


def test_process_scene_tum_rgbd(tmp_path, monkeypatch):
    pre = v3d('preprocess')
    stubs = Stubs(monkeypatch, pre)
    scene = str(tmp_path / 'rgbd_dataset_freiburg1_desk')
    depth_t, rgb_t = [10.00, 10.10, 10.40], [10.30, 9.95, 10.05, 10.15]            # rgb.txt need not be sorted
    pose_t = [9.0, 10.05, 10.15, 12.0]
    files = po.MemoryFiles()
    for t in depth_t:
        _touch(os.path.join(scene, 'depth', '%.2f.png' % t))
        files.files[os.path.join(scene, 'depth', '%.2f.png' % t)] = np.array([[0, 1255, 5000], [65535, 4, 5]], dtype=np.uint16)
    for t in sorted(rgb_t):
        _touch(os.path.join(scene, 'rgb', '%.2f.png' % t))
    for name, stamps in (('depth.txt', depth_t), ('rgb.txt', rgb_t)):
        with open(os.path.join(scene, name), 'w') as f:
            f.write('# timestamp filename\n' + ''.join('%.2f x/%.2f.png\n' % (t, t) for t in stamps))
    rng = np.random.RandomState(3)
    gt = np.concatenate((np.array(pose_t)[:, None], rng.randn(4, 3), rng.randn(4, 4)), axis=1)
    np.savetxt(os.path.join(scene, 'groundtruth.txt'), gt, header='timestamp tx ty tz qx qy qz qw')
    gt = np.loadtxt(os.path.join(scene, 'groundtruth.txt'))
    io = dict(read_image=files.read_image, write_image=files.write_image, exists=files.exists)
    data = pre.process_scene_tum_rgbd(scene, **io)
    with open(os.path.join(scene, 'info.json')) as f:
        info = json.load(f)
    assert info == data and list(info) == ['scene', 'path', 'intrinsics', 'gt_mesh', 'frames']
    assert np.array_equal(info['intrinsics'], pre.K_TUM_RGBD) and info['gt_mesh'] == os.path.join(scene, 'gt_mesh.ply')
    # depth 10.00: poses 10.05 (|.05|); rgb 9.95 and 10.05 are equally close up to rounding -> whichever argmin takes in float64;
    # depth 10.10: poses 10.05 / 10.15 tie -> the first (up to rounding); depth 10.40: pose 10.15, rgb 10.30.  The sorted FILE LIST is
    # indexed with the position in rgb.txt, as the reference does.
    image_files = sorted(os.path.join(scene, 'rgb', '%.2f.png' % t) for t in rgb_t)
    for f, t in zip(info['frames'], depth_t):
        pi = int(np.argmin(np.abs(np.array(pose_t) - t)))
        ii = int(np.argmin(np.abs(np.array(rgb_t) - t)))
        assert f['filename_color'] == image_files[ii]
        assert f['filename_depth'] == os.path.join(scene, 'depth_processed', '%.2f.png' % t)
        P = np.eye(4)
        P[:3, :3] = pre.quat_to_matrix(gt[pi, 4:])
        P[:3, 3] = gt[pi, 1:4]
        assert np.array_equal(f['pose'], P)
        assert np.array_equal(files.files[f['filename_depth']], po.lut('tum-rgbd')[np.array([[0, 1255, 5000], [65535, 4, 5]])])
    assert files.files[info['frames'][0]['filename_depth']][0, 1] == 250          # the float32 table
    assert info['frames'][2]['filename_color'] == image_files[0]                  # position 0 of rgb.txt (10.30) -> the first FILE
    assert len(stubs.meshes) == 1 and stubs.meshes[0][2] == {}
    files.writes.clear()
    pre.process_scene_tum_rgbd(scene, **io)
    assert files.writes == [] and len(stubs.meshes) == 1
    pre.process_scene_tum_rgbd(scene, overwrite_depth=True, overwrite_mesh=True, **io)
    assert len(files.writes) == 3 and len(stubs.meshes) == 2


# ---- the C entry points on the host ---------------------------------------------------------------------------------------------

def test_error_codes_of_the_entry_points():
    lib = v3d('_lib').load()
    BAD_SHAPE, BAD_ARG = -1, -2
    p = ctypes.c_void_p(4096)          # never dereferenced: every call below returns before any launch
    H = (ctypes.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1)
    reg = lib.v3d_register_colour_u8
    assert reg(None, 1, 8, 8, H, 4, 4, p, None) == BAD_ARG and b'null' in lib.v3d_last_error()
    assert reg(p, 1, 8, 8, None, 4, 4, p, None) == BAD_ARG and b'v3d_register_colour_u8' in lib.v3d_last_error()
    assert reg(p, 1, 8, 8, H, 4, 4, None, None) == BAD_ARG
    for bad in ((0, 8, 8, 4, 4), (1, 0, 8, 4, 4), (1, 8, -3, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, 0)):
        n, Hc, Wc, h, w = bad
        assert reg(p, n, Hc, Wc, H, h, w, p, None) == BAD_SHAPE and b'positive' in lib.v3d_last_error(), bad
    big = 2 ** 31 - 1
    assert reg(p, big, 8, 8, H, big, 1024, p, None) == BAD_SHAPE and b'too many for one launch' in lib.v3d_last_error()
    assert reg(p, big, big, big, H, 4, 4, p, None) == BAD_SHAPE and b'frame pixels' in lib.v3d_last_error()
    lut = lib.v3d_lut_u16
    assert lut(None, 8, p, p, None) == BAD_ARG and b'null' in lib.v3d_last_error()
    assert lut(p, 8, None, p, None) == BAD_ARG and lut(p, 8, p, None, None) == BAD_ARG
    assert lut(p, 8, ctypes.c_void_p(4097), p, None) == BAD_ARG and b'aligned' in lib.v3d_last_error()      # a misaligned lut
    assert lut(ctypes.c_void_p(4097), 8, p, p, None) == BAD_ARG and lut(p, 8, p, ctypes.c_void_p(4099), None) == BAD_ARG
    assert lut(p, 0, p, p, None) == BAD_SHAPE and b'positive' in lib.v3d_last_error()
    assert lut(p, 2 ** 31 * 256 * 8, p, p, None) == BAD_SHAPE and b'workgroups' in lib.v3d_last_error()     # 16-byte aligned: 8 a thread
    assert lut(ctypes.c_void_p(4098), 2 ** 31 * 256, p, p, None) == BAD_SHAPE                               # unaligned: 1 a thread


def test_no_cpu_fallback(monkeypatch):
    pre, lib_mod = v3d('preprocess'), v3d('_lib')
    K = np.eye(3)
    if not torch.cuda.is_available():
        with pytest.raises(lib_mod.V3DLibraryError):
            pre.register_colour(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), (2, 2), K, K)
        with pytest.raises(lib_mod.V3DLibraryError):
            pre.convert_depth(torch.zeros((2, 2), dtype=torch.int16), pre.depth_lut('icl-nuim'))
        with pytest.raises(lib_mod.V3DLibraryError):
            pre.gt_mesh_from_frames(np.zeros((1, 4, 4, 3), dtype=np.uint8), np.ones((1, 4, 4), dtype=np.uint16), K, np.eye(4)[None])
    # without the library: every pixel function fails before any work
    monkeypatch.setattr(lib_mod, '_lib', None)
    monkeypatch.setattr(lib_mod, 'LIB_PATH', lib_mod.LIB_PATH + '.missing')
    with pytest.raises(lib_mod.V3DLibraryError, match='not found'):
        pre.register_colour(torch.zeros((1, 4, 4, 3), dtype=torch.uint8), (2, 2), K, K)
    with pytest.raises(lib_mod.V3DLibraryError, match='not found'):
        pre.convert_depth(torch.zeros((2, 2), dtype=torch.int16), pre.depth_lut('tum-rgbd'))
    with pytest.raises(lib_mod.V3DLibraryError, match='not found'):
        pre.gt_mesh_from_frames(np.zeros((1, 4, 4, 3), dtype=np.uint8), np.ones((1, 4, 4), dtype=np.uint16), K, np.eye(4)[None])
    with pytest.raises(lib_mod.V3DLibraryError, match='not found'):
        pre.generate_gt_mesh('/nonexistent')
