"""CPU: the host half of the scene-batch front end (3dvnet_amd/frameselector.py, 3dvnet_amd/dataset.py) against the reference's
recorded outputs (tests/golden/Dset_*.npz, written by tests/golden/make_golden_dataset.py), and the NumPy checker the GPU tests use
(tests/dataset_oracle.py) against stock torch on the CPU."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dataset_oracle as oracle
from conftest import ROOT, v3d

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DYADIC = [(480, 640, 256, 320, (0, 0)), (480, 640, 256, 320, (0, 20)), (480, 640, 240, 320, (0, 0)), (480, 640, 240, 320, (0, 20))]
ODD = [(37, 53, 16, 24, (0, 0)), (37, 53, 48, 64, (0, 0)), (37, 53, 15, 22, (3, 0))]
NEAREST = [(480, 256, 56), (640, 320, 56), (480, 256, 480), (640, 320, 640), (37, 16, 7), (53, 24, 9)]


# ---- selectors and PreprocessImage against the reference's recorded outputs ----------------------------------------------------------

def test_pose_walks_are_the_recorded_ones():
    z = np.load(os.path.join(GOLDEN, 'Dset_selectors.npz'))
    for w in oracle.WALKS:
        assert oracle.digest(oracle.pose_walk(w)) == str(z['sha_' + w])


@pytest.mark.parametrize('tag,cls,args', oracle.SELECTORS, ids=[s[0] for s in oracle.SELECTORS])
def test_selectors_equal_the_reference(tag, cls, args):
    fs = v3d('frameselector')
    z = np.load(os.path.join(GOLDEN, 'Dset_selectors.npz'))
    walks = {w: oracle.pose_walk(w) for w in oracle.WALKS}
    cases = [c for c in oracle.selector_cases() if c[2] == cls]
    assert len(cases) == 27
    lengths = set()
    for key, walk, _, _, n_frames, seed_idx, np_seed in cases:
        np.random.seed(np_seed)
        got = getattr(fs, cls)(*args).select_frames(walks[walk], n_frames, seed_idx)
        want = z[key]
        assert isinstance(got, np.ndarray) and got.dtype.kind == 'i' and got.shape == want.shape, (key, got, want)
        assert np.array_equal(got, want), (key, got.tolist(), want.tolist())
        lengths.add(len(want))
    assert len(lengths) > 2                                                       # early exits and full lengths both occur


def test_selector_fixtures_cover_the_early_exits():
    z = np.load(os.path.join(GOLDEN, 'Dset_selectors.npz'))
    assert z['short_best_10_0'].tolist() == [0, 5] and z['short_next_10_3'].tolist() == [3]    # sequence shorter than n_frames
    assert len(z['jumps_next_10_45']) < 10                                         # the walk runs off the end of the sequence
    assert z['jumps_next_100000_0'].tolist()[1:5] == [9, 18, 27, 36]               # a stall longer than search_interval = 8: forced steps
    assert z['gentle_range_4_none'][0] > 0 and z['gentle_nth_4_none'][0] > 0       # the random seed frame was drawn
    assert not np.array_equal(z['gentle_range_10_none'], z['gentle_range_10_0'])   # np.random.choice among the valid frames was drawn
    assert z['jumps_neucon_10_45'][0] == 45 and (np.diff(z['jumps_neucon_10_45']) < 0).any()   # np.roll wraps round


@pytest.mark.parametrize('key,H,W,nh,nw,crop', oracle.PREPROCESS_CASES, ids=[c[0] for c in oracle.PREPROCESS_CASES])
def test_preprocess_image_equals_the_reference(key, H, W, nh, nw, crop):
    ds = v3d('dataset')
    z = np.load(os.path.join(GOLDEN, 'Dset_preprocess.npz'))
    p = ds.PreprocessImage(K=oracle.intrinsics(H, W), old_width=W, old_height=H, new_width=nw, new_height=nh, distortion_crop=0,
                           perform_crop=crop)
    assert [p.crop_x, p.crop_y] == z[key + '_crop'].tolist()
    K = p.get_updated_intrinsics()
    assert K.dtype == np.float64 and K.tobytes() == z[key + '_K'].tobytes(), (K, z[key + '_K'])


def test_preprocess_fixtures_crop_both_ways():
    z = np.load(os.path.join(GOLDEN, 'Dset_preprocess.npz'))
    assert z['a_crop_crop'].tolist() == [20, 0] and z['e_portrait_crop'].tolist() == [0, 128] and z['c_crop_crop'].tolist() == [2, 0]


# ---- the package's tables against the checker's scalar loops, and the checker against torch ------------------------------------------

@pytest.mark.parametrize('H,W,oh,ow,crop', DYADIC + ODD)
def test_linear_tables_equal_the_checker(H, W, oh, ow, crop):
    ds = v3d('dataset')
    want = oracle.linear_tables(H, W, oh, ow, crop)
    got = ds.linear_axis(oh, H, crop[0]) + ds.linear_axis(ow, W, crop[1])
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes()
    y0, y1, wy, x0, x1, wx = want
    assert y0.min() >= crop[0] and y1.max() <= H - 1 - crop[0] and x0.min() >= crop[1] and x1.max() <= W - 1 - crop[1]
    assert (wy >= 0).all() and (wy < 1).all() and (wx >= 0).all() and (wx < 1).all()


def test_preprocess_image_hands_out_the_tables_of_its_crop():
    ds = v3d('dataset')
    p = ds.PreprocessImage(K=oracle.intrinsics(480, 640), old_width=640, old_height=480, new_width=320, new_height=256, perform_crop=True)
    assert (p.crop_x, p.crop_y) == (20, 0)
    for g, w in zip(p.linear_tables(), oracle.linear_tables(480, 640, 256, 320, (0, 20))):
        assert g.tobytes() == w.tobytes()
    for g, w in zip(p.nearest_tables((56, 56)), oracle.nearest_tables(480, 640, (256, 320), (56, 56), (0, 20))):
        assert g.dtype == np.int32 and g.tobytes() == w.tobytes()


def _torch_bilinear(frames, oh, ow, crop, dtype=np.float32):
    n, H, W, _ = frames.shape
    x = torch.from_numpy(frames[:, crop[0]:H - crop[0], crop[1]:W - crop[1]].astype(dtype)).permute(0, 3, 1, 2)
    return F.interpolate(x, (oh, ow), mode='bilinear', align_corners=False).numpy()


@pytest.mark.parametrize('H,W,oh,ow,crop', DYADIC)
def test_linear_resize_is_torch_bilinear_bit_for_bit_at_dyadic_scales(H, W, oh, ow, crop):
    frames = oracle.colour_frames(1, H, W, 5)
    v = oracle.blend64(frames, oracle.linear_tables(H, W, oh, ow, crop))
    assert np.array_equal(v, v.astype(np.float32).astype(np.float64))              # exact in fp32: the kernel's blend has no rounding here
    assert v.astype(np.float32).tobytes() == _torch_bilinear(frames, oh, ow, crop).tobytes()


@pytest.mark.parametrize('H,W,oh,ow,crop', ODD)
def test_linear_resize_is_torch_bilinear_at_odd_sizes(H, W, oh, ow, crop):
    """Against torch on float64 tensors, which computes its positions and weights in float64 as the tables do: what is left is the one
    rounding of each weight to fp32, 2^-25 of a weight below 1 times 255 grey levels, twice = 1.5e-5 at the very most.  (On float32
    tensors torch computes the positions in fp32 as well and is itself only good to some 1e-3 grey levels at these sizes.)"""
    frames = oracle.colour_frames(3, H, W, 6)
    v = oracle.blend64(frames, oracle.linear_tables(H, W, oh, ow, crop))
    err = np.abs(v - _torch_bilinear(frames, oh, ow, crop, np.float64)).max()
    print('%dx%d -> %dx%d crop %s: max |checker - torch| = %.3g grey levels' % (H, W, oh, ow, crop, err))
    assert err <= 1e-5


@pytest.mark.parametrize('src,mid,out', NEAREST)
@pytest.mark.parametrize('crop', [0, 3])
def test_composed_nearest_table_is_the_two_step_route(src, mid, out, crop):
    ds = v3d('dataset')
    n = src - 2 * crop
    first = np.minimum(np.floor(np.arange(mid) * (1.0 / (mid / n))).astype(np.int64), n - 1) + crop      # cv2.INTER_NEAREST, restated
    resized = torch.from_numpy(first.astype(np.float32)).view(1, 1, 1, mid)                             # the row index as the "image"
    two_step = F.interpolate(resized, (1, out), mode='nearest').view(-1).numpy().astype(np.int64)
    got = ds.nearest_axis(out, mid, src, crop)
    assert got.dtype == np.int32 and np.array_equal(got, two_step)
    assert np.array_equal(got, oracle.nearest_axis(out, mid, src, crop))
    assert got.min() >= crop and got.max() <= src - 1 - crop


@pytest.mark.parametrize('scale_rgb', [255., 1.])
def test_normalisation_chain_is_the_references_lines_in_torch(scale_rgb):
    levels = np.broadcast_to(np.arange(256, dtype=np.float32)[None, None, :, None], (1, 3, 256, 1)).copy()
    image = torch.from_numpy(levels[0].copy())
    image = image / 255.0                                                          # dataset.py:197
    image = (image * 255.0) / scale_rgb                                            # :202
    for c in range(3):                                                             # :203-205
        image[c, :, :] = (image[c, :, :] - oracle.MEAN[c]) / oracle.STD[c]
    got = oracle.chain32(levels, scale_rgb)
    assert got.dtype == np.float32 and got[0].tobytes() == image.numpy().tobytes()
    assert np.abs(oracle.chain64(levels, scale_rgb) - got).max() <= oracle.unquantised_bound(scale_rgb)


def test_depth_checker_applies_the_invalid_rule():
    mm = np.array([[[0, 65000, 65001, 65535, 1234]]], dtype=np.uint16)
    d = oracle.depths(mm, (np.zeros(1, np.int32), np.arange(5, dtype=np.int32)))
    assert d.dtype == np.float32 and d[0, 0].tolist() == [0.0, 65.0, 0.0, 0.0, float(np.float32(1234) / np.float32(1000))]
    frames = oracle.depth_frames(2, 30, 40, 1)
    for v in (0, 65000, 65001, 65535):
        assert (frames == v).reshape(2, -1).any(1).all()


# ---- the host half of a batch --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('k', [0, 1, 2])
def test_scene_geometry_equals_the_transcribed_reference(k):
    ds = v3d('dataset')
    poses = oracle.pose_walk('gentle')
    img_idx = np.arange(3, 3 + 2 * 7, 2)                                           # 7 frames
    geo = ds.scene_geometry(oracle.intrinsics(37, 53), poses, img_idx, (37, 53), (16, 24), False, k)
    ref_idx, edges, rotmats, tvecs = oracle.transcribed_geometry(poses, img_idx, k)
    assert np.array_equal(geo['ref_idx'], ref_idx) and len(ref_idx) == (7 - 2 * k if k else 0)
    assert geo['ref_src_edges'].dtype == torch.long and geo['ref_src_edges'].shape == edges.shape and torch.equal(geo['ref_src_edges'], edges)
    for name, want in (('rotmats', rotmats), ('tvecs', tvecs)):
        assert geo[name].dtype == torch.float32 and geo[name].numpy().tobytes() == want.numpy().tobytes()
    pre = ds.PreprocessImage(oracle.intrinsics(37, 53), 53, 37, 24, 16, 0, False)
    assert geo['K'].shape == (7, 3, 3) and geo['K'].dtype == torch.float32
    assert torch.equal(geo['K'][3], torch.from_numpy(pre.get_updated_intrinsics().astype(np.float32)))
    if k:
        assert edges.shape[1] == (7 - 2 * k) * (2 * k + 1) and edges[0].min() == k and edges[1].max() == 6


def test_augment_raises():
    ds, fs = v3d('dataset'), v3d('frameselector')
    with pytest.raises(NotImplementedError):
        ds.Dataset(['nowhere'], fs.EveryNthSelector(1), augment=True)
    d = ds.Dataset(['a', 'b'], fs.EveryNthSelector(1), 5, n_src_on_either_side=2)
    assert d.len() == 2 and len(d) == 2 and d.n_src_on_either_side == 2 and d.quantize is True


def test_default_reader_round_trips_png(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    ds = v3d('dataset')
    rgb = oracle.colour_frames(1, 5, 7, 3)[0]
    depth = np.array([[0, 1, 255, 256, 65000, 65001, 65535]] * 5, dtype=np.uint16)
    Image.fromarray(rgb).save(tmp_path / 'c.png')
    Image.fromarray(depth).save(tmp_path / 'd.png')
    info = {'filename_color': str(tmp_path / 'c.png'), 'filename_depth': str(tmp_path / 'd.png')}
    colour, got = ds.default_read_frame(info)
    assert colour.dtype == np.uint8 and colour.flags['C_CONTIGUOUS'] and np.array_equal(colour, rgb[:, :, ::-1])   # OpenCV's order
    assert got.dtype == np.uint16 and np.array_equal(got, depth)


def test_get_needs_the_library_before_it_reads_a_frame(tmp_path, monkeypatch):
    """No CPU path: without the library ``get`` fails through ``_lib``; with it, but without a device, at the first upload."""
    ds, fs, lib_mod = v3d('dataset'), v3d('frameselector'), v3d('_lib')
    poses = oracle.pose_walk('short')
    info = dict(intrinsics=oracle.intrinsics(37, 53).tolist(), frames=[dict(pose=p.tolist()) for p in poses])
    (tmp_path / 'info.json').write_text(json.dumps(info))
    read = []
    d = ds.Dataset([str(tmp_path)], fs.EveryNthSelector(1), read_frame=lambda f: read.append(f) or (None, None))
    monkeypatch.setattr(lib_mod, '_lib', None)
    monkeypatch.setattr(lib_mod, 'LIB_PATH', str(tmp_path / 'missing.so'))
    with pytest.raises(lib_mod.V3DLibraryError):
        d.get(0)
    assert read == []


def test_frame_entry_points_reject_bad_arguments_before_any_launch():
    """Host-side checks of include/v3d.h: they return before anything is enqueued, so they run without a device (the pointers
    are never followed)."""
    import ctypes
    lib_mod = v3d('_lib')
    lib = lib_mod.load()
    p = 4096                                                                       # any aligned non-null address
    mean, std = (ctypes.c_float * 3)(*oracle.MEAN), (ctypes.c_float * 3)(*oracle.STD)

    def images(frames=p, n=2, H=8, W=8, y0=p, oh=4, ow=4, scale=255., mean=mean, std=std, out=p):
        return lib.v3d_frames_to_images_f32(frames, n, H, W, y0, p, p, p, p, p, oh, ow, 1, scale, mean, std, out, None)

    def depths(mm=p, n=2, H=8, W=8, ys=p, oh=4, ow=4, out=p):
        return lib.v3d_frames_to_depths_f32(mm, n, H, W, ys, p, oh, ow, out, None)
    BAD_SHAPE, BAD_ARG = -1, -2
    assert images(frames=None) == BAD_ARG and b'null' in lib.v3d_last_error()
    assert images(out=None) == BAD_ARG and images(mean=None) == BAD_ARG and depths(mm=None) == BAD_ARG and depths(out=None) == BAD_ARG
    assert images(y0=p + 2) == BAD_ARG and images(out=p + 1) == BAD_ARG and depths(mm=p + 1) == BAD_ARG and depths(ys=p + 2) == BAD_ARG
    for bad in (dict(n=0), dict(H=0), dict(W=-1), dict(oh=0), dict(ow=-3)):
        assert images(**bad) == BAD_SHAPE and depths(**bad) == BAD_SHAPE, bad
    big = 2 ** 31 - 1
    assert images(n=big, oh=big, ow=big) == BAD_SHAPE and b'too many' in lib.v3d_last_error()
    assert depths(n=big, oh=big, ow=big) == BAD_SHAPE
    assert images(n=big, H=big, W=big) == BAD_SHAPE and depths(n=big, H=big, W=big) == BAD_SHAPE     # 3 n H W beyond 64-bit offsets
    assert images(n=4096, oh=4096, ow=4 * 2 ** 15 * 256) == BAD_SHAPE              # 2^24 rows x 2^23 threads = 2^31 workgroups exactly
    assert depths(n=4096, oh=4096, ow=2 ** 15 * 256) == BAD_SHAPE
    assert images(scale=0.) == BAD_ARG and images(scale=float('nan')) == BAD_ARG
    assert images(std=(ctypes.c_float * 3)(0.2, 0., 0.2)) == BAD_ARG and images(mean=(ctypes.c_float * 3)(0.2, float('inf'), 0.2)) == BAD_ARG
