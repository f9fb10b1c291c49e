"""GPU: scene preparation (3dvnet_amd/preprocess.py -> csrc/prepare.hip, and the kernels of frames.hip, order_stats.hip, tsdf.hip,
mesh.hip behind ``gt_mesh_from_frames``).

``register_colour`` against the reference's recorded outputs (tests/golden/P_register_*.npz) and the NumPy checker
(tests/preprocess_oracle.py), which equals the reference bit for bit: compared for EQUALITY, no tolerance, no exempt pixel.  Every
output lies between two poisoned guard bands that must come back untouched.  ``convert_depth`` against NumPy indexing, exactly.
``gt_mesh_from_frames`` against the same steps called one by one through the public entry points (``dataset.frames_to_batch`` per
chunk, ``tsdf.volume_bounds``, ``TSDFFusion.integrate`` per view, ``get_tsdf().get_mesh()``), tensor for tensor: the glue is
checked without a new tolerance.  With ICL-NUIM's intrinsics (fy < 0) the fused volume is also held against the float64 checker of
tests/tsdf_oracle.py under the rules and bounds of tests/test_tsdf_gpu.py.

A zero third row of the homography: d = 0 + 1e-8f is then 1e-8, the coordinates are about 1e8 times the numerators -- finite where
the numerators are, and far outside the frame; a denominator of exactly zero (inf and NaN coordinates) needs H22 = -1e-8f.  Both
are run, and a NaN matrix: all three give zeros everywhere.

Measured on one MI355X: every byte comparison equal; the room of 7 frames fuses into 21 x 53 x 35 voxels of 8 cm and gives 2 746
vertices, all coloured, and 5 280 triangles on both bounds routes; with fy = -24 the uncertain share is 0.144 % of the touched voxels
(cap 0.5 %), no weight differs outside it, tsdf sum 9.78e-6 = 0.99 x the yardstick (bound 4 x), averaged tsdf 0.85 x, colour sums exact,
averaged colours 1.00 x; the end-to-end ICL-NUIM scene gives 503 vertices and 896 triangles, fscore 0.999999995.  Wall time of the
module's 18 tests: 3.7 s.
"""
import functools
import os

import numpy as np
import pytest
import torch

import preprocess_oracle as po
import tsdf_oracle as to
from conftest import v3d
from test_tsdf_oracle import ref_err

pytestmark = pytest.mark.gpu

GUARD = 512                     # bytes on either side of an output
POISON = 0xA5
SIZE, N_FRAMES, BATCH, VOX, MARGIN = (24, 32), 7, 3, 0.08, 0.3


@functools.lru_cache(maxsize=None)
def small(name):
    g = po.fixture(name)
    for a in g.values():
        a.setflags(write=False)
    return g


def guarded_bytes(nbytes, device, shift=0):
    """-> (whole uint8 buffer, the nbytes view handed to the call, its offset); `shift` moves the view off its alignment"""
    whole = torch.full((nbytes + 2 * GUARD + 16,), POISON, dtype=torch.uint8, device=device)
    start = GUARD + shift
    assert whole.data_ptr() % 16 == 0
    return whole, whole[start:start + nbytes], start


def assert_guards(whole, start, nbytes):
    torch.cuda.synchronize()
    assert bool((whole[:start] == POISON).all()) and bool((whole[start + nbytes:] == POISON).all()), 'a guard byte was written'


def run_register(cuda, colour, depth_size, K_color, K_depth, shift=0):
    """through a guarded output; the input must come back unchanged"""
    pre = v3d('preprocess')
    n, (h, w) = colour.shape[0], depth_size
    src = torch.from_numpy(np.array(colour)).to(cuda)
    whole, view, start = guarded_bytes(n * h * w * 3, cuda, shift)
    out = view.view(n, h, w, 3)
    got = pre.register_colour(src, (h, w), K_color, K_depth, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert_guards(whole, start, n * h * w * 3)
    assert np.array_equal(src.cpu().numpy(), colour), 'the input was written'
    return out.cpu().numpy()


# ---- register_colour ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', po.SMALL)
def test_register_equals_the_reference_byte_for_byte(cuda, name):
    """3 x (19 x 27): 7 threads a row, 399 threads = two workgroups, the last ragged, and a ragged last thread per row (byte
    stores); 12 x 16: the dword-store path; the tie case rounds half to even."""
    g = small(name)
    got = run_register(cuda, g['colour'], tuple(int(v) for v in g['depth_size']), g['K_color'], g['K_depth'])
    assert got.dtype == np.uint8 and got.tobytes() == g['expected'].tobytes(), \
        'first difference at %s' % (np.argwhere(got != g['expected'])[:1],)
    if name == 'register_tie':
        assert np.array_equal(got[0, 1, 1], g['colour'][0, 2, 2])


def test_register_full_size_frame_equals_the_checker(cuda):
    g = small('register_full_b')
    colour = po.random_colour(int(g['seed']), 1, 968, 1296)
    want, outside = po.register(colour, (480, 640), po.homography(g['K_color'], g['K_depth']))
    got = run_register(cuda, colour, (480, 640), g['K_color'], g['K_depth'])
    assert int(outside.sum()) == 2077 and not got[0][outside].any()
    assert got.tobytes() == want.tobytes() and po.sha256(got[0]) == str(g['sha256'])


def test_register_byte_path_gives_the_bytes_of_the_dword_path(cuda):
    g = small('register_aligned')
    args = (g['colour'], (12, 16), g['K_color'], g['K_depth'])
    aligned = run_register(cuda, *args)
    assert aligned.tobytes() == g['expected'].tobytes()
    assert run_register(cuda, *args, shift=1).tobytes() == aligned.tobytes()       # an output view one byte off


def test_register_batch_equals_single_frames_and_launches_repeat(cuda):
    for name in ('register_down2', 'register_aligned'):
        g = small(name)
        size = tuple(int(v) for v in g['depth_size'])
        whole = run_register(cuda, g['colour'], size, g['K_color'], g['K_depth'])
        for i in range(3):
            assert run_register(cuda, g['colour'][i:i + 1], size, g['K_color'], g['K_depth']).tobytes() == whole[i:i + 1].tobytes()
        for _ in range(9):
            assert run_register(cuda, g['colour'], size, g['K_color'], g['K_depth']).tobytes() == whole.tobytes()
    # a single frame without the batch axis
    pre = v3d('preprocess')
    one = pre.register_colour(torch.from_numpy(np.array(g['colour'][0])).to(cuda), size, g['K_color'], g['K_depth'])
    assert tuple(one.shape) == (1,) + size + (3,) and one.cpu().numpy().tobytes() == whole[:1].tobytes()


@pytest.mark.parametrize('third_row', [(0., 0., 0.), (0., 0., -1e-8), (np.nan, np.nan, np.nan)], ids=['zero', 'zero-denominator', 'nan'])
def test_register_degenerate_homography_returns_zeros(cuda, third_row):
    """K_depth = I, so H = float32(K_color): u >= 5, v >= 5 and the denominator is 1e-8, exactly 0, or a NaN"""
    g = small('register_down2')
    H = np.array([[2., 0., 5.], [0., 2., 5.], list(third_row)])
    want, outside = po.register(g['colour'], (19, 27), po.homography(H, np.eye(3)))
    assert outside.all() and not want.any()
    jx, _ = po.sample_positions(po.homography(H, np.eye(3)), 37, 53, 19, 27)
    assert np.isfinite(jx).all() == (third_row == (0., 0., 0.))
    got = run_register(cuda, g['colour'], (19, 27), H, np.eye(3))
    assert not got.any()


# ---- convert_depth --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['icl-nuim', 'tum-rgbd'])
def test_convert_depth_every_value_ragged_tail_and_unaligned_view(cuda, kind):
    pre = v3d('preprocess')
    lut = pre.depth_lut(kind)
    raw = np.concatenate((np.random.RandomState(3).permutation(65536), [1255, 0, 65535, 4, 1255])).astype(np.uint16)
    want = po.lut(kind)[raw]
    for shift in (0, 2):                                                           # 16-byte loads with a ragged tail; element by element
        src_whole, src_view, _ = guarded_bytes(raw.nbytes, cuda, shift)
        src = src_view.view(torch.int16)
        src.copy_(torch.from_numpy(raw.view(np.int16)))
        whole, view, start = guarded_bytes(raw.nbytes, cuda, shift)
        out = view.view(torch.int16)
        got = pre.convert_depth(src, lut, out=out)
        assert got.data_ptr() == out.data_ptr() and (got.data_ptr() % 16 == 0) == (shift == 0)
        assert_guards(whole, start, raw.nbytes)
        assert np.array_equal(src.cpu().numpy().view(np.uint16), raw), 'the input was written'
        assert np.array_equal(out.cpu().numpy().view(np.uint16), want)
    # a uint16 tensor of another shape, the anchor inputs in a slice of it
    frame = torch.from_numpy(np.arange(1200, 1200 + 6 * 16, dtype=np.uint16).reshape(6, 16).view(np.int16)).to(cuda).view(torch.uint16)
    got = pre.convert_depth(frame, lut)
    assert got.dtype == torch.uint16 and got.shape == (6, 16)
    got = got.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, po.lut(kind)[np.arange(1200, 1296).reshape(6, 16)])
    assert got[3, 7] == {'icl-nuim': 251, 'tum-rgbd': 250}[kind]                   # raw 1255


# ---- gt_mesh_from_frames --------------------------------------------------------------------------------------------------------

def by_hand(cuda, colour, depth_mm, K, poses, bounds='host', max_depth=None):
    """The reference's generate_gt_mesh step by step through the public entry points -> (mesh, fusion, what was integrated, the
    bounds)."""
    ds, tsdf = v3d('dataset'), v3d('tsdf')
    n = colour.shape[0]
    parts = []
    for start in range(0, n, BATCH):
        idx = np.arange(start, min(start + BATCH, n))
        batch = ds.frames_to_batch(colour[idx], depth_mm[idx], K, poses, idx, SIZE, SIZE, 1., (0., 0., 0.), (1., 1., 1.), 0, False, cuda)
        w2c = torch.eye(4).repeat(len(idx), 1, 1)
        w2c[:, :3, :3], w2c[:, :3, 3] = batch.rotmats.cpu(), batch.tvecs.cpu()
        parts.append((batch.images, batch.depth_images, batch.K.cpu(), w2c))
    depths = torch.cat([p[1] for p in parts])
    for_bounds = depths.clone()
    if max_depth is not None:
        for_bounds[for_bounds > max_depth] = 0.
    fn = tsdf.volume_bounds if bounds == 'host' else tsdf.volume_bounds_device
    origin, vol_max, dim = fn(for_bounds, torch.cat([p[2] for p in parts]), torch.cat([p[3] for p in parts]), .995, MARGIN, VOX, BATCH)
    fus = tsdf.TSDFFusion(dim, VOX, origin, 3, cuda, color=True)
    fed = []
    for images, d, K32, w2c in parts:
        P = tsdf.projection_matrices(K32, w2c)
        for i in range(d.shape[0]):
            fus.integrate(P[i], d[i], images[i])
        fed.append((P, d.cpu(), images.cpu()))
    return fus.get_tsdf().get_mesh(), fus, fed, (origin, vol_max, dim)


def assert_same_mesh(a, b):
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.triangles, b.triangles)
    assert torch.equal(a.vertex_colors_u8, b.vertex_colors_u8)


def run_gt_mesh(cuda, scene, **kw):
    return v3d('preprocess').gt_mesh_from_frames(*scene, img_batch=BATCH, vox_res=VOX, vol_margin=MARGIN, device=cuda, **kw)


@pytest.mark.parametrize('bounds', ['host', 'device'])
def test_gt_mesh_equals_the_steps_called_one_by_one(cuda, bounds):
    """7 frames of 24 x 32 in chunks of 3: three chunks, the last of one frame, and that frame all zero (an empty batch, skipped by
    the bounds and integrated as nothing)."""
    scene = po.room_frames(N_FRAMES, SIZE, zero_frame=6)
    assert (scene[1][6] == 0).all() and (scene[1][:6] > 0).mean() > 0.9
    want, fus, _, (_, _, dim) = by_hand(cuda, *scene, bounds=bounds)
    got = run_gt_mesh(cuda, scene, bounds=bounds)
    assert_same_mesh(got, want)
    assert got.vertices.is_cuda and got.vertices.dtype == torch.float32 and got.triangles.dtype == torch.int32
    n_v = got.vertices.shape[0]
    coloured = int((got.vertex_colors_u8 != 0).any(dim=1).sum())
    print('bounds=%s: volume %s, %d vertices, %d triangles, %d vertices with a colour' % (bounds, dim, n_v, got.triangles.shape[0], coloured))
    assert (N_FRAMES - 1) // BATCH + 1 >= 3 and n_v > 100 and got.triangles.shape[0] > 100 and coloured > 0.5 * n_v


def test_gt_mesh_max_depth_masks_the_bounds_only(cuda):
    scene = po.room_frames(N_FRAMES, SIZE, zero_frame=6, scale=1.6)
    seen = scene[1][scene[1] > 0]
    assert 0.05 < (seen > 4000).mean() < 0.95                                      # depths on both sides of 4 m
    want, _, fed, masked = by_hand(cuda, *scene, max_depth=4.)
    plain, _, fed_plain, unmasked = by_hand(cuda, *scene)
    print('bounds with max_depth=4: %s %s; without: %s %s' % (masked[0].tolist(), masked[2], unmasked[0].tolist(), unmasked[2]))
    assert not torch.equal(masked[0], unmasked[0]) or masked[2] != unmasked[2]
    assert all(torch.equal(a[1], b[1]) for a, b in zip(fed, fed_plain))            # what is integrated is not masked
    assert float(max(d.max() for _, d, _ in fed)) > 4.
    got = run_gt_mesh(cuda, scene, max_depth=4.)
    assert_same_mesh(got, want)
    assert got.vertices.shape[0] > 100
    assert got.vertices.shape != plain.vertices.shape or not torch.equal(got.vertices, plain.vertices)


def test_gt_mesh_with_a_negative_focal_length(cuda):
    """ICL-NUIM's intrinsics scaled to 24 x 32 (fy = -24): the glue as above, and the fused volume against the float64 checker under
    the two rules of tests/test_tsdf_gpu.py.  Yardstick as derived there for a case without a reference output: the reference's own
    error on fixture a (same room, same depth range, same voxel size and truncation margin) times n / 6 views."""
    from test_tsdf_gpu import compare
    pre = v3d('preprocess')
    K = pre.K_ICL_NUIM.copy()
    K[0] *= SIZE[1] / 640.
    K[1] *= SIZE[0] / 480.
    assert K[1, 1] == -24.0
    scene = po.room_frames(N_FRAMES, SIZE, zero_frame=6, K=K)
    want, fus, fed, (origin, _, dim) = by_hand(cuda, *scene)
    got = run_gt_mesh(cuda, scene)
    assert_same_mesh(got, want)
    assert got.vertices.shape[0] > 100
    P = torch.cat([f[0] for f in fed])
    assert bool((P[:, 1, :3].norm(dim=1) > 20).all())                              # the second row carries fy
    depths, images = torch.cat([f[1] for f in fed]), torch.cat([f[2] for f in fed])
    res = to.integrate(dim, VOX, origin.numpy(), VOX * 3, P.numpy(), depths.numpy(), images.numpy())
    ra = ref_err('a')
    n = N_FRAMES
    bounds = dict(tsdf=4 * ra['tsdf'] * n / 6, tsdf_avg=4 * ra['tsdf_avg'] * n / 6, color=0.0, color_avg=4 * ra['color_avg'])
    compare('negative focal length', res, fus, bounds)
    assert int((res['weight'] > 0).sum()) > 1000


# ---- process_scene_icl_nuim end to end -----------------------------------------------------------------------------------------

def test_process_scene_icl_nuim_end_to_end(cuda, tmp_path):
    """A raw ICL-NUIM scene whose images live in memory, real pixel functions: 5 frames of 24 x 32 seen through the reference's
    640 x 480 intrinsics (the top-left corner of the sensor: a narrow view of one wall)."""
    pre, mesh_mod, m3d = v3d('preprocess'), v3d('mesh'), v3d('metrics3d')
    syn = v3d('synthetic')
    scene = str(tmp_path / 'office_traj1')
    os.makedirs(scene)
    n = 5
    quats = np.array([[0.02 * i, 0.03, -0.01 * i, 1.0] for i in range(n)])
    centres = np.array([[3.0 + 0.05 * i, 2.5, 1.5 + 0.02 * i] for i in range(n)])
    R_fix = pre.FIX_POSE_R.astype(np.float64)
    tvecs_raw = centres @ R_fix                                                    # R_fix^T c: fix_pose puts the camera back at c
    poses = []
    for q, t in zip(quats, tvecs_raw):
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = pre.quat_to_matrix(q), t
        poses.append(pre.fix_pose(P))
    w2c = torch.from_numpy(np.linalg.inv(np.stack(poses))).float()
    K = torch.from_numpy(pre.K_ICL_NUIM).float()[None].repeat(n, 1, 1)
    depth_m = syn.ray_box_depth(w2c[:, :3, :3].contiguous(), w2c[:, :3, 3].contiguous(), K, SIZE, SIZE).numpy().astype(np.float64)
    assert np.isfinite(depth_m).all() and depth_m.min() > 0.5 and depth_m.max() < 13
    raw = np.rint(depth_m * 5000.).astype(np.uint16)
    files = po.MemoryFiles()
    with open(os.path.join(scene, 'associations.txt'), 'w') as f, open(os.path.join(scene, 'traj1.gt.freiburg'), 'w') as g:
        for i in range(n):
            f.write('%d depth/%d.png %d rgb/%d.png\n' % (i, i, i, i))
            g.write('%d %s %s\n' % (i, ' '.join(repr(float(v)) for v in tvecs_raw[i]), ' '.join(repr(float(v)) for v in quats[i])))
            files.files[os.path.join(scene, 'depth/%d.png' % i)] = raw[i]
            files.files[os.path.join(scene, 'rgb/%d.png' % i)] = np.random.RandomState(i).randint(1, 256, SIZE + (3,)).astype(np.uint8)
    kw = dict(img_batch=2, vox_res=0.02, vol_margin=0.2)
    io = dict(read_image=files.read_image, write_image=files.write_image, exists=files.exists)
    info = pre.process_scene_icl_nuim(scene, device=cuda, **io, **kw)
    assert len(info['frames']) == n
    lut = po.lut('icl-nuim')
    for i, frame in enumerate(info['frames']):
        written = files.files[frame['filename_depth']]
        assert written.dtype == np.uint16 and np.array_equal(written, lut[raw[i]])
        assert np.array_equal(frame['pose'], poses[i])
    in_memory = pre.generate_gt_mesh(scene, lambda fr: (files.files[fr['filename_color']], files.files[fr['filename_depth']]), device=cuda, **kw)
    on_disk = mesh_mod.read_triangle_mesh(info['gt_mesh'])
    n_v, n_f = in_memory.vertices.shape[0], in_memory.triangles.shape[0]
    print('gt_mesh.ply: %d vertices, %d triangles' % (n_v, n_f))
    assert n_v > 50 and n_f > 50
    assert on_disk.vertices.shape[0] == n_v and on_disk.triangles.shape[0] == n_f
    assert torch.equal(on_disk.triangles, in_memory.triangles.cpu()) and torch.equal(on_disk.vertices, in_memory.vertices.cpu())
    score = m3d.eval_mesh(on_disk, on_disk, device=cuda)
    print(score)
    assert abs(score['fscore'] - 1.0) <= 1e-7 and score['acc'] == 0.0 and score['comp'] == 0.0
