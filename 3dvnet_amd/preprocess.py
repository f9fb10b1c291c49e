"""Raw ScanNet, ICL-NUIM and TUM RGB-D scenes -> prepared scene folders: counterpart of ``data_preprocess/preprocess_scannet.py``,
``preprocess_icl_nuim.py`` and ``preprocess_tum_rgbd.py``.

A prepared scene folder is what every other path of the package starts from: an ``info.json`` whose colour frames have the depth
frames' size, whose depth frames are 16-bit millimetres and whose ``gt_mesh`` entry names a mesh file.  The host does what is
sequential or tiny -- file lists, timestamps, quaternions, poses, ``info.json``, all in the reference's number types -- and the
device does the pixels and the fusion:

    colour_to_depth_homography   K_color K_depth^-1 in float64, cast once (preprocess_scannet.py:48-49)
    register_colour              a colour frame resampled into the depth camera (csrc/prepare.hip: v3d_register_colour_u8)
    depth_lut / convert_depth    the depth-unit conversion of the TUM-format datasets as a 65 536-entry table (v3d_lut_u16)
    gt_mesh_from_frames          every sensor depth frame of a scene fused into a TSDF, the mesh extracted (``generate_gt_mesh`` of
                                 the two TUM-format scripts) with the kernels of frames.hip, order_stats.hip, tsdf.hip and mesh.hip
    generate_gt_mesh             the same over a prepared scene folder
    process_scene_scannet / process_scene_icl_nuim / process_scene_tum_rgbd     the three scripts' ``process_scene``
    quat_to_matrix               ``scipy.spatial.transform.Rotation.from_quat(q).as_matrix()`` restated (SciPy is not a dependency)

There is no CPU path for the pixels: without the library or a HIP device ``register_colour``, ``convert_depth`` and
``gt_mesh_from_frames`` raise ``V3DLibraryError``.  Image files are decoded and encoded on the host (``read_image`` /
``write_image``: OpenCV, else Pillow, or the caller's).  Not built: the scene lists of ``mv3d/dsets/scenelists.py`` (folder names:
the caller passes scene folders).
"""
import glob
import json
import os
import shutil
import time

import numpy as np
import torch

from . import _lib
from . import dataset as _dataset
from . import tsdf as _tsdf

# the reference's intrinsics (preprocess_icl_nuim.py:18-20, https://www.doc.ic.ac.uk/~ahanda/VaFRIC/codes.html: fy is negative;
# preprocess_tum_rgbd.py:17-19)
K_ICL_NUIM = np.array([[481.20, 0, 319.50],
                       [0, -480.00, 239.50],
                       [0, 0, 1]])
K_TUM_RGBD = np.array([[525.0, 0.0, 320.0],
                       [0.0, 525.0, 240.0],
                       [0.0, 0.0, 1.0]])
IMG_BATCH, VOX_RES, VOL_PRCNT, VOL_MARGIN, TRUNC_RATIO = 20, 0.02, .995, 1.5, 3

# fix_pose (preprocess_icl_nuim.py:64-72): the matrix cv2.Rodrigues gives for the float32 rotation vector (pi / 2, 0, 0), cast to
# float32 -- cos(theta) I + (1 - cos(theta)) r r^T + sin(theta) [r]x with r = (1, 0, 0), evaluated in float64 on theta =
# float32(pi / 2).  Restated from the definition: OpenCV is not a dependency.
_FIX_THETA = np.float64(np.float32((1. / 2.) * np.pi))
FIX_POSE_COS = np.float32(np.cos(_FIX_THETA))                    # -4.371139e-08
FIX_POSE_SIN = np.float32(np.sin(_FIX_THETA))                    # 1
FIX_POSE_R = np.array([[1, 0, 0],
                       [0, FIX_POSE_COS, -FIX_POSE_SIN],
                       [0, FIX_POSE_SIN, FIX_POSE_COS]], dtype=np.float32)


# ---- pixels ---------------------------------------------------------------------------------------------------------------------

def colour_to_depth_homography(K_color, K_depth):
    """-> fp32 [3, 3]: ``K_color . inv(K_depth)`` in float64 with ``np.linalg.inv``, cast once, as the reference forms it."""
    K_color, K_depth = np.asarray(K_color, dtype=np.float64), np.asarray(K_depth, dtype=np.float64)
    if K_color.shape != (3, 3) or K_depth.shape != (3, 3):
        raise ValueError('colour_to_depth_homography: two [3, 3] matrices expected, got %s and %s' % (K_color.shape, K_depth.shape))
    return K_color.dot(np.linalg.inv(K_depth)).astype(np.float32)


def _on_device(t, what):
    if not torch.cuda.is_available() or not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.V3DLibraryError('%s: the frames must live on a HIP device (no CPU fallback)' % what)


def register_colour(colour, depth_size, K_color, K_depth, out=None):
    """colour: uint8 [n, Hc, Wc, 3] or [Hc, Wc, 3] on the device, channel order as stored; depth_size (h, w); the two intrinsics of
    the scene.  -> uint8 [n, h, w, 3] on the device: the reference's ``process_color_image`` (preprocess_scannet.py:36-70), i.e. a
    nearest ``grid_sample`` with zero padding through ``colour_to_depth_homography`` (include/v3d.h: v3d_register_colour_u8 pins the
    arithmetic, the reference's normalisers included).  ``out``: a contiguous uint8 [n, h, w, 3] device tensor to write into."""
    lib = _lib.load()
    _on_device(colour, 'register_colour')
    if colour.dim() == 3:
        colour = colour[None]
    if colour.dtype != torch.uint8 or colour.dim() != 4 or colour.shape[3] != 3:
        raise ValueError('register_colour: colour must be uint8 [n, Hc, Wc, 3], got %s %s' % (colour.dtype, tuple(colour.shape)))
    colour = colour.contiguous()
    n, Hc, Wc, _ = (int(v) for v in colour.shape)
    h, w = (int(v) for v in depth_size)
    H = colour_to_depth_homography(K_color, K_depth)
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=colour.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or out.device != colour.device:
        raise ValueError('register_colour: out must be uint8 %s on the frames\' device' % ((n, h, w, 3),))
    h_host = (_lib.c_float * 9)(*[float(v) for v in H.reshape(-1)])
    with torch.cuda.device(colour.device):
        _lib.check(lib.v3d_register_colour_u8(_lib.ptr(colour), n, Hc, Wc, h_host, h, w, _lib.ptr(out), _lib.stream_ptr(colour.device)),
                   'v3d_register_colour_u8')
    return out


def depth_lut(kind):
    """-> uint16 [65536] (NumPy): what the reference's script turns every raw 16-bit depth value into (raw / 5000 metres ->
    millimetres, truncated).  ``'icl-nuim'``: in float64 (preprocess_icl_nuim.py:181-185); ``'tum-rgbd'``: in float32
    (preprocess_tum_rgbd.py:177-180).  The two differ on 144 of the 65 536 values, and neither equals ``raw // 5``, so the
    conversion is a table of the reference's own expression and not arithmetic of this package's.  The reference's NaN and inf
    lines cannot fire on converted integers."""
    raw = np.arange(65536, dtype=np.uint16)
    if kind == 'icl-nuim':
        return (raw.astype(np.float64) / 5_000. * 1000).astype(np.uint16)
    if kind == 'tum-rgbd':
        return (raw.astype(np.float32) / 5000. * 1000.).astype(np.uint16)
    raise ValueError("depth_lut: kind must be 'icl-nuim' or 'tum-rgbd', got %r" % (kind,))


def convert_depth(depth_raw, lut, out=None):
    """depth_raw: a device tensor of any shape holding the bits of uint16 values (a uint16 tensor, or an int16 tensor that holds
    them, as ``dataset.depths_from_frames`` accepts them); lut: ``depth_lut(kind)`` (NumPy, or a 65 536-element 16-bit device
    tensor).  -> ``lut[depth_raw]`` in the shape and dtype of ``depth_raw`` (v3d_lut_u16)."""
    lib = _lib.load()
    _on_device(depth_raw, 'convert_depth')
    if depth_raw.element_size() != 2 or depth_raw.dtype.is_floating_point:
        raise ValueError('convert_depth: depth_raw must hold 16-bit integers, got %s' % depth_raw.dtype)
    if not torch.is_tensor(lut):
        lut = torch.from_numpy(np.ascontiguousarray(np.asarray(lut, dtype=np.uint16)).view(np.int16)).to(depth_raw.device)
    if lut.numel() != 65536 or lut.element_size() != 2 or lut.dtype.is_floating_point or lut.device != depth_raw.device:
        raise ValueError('convert_depth: lut must hold 65536 16-bit integers on the device of depth_raw')
    depth_raw, lut = depth_raw.contiguous(), lut.contiguous()
    if out is None:
        out = torch.empty_like(depth_raw)
    elif out.shape != depth_raw.shape or out.dtype != depth_raw.dtype or out.device != depth_raw.device or out.data_ptr() == depth_raw.data_ptr():
        raise ValueError('convert_depth: out must be another tensor of the shape, dtype and device of depth_raw')
    if depth_raw.numel() == 0:
        return out
    with torch.cuda.device(depth_raw.device):
        _lib.check(lib.v3d_lut_u16(_lib.ptr(depth_raw), depth_raw.numel(), _lib.ptr(lut), _lib.ptr(out), _lib.stream_ptr(depth_raw.device)),
                   'v3d_lut_u16')
    return out


# ---- ground-truth mesh ----------------------------------------------------------------------------------------------------------

def gt_mesh_from_frames(colour, depth_mm, K, poses, img_batch=IMG_BATCH, vox_res=VOX_RES, vol_prcnt=VOL_PRCNT, vol_margin=VOL_MARGIN,
                        trunc_ratio=TRUNC_RATIO, max_depth=None, bounds='host', device=None, stages=None):
    """The reference's ``generate_gt_mesh`` (preprocess_icl_nuim.py:75-135, preprocess_tum_rgbd.py:63-126) -> ``mesh.TriangleMesh``
    on the device: every sensor depth frame of a scene fused into a TSDF of ``vox_res`` metres, the mesh extracted.

    colour uint8 [N, H, W, 3] as stored, depth_mm uint16 [N, H, W], K [3, 3] and poses [N, 4, 4] (camera -> world) float64 as in
    ``info.json``.  For every consecutive chunk of ``img_batch`` frames this forms the batch that ``Dataset(scene,
    EveryNthSelector(1), img_batch, (H, W), (H, W), False, scale_rgb=1., mean_rgb=[0, 0, 0], std_rgb=[1, 1, 1], crop=False,
    n_src_on_either_side=0).get(0, seed_idx=i * img_batch)`` returns -- the images as float grey levels, the depths in metres with
    the invalid ones zeroed (``dataset.images_from_frames`` / ``depths_from_frames``), projections ``K [R | t]`` formed on the
    host -- twice:
      1. bounds: ``tsdf.volume_bounds`` (``bounds='device'``: ``tsdf.volume_bounds_device``) of each chunk, i.e. with ``img_batch``
         as its batch size; a chunk without a usable pixel is skipped; running minimum / maximum across chunks.  ``max_depth``:
         depths above it are zeroed for this pass only (preprocess_tum_rgbd.py:81-82; the reference compares with the literal 4.
         whatever the argument -- here the argument's value is used, and 4. reproduces the reference);
      2. fusion: a ``TSDFFusion`` with colour integrates every view in order (one launch per chunk, the bits of one call per
         view), then ``get_tsdf().get_mesh()``.
    The frames are uploaded once and stay on the device for both passes (the reference reads every file twice): 5 bytes per
    pixel, 1.5 MB per 480 x 640 frame, 4 GB for a 2 600-frame scene; a chunk's float images and depths (16 bytes per pixel of
    ``img_batch`` frames) live only while the chunk is worked on.  Intrinsics with a negative focal length (ICL-NUIM's) need nothing
    special: the bounds and the TSDF kernels project through general 3 x 4 matrices.  The triangulation is this project's
    (DESIGN.md §6).  No CPU fallback.  ``stages``: a dict that receives the wall-clock seconds of ``upload``, ``bounds``, ``fusion``
    and ``mesh`` and the ``voxel_dim``, each stage closed by a device synchronisation (for measuring; None: none is added)."""
    _lib.load()
    colour, depth_mm = np.asarray(colour), np.asarray(depth_mm)
    if colour.dtype != np.uint8 or colour.ndim != 4 or colour.shape[3] != 3 or colour.shape[0] == 0:
        raise ValueError('gt_mesh_from_frames: colour must be uint8 [N, H, W, 3], got %s %s' % (colour.dtype, colour.shape))
    if depth_mm.dtype != np.uint16 or depth_mm.shape != colour.shape[:3]:
        raise ValueError('gt_mesh_from_frames: depth_mm must be uint16 %s, got %s %s' % (colour.shape[:3], depth_mm.dtype, depth_mm.shape))
    poses = np.asarray(poses, dtype=np.float64)
    n, H, W = depth_mm.shape
    if poses.shape != (n, 4, 4):
        raise ValueError('gt_mesh_from_frames: poses must be [%d, 4, 4], got %s' % (n, poses.shape))
    step = int(img_batch)
    if step < 1:
        raise ValueError('gt_mesh_from_frames: img_batch=%r' % (img_batch,))
    bounds_fn = _tsdf._bounds_fn(bounds, 'gt_mesh_from_frames')
    if not torch.cuda.is_available():
        raise _lib.V3DLibraryError('gt_mesh_from_frames: no HIP device (no CPU fallback)')
    dev = _dataset._device(device)
    clock = [time.perf_counter()]

    def stage(name):
        if stages is not None:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            stages[name], clock[0] = now - clock[0], now

    colour_dev, depth_dev = _dataset._upload(colour, dev), _dataset._upload(depth_mm, dev)
    stage('upload')
    # the host half of each chunk, as frames_to_batch forms it for that chunk's indices: (slice, K [m, 3, 3], world -> camera [m, 4, 4])
    chunks = []
    for start in range(0, n, step):
        sl = slice(start, min(start + step, n))
        geo = _dataset.scene_geometry(K, poses, np.arange(sl.start, sl.stop), (H, W), (H, W), False, 0)
        w2c = torch.eye(4).repeat(sl.stop - sl.start, 1, 1)
        w2c[:, :3, :3], w2c[:, :3, 3] = geo['rotmats'], geo['tvecs']
        chunks.append((sl, geo['K'].contiguous(), w2c))
    pre = geo['preprocessor']                                                      # one size, one K: the same tables for every chunk
    linear = [_dataset._upload(t, dev) for t in pre.linear_tables()]
    nearest = [_dataset._upload(t, dev) for t in pre.nearest_tables((H, W))]
    origin = vol_max = None
    for sl, K32, w2c in chunks:
        d = _dataset.depths_from_frames(depth_dev[sl], nearest)
        if max_depth is not None:
            d[d > max_depth] = 0.
        try:
            lo, hi, _ = bounds_fn(d, K32, w2c, vol_prcnt, vol_margin, vox_res, step)
        except ValueError:                                                         # no usable pixel in this chunk: skipped
            continue
        origin = lo if origin is None else torch.minimum(origin, lo)
        vol_max = hi if vol_max is None else torch.maximum(vol_max, hi)
    if origin is None:
        raise ValueError('gt_mesh_from_frames: no depth frame has a usable pixel')
    vol_dim = ((vol_max - origin) / vox_res).int().tolist()
    stage('bounds')
    fus = _tsdf.TSDFFusion(vol_dim, vox_res, origin, trunc_ratio, dev, color=True, label=False)
    for sl, K32, w2c in chunks:
        images = _dataset.images_from_frames(colour_dev[sl], linear, 1., (0., 0., 0.), (1., 1., 1.), True)
        d = _dataset.depths_from_frames(depth_dev[sl], nearest)
        fus.integrate_batch(_tsdf.projection_matrices(K32, w2c), d, images)
    stage('fusion')
    mesh = fus.get_tsdf().get_mesh()
    stage('mesh')
    if stages is not None:
        stages['voxel_dim'] = vol_dim
    return mesh


def _frame_reader(read_image):
    if read_image is None:
        return _dataset.default_read_frame
    return lambda frame: (read_image(frame['filename_color'], False), read_image(frame['filename_depth'], True))


def generate_gt_mesh(scene_dir, read_frame=None, **kw):
    """``gt_mesh_from_frames`` over a prepared scene folder: ``info.json``'s intrinsics and poses, every frame read once with
    ``read_frame(frame_info) -> (colour, depth)`` (default ``dataset.default_read_frame``)."""
    _lib.load()
    with open(os.path.join(scene_dir, 'info.json'), 'r') as f:
        info = json.load(f)
    read_frame = read_frame or _dataset.default_read_frame
    frames = [read_frame(frame) for frame in info['frames']]
    if not frames:
        raise ValueError('generate_gt_mesh: %s has no frames' % scene_dir)
    return gt_mesh_from_frames(np.stack([np.asarray(c) for c, _ in frames]), np.stack([np.asarray(d) for _, d in frames]),
                               np.asarray(info['intrinsics']), np.stack([np.asarray(fr['pose']) for fr in info['frames']]), **kw)


# ---- image files ----------------------------------------------------------------------------------------------------------------

def _cv2():
    try:
        import cv2
        return cv2
    except ImportError:
        return None


def default_read_image(path, depth):
    """One image file -> array: colour uint8 [H, W, 3] as OpenCV stores it (BGR), or (``depth``) the file's own 16-bit values
    [H, W]: ``cv2.imread`` where OpenCV is installed, else Pillow, as ``dataset.default_read_frame``."""
    cv2 = _cv2()
    if cv2 is not None:
        img = cv2.imread(path, cv2.IMREAD_ANYDEPTH) if depth else cv2.imread(path)
        if img is None:
            raise FileNotFoundError('cannot read %s' % path)
        return img
    try:
        from PIL import Image
    except ImportError:
        raise ImportError('reading images needs OpenCV (cv2) or Pillow (PIL); neither is installed -- pass read_image=')
    with Image.open(path) as im:
        if not depth:
            return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])
        if im.mode not in ('I;16', 'I;16L', 'I;16B', 'I'):
            raise ValueError('%s: a depth frame must be a 16-bit image, mode is %s' % (path, im.mode))
        arr = np.asarray(im)
    if arr.min() < 0 or arr.max() > 65535:
        raise ValueError('%s: depth values outside 16 bits' % path)
    return arr.astype(np.uint16)


def default_write_image(path, array):
    """uint8 [H, W, 3] (BGR, as OpenCV takes it) or uint16 [H, W] -> the file type of ``path``'s suffix: ``cv2.imwrite``, else
    Pillow.  A JPEG's bytes depend on the encoder at hand."""
    array = np.asarray(array)
    cv2 = _cv2()
    if cv2 is not None:
        if not cv2.imwrite(path, array):
            raise IOError('cannot write %s' % path)
        return
    try:
        from PIL import Image
    except ImportError:
        raise ImportError('writing images needs OpenCV (cv2) or Pillow (PIL); neither is installed -- pass write_image=')
    if array.ndim == 3:
        Image.fromarray(np.ascontiguousarray(array[:, :, ::-1])).save(path)
    else:
        Image.fromarray(np.ascontiguousarray(array.astype(np.uint16))).save(path)


def _io(read_image, write_image, exists):
    return read_image or default_read_image, write_image or default_write_image, exists or os.path.exists


# ---- scene drivers --------------------------------------------------------------------------------------------------------------

def quat_to_matrix(q_xyzw):
    """[4] or [n, 4] quaternions (x, y, z, w; any non-zero norm) -> [3, 3] or [n, 3, 3] float64 rotation matrices, as
    ``scipy.spatial.transform.Rotation.from_quat(q).as_matrix()``: the quaternion divided by its norm, then sums of products of
    its components."""
    q = np.asarray(q_xyzw, dtype=np.float64)
    single = q.ndim == 1
    q = q.reshape(-1, 4)
    norm = np.sqrt(np.sum(q * q, axis=1))
    if np.any(norm == 0):
        raise ValueError('quat_to_matrix: a quaternion of zero norm')              # as SciPy; a NaN gives a NaN matrix
    q = q / norm[:, None]
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    x2, y2, z2, w2 = x * x, y * y, z * z, w * w
    xy, zw, xz, yw, yz, xw = x * y, z * w, x * z, y * w, y * z, x * w
    m = np.empty((q.shape[0], 3, 3), dtype=np.float64)
    m[:, 0, 0] = x2 - y2 - z2 + w2
    m[:, 1, 0] = 2 * (xy + zw)
    m[:, 2, 0] = 2 * (xz - yw)
    m[:, 0, 1] = 2 * (xy - zw)
    m[:, 1, 1] = -x2 + y2 - z2 + w2
    m[:, 2, 1] = 2 * (yz + xw)
    m[:, 0, 2] = 2 * (xz + yw)
    m[:, 1, 2] = 2 * (yz - xw)
    m[:, 2, 2] = -x2 - y2 + z2 + w2
    return m[0] if single else m


def fix_pose(P):
    """ICL-NUIM's poses turned by a quarter about x (preprocess_icl_nuim.py:64-72): ``P_fix @ P`` in float64, ``P_fix`` the
    identity with ``FIX_POSE_R`` in its corner."""
    P_fix = np.eye(4)
    P_fix[:3, :3] = FIX_POSE_R
    return P_fix @ P


def get_closest_index(target_timestamp, other_timestamps):
    """The first index of the smallest |difference| (preprocess_tum_rgbd.py:129-131)."""
    return np.argmin(np.abs(other_timestamps - target_timestamp))


def _to_host_u16(t):
    return t.cpu().numpy().view(np.uint16)


def process_scene_scannet(scene_dir_src, scene_dir_dst, device=None, read_image=None, write_image=None, exists=None):
    """``process_scene`` of preprocess_scannet.py:73-134: an exported ScanNet scene (``color/<id>.jpg``, ``depth/<id>.png``,
    ``pose/<id>.txt``, ``intrinsic/intrinsic_{color,depth}.txt``, ``<scene>_vh_clean_2.ply``) -> ``scene_dir_dst`` with the colour
    frames registered into the depth camera (``register_colour``, only where the two sizes differ), the depth frames copied, the
    mesh file copied and ``info.json`` with the reference's keys.  Frames with a non-finite pose are skipped.  The reference's file
    names are kept, its ``'{}.jpg'.format(id).zfill(9)`` padding of the whole name included.  ``read_image(path, depth) -> array``,
    ``write_image(path, array)`` and ``exists(path)`` replace the file access of the images (the text files and the mesh are real
    files).  The registered frame is stored as JPEG: the pixels handed to the encoder are the reference's, the file's bytes are the
    encoder's."""
    read_image, write_image, exists = _io(read_image, write_image, exists)
    scene_name = os.path.basename(scene_dir_src)
    data = {'scene': scene_name, 'path': scene_dir_dst, 'frames': []}
    for d in (scene_dir_dst, os.path.join(scene_dir_dst, 'color'), os.path.join(scene_dir_dst, 'depth')):
        os.makedirs(d, exist_ok=True)
    gt_mesh_src = os.path.join(scene_dir_src, '{}_vh_clean_2.ply'.format(scene_name))
    gt_mesh_dst = os.path.join(scene_dir_dst, '{}_vh_clean_2.ply'.format(scene_name))
    shutil.copy(gt_mesh_src, gt_mesh_dst)
    data['gt_mesh'] = gt_mesh_dst
    K_color = np.loadtxt(os.path.join(scene_dir_src, 'intrinsic', 'intrinsic_color.txt'))[:3, :3]
    K_depth = np.loadtxt(os.path.join(scene_dir_src, 'intrinsic', 'intrinsic_depth.txt'))[:3, :3]
    data['intrinsics'] = K_depth.tolist()
    frames = sorted([f for f in os.listdir(os.path.join(scene_dir_src, 'color')) if f.endswith('.jpg')],
                    key=lambda x: int(x.split('.')[0]))
    for frame in frames:
        frame_id = int(frame.split('.')[0])
        fname_color_src = os.path.join(scene_dir_src, 'color', frame)
        fname_depth_src = os.path.join(scene_dir_src, 'depth', '{}.png'.format(frame_id))
        fname_color_dst = os.path.join(scene_dir_dst, 'color', '{}.jpg'.format(frame_id).zfill(9))
        fname_depth_dst = os.path.join(scene_dir_dst, 'depth', '{}.png'.format(frame_id).zfill(9))
        color = np.asarray(read_image(fname_color_src, False))
        depth = np.asarray(read_image(fname_depth_src, True))
        P = np.loadtxt(os.path.join(scene_dir_src, 'pose', '{}.txt'.format(frame_id)))
        if not np.all(np.isfinite(P)):                                             # skip invalid poses
            continue
        if color.shape[:2] != depth.shape[:2]:
            dev = _dataset._device(device)
            color = register_colour(_dataset._upload(color, dev), depth.shape[:2], K_color, K_depth)[0].cpu().numpy()
            write_image(fname_color_dst, color)
        elif not exists(fname_color_dst):
            write_image(fname_color_dst, color)
        if not exists(fname_depth_dst):
            write_image(fname_depth_dst, depth)
        data['frames'].append({'filename_color': fname_color_dst, 'filename_depth': fname_depth_dst, 'pose': P.tolist()})
    with open(os.path.join(scene_dir_dst, 'info.json'), 'w') as f:
        json.dump(data, f)
    return data


def _convert_depth_file(src, dst, lut, device, read_image, write_image):
    raw = np.asarray(read_image(src, True))
    if raw.dtype != np.uint16:
        raise ValueError('%s: a raw depth frame must be 16-bit, got %s' % (src, raw.dtype))
    write_image(dst, _to_host_u16(convert_depth(_dataset._upload(raw, _dataset._device(device)), lut)))


def _finish_scene(scene, data, gt_mesh_file, overwrite_mesh, read_image, mesh_kw, device):
    if device is not None:
        mesh_kw = dict(mesh_kw, device=device)
    with open(os.path.join(scene, 'info.json'), 'w') as f:
        json.dump(data, f)
    if not os.path.exists(gt_mesh_file) or overwrite_mesh:
        generate_gt_mesh(scene, _frame_reader(read_image), **mesh_kw).write_ply(gt_mesh_file)
    return data


def process_scene_icl_nuim(scene, overwrite_depth=False, overwrite_mesh=False, device=None, read_image=None, write_image=None,
                           exists=None, **mesh_kw):
    """``process_scene`` of preprocess_icl_nuim.py:138-200, in place: ``associations.txt`` and the ``*.gt.freiburg`` poses ->
    ``depth_processed/`` (``convert_depth`` with the float64 table), ``info.json`` (the reference's K, poses = ``fix_pose`` of the
    quaternion's matrix; frames without a pose or with a non-finite one are skipped) and ``gt_mesh.ply`` (``generate_gt_mesh``,
    written by ``TriangleMesh.write_ply``; ``mesh_kw`` goes to ``gt_mesh_from_frames``).  ``read_image`` / ``write_image`` /
    ``exists`` as in ``process_scene_scannet``; passed a ``read_image``, the mesh pass reads its frames through it as well."""
    reader = read_image
    read_image, write_image, exists = _io(read_image, write_image, exists)
    scene_name = os.path.basename(scene)
    process_depth_dir = os.path.join(scene, 'depth_processed')
    gt_mesh_file = os.path.join(scene, 'gt_mesh.ply')
    os.makedirs(process_depth_dir, exist_ok=True)
    data = {'scene': scene_name, 'path': scene, 'intrinsics': K_ICL_NUIM.tolist(), 'gt_mesh': gt_mesh_file, 'frames': []}
    with open(os.path.join(scene, 'associations.txt'), 'r') as f:
        raw_frames_info = f.readlines()
    with open(glob.glob(os.path.join(scene, '*.gt.freiburg'))[0], 'r') as f:
        raw_poses_info = f.readlines()
    poses_dict = {}
    for raw_pose_info in raw_poses_info:
        split = raw_pose_info.strip().split(' ')
        poses_dict[split[0]] = np.asarray([float(v) for v in split[1:]])
    lut = None
    for raw_frame_info in raw_frames_info:
        split = raw_frame_info.strip().split(' ')
        if split[0] not in poses_dict:
            continue
        pose_raw = poses_dict[split[0]]
        depth_filepath_src = os.path.join(scene, split[1])
        depth_filepath_dst = os.path.join(process_depth_dir, os.path.basename(depth_filepath_src))
        color_filepath = os.path.join(scene, split[3])
        rotmat = quat_to_matrix(pose_raw[3:])
        P = np.concatenate((np.concatenate((rotmat, np.reshape(pose_raw[:3], (3, 1))), axis=1), np.array([[0., 0., 0., 1.]])), axis=0)
        P = fix_pose(P)
        if not np.all(np.isfinite(P)):                                             # skip invalid poses
            continue
        if overwrite_depth or not exists(depth_filepath_dst):
            if lut is None:
                lut = depth_lut('icl-nuim')
            _convert_depth_file(depth_filepath_src, depth_filepath_dst, lut, device, read_image, write_image)
        data['frames'].append({'filename_color': color_filepath, 'filename_depth': depth_filepath_dst, 'pose': P.tolist()})
    return _finish_scene(scene, data, gt_mesh_file, overwrite_mesh, reader, mesh_kw, device)


def process_scene_tum_rgbd(scene, overwrite_depth=False, overwrite_mesh=False, device=None, read_image=None, write_image=None,
                           exists=None, **mesh_kw):
    """``process_scene`` of preprocess_tum_rgbd.py:134-194, in place: every depth frame of ``depth/`` with the pose of
    ``groundtruth.txt`` and the colour frame of ``rgb/`` whose timestamps are closest to its own (``get_closest_index``: the first
    of equally close ones) -> ``depth_processed/`` (``convert_depth`` with the float32 table), ``info.json`` (the reference's K)
    and ``gt_mesh.ply``.  Arguments as ``process_scene_icl_nuim``."""
    reader = read_image
    read_image, write_image, exists = _io(read_image, write_image, exists)
    depth_out_dir = os.path.join(scene, 'depth_processed')
    os.makedirs(depth_out_dir, exist_ok=True)
    scene_name = os.path.basename(scene)
    gt_mesh_file = os.path.join(scene, 'gt_mesh.ply')
    data = {'scene': scene_name, 'path': scene, 'intrinsics': K_TUM_RGBD.tolist(), 'gt_mesh': gt_mesh_file, 'frames': []}
    image_filenames = sorted(glob.glob(os.path.join(scene, 'rgb', '*.png')))
    image_timestamps = np.atleast_1d(np.loadtxt(os.path.join(scene, 'rgb.txt'), usecols=0))
    depth_filenames = sorted(glob.glob(os.path.join(scene, 'depth', '*.png')))
    depth_timestamps = np.atleast_1d(np.loadtxt(os.path.join(scene, 'depth.txt'), usecols=0))
    poses_with_quat = np.atleast_2d(np.loadtxt(os.path.join(scene, 'groundtruth.txt')))
    pose_timestamps = poses_with_quat[:, 0]
    pose_locations = poses_with_quat[:, 1:4]
    pose_quaternions = poses_with_quat[:, 4:]
    lut = None
    for i in range(len(depth_filenames)):
        depth_timestamp = depth_timestamps[i]
        pose_index = get_closest_index(depth_timestamp, pose_timestamps)
        image_index = get_closest_index(depth_timestamp, image_timestamps)
        depth_filename_src = depth_filenames[i]
        depth_filename_dst = os.path.join(depth_out_dir, os.path.basename(depth_filename_src))
        pose = np.eye(4)
        pose[0:3, 0:3] = quat_to_matrix(pose_quaternions[pose_index])
        pose[0:3, 3] = pose_locations[pose_index]
        if not exists(depth_filename_dst) or overwrite_depth:
            if lut is None:
                lut = depth_lut('tum-rgbd')
            _convert_depth_file(depth_filename_src, depth_filename_dst, lut, device, read_image, write_image)
        data['frames'].append({'filename_color': image_filenames[image_index], 'filename_depth': depth_filename_dst,
                               'pose': pose.tolist()})
    return _finish_scene(scene, data, gt_mesh_file, overwrite_mesh, reader, mesh_kw, device)
