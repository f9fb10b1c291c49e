"""Scene batches from decoded frames: counterpart of ``mv3d/dsets/dataset.py`` (PreprocessImage :21-96, Dataset :99-237).

The reference prepares a scene on the host, one frame at a time: crop, ``cv2.resize``, a torch normalisation per image, a NumPy
conversion and two nearest resizes per depth frame.  Here the host does what is sequential or tiny -- ``info.json``, the frame
selector, the crop and intrinsics arithmetic, the edge window, the pose inversion and the gather tables of the two resizes, all in
the reference's number types -- and the device does the pixels: the decoded frames are stacked, uploaded once and turned into
``images`` and ``depth_images`` by two gather kernels (csrc/frames.hip; include/v3d.h: v3d_frames_to_images_f32,
v3d_frames_to_depths_f32).  Every tensor of the returned ``Batch`` lives on the device.  There is no CPU path: without a HIP device
``get`` fails through ``_lib`` as the rest of the package does.

    scene_geometry    the host half of a batch: edges, reference views, rotations, translations, intrinsics (no device needed)
    frames_to_batch   decoded arrays + K + poses + img_idx -> Batch (for callers that hold frames in memory)
    Dataset           the reference's class: scene folders + a frame selector -> Batch

Not built: ``augment=True`` (colour jitter, random rotation and scale) raises NotImplementedError -- the package has no training
pass; ``get_dataloader`` and torch_geometric collation.
"""
import json
import os

import numpy as np
import torch

from . import _lib
from .batch import Batch


class PreprocessImage:
    """Crop to the target aspect ratio, resize, and the intrinsics that go with both: the reference's constructor and
    ``get_updated_intrinsics`` in float64, operation for operation, plus the gather tables the device kernels read in place of
    its two ``cv2.resize`` calls."""

    def __init__(self, K, old_width, old_height, new_width, new_height, distortion_crop=0, perform_crop=True):
        self.old_width, self.old_height = int(old_width), int(old_height)          # of the frames as stored
        self.new_width, self.new_height = new_width, new_height
        self.perform_crop = perform_crop
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        self.crop_x = self.crop_y = 0
        if perform_crop:
            inner_h = old_height - 2 * distortion_crop
            inner_w = old_width - 2 * distortion_crop
            new_aspect = float(new_width) / float(new_height)
            if float(inner_w) / float(inner_h) > new_aspect:                       # too wide: crop columns
                self.crop_x = int(np.floor((inner_w - inner_h * new_aspect) / 2.0)) + distortion_crop
                self.crop_y = distortion_crop
            else:                                                                  # too tall: crop rows
                self.crop_x = distortion_crop
                self.crop_y = int(np.floor((inner_h - inner_w / new_aspect) / 2.0)) + distortion_crop
            cx = cx - self.crop_x
            cy = cy - self.crop_y
        factor_x = float(new_width) / float(old_width - 2 * self.crop_x)
        factor_y = float(new_height) / float(old_height - 2 * self.crop_y)
        self.fx, self.fy, self.cx, self.cy = fx * factor_x, fy * factor_y, cx * factor_x, cy * factor_y

    def get_updated_intrinsics(self):
        return np.array([[self.fx, 0, self.cx],
                         [0, self.fy, self.cy],
                         [0, 0, 1]])

    def linear_tables(self):
        """(y0, y1, wy, x0, x1, wx): per output row / column of the resized image the two rows / columns of the STORED frame it
        blends (int32) and the weight of the second (float32): the linear filter with half-pixel centres and a replicated border,
        without antialiasing, over the cropped frame.  Float64 on the host, as OpenCV computes its own tables; the weight is
        rounded to fp32 once."""
        return (linear_axis(self.new_height, self.old_height, self.crop_y) +
                linear_axis(self.new_width, self.old_width, self.crop_x))

    def nearest_tables(self, depth_img_size):
        """(ys, xs): the row / column of the STORED depth frame that row / column of the final depth map is taken from (int32):
        the composition of ``cv2.resize(INTER_NEAREST)`` from the cropped frame to the image size (apply_depth) and
        ``F.interpolate(mode='nearest')`` from the image size to ``depth_img_size`` (dataset.py:219)."""
        return (nearest_axis(depth_img_size[0], self.new_height, self.old_height, self.crop_y),
                nearest_axis(depth_img_size[1], self.new_width, self.old_width, self.crop_x))


def linear_axis(dst, src, crop):
    """Linear gather table of one axis: `dst` output cells over the n = src - 2 crop inner cells of a source axis of `src`."""
    n = src - 2 * crop
    f = (np.arange(dst, dtype=np.float64) + 0.5) * (float(n) / float(dst)) - 0.5
    s = np.floor(f)
    w = f - s
    low, high = s < 0, s >= n - 1
    s = np.where(low, 0, np.where(high, n - 1, s)).astype(np.int64)
    w = np.where(low | high, 0.0, w)
    i0 = s + crop
    i1 = np.minimum(s + 1, n - 1) + crop
    return i0.astype(np.int32), i1.astype(np.int32), w.astype(np.float32)


def nearest_axis(out, mid, src, crop):
    """Composed nearest table of one axis: `out` final cells <- `mid` cells of the resized frame <- the n = src - 2 crop inner
    cells of the stored frame.  First step as OpenCV's INTER_NEAREST (float64: floor(d * (1 / (mid / n))), clamped to n - 1),
    second as torch's nearest (fp32: floorf(d * (float(mid) / float(out))), clamped to mid - 1)."""
    n = src - 2 * crop
    first = np.minimum(np.floor(np.arange(mid, dtype=np.float64) * (1.0 / (float(mid) / float(n)))).astype(np.int64), n - 1) + crop
    scale = np.float32(mid) / np.float32(out)
    second = np.minimum(np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64), mid - 1)
    return first[second].astype(np.int32)


def scene_geometry(K, poses, img_idx, frame_size, img_size=(256, 320), crop=False, n_src_on_either_side=1):
    """The host half of a batch (dataset.py:130-137, :148-154, :214-216, :226): no device needed.

    K [3, 3] and poses [n_frames, 4, 4] float64 as info.json holds them, img_idx the selected frames, frame_size (H, W) of the
    stored frames.  Returns a dict: ``preprocessor`` (PreprocessImage), ``ref_idx`` (the frames that are reference views; with
    n_src_on_either_side = 0 the reference's slice [0:-0] is empty: no reference views, no edges), ``ref_src_edges`` [2, n_ref *
    (2 k + 1)] int64, ``rotmats`` [n, 3, 3], ``tvecs`` [n, 3] and ``K`` [n, 3, 3] (float32, CPU; K an expanded view)."""
    K = np.asarray(K)
    poses = np.asarray(poses)
    img_idx = np.asarray(img_idx)
    k = n_src_on_either_side
    ref_idx = img_idx[k:-k]
    n_ref, per_ref = ref_idx.shape[0], 2 * k + 1
    first = torch.arange(n_ref, dtype=torch.long)
    ref_src_edges = torch.stack(((first + k).repeat_interleave(per_ref),
                                 (first[:, None] + torch.arange(per_ref, dtype=torch.long)[None]).reshape(-1)))
    pre = PreprocessImage(K=K, old_width=frame_size[1], old_height=frame_size[0], new_width=img_size[1], new_height=img_size[0],
                          distortion_crop=0, perform_crop=crop)
    rotmats = torch.from_numpy(poses[img_idx, :3, :3]).float().transpose(2, 1)
    tvecs = -torch.bmm(rotmats, torch.from_numpy(poses[img_idx, :3, 3, None]).float())[..., 0]
    rotmats = rotmats @ torch.eye(3, dtype=torch.float32).T                        # R_aug of a pass without augmentation
    K32 = torch.from_numpy(pre.get_updated_intrinsics().astype(np.float32)).unsqueeze(0).expand(img_idx.shape[0], 3, 3)
    return dict(preprocessor=pre, ref_idx=ref_idx, ref_src_edges=ref_src_edges, rotmats=rotmats, tvecs=tvecs, K=K32)


def _device(device):
    return torch.device('cuda' if device is None else device)


def _upload(array, device):
    """One host array -> device tensor: through pinned memory when a device is there (one asynchronous copy).  uint16 travels
    as the int16 tensor of the same bits."""
    array = np.ascontiguousarray(array)
    t = torch.from_numpy(array.view(np.int16) if array.dtype == np.uint16 else array)
    if torch.cuda.is_available():
        t = t.pin_memory()
    return t.to(device, non_blocking=True)


def images_from_frames(frames, tables, scale_rgb=255., mean_rgb=(0.485, 0.456, 0.406), std_rgb=(0.229, 0.224, 0.225),
                       quantize=True, out=None):
    """frames: uint8 [n, H, W, 3] on the device; tables: PreprocessImage.linear_tables() as device tensors.  -> fp32
    [n, 3, oh, ow] (v3d_frames_to_images_f32)."""
    lib = _lib.load()
    y0, y1, wy, x0, x1, wx = tables
    n, H, W, _ = frames.shape
    assert frames.dtype == torch.uint8 and frames.shape[3] == 3
    oh, ow = y0.numel(), x0.numel()
    if out is None:
        out = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=frames.device)
    mean = (_lib.c_float * 3)(*[np.float32(v) for v in mean_rgb])
    std = (_lib.c_float * 3)(*[np.float32(v) for v in std_rgb])
    _lib.check(lib.v3d_frames_to_images_f32(_lib.ptr(frames), n, H, W, _lib.ptr(y0), _lib.ptr(y1), _lib.ptr(wy), _lib.ptr(x0),
                                            _lib.ptr(x1), _lib.ptr(wx), oh, ow, 1 if quantize else 0, float(np.float32(scale_rgb)),
                                            mean, std, _lib.ptr(out), _lib.stream_ptr(frames.device)), 'v3d_frames_to_images_f32')
    return out


def depths_from_frames(depth_mm, tables, out=None):
    """depth_mm: [n, H, W] on the device, the bits of uint16 millimetres (a uint16 tensor, or an int16 tensor that holds them);
    tables: PreprocessImage.nearest_tables(size) as device tensors.  -> fp32 metres [n, oh, ow], invalid (> 65 m) depths zeroed
    (v3d_frames_to_depths_f32)."""
    lib = _lib.load()
    ys, xs = tables
    n, H, W = depth_mm.shape
    assert depth_mm.element_size() == 2 and not depth_mm.dtype.is_floating_point
    oh, ow = ys.numel(), xs.numel()
    if out is None:
        out = torch.empty((n, oh, ow), dtype=torch.float32, device=depth_mm.device)
    _lib.check(lib.v3d_frames_to_depths_f32(_lib.ptr(depth_mm), n, H, W, _lib.ptr(ys), _lib.ptr(xs), oh, ow, _lib.ptr(out),
                                            _lib.stream_ptr(depth_mm.device)), 'v3d_frames_to_depths_f32')
    return out


def frames_to_batch(colour, depth_mm, K, poses, img_idx, depth_img_size=(56, 56), img_size=(256, 320), scale_rgb=255.,
                    mean_rgb=(0.485, 0.456, 0.406), std_rgb=(0.229, 0.224, 0.225), n_src_on_either_side=1, crop=False, device=None,
                    quantize=True):
    """Decoded frames -> ``Batch`` on the device.

    colour [n, H, W, 3] uint8 (channel order as stored) and depth_mm [n, H, W] uint16: the frames ``img_idx`` selects, in that
    order; K, poses: of the whole scene, float64, as in info.json (``poses[img_idx]`` are the frames' poses).  ``quantize``:
    round the resized grey levels to integers before the normalisation, as the uint8 image ``cv2.resize`` returns does."""
    _lib.load()                                                                    # no CPU path: fail before any work
    colour, depth_mm = np.asarray(colour), np.asarray(depth_mm)
    if colour.dtype != np.uint8 or colour.ndim != 4 or colour.shape[3] != 3:
        raise ValueError('frames_to_batch: colour must be uint8 [n, H, W, 3], got %s %s' % (colour.dtype, colour.shape))
    if depth_mm.dtype != np.uint16 or depth_mm.shape != colour.shape[:3]:
        raise ValueError('frames_to_batch: depth_mm must be uint16 %s, got %s %s' % (colour.shape[:3], depth_mm.dtype, depth_mm.shape))
    if colour.shape[0] != len(img_idx):
        raise ValueError('frames_to_batch: %d frames for %d indices' % (colour.shape[0], len(img_idx)))
    device = _device(device)
    geo = scene_geometry(K, poses, img_idx, colour.shape[1:3], img_size, crop, n_src_on_either_side)
    pre, k = geo['preprocessor'], n_src_on_either_side
    if k > 0:
        depth_mm = depth_mm[k:-k]                                                  # depth maps of the reference views only
    linear = [_upload(t, device) for t in pre.linear_tables()]
    nearest = [_upload(t, device) for t in pre.nearest_tables(depth_img_size)]
    images = images_from_frames(_upload(colour, device), linear, scale_rgb, mean_rgb, std_rgb, quantize)
    if depth_mm.shape[0]:
        depth_images = depths_from_frames(_upload(depth_mm, device), nearest)
    else:
        depth_images = torch.empty((0,) + tuple(depth_img_size), dtype=torch.float32, device=device)
    return Batch(images, geo['rotmats'].to(device), geo['tvecs'].to(device), geo['K'].to(device).contiguous(), depth_images,
                 geo['ref_src_edges'].to(device))


def default_read_frame(frame_info):
    """(colour uint8 [H, W, 3] as OpenCV stores it (BGR), depth uint16 [H, W]) of one ``info.json`` frame record: ``cv2.imread``
    where OpenCV is installed, else PIL (RGB reversed to OpenCV's order, 16-bit PNG read as 16 bits).  ImportError without either."""
    try:
        import cv2
    except ImportError:
        cv2 = None
    if cv2 is not None:
        colour = cv2.imread(frame_info['filename_color'])
        depth = cv2.imread(frame_info['filename_depth'], cv2.IMREAD_ANYDEPTH)
        if colour is None or depth is None:
            raise FileNotFoundError('cannot read %s / %s' % (frame_info['filename_color'], frame_info['filename_depth']))
        return colour, depth
    try:
        from PIL import Image
    except ImportError:
        raise ImportError('reading frames needs OpenCV (cv2) or Pillow (PIL); neither is installed -- pass read_frame= to Dataset')
    with Image.open(frame_info['filename_color']) as im:
        colour = np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])
    with Image.open(frame_info['filename_depth']) as im:
        if im.mode not in ('I;16', 'I;16L', 'I;16B', 'I'):
            raise ValueError('%s: a depth frame must be a 16-bit image, mode is %s' % (frame_info['filename_depth'], im.mode))
        depth = np.asarray(im)
    if depth.min() < 0 or depth.max() > 65535:
        raise ValueError('%s: depth values outside 16 bits' % frame_info['filename_depth'])
    return colour, depth.astype(np.uint16)


class Dataset:
    """``mv3d.dsets.dataset.Dataset`` with the device doing the pixels: ``get`` returns a ``Batch`` whose tensors are all on
    ``device``.  ``read_frame(frame_info) -> (colour uint8 [H, W, 3] as stored, depth uint16 [H, W])`` replaces the default reader."""

    def __init__(self, scene_dirs, frame_selector, n_ref_imgs=None, depth_img_size=(56, 56), img_size=(256, 320), augment=False,
                 scale_rgb=255., mean_rgb=[0.485, 0.456, 0.406], std_rgb=[0.229, 0.224, 0.225], n_src_on_either_side=1, crop=False,
                 device=None, read_frame=None, quantize=True):
        if augment:
            raise NotImplementedError('Dataset(augment=True): colour, rotation and scale augmentation are not built (the package '
                                      'has no training pass)')
        self.scene_dirs = scene_dirs
        self.n_ref_imgs = n_ref_imgs
        self.depth_img_size = depth_img_size
        self.img_size = img_size
        self.augment = augment
        self.n_src_on_either_side = n_src_on_either_side
        self.frame_selector = frame_selector
        self.crop = crop
        self.scale_rgb = scale_rgb
        self.mean_rgb = mean_rgb
        self.std_rgb = std_rgb
        self.device = device
        self.read_frame = read_frame or default_read_frame
        self.quantize = quantize

    def len(self):
        return len(self.scene_dirs)

    __len__ = len

    def get(self, idx, return_verbose=False, seed_idx=None):
        _lib.load()                                                                # no CPU path: fail before reading a frame
        scene_dir = self.scene_dirs[idx]
        with open(os.path.join(scene_dir, 'info.json'), 'r') as f:
            scene_info = json.load(f)
        all_poses = np.stack([np.asarray(frame['pose']) for frame in scene_info['frames']], axis=0)
        K = np.asarray(scene_info['intrinsics'])
        k = self.n_src_on_either_side
        n_imgs = self.n_ref_imgs + 2 * k if self.n_ref_imgs is not None else 100_000
        img_idx = self.frame_selector.select_frames(all_poses, n_imgs, seed_idx)
        colour, depth = [], []
        for i in img_idx:
            c, d = self.read_frame(scene_info['frames'][i])
            c, d = np.asarray(c), np.asarray(d)
            if colour and c.shape != colour[0].shape:                              # one PreprocessImage serves the whole scene
                raise ValueError('%s: frame %d is %s, the first selected frame is %s' % (scene_dir, i, c.shape, colour[0].shape))
            if d.shape != c.shape[:2]:
                raise ValueError('%s: depth frame %d is %s, its colour frame %s' % (scene_dir, i, d.shape, c.shape))
            colour.append(c)
            depth.append(d)
        batch = frames_to_batch(np.stack(colour), np.stack(depth), K, all_poses, img_idx, self.depth_img_size, self.img_size,
                                self.scale_rgb, self.mean_rgb, self.std_rgb, k, self.crop, self.device, self.quantize)
        if return_verbose:
            return batch, torch.eye(3, dtype=torch.float32), 1., img_idx
        return batch
