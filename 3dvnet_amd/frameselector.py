"""Frame selectors of ``mv3d/dsets/frameselector.py``: which frames of a scene's pose sequence become the images of a batch.

Host code, NumPy, float64 poses [n, 4, 4] (camera to world).  The selectors are short sequential walks over the sequence -- each
choice depends on the one before -- so there is nothing here for the device.  The constructor arguments, the
``select_frames(poses, n_frames, seed_idx=None)`` signature and the returned index arrays are the reference's; where the reference
draws from ``np.random`` the same calls are made in the same order, so under one ``np.random.seed`` the outputs coincide
(tests/test_dataset_oracle.py against tests/golden/Dset_selectors.npz).
"""
import numpy as np

_EYE3 = np.eye(3, dtype=np.float32)       # the reference's identity is float32; the subtraction promotes it to float64


def pose_distance(ref_inv, pose):
    """sqrt(|t_rel|^2 + 2/3 tr(I - R_rel)) of the relative pose ref^-1 pose (frameselector.py:40-43), float64."""
    rel = ref_inv @ pose
    t_rel = rel[:3, 3, None]
    return np.sqrt(np.sum(t_rel ** 2) + (2. / 3.) * np.trace(_EYE3 - rel[:3, :3]))


def _seed(seed_idx, n_total, n_frames, step):
    """The first frame: the caller's, or a random one that leaves room for n_frames steps (one np.random.randint at most)."""
    if seed_idx is not None:
        return seed_idx
    max_idx = n_total - n_frames * step - 1
    return 0 if max_idx <= 0 else np.random.randint(0, max_idx)


def _window_distances(poses, ref, search_interval):
    """Pose distances from frame `ref` to the frames ref + 1 .. ref + search_interval that exist."""
    ref_inv = np.linalg.inv(poses[ref])
    stop = min(ref + 1 + search_interval, poses.shape[0])
    return np.asarray([pose_distance(ref_inv, poses[j]) for j in range(ref + 1, stop)])


class FrameSelector:
    def select_frames(self, poses, n_frames, seed_idx=None):
        raise NotImplementedError


class _WindowSelector(FrameSelector):
    """Walks forward: the next frame is picked among the `search_interval` frames behind the current one; the walk ends early
    when the sequence does."""
    search_interval = None

    def pick(self, pdists):
        raise NotImplementedError

    def select_frames(self, poses, n_frames, seed_idx=None):
        img_idx = [_seed(seed_idx, poses.shape[0], n_frames, self.search_interval)]
        for _ in range(n_frames - 1):
            pdists = _window_distances(poses, img_idx[-1], self.search_interval)
            if len(pdists) == 0:
                break
            img_idx.append(img_idx[-1] + self.pick(pdists) + 1)
        return np.asarray(img_idx)


class RangePoseDistSelector(_WindowSelector):
    """A random frame whose pose distance lies in (p_min, p_max); the one nearest the middle of the range when there is none."""

    def __init__(self, p_min, p_max, search_interval):
        self.p_min = p_min
        self.p_max = p_max
        self.p_opt = p_min + (p_max - p_min) / 2.
        self.search_interval = search_interval

    def pick(self, pdists):
        valid = (pdists > self.p_min) & (pdists < self.p_max)
        if np.sum(valid) == 0:
            return np.argmin(np.abs(pdists - self.p_opt))
        return np.random.choice(np.arange(len(pdists))[valid])


class BestPoseDistSelector(_WindowSelector):
    """The frame whose pose distance is nearest p_opt."""

    def __init__(self, p_opt, search_interval):
        self.p_opt = p_opt
        self.search_interval = search_interval

    def pick(self, pdists):
        return np.argmin(np.abs(pdists - self.p_opt))


class NextPoseDistSelector(FrameSelector):
    """The first frame at a pose distance of p_thresh or more, or the frame `search_interval` steps on when none of the frames in
    between is; the walk ends when that frame lies behind the sequence."""

    def __init__(self, p_thresh, search_interval=30):
        self.p_thresh = p_thresh
        self.search_interval = search_interval

    def select_frames(self, poses, n_frames, seed_idx=None):
        n_total = poses.shape[0]
        img_idx = [_seed(seed_idx, n_total, n_frames, self.search_interval)]
        for _ in range(n_frames - 1):
            ref_inv = np.linalg.inv(poses[img_idx[-1]])
            cur = img_idx[-1] + 1
            for _ in range(self.search_interval):
                if cur > n_total - 1 or pose_distance(ref_inv, poses[cur]) >= self.p_thresh:
                    break
                cur += 1
            if cur > n_total - 1:
                break
            img_idx.append(cur)
        return np.asarray(img_idx)


class NeuralReconSelector(FrameSelector):
    """Key frames as NeuralRecon picks them: a frame is kept when it has moved more than tmin or turned its viewing axis by more
    than rmin_deg against the last kept frame.  n_frames is not used; seed_idx rolls the frame order (np.roll), as in the reference."""

    def __init__(self, tmin=.1, rmin_deg=15):
        self.tmin = tmin
        self.rmin_deg = rmin_deg

    def select_frames(self, poses, n_frames, seed_idx=None):
        cos_t_max = np.cos(self.rmin_deg * np.pi / 180)
        order = np.arange(len(poses))
        if seed_idx is not None:
            order = np.roll(order, seed_idx)
        kept = [order[0]]
        for i in order[1:]:
            last, cand = poses[kept[-1]], poses[i]
            cos_t = np.sum(last[:3, 2] * cand[:3, 2])
            tdist = np.linalg.norm(last[:3, 3] - cand[:3, 3])
            if tdist > self.tmin or cos_t < cos_t_max:
                kept.append(i)
        return np.asarray(kept)


class EveryNthSelector(FrameSelector):
    """Every interval-th frame from the seed, n_frames of them or as many as the sequence holds."""

    def __init__(self, interval):
        self.interval = interval

    def select_frames(self, poses, n_frames, seed_idx=None):
        n_total = poses.shape[0]
        seed_idx = _seed(seed_idx, n_total, n_frames, self.interval)
        end_idx = min(n_total, seed_idx + self.interval * (n_frames - 1) + 1)
        return np.arange(seed_idx, end_idx, self.interval)
