"""Float64 oracle of the two gradients of the back-projected variance (csrc/backproject_backward.hip): var -> features and, for
n = 0, pts -> depth.  TEST HELPER, no product code.  The feature gradient is tests/psv_backward_oracle.py's core (variance_gradient: both
kernels are one walk, csrc/variance_backward.h) on this operation's positions; its taps, bound and cases are reused as well.

The sample positions are the fp32 positions of ``oracle/pinned.py`` (``backproject_points`` at depth + i * offset for i = -n .. n,
then ``sample_positions``: the orders the forward kernel implements bit for bit), promoted to float64; everything after them is
float64.  Layouts: ``gvar`` [n_ref * P, n_hyp, C], ``gpts`` [n_ref * P, 1, 3], the sample index within a reference is
pixel * n_hyp + hypothesis.

``gradient`` returns g64, N, M, cnt_max of ``pbo.variance_gradient``, so ``pbo.bound`` -- (N + 32 + max(0, cnt_max - 9))
2^-24 M -- and ``pbo.violations`` apply; the derivation in ``pbo.bound``'s docstring carries over term for term (the hypothesis axis
plays the role of the plane axis).  ``depth_gradient`` returns (g64, M_d) with M_d = sum_j |gp_j| sum_i |R_ij| sum_k |Kinv_ik| |p_k|;
its bound is 16 * 2^-24 * M_d: nine roundings in three nested 3-term chains, plus slack.
"""
import importlib

import numpy as np
import torch

import psv_backward_oracle as pbo
from oracle import pinned as pin

U = pbo.U
SEGMENT = 8             # hypotheses per workgroup with n > 0 (csrc/backproject_backward.hip: the S of its launch)
CASES = [(C, cam, n) for n in (3, 0) for C, cam in ((16, 'rotated'), (32, 'rotated'), (32, 'sliding'))]
CHUNK_CASES = [('chunk', C, cam, 4) for C in (16, 32) for cam in ('rotated', 'dense')]
SEGMENT_CASES = [('chunk', 32, 'dense', n) for n in (0, 1, 3, 7, 8, 16)]      # 1, 3, 7, 15, 17, 33 hypotheses
ALL_CASES = CASES + CHUNK_CASES + SEGMENT_CASES
BASE_VARIANTS = ('no_avg', 'global_cnt', 'swap_ne_sw', 'tail_hyp', 'centre_only', 'reversed_hyp')
CHUNK_VARIANTS = ('avg_first_chunk', 'drop_later_chunks', 'stale_records', 'tail_hyp', 'first_segment')
DEPTH_VARIANTS = ('R_not_RT', 'drop_z')

case_id = pbo.case_id


def build(param):
    return make_chunk_case(*param[1:]) if param[0] == 'chunk' else make_case(*param)


def _finish(base, plane_size, n, offset, seed):
    """Cameras, features and edges of a pbo case + the depth maps and the upstream gradients of this operation."""
    syn = importlib.import_module('3dvnet_amd.synthetic')
    refs = torch.unique(base['edges'][0])
    g = torch.Generator().manual_seed(seed)
    depth = syn.ray_box_depth(base['rotmats'][refs], base['tvecs'][refs], base['K'][refs], base['img_size'], plane_size)
    depth = (depth * (1 + 0.1 * torch.randn(depth.shape, generator=g))).float()
    depth[-1, 0, 0] = 0.1               # the lowest hypotheses are negative: behind the camera
    depth[-1, 0, 1] = 0.0
    depth[-1, 0, 2] = float('nan')      # no position, no tap
    rows, C = depth.numel(), base['feat'].shape[1]
    gvar = torch.randn((rows, 2 * n + 1, C), generator=g, dtype=torch.float32)
    gpts = torch.randn((rows, 1, 3), generator=g, dtype=torch.float32)
    return dict(feat=base['feat'], rotmats=base['rotmats'], tvecs=base['tvecs'], K=base['K'], edges=base['edges'],
                img_size=base['img_size'], depth_map=depth, offset=float(offset), n=int(n), gvar=gvar, gpts=gpts,
                unused=base['unused'])


def make_case(C, cameras='rotated', n=3, offset=0.05, seed=3):
    """pbo.make_case's images, features (8 x 10) and edges -- 5 images, references 0, 1, 2 with 1, 3, 4 edges, image 4 in no edge --
    with a 7 x 9 depth map per reference: ray_box_depth * (1 + 0.1 randn), and three special pixels on the last reference."""
    return _finish(pbo.make_case(C, cameras, seed=seed), (7, 9), n, offset, seed + 100)


def make_chunk_case(C, cameras='dense', n=4, edge_counts=(8, 9, 17), offset=0.05, seed=10):
    """pbo.make_chunk_case's 19 images and shuffled edges (8, 9 and 17 per reference, the last image in no edge) with 5 x 7 depth
    maps: the references cross the kernel's chunks of 8 edges, and n chooses the number of hypotheses around its segment of 8."""
    base = pbo.make_chunk_case(C, cameras, edge_counts=edge_counts, D=1, plane_size=(5, 7), n_img=19, seed=seed)
    return _finish(base, (5, 7), n, offset, seed + 300)


def make_strip_case(seed=3):
    """pbo.make_strip_case's feature strip (Hf = 2, Wf = 32759, C = 16, two images) with a 3 x 64 depth map and n = 3."""
    return _finish(pbo.make_strip_case(seed=seed), (3, 64), 3, 0.05, seed + 400)


def positions(case):
    """[(ref row r, source image, ix float32 [P * n_hyp], iy)] in CSR order; sample index pixel * n_hyp + hypothesis."""
    K, R, t, edges = case['K'], case['rotmats'], case['tvecs'], case['edges']
    n, offset, depth = case['n'], case['offset'], case['depth_map']
    _, P = pin.camera_blocks(K, R, t)
    Hf, Wf = case['feat'].shape[2:]
    out = []
    for r, ref in enumerate(torch.unique(edges[0]).tolist()):
        X = torch.stack([pin.backproject_points(K[ref:ref + 1], R[ref:ref + 1], t[ref:ref + 1], depth[r:r + 1] + i * offset,
                                                case['img_size'])[0] for i in range(-n, n + 1)], dim=2).reshape(3, -1)
        for src in edges[1][edges[0] == ref].tolist():
            ix, iy = pin.sample_positions(X, P[src], case['img_size'], (Hf, Wf))
            out.append((r, src, ix, iy))
    return out


def tap_columns(case):
    Hf, Wf = case['feat'].shape[2:]
    return torch.cat([idx[ok] % Wf for _, _, ix, iy in positions(case) for _, idx, ok in pbo._taps(ix, iy, Hf, Wf)])


def _per_ref(gvar, n_ref, C):
    """[n_ref * P, n_hyp, C] -> [n_ref, C, P * n_hyp]"""
    n_hyp = gvar.shape[1]
    return gvar.reshape(n_ref, -1, n_hyp, C).permute(0, 3, 1, 2).reshape(n_ref, C, -1)


def gradient(case, gvar=None, variant=None, dtype=torch.float64):
    """-> dict(g64, N, M) [n_img, C, Hf, Wf] and cnt_max, as pbo.gradient: pbo.variance_gradient on this operation's positions and
    upstream gradient.  ``dtype=torch.float32``: the same taps and weights evaluated with float32 torch ops (g64 is then that
    float32 gradient; N and M stay float64).
    variant: None | the variants of pbo.variance_gradient | the bugs along the hypothesis axis:
      'tail_hyp'       the last hypothesis contributes nothing;     'centre_only'   only hypothesis n contributes;
      'reversed_hyp'   gvar is applied in reverse hypothesis order;  'first_segment' hypotheses >= 8 contribute nothing."""
    C = case['feat'].shape[1]
    n_hyp = 2 * case['n'] + 1
    gv = (case['gvar'] if gvar is None else gvar).double().clone()
    if variant == 'tail_hyp':
        gv[:, n_hyp - 1:] = 0.0
    elif variant == 'first_segment':
        gv[:, SEGMENT:] = 0.0
    elif variant == 'centre_only':
        gv[:, :case['n']] = 0.0
        gv[:, case['n'] + 1:] = 0.0
    elif variant == 'reversed_hyp':
        gv = gv.flip(1)
    n_ref = len(torch.unique(case['edges'][0]))
    return pbo.variance_gradient(positions(case), _per_ref(gv, n_ref, C), case['feat'], variant, dtype)


def affected_images(case, variant):
    """pbo.affected_images over this operation's positions (with 'no_avg' and the hypothesis variants a one-edge reference changes
    nothing: its gradient is zero either way, and zero elements are not counted)."""
    return pbo.affected_images(case, variant, positions(case))


bound = pbo.bound
violations = pbo.violations


def _rays(case):
    """Kinv (float64 inverse rounded to fp32), R and p = (x, y, 1) of every reference in float64 -> Kinv [n,3,3], R [n,3,3], p [3,P]"""
    refs = torch.unique(case['edges'][0])
    H, W = case['img_size']
    h, w = case['depth_map'].shape[1:]
    xs = torch.from_numpy(np.linspace(0, W - 1, w, dtype=np.float32)).double()
    ys = torch.from_numpy(np.linspace(0, H - 1, h, dtype=np.float32)).double()
    p = torch.stack((xs[None, :].expand(h, w).reshape(-1), ys[:, None].expand(h, w).reshape(-1), torch.ones(h * w, dtype=torch.float64)))
    Kinv = torch.linalg.inv(case['K'][refs].double()).float().double()
    return Kinv, case['rotmats'][refs].double(), p


def depth_gradient(case, gpts=None, variant=None):
    """-> (g64 [n_ref, h, w], M_d [n_ref, h, w]): grad_depth = sum_j gp_j ray_j, ray = R^T Kinv p.
    variant: None | 'R_not_RT' (ray = R Kinv p) | 'drop_z' (the j = 2 term dropped)."""
    Kinv, R, p = _rays(case)
    n_ref, h, w = case['depth_map'].shape
    gp = (case['gpts'] if gpts is None else gpts).double().reshape(n_ref, h * w, 3)
    c = Kinv @ p                                                             # [n, 3, P]
    ray = (R if variant == 'R_not_RT' else R.transpose(1, 2)) @ c
    Mray = R.abs().transpose(1, 2) @ (Kinv.abs() @ p.abs())
    if variant == 'drop_z':
        ray = ray.clone()
        ray[:, 2] = 0.0
    g = (gp.transpose(1, 2) * ray).sum(dim=1)
    M = (gp.abs().transpose(1, 2) * Mray).sum(dim=1)
    return g.reshape(n_ref, h, w), M.reshape(n_ref, h, w)


def depth_bound(M_d):
    return 16.0 * U * M_d


def depth_violations(g, g64, M_d):
    """-> (pixels outside the bound, worst |g - g64| / bound over the pixels with a non-zero bound)"""
    err, b = (g.detach().double().cpu() - g64).abs(), depth_bound(M_d)
    nz = b > 0
    return int((~(err <= b)).sum()), float((err[nz] / b[nz]).max()) if nz.any() else 0.0


def _grid(ix, iy, Hf, Wf):
    """float64 grid_sample coordinates of pinned positions; a NaN or huge position becomes one far outside the image."""
    ix = torch.nan_to_num(ix.double(), nan=-1e4, posinf=1e4, neginf=-1e4).clamp(-1e4, 1e4)
    iy = torch.nan_to_num(iy.double(), nan=-1e4, posinf=1e4, neginf=-1e4).clamp(-1e4, 1e4)
    return torch.stack((ix / (Wf - 1) * 2 - 1, iy / (Hf - 1) * 2 - 1), dim=-1)[None, :, None]


def autograd_reference(case):
    """d sum(var * gvar) / d feat by float64 torch.autograd through F.grid_sample on the float64 grid made from the pinned
    positions, var = mean_e x^2 - (mean_e x)^2 per reference."""
    import torch.nn.functional as F
    feat = case['feat'].double().requires_grad_(True)
    C, Hf, Wf = feat.shape[1:]
    pos = positions(case)
    n_ref = len(torch.unique(case['edges'][0]))
    gv = _per_ref(case['gvar'].double(), n_ref, C)
    loss = 0.0
    for r in range(n_ref):
        xs = torch.stack([F.grid_sample(feat[src:src + 1], _grid(ix, iy, Hf, Wf), mode='bilinear', padding_mode='zeros',
                                        align_corners=True)[0, :, :, 0] for rr, src, ix, iy in pos if rr == r])
        var = (xs ** 2).mean(dim=0) - xs.mean(dim=0) ** 2
        loss = loss + (var * gv[r]).sum()
    return torch.autograd.grad(loss, feat)[0]


def depth_autograd_reference(case):
    """d sum(pts * gpts) / d depth by float64 autograd through pts = R^T (Kinv (p d) - t)."""
    Kinv, R, p = _rays(case)
    refs = torch.unique(case['edges'][0])
    n_ref, h, w = case['depth_map'].shape
    d = torch.nan_to_num(case['depth_map'].double(), nan=1.0).reshape(n_ref, 1, h * w).requires_grad_(True)
    pts = R.transpose(1, 2) @ (Kinv @ (p[None] * d) - case['tvecs'][refs].double()[:, :, None])       # [n, 3, P]
    loss = (pts.transpose(1, 2) * case['gpts'].double().reshape(n_ref, h * w, 3)).sum()
    return torch.autograd.grad(loss, d)[0].reshape(n_ref, h, w)
