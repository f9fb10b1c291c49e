"""Float64 oracle of the gradient of the plane-sweep variance with respect to the features.  TEST HELPER, no product code.

The sample positions are the fp32 positions of ``oracle/pinned.py`` (``world_points`` / ``sample_positions``: the orders the
HIP kernels implement bit for bit), promoted to float64; everything after them -- floor, weights, blends, mean, gradient,
scatter -- is float64.  For every element i of ``grad_feat`` [n_img, C, Hf, Wf]:

  g64_i   the gradient;
  N_i     the number of (voxel, edge, tap) contributions to element i (in-image taps);
  M_i     sum over those contributions of  w_tap |gV| (2 / cnt) (A_e + mean_e A_e),  A_e = the bilinear blend of |feat|:
          a bound of the sum of the ABSOLUTE contributions that also holds under the cancellation in x_e - avg.

``variant`` selects deliberately wrong gradients (tests/test_psv_backward_oracle.py shows the acceptance bound rejects them).
"""
import importlib

import torch

from oracle import pinned as pin

U = 2.0 ** -24          # unit roundoff of fp32
CASES = [(16, 'rotated'), (32, 'rotated'), (32, 'sliding')]      # (C, cameras) of make_case


def make_case(C, cameras='rotated', seed=3):
    """The shapes and edge list of tests/test_psv_backward_gpu.py: image 32 x 40, features 8 x 10, D = 8, plane grid 7 x 9 (odd,
    no multiple of a tile), 5 images; references 0, 1, 2 with 1, 3 and 4 edges in interleaved order; image 1 is a source of
    references 1 and 2 and a reference itself; image 4 is in no edge.  cameras='rotated': the A_tiny_rotated fixture's kind
    (45 degrees of yaw per view): mirrored samples (|z| + 1e-8), samples partly outside, sources wholly outside for a range
    of planes.  cameras='sliding': the overlapping views of a sliding window (most samples inside, many contributions per
    texel)."""
    syn = importlib.import_module('3dvnet_amd.synthetic')
    img_size, feat_size, plane_size = (32, 40), (8, 10), (7, 9)
    rot, tv, K = (syn.make_cameras(5, img_size, seed=5, yaw_step_deg=45.0) if cameras == 'rotated' else
                  syn.make_cameras(5, img_size, seed=11))
    feat = syn.make_features(5, C, *feat_size, seed=seed) * 2 - 1
    edges = torch.tensor([[1, 2, 0, 1, 2, 2, 1, 2], [0, 1, 0, 1, 2, 3, 2, 0]], dtype=torch.long)
    g = torch.Generator().manual_seed(seed + 100)
    gvar = torch.randn((3, C, 8) + plane_size, generator=g, dtype=torch.float32)
    return dict(feat=feat, rotmats=rot, tvecs=tv, K=K, edges=edges, depth=(0.5, 0.25, 8), img_size=img_size,
                plane_size=plane_size, gvar=gvar)


def positions(case):
    """[(ref row r, source image, ix float32 [N], iy float32 [N])] in CSR order (references sorted, edges in list order)."""
    K, R, t, edges = case['K'], case['rotmats'], case['tvecs'], case['edges']
    start, interval, D = case['depth']
    _, P = pin.camera_blocks(K, R, t)
    Hf, Wf = case['feat'].shape[2:]
    out = []
    for r, ref in enumerate(torch.unique(edges[0]).tolist()):
        X = pin.world_points(K, R, t, ref, start, interval, D, case['img_size'], case['plane_size'])
        for src in edges[1][edges[0] == ref].tolist():
            ix, iy = pin.sample_positions(X, P[src], case['img_size'], (Hf, Wf))
            out.append((r, src, ix, iy))
    return out


def _taps(ix, iy, Hf, Wf):
    """-> [(weight f64 [N] (0 where the tap is outside the image), flat index long [N], inside bool [N])] for nw, ne, sw, se."""
    ix, iy = torch.nan_to_num(ix.double(), nan=-1e9), torch.nan_to_num(iy.double(), nan=-1e9)
    x0, y0 = torch.floor(ix), torch.floor(iy)
    x1, y1 = x0 + 1, y0 + 1
    wx0, wx1, wy0, wy1 = x1 - ix, ix - x0, y1 - iy, iy - y0
    out = []
    for w, yy, xx in ((wx0 * wy0, y0, x0), (wx1 * wy0, y0, x1), (wx0 * wy1, y1, x0), (wx1 * wy1, y1, x1)):
        ok = (xx >= 0) & (xx <= Wf - 1) & (yy >= 0) & (yy <= Hf - 1)
        idx = (yy.clamp(0, Hf - 1) * Wf + xx.clamp(0, Wf - 1)).long()
        out.append((torch.where(ok, w, torch.zeros_like(w)), idx, ok))
    return out


def gradient(case, gvar=None, variant=None):
    """-> dict(g64, N, M), each [n_img, C, Hf, Wf] float64.  ``gvar`` [n_ref, C, D, h, w] (default: the case's).
    variant: None | 'no_avg' (the -avg term dropped) | 'global_cnt' (cnt = all edges of the batch) | 'swap_ne_sw'."""
    feat = case['feat'].double()
    n_img, C, Hf, Wf = feat.shape
    gv = (case['gvar'] if gvar is None else gvar).double().reshape(-1, C, case['depth'][2] * case['plane_size'][0] * case['plane_size'][1])
    flat, aflat = feat.reshape(n_img, C, Hf * Wf), feat.abs().reshape(n_img, C, Hf * Wf)
    g64, M = torch.zeros_like(flat), torch.zeros_like(flat)
    N = torch.zeros((n_img, Hf * Wf), dtype=torch.float64)
    pos = positions(case)
    for r in sorted({p[0] for p in pos}):
        mine = [p for p in pos if p[0] == r]
        cnt = float(len(pos) if variant == 'global_cnt' else len(mine))
        taps = [_taps(ix, iy, Hf, Wf) for _, _, ix, iy in mine]
        if variant == 'swap_ne_sw':
            taps = [[tp[0], (tp[1][0], tp[2][1], tp[2][2]), (tp[2][0], tp[1][1], tp[1][2]), tp[3]] for tp in taps]
        xs = [sum(w[None] * flat[src][:, idx] for w, idx, _ in tp) for (_, src, _, _), tp in zip(mine, taps)]
        As = [sum(w[None] * aflat[src][:, idx] for w, idx, _ in tp) for (_, src, _, _), tp in zip(mine, taps)]
        avg, Aavg = sum(xs) / cnt, sum(As) / cnt
        for (_, src, _, _), tp, x, A in zip(mine, taps, xs, As):
            ge = gv[r] * 2.0 * (x if variant == 'no_avg' else x - avg) / cnt
            me = gv[r].abs() * (2.0 / cnt) * (A + Aavg)
            for w, idx, ok in tp:
                g64[src].index_add_(1, idx, w[None] * ge)
                M[src].index_add_(1, idx, w[None] * me)
                N[src].index_add_(0, idx, ok.double())
    shape = (n_img, C, Hf, Wf)
    return dict(g64=g64.reshape(shape), M=M.reshape(shape), N=N[:, None].expand(n_img, C, Hf * Wf).reshape(shape).clone())


def bound(orc):
    """The acceptance bound of the HIP gradient, per element: (N + 32) 2^-24 M -- N additions in any order, and at most 32
    roundings per contribution (two 4-tap blends, a mean of at most 9 terms, the subtraction, three products)."""
    return (orc['N'] + 32.0) * U * orc['M']


def violations(g, orc):
    """-> (number of elements of ``g`` outside the bound, worst |g - g64| / bound over the elements with a non-zero bound,
    worst |g - g64| over the elements whose bound is zero)."""
    err, b = (g.detach().double().cpu() - orc['g64']).abs(), bound(orc)
    bad = int((~(err <= b)).sum())
    nz = b > 0
    worst = float((err[nz] / b[nz]).max()) if nz.any() else 0.0
    return bad, worst, float(err[~nz].max()) if (~nz).any() else 0.0


def autograd_reference(case):
    """d sum(var * gvar) / d feat by torch.autograd through the stock-torch oracle chain of oracle/costvolume.py (its own fp32
    positions from torch.bmm), features in float64 and the sampling grid cast to float64."""
    import torch.nn.functional as F
    from oracle import costvolume as cv
    feat = case['feat'].double().requires_grad_(True)
    edges = case['edges']
    start, interval, D = case['depth']
    ref_idx, gather_idx = torch.unique(edges[0], return_inverse=True)
    pts = cv.plane_sweep_points(start, interval, D, case['rotmats'], case['tvecs'], case['K'], case['img_size'], case['plane_size'])
    grid = cv.project_to_grid(pts[edges[0]], case['rotmats'], case['tvecs'], case['K'], edges[1], case['img_size'])
    x = F.grid_sample(feat[edges[1]], grid.double(), mode='bilinear', align_corners=True)
    x = x.squeeze(3).view(-1, feat.shape[1], D, *case['plane_size'])
    var = cv.scatter_mean(x ** 2, gather_idx, len(ref_idx)) - cv.scatter_mean(x, gather_idx, len(ref_idx)) ** 2
    return torch.autograd.grad((var * case['gvar'].double()).sum(), feat)[0]
