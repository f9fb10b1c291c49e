"""Float64 oracle of the gradient of the plane-sweep variance with respect to the features.  TEST HELPER, no product code.

The sample positions are the fp32 positions of ``oracle/pinned.py`` (``world_points`` / ``sample_positions``: the orders the
HIP kernels implement bit for bit), promoted to float64; everything after them -- floor, weights, blends, mean, gradient,
scatter -- is float64.  For every element i of ``grad_feat`` [n_img, C, Hf, Wf]:

  g64_i   the gradient;
  N_i     the number of (voxel, edge, tap) contributions to element i (in-image taps);
  M_i     sum over those contributions of  w_tap |gV| (2 / cnt) (A_e + mean_e A_e),  A_e = the bilinear blend of |feat|:
          a bound of the sum of the ABSOLUTE contributions that also holds under the cancellation in x_e - avg.

``variant`` selects deliberately wrong gradients (tests/test_psv_backward_oracle.py shows the acceptance bound rejects them).

Two families of cases: ``CASES`` (``make_case``: at most 4 edges per reference, one depth segment) and ``CHUNK_CASES``
(``make_chunk_case``: 8, 9 and 17 edges per reference and 33 planes -- the kernel keeps the tap records of ``CHUNK`` = 8 edges in
LDS and walks ``SEGMENT`` = 16 planes per workgroup, so these cross both boundaries).  ``build(param)`` makes either.
"""
import importlib

import torch

from oracle import pinned as pin

U = 2.0 ** -24          # unit roundoff of fp32
CASES = [(16, 'rotated'), (32, 'rotated'), (32, 'sliding')]      # (C, cameras) of make_case
CHUNK = 8               # edges whose tap records both kernels keep in LDS at a time (csrc/variance_backward.h: kBwdMaxE)
SEGMENT = 16            # depth planes per workgroup (csrc/psv_backward.hip: kBDS)
CHUNK_CASES = [('chunk', 16, 'rotated'), ('chunk', 16, 'dense'), ('chunk', 32, 'rotated'), ('chunk', 32, 'dense')]
CHUNK_VARIANTS = ('avg_first_chunk', 'drop_later_chunks', 'stale_records', 'first_segment', 'tail_plane')


def case_id(param):
    return '-'.join(str(x) for x in param)


def build(param):
    """A member of CASES or CHUNK_CASES -> its case."""
    return make_chunk_case(*param[1:]) if param[0] == 'chunk' else make_case(*param)


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
                plane_size=plane_size, gvar=gvar, unused=4)


def make_chunk_case(C, cameras='dense', edge_counts=(8, 9, 17), D=33, plane_size=(5, 7), n_img=19, seed=10):
    """Cases that cross the kernel's edge chunks (8 edges) and depth segments (16 planes): image 32 x 40, features 8 x 10,
    plane grid 5 x 7 (35 pixels, no multiple of the 2 or 4 pixels of a wave), D = 33 planes 0.125 apart from 0.5 (three
    segments, the last with one live plane), 19 images.  Reference r (image r) has ``edge_counts[r]`` edges -- 8, 9, 17: exactly
    one chunk, 8 + 1, 8 + 8 + 1 -- whose sources are drawn without repetition from images 0 .. n_img - 2; the last image is in no
    edge.  The edge list is shuffled, so the CSR order (references sorted, list order within a reference) is not the list order.
    cameras='rotated': 45 degrees of yaw per view as in make_case (mirrored samples, most samples outside);
    cameras='dense': 2 degrees per view, every edge has in-image taps on a good part of its samples, so every chunk carries
    gradient (with make_cameras' default of 6 degrees most edges of the later chunks are wholly outside).
    ``seed`` draws the features, the edges and gvar.  With 'rotated' a source sees its reference only when their yaws are at most
    one step apart, so which edges land in the later chunks decides how much gradient those chunks carry: seed 10 puts in-image
    edges there (seed 3, make_case's, leaves 'drop_later_chunks' visible on a third of the affected elements only; see
    tests/test_psv_backward_oracle.py)."""
    syn = importlib.import_module('3dvnet_amd.synthetic')
    img_size, feat_size = (32, 40), (8, 10)
    rot, tv, K = (syn.make_cameras(n_img, img_size, seed=5, yaw_step_deg=45.0) if cameras == 'rotated' else
                  syn.make_cameras(n_img, img_size, seed=11, yaw_step_deg=2.0))
    feat = syn.make_features(n_img, C, *feat_size, seed=seed) * 2 - 1
    g = torch.Generator().manual_seed(seed + 200)
    pairs = [(r, int(s)) for r, n in enumerate(edge_counts) for s in torch.randperm(n_img - 1, generator=g)[:n]]
    edges = torch.tensor(pairs, dtype=torch.long)[torch.randperm(len(pairs), generator=g)].t().contiguous()
    gvar = torch.randn((len(edge_counts), C, D) + tuple(plane_size), generator=g, dtype=torch.float32)
    return dict(feat=feat, rotmats=rot, tvecs=tv, K=K, edges=edges, depth=(0.5, 0.125, D), img_size=img_size,
                plane_size=tuple(plane_size), gvar=gvar, unused=n_img - 1)


def make_strip_case(seed=3):
    """The widest feature map the entry point accepts: one strip Hf = 2, Wf = 32759, C = 16, two images (8 MB), each the
    reference of two edges (itself and the other), D = 2, plane grid 3 x 64, two views 2 degrees of yaw apart over an image of
    8 x 1024 pixels: the samples spread over the whole width, so the tap records carry columns far above 8 and 14 bits."""
    syn = importlib.import_module('3dvnet_amd.synthetic')
    img_size, feat_size, plane_size = (8, 1024), (2, 32759), (3, 64)
    rot, tv, K = syn.make_cameras(2, img_size, seed=11, yaw_step_deg=2.0)
    feat = syn.make_features(2, 16, *feat_size, seed=seed) * 2 - 1
    edges = torch.tensor([[0, 1, 1, 0], [0, 1, 0, 1]], dtype=torch.long)
    g = torch.Generator().manual_seed(seed + 300)
    gvar = torch.randn((2, 16, 2) + plane_size, generator=g, dtype=torch.float32)
    return dict(feat=feat, rotmats=rot, tvecs=tv, K=K, edges=edges, depth=(0.5, 0.25, 2), img_size=img_size,
                plane_size=plane_size, gvar=gvar, unused=None)


def block_count(case):
    """Workgroups of the backward launch, computed as the entry point does: n_ref * ceil(h w / (64 / C)) * ceil(D / 16)."""
    C, P, D = case['feat'].shape[1], case['plane_size'][0] * case['plane_size'][1], case['depth'][2]
    ppw = 64 // C
    return len(torch.unique(case['edges'][0])) * ((P + ppw - 1) // ppw) * ((D + SEGMENT - 1) // SEGMENT)


def tap_columns(case):
    """Columns of all in-image taps of all samples, long [n]."""
    Hf, Wf = case['feat'].shape[2:]
    return torch.cat([idx[ok] % Wf for _, _, ix, iy in positions(case) for _, idx, ok in _taps(ix, iy, Hf, Wf)])


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
    """-> dict(g64, N, M), each [n_img, C, Hf, Wf] float64, and cnt_max, the largest edge count of a reference.  ``gvar``
    [n_ref, C, D, h, w] (default: the case's).
    variant: None | the variants of ``variance_gradient`` | the bugs along the plane axis:
      'first_segment'      planes d >= 16 contribute nothing;
      'tail_plane'         plane D - 1 contributes nothing."""
    C = case['feat'].shape[1]
    D, n_pix = case['depth'][2], case['plane_size'][0] * case['plane_size'][1]
    gv = (case['gvar'] if gvar is None else gvar).double().reshape(-1, C, D, n_pix)
    if variant in ('first_segment', 'tail_plane'):
        gv = gv.clone()
        gv[:, :, (SEGMENT if variant == 'first_segment' else D - 1):] = 0.0
    return variance_gradient(positions(case), gv.reshape(-1, C, D * n_pix), case['feat'], variant)


def variance_gradient(pos, gv, feat, variant=None, dtype=torch.float64):
    """The core both oracles share (tests/backproject_backward_oracle.py calls it with its own positions and upstream gradient).
    ``pos``: a positions list [(ref row r, source image, ix, iy)] in CSR order; ``gv`` [n_ref, C, samples] float64, the upstream
    gradient in the sample order of ``pos`` (the caller has applied the variants of its own axis); ``feat`` [n_img, C, Hf, Wf].
    -> dict(g64, N, M) and cnt_max as ``gradient`` documents.  ``dtype=torch.float32``: the same taps and weights evaluated with
    float32 torch ops (g64 is then that float32 gradient; N and M stay float64).
    variant: None or another name (nothing to do here) | 'no_avg' (the -avg term dropped) | 'global_cnt' (cnt = all edges of the
    batch) | 'swap_ne_sw', and the bugs a chunked kernel could have (chunk membership by CSR position k within the reference):
      'avg_first_chunk'    avg is summed over positions 0 .. 7 only, then divided by the full cnt;
      'drop_later_chunks'  edges at position 8 or higher scatter nothing;
      'stale_records'      an edge at position k >= 8 samples (its own source image) and scatters with the taps -- weights, cells,
                           validity -- of the edge at position k % 8."""
    feat = feat.double()
    n_img, C, Hf, Wf = feat.shape
    flat, aflat = feat.reshape(n_img, C, Hf * Wf), feat.abs().reshape(n_img, C, Hf * Wf)
    fl = flat.to(dtype)
    g, M = torch.zeros_like(fl), torch.zeros_like(flat)
    N = torch.zeros((n_img, Hf * Wf), dtype=torch.float64)
    cnt_max = 0
    for r in sorted({p[0] for p in pos}):
        mine = [p for p in pos if p[0] == r]
        cnt_max = max(cnt_max, len(mine))
        cnt = float(len(pos) if variant == 'global_cnt' else len(mine))
        taps = [_taps(ix, iy, Hf, Wf) for _, _, ix, iy in mine]
        if variant == 'swap_ne_sw':
            taps = [[tp[0], (tp[1][0], tp[2][1], tp[2][2]), (tp[2][0], tp[1][1], tp[1][2]), tp[3]] for tp in taps]
        if variant == 'stale_records':
            taps = [taps[k % CHUNK] if k >= CHUNK else tp for k, tp in enumerate(taps)]
        xs = [sum(w[None].to(dtype) * fl[src][:, idx] for w, idx, _ in tp) for (_, src, _, _), tp in zip(mine, taps)]
        As = [sum(w[None] * aflat[src][:, idx] for w, idx, _ in tp) for (_, src, _, _), tp in zip(mine, taps)]
        avg, Aavg = sum(xs[:CHUNK] if variant == 'avg_first_chunk' else xs) / cnt, sum(As) / cnt
        for k, ((_, src, _, _), tp, x, A) in enumerate(zip(mine, taps, xs, As)):
            if variant == 'drop_later_chunks' and k >= CHUNK:
                continue
            ge = gv[r].to(dtype) * 2.0 * (x if variant == 'no_avg' else x - avg) / cnt
            me = gv[r].abs() * (2.0 / cnt) * (A + Aavg)
            for w, idx, ok in tp:
                g[src].index_add_(1, idx, w[None].to(dtype) * ge)
                M[src].index_add_(1, idx, w[None] * me)
                N[src].index_add_(0, idx, ok.double())
    shape = (n_img, C, Hf, Wf)
    return dict(g64=g.reshape(shape), M=M.reshape(shape), N=N[:, None].expand(n_img, C, Hf * Wf).reshape(shape).clone(),
                cnt_max=cnt_max)


def affected_images(case, variant, pos=None):
    """bool [n_img]: the images whose gradient a wrong-gradient variant can change -- for 'avg_first_chunk' the sources of the
    references with more than one chunk, for 'drop_later_chunks' / 'stale_records' their sources at CSR position 8 or higher,
    for every other variant (the plane variants here) all sources of a reference.  ``pos``: the positions list (default: this
    module's ``positions(case)``)."""
    pos = positions(case) if pos is None else pos
    mask = torch.zeros(case['feat'].shape[0], dtype=torch.bool)
    for r in sorted({p[0] for p in pos}):
        srcs = [p[1] for p in pos if p[0] == r]
        if variant not in ('avg_first_chunk', 'drop_later_chunks', 'stale_records'):
            mask[srcs] = True
        elif len(srcs) > CHUNK:
            mask[srcs if variant == 'avg_first_chunk' else srcs[CHUNK:]] = True
    return mask


def bound(orc):
    """The acceptance bound of the HIP gradient, per element: (N + c) 2^-24 M -- N additions in any order, and at most c
    roundings per contribution, c = 32 + max(0, cnt_max - 9) with cnt_max the largest edge count of a reference in the batch.
    The 32 are two 4-tap blends, a mean of at most 9 terms, the subtraction and three products.  A mean of cnt terms is cnt - 1
    additions and a division, each one rounding relative to a partial sum that M's (A_e + mean_e A_e) bounds; the 32 hold 9 of
    them, so every term past the ninth adds one: with 17 edges c = 40.  c = 32 for every case of at most 9 edges per reference."""
    return (orc['N'] + 32.0 + max(0, orc['cnt_max'] - 9)) * U * orc['M']


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
