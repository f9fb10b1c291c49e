"""GPU: the trainable sparse U-Net of 3dvnet_amd/training.py -- ``SparseConv`` / ``sparse_conv`` and ``sparse_unet`` -- on
``SparseUNet(dims=(16, 32, 32), n_groups=(2, 4, 4), n_res=(1, 2, 3))`` over a two-batch map of 400 voxels (three non-empty levels).
Every GroupNorm weight is set to a random non-zero value: the reference initialises ``n2.gn.weight`` to 0, which would silence the
gradient of every first convolution of a residual block.

  * forward: ``level_feats`` against ``xs[i]['feats']`` of the inference forward.  The truth is a stock graph (27 x index_select +
    matmul per convolution, F.group_norm) in float64 on the device, the yardstick e32 the same graph in float32 (max-norm relative
    error per level).  Precision 'fp32': |level_feats - inference| <= 4 e32 max|truth|.  Precision 'split_bf16': both routes run the
    same convolution kernels and differ in the epilogue's rounding only, but the bf16 split is not continuous (a last-bit change
    of an input moves hi + lo by up to 2^-17 of it), so the two chains drift apart at the split's precision, not at fp32's: there
    err(level_feats) <= 4 max(err(inference), e32), both against the truth;
  * gradients of a loss on all three levels: finite and non-zero on F and on every parameter (22 convolution kernels, 2 feat_adj
    kernels, 24 GroupNorm weights and 24 biases: 73 gradients);
  * 'fp32': every gradient's max-norm relative error is at most 4 times the stock float32 graph's own
    (test_training_decoder_gpu.py's rule: different summation orders, not a different algorithm);
    A gradient through a ReLU is not continuous in the forward values: where the argument of a ReLU lies within the forward's
    rounding error of zero, two correct float32 routes can land on either side of the kink and differ by a whole term.  Seed 5, the
    first one tried, has such an argument (6.1e-07 from zero in float64; the HIP route and the stock float32 graph took different
    sides and every gradient upstream of that element differed by about 1e-2).  The seed is therefore chosen on the float64
    stock graph ALONE, on the CPU: the first seed from 5 upwards whose smallest |ReLU argument| exceeds 16 times the stock
    float32 graph's largest error of such an argument is 92 (9.7e-05 against 4.9e-06; seeds 5..91 fall short).  The test asserts
    the precondition with KINK_FACTOR = 8 from its own two stock graphs before it compares anything;
  * 'split_bf16': the input gradients carry about 2^-16 per product, so that ratio does not apply.  The chain has no atomics and is
    deterministic; each gradient's error against the float64 graph was measured on an MI355X: 6.7e-08 .. 7.6e-05 over the 73
    gradients, median 3.1e-05; all 73 values stand in SPLIT_MEASURED below and in DESIGN.md 4.1e, and twice ITS OWN value is
    asserted for every gradient, so that a reordering by a new compiler or library does not fail the test.  Before that the test
    asserts that the split forward (2e-05 .. 4e-05 from float64) puts no ReLU argument on the other side of zero than the float64
    graph: a crossed kink shows errors of 1e-2 that are the data's, not a kernel's.  The weight-gradient kernel itself is exact
    fp32 in both modes;
  * the function node: strided (a slice of a wider row, what ``cat``'s backward hands out) and stride-0 (a ``.sum()``) gradients
    give the bits of their contiguous copies;
  * end to end on the scene of test_training_decoder_gpu.py: ``sparse_unet`` -> ``pointflow_offset(level_feats=...)`` ->
    ``masked_mae``: gradients reach F and every U-Net parameter; ``unet.state_dict()`` keys are unchanged.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_conv_backward_oracle as sco
from conftest import v3d

pytestmark = pytest.mark.gpu

DIMS, GROUPS, N_RES = (16, 32, 32), (2, 4, 4), (1, 2, 3)
N_VOX, SIDE, RES = 400, 8, 0.08
SEED = 92                 # of the GroupNorm affines, the input and the loss; chosen on the float64 stock graph alone (docstring)
# max-norm relative error of every gradient against the float64 stock graph in precision 'split_bf16', measured on an MI355X (the
# test prints them); twice each value is asserted for its own gradient.  The figures were the same, digit for digit, in two processes
SPLIT_MEASURED = {
    'F': 4.654e-05, 'res_down.0.0.n1.gn.weight': 3.065e-05, 'res_down.0.0.n1.gn.bias': 5.454e-05,
    'res_down.0.0.n2.gn.weight': 5.493e-05, 'res_down.0.0.n2.gn.bias': 2.541e-05, 'res_down.0.0.conv1.kernel': 4.160e-05,
    'res_down.0.0.conv2.kernel': 3.350e-05, 'res_down.1.0.n1.gn.weight': 5.932e-05, 'res_down.1.0.n1.gn.bias': 4.227e-05,
    'res_down.1.0.n2.gn.weight': 5.185e-05, 'res_down.1.0.n2.gn.bias': 3.209e-05, 'res_down.1.0.conv1.kernel': 3.718e-05,
    'res_down.1.0.conv2.kernel': 4.586e-05, 'res_down.1.1.n1.gn.weight': 7.612e-05, 'res_down.1.1.n1.gn.bias': 5.860e-05,
    'res_down.1.1.n2.gn.weight': 3.550e-05, 'res_down.1.1.n2.gn.bias': 3.517e-05, 'res_down.1.1.conv1.kernel': 2.224e-05,
    'res_down.1.1.conv2.kernel': 4.076e-05, 'res_down.2.0.n1.gn.weight': 2.429e-05, 'res_down.2.0.n1.gn.bias': 2.815e-05,
    'res_down.2.0.n2.gn.weight': 5.167e-05, 'res_down.2.0.n2.gn.bias': 4.693e-05, 'res_down.2.0.conv1.kernel': 4.197e-05,
    'res_down.2.0.conv2.kernel': 2.190e-05, 'res_down.2.1.n1.gn.weight': 2.725e-05, 'res_down.2.1.n1.gn.bias': 2.738e-05,
    'res_down.2.1.n2.gn.weight': 2.329e-05, 'res_down.2.1.n2.gn.bias': 2.079e-05, 'res_down.2.1.conv1.kernel': 3.623e-05,
    'res_down.2.1.conv2.kernel': 2.346e-05, 'res_down.2.2.n1.gn.weight': 1.989e-05, 'res_down.2.2.n1.gn.bias': 2.440e-05,
    'res_down.2.2.n2.gn.weight': 1.548e-05, 'res_down.2.2.n2.gn.bias': 8.044e-06, 'res_down.2.2.conv1.kernel': 2.351e-05,
    'res_down.2.2.conv2.kernel': 3.046e-05, 'down.0.0.kernel': 4.208e-05, 'down.0.1.gn.weight': 6.048e-05,
    'down.0.1.gn.bias': 5.444e-05, 'down.1.0.kernel': 7.579e-05, 'down.1.1.gn.weight': 3.672e-05, 'down.1.1.gn.bias': 4.177e-05,
    'res_up.0.0.n1.gn.weight': 2.449e-05, 'res_up.0.0.n1.gn.bias': 2.285e-05, 'res_up.0.0.n2.gn.weight': 2.948e-05,
    'res_up.0.0.n2.gn.bias': 1.256e-05, 'res_up.0.0.conv1.kernel': 3.033e-05, 'res_up.0.0.conv2.kernel': 4.215e-05,
    'res_up.0.1.n1.gn.weight': 2.755e-05, 'res_up.0.1.n1.gn.bias': 1.933e-05, 'res_up.0.1.n2.gn.weight': 2.744e-05,
    'res_up.0.1.n2.gn.bias': 4.515e-06, 'res_up.0.1.conv1.kernel': 3.010e-05, 'res_up.0.1.conv2.kernel': 2.047e-05,
    'res_up.1.0.n1.gn.weight': 1.905e-05, 'res_up.1.0.n1.gn.bias': 1.883e-05, 'res_up.1.0.n2.gn.weight': 8.956e-06,
    'res_up.1.0.n2.gn.bias': 6.665e-08, 'res_up.1.0.conv1.kernel': 2.200e-05, 'res_up.1.0.conv2.kernel': 1.874e-05,
    'up.0.0.kernel': 3.614e-05, 'up.0.1.gn.weight': 4.642e-05, 'up.0.1.gn.bias': 3.036e-05, 'up.1.0.kernel': 3.389e-05,
    'up.1.1.gn.weight': 1.548e-05, 'up.1.1.gn.bias': 2.786e-05, 'feat_adj.0.0.kernel': 4.096e-05,
    'feat_adj.0.1.gn.weight': 3.071e-05, 'feat_adj.0.1.gn.bias': 4.411e-05, 'feat_adj.1.0.kernel': 2.418e-05,
    'feat_adj.1.1.gn.weight': 3.095e-05, 'feat_adj.1.1.gn.bias': 3.448e-05,
}
KINK_FACTOR = 8           # the smallest |ReLU argument| of the float64 graph must exceed this many float32 errors of such an argument
_cache = {}


def setup(cuda, precision):
    if precision in _cache:
        return _cache[precision]
    sm = v3d('scenemodeling')
    torch.manual_seed(0)
    unet = sm.SparseUNet(dims=DIMS, n_groups=GROUPS, n_res=N_RES, precision=precision)
    g = torch.Generator().manual_seed(SEED)
    with torch.no_grad():
        for name, p in unet.named_parameters():
            if name.endswith('gn.weight'):
                sign = torch.where(torch.rand(p.shape, generator=g) < 0.5, -1.0, 1.0)
                p.copy_(sign * (0.5 + torch.rand(p.shape, generator=g)))
            elif name.endswith('gn.bias'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    unet = unet.to(cuda)
    c = sco.occupancy_map(N_VOX, SIDE, 21)
    c[:, 1:] += 2
    idx = torch.from_numpy(c[:, 1:]).to(cuda)
    batch = torch.from_numpy(c[:, 0]).to(cuda)
    pts = idx.float() * RES + 0.1
    feats = torch.randn((N_VOX, DIMS[0]), generator=g).to(cuda)
    with torch.no_grad():
        xs = unet(feats, pts, idx, batch, RES)
    assert len(xs) == 3 and [int(x['stride']) for x in xs] == [4, 2, 1] and all(x['feats'].shape[0] > 0 for x in xs)
    assert [x['feats'].shape[1] for x in xs] == [32, 32, 16]
    proj = [torch.randn(x['feats'].shape, generator=g).to(cuda) for x in xs]             # the loss: sum_l <level_l, proj_l> / N_l
    _cache[precision] = dict(unet=unet, feats=feats, xs=xs, proj=proj)
    print('levels: %s rows' % [x['feats'].shape[0] for x in xs])
    return _cache[precision]


def _loss(level_feats, proj):
    return sum((f * p.to(f.dtype)).sum() / f.shape[0] for f, p in zip(level_feats, proj))


def hip_route(s):
    tr = v3d('training')
    feats = s['feats'].clone().requires_grad_(True)
    params = dict(s['unet'].named_parameters())
    level = tr.sparse_unet(s['unet'], feats, s['xs'])
    grads = torch.autograd.grad(_loss(level, s['proj']), [feats] + list(params.values()))
    return [f.detach() for f in level], dict(zip(['F'] + list(params), grads))


def hip_relu_arguments(s):
    """The argument of every ReLU of training.sparse_unet, in call order (the order of stock_route's): F.relu is wrapped while
    the function runs."""
    tr = v3d('training')
    pre, relu = [], F.relu

    def recording(t, *a, **k):
        pre.append(t.detach())
        return relu(t, *a, **k)
    F.relu = recording
    try:
        with torch.no_grad():
            tr.sparse_unet(s['unet'], s['feats'], s['xs'])
    finally:
        F.relu = relu
    return pre


def _stock_conv(x, kernel, nbr):
    """27 x index_select + matmul; row 0 of the padded source is the zero row of an absent neighbour"""
    xp = torch.cat((x.new_zeros((1, x.shape[1])), x), dim=0)
    return sum(xp.index_select(0, nbr[k].long() + 1) @ kernel[k] for k in range(27))


def stock_route(s, dtype):
    """The same function from stock torch ops in ``dtype`` over the same tables (data) -> (level_feats, gradients by name, the
    argument of every ReLU)."""
    unet = s['unet']
    levels = [x['sparse'] for x in s['xs']][::-1]
    n_lv = len(levels)
    same = [lv.neighbors(lv.coords, lv.stride) for lv in levels]
    down = [None] + [levels[i - 1].neighbors(levels[i].coords, levels[i - 1].stride) for i in range(1, n_lv)]
    up = [None] + [levels[i].neighbors(levels[i - 1].coords, -levels[i - 1].stride) for i in range(1, n_lv)]
    P = {k: v.detach().to(dtype).requires_grad_(True) for k, v in unet.named_parameters()}
    feats = s['feats'].detach().to(dtype).requires_grad_(True)
    pre = []                                                    # the argument of every ReLU

    def relu(t):
        pre.append(t.detach())
        return F.relu(t)

    def gn(prefix, mod, y):
        return F.group_norm(y, mod.gn.num_groups, P[prefix + '.gn.weight'], P[prefix + '.gn.bias'], mod.gn.eps)

    def layer(prefix, seq, x, nbr):
        return relu(gn(prefix + '.1', seq[1], _stock_conv(x, P[prefix + '.0.kernel'], nbr)))

    def residual(prefix, blk, x, nbr):
        y = relu(gn(prefix + '.n1', blk.n1, _stock_conv(x, P[prefix + '.conv1.kernel'], nbr)))
        return relu(gn(prefix + '.n2', blk.n2, _stock_conv(y, P[prefix + '.conv2.kernel'], nbr)) + x)

    x = feats
    skips = []
    for i in range(n_lv):
        if i > 0:
            x = layer('down.%d' % (i - 1), unet.down[i - 1], x, down[i])
        for l, blk in enumerate(unet.res_down[i]):
            x = residual('res_down.%d.%d' % (i, l), blk, x, same[i])
        skips.append(x)
    out = [x]
    for j in range(n_lv - 1):
        i = n_lv - 1 - j
        u = layer('up.%d' % j, unet.up[j], x, up[i])
        adj = unet.feat_adj[j]
        x = relu(gn('feat_adj.%d.1' % j, adj[1], torch.cat((u, skips[i - 1]), dim=1) @ P['feat_adj.%d.0.kernel' % j]))
        for l, blk in enumerate(unet.res_up[j]):
            x = residual('res_up.%d.%d' % (j, l), blk, x, same[i - 1])
        out.append(x)
    grads = torch.autograd.grad(_loss(out, s['proj']), [feats] + list(P.values()))
    return [f.detach() for f in out], dict(zip(['F'] + list(P), grads)), pre


def _routes(cuda, precision):
    key = 'routes ' + precision
    if key not in _cache:
        s = setup(cuda, precision)
        _cache[key] = (s, hip_route(s), stock_route(s, torch.float64), stock_route(s, torch.float32))
    return _cache[key]


def kink_margin(pre64, pre32):
    """(smallest |argument of a ReLU| in the float64 graph, largest |float32 - float64| of such an argument)"""
    return (min(float(t.abs().min()) for t in pre64), max(float((a.double() - b).abs().max()) for a, b in zip(pre32, pre64)))


def _rel(a, truth):
    return float((a.double() - truth).abs().max()) / float(truth.abs().max())


@pytest.mark.parametrize('precision', ['fp32', 'split_bf16'])
def test_forward_is_the_inference_forward(precision, cuda):
    s, (level, _), (lv64, _, _), (lv32, _, _) = _routes(cuda, precision)
    assert len(level) == 3
    for i, x in enumerate(s['xs']):
        assert level[i].shape == x['feats'].shape and float(lv64[i].abs().max()) > 0
        e32, e_inf, e_hip = _rel(lv32[i], lv64[i]), _rel(x['feats'], lv64[i]), _rel(level[i], lv64[i])
        diff = float((level[i] - x['feats']).abs().max()) / float(lv64[i].abs().max())
        print('%s level %d: err stock float32 %.3e, err inference %.3e, err sparse_unet %.3e, |sparse_unet - inference| %.3e'
              % (precision, i, e32, e_inf, e_hip, diff))
        if precision == 'fp32':
            assert diff <= 4 * e32, (i, diff, e32)
        else:
            assert e_hip <= 4 * max(e_inf, e32), (i, e_hip, e_inf, e32)


@pytest.mark.parametrize('precision', ['fp32', 'split_bf16'])
def test_gradients_reach_the_input_and_every_parameter(precision, cuda):
    s, (_, grads), _, _ = _routes(cuda, precision)
    names = ['F'] + [n for n, _ in s['unet'].named_parameters()]
    assert list(grads) == names and len(names) == 73
    assert sum(n.endswith('kernel') for n in names) == 24 and sum(n.endswith('gn.weight') for n in names) == 24
    for name, g in grads.items():
        assert bool(torch.isfinite(g).all()), name
        assert bool((g != 0).any()), name


def test_fp32_gradients_match_the_stock_graph_in_float64(cuda):
    """err(x) = max |g_x - g_64| / max |g_64| per gradient; err(HIP route) <= 4 err(stock float32 graph).

    Measured on an MI355X (seed 92): the ratio is 0.44 .. 2.85 over the 73 gradients, median 1.09; the largest are
    res_down.0.0.n2.gn.weight 2.85 (2.31e-06 against 8.09e-07), feat_adj.0.0.kernel 2.08, down.1.1.gn.weight 1.84.  The HIP route's
    errors lie between 6.7e-08 and 2.6e-06, the stock float32 graph's between 6.7e-08 and 2.1e-06.

    With the forward of a convolution as ONE 27-offset call the same measurement gave 0.53 .. 4.80, median 1.58, and this test
    failed on feat_adj.1.1.gn.bias (3.26e-06 against 6.79e-07).  The cause was found by exchanging the halves of the function node
    for stock ops: stock forward + HIP backward 1.13 median, 1.89 at most; HIP forward + stock backward 1.47 and 5.02.  The
    exact-fp32 kernel adds the 27 x Ci products of an output into one accumulator in sequence, and GroupNorm's backward carries the
    forward's error into every gradient.  Precision 'fp32' now runs the forward as nine calls of three offsets whose partial results
    are added pairwise (training.SparseConv): feat_adj.1.1.gn.bias is at 7.27e-07, ratio 1.07, and the level features are 6.0e-07 ..
    7.8e-07 from float64 (before: 1.0e-06 .. 1.4e-06; the stock graph 5.3e-07 .. 9.1e-07)."""
    s, (_, g_hip), (_, g64, pre64), (_, g32, pre32) = _routes(cuda, 'fp32')
    margin, err32 = kink_margin(pre64, pre32)
    print('smallest |ReLU argument| in float64 %.3e, largest float32 error of a ReLU argument %.3e' % (margin, err32))
    assert margin > KINK_FACTOR * err32, 'SEED puts a ReLU argument within rounding of its kink: choose another (module docstring)'
    failed = []
    for name in g64:
        scale = float(g64[name].abs().max())
        assert scale > 0
        e_hip = float((g_hip[name].double() - g64[name]).abs().max()) / scale
        e_32 = float((g32[name].double() - g64[name]).abs().max()) / scale
        print('%-28s err HIP route = %.3e, err stock float32 = %.3e, ratio %.2f' % (name, e_hip, e_32, e_hip / e_32 if e_32 else np.inf))
        if not e_hip <= 4 * e_32:
            failed.append((name, e_hip, e_32))
    assert not failed, failed


def test_split_bf16_gradients_stay_within_twice_the_measured_error(cuda):
    """Every gradient's error against the float64 graph is at most twice the value measured for THAT gradient (SPLIT_MEASURED).
    Before anything is compared: no argument of a ReLU of the HIP route lies on the other side of zero than in the float64 graph.
    The split forward is 2e-05 .. 4e-05 from float64 and the smallest |ReLU argument| of the float64 graph is 9.7e-05: a toolchain
    that moves the split forward can cross a kink, and the errors of 1e-2 that follow are the test's data, not a kernel's."""
    s = setup(cuda, 'split_bf16')
    _, (_, g_hip), (_, g64, pre64), (_, g32, _) = _routes(cuda, 'split_bf16')
    pre_hip = hip_relu_arguments(s)
    assert len(pre_hip) == len(pre64) and all(a.shape == b.shape for a, b in zip(pre_hip, pre64))
    margin = min(float(t.abs().min()) for t in pre64)
    err = max(float((a.double() - b).abs().max()) for a, b in zip(pre_hip, pre64))
    flipped = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(pre_hip, pre64))
    print('smallest |ReLU argument| in float64 %.3e, largest error of a ReLU argument of the HIP route %.3e, arguments on the other '
          'side of zero: %d' % (margin, err, flipped))
    assert flipped == 0, 'the split forward crosses %d ReLU kinks with SEED = %d: choose another seed (module docstring)' % (flipped, SEED)
    assert list(g64) == list(SPLIT_MEASURED)
    failed = []
    for name in g64:
        scale = float(g64[name].abs().max())
        assert scale > 0
        e_hip = float((g_hip[name].double() - g64[name]).abs().max()) / scale
        e_32 = float((g32[name].double() - g64[name]).abs().max()) / scale
        print('%-28s err HIP route = %.3e, err stock float32 = %.3e, measured %.3e' % (name, e_hip, e_32, SPLIT_MEASURED[name]))
        if not e_hip <= 2 * SPLIT_MEASURED[name]:
            failed.append((name, e_hip, SPLIT_MEASURED[name]))
    assert not failed, failed


def test_two_backward_passes_give_the_same_bits(cuda):
    s = setup(cuda, 'split_bf16')
    _, a = hip_route(s)
    _, b = hip_route(s)
    assert all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('precision', ['fp32', 'split_bf16'])
def test_function_handles_strided_and_expanded_gradients(precision, cuda):
    tr = v3d('training')
    s = setup(cuda, precision)
    lv = s['xs'][-1]['sparse']                                                  # the finest level
    nbr = lv.neighbors(lv.coords, lv.stride)
    inv = nbr.flip(0).contiguous()
    g = torch.Generator().manual_seed(8)
    x = torch.randn((lv.n, 16), generator=g).to(cuda).requires_grad_(True)
    w = (0.2 * torch.randn((27, 16, 32), generator=g)).to(cuda).requires_grad_(True)
    y = tr.sparse_conv(x, w, nbr, inv, precision)
    with torch.no_grad():                                                       # the forward is the inference kernel's convolution
        ref = _stock_conv(x.double(), w.double(), nbr)
    assert y.shape == (lv.n, 32) and _rel(y.detach(), ref) < (1e-5 if precision == 'fp32' else 1e-4)
    gy = torch.randn((lv.n, 32), generator=g).to(cuda)
    want = torch.autograd.grad(y, (x, w), gy, retain_graph=True)
    # through cat: the gradient of `y` is a view with row stride 48 at column 16
    other = torch.zeros((lv.n, 16), device=cuda, requires_grad=True)
    wide = torch.full((lv.n, 48), float('nan'), device=cuda)
    wide[:, 16:] = gy
    got = torch.autograd.grad(torch.cat((other, y), dim=1), (x, w), wide, retain_graph=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    # a .sum() upstream: a stride-0 expanded gradient of ones
    ones = torch.autograd.grad(y, (x, w), torch.ones_like(y), retain_graph=True)
    got = torch.autograd.grad(y.sum(), (x, w), retain_graph=True)
    assert torch.equal(got[0], ones[0]) and torch.equal(got[1], ones[1])
    # only one side asked for
    assert torch.equal(torch.autograd.grad(y, x, gy, retain_graph=True)[0], want[0])
    assert torch.equal(torch.autograd.grad(y, w, gy, retain_graph=True)[0], want[1])


def test_end_to_end_loss_reaches_the_unet(cuda):
    import test_training_decoder_gpu as tdg
    tr = v3d('training')
    s = tdg.scene(cuda)
    net = s['net']
    unet = net.sparse_conv
    keys = list(unet.state_dict())
    seen = {}
    hook = unet.register_forward_pre_hook(lambda mod, args: seen.update(F=args[0]))
    try:
        with torch.no_grad():
            xs = net.model_scene(s['depth'], s['depth_batch'], s['feat'], s['rot'], s['tv'], s['K'], s['edges'])
    finally:
        hook.remove()
    feats = seen['F'].detach().clone().requires_grad_(True)
    level = tr.sparse_unet(unet, feats, xs)                                     # (the synthetic GroupNorm weights are non-zero)
    assert [f.shape for f in level] == [x['feats'].shape for x in xs]
    off = tr.pointflow_offset(net.decoder, xs, s['depth'], s['depth_batch'], s['feat'], *tdg._geometry(s), level_feats=level)
    loss = tr.masked_mae(s['depth'] + off, s['gt'], tdg.INTERVAL)
    params = dict(unet.named_parameters())
    assert all(float(v.abs().max()) > 0 for k, v in params.items() if k.endswith('gn.weight'))
    grads = torch.autograd.grad(loss, [feats] + list(params.values()))
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    for name, g in zip(['F'] + list(params), grads):
        assert bool(torch.isfinite(g).all()) and bool((g != 0).any()), name
    assert list(unet.state_dict()) == keys and len(params) == 72
