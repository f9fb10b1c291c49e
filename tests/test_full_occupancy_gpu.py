"""Every element of launches that fill the machine, against float64 references.

A 16-byte LDS read that feeds vector instructions beside matrix instructions in flight has returned stale upper lanes three
times in this project: a few wrong elements per launch, always in the same places, only under real occupancy.  A soft-argmin
depth or a small parity test does not see that.  Here the kernels that make the headline number run at production sizes and
every output element is compared:

(a) the regulariser on a 16-view cfg2 volume through the two routes the product takes (split-bf16 ``SplitVariance`` hand-off:
    batched conv0z, conv12z march, split tail, conv9_prob; exact-fp32 ``Cl8Variance``: conv0z<true> + the per-layer kernels)
    against the float64 CostRegNet of the same fp32 volume, and the batched call against one view per call, bit for bit;
(b) stage 3 (csrc/propz.hip) at the sizes of cfg3 -- 64 views at 256 x 320 (4-channel net), 128 x 160 and 64 x 80 (33
    channels), 64 x 80 (17 channels) -- ``forward`` and ``forward_resized``, both operand precisions, against the float64
    PropagationNet after torch's nearest resize;
(c) the same launches 10 times each while fp32 GEMMs run on a second stream: every launch bit-identical to the first.

References are built from torch ops on float64 tensors on the device (oracle/costvolume.py, oracle/scene.py), a view chunk
at a time; no kernel of this library computes any part of them.  A failure reports how many elements fail, the worst one and
where the failures sit by ``x % 64`` and by view, which is what a stale-lane bug looks like.

Bounds, and the largest error measured on MI355X as a fraction of the bound:
  reg, split-bf16  : 5e-5 * max|ref| (the fuzz test's bound)    0.24    depth 1e-4 relative   0.44
  reg, exact fp32  : 1.5e-6 * max|ref|                          0.42    depth 2e-5 relative   0.09
  stage 3          : 2e-5 relative (split-bf16)                 0.018
                     3e-6 relative (fp32), as test_parity_net_gpu  0.124
"""
import collections

import pytest
import torch
import torch.nn.functional as F

from conftest import v3d
from oracle import costvolume as ocv
from oracle import scene as osc
from test_costvolume_gpu import _decode_split, _split_roundtrip

pytestmark = pytest.mark.gpu

N_REF = 16
REG_SPLIT_ATOL = 5e-5          # of max|ref|
# exact-fp32 Cl8 route: measured 6.3e-7 of max|ref| on MI355X (16 views of cfg2); the bound is 2.4x that.  conv0z<true> on
# split-bf16 operands (hi + lo of both) behind precision='fp32' measured 4.0e-6: a split-bf16 kernel in this chain fails it
REG_F32_ATOL = 1.5e-6
DEPTH_SPLIT_RTOL, DEPTH_F32_RTOL = 1e-4, 2e-5
PROP_RTOL = {'split_bf16': 2e-5, 'fp32': 3e-6}
N_LOAD = 10


# ---- reporting ------------------------------------------------------------------------------------------------------------

def _hist(idx, strip):
    """Failing positions by x % 64, by view and, for the row-marching stage-3 kernel, by the column of its 40-wide strip
    (lane = 4 + x % 40)."""
    out = '  failing by x %% 64: %s\n  failing by view: %s' % (dict(sorted(collections.Counter((idx[:, -1] % 64).tolist()).items())),
                                                          dict(sorted(collections.Counter(idx[:, 0].tolist()).items())))
    if strip:
        out += '\n  failing by x %% %d: %s' % (strip, dict(sorted(collections.Counter((idx[:, -1] % strip).tolist()).items())))
    return out


def _check(got, ref, bound, what, strip=None):
    """|got - ref| <= bound elementwise (bound: scalar or tensor like ref), over every element.  -> worst err / bound."""
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    err = (got.double() - ref).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=ref.device)
    ratio = err / bound
    bad = ~(err <= bound)                                   # NaN fails too
    n_bad = int(bad.sum())
    worst = float(torch.nan_to_num(ratio, nan=float('inf')).max())
    if n_bad:
        idx = torch.nonzero(bad)
        k = int(torch.nan_to_num(ratio, nan=float('inf')).flatten().argmax())
        pos = tuple(int(i) for i in torch.unravel_index(torch.tensor(k), ref.shape))
        raise AssertionError('%s: %d of %d elements outside the bound; worst at %s: got %.9g, ref %.9g, err %.3g = %.3g x bound\n%s'
                             % (what, n_bad, ref.numel(), pos, float(got[pos]), float(ref[pos]), float(err[pos]), worst,
                                _hist(idx, strip)))
    print('%s: max err = %.3f of the bound' % (what, worst))
    return worst


def _under_load(launch, first, what, cuda, strip=None):
    """N_LOAD launches of `launch()` while a second stream multiplies fp32 matrices: each bit-identical to `first`."""
    side = torch.cuda.Stream()
    junk = torch.randn(2048, 2048, device=cuda)
    torch.cuda.synchronize()
    for i in range(N_LOAD):
        with torch.cuda.stream(side):
            junk = (junk @ junk).tanh_()
        out = launch()
        torch.cuda.synchronize()
        outs = out if isinstance(out, tuple) else (out,)
        refs = first if isinstance(first, tuple) else (first,)
        for o, r in zip(outs, refs):
            if not torch.equal(o, r):
                d = o != r
                raise AssertionError('%s: launch %d differs from the first in %d elements\n%s'
                                     % (what, i, int(d.sum()), _hist(torch.nonzero(d), strip)))


# ---- (a) the regulariser ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def regvol(cuda):
    """16 views of cfg2: the variance volume in the three formats the warp kernel writes, the net, and the float64 reference."""
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    inp = syn.make_costvolume_inputs('cfg2', n_ref=N_REF)
    sd = syn.costregnet_weights(sharpen=200.0)
    net = mvs.MVSNet(32, inp['img_size']).eval()
    net.cnn_3d.load_state_dict(sd, strict=False)
    net = net.to(cuda)
    d0, dd, D = inp['depth']
    args = (inp['feat'].to(cuda), inp['rotmats'], inp['tvecs'], inp['K'], inp['edges'].to(cuda), d0, dd, D, inp['img_size'],
            inp['plane_size'])
    with torch.no_grad():
        var = mvs.plane_sweep_variance(*args)
        sv = mvs.plane_sweep_variance(*args, split=True)
        cv = mvs.plane_sweep_variance(*args, cl8=True)
        n, C, D, h, w = var.shape
        # the formats hold the same volume: the reference below is computed from exactly what the kernels receive
        assert torch.equal(_decode_split(sv), _split_roundtrip(var))
        assert torch.equal(cv.data.contiguous().view(n, 4, 2, D, h, w, 4).permute(0, 1, 2, 6, 3, 4, 5).reshape(n, 32, D, h, w), var)
        vals = net.depth_values(d0, dd, D, cuda)
        sd64 = {k: v.to(cuda, torch.float64) for k, v in sd.items()}
        ref = torch.cat([ocv.costregnet(var[i:i + 1].double(), sd64).squeeze(1) for i in range(n)])
        prob = F.softmax(-ref, dim=1)
        depth = (prob * vals.double().view(1, D, 1, 1)).sum(1)
    torch.cuda.synchronize()
    return dict(net=net, var=var, sv=sv, cv=cv, vals=vals, ref=ref, depth=depth, shape=(n, C, D, h, w))


def _one_view(x, i):
    cls = type(x)
    return cls(x.data[i:i + 1], (1,) + tuple(x.shape[1:]))


def test_regulariser_split_route_every_element(regvol):
    """The headline route (SplitVariance hand-off, batched conv0z, conv12z march, split tail, conv9_prob): reg within 5e-5 of
    max|ref| everywhere, depth within 1e-4 relative of the float64 soft-argmin."""
    with torch.no_grad():
        depth, reg = regvol['net'].cnn_3d.regularize_depth(regvol['sv'], regvol['vals'], return_reg=True)
    torch.cuda.synchronize()
    ref = regvol['ref']
    _check(reg, ref, REG_SPLIT_ATOL * float(ref.abs().max()), 'reg (split-bf16 route)')
    _check(depth, regvol['depth'], DEPTH_SPLIT_RTOL * regvol['depth'].abs(), 'depth (split-bf16 route)')


def test_regulariser_cl8_route_every_element(regvol):
    """The exact-fp32 route (Cl8Variance, conv0z<true> + per-layer exact-fp32 kernels): reg within REG_F32_ATOL of max|ref|,
    a bound a split-bf16 kernel anywhere in the chain exceeds; depth within 2e-5 relative."""
    with torch.no_grad():
        depth, reg = regvol['net'].cnn_3d.regularize_depth(regvol['cv'], regvol['vals'], return_reg=True, precision='fp32')
    torch.cuda.synchronize()
    ref = regvol['ref']
    _check(reg, ref, REG_F32_ATOL * float(ref.abs().max()), 'reg (exact-fp32 Cl8 route)')
    _check(depth, regvol['depth'], DEPTH_F32_RTOL * regvol['depth'].abs(), 'depth (exact-fp32 Cl8 route)')


@pytest.mark.parametrize('route', ['split', 'cl8'])
def test_regulariser_batch_is_bit_identical_to_single_views(route, regvol):
    """A view's regularised volume and depth do not depend on the other views of the launch (the batched conv0z)."""
    x, pr = (regvol['sv'], 'split_bf16') if route == 'split' else (regvol['cv'], 'fp32')
    c = regvol['net'].cnn_3d
    with torch.no_grad():
        depth, reg = c.regularize_depth(x, regvol['vals'], return_reg=True, precision=pr)
        for i in range(x.shape[0]):
            d1, r1 = c.regularize_depth(_one_view(x, i), regvol['vals'], return_reg=True, precision=pr)
            assert torch.equal(r1[0], reg[i]), 'view %d: reg of the batched call != single-view call' % i
            assert torch.equal(d1[0], depth[i]), 'view %d: depth of the batched call != single-view call' % i


@pytest.mark.parametrize('route', ['split', 'cl8'])
def test_regulariser_deterministic_under_load(route, regvol, cuda):
    x, pr = (regvol['sv'], 'split_bf16') if route == 'split' else (regvol['cv'], 'fp32')
    c = regvol['net'].cnn_3d

    def launch():
        with torch.no_grad():
            return c.regularize_depth(x, regvol['vals'], return_reg=True, precision=pr)
    first = tuple(t.clone() for t in launch())
    _under_load(launch, first, 'regulariser, %s route' % route, cuda)


# ---- (b) stage 3 at the sizes of cfg3 -------------------------------------------------------------------------------------

# (guide + depth channels, H, W, weight seed): the 4-channel net at full resolution, the 33-channel nets at 1/2 and 1/4, the
# 17-channel net (feat_dim 16) at 1/4
STAGE3 = [(4, 256, 320, 7), (33, 128, 160, 6), (33, 64, 80, 5), (17, 64, 80, 8)]
N_VIEWS = 64
STRIP = 40                     # output columns per strip of propz_kernel (kTWO)


def stage3_inputs(cin, H, W, seed, mode, cuda):
    """-> (state_dict, guide [64, cin-1, H, W], depth input, depth at the guide's size [64, H, W]), seeded.
    mode 'forward': depth [64, 1, H, W]; 'resized': depth [64, H/2, W/2] and torch's nearest resize of it."""
    sd = v3d('synthetic').propagation_weights(cin, 32, seed)
    g = torch.Generator(device=cuda).manual_seed(1000 * cin + H + (mode == 'resized'))
    guide = torch.rand((N_VIEWS, cin - 1, H, W), generator=g, device=cuda)
    if mode == 'forward':
        depth = 1 + torch.rand((N_VIEWS, 1, H, W), generator=g, device=cuda)
        return sd, guide, depth, depth[:, 0]
    depth = 1 + torch.rand((N_VIEWS, H // 2, W // 2), generator=g, device=cuda)
    return sd, guide, depth, F.interpolate(depth.unsqueeze(1), (H, W), mode='nearest')[:, 0]


def stage3_reference(sd, guide, full, cuda):
    """float64 PropagationNet (oracle/scene.py) of the fp32 inputs, ~8 M pixels per chunk."""
    sd64 = {k: v.to(cuda, torch.float64) for k, v in sd.items()}
    B, _, H, W = guide.shape
    step = max(1, (8 << 20) // (H * W))
    with torch.no_grad():
        return torch.cat([osc.propagation_net(guide[s:s + step].double(), full[s:s + step, None].double(), sd64)
                          for s in range(0, B, step)])


def _stage3_net(cin, sd, precision, cuda):
    up = v3d('upsampling')
    net = up.PropagationNet(cin, 32, precision=precision).eval()
    net.load_state_dict(sd, strict=False)
    return net.to(cuda)


def _stage3_launch(net, guide, depth, mode):
    with torch.no_grad():
        return net(guide, depth) if mode == 'forward' else net.forward_resized(guide, depth)


STAGE3_IDS = ['%dch_%dx%d' % c[:3] for c in STAGE3]


@pytest.mark.parametrize('mode', ['forward', 'resized'])
@pytest.mark.parametrize('case', STAGE3, ids=STAGE3_IDS)
def test_stage3_every_element_at_cfg3_size(case, mode, cuda):
    cin, H, W, seed = case
    sd, guide, depth, full = stage3_inputs(cin, H, W, seed, mode, cuda)
    ref = stage3_reference(sd, guide, full, cuda)
    for pr in ('split_bf16', 'fp32'):
        out = _stage3_launch(_stage3_net(cin, sd, pr, cuda), guide, depth, mode)
        torch.cuda.synchronize()
        what = 'stage 3 %dch %dx%d %s %s' % (cin, H, W, mode, pr)
        # not vacuous: most outputs moved away from the (resized) input depth
        assert float(((out - full).abs() > 1e-3 * full).double().mean()) > 0.5, what + ': output is (nearly) its input'
        _check(out, ref, PROP_RTOL[pr] * ref.abs(), what, strip=STRIP)


@pytest.mark.parametrize('precision', ['split_bf16', 'fp32'])
@pytest.mark.parametrize('mode', ['forward', 'resized'])
@pytest.mark.parametrize('case', STAGE3, ids=STAGE3_IDS)
def test_stage3_deterministic_under_load(case, mode, precision, cuda):
    cin, H, W, seed = case
    sd, guide, depth, _ = stage3_inputs(cin, H, W, seed, mode, cuda)
    net = _stage3_net(cin, sd, precision, cuda)
    first = _stage3_launch(net, guide, depth, mode).clone()
    _under_load(lambda: _stage3_launch(net, guide, depth, mode), first, 'stage 3 %dch %dx%d %s %s' % (cin, H, W, mode, precision),
                cuda, strip=STRIP)
