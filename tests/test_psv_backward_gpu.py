"""GPU: backward of the plane-sweep variance (csrc/psv_backward.hip, 3dvnet_amd/training.py) against the float64 oracle of
tests/psv_backward_oracle.py, per element, within the worst-case fp32 bound (N + 32) 2^-24 M; the whole supervised stage 1
against float64 autograd of the oracle chain.  No bit-identity of the gradient is asserted anywhere: its sums are fp32 atomics."""
import types

import pytest
import torch
import torch.nn.functional as F

import psv_backward_oracle as pbo
from conftest import v3d
from oracle import costvolume as cv

pytestmark = pytest.mark.gpu


def _geom(case):
    return case['depth'] + (case['img_size'], case['plane_size'])


def _variance(case, dev, requires_grad=True):
    tr = v3d('training')
    feat = case['feat'].to(dev).requires_grad_(requires_grad)
    var = tr.plane_sweep_variance(feat, case['rotmats'], case['tvecs'], case['K'], case['edges'], *_geom(case))
    return feat, var


def _inside(g, orc, what):
    bad, worst, worst_zero = pbo.violations(g, orc)
    print('%s: worst |g - g64| / bound = %.3f, outside: %d, worst error where the bound is 0: %g' % (what, worst, bad, worst_zero))
    assert not torch.isnan(g).any(), what
    assert bad == 0, '%s: %d elements outside (N + 32) 2^-24 M, worst ratio %.3f' % (what, bad, worst)


@pytest.fixture(scope='module', params=pbo.CASES, ids=lambda p: '%d-%s' % p)
def run(request, cuda):
    """One case, its oracle (computed once, never modified) and the gradient of two consecutive backward calls."""
    case = pbo.make_case(*request.param)
    orc = pbo.gradient(case)
    feat, var = _variance(case, cuda)
    gv = case['gvar'].to(cuda)
    g1 = torch.autograd.grad(var, feat, grad_outputs=gv, retain_graph=True)[0]
    g2 = torch.autograd.grad(var, feat, grad_outputs=gv)[0]
    return types.SimpleNamespace(case=case, orc=orc, var=var.detach(), g1=g1, g2=g2, dev=cuda)


def test_forward_is_the_inference_kernel(run):
    """1. the Function's forward is mvsnet.plane_sweep_variance, bit for bit."""
    mvs, c = v3d('mvsnet'), run.case
    want = mvs.plane_sweep_variance(c['feat'].to(run.dev), c['rotmats'], c['tvecs'], c['K'], c['edges'].to(run.dev), *_geom(c))
    assert run.var.shape == want.shape and torch.equal(run.var, want)


def test_gradient_within_the_fp32_bound(run):
    """2. + 5. every element of two consecutive calls; 3. the unused image stays exactly zero."""
    assert run.g1.shape == run.case['feat'].shape and run.g1.dtype == torch.float32
    _inside(run.g1, run.orc, 'first call')
    _inside(run.g2, run.orc, 'second call')
    assert not run.g1[4].any() and not run.g2[4].any()
    assert float(run.g1.abs().max()) > 0


def test_one_edge_reference_contributes_exactly_zero(run):
    """3. x_e - avg == 0 for the reference with a single edge."""
    feat, var = _variance(run.case, run.dev)
    gv = torch.zeros_like(var)
    gv[0] = run.case['gvar'][0].to(run.dev)
    g = torch.autograd.grad(var, feat, grad_outputs=gv)[0]
    assert not g.any()


@pytest.mark.parametrize('byte', [0x00, 0xFF])
def test_output_poison(run, byte):
    """4. the entry point zero-fills its accumulation target itself: an output of 0x00 bytes and one of 0xFF bytes (NaN)."""
    lib_mod, mvs, c, dev = v3d('_lib'), v3d('mvsnet'), run.case, run.dev
    lib = lib_mod.load()
    feat_cl = c['feat'].to(dev).permute(0, 2, 3, 1).contiguous()
    n_img, Hf, Wf, C = feat_cl.shape
    _, ref_img, edge_ofs, edge_src = mvs.edges_to_csr(c['edges'].to(dev))
    K, R, t, gv = (x.to(dev).contiguous() for x in (c['K'], c['rotmats'], c['tvecs'], c['gvar']))
    out = torch.full((n_img * Hf * Wf * C * 4,), byte, dtype=torch.uint8, device=dev).view(torch.float32).view(n_img, Hf, Wf, C)
    start, interval, D = c['depth']
    rc = lib.v3d_psv_variance_backward_f32(feat_cl.data_ptr(), K.data_ptr(), R.data_ptr(), t.data_ptr(), ref_img.data_ptr(),
                                           edge_ofs.data_ptr(), edge_src.data_ptr(), n_img, ref_img.shape[0], edge_src.shape[0], C,
                                           Hf, Wf, c['img_size'][0], c['img_size'][1], start, interval, D, c['plane_size'][0],
                                           c['plane_size'][1], gv.data_ptr(), out.data_ptr(), lib_mod.stream_ptr(dev))
    lib_mod.check(rc, 'v3d_psv_variance_backward_f32')
    _inside(out.permute(0, 3, 1, 2), run.orc, 'output pre-filled with 0x%02X' % byte)


def test_stride0_and_sliced_grad_output(run):
    """6. loss = var.sum() hands the backward a stride-0 expanded gradient; a slice of a wider tensor a non-contiguous one."""
    feat, var = _variance(run.case, run.dev)
    var.sum().backward()
    _inside(feat.grad, pbo.gradient(run.case, gvar=torch.ones_like(run.case['gvar'])), 'stride-0 grad_output')
    wide = torch.randn(tuple(var.shape[:-1]) + (2 * var.shape[-1],), generator=torch.Generator().manual_seed(9))
    sliced = wide.to(run.dev)[..., ::2]
    assert not sliced.is_contiguous()
    feat, var = _variance(run.case, run.dev)
    g = torch.autograd.grad(var, feat, grad_outputs=sliced)[0]
    _inside(g, pbo.gradient(run.case, gvar=wide[..., ::2]), 'sliced grad_output')


def test_no_gradient_wanted_launches_nothing(run):
    """7. features that need no gradient: the variance is no part of a graph, and the Function's backward returns None without
    touching its saved tensors or the library."""
    tr = v3d('training')
    _, var = _variance(run.case, run.dev, requires_grad=False)
    assert not var.requires_grad and torch.equal(var, run.var)

    class Ctx:
        needs_input_grad = (False,) * 8

        @property
        def saved_tensors(self):
            raise AssertionError('the backward read its saved tensors although no gradient is wanted')
    assert tr.PlaneSweepVariance.backward(Ctx(), torch.ones_like(var)) == (None,) * 8


# ---- 8. the whole supervised stage ------------------------------------------------------------------------------------
PARAMS = ('conv0.conv.weight', 'conv6.conv.weight', 'prob.weight', 'prob.bias')


def _stage_inputs():
    syn = v3d('synthetic')
    img_size, feat_size, plane_size, depth = (64, 80), (16, 20), (8, 8), (0.5, 0.25, 8)
    edges, n_img = syn.make_edges(2, 1, 1)
    rot, tv, K = syn.make_cameras(n_img, img_size, seed=11)
    feat = syn.make_features(n_img, 32, *feat_size, seed=11)
    refs = torch.unique(edges[0])
    gt = syn.ray_box_depth(rot[refs], tv[refs], K[refs], img_size, img_size).float()
    gt[:, :9, :17] = 0.0                                   # pixels without ground truth
    return dict(img_size=img_size, plane_size=plane_size, depth=depth, edges=edges, rotmats=rot, tvecs=tv, K=K, feat=feat,
                gt=gt, sd=syn.costregnet_weights(seed=0, sharpen=200.0))


def _oracle_chain(s, dtype):
    """warp_variance -> costregnet -> soft_argmin_depth -> masked MAE of oracle/costvolume.py on the CPU in ``dtype`` (the
    sampling grid is computed in fp32 as the reference does and cast) -> gradients with respect to the features and PARAMS."""
    feat = s['feat'].detach().clone().to(dtype).requires_grad_(True)
    sd = {k: v.detach().clone().to(dtype).requires_grad_(k in PARAMS) if v.is_floating_point() else v for k, v in s['sd'].items()}
    start, interval, D = s['depth']
    edges = s['edges']
    ref_idx, gather_idx = torch.unique(edges[0], return_inverse=True)
    pts = cv.plane_sweep_points(start, interval, D, s['rotmats'], s['tvecs'], s['K'], s['img_size'], s['plane_size'])
    grid = cv.project_to_grid(pts[edges[0]], s['rotmats'], s['tvecs'], s['K'], edges[1], s['img_size'])
    x = F.grid_sample(feat[edges[1]], grid.to(dtype), mode='bilinear', align_corners=True)
    x = x.squeeze(3).view(-1, feat.shape[1], D, *s['plane_size'])
    var = cv.scatter_mean(x ** 2, gather_idx, len(ref_idx)) - cv.scatter_mean(x, gather_idx, len(ref_idx)) ** 2
    depth, _ = cv.soft_argmin_depth(cv.costregnet(var, sd).squeeze(1), start, interval, D)
    gt = F.interpolate(s['gt'].unsqueeze(1), depth.shape[-2:], mode='nearest').squeeze(1).to(dtype)
    mask = (gt != 0).to(dtype)
    loss = (((mask * (depth - gt).abs()).sum(dim=(1, 2)) / interval) / (mask.sum(dim=(1, 2)) + 1e-7)).mean()
    grads = torch.autograd.grad(loss, [feat] + [sd[k] for k in PARAMS] + [var])
    return loss.detach(), dict(zip(('features',) + PARAMS + ('variance',), grads))


def test_initial_depth_loss_gradients(cuda):
    """8. gradients of initial_depth_loss against float64 autograd of the oracle chain.  The device's convolution algorithms are
    not this project's, so the tolerance is measured here, on the CPU, never from the code under test: the deviation of the
    SAME chain in float32 from the float64 one, relative to max|g64| per tensor, times 10 for the other summation orders.
    Measured on an MI355X (float32 CPU chain / device): features 1.83e-6 / 1.56e-5, conv0.conv.weight 5.2e-7 / 2.5e-6,
    conv6.conv.weight 2.4e-6 / 7.3e-6, prob.weight 2.3e-7 / 6.1e-7.  The prob.bias row checks nothing: that gradient is zero
    in exact arithmetic (softmax over the planes ignores a common shift), so max|g64| is rounding noise (9e-17)."""
    tr, mvs = v3d('training'), v3d('mvsnet')
    s = _stage_inputs()
    loss64, g64 = _oracle_chain(s, torch.float64)
    loss32, g32 = _oracle_chain(s, torch.float32)
    net = mvs.MVSNet(32, s['img_size']).eval()
    net.cnn_3d.load_state_dict(s['sd'], strict=False)
    net = net.to(cuda)
    feat = s['feat'].to(cuda).requires_grad_(True)
    batch = types.SimpleNamespace(rotmats=s['rotmats'], tvecs=s['tvecs'], K=s['K'], ref_src_edges=s['edges'])
    cfg = dict(depth_start=s['depth'][0], depth_interval=s['depth'][1], n_intervals=s['depth'][2], size=s['plane_size'])
    loss, depth = tr.initial_depth_loss(net, feat, batch, cfg, s['gt'].to(cuda))
    assert depth.shape == (2,) + s['plane_size'] and loss.dim() == 0
    params = dict(net.cnn_3d.named_parameters())
    grads = torch.autograd.grad(loss, [feat] + [params[k] for k in PARAMS])
    print('loss: device %.9g, float64 %.9g, float32 on the CPU %.9g' % (float(loss.detach()), float(loss64), float(loss32)))
    failed = []
    for name, g in zip(('features',) + PARAMS, grads):
        scale = float(g64[name].abs().max())
        cpu32 = float((g32[name].double() - g64[name]).abs().max()) / scale
        dev = float((g.double().cpu() - g64[name]).abs().max()) / scale
        print('%-18s max|g64| %.4g   float32 CPU chain %.3g   device %.3g   tolerance %.3g' % (name, scale, cpu32, dev, 10 * cpu32))
        assert scale > 0 and not torch.isnan(g).any()
        if not dev <= 10 * cpu32:
            failed.append((name, dev, 10 * cpu32))
    # for the record, not a check: the gradient that ENTERS the HIP backward (d loss / d variance, made by the stock
    # convolutions' backward on the device) against the same two CPU chains
    var = tr.plane_sweep_variance(feat.detach(), batch.rotmats, batch.tvecs, batch.K, batch.ref_src_edges, *s['depth'],
                                  s['img_size'], s['plane_size']).requires_grad_(True)
    x_reg = tr.costregnet(net.cnn_3d, var).squeeze(1)
    d2 = torch.sum(net.depth_values(*s['depth'], cuda).view(1, -1, 1, 1) * F.softmax(-x_reg, dim=1), dim=1)
    gvar = torch.autograd.grad(tr.masked_mae(d2, s['gt'].to(cuda), s['depth'][1]), var)[0]
    scale = float(g64['variance'].abs().max())
    print('%-18s max|g64| %.4g   float32 CPU chain %.3g   device %.3g   (not asserted)'
          % ('variance', scale, float((g32['variance'].double() - g64['variance']).abs().max()) / scale,
             float((gvar.double().cpu() - g64['variance']).abs().max()) / scale))
    assert not failed, failed
    # every parameter of the regulariser receives a gradient
    all_grads = torch.autograd.grad(tr.initial_depth_loss(net, feat, batch, cfg, s['gt'].to(cuda))[0], list(params.values()))
    assert all(g is not None and torch.isfinite(g).all() for g in all_grads)


def test_backward_memory_is_not_edge_sized(cuda):
    """The Function's peak extra allocation in backward is at most grad_feat_cl + the channel-last feature copy + a contiguous
    copy of grad_output: nothing of size E C D h w, which here is far above the sum of the allowed pieces."""
    tr, syn = v3d('training'), v3d('synthetic')
    img_size, feat_size, plane_size, depth = (64, 80), (16, 20), (32, 40), (0.5, 0.05, 32)
    edges, n_img = syn.make_edges(3, 2, 2)
    rot, tv, K = syn.make_cameras(n_img, img_size, seed=11)
    feat = syn.make_features(n_img, 32, *feat_size, seed=11).to(cuda).requires_grad_(True)
    var = tr.plane_sweep_variance(feat, rot, tv, K, edges, *depth, img_size, plane_size)
    loss = var.sum()                                         # stride-0 grad_output: the backward makes its contiguous copy
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(cuda)
    base = torch.cuda.memory_allocated(cuda)
    g = torch.autograd.grad(loss, feat)[0]
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(cuda) - base
    # the three pieces; torch's caching allocator hands a block of a 2-MiB-rounded segment out unsplit when at most 1 MiB of it
    # would remain, so each piece can count up to 1 MiB more than was asked for (+ 64 KB for autograd's scalars)
    allowed = 2 * feat.numel() * 4 + var.numel() * 4 + 3 * 2 ** 20 + 64 * 1024
    edge_sized = edges.shape[1] * var[0].numel() * 4
    print('backward peak extra %.2f MB, allowed %.2f MB, one E C D h w tensor %.2f MB' % (extra / 2**20, allowed / 2**20,
                                                                                          edge_sized / 2**20))
    assert g.shape == feat.shape and float(g.abs().max()) > 0
    assert edge_sized > 3 * allowed
    assert extra <= allowed
