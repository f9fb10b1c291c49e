"""GPU: backward of the plane-sweep variance (csrc/psv_backward.hip, 3dvnet_amd/training.py) against the float64 oracle of
tests/psv_backward_oracle.py, per element, within the worst-case fp32 bound (N + c) 2^-24 M (c = 32 up to 9 edges per reference,
one more per further edge: pbo.bound); the whole supervised stage 1 against float64 autograd of the oracle chain.  No bit-identity
of the gradient is asserted anywhere: its sums are fp32 atomics.  The cases of pbo.CHUNK_CASES, the segment sweep and the limits
reach what the three cases of pbo.CASES do not: more than the 8 edges whose tap records fit in LDS (pass 2 projects every chunk a
second time), more than one 16-plane depth segment, dead planes in the last one, block counts that are no multiple of 8."""
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
    assert bad == 0, '%s: %d elements outside the bound of pbo.bound, worst ratio %.3f' % (what, bad, worst)


_RUNS = {}


def _run(param, cuda):
    """One case, its oracle (computed once, never modified) and the gradient of two consecutive backward calls."""
    if param not in _RUNS:
        case = pbo.build(param)
        orc = pbo.gradient(case)
        feat, var = _variance(case, cuda)
        gv = case['gvar'].to(cuda)
        g1 = torch.autograd.grad(var, feat, grad_outputs=gv, retain_graph=True)[0]
        g2 = torch.autograd.grad(var, feat, grad_outputs=gv)[0]
        _RUNS[param] = types.SimpleNamespace(case=case, orc=orc, var=var.detach(), g1=g1, g2=g2, dev=cuda)
    return _RUNS[param]


@pytest.fixture(scope='module', params=pbo.CASES, ids=pbo.case_id)
def run(request, cuda):
    """The cases of at most 4 edges and 8 planes (reference 0 has a single edge)."""
    return _run(request.param, cuda)


@pytest.fixture(scope='module', params=pbo.CASES + pbo.CHUNK_CASES, ids=pbo.case_id)
def run_all(request, cuda):
    """Those, and the cases of 8, 9 and 17 edges with three depth segments."""
    return _run(request.param, cuda)


def _backward_raw(c, dev, feat_cl, gvar, out):
    """v3d_psv_variance_backward_f32 itself on the cameras, edges and geometry of case ``c`` -> its return code."""
    lib_mod, mvs = v3d('_lib'), v3d('mvsnet')
    n_img, Hf, Wf, C = feat_cl.shape
    _, ref_img, edge_ofs, edge_src = mvs.edges_to_csr(c['edges'].to(dev))
    K, R, t = (x.to(dev).contiguous() for x in (c['K'], c['rotmats'], c['tvecs']))
    start, interval, D = c['depth']
    assert feat_cl.is_contiguous() and gvar.is_contiguous() and out.is_contiguous() and out.numel() == feat_cl.numel()
    assert gvar.shape == (ref_img.shape[0], C, D) + tuple(c['plane_size'])
    return lib_mod.load().v3d_psv_variance_backward_f32(
        feat_cl.data_ptr(), K.data_ptr(), R.data_ptr(), t.data_ptr(), ref_img.data_ptr(), edge_ofs.data_ptr(), edge_src.data_ptr(),
        n_img, ref_img.shape[0], edge_src.shape[0], C, Hf, Wf, c['img_size'][0], c['img_size'][1], start, interval, D,
        c['plane_size'][0], c['plane_size'][1], gvar.data_ptr(), out.data_ptr(), lib_mod.stream_ptr(dev))


def _poisoned(shape, byte, dev):
    n = 1
    for k in shape:
        n *= k
    return torch.full((n * 4,), byte, dtype=torch.uint8, device=dev).view(torch.float32).view(shape)


def test_forward_is_the_inference_kernel(run_all):
    """1. the Function's forward is mvsnet.plane_sweep_variance, bit for bit."""
    run = run_all
    mvs, c = v3d('mvsnet'), run.case
    want = mvs.plane_sweep_variance(c['feat'].to(run.dev), c['rotmats'], c['tvecs'], c['K'], c['edges'].to(run.dev), *_geom(c))
    assert run.var.shape == want.shape and torch.equal(run.var, want)


def test_gradient_within_the_fp32_bound(run_all, request):
    """2. + 5. every element of two consecutive calls; 3. the unused image stays exactly zero."""
    run = run_all
    assert run.g1.shape == run.case['feat'].shape and run.g1.dtype == torch.float32
    _inside(run.g1, run.orc, '%s first call' % request.node.callspec.id)
    _inside(run.g2, run.orc, '%s second call' % request.node.callspec.id)
    unused = run.case['unused']
    assert unused not in run.case['edges'].flatten().tolist()
    assert not run.g1[unused].any() and not run.g2[unused].any()
    assert float(run.g1.abs().max()) > 0


def test_one_edge_reference_contributes_exactly_zero(run):
    """3. x_e - avg == 0 for the reference with a single edge."""
    feat, var = _variance(run.case, run.dev)
    gv = torch.zeros_like(var)
    gv[0] = run.case['gvar'][0].to(run.dev)
    g = torch.autograd.grad(var, feat, grad_outputs=gv)[0]
    assert not g.any()


@pytest.mark.parametrize('byte', [0x00, 0xFF])
def test_output_poison(run_all, byte):
    """4. the entry point zero-fills its accumulation target itself: an output of 0x00 bytes and one of 0xFF bytes (NaN)."""
    run = run_all
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


def test_stride0_and_sliced_grad_output(run_all):
    """6. loss = var.sum() hands the backward a stride-0 expanded gradient; a slice of a wider tensor a non-contiguous one."""
    run = run_all
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


# ---- depth segments, feature dtype and layout, the entry point's limits ------------------------------------------------
@pytest.mark.parametrize('D', [15, 16, 17, 32])
def test_segment_boundaries(cuda, D):
    """One reference of 9 edges (two chunks) at plane counts around the 16-plane segment: one segment with a dead plane, exactly
    one, one plus a single live plane, exactly two.  Then with only the last segment's grad_output non-zero: the gradient of the
    tail alone is inside the same bound and not all zero."""
    case = pbo.make_chunk_case(32, 'dense', edge_counts=(9,), D=D)
    feat, var = _variance(case, cuda)
    assert var.shape[2] == D
    g = torch.autograd.grad(var, feat, grad_outputs=case['gvar'].to(cuda), retain_graph=True)[0]
    orc = pbo.gradient(case)
    assert orc['cnt_max'] == 9
    _inside(g, orc, 'D = %d' % D)
    assert float(g.abs().max()) > 0 and not g[case['unused']].any()
    tail = torch.zeros_like(case['gvar'])
    d0 = (D - 1) // pbo.SEGMENT * pbo.SEGMENT
    tail[:, :, d0:] = case['gvar'][:, :, d0:]
    g = torch.autograd.grad(var, feat, grad_outputs=tail.to(cuda))[0]
    _inside(g, pbo.gradient(case, gvar=tail), 'D = %d, planes %d .. %d only' % (D, d0, D - 1))
    assert float(g.abs().max()) > 0


def test_feature_layout_and_dtype(cuda):
    """The wrapper's copies going in (.float().permute().contiguous()) and coming out (.to(features_quarter.dtype)): features in
    channels_last, features that are a channel slice of a wider tensor, and bfloat16 features -- the oracle then takes the bf16
    values promoted to float64, and the result may carry one more bf16 rounding: |g - g64| <= bound + 2^-8 |g64|."""
    tr = v3d('training')
    param = ('chunk', 32, 'dense')
    case, orc = pbo.build(param), _run(param, cuda).orc
    gv = case['gvar'].to(cuda)

    def grad(feat):
        feat.requires_grad_(True)
        var = tr.plane_sweep_variance(feat, case['rotmats'], case['tvecs'], case['K'], case['edges'], *_geom(case))
        return torch.autograd.grad(var, feat, grad_outputs=gv)[0]
    cl = case['feat'].to(cuda).contiguous(memory_format=torch.channels_last)
    assert not cl.is_contiguous()
    _inside(grad(cl), orc, 'channels_last features')
    wide = torch.randn((19, 40, 8, 10), generator=torch.Generator().manual_seed(4)).to(cuda)
    wide[:, 4:36] = case['feat'].to(cuda)
    sliced = wide[:, 4:36].detach()
    assert not sliced.is_contiguous() and torch.equal(sliced, case['feat'].to(cuda))
    _inside(grad(sliced), orc, 'features sliced out of 40 channels')
    bf = case['feat'].to(cuda).bfloat16()
    g = grad(bf)
    assert g.dtype == torch.bfloat16 and g.shape == bf.shape
    orc16 = pbo.gradient(dict(case, feat=bf.detach().float().cpu()))
    err = (g.double().cpu() - orc16['g64']).abs()
    allowed = pbo.bound(orc16) + 2.0 ** -8 * orc16['g64'].abs()
    nz = allowed > 0
    print('bfloat16 features: worst |g - g64| / (bound + 2^-8 |g64|) = %.3f, outside: %d'
          % (float((err[nz] / allowed[nz]).max()), int((~(err <= allowed)).sum())))
    assert not torch.isnan(g).any() and bool((err <= allowed).all()) and float(g.abs().max()) > 0
    assert not g[case['unused']].any()


def test_widest_feature_map_is_accepted(cuda):
    """Wf = 32759, the largest width the packed 16-bit columns of the tap records are declared for: accepted, inside the bound,
    with taps (counted by the oracle) whose columns need more than 8 and more than 14 bits."""
    c = pbo.make_strip_case()
    cols = pbo.tap_columns(c)
    assert int((cols >= 256).sum()) >= 1000 and int((cols >= 16384).sum()) > 0
    feat_cl = c['feat'].to(cuda).permute(0, 2, 3, 1).contiguous()
    out = _poisoned(tuple(feat_cl.shape), 0xFF, cuda)
    rc = _backward_raw(c, cuda, feat_cl, c['gvar'].to(cuda), out)
    v3d('_lib').check(rc, 'v3d_psv_variance_backward_f32')
    g = out.permute(0, 3, 1, 2)
    _inside(g, pbo.gradient(c), 'Hf = 2, Wf = 32759')
    assert float(g[..., 16384:].abs().max()) > 0


@pytest.mark.parametrize('what', ['Wf=32760', 'C=8'])
def test_limits_are_refused_and_the_output_untouched(cuda, what):
    """One column more than the tap records can pack, and a channel count the kernel has no instance for: the documented error
    code, and an output of 0xFF bytes keeps every byte.  All buffers have the declared size."""
    codes = {name: rc for rc, name in v3d('_lib')._ERR_NAMES.items()}
    c = pbo.make_strip_case()
    if what == 'Wf=32760':
        shape, want = (2, 2, 32760, 16), codes['V3D_ERR_BAD_SHAPE']
        gvar = c['gvar'].to(cuda)
    else:
        c = pbo.make_case(16)
        shape, want = (5, 8, 10, 8), codes['V3D_ERR_UNSUPPORTED']
        gvar = c['gvar'][:, :8].contiguous().to(cuda)
    feat_cl = torch.rand(shape, generator=torch.Generator().manual_seed(1)).to(cuda)
    out = _poisoned(shape, 0xFF, cuda)
    rc = _backward_raw(c, cuda, feat_cl, gvar, out)
    torch.cuda.synchronize()
    assert rc == want, (rc, want)
    assert bool((out.view(torch.uint8) == 0xFF).all())


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
