"""GPU: backward of the back-projected variance (csrc/backproject_backward.hip, 3dvnet_amd/training.py) against the float64 oracle
of tests/backproject_backward_oracle.py: the feature gradient per element within pbo.bound, (N + 32 + max(0, cnt_max - 9)) 2^-24 M;
the depth gradient per pixel within 16 * 2^-24 * M_d and bit-identical over two calls.  No bit-identity of the feature gradient is
asserted anywhere: its sums are fp32 atomics.  Every case is a few thousand samples."""
import types

import pytest
import torch

import backproject_backward_oracle as bbo
from conftest import v3d

pytestmark = pytest.mark.gpu


def _forward(case, dev, feat=None, feat_grad=True, depth_grad=False):
    tr = v3d('training')
    depth = case['depth_map'].to(dev).requires_grad_(depth_grad)
    feat = (case['feat'].to(dev) if feat is None else feat).requires_grad_(feat_grad)
    pts, var = tr.backproject_variance(depth, feat, case['rotmats'], case['tvecs'], case['K'], case['edges'], case['img_size'],
                                       offset=case['offset'], n=case['n'])
    return depth, feat, pts, var


def _inside(g, orc, what):
    bad, worst, worst_zero = bbo.violations(g, orc)
    print('%s: worst |g - g64| / bound = %.3f, outside: %d, worst error where the bound is 0: %g' % (what, worst, bad, worst_zero))
    assert not torch.isnan(g).any(), what
    assert bad == 0, '%s: %d elements outside the bound of pbo.bound, worst ratio %.3f' % (what, bad, worst)


def _depth_inside(g, case, what, gpts=None):
    g64, M = bbo.depth_gradient(case, gpts=gpts)
    bad, worst = bbo.depth_violations(g, g64, M)
    print('%s: depth gradient, worst |g - g64| / bound = %.3f, outside: %d' % (what, worst, bad))
    assert torch.isfinite(g).all(), what
    assert bad == 0, '%s: %d pixels outside 16 * 2^-24 * M_d, worst ratio %.3f' % (what, bad, worst)


_RUNS = {}


def _run(param, cuda):
    """One case, its oracle (computed once, never modified) and the feature gradient of two consecutive backward calls."""
    if param not in _RUNS:
        case = bbo.build(param)
        orc = bbo.gradient(case)
        _, feat, pts, var = _forward(case, cuda)
        gv = case['gvar'].to(cuda)
        g1 = torch.autograd.grad(var, feat, grad_outputs=gv, retain_graph=True)[0]
        g2 = torch.autograd.grad(var, feat, grad_outputs=gv)[0]
        _RUNS[param] = types.SimpleNamespace(case=case, orc=orc, pts=pts.detach(), var=var.detach(), g1=g1, g2=g2, dev=cuda)
    return _RUNS[param]


@pytest.fixture(scope='module', params=bbo.ALL_CASES, ids=bbo.case_id)
def run_all(request, cuda):
    return _run(request.param, cuda)


@pytest.fixture(scope='module', params=bbo.CASES + bbo.CHUNK_CASES, ids=bbo.case_id)
def run(request, cuda):
    return _run(request.param, cuda)


@pytest.fixture(scope='module', params=[p for p in bbo.ALL_CASES if p[-1] == 0], ids=bbo.case_id)
def run0(request, cuda):
    """The cases of n = 0: the scene point cloud, whose points carry a gradient to the depth."""
    return _run(request.param, cuda)


def _raw(c, dev, feat_cl, gvar, gpts, gfeat, gdepth, n=None, C=None):
    """v3d_backproject_variance_backward_f32 itself on the cameras, edges and geometry of case ``c`` -> its return code."""
    lib_mod, mvs = v3d('_lib'), v3d('mvsnet')
    n_img, Hf, Wf, Cf = feat_cl.shape
    _, ref_img, edge_ofs, edge_src = mvs.edges_to_csr(c['edges'].to(dev))
    K, R, t, depth = (x.to(dev).contiguous() for x in (c['K'], c['rotmats'], c['tvecs'], c['depth_map']))
    n_ref, h, w = depth.shape
    n = c['n'] if n is None else n
    for x in (feat_cl, gvar, gpts, gfeat, gdepth):
        assert x is None or x.is_contiguous()
    assert gvar is None or gvar.numel() == n_ref * h * w * (2 * n + 1) * Cf
    assert gfeat is None or gfeat.numel() == feat_cl.numel()
    assert gpts is None or gpts.numel() == n_ref * h * w * 3
    assert gdepth is None or gdepth.numel() == n_ref * h * w
    ptr = lib_mod.ptr
    return lib_mod.load().v3d_backproject_variance_backward_f32(
        ptr(depth), ptr(feat_cl), ptr(K), ptr(R), ptr(t), ptr(ref_img), ptr(edge_ofs), ptr(edge_src), n_img, n_ref,
        edge_src.shape[0], Cf if C is None else C, Hf, Wf, c['img_size'][0], c['img_size'][1], h, w, c['offset'], n, ptr(gvar),
        ptr(gpts), ptr(gfeat), ptr(gdepth), lib_mod.stream_ptr(dev))


def _poisoned(shape, byte, dev):
    n = 1
    for k in shape:
        n *= k
    return torch.full((n * 4,), byte, dtype=torch.uint8, device=dev).view(torch.float32).view(shape)


def test_forward_is_the_inference_kernel(run_all):
    """1. the Function's forward is lightningmodel.backproject_variance, bit for bit, n = 0 and n > 0."""
    run = run_all
    lm, c = v3d('lightningmodel'), run.case
    pts, var = lm.backproject_variance(c['depth_map'].to(run.dev), c['feat'].to(run.dev), c['rotmats'], c['tvecs'], c['K'],
                                       c['edges'].to(run.dev), c['img_size'], offset=c['offset'], n=c['n'])
    n_hyp = 2 * c['n'] + 1
    assert run.pts.shape == pts.shape == (c['depth_map'].numel(), n_hyp, 3) and run.var.shape == var.shape
    assert torch.equal(run.var, var)
    assert torch.equal(run.pts.view(torch.int32), pts.view(torch.int32))          # bits: the NaN pixel's points are NaN


def test_feature_gradient_within_the_fp32_bound(run_all, request):
    """2. every element of two consecutive calls; the unused image stays exactly zero."""
    run = run_all
    assert run.g1.shape == run.case['feat'].shape and run.g1.dtype == torch.float32
    _inside(run.g1, run.orc, '%s first call' % request.node.callspec.id)
    _inside(run.g2, run.orc, '%s second call' % request.node.callspec.id)
    unused = run.case['unused']
    assert unused not in run.case['edges'].flatten().tolist()
    assert not run.g1[unused].any() and not run.g2[unused].any()
    assert float(run.g1.abs().max()) > 0


@pytest.mark.parametrize('param', bbo.CASES, ids=bbo.case_id)
def test_one_edge_reference_contributes_exactly_zero(cuda, param):
    """3. x_e - avg == 0 for the reference with a single edge."""
    case = bbo.build(param)
    _, feat, _, var = _forward(case, cuda)
    gv = torch.zeros_like(var)
    P = case['depth_map'][0].numel()
    gv[:P] = case['gvar'][:P].to(cuda)
    g = torch.autograd.grad(var, feat, grad_outputs=gv)[0]
    assert not g.any()


def test_depth_gradient(run0, request):
    """4. inside 16 * 2^-24 * M_d per pixel, bit-identical over two calls, finite at the NaN, zero and 0.1 depth pixels."""
    case, dev = run0.case, run0.dev
    depth, _, pts, _ = _forward(case, dev, feat_grad=False, depth_grad=True)
    assert pts.requires_grad
    gp = case['gpts'].to(dev)
    g1 = torch.autograd.grad(pts, depth, grad_outputs=gp, retain_graph=True)[0]
    g2 = torch.autograd.grad(pts, depth, grad_outputs=gp)[0]
    assert g1.shape == depth.shape and g1.dtype == torch.float32
    _depth_inside(g1, case, request.node.callspec.id)
    assert torch.equal(g1, g2)
    assert torch.isnan(case['depth_map'][-1, 0, 2]) and torch.isfinite(g1[-1, 0, :3]).all() and float(g1.abs().max()) > 0


def test_hypothesis_points_are_not_differentiable(cuda):
    """4. with n = 3 pts.requires_grad is False and depth.grad stays None after a backward through var."""
    case = bbo.make_case(32, 'sliding', 3)
    depth, feat, pts, var = _forward(case, cuda, depth_grad=True)
    assert not pts.requires_grad and var.requires_grad
    (var * case['gvar'].to(cuda)).sum().backward()
    assert depth.grad is None and feat.grad is not None and float(feat.grad.abs().max()) > 0


def test_joint_loss_through_the_point_cloud(run0):
    """5. L = sum a . pts + sum b . pts_feat through feature_rich_pointcloud, both inputs requiring gradients: each gradient is
    inside its own bound -- the two paths do not mix (the reference detaches the grid)."""
    tr, case, dev = v3d('training'), run0.case, run0.dev
    depth = case['depth_map'].to(dev).requires_grad_(True)
    feat = case['feat'].to(dev).requires_grad_(True)
    batch = torch.arange(depth.shape[0], device=dev)
    pts, pts_feat, pts_batch = tr.feature_rich_pointcloud(depth, batch, feat, case['rotmats'], case['tvecs'], case['K'],
                                                          case['edges'], case['img_size'])
    Np, C = depth.numel(), feat.shape[1]
    assert pts.shape == (Np, 3) and pts_feat.shape == (Np, C) and pts_batch.shape == (Np,)
    assert torch.equal(pts_batch, batch.repeat_interleave(depth[0].numel()))
    a, b = case['gpts'].to(dev).view(Np, 3), case['gvar'].to(dev).view(Np, C)
    mask = ~torch.isnan(pts)                                     # the NaN pixel's points stay out of the loss VALUE only
    loss = (a * torch.where(mask, pts, torch.zeros_like(pts))).sum() + (b * pts_feat).sum()
    assert torch.isfinite(loss)
    loss.backward()
    _inside(feat.grad, run0.orc, 'joint loss')
    gp = torch.where(mask, a, torch.zeros_like(a)).cpu().view(Np, 1, 3)
    _depth_inside(depth.grad, case, 'joint loss', gpts=gp)


@pytest.mark.parametrize('byte', [0x00, 0xFF])
def test_output_poison(run, byte):
    """6. the entry point zero-fills grad_feat_cl itself and writes every element of grad_depth: outputs of 0x00 bytes and of
    0xFF bytes (NaN) give results inside the bounds; with n = 0 both pairs go through one call."""
    c, dev = run.case, run.dev
    feat_cl = c['feat'].to(dev).permute(0, 2, 3, 1).contiguous()
    gfeat = _poisoned(tuple(feat_cl.shape), byte, dev)
    both = c['n'] == 0
    gdepth = _poisoned(tuple(c['depth_map'].shape), byte, dev) if both else None
    rc = _raw(c, dev, feat_cl, c['gvar'].to(dev), c['gpts'].to(dev) if both else None, gfeat, gdepth)
    v3d('_lib').check(rc, 'v3d_backproject_variance_backward_f32')
    _inside(gfeat.permute(0, 3, 1, 2), run.orc, 'output pre-filled with 0x%02X' % byte)
    if both:
        _depth_inside(gdepth, c, 'output pre-filled with 0x%02X' % byte)
        only = _poisoned(tuple(c['depth_map'].shape), byte, dev)                  # the depth pair alone
        v3d('_lib').check(_raw(c, dev, feat_cl, None, c['gpts'].to(dev), None, only), 'v3d_backproject_variance_backward_f32')
        assert torch.equal(only, gdepth)


def test_stride0_and_sliced_upstream_gradients(run):
    """7. loss = var.sum() hands the backward a stride-0 expanded gradient; a slice of a wider tensor a non-contiguous one."""
    case, dev = run.case, run.dev
    _, feat, _, var = _forward(case, dev)
    var.sum().backward()
    _inside(feat.grad, bbo.gradient(case, gvar=torch.ones_like(case['gvar'])), 'stride-0 grad_var')
    wide = torch.randn(tuple(var.shape[:-1]) + (2 * var.shape[-1],), generator=torch.Generator().manual_seed(9))
    sliced = wide.to(dev)[..., ::2]
    assert not sliced.is_contiguous()
    _, feat, _, var = _forward(case, dev)
    g = torch.autograd.grad(var, feat, grad_outputs=sliced)[0]
    _inside(g, bbo.gradient(case, gvar=wide[..., ::2]), 'sliced grad_var')
    if case['n'] == 0:
        depth, _, pts, _ = _forward(case, dev, feat_grad=False, depth_grad=True)
        pts.sum().backward()                 # (the value is NaN through the NaN pixel; its gradient is the expanded 1)
        _depth_inside(depth.grad, case, 'stride-0 grad_pts', gpts=torch.ones(tuple(pts.shape)))
        widep = torch.randn((pts.shape[0], 1, 6), generator=torch.Generator().manual_seed(8))
        depth, _, pts, _ = _forward(case, dev, feat_grad=False, depth_grad=True)
        g = torch.autograd.grad(pts, depth, grad_outputs=widep.to(dev)[..., ::2])[0]
        _depth_inside(g, case, 'sliced grad_pts', gpts=widep[..., ::2])


def test_feature_layout_and_dtype(cuda):
    """8. features in channels_last, features that are a channel slice of a wider tensor, and bfloat16 features -- the oracle then
    takes the bf16 values promoted to float64, and the result may carry one more bf16 rounding: |g - g64| <= bound + 2^-8 |g64|."""
    param = ('chunk', 32, 'dense', 4)
    case, orc = bbo.build(param), _run(param, cuda).orc
    gv = case['gvar'].to(cuda)

    def grad(feat):
        _, feat, _, var = _forward(case, cuda, feat=feat)
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
    orc16 = bbo.gradient(dict(case, feat=bf.detach().float().cpu()))
    err = (g.double().cpu() - orc16['g64']).abs()
    allowed = bbo.bound(orc16) + 2.0 ** -8 * orc16['g64'].abs()
    nz = allowed > 0
    print('bfloat16 features: worst |g - g64| / (bound + 2^-8 |g64|) = %.3f, outside: %d'
          % (float((err[nz] / allowed[nz]).max()), int((~(err <= allowed)).sum())))
    assert not torch.isnan(g).any() and bool((err <= allowed).all()) and float(g.abs().max()) > 0
    assert not g[case['unused']].any()


def test_no_gradient_wanted_launches_nothing(cuda):
    """9. inputs that need no gradient: var is no part of a graph, and the Function's backward returns None without touching its
    saved tensors or the library."""
    tr = v3d('training')
    case = bbo.make_case(32, 'sliding', 3)
    _, _, pts, var = _forward(case, cuda, feat_grad=False)
    assert not var.requires_grad and not pts.requires_grad

    class Ctx:
        needs_input_grad = (False,) * 9

        @property
        def saved_tensors(self):
            raise AssertionError('the backward read its saved tensors although no gradient is wanted')
    assert tr.BackprojectVariance.backward(Ctx(), torch.ones_like(pts), torch.ones_like(var)) == (None,) * 9


def test_saved_state_is_not_edge_sized(cuda):
    """10. the node saves at most features + depth + cameras + edge tables, and depth_pred.add_() between forward and backward
    neither raises nor changes the gradient."""
    case = bbo.make_case(32, 'sliding', 0)
    orc = bbo.gradient(case)
    depth, feat, pts, var = _forward(case, cuda, depth_grad=True)
    saved = var.grad_fn.saved_tensors
    n_img, n_ref, E = feat.shape[0], depth.shape[0], case['edges'].shape[1]
    allowed = feat.numel() * 4 + depth.numel() * 4 + n_img * 21 * 4 + (n_ref + n_ref + 1 + E) * 4
    got = sum(x.numel() * x.element_size() for x in saved)
    print('saved %d bytes, allowed %d' % (got, allowed))
    assert got <= allowed
    with torch.no_grad():
        depth.add_(0.25)
    gf, gd = torch.autograd.grad([var, pts], [feat, depth], grad_outputs=[case['gvar'].to(cuda), case['gpts'].to(cuda)])
    _inside(gf, orc, 'depth_pred.add_() between forward and backward')
    _depth_inside(gd, case, 'depth_pred.add_() between forward and backward')


@pytest.mark.parametrize('cam', ['rotated', 'sliding'])
def test_plane_sweep_and_backprojection_are_one_walk(cuda, cam):
    """The two entry points run one walk (csrc/variance_backward.h) over two sample axes.  A matched problem: pbo.make_case(32, cam)
    with 7 planes 0.5, 0.75 .. 2.0, and the same cameras, features and edges with a constant depth map 1.25 on the 7 x 9 grid,
    offset 0.25, n = 3 and the same gvar permuted to [n_ref * P, 7, C].  Every number is exact in binary, so the hypothesis depths
    are the plane depths and the sample positions are bit-equal (asserted on the oracles' positions).  Each feature gradient lies
    within pbo.bound of the ONE oracle, and the two agree within twice that bound per element: each is within the bound of the
    same g64, and the atomics fix no order, so no bit-equality is asked for."""
    import psv_backward_oracle as pbo
    tr = v3d('training')
    pc = pbo.make_case(32, cam)
    pc = dict(pc, depth=(0.5, 0.25, 7), gvar=pc['gvar'][:, :, :7].contiguous())
    n_ref, C, D, h, w = pc['gvar'].shape
    bc = dict(pc, depth_map=torch.full((n_ref, h, w), 1.25), offset=0.25, n=3,
              gvar=pc['gvar'].permute(0, 3, 4, 2, 1).reshape(n_ref * h * w, D, C).contiguous())
    for (rp, sp, xp, yp), (rb, sb, xb, yb) in zip(pbo.positions(pc), bbo.positions(bc)):
        assert (rp, sp) == (rb, sb)
        for a, b in ((xp, xb), (yp, yb)):
            assert torch.equal(a.view(D, h * w).t().reshape(-1).view(torch.int32), b.view(torch.int32))
    orc = pbo.gradient(pc)
    feat = pc['feat'].to(cuda).requires_grad_(True)
    var = tr.plane_sweep_variance(feat, pc['rotmats'], pc['tvecs'], pc['K'], pc['edges'], *pc['depth'], pc['img_size'],
                                  pc['plane_size'])
    g_psv = torch.autograd.grad(var, feat, grad_outputs=pc['gvar'].to(cuda))[0]
    _, feat, _, var = _forward(bc, cuda)
    g_bp = torch.autograd.grad(var, feat, grad_outputs=bc['gvar'].to(cuda))[0]
    _inside(g_psv, orc, 'plane sweep, %s' % cam)
    _inside(g_bp, orc, 'back-projection, %s' % cam)
    diff, allowed = (g_psv.double() - g_bp.double()).abs().cpu(), 2.0 * pbo.bound(orc)
    nz = allowed > 0
    print('%s: worst |g_psv - g_bp| / (2 bound) = %.3f' % (cam, float((diff[nz] / allowed[nz]).max())))
    assert float(g_psv.abs().max()) > 0 and bool((diff <= allowed).all())


LIMITS = ['C=8', 'grad_pts with n_half=1', 'grad_var without grad_feat_cl', 'grad_feat_cl without grad_var',
          'grad_pts without grad_depth', 'grad_depth without grad_pts', 'neither pair', 'Wf=32760', 'Hf=32760', 'H=1', 'W=1']


@pytest.mark.parametrize('what', LIMITS)
def test_limits_are_refused_and_the_outputs_untouched(cuda, what):
    """11. the documented error code, and outputs of 0xFF bytes keep every byte.  All buffers have the declared size."""
    codes = {name: rc for rc, name in v3d('_lib')._ERR_NAMES.items()}
    c = bbo.make_case(16, 'rotated', 0)
    shape, n, C, want = (5, 8, 10, 16), 0, None, codes['V3D_ERR_BAD_ARG']
    use = dict(gvar=True, gpts=True, gfeat=True, gdepth=True)
    if what == 'C=8':
        shape, want = (5, 8, 10, 8), codes['V3D_ERR_UNSUPPORTED']
    elif what == 'grad_pts with n_half=1':
        n = 1
    elif what == 'grad_var without grad_feat_cl':
        use['gfeat'] = False
    elif what == 'grad_feat_cl without grad_var':
        use['gvar'] = False
    elif what == 'grad_pts without grad_depth':
        use['gdepth'] = False
    elif what == 'grad_depth without grad_pts':
        use['gpts'] = False
    elif what == 'neither pair':
        use = dict(gvar=False, gpts=False, gfeat=False, gdepth=False)
    elif what == 'Wf=32760':
        shape, want = (2, 2, 32760, 16), codes['V3D_ERR_BAD_SHAPE']
        c = dict(bbo.make_strip_case(), n=0)
    elif what == 'Hf=32760':
        shape, want = (2, 32760, 2, 16), codes['V3D_ERR_BAD_SHAPE']
        c = dict(bbo.make_strip_case(), n=0)
    else:
        want = codes['V3D_ERR_BAD_SHAPE']
        c = dict(c, img_size=(1, 40) if what == 'H=1' else (32, 1))
    rows = c['depth_map'].numel()
    feat_cl = torch.rand(shape, generator=torch.Generator().manual_seed(1)).to(cuda)
    gvar = torch.ones((rows, 2 * n + 1, shape[3]), device=cuda) if use['gvar'] else None
    gpts = torch.ones((rows, 1, 3), device=cuda) if use['gpts'] else None
    gfeat = _poisoned(shape, 0xFF, cuda)
    gdepth = _poisoned(tuple(c['depth_map'].shape), 0xFF, cuda)
    rc = _raw(c, cuda, feat_cl, gvar, gpts, gfeat if use['gfeat'] else None, gdepth if use['gdepth'] else None, n=n, C=C)
    torch.cuda.synchronize()
    assert rc == want, (rc, want, v3d('_lib').load().v3d_last_error())
    assert bool((gfeat.view(torch.uint8) == 0xFF).all()) and bool((gdepth.view(torch.uint8) == 0xFF).all())


def test_widest_feature_map_is_accepted(cuda):
    """11. Wf = 32759, the largest width the packed 16-bit columns of the tap records are declared for, with a 3 x 64 depth map and
    n = 3: accepted, inside the bound, with taps (counted by the oracle) whose columns need more than 8 and more than 14 bits."""
    c = bbo.make_strip_case()
    cols = bbo.tap_columns(c)
    print('in-image taps: %d, column >= 256: %d, column >= 16384: %d' % (cols.numel(), int((cols >= 256).sum()), int((cols >= 16384).sum())))
    assert int((cols >= 256).sum()) >= 1000 and int((cols >= 16384).sum()) > 0
    feat_cl = c['feat'].to(cuda).permute(0, 2, 3, 1).contiguous()
    out = _poisoned(tuple(feat_cl.shape), 0xFF, cuda)
    rc = _raw(c, cuda, feat_cl, c['gvar'].to(cuda), None, out, None)
    v3d('_lib').check(rc, 'v3d_backproject_variance_backward_f32')
    g = out.permute(0, 3, 1, 2)
    _inside(g, bbo.gradient(c), 'Hf = 2, Wf = 32759')
    assert float(g[..., 16384:].abs().max()) > 0
