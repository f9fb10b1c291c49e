"""GPU: v3d_sparse_interp_backward_f32 (csrc/sparse_interp.hip) through the C ABI and through training.SparseInterpolate, per element
against tests/sparse_interp_backward_oracle.py (float64 sums over the corner table of tests/sparse_oracle.py; pinned on the CPU by
tests/test_sparse_interp_backward_oracle.py):

  * every case: every element within (cnt + 2) * 2^-24 * S of the float64 sum, none NaN, rows nobody touches +0 bit for bit;
  * exact cases (quarter-cell queries, integer gradients): bit equality, whatever the summation order -- the hot row included,
    whose list spans three full chunks and a partial one;
  * the output pre-filled with NaN is fully overwritten, workspace poison changes nothing, two calls are bit-identical;
  * a gradient held in wide rows (ld_grad > C, col0 > 0, NaN elsewhere) gives the bits of its contiguous copy;
  * n_pts == 0 zero-fills; the error codes of a null pointer, C = 6 and a short workspace, with the output untouched;
  * the Function's forward is HypothesisDecoder.features bit for bit, its backward the C call's bits, also for the strided views
    that the backward of ``cat`` hands out.

Measured on an MI355X: worst |g - g64| / bound per case in DESIGN.md 4.1d.  No number here comes from the kernel under test.
"""
import numpy as np
import pytest
import torch

import sparse_interp_backward_oracle as sbo
from conftest import v3d

pytestmark = pytest.mark.gpu

OK, BAD_SHAPE, BAD_ARG, WS_SMALL, UNSUPPORTED = 0, -1, -2, -3, -5           # include/v3d.h


def _to(a, cuda, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(cuda).contiguous()


class _Level:
    """One hashed level of a case on the device + v3d_sparse_interp_backward_f32 into a NaN-filled [N, C] buffer."""

    def __init__(self, case, cuda):
        self.libm = v3d('_lib')
        self.lib = self.libm.load()
        self.case, self.cuda = case, cuda
        self.level = v3d('scenemodeling').SparseLevel(_to(case['coords'], cuda, torch.int32), case['ts'])
        self.level.check()
        self.mn = _to(case['min_pts'], cuda, torch.float32)
        self.pts = _to(case['pts'], cuda, torch.float32)
        self.pb = _to(case['pts_batch'], cuda, torch.int64)
        self.grad = _to(case['grad_out'], cuda, torch.float32)

    def run(self, grad=None, ld=None, col0=None, poison=0xFF, C=None, n_pts=None, ws_short=0, null=None, expect=OK):
        c = self.case
        N = c['coords'].shape[0]
        C = c['C'] if C is None else C
        n_pts = c['n_pts'] if n_pts is None else n_pts
        grad = self.grad if grad is None else grad
        ld = c['ld'] if ld is None else ld
        col0 = c['col0'] if col0 is None else col0
        out = torch.full((N, c['C']), float('nan'), dtype=torch.float32, device=self.cuda)
        nbytes = self.lib.v3d_sparse_interp_backward_workspace_bytes(N, c['C'], c['n_pts'], c['n_hyp'])
        ws = torch.full((nbytes,), poison, dtype=torch.uint8, device=self.cuda)
        args = dict(table=self.level.table.data_ptr(), pts=self.pts.data_ptr(), pb=self.pb.data_ptr(), mn=self.mn.data_ptr(),
                    grad=grad.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr() if n_pts else None)
        if null:
            args[null] = None
        rc = self.lib.v3d_sparse_interp_backward_f32(args['table'], N, C, c['ts'], args['pts'], args['pb'], n_pts, c['n_hyp'],
                                                     args['mn'], float(c['res']), args['grad'], ld, col0, args['out'], args['ws'],
                                                     nbytes - ws_short, self.libm.stream_ptr(self.cuda))
        assert rc == expect, (rc, self.lib.v3d_last_error())
        return out.cpu().numpy()


@pytest.fixture(scope='module', params=sbo.CASES, ids=sbo.case_id)
def run(request, cuda):
    case = sbo.build(request.param)
    lv = _Level(case, cuda)
    return request.param, case, sbo.gradient(case), lv, lv.run()


def test_every_element_within_the_bound(run):
    param, case, orc, lv, g = run
    assert not np.isnan(g).any() and np.isfinite(g).all()
    bad, worst, worst_zero = sbo.violations(g, orc)
    print('%s: worst |g - g64| / bound = %.3f over %d elements (%d with S = 0), outside: %d'
          % (sbo.case_id(param), worst, g.size, (orc['S'] == 0).sum(), bad))
    assert bad == 0 and worst_zero == 0.0
    untouched = orc['cnt'] == 0
    assert untouched.any() and (g[untouched].view(np.int32) == 0).all()                      # +0, bit for bit
    if case['exact']:
        assert np.array_equal(g.view(np.int32), orc['g64'].astype(np.float32).view(np.int32))
    else:
        assert worst > 0                                                                     # fp32 sums of random data do round


def test_two_calls_agree_whatever_the_workspace_held(run):
    param, case, orc, lv, g = run
    again = lv.run(poison=0x00)
    assert np.array_equal(again.view(np.int32), g.view(np.int32))
    assert np.array_equal(lv.run(poison=0x7F).view(np.int32), g.view(np.int32))


@pytest.mark.parametrize('param', sbo.STRIDED_CASES + sbo.HOT_CASES, ids=sbo.case_id)
def test_wide_rows_equal_the_contiguous_gradient(param, cuda):
    """The case's own layout against the same gradient in rows of exactly C floats, and in rows of C + 12 floats from column 8 and
    C + 11 floats from column 5 (16-byte and 4-byte reads of the gradient rows): the same bits."""
    case = sbo.build(param)
    lv = _Level(case, cuda)
    g = lv.run()
    C, nq = case['C'], case['n_pts'] * case['n_hyp']
    inner = case['grad_out'][:, case['col0']:case['col0'] + C]
    assert np.array_equal(lv.run(grad=_to(inner, cuda, torch.float32), ld=C, col0=0).view(np.int32), g.view(np.int32))
    for ld, col0 in ((C + 12, 8), (C + 11, 5)):
        wide = np.full((nq, ld), np.nan, dtype=np.float32)
        wide[:, col0:col0 + C] = inner
        assert np.array_equal(lv.run(grad=_to(wide, cuda, torch.float32), ld=ld, col0=col0).view(np.int32), g.view(np.int32))


def test_no_points_zero_fills_and_errors_leave_the_output_untouched(cuda):
    case = sbo.build(('generic', 64, 2, 7))
    lv = _Level(case, cuda)
    g = lv.run(n_pts=0)
    assert (g.view(np.int32) == 0).all()
    for null in ('table', 'pts', 'pb', 'mn', 'grad', 'out'):
        assert np.isnan(lv.run(null=null, expect=BAD_ARG)).all()
    assert np.isnan(lv.run(C=6, expect=UNSUPPORTED)).all()
    assert np.isnan(lv.run(ws_short=1, expect=WS_SMALL)).all()
    assert np.isnan(lv.run(null='ws', expect=WS_SMALL)).all()
    assert np.isnan(lv.run(ld=case['C'] - 1, expect=BAD_SHAPE)).all()
    bad, _, _ = sbo.violations(lv.run(), sbo.gradient(case))                                 # and the same call, complete, works
    assert bad == 0


@pytest.mark.parametrize('param', [('generic', 64, 2, 7), ('hot', 128, 2, 1), ('exact', 4, 2, 1)], ids=sbo.case_id)
def test_function_forward_and_backward_are_the_kernels(param, cuda):
    """training.sparse_interpolate on a level dict: the forward is HypothesisDecoder.features bit for bit; the backward with a
    contiguous gradient, with a slice of a wider tensor (what ``cat``'s backward hands out) and with a stride-0 expanded gradient
    equals the C call on the same numbers bit for bit; pts and pts_batch receive no gradient."""
    tr, rf = v3d('training'), v3d('refinement')
    case = sbo.build(param)
    lv = _Level(case, cuda)
    C, n_pts, n_hyp = case['C'], case['n_pts'], case['n_hyp']
    rng = np.random.default_rng(5)
    feats = _to(rng.standard_normal((case['coords'].shape[0], C)), cuda, torch.float32).requires_grad_(True)
    x = dict(sparse=lv.level, feats=feats.detach(), stride=case['ts'], res=case['res'], _min_pts=lv.mn)
    pts = lv.pts.clone().requires_grad_(True)
    out = tr.sparse_interpolate(x, pts, lv.pb, feats)
    dec = rf.HypothesisDecoder(in_dim=C, h_dim=8)
    with torch.no_grad():
        ref = dec.features([x], lv.pts, None, lv.pb)
    assert out.shape == (n_pts, n_hyp, C) and torch.equal(out, ref) and out.requires_grad
    inner = _to(case['grad_out'][:, case['col0']:case['col0'] + C], cuda, torch.float32).view(n_pts, n_hyp, C)
    want = lv.run(grad=inner, ld=C, col0=0)
    (g,) = torch.autograd.grad(out, feats, inner, retain_graph=True)
    assert np.array_equal(g.cpu().numpy().view(np.int32), want.view(np.int32))
    # through cat: the gradient of `out` is a view with row stride C + 16 at column 16
    other = torch.zeros((n_pts, n_hyp, 16), device=cuda, requires_grad=True)
    wide_grad = torch.full((n_pts, n_hyp, C + 16), float('nan'), device=cuda)
    wide_grad[:, :, 16:] = inner
    (g2,) = torch.autograd.grad(torch.cat((other, out), dim=2), feats, wide_grad, retain_graph=True)
    assert np.array_equal(g2.cpu().numpy().view(np.int32), want.view(np.int32))
    # a .sum() upstream: a stride-0 expanded gradient of ones
    ones = lv.run(grad=torch.ones((n_pts * n_hyp, C), device=cuda), ld=C, col0=0)
    (g3,) = torch.autograd.grad(out.sum(), feats, retain_graph=True)
    assert np.array_equal(g3.cpu().numpy().view(np.int32), ones.view(np.int32))
    assert torch.autograd.grad(out.sum(), pts, allow_unused=True)[0] is None
