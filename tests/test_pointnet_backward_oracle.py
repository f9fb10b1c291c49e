"""CPU: the oracle of the PointNet backward (tests/pointnet_backward_oracle.py) against autograd through the restated reference
(oracle/scene.py), in float64."""
import torch

import pointnet_backward_oracle as pbo
from oracle import scene as osc


def _leaves(c):
    x = c['x'].clone().requires_grad_(True)
    sd = {k: v.clone().requires_grad_(True) for k, v in c['sd'].items()}
    return x, sd


def test_lowest_row_argmax_on_ties_nan_and_empty_segments():
    nan = float('nan')
    inf = float('inf')
    x = torch.tensor([[1., 5.], [3., 5.], [3., nan], [nan, nan], [2., -1.], [-inf, inf], [-inf, nan]])
    idx = torch.tensor([0, 0, 0, 2, 3, 4, 4])
    assert pbo.lowest_row_argmax(x, idx, 6).tolist() == [[1, 0], [-1, -1], [-1, -1], [4, 4], [5, 5], [-1, -1]]
    assert pbo.highest_row_argmax(x, idx, 6).tolist() == [[2, 1], [-1, -1], [-1, -1], [4, 4], [6, 5], [-1, -1]]


def test_stock_route_is_autograd_through_the_reference_without_ties():
    c = pbo.case(3, 16, 8, 19, 200, 30)
    x, sd = _leaves(c)
    tr = {}
    out = pbo.stock_route(x, c['idx'], c['n_idx'], sd, trace=tr)
    assert min(pbo.runner_up_gap(tr['x%d' % k], c['idx'], c['n_idx']) for k in range(1, 5)) > 0      # no two equal maxima
    got = pbo.gradients(out, c['proj'], x, sd)
    x2, sd2 = _leaves(c)
    ref_out = osc.pointnet(x2, c['idx'], c['n_idx'], sd2)
    want = pbo.gradients(ref_out, c['proj'], x2, sd2)
    assert torch.equal(out, ref_out)
    assert list(got) == list(want) and len(got) == 13
    for k in want:
        assert float(want[k].abs().max()) > 0
        torch.testing.assert_close(got[k], want[k], rtol=1e-12, atol=1e-14 * float(want[k].abs().max()))
    # ... and the frozen graph with the decisions of that forward is the same function and has the same gradients
    x3, sd3 = _leaves(c)
    masks = {k: tr[k] > 0 for k in pbo.RELU_ARGS}
    fr = pbo.frozen_route(x3, c['idx'], sd3, masks, tr)
    torch.testing.assert_close(fr, ref_out, rtol=1e-13, atol=1e-14)
    frozen = pbo.gradients(fr, c['proj'], x3, sd3)
    for k in want:
        torch.testing.assert_close(frozen[k], want[k], rtol=1e-12, atol=1e-14 * float(want[k].abs().max()))


def test_duplicated_rows_tell_the_three_tie_rules_apart():
    """Rows 0..39 appear twice, in the same voxel: every maximum one of them holds is held by two rows.  Lowest row, highest row and
    the even split are three different gradients of x; what the two copies receive TOGETHER is the same under all three."""
    c = pbo.case(4, 16, 8, 19, 160, 20)
    c['x'] = torch.cat((c['x'], c['x'][:40]))
    c['idx'] = torch.cat((c['idx'], c['idx'][:40]))
    g = {}
    for name, route in (('lowest', lambda x, sd: pbo.stock_route(x, c['idx'], c['n_idx'], sd)),
                        ('highest', lambda x, sd: pbo.stock_route(x, c['idx'], c['n_idx'], sd, argmax=pbo.highest_row_argmax)),
                        ('even', lambda x, sd: pbo.even_split_route(x, c['idx'], c['n_idx'], sd))):
        x, sd = _leaves(c)
        g[name] = pbo.gradients(route(x, sd), c['proj'], x, sd)
    scale = float(g['even']['x'].abs().max())
    for a, b in (('lowest', 'highest'), ('lowest', 'even'), ('highest', 'even')):
        assert float((g[a]['x'] - g[b]['x']).abs().max()) > 1e-3 * scale, (a, b)
    both = lambda t: t[:40] + t[160:]
    for name in ('highest', 'even'):
        torch.testing.assert_close(both(g[name]['x']), both(g['lowest']['x']), rtol=1e-10, atol=1e-13 * scale)
        torch.testing.assert_close(g[name]['x'][40:160], g['lowest']['x'][40:160], rtol=1e-10, atol=1e-13 * scale)
    torch.testing.assert_close(g['even']['x'][:40], 0.5 * both(g['lowest']['x']), rtol=1e-10, atol=1e-13 * scale)
    # the duplicates change no forward value, so no parameter gradient: those agree under all three
    for k in c['sd']:
        torch.testing.assert_close(g['highest'][k], g['lowest'][k], rtol=1e-10, atol=1e-13 * float(g['lowest'][k].abs().max()))


def test_bmin_trick_is_autograd_through_the_reference_anchors():
    """oracle.scene.voxelize builds anchor_pts = idx3d * edge + bbox_min + edge / 2 with bbox_min = pts.min(dim=0)[0] inside the
    graph.  The PointNet input's position columns assembled from DETACHED anchors minus (bmin - bmin.detach()) have the same values
    and the same gradient: the point that holds an axis' minimum receives minus that column's sum on top of its own row."""
    g = torch.Generator().manual_seed(11)
    pts0 = torch.rand((300, 3), generator=g, dtype=torch.float64) * torch.tensor([1.3, 0.9, 0.7], dtype=torch.float64) + 0.011
    batch = torch.zeros(300, dtype=torch.long)
    proj = torch.randn((300, 3), generator=g, dtype=torch.float64)
    pts = pts0.clone().requires_grad_(True)
    anchor_pts, _, _, edges = osc.voxelize(pts, batch, 0.16)
    assert anchor_pts.requires_grad and anchor_pts.shape[0] > 20
    ref = pts[edges[1]] - anchor_pts[edges[0]]
    want, = torch.autograd.grad((ref * proj).sum(), pts)

    p2 = pts0.clone().requires_grad_(True)
    bmin = p2.min(dim=0)[0]
    rel = p2.index_select(0, edges[1]) - anchor_pts.detach().index_select(0, edges[0]) - (bmin - bmin.detach())
    got, = torch.autograd.grad((rel * proj).sum(), p2)
    assert torch.equal(rel.detach(), ref.detach())
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    extra = got - proj                                          # e1 is arange: without the anchors' path the gradient is proj
    rows = pts0.argmin(dim=0)
    expect = torch.zeros_like(extra)
    expect[rows, torch.arange(3)] = -proj.sum(dim=0)
    torch.testing.assert_close(extra, expect, rtol=1e-12, atol=1e-12)
