"""Oracle of the PointNet backward (3dvnet_amd/training.py ``pointnet``), stock torch ops on any device and in any
float dtype.  TEST INFRASTRUCTURE ONLY.

  * ``lowest_row_argmax`` / ``highest_row_argmax``: the row that holds a segment's maximum, per column; -1 for a segment without rows
    (or with NaN rows only).  Lowest row among equal values is ``v3d_segment_max_arg_f32``'s rule, torch_scatter's on the CPU;
  * ``stock_route``: ``oracle.scene.pointnet`` with every pooling as ``x.gather(0, arg)``, ``arg`` built under ``no_grad``: the whole
    gradient of a pooled value goes to ONE row (torch's ``scatter_reduce('amax')`` splits it evenly among equal values);
  * ``frozen_route``: the same graph with every decision taken from outside: each ReLU is a multiplication by a given 0/1 mask, each
    pooling a gather by a given ``arg`` table.  It is smooth in its inputs, so two evaluations in different precisions differ by
    rounding alone, wherever the activations lie;
  * ``case`` / ``margins``: the random cases of the tests and how far their float64 stock graph stays from a kink.
"""
import torch
import torch.nn.functional as F

LAYERS = ('fc_pos', 'fc1', 'fc2', 'fc3', 'fc4', 'fc_out')
RELU_ARGS = ('h0', 'x1', 'x2', 'x3', 'pool1', 'pool2', 'pool3', 'pool4')        # what a ReLU reads (x4 is pooled only)
_NEG_INF = float('-inf')


def _segment_max(x, idx, n_idx):
    out = x.new_full((n_idx, x.shape[1]), _NEG_INF)
    x = torch.nan_to_num(x, nan=_NEG_INF, posinf=float('inf'), neginf=_NEG_INF)            # a NaN never wins; infinities stay
    return out.scatter_reduce(0, idx.view(-1, 1).expand_as(x), x, 'amax', include_self=True)


def _extreme_row(x, idx, n_idx, lowest):
    idx = idx.long()
    n = x.shape[0]
    top = _segment_max(x, idx, n_idx)
    rows = torch.arange(n, device=x.device).view(-1, 1).expand_as(x)
    hit = (x == top[idx])                                                       # a NaN equals nothing
    e = idx.view(-1, 1).expand_as(x)
    if lowest:
        arg = torch.full((n_idx, x.shape[1]), n, dtype=torch.long, device=x.device)
        arg = arg.scatter_reduce(0, e, torch.where(hit, rows, torch.full_like(rows, n)), 'amin', include_self=True)
        return torch.where(arg == n, torch.full_like(arg, -1), arg)
    arg = torch.full((n_idx, x.shape[1]), -1, dtype=torch.long, device=x.device)
    return arg.scatter_reduce(0, e, torch.where(hit, rows, torch.full_like(rows, -1)), 'amax', include_self=True)


def lowest_row_argmax(x, idx, n_idx):
    """arg [n_idx, C] int64: the lowest row r with idx[r] == s and x[r, c] == max of segment s; -1 where there is none."""
    return _extreme_row(x, idx, n_idx, True)


def highest_row_argmax(x, idx, n_idx):
    return _extreme_row(x, idx, n_idx, False)


def gather_pool(x, arg, empty=_NEG_INF):
    """x [n, C], arg [n_idx, C] -> x[arg[s, c], c]; ``empty`` where arg is -1"""
    return torch.where(arg >= 0, x.gather(0, arg.clamp(min=0)), x.new_full((), empty))


def _lin(t, sd, name):
    return F.linear(t, sd[name + '.weight'], sd[name + '.bias'])


def stock_route(x, idx, n_idx, sd, argmax=lowest_row_argmax, trace=None):
    """scenemodeling.py:127-144 with single-winner poolings -> [n_idx, out_dim]; ``trace`` receives h0, x1..x4, pool1..4, arg1..4"""
    idx = idx.long()
    tr = {}
    tr['h0'] = _lin(x, sd, 'fc_pos')
    y = _lin(F.relu(tr['h0']), sd, 'fc1')
    for k in range(1, 5):
        tr['x%d' % k] = y
        with torch.no_grad():
            tr['arg%d' % k] = argmax(y, idx, n_idx)
        pool = tr['pool%d' % k] = gather_pool(y, tr['arg%d' % k])
        if k < 4:
            y = _lin(F.relu(torch.cat((y, pool[idx]), dim=1)), sd, 'fc%d' % (k + 1))
    if trace is not None:
        trace.update({k: v.detach() for k, v in tr.items()})
    return _lin(F.relu(pool), sd, 'fc_out')


def even_split_route(x, idx, n_idx, sd):
    """the same network through torch's own scatter_reduce('amax'), whose backward splits a gradient evenly among equal values"""
    idx = idx.long()
    y = _lin(F.relu(_lin(x, sd, 'fc_pos')), sd, 'fc1')
    e = idx.view(-1, 1).expand(-1, y.shape[1])
    pool = lambda t: t.new_zeros((n_idx, t.shape[1])).scatter_reduce(0, e, t, 'amax', include_self=False)
    for name in ('fc2', 'fc3', 'fc4'):
        y = _lin(F.relu(torch.cat((y, pool(y)[idx]), dim=1)), sd, name)
    return _lin(F.relu(pool(y)), sd, 'fc_out')


def frozen_route(x, idx, sd, masks, args, trace=None):
    """The graph of ``stock_route`` with its decisions given: ``masks[name]`` (bool, name in RELU_ARGS) in place of ``t > 0``,
    ``args['arg1'..'arg4']`` (-1: the pooled value is taken as 0, and its mask must be False) in place of the argmax."""
    idx = idx.long()
    m = {k: v.to(x.dtype) for k, v in masks.items()}
    tr = {}
    tr['h0'] = _lin(x, sd, 'fc_pos')
    y = _lin(tr['h0'] * m['h0'], sd, 'fc1')
    for k in range(1, 5):
        tr['x%d' % k] = y
        pool = tr['pool%d' % k] = gather_pool(y, args['arg%d' % k].long(), empty=0.0)
        if k < 4:
            y = _lin(torch.cat((y * m['x%d' % k], (pool * m['pool%d' % k])[idx]), dim=1), sd, 'fc%d' % (k + 1))
    if trace is not None:
        trace.update({k: v.detach() for k, v in tr.items()})
    return _lin(pool * m['pool4'], sd, 'fc_out')


def case(seed, hidden, out_dim, in_dim, n_pts, n_vox, n_empty=0, dtype=torch.float64):
    """A random PointNet, its input and a loss, all from ``seed``, on the CPU -> dict(sd, x, idx, n_idx, proj).  Every voxel but the
    last ``n_empty`` holds a point; the rows of a voxel are spread over the whole input."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, (ci, co) in zip(LAYERS, ((in_dim, hidden), (hidden, hidden), (2 * hidden, hidden), (2 * hidden, hidden),
                                       (2 * hidden, hidden), (hidden, out_dim))):
        b = ci ** -0.5
        sd[name + '.weight'] = (torch.rand((co, ci), generator=g, dtype=torch.float64) * 2 - 1) * b
        sd[name + '.bias'] = (torch.rand((co,), generator=g, dtype=torch.float64) * 2 - 1) * b
    x = torch.randn((n_pts, in_dim), generator=g, dtype=torch.float64).float().to(dtype)        # float32 values in every dtype
    sd = {k: v.float().to(dtype) for k, v in sd.items()}
    full = n_vox - n_empty
    assert n_pts >= full
    idx = torch.cat((torch.arange(full), torch.randint(0, full, (n_pts - full,), generator=g)))[torch.randperm(n_pts, generator=g)]
    proj = torch.randn((n_vox, out_dim), generator=g, dtype=torch.float64).float().to(dtype)
    return dict(sd=sd, x=x, idx=idx, n_idx=n_vox, proj=proj)


def runner_up_gap(x, idx, n_idx):
    """the smallest difference between a segment's maximum and its second value over all segments with two rows or more and all
    columns (inf if there is none)"""
    idx = idx.long()
    arg = lowest_row_argmax(x, idx, n_idx)
    top = gather_pool(x, arg)
    rest = x.clone()
    cols = torch.arange(x.shape[1], device=x.device).expand_as(arg)
    ok = arg >= 0
    rest[arg[ok], cols[ok]] = _NEG_INF
    second = _segment_max(rest, idx, n_idx)
    gap = top - second
    return float(gap[torch.isfinite(gap)].min()) if bool(torch.isfinite(gap).any()) else float('inf')


def margins(tr64, tr32, idx, n_idx):
    """(smallest |ReLU argument| of the float64 trace, smallest winner / runner-up gap of its four poolings, largest |float32 -
    float64| over the activations h0, x1..x4)"""
    arg_min = min(float(tr64[k][torch.isfinite(tr64[k])].abs().min()) for k in RELU_ARGS)
    gap = min(runner_up_gap(tr64['x%d' % k], idx, n_idx) for k in range(1, 5))
    err = max(float((tr32[k].double() - tr64[k]).abs().max()) for k in ('h0', 'x1', 'x2', 'x3', 'x4'))
    return arg_min, gap, err


def gradients(out, proj, x, sd):
    """loss = <out, proj> / n_idx -> {'x': ..., parameter name: ...}"""
    names = ['x'] + list(sd)
    grads = torch.autograd.grad((out * proj).sum() / out.shape[0], [x] + [sd[k] for k in sd])
    return dict(zip(names, grads))
