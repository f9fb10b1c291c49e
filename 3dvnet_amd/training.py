"""Training of the cost-volume stage (stage 1) and of the entry of stage 2: the pieces of ``mv3d/subnetworks/mvsnet.py:186-227``,
of the initial depth supervision (``mv3d/lightningmodel.py:57-63``) and of the back-projected variance with a backward pass.

Only one operation of stage 1 has no stock-torch route that is usable on the device: the fused warp + variance (rows
A1-A4).  Its backward is ``csrc/psv_backward.hip`` behind ``v3d_psv_variance_backward_f32`` (include/v3d.h); like the forward
it never materialises the warped volume, its square or the sampling grid -- the autograd node saves the features and the edge
tables, nothing of size E * C * D * h * w.  Everything else -- CostRegNet's 3D convolutions, the soft-argmin, the masked MAE
-- runs as stock differentiable torch ops over the parameters the inference modules already hold:

  * ``PlaneSweepVariance`` / ``plane_sweep_variance``   the variance volume as an autograd function of the features;
  * ``costregnet``                                       the regulariser of an existing ``mvsnet.CostRegNet``, functional;
  * ``initial_depth_loss``                               variance -> regulariser -> soft-argmin -> masked MAE.

The entry of stage 2 is the back-projected variance (rows B1-B2 / C1, ``mv3d/lightningmodel.py:132-174, 187-235``).  Its backward
is ``csrc/backproject_backward.hip`` behind ``v3d_backproject_variance_backward_f32``: the only place where a stage-2 loss reaches
the image features and the stage-1 depth.  Its node saves the features, the depth map, the cameras and the edge tables:

  * ``BackprojectVariance`` / ``backproject_variance``   ``(pts, var)``: ``var`` -> features; with ``n == 0`` ``pts`` -> depth;
  * ``feature_rich_pointcloud``                          the differentiable twin of ``construct_feature_rich_pointcloud``;
  * ``pointflow_hypotheses``                             the hypothesis points and features of ``run_pointflow``.

The consumer of those hypotheses is the hypothesis decoder (``mv3d/subnetworks/refinement.py:28-44``, ``lightningmodel.py:
237-241``).  One piece of it has no usable stock route: the sparse trilinear interpolation, whose stock formulation materialises
nq * 8 * C floats per level.  Its backward is ``v3d_sparse_interp_backward_f32`` (``csrc/sparse.hip``): a per-row sum through an
inverted index of the forward's corner table, without atomics, bitwise reproducible:

  * ``SparseInterpolate`` / ``sparse_interpolate``       one level at the hypothesis points -> level features;
  * ``decoder_features``                                 the wide feature row of ``HypothesisDecoder.features``;
  * ``hypothesis_decoder``                               Conv1d / BatchNorm1d / ReLU stack, head and softmax, functional;
  * ``pointflow_offset``                                 hypotheses -> features -> decoder -> expected offset of ``run_pointflow``.

Cameras, plane depths, offsets and edges are data (no gradient), as in the reference, which also builds every sampling grid under
``no_grad``.  The image-feature gradients are summed with fp32 atomic adds: their last bits can differ from call to call (DESIGN.md
4.1b, 4.1c).  Out of scope: the rest of stage 2 (PointNet and the sparse U-Net: they connect to the level-feature gradients
produced here), stage 3, the native backbone, the split / channel-last variance formats, ``PL3DVNet.forward`` in training mode,
an optimiser loop.  No CPU fallback.
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib, lightningmodel, mvsnet


def _feature_gradient(features, grad_var, shape, call):
    """The feature-gradient plumbing both backward passes share.  ``features`` [n_img, C, Hf, Wf] of any float dtype and layout go
    in as a channel-last fp32 copy; ``grad_var`` (or None: no feature gradient is wanted) as an fp32 contiguous copy of ``shape``;
    ``call(feat_cl, grad_var, grad_cl)`` runs the entry point, which zero-fills the target ``grad_cl`` [n_img, Hf, Wf, C] itself (None
    with ``grad_var``); -> the gradient in the shape and dtype of ``features``, or None."""
    n_img, C, Hf, Wf = features.shape
    feat_cl = features.detach().float().permute(0, 2, 3, 1).contiguous()
    grad_cl = None
    if grad_var is not None:
        # a .sum() upstream hands autograd a stride-0 expanded tensor, a slice a non-contiguous one
        grad_var = grad_var.float().contiguous()
        assert grad_var.shape == shape
        grad_cl = torch.empty((n_img, Hf, Wf, C), dtype=torch.float32, device=features.device)
    call(feat_cl, grad_var, grad_cl)
    return None if grad_cl is None else grad_cl.permute(0, 3, 1, 2).to(features.dtype)


class PlaneSweepVariance(torch.autograd.Function):
    """``mvsnet.plane_sweep_variance`` (the same kernel: the same bits) with a backward with respect to the features."""

    @staticmethod
    def forward(ctx, features_quarter, Kc, Rc, tc, ref_img, edge_ofs, edge_src, geom):
        depth_start, depth_interval, n_planes, img_size, depth_img_size = geom
        csr = mvsnet.EdgeCsr((ref_img.to(torch.int64), ref_img, edge_ofs, edge_src))
        var = mvsnet.plane_sweep_variance(features_quarter, Rc, tc, Kc, None, depth_start, depth_interval, n_planes, img_size,
                                          depth_img_size, csr=csr)
        ctx.save_for_backward(features_quarter, Kc, Rc, tc, ref_img, edge_ofs, edge_src)
        ctx.geom = geom
        return var

    @staticmethod
    def backward(ctx, grad_var):
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        features_quarter, Kc, Rc, tc, ref_img, edge_ofs, edge_src = ctx.saved_tensors
        depth_start, depth_interval, n_planes, img_size, depth_img_size = ctx.geom
        lib = _lib.load()
        dev = features_quarter.device
        n_img, C, Hf, Wf = features_quarter.shape
        h, w = depth_img_size

        def call(feat_cl, grad_var, grad_cl):
            with torch.cuda.device(dev):
                rc = lib.v3d_psv_variance_backward_f32(
                    _lib.ptr(feat_cl), _lib.ptr(Kc), _lib.ptr(Rc), _lib.ptr(tc), _lib.ptr(ref_img), _lib.ptr(edge_ofs),
                    _lib.ptr(edge_src), n_img, ref_img.shape[0], edge_src.shape[0], C, Hf, Wf, int(img_size[0]), int(img_size[1]),
                    float(depth_start), float(depth_interval), int(n_planes), int(h), int(w), _lib.ptr(grad_var),
                    _lib.ptr(grad_cl), _lib.stream_ptr(dev))
            _lib.check(rc, 'v3d_psv_variance_backward_f32')
        return (_feature_gradient(features_quarter, grad_var, (ref_img.shape[0], C, n_planes, h, w), call),) + (None,) * 7


def plane_sweep_variance(features_quarter, rotmats, tvecs, K, ref_src_edges, depth_start, depth_interval, n_planes, img_size,
                         depth_img_size, csr=None, n_ref=None):
    """Rows A1-A4 (mvsnet.py:186-216) as a differentiable function of ``features_quarter`` [n_img, C, Hf, Wf] (C in {16, 32}):
    the variance volume [n_ref, C, D, h, w] of ``mvsnet.plane_sweep_variance``, bit for bit.  ``csr`` / ``n_ref`` as there."""
    mvsnet._require_cuda(features_quarter, 'training.plane_sweep_variance')
    dev = features_quarter.device
    if csr is None:
        csr = mvsnet.edges_to_csr(ref_src_edges.to(dev), n_ref=n_ref, n_img=features_quarter.shape[0])
    _, ref_img, edge_ofs, edge_src = csr
    Kc, Rc, tc = (x.detach().to(dev).contiguous().float() for x in (K, rotmats, tvecs))
    geom = (float(depth_start), float(depth_interval), int(n_planes), (int(img_size[0]), int(img_size[1])),
            (int(depth_img_size[0]), int(depth_img_size[1])))
    return PlaneSweepVariance.apply(features_quarter, Kc, Rc, tc, ref_img, edge_ofs, edge_src, geom)


class BackprojectVariance(torch.autograd.Function):
    """``lightningmodel.backproject_variance`` (the same kernel: the same bits) -> ``(pts, var)`` with the two gradients the
    reference has (lightningmodel.py:132-174, 187-235; the grid is built under ``no_grad`` there): ``var`` -> features, and, for
    ``n == 0`` only, ``pts`` -> depth.  With ``n > 0`` ``pts`` is non-differentiable and the depth receives no gradient."""

    @staticmethod
    def forward(ctx, depth_pred, img_feats, Kc, Rc, tc, ref_img, edge_ofs, edge_src, geom):
        img_size, offset, n = geom
        pts, var = lightningmodel.backproject_variance(depth_pred, img_feats, Rc, tc, Kc, None, img_size, offset=offset, n=n,
                                                       csr=(None, ref_img, edge_ofs, edge_src))
        # the depth map is a few hundred KB: its clone keeps the reference's `depth_pred += offset_pred` legal between forward
        # and backward.  Nothing of size E * C * n_hyp * P is kept.
        ctx.save_for_backward(img_feats, depth_pred.detach().clone(), Kc, Rc, tc, ref_img, edge_ofs, edge_src)
        ctx.geom = geom
        ctx.set_materialize_grads(False)
        if n > 0:
            ctx.mark_non_differentiable(pts)
        return pts, var

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_pts, grad_var):
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * 9
        img_size, offset, n = ctx.geom
        # only the pair(s) needed: an output the loss does not use arrives as None (set_materialize_grads(False))
        want_depth = ctx.needs_input_grad[0] and n == 0 and grad_pts is not None
        want_feat = ctx.needs_input_grad[1] and grad_var is not None
        if not (want_depth or want_feat):
            return (None,) * 9
        img_feats, depth, Kc, Rc, tc, ref_img, edge_ofs, edge_src = ctx.saved_tensors
        lib = _lib.load()
        dev = img_feats.device
        n_img, C, Hf, Wf = img_feats.shape
        n_ref, h, w = depth.shape
        rows = n_ref * h * w
        d = depth.float().contiguous()
        grad_depth = None
        if want_depth:
            grad_pts = grad_pts.float().contiguous()            # stride-0 or sliced, as grad_var (_feature_gradient)
            assert grad_pts.shape == (rows, 1, 3)
            grad_depth = torch.empty((n_ref, h, w), dtype=torch.float32, device=dev)       # every element is written

        def call(feat_cl, grad_var, grad_cl):
            with torch.cuda.device(dev):
                rc = lib.v3d_backproject_variance_backward_f32(
                    _lib.ptr(d), _lib.ptr(feat_cl), _lib.ptr(Kc), _lib.ptr(Rc), _lib.ptr(tc), _lib.ptr(ref_img), _lib.ptr(edge_ofs),
                    _lib.ptr(edge_src), n_img, n_ref, edge_src.shape[0], C, Hf, Wf, int(img_size[0]), int(img_size[1]), h, w,
                    float(offset), int(n), _lib.ptr(grad_var), _lib.ptr(grad_pts if want_depth else None), _lib.ptr(grad_cl),
                    _lib.ptr(grad_depth), _lib.stream_ptr(dev))
            _lib.check(rc, 'v3d_backproject_variance_backward_f32')
        grad_feats = _feature_gradient(img_feats, grad_var if want_feat else None, (rows, 2 * n + 1, C), call)
        return (grad_depth.to(depth.dtype) if want_depth else None, grad_feats) + (None,) * 7


def backproject_variance(depth_pred, img_feats, rotmats, tvecs, K, ref_src_edges, img_size, offset=0.0, n=0, csr=None):
    """Rows B1-B2 / C1 as a differentiable function: -> ``(pts [n_ref*P, 2n+1, 3], var [n_ref*P, 2n+1, C])`` of
    ``lightningmodel.backproject_variance``, bit for bit.  ``var`` is differentiable with respect to ``img_feats`` [n_img, C, Hf,
    Wf] (C in {16, 32}); with ``n == 0`` ``pts`` is differentiable with respect to ``depth_pred`` [n_ref, h, w].  ``csr``: the
    result of ``mvsnet.edges_to_csr(ref_src_edges)`` when the caller holds it."""
    mvsnet._require_cuda(depth_pred, 'training.backproject_variance')
    mvsnet._require_cuda(img_feats, 'training.backproject_variance')
    dev = depth_pred.device
    if csr is None:
        csr = mvsnet.edges_to_csr(ref_src_edges.to(dev))
    _, ref_img, edge_ofs, edge_src = csr
    Kc, Rc, tc = (x.detach().to(dev).contiguous().float() for x in (K, rotmats, tvecs))
    geom = ((int(img_size[0]), int(img_size[1])), float(offset), int(n))
    return BackprojectVariance.apply(depth_pred, img_feats, Kc, Rc, tc, ref_img, edge_ofs, edge_src, geom)


def _pts_batch(depth_pred, depth_batch):
    n_ref, h, w = depth_pred.shape
    return depth_batch.unsqueeze(1).expand(n_ref, h * w).reshape(-1)


def feature_rich_pointcloud(depth_pred, depth_batch, img_feats, rotmats, tvecs, K, ref_src_edges, img_size, csr=None):
    """The differentiable twin of ``PL3DVNet.construct_feature_rich_pointcloud`` (lightningmodel.py:132-174) -> ``(pts [Np, 3],
    pts_feat [Np, C], pts_batch [Np])``: ``pts`` carries the gradient to ``depth_pred``, ``pts_feat`` to ``img_feats``."""
    pts, var = backproject_variance(depth_pred, img_feats, rotmats, tvecs, K, ref_src_edges, img_size, csr=csr)
    return pts.view(-1, 3), var.view(-1, var.shape[-1]), _pts_batch(depth_pred, depth_batch)


def pointflow_hypotheses(depth_pred, depth_batch, img_feats, rotmats, tvecs, K, ref_src_edges, offset, n, img_size, csr=None):
    """The hypothesis points and features of ``run_pointflow`` (lightningmodel.py:187-235) -> ``(pts_hyp [Np, 2n+1, 3], pts_feat
    [Np, 2n+1, C], pts_batch [Np])``.  The gradient reaches ``img_feats`` only: the reference builds ``pts_hyp`` and the grid
    under ``no_grad``."""
    pts_hyp, pts_feat = backproject_variance(depth_pred, img_feats, rotmats, tvecs, K, ref_src_edges, img_size, offset=offset,
                                             n=n, csr=csr)
    return pts_hyp, pts_feat, _pts_batch(depth_pred, depth_batch)


def _level_min_pts(x):
    """scatter(x.pts, x.batch, reduce='min') (refinement.py:33), cached on the level dict as ``HypothesisDecoder.features`` does."""
    if '_min_pts' not in x:
        nb = int(x['batch'].max().item()) + 1
        x['_min_pts'] = torch.stack([x['pts'][x['batch'] == b].amin(dim=0) for b in range(nb)]) \
            if nb > 1 else x['pts'].amin(dim=0, keepdim=True)
    return x['_min_pts']


class SparseInterpolate(torch.autograd.Function):
    """``v3d_sparse_interp_f32`` (``MinkowskiInterpolation``, refinement.py:26,39) -> [n_pts, n_hyp, C] with its one gradient,
    to the level features: ``v3d_sparse_interp_backward_f32`` (no atomics, bitwise reproducible).  The node
    saves the queries, their batch indices, ``min_pts`` and the hash table: 12 bytes per query, nothing of size nq * 8 * C."""

    @staticmethod
    def forward(ctx, feats, pts, pts_batch, table, min_pts, geom):
        n_in, stride, res = geom
        lib = _lib.load()
        dev = pts.device
        n_pts, n_hyp = pts.shape[:2]
        f = feats.detach().float().contiguous()
        assert f.shape[0] == n_in
        C = f.shape[1]
        out = torch.empty((n_pts, n_hyp, C), dtype=torch.float32, device=dev)
        ws = torch.empty(lib.v3d_sparse_interp_workspace_bytes(n_pts, n_hyp), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = lib.v3d_sparse_interp_f32(_lib.ptr(table), n_in, _lib.ptr(f), C, stride, _lib.ptr(pts), _lib.ptr(pts_batch),
                                           n_pts, n_hyp, _lib.ptr(min_pts), res, _lib.ptr(out), C, 0, _lib.ptr(ws), ws.numel(),
                                           _lib.stream_ptr(dev))
        _lib.check(rc, 'v3d_sparse_interp_f32')
        ctx.save_for_backward(pts, pts_batch, table, min_pts)
        ctx.geom = geom
        ctx.feats_meta = (C, feats.dtype)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        pts, pts_batch, table, min_pts = ctx.saved_tensors
        n_in, stride, res = ctx.geom
        C, dtype = ctx.feats_meta
        lib = _lib.load()
        dev = pts.device
        n_pts, n_hyp = pts.shape[:2]
        assert grad_out.shape == (n_pts, n_hyp, C)
        # the backward of `cat` hands out a view of the wide feature row: its own row stride is passed on (ld_grad) instead of
        # copying it.  Anything else (a stride-0 expanded tensor of a .sum(), a transposed view) becomes one contiguous copy.
        g = grad_out
        st = g.stride()
        strided = g.dtype == torch.float32 and n_pts * n_hyp > 0 and st[2] == 1 and st[1] >= C and st[0] == n_hyp * st[1]
        if not strided:
            g = g.float().contiguous()
        ld = g.stride(1)
        grad_feats = torch.empty((n_in, C), dtype=torch.float32, device=dev)        # every element is written
        ws = torch.empty(lib.v3d_sparse_interp_backward_workspace_bytes(n_in, C, n_pts, n_hyp), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc = lib.v3d_sparse_interp_backward_f32(_lib.ptr(table), n_in, C, stride, _lib.ptr(pts), _lib.ptr(pts_batch), n_pts,
                                                    n_hyp, _lib.ptr(min_pts), res, g.data_ptr(), ld, 0, _lib.ptr(grad_feats),
                                                    _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
        _lib.check(rc, 'v3d_sparse_interp_backward_f32')
        return (grad_feats.to(dtype),) + (None,) * 5


def sparse_interpolate(x, pts, pts_batch, feats=None):
    """Sparse trilinear interpolation of one level of ``SparseUNet.forward`` (``x``: its dict with ``'sparse'``, ``'stride'``,
    ``'res'``, ``'pts'``, ``'batch'``) at ``pts`` [n_pts, n_hyp, 3] -> [n_pts, n_hyp, C]: the bits of the corresponding columns
    of ``HypothesisDecoder.features``, differentiable in ``feats`` [N, C] (default ``x['feats']``; a leaf or the output of a
    differentiable U-Net).  ``pts`` and ``pts_batch`` [n_pts] are data: the reference builds the hypotheses under ``no_grad``."""
    mvsnet._require_cuda(pts, 'training.sparse_interpolate')
    feats = x['feats'] if feats is None else feats
    mvsnet._require_cuda(feats, 'training.sparse_interpolate')
    lv = x['sparse']
    assert feats.dim() == 2 and feats.shape[0] == lv.n, (tuple(feats.shape), lv.n)
    pts = pts.detach().contiguous().float()
    pts_batch = pts_batch.contiguous().long()
    min_pts = _level_min_pts(x).detach().contiguous().float()
    return SparseInterpolate.apply(feats, pts, pts_batch, lv.table, min_pts, (int(lv.n), int(x['stride']), float(x['res'])))


def decoder_features(xs, pts, pts_feat, pts_batch, level_feats=None):
    """Row C2a as a differentiable function -> [n_pts, n_hyp, in_dim] in the layout (and with the bits) of
    ``HypothesisDecoder.features``: finest level first, ``pts_feat`` last (refinement.py:32-41).  ``xs``: the levels of
    ``SparseUNet.forward``, coarse to fine; ``level_feats``: one [N_l, C_l] tensor per level in the order of ``xs`` (default
    ``x['feats']``).  Differentiable in the level features and in ``pts_feat`` (None: no point features)."""
    if level_feats is None:
        level_feats = [None] * len(xs)
    assert len(level_feats) == len(xs)
    features = pts_feat
    for x, f in zip(xs, level_feats):
        feats = sparse_interpolate(x, pts, pts_batch, f)
        features = feats if features is None else torch.cat((feats, features.to(feats.dtype)), dim=2)
    return features


def hypothesis_decoder(decoder, features, bn_training=False):
    """The Conv1d + BatchNorm1d + ReLU stack, the Conv1d head and the softmax of ``HypothesisDecoder.forward``
    (refinement.py:42-43) with stock differentiable torch ops over the parameters and buffers of an existing
    ``refinement.HypothesisDecoder`` (no second parameter set; its ``state_dict`` keys are untouched).  features [n_pts, n_hyp,
    in_dim] -> preds [n_pts, n_hyp].  ``bn_training`` as in ``costregnet``."""
    y = features.transpose(2, 1)
    for i in range(3):
        conv, bn = decoder.net[i][0], decoder.net[i][1]
        y = F.conv1d(y, conv.weight, None, stride=conv.stride, padding=conv.padding)
        y = F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, training=bn_training, momentum=bn.momentum,
                         eps=bn.eps)
        y = F.relu(y)
    head = decoder.net[3]
    y = F.conv1d(y, head.weight, head.bias, stride=head.stride, padding=head.padding)
    return F.softmax(y.squeeze(1), dim=1)


def pointflow_offset(decoder, xs, depth_pred, depth_batch, img_feats, rotmats, tvecs, K, ref_src_edges, offset, n, img_size,
                     level_feats=None, bn_training=False, csr=None):
    """``run_pointflow`` (lightningmodel.py:187-242) as a differentiable function -> the expected offset [n_ref, h, w]; the caller
    forms ``depth_pred + offset`` and applies ``masked_mae`` (lightningmodel.py:70-79).  The gradient reaches the level
    features (``level_feats``, default each ``x['feats']``), ``img_feats`` (through the point features) and every parameter of
    ``decoder``; none reaches ``depth_pred``: the hypotheses are data."""
    pts_hyp, pts_feat, pts_batch = pointflow_hypotheses(depth_pred, depth_batch, img_feats, rotmats, tvecs, K, ref_src_edges,
                                                        offset, n, img_size, csr=csr)
    features = decoder_features(xs, pts_hyp, pts_feat, pts_batch, level_feats=level_feats)
    preds = hypothesis_decoder(decoder, features, bn_training=bn_training)
    offset_vals = torch.linspace(-n * offset, n * offset, 2 * n + 1).to(preds)       # on the CPU, then moved (:238-240)
    return torch.sum(offset_vals.unsqueeze(0) * preds, dim=1).view(depth_pred.shape)


def _conv_bn_relu(mod, x, bn_training):
    if hasattr(mod, 'deconv'):
        d = mod.deconv
        y = F.conv_transpose3d(x, d.weight, None, stride=d.stride, padding=d.padding, output_padding=d.output_padding)
    else:
        y = F.conv3d(x, mod.conv.weight, None, stride=mod.conv.stride, padding=mod.conv.padding)
    bn = mod.bn
    y = F.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, training=bn_training, momentum=bn.momentum,
                     eps=bn.eps)
    return F.relu(y)


def costregnet(cnn_3d, x, bn_training=False):
    """CostRegNet.forward (mvsnet.py:154-163) with stock differentiable torch ops over the parameters and buffers of an
    existing ``mvsnet.CostRegNet`` (no second parameter set; its ``state_dict`` keys are untouched).  x [B, Cin, D, h, w] ->
    [B, 1, D, h, w].  ``bn_training=False``: running statistics (the reference's ``freeze_batchnorm`` mode);
    ``bn_training=True``: batch statistics, and the running buffers are updated."""
    m = cnn_3d
    conv0 = _conv_bn_relu(m.conv0, x, bn_training)
    conv2 = _conv_bn_relu(m.conv2, _conv_bn_relu(m.conv1, conv0, bn_training), bn_training)
    conv4 = _conv_bn_relu(m.conv4, _conv_bn_relu(m.conv3, conv2, bn_training), bn_training)
    y = _conv_bn_relu(m.conv6, _conv_bn_relu(m.conv5, conv4, bn_training), bn_training)
    y = conv4 + _conv_bn_relu(m.conv7, y, bn_training)
    y = conv2 + _conv_bn_relu(m.conv8, y, bn_training)
    y = conv0 + _conv_bn_relu(m.conv9, y, bn_training)
    return F.conv3d(y, m.prob.weight, m.prob.bias, stride=1, padding=1)


def masked_mae(depth_pred, depth_gt, depth_interval):
    """The reference's ``MAELoss.forward`` (mv3d/loss.py:6-20) in differentiable torch: ground truth of another size reduced
    with a nearest resize, pixels with ``gt != 0`` only, ``+ 1e-7`` in the denominator, in units of ``depth_interval``, mean
    over the views."""
    if depth_gt.shape != depth_pred.shape:
        depth_gt = F.interpolate(depth_gt.unsqueeze(1), depth_pred.shape[-2:], mode='nearest').squeeze(1)
    mask = (depth_gt != 0).to(depth_pred.dtype)
    denom = mask.sum(dim=(1, 2)) + 1e-7
    mae = (mask * (depth_pred - depth_gt).abs()).sum(dim=(1, 2))
    return ((mae / depth_interval) / denom).mean()


def initial_depth_loss(mvsnet_module, features_quarter, batch, depth_config, depth_gt, bn_training=False):
    """Stage 1 with its supervision (mvsnet.py:186-227, lightningmodel.py:57-63) -> ``(loss, depth [n_ref, h, w])``.
    ``mvsnet_module``: an ``mvsnet.MVSNet`` (its ``cnn_3d`` and ``img_size`` are used); ``features_quarter`` comes from the
    caller's own differentiable backbone or is a leaf; ``depth_config``: ``depth_start``, ``depth_interval``, ``n_intervals``,
    ``size``; ``depth_gt`` [n_ref, H, W].  The gradient of the loss reaches ``features_quarter`` and every parameter of
    ``cnn_3d``."""
    start, interval, n_planes = depth_config['depth_start'], depth_config['depth_interval'], depth_config['n_intervals']
    var = plane_sweep_variance(features_quarter, batch.rotmats, batch.tvecs, batch.K, batch.ref_src_edges, start, interval,
                               n_planes, mvsnet_module.img_size, depth_config['size'])
    x_reg = costregnet(mvsnet_module.cnn_3d, var, bn_training=bn_training).squeeze(1)
    prob = F.softmax(-x_reg, dim=1)
    vals = mvsnet_module.depth_values(start, interval, n_planes, var.device).view(1, n_planes, 1, 1)
    depth = torch.sum(vals * prob, dim=1)
    return masked_mae(depth, depth_gt.to(depth.device), interval), depth
