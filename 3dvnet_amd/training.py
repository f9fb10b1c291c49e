"""Training of the cost-volume stage (stage 1) and of stage 2 -- its entry, PointNet and the voxel pooling, the sparse U-Net and the
hypothesis decoder: the pieces of ``mv3d/subnetworks/mvsnet.py:186-227``, of the initial depth supervision
(``mv3d/lightningmodel.py:57-63``), of the back-projected variance, of ``model_scene`` and of ``run_pointflow`` with a backward pass.

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
nq * 8 * C floats per level.  Its backward is ``v3d_sparse_interp_backward_f32`` (``csrc/sparse_interp.hip``): a per-row sum through an
inverted index of the forward's corner table, without atomics, bitwise reproducible:

  * ``SparseInterpolate`` / ``sparse_interpolate``       one level at the hypothesis points -> level features;
  * ``decoder_features``                                 the wide feature row of ``HypothesisDecoder.features``;
  * ``hypothesis_decoder``                               Conv1d / BatchNorm1d / ReLU stack, head and softmax, functional;
  * ``pointflow_offset``                                 hypotheses -> features -> decoder -> expected offset of ``run_pointflow``.

The producer of those level features is the sparse U-Net (``mv3d/subnetworks/scenemodeling.py:147-237``).  Its convolutions have
no usable stock route either: 27 ``index_select`` + ``matmul`` pairs per convolution whose gathered copies autograd keeps.  The
input gradient of a convolution is the forward gather-GEMM (``v3d_sparse_conv_f32``) on the output gradient over the INVERSE
neighbour table with every slab transposed; the weight gradient is ``v3d_sparse_conv_weight_grad_f32`` (``csrc/gemm_wgrad.hip``):
exact-fp32 matrix instructions, partial tiles per row chunk added in chunk order, no atomics, bitwise reproducible.
GroupNorm, ReLU, the residual add and the 1x1 ``feat_adj`` are stock differentiable torch ops over the existing parameters:

  * ``SparseConv`` / ``sparse_conv``                     one convolution (no norm, residual or ReLU) -> x and kernel gradients;
  * ``sparse_unet``                                      ``SparseUNet.forward`` -> the level features, differentiable in the
                                                         input F and in every U-Net parameter; plugs into ``pointflow_offset``.

The producer of F is PointNet (``mv3d/subnetworks/scenemodeling.py:116-144``).  Its stock graph keeps ``cat(x, pool[idx])``
[Np, 2H] three times, sums the pooled gradients with ``index_add`` atomics and, with torch's ``scatter_reduce('amax')``, splits a
gradient among equal values where ``torch_scatter`` hands it to one row.  Here it is one node over three streaming kernels
(``csrc/segment.hip``, beside the forward's pooling: ``v3d_segment_max_arg_f32``, ``v3d_segment_sum_f32``, ``v3d_pointnet_pool_backward_f32``; no atomics,
bitwise reproducible) and ``torch.mm``:

  * ``PointNetFunction`` / ``pointnet``                  ``PointNet.forward`` (the same bits) -> x and the twelve parameters;
  * ``scene_features``                                   the differentiable twin of ``model_scene``: point cloud -> voxels (data)
                                                         -> PointNet -> ``sparse_unet``; with ``pointflow_offset`` and ``masked_mae``
                                                         a loss on a refined depth reaches ``depth_pred``, ``img_feats`` and every
                                                         parameter of stage 2.

Cameras, plane depths, offsets and edges are data (no gradient), as in the reference, which also builds every sampling grid under
``no_grad``.  The image-feature gradients are summed with fp32 atomic adds: their last bits can differ from call to call (DESIGN.md
4.1b, 4.1c).  Out of scope: stage 3, the native backbone, the split / channel-last variance formats, ``PL3DVNet.forward`` in
training mode, an optimiser loop.  No CPU fallback.
"""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib, lightningmodel, mvsnet, utils


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


def _row_matrix(t, C):
    """A [rows, C] gradient as the C ABI takes it -> (tensor, row stride).  The backward of `cat` hands out a view of a wider row:
    its own row stride is passed on when 16-byte loads can read it; anything else (a stride-0 expanded tensor of a .sum(), a
    transposed view, another dtype) becomes one contiguous fp32 copy."""
    st = t.stride()
    if not (t.dtype == torch.float32 and t.shape[0] > 0 and st[1] == 1 and st[0] >= C and st[0] % 4 == 0 and t.data_ptr() % 16 == 0):
        t = t.float().contiguous()
        return t, C
    return t, st[0]


def _gather_gemm(src, ld, kernel, nbr, n_rows, transposed, n_calls, precision):
    """``v3d_sparse_conv_f32`` (``use_gn = 0``, ``relu_out = 0``, no residual) over the offsets of ``nbr`` [n_seg, >= n_rows] ->
    [n_rows, Co] (``transposed``: every slab transposed -> [n_rows, Ci]).  ``n_calls`` > 1: one call per group of n_seg / n_calls
    consecutive offsets, the partial results added pairwise (shorter accumulation chains, see ``SparseConv``)."""
    from .scenemodeling import PackedGemm
    lib = _lib.load()
    dev = src.device
    n_seg, ci, co = kernel.shape
    per = n_seg // n_calls
    N, K = (ci, co) if transposed else (co, ci)
    outs = []
    with torch.cuda.device(dev):
        for j in range(n_calls):
            # slab k addressed as w[k][n][kk]: [Ci, Co] read as (n = co, kk = ci), transposed as (n = ci, kk = co)
            pack = PackedGemm(kernel.detach()[j * per:(j + 1) * per], ci * co, co if transposed else 1, 1 if transposed else co, per,
                              N, K, device=dev)                                              # no GroupNorm affine
            y = torch.empty((n_rows, N), dtype=torch.float32, device=dev)
            rc = lib.v3d_sparse_conv_f32(pack.handle, n_rows, src.data_ptr(), ld, nbr[j * per:].data_ptr(), nbr.shape[1], 0, 0.0, None,
                                         0, 0, _lib.ptr(y), N, _lib.precision_code(precision), _lib.stream_ptr(dev))
            _lib.check(rc, 'v3d_sparse_conv_f32')
            outs.append(y)
    while len(outs) > 1:
        outs = [outs[i] + outs[i + 1] if i + 1 < len(outs) else outs[i] for i in range(0, len(outs), 2)]
    return outs[0]


class SparseConv(torch.autograd.Function):
    """A sparse convolution without norm, residual or ReLU -- ``v3d_sparse_conv_f32`` with ``use_gn = 0``, ``relu_out = 0`` -- with
    both gradients.  ``nbr`` [27, n_out] is the forward's table A.neighbors(B.coords, step), ``nbr_inv`` [27, n_in]
    its inverse B.neighbors(A.coords, -step).  To ``x``: the same call on ``grad_out`` over ``nbr_inv`` with every slab transposed
    (the same offset index).  To ``kernel``: ``v3d_sparse_conv_weight_grad_f32`` (exact fp32 in both precisions, no atomics,
    bitwise reproducible).  The node saves ``x``, ``kernel`` and the two tables: nothing of size 27 * M * C.

    Precision ``'fp32'`` runs the FORWARD as nine calls of three offsets each and adds the nine partial results pairwise.  The
    exact-fp32 kernel adds the 27 * Ci products of an output into one accumulator in sequence; GroupNorm's backward reads the
    forward values, and with one 27-offset call the gradients of the whole U-Net were about twice as far from float64 as those of a
    stock float32 graph (up to 4.8 times on single gradients); with chains of 3 * Ci they are as close.  The
    default ``'split_bf16'``, whose products carry 2^-16 each, is one call: the bits of the inference forward."""
    FP32_FORWARD_CALLS = 9

    @staticmethod
    def forward(ctx, x, kernel, nbr, nbr_inv, precision):
        n_seg, ci, co = kernel.shape
        n_out = nbr.shape[1]
        assert x.dim() == 2 and x.shape[1] == ci and nbr.shape[0] == n_seg and nbr_inv.shape == (n_seg, x.shape[0])
        assert nbr.dtype == torch.int32 and nbr_inv.dtype == torch.int32
        xc = x.detach().float().contiguous()
        n_calls = SparseConv.FP32_FORWARD_CALLS if precision == 'fp32' and n_seg % SparseConv.FP32_FORWARD_CALLS == 0 else 1
        y = _gather_gemm(xc, ci, kernel, nbr, n_out, False, n_calls, precision)
        ctx.save_for_backward(x, kernel, nbr, nbr_inv)
        ctx.precision = precision
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, kernel, nbr, nbr_inv = ctx.saved_tensors
        lib = _lib.load()
        dev = x.device
        n_seg, ci, co = kernel.shape
        n_in, n_out = x.shape[0], nbr.shape[1]
        assert grad_out.shape == (n_out, co)
        g, ld_g = _row_matrix(grad_out, co)
        grad_x = grad_w = None
        if ctx.needs_input_grad[0]:
            # dx[a] = sum_k g[nbr_inv[k, a]] @ kernel[k]^T
            grad_x = _gather_gemm(g, ld_g, kernel, nbr_inv, n_in, True, 1, ctx.precision).to(x.dtype)
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[1]:
                xc = x.detach().float().contiguous()
                grad_w = torch.empty((n_seg, ci, co), dtype=torch.float32, device=dev)      # every element is written
                nbytes = lib.v3d_sparse_conv_weight_grad_workspace_bytes(n_out, n_seg, ci, co)
                ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
                rc = lib.v3d_sparse_conv_weight_grad_f32(_lib.ptr(xc), ci, _lib.ptr(nbr), nbr.shape[1], n_seg, g.data_ptr(), ld_g, n_out,
                                                         ci, co, _lib.ptr(grad_w), _lib.ptr(ws), nbytes, _lib.stream_ptr(dev))
                _lib.check(rc, 'v3d_sparse_conv_weight_grad_f32')
                grad_w = grad_w.to(kernel.dtype)
        return grad_x, grad_w, None, None, None


def sparse_conv(x, kernel, nbr, nbr_inv, precision='split_bf16'):
    """y[p] = sum_k [nbr[k, p] >= 0] x[nbr[k, p]] @ kernel[k] as a differentiable function of ``x`` [n_in, Ci] and ``kernel``
    [27, Ci, Co] (Ci, Co multiples of 16 up to 128); ``nbr`` [27, n_out] / ``nbr_inv`` [27, n_in] int32 as in ``SparseConv``."""
    mvsnet._require_cuda(x, 'training.sparse_conv')
    mvsnet._require_cuda(kernel, 'training.sparse_conv')
    _lib.precision_code(precision)
    return SparseConv.apply(x, kernel, nbr.contiguous(), nbr_inv.contiguous(), precision)


def _group_norm(norm, y):
    gn = norm.gn                                                # MinkowskiGroupNorm: gn(input.F), every voxel row on its own
    return F.group_norm(y, gn.num_groups, gn.weight, gn.bias, gn.eps)


def sparse_unet(unet, feats, xs):
    """``SparseUNet.forward`` (scenemodeling.py:147-237) as a differentiable function -> ``level_feats``: one [N_l, C_l] tensor
    per level in the order of ``xs`` (coarse to fine), differentiable in ``feats`` [N, C_0] and in every parameter of ``unet``
    (kernels, GroupNorm weights and biases, ``feat_adj``; no second parameter set, ``state_dict`` keys untouched).  ``xs``: the
    result of the inference call ``unet(feats, pts, idx, batch, res)`` on the same input; its ``x['sparse']`` supply every
    coordinate map and hash table.  Convolutions are ``sparse_conv`` in ``unet.precision``; GroupNorm, ReLU, the residual add and
    the 1x1 ``feat_adj`` are stock torch ops.  The result plugs into ``pointflow_offset(..., level_feats=...)``."""
    mvsnet._require_cuda(feats, 'training.sparse_unet')
    prec = unet.precision
    n_lv = len(unet.dims)
    assert len(xs) == n_lv
    levels = [x['sparse'] for x in xs][::-1]                    # fine to coarse, as SparseUNet.forward builds them
    assert feats.shape[0] == levels[0].n
    # each same-level table once per level; its inverse is the table with the 27 rows reversed (o_{26 - k} = -o_k)
    same = [lv.neighbors(lv.coords, lv.stride) for lv in levels]
    same_inv = [t.flip(0).contiguous() for t in same]
    # down table of level i (rows of level i - 1) and up table back (rows of level i): each other's inverse
    down = [None] + [levels[i - 1].neighbors(levels[i].coords, levels[i - 1].stride) for i in range(1, n_lv)]
    up = [None] + [levels[i].neighbors(levels[i - 1].coords, -levels[i - 1].stride) for i in range(1, n_lv)]

    def conv_gn_relu(seq, x, nbr, inv):
        return F.relu(_group_norm(seq[1], sparse_conv(x, seq[0].kernel, nbr, inv, prec)))

    def residual(blk, x, i):
        y = F.relu(_group_norm(blk.n1, sparse_conv(x, blk.conv1.kernel, same[i], same_inv[i], prec)))
        return F.relu(_group_norm(blk.n2, sparse_conv(y, blk.conv2.kernel, same[i], same_inv[i], prec)) + x)

    x = feats.float()
    skips = []
    for i in range(n_lv):
        if i > 0:
            x = conv_gn_relu(unet.down[i - 1], x, down[i], up[i])                       # stride-2 conv
        for blk in unet.res_down[i]:
            x = residual(blk, x, i)
        skips.append(x)
    out = [x]
    for j in range(n_lv - 1):
        i = n_lv - 1 - j                                                                 # from level i up to level i - 1
        u = conv_gn_relu(unet.up[j], x, up[i], down[i])                                  # transposed conv
        adj = unet.feat_adj[j]
        x = F.relu(_group_norm(adj[1], torch.cat((u, skips[i - 1]), dim=1) @ adj[0].kernel))      # 1x1 on ME.cat
        for blk in unet.res_up[j]:
            x = residual(blk, x, i - 1)
        out.append(x)
    return out


class PointNetFunction(torch.autograd.Function):
    """``PointNet.forward`` (scenemodeling.py:127-144) as ONE node with the gradients to ``x`` and to the twelve parameters
    (DESIGN.md 4.1f).  The forward is the inference forward call for call in ``pn.precision`` (the same bits), with
    ``v3d_segment_max_arg_f32`` in place of ``v3d_segment_max_f32``: it names the row that won each pooled value.  The node saves
    ``x``, ``h0 = fc_pos(x)``, the four layer outputs ``x1..x4`` [Np, H], the four pools and winner tables [Nv, H] and the segment
    list: nothing of width 2H (``cat(x, pool[idx])`` is never built, in neither direction).

    The backward runs in fp32 for both precisions.  Dense products are ``torch.mm``; what autograd would do with ``index_add``
    (atomics) and ``cat`` is three kernels: the sum of a voxel's gradient rows S = ``v3d_segment_sum_f32`` (the gradient of the
    pooled half of ``fc_k`` is a function of the voxel alone, so its products run over Nv rows), and
    ``v3d_pointnet_pool_backward_f32``, which masks the direct path by the ReLU and hands the pooled gradient to the ONE row that
    won (torch_scatter's rule; torch's own ``scatter_reduce('amax')`` splits it among ties)."""

    @staticmethod
    def forward(ctx, pn, trace, idx32, n_idx, x, *params):
        lib = _lib.load()
        dev = x.device
        pn._dev = dev
        g = pn._cache.get(pn._build, dev)
        xc = x.detach().contiguous().float()
        H = pn.hidden_dim
        xs, pools, args = [], [], []
        with torch.cuda.device(dev):
            stream = _lib.stream_ptr(dev)
            perm, offs = pn._segments(idx32, n_idx, dev)

            def pooled(t):
                pool = torch.empty((n_idx, H), dtype=torch.float32, device=dev)
                arg = torch.empty((n_idx, H), dtype=torch.int32, device=dev)
                _lib.check(lib.v3d_segment_max_arg_f32(t.data_ptr(), t.stride(0), perm.data_ptr(), offs.data_ptr(), n_idx, H,
                                                       pool.data_ptr(), H, arg.data_ptr(), H, stream), 'v3d_segment_max_arg_f32')
                xs.append(t)
                pools.append(pool)
                args.append(arg)
                return pool
            out, h0 = pn._layers(g, xc, idx32, n_idx, pooled)
        if trace is not None:
            trace.update(h0=h0, **{'x%d' % (i + 1): t for i, t in enumerate(xs)}, **{'pool%d' % (i + 1): t for i, t in enumerate(pools)},
                         **{'arg%d' % (i + 1): t for i, t in enumerate(args)})
        ctx.save_for_backward(x, h0, *xs, *pools, *args, idx32, perm, offs, *params)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        x, h0, xs, pools, args = saved[0], saved[1], saved[2:6], saved[6:10], saved[10:14]
        idx32, perm, offs = saved[14:17]
        W = saved[17::2]                                        # the six weights, in the order of PointNet.LAYERS
        need_x, need = ctx.needs_input_grad[4], ctx.needs_input_grad[5:]
        wants = [need[2 * i] or need[2 * i + 1] for i in range(6)]
        # the chain runs down to the lowest layer anybody asks about (x lies below fc_pos)
        lowest = -1 if need_x else min((i for i in range(6) if wants[i]), default=6)
        grads = [None] * 12

        def result(grad_x=None):
            return (None, None, None, None, grad_x) + tuple(None if t is None else t.to(p.dtype) for t, p in zip(grads, saved[17:]))
        if lowest == 6:
            return result()
        lib = _lib.load()
        dev = x.device
        Np, H, n_idx = h0.shape[0], h0.shape[1], pools[0].shape[0]
        stream = _lib.stream_ptr(dev)

        def segment_sum(G):
            S = torch.empty((n_idx, H), dtype=torch.float32, device=dev)                # every element is written
            _lib.check(lib.v3d_segment_sum_f32(G.data_ptr(), H, perm.data_ptr(), offs.data_ptr(), n_idx, H, S.data_ptr(), H, stream),
                       'v3d_segment_sum_f32')
            return S

        def pool_backward(g_lin, x_k, g_pool, arg):
            G = torch.empty((Np, H), dtype=torch.float32, device=dev)                   # every element is written
            _lib.check(lib.v3d_pointnet_pool_backward_f32(_lib.ptr(g_lin), H, _lib.ptr(x_k), H, idx32.data_ptr(), g_pool.data_ptr(), H,
                                                          arg.data_ptr(), H, Np, H, G.data_ptr(), H, stream),
                       'v3d_pointnet_pool_backward_f32')
            return G

        def linear_grads(i, G, inputs, bias_rows):
            # dW = [G_0^T a_0 | G_1^T a_1 ...] over (gradient rows, ReLU'd input) pairs, db = the column sums of `bias_rows`
            if need[2 * i]:
                parts = [Gj.t() @ a for Gj, a in inputs]
                grads[2 * i] = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
            if need[2 * i + 1]:
                grads[2 * i + 1] = bias_rows.sum(dim=0)

        with torch.cuda.device(dev):
            # a slice of a wider row or a stride-0 expanded tensor (a .sum() upstream) becomes one contiguous fp32 copy, [Nv, out_dim]:
            # only torch.mm reads it
            g = grad_out.float().contiguous()
            linear_grads(5, g, [(g, F.relu(pools[3]))], g)
            if lowest >= 5:
                return result()
            G = pool_backward(None, None, (g @ W[5]).mul_(pools[3] > 0), args[3])       # the gradient of x4
            for k in (4, 3, 2):                                                          # fc_k reads x_{k-1} and pool_{k-1}[idx]
                x_in, pool_in, arg_in = xs[k - 2], pools[k - 2], args[k - 2]
                S = segment_sum(G)
                linear_grads(k, G, [(G, F.relu(x_in)), (S, F.relu(pool_in))], S)
                if lowest >= k:
                    return result()
                G = pool_backward(G @ W[k][:, :H], x_in, (S @ W[k][:, H:]).mul_(pool_in > 0), arg_in)
            linear_grads(1, G, [(G, F.relu(h0))], G)                                     # G: the gradient of x1 = fc1(relu(h0))
            if lowest >= 1:
                return result()
            G = (G @ W[1]).mul_(h0 > 0)
            linear_grads(0, G, [(G, x.detach().float())], G)
            return result((G @ W[0]).to(x.dtype) if need_x else None)


def pointnet(pn, x, idx, n_idx, trace=None):
    """``pn(x, idx, n_idx)`` of an existing ``scenemodeling.PointNet`` (the same bits, in ``pn.precision``) -> [n_idx, out_dim],
    differentiable in ``x`` [Np, in_dim] and in the twelve parameters of ``pn`` (no second parameter set; ``state_dict`` keys
    untouched).  ``idx`` [Np]: the voxel of each point, data.  ``trace``: a dict that receives ``h0``, ``x1..x4`` (the arguments of
    the ReLUs), ``pool1..pool4`` and ``arg1..arg4`` (the winner rows) of the forward.  ``hidden_dim`` must be a multiple of 4 up to
    128."""
    mvsnet._require_cuda(x, 'training.pointnet')
    assert x.dim() == 2 and idx.shape == (x.shape[0],)
    params = [p for name in pn.LAYERS for p in (getattr(pn, name).weight, getattr(pn, name).bias)]
    return PointNetFunction.apply(pn, trace, idx.to(torch.int32).contiguous(), int(n_idx), x, *params)


def scene_features(net, depth_pred, depth_batch, img_feats, rotmats, tvecs, K, ref_src_edges, csr=None, trace=None):
    """The differentiable twin of ``PL3DVNet.model_scene`` (lightningmodel.py:176-185) -> ``(xs, level_feats)``: ``xs`` the levels of
    the inference U-Net (coordinate maps, tables: data), ``level_feats`` one [N_l, C_l] tensor per level with the gradient to
    ``depth_pred`` (through the points), to ``img_feats`` (through the point features) and to every parameter of ``net.pointnet``
    and ``net.sparse_conv``; both plug into ``pointflow_offset(net.decoder, xs, ..., level_feats=level_feats)``.

    The voxel grid is data (``utils.voxelize`` on detached points) with one exception the reference has too: its anchors are
    ``idx3d * edge + bbox_min + edge / 2`` with ``bbox_min = pts.min(dim=0)[0]`` OUTSIDE ``no_grad`` (mv3d/utils.py:39,58), so the
    point that holds an axis' minimum receives minus the sum of that column of the PointNet input's gradient.  Taking the exact
    zero ``bmin - bmin.detach()`` off the input's position columns keeps their bits and adds that path.  ``trace``: a dict that receives ``pts``, ``pts_feat``, ``edges``,
    ``anchor_pts``, ``x`` (the PointNet input) and ``F`` (the U-Net input)."""
    pts, pts_feat, pts_batch = feature_rich_pointcloud(depth_pred, depth_batch, img_feats, rotmats, tvecs, K, ref_src_edges,
                                                       net.hparams.img_size, csr=csr)
    with torch.no_grad():
        anchor_pts, anchor_idx3d, anchor_batch, edges = utils.voxelize(pts, pts_batch, net.edge_len)
    # p - (anchor + (bmin - bmin.detach())) with the exact zero taken off the difference instead: the same bits, the same
    # gradient, and bmin's is a column sum over the points instead of an index_add (atomics) into the anchors
    bmin = pts.min(dim=0)[0]
    rel = pts.index_select(0, edges[1]) - anchor_pts.index_select(0, edges[0]) - (bmin - bmin.detach())
    x = torch.cat((rel, pts_feat.index_select(0, edges[1])), dim=1)
    feats = pointnet(net.pointnet, x, edges[0], anchor_pts.shape[0])
    unet = net.sparse_conv
    with torch.no_grad():
        xs = unet(feats.detach(), anchor_pts, anchor_idx3d, anchor_batch, net.edge_len, idx_min_zero=True)
    if trace is not None:
        trace.update(pts=pts, pts_feat=pts_feat, edges=edges, anchor_pts=anchor_pts, x=x, F=feats)
    return xs, sparse_unet(unet, feats, xs)


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
