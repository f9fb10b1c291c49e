"""GPU: the trainable hypothesis decoder of 3dvnet_amd/training.py -- ``decoder_features``, ``hypothesis_decoder``,
``pointflow_offset`` -- on the smallest scene that yields three non-empty U-Net levels: 3 reference views with a (1, 1) window = 5
images of 64 x 80, features and depth at 16 x 20, n = 3 (7 hypotheses), offset 0.05.

  * layout: ``decoder_features`` is ``HypothesisDecoder.features`` bit for bit;
  * gradient flow: ``pointflow_offset`` + ``masked_mae`` gives finite, non-zero gradients on every level's features, on the image
    features and on every decoder parameter, and none on the depth through the hypotheses.  One parameter is exempt from "non-zero":
    the bias of the head.  A softmax does not change when a constant is added to its logits, so that gradient is zero in exact
    arithmetic; what arrives is rounding residue, required to be finite here and bounded in the accuracy test;
  * gradient accuracy: every gradient against the same graph built from stock index ops (grid_sample + index_add_ mean; corner
    table -> gather, weight, sum; pad + matmul convolutions) in float64 on the device.  Yardstick: that stock graph in float32.
    The HIP route's max-norm relative error may be at most 4 times the stock float32 graph's own (different summation orders, not
    a different algorithm).  Both errors are printed.  The head bias, exactly zero in float64, is held to an
    absolute rounding bound instead (derived in the test);
  * BatchNorm modes, untouched state_dict keys, and PL3DVNet.forward still raising in training mode.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import v3d

pytestmark = pytest.mark.gpu

IMG, QUARTER = (64, 80), (16, 20)
EDGE_LEN = 0.16
N_REF, WINDOW = 3, (1, 1)
OFFSET, N = 0.05, 3
INTERVAL = 0.6
HEAD_BIAS = 'net.3.bias'
_cache = {}


def scene(cuda):
    if 'scene' in _cache:
        return _cache['scene']
    syn, lm = v3d('synthetic'), v3d('lightningmodel')
    net = lm.PL3DVNet(None, {'depth_start': .5, 'depth_interval': INTERVAL, 'n_intervals': 8, 'size': (8, 16)}, EDGE_LEN, feat_dim=32,
                      img_size=IMG).eval()
    net.pointnet.load_state_dict(syn.pointnet_weights(seed=1))
    net.sparse_conv.load_state_dict(syn.sparse_unet_weights(seed=2))
    net.decoder.load_state_dict(syn.decoder_weights(seed=3, sharpen=5.0), strict=False)
    net = net.to(cuda)
    edges, n_img = syn.make_edges(N_REF, *WINDOW)
    assert n_img == 5
    rot, tv, K = syn.make_cameras(n_img, IMG, seed=51)
    k = WINDOW[0]
    truth = syn.ray_box_depth(rot[k:k + N_REF], tv[k:k + N_REF], K[k:k + N_REF], IMG, QUARTER).float()
    g = torch.Generator().manual_seed(9)
    depth = (truth + 0.04 * torch.randn(truth.shape, generator=g)).contiguous()
    gt = truth.clone()
    gt[:, 3:6, 4:9] = 0.0                                         # holes: outside the loss
    feat = syn.make_features(n_img, 32, *QUARTER, seed=51)
    s = dict(net=net, depth=depth.to(cuda), gt=gt.to(cuda), feat=feat.to(cuda), rot=rot.to(cuda), tv=tv.to(cuda), K=K.to(cuda),
             edges=edges.to(cuda), depth_batch=torch.zeros(N_REF, dtype=torch.long, device=cuda))
    with torch.no_grad():
        s['xs'] = net.model_scene(s['depth'], s['depth_batch'], s['feat'], s['rot'], s['tv'], s['K'], s['edges'])
    assert len(s['xs']) == 3 and [int(x['stride']) for x in s['xs']] == [4, 2, 1]
    assert all(x['feats'].shape[0] > 0 for x in s['xs']) and [x['feats'].shape[1] for x in s['xs']] == [128, 128, 64]
    print('levels: %s rows' % [x['feats'].shape[0] for x in s['xs']])
    _cache['scene'] = s
    return s


def _geometry(s):
    return s['rot'], s['tv'], s['K'], s['edges'], OFFSET, N, IMG


def hip_gradients(s, bn_training=False):
    """loss = masked_mae(depth + pointflow_offset(...), gt) -> (loss, offset, gradients by name)"""
    tr = v3d('training')
    dec = s['net'].decoder
    level = [x['feats'].detach().clone().requires_grad_(True) for x in s['xs']]
    feat = s['feat'].clone().requires_grad_(True)
    depth = s['depth'].clone().requires_grad_(True)
    off = tr.pointflow_offset(dec, s['xs'], depth, s['depth_batch'], feat, *_geometry(s), level_feats=level, bn_training=bn_training)
    loss = tr.masked_mae(depth + off, s['gt'], INTERVAL)
    params = dict(dec.named_parameters())
    names = ['level%d' % i for i in range(3)] + ['img_feats'] + list(params)
    grads = torch.autograd.grad(loss, level + [feat] + list(params.values()), retain_graph=True)
    through = torch.autograd.grad(off.sum(), depth, allow_unused=True)[0]
    return loss, off, dict(zip(names, grads)), through


def _corner_table(x, pts, pts_batch, cuda):
    """(rows int64 [nq, 8], w float32 [nq, 8]) out of the forward's workspace"""
    libm = v3d('_lib')
    lib = libm.load()
    n_pts, n_hyp = pts.shape[:2]
    nq = n_pts * n_hyp
    C = x['feats'].shape[1]
    ws = torch.empty(lib.v3d_sparse_interp_workspace_bytes(n_pts, n_hyp), dtype=torch.uint8, device=cuda)
    out = torch.empty((nq, C), dtype=torch.float32, device=cuda)
    f = x['feats'].contiguous()
    libm.check(lib.v3d_sparse_interp_f32(x['sparse'].table.data_ptr(), x['sparse'].n, f.data_ptr(), C, int(x['stride']),
                                         pts.data_ptr(), pts_batch.data_ptr(), n_pts, n_hyp, v3d('training')._level_min_pts(x).contiguous().data_ptr(),
                                         float(x['res']), out.data_ptr(), C, 0, ws.data_ptr(), ws.numel(), libm.stream_ptr(cuda)),
               'v3d_sparse_interp_f32')
    half = (nq * 8 * 4 + 255) // 256 * 256
    rows = ws[:nq * 32].view(torch.int32).view(nq, 8).long()
    w = ws[half:half + nq * 32].view(torch.float32).view(nq, 8).clone()
    return rows, w


def stock_gradients(s, dtype, cuda):
    """The same loss from stock torch ops in ``dtype``.  The hypothesis points, the corner rows and the fp32 corner weights are
    data (the reference builds them under no_grad) and come from the forward kernels."""
    tr, mvs = v3d('training'), v3d('mvsnet')
    dec = s['net'].decoder
    rot, tv, K, edges = s['rot'], s['tv'], s['K'], s['edges']
    n_ref, h, w = s['depth'].shape
    n_hyp, C = 2 * N + 1, s['feat'].shape[1]
    S = h * w * n_hyp
    with torch.no_grad():
        pts_hyp, _, pts_batch = tr.pointflow_hypotheses(s['depth'], s['depth_batch'], s['feat'], *_geometry(s))
        pts_hyp = pts_hyp.contiguous()
        pts_batch = pts_batch.contiguous()
        tables = [_corner_table(x, pts_hyp, pts_batch, cuda) for x in s['xs']]
        _, _, edge_ofs, edge_src = mvs.edges_to_csr(edges)
        counts = (edge_ofs[1:] - edge_ofs[:-1]).long()
        gather = torch.repeat_interleave(torch.arange(n_ref, device=cuda), counts)
        src = edge_src.long()
        P = torch.bmm(K[src].to(dtype), torch.cat((rot[src], tv[src].unsqueeze(2)), dim=2).to(dtype))
        X = pts_hyp.to(dtype).view(n_ref, S, 3)[gather].transpose(1, 2)
        q = torch.bmm(P[:, :, :3], X) + P[:, :, 3:]
        uv = q[:, :2] / (q[:, 2:3].abs() + 1e-8)
        grid = torch.stack((uv[:, 0] / (IMG[1] - 1) * 2 - 1, uv[:, 1] / (IMG[0] - 1) * 2 - 1), dim=-1).unsqueeze(2)
    level = [x['feats'].detach().to(dtype).requires_grad_(True) for x in s['xs']]
    feat = s['feat'].detach().to(dtype).clone().requires_grad_(True)
    params = {k: v.detach().to(dtype).requires_grad_(True) for k, v in dec.named_parameters()}
    bufs = {k: v.detach().to(dtype) for k, v in dec.named_buffers()}
    x = F.grid_sample(feat[src], grid, mode='bilinear', align_corners=True).squeeze(3)                      # [E, C, S]
    cnt = counts.clamp(min=1).view(-1, 1, 1).to(dtype)
    avg = torch.zeros((n_ref, C, S), device=cuda, dtype=dtype).index_add_(0, gather, x) / cnt
    avg_sq = torch.zeros((n_ref, C, S), device=cuda, dtype=dtype).index_add_(0, gather, x ** 2) / cnt
    features = (avg_sq - avg ** 2).view(n_ref, C, h * w, n_hyp).permute(0, 2, 3, 1).reshape(n_ref * h * w, n_hyp, C)
    for f, (rows, wgt) in zip(level, tables):
        gathered = f[rows.clamp(min=0)] * (rows >= 0).to(dtype).unsqueeze(-1)                                # [nq, 8, C]
        interp = (gathered * wgt.to(dtype).unsqueeze(-1)).sum(dim=1).view(n_ref * h * w, n_hyp, -1)
        features = torch.cat((interp, features), dim=2)
    y = features.transpose(2, 1)
    for i in range(3):
        W = params['net.%d.0.weight' % i]
        yp = F.pad(y, (1, 1))
        y = sum(torch.einsum('oi,nil->nol', W[:, :, t], yp[:, :, t:t + n_hyp]) for t in range(3))
        rm, rv = bufs['net.%d.1.running_mean' % i], bufs['net.%d.1.running_var' % i]
        y = (y - rm[None, :, None]) / torch.sqrt(rv[None, :, None] + dec.net[i][1].eps)
        y = F.relu(y * params['net.%d.1.weight' % i][None, :, None] + params['net.%d.1.bias' % i][None, :, None])
    yp = F.pad(y, (1, 1))
    y = sum(torch.einsum('oi,nil->nol', params['net.3.weight'][:, :, t], yp[:, :, t:t + n_hyp]) for t in range(3))
    preds = F.softmax((y + params[HEAD_BIAS][None, :, None]).squeeze(1), dim=1)
    vals = torch.linspace(-N * OFFSET, N * OFFSET, n_hyp).to(preds)
    off = torch.sum(vals.unsqueeze(0) * preds, dim=1).view(n_ref, h, w)
    loss = tr.masked_mae(s['depth'].to(dtype) + off, s['gt'].to(dtype), INTERVAL)
    names = ['level%d' % i for i in range(3)] + ['img_feats'] + list(params)
    grads = torch.autograd.grad(loss, level + [feat] + list(params.values()) + [preds])
    # A = sum_pj p_j (|gp_j| + sum_i |gp_i| p_i): the magnitude the terms of the head bias's gradient are rounded against
    gp = grads[-1].abs()
    residue_scale = float((preds.detach() * (gp + (gp * preds.detach()).sum(dim=1, keepdim=True))).sum())
    return loss, off, dict(zip(names, grads[:-1])), residue_scale


def test_decoder_features_are_the_inference_features(cuda):
    s = scene(cuda)
    tr = v3d('training')
    with torch.no_grad():
        pts_hyp, pts_feat, pts_batch = tr.pointflow_hypotheses(s['depth'], s['depth_batch'], s['feat'], *_geometry(s))
        ref = s['net'].decoder.features(s['xs'], pts_hyp, pts_feat, pts_batch)
        got = tr.decoder_features(s['xs'], pts_hyp, pts_feat, pts_batch)
    assert got.shape == ref.shape == (N_REF * QUARTER[0] * QUARTER[1], 2 * N + 1, 352) and torch.equal(got, ref)
    assert all(bool((ref[:, :, a:b] != 0).any()) for a, b in ((0, 64), (64, 192), (192, 320), (320, 352)))
    with torch.no_grad():
        preds = tr.hypothesis_decoder(s['net'].decoder, got)
    with torch.no_grad():
        want = s['net'].decoder.decode(ref) if not s['net'].decoder.can_fuse(s['xs'], pts_hyp, pts_feat) else \
            s['net'].decoder.decode_fused(s['xs'], pts_hyp, pts_feat, pts_batch)
    # the inference kernels run the stack with split-bf16 matrix operands and folded BatchNorm: no bit equality.  1e-3 on a
    # probability is ten times what the inference tests allow between the fused kernel and its unfused chain.
    print('max |stock preds - inference preds| = %.3e' % float((preds - want).abs().max()))
    assert preds.shape == want.shape and float((preds - want).abs().max()) < 1e-3
    assert torch.allclose(preds.sum(dim=1), torch.ones_like(preds[:, 0]), atol=1e-5)


def test_gradients_reach_levels_features_and_every_parameter(cuda):
    s = scene(cuda)
    loss, off, grads, through_hyp = hip_gradients(s)
    assert off.shape == s['depth'].shape and bool(torch.isfinite(loss)) and float(loss.detach()) > 0
    assert through_hyp is None                                   # the hypotheses are data: no gradient to the depth through them
    for name, g in grads.items():
        print('%-16s max |grad| = %.3e' % (name, float(g.abs().max())))
        assert bool(torch.isfinite(g).all()), name
        if name != HEAD_BIAS:                                     # zero in exact arithmetic (shift invariance of the softmax):
            assert bool((g != 0).any()), name                     # bounded in test_gradients_match_the_stock_graph_in_float64
    expect = ['level0', 'level1', 'level2', 'img_feats'] + list(dict(s['net'].decoder.named_parameters()))
    assert list(grads) == expect and len(expect) == 4 + 11


def test_gradients_match_the_stock_graph_in_float64(cuda):
    """err(x) = max |g_x - g_64| / max |g_64| per gradient; err(HIP route) <= 4 err(stock float32 graph).

    The head bias is the one gradient this ratio cannot judge: it is sum_pj d_pj with d_pj = p_j (gp_j - sum_i gp_i p_i), and
    sum_j d_pj = (1 - sum_j p_j) sum_i gp_i p_i = 0 for every point, so its float64 value is 0 and both float32 routes return
    rounding residue only -- of torch's own softmax and convolution backward, which is not the code under test and whose summation
    order the convolution library chooses per run (seen: ratios of 2.0 and 6.0 on the same inputs).  It is printed like the others
    and held to an absolute bound instead: n = n_pts n_hyp terms, each rounded against p_j (|gp_j| + sum_i |gp_i| p_i) a few times
    (product, difference, an n_hyp-term sum whose p sum to 1 within n_hyp u), then summed in some order:
    |g_bias| <= (n + 2 n_hyp + 8) u A, A = sum_pj p_j (|gp_j| + sum_i |gp_i| p_i) from the float64 graph, u = 2^-24."""
    s = scene(cuda)
    loss, off, g_hip, _ = hip_gradients(s)
    loss64, off64, g64, residue_scale = stock_gradients(s, torch.float64, cuda)
    loss32, off32, g32, _ = stock_gradients(s, torch.float32, cuda)
    print('loss: HIP route %.9f, stock float32 %.9f, stock float64 %.12f' % (float(loss.detach()), float(loss32.detach()), float(loss64.detach())))
    print('max |offset - offset64|: HIP route %.3e, stock float32 %.3e'
          % (float((off - off64).detach().abs().max()), float((off32 - off64).detach().abs().max())))
    failed = []
    for name in g64:
        scale = float(g64['net.3.weight' if name == HEAD_BIAS else name].abs().max())
        assert scale > 0
        e_hip = float((g_hip[name].double() - g64[name]).abs().max()) / scale
        e_32 = float((g32[name].double() - g64[name]).abs().max()) / scale
        print('%-16s err HIP route = %.3e, err stock float32 = %.3e, ratio %.2f' % (name, e_hip, e_32, e_hip / e_32 if e_32 else np.inf))
        if name != HEAD_BIAS and not e_hip <= 4 * e_32:
            failed.append(name)
    assert not failed, failed
    n_terms = off.numel() * (2 * N + 1)
    bound = (n_terms + 2 * (2 * N + 1) + 8) * 2.0 ** -24 * residue_scale
    got = float(g_hip[HEAD_BIAS].abs().max())
    print('%-16s |grad| HIP route = %.3e, float64 = %.3e, bound (n + 2 n_hyp + 8) u A = %.3e (A = %.3e); head weight %.3e'
          % (HEAD_BIAS, got, float(g64[HEAD_BIAS].abs().max()), bound, residue_scale, float(g64['net.3.weight'].abs().max())))
    assert float(g64[HEAD_BIAS].abs().max()) <= 1e-12 * residue_scale and got <= bound < float(g64['net.3.weight'].abs().max())


def test_batchnorm_modes_state_dict_and_training_mode(cuda):
    s = scene(cuda)
    dec = s['net'].decoder
    keys = list(dec.state_dict())
    bufs = {k: v.clone() for k, v in dec.named_buffers()}
    hip_gradients(s, bn_training=False)
    assert all(torch.equal(v, bufs[k]) for k, v in dec.named_buffers())
    try:
        _, _, grads, _ = hip_gradients(s, bn_training=True)
        changed = [k for k, v in dec.named_buffers() if not torch.equal(v, bufs[k])]
        assert all(any(c == 'net.%d.1.%s' % (i, b) for c in changed) for i in range(3) for b in ('running_mean', 'running_var'))
        assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    finally:
        with torch.no_grad():
            for k, v in dec.named_buffers():
                v.copy_(bufs[k])
    assert list(dec.state_dict()) == keys
    net = s['net']
    net.train()
    try:
        with pytest.raises(RuntimeError):
            net(None, [OFFSET], 1)
    finally:
        net.eval()
