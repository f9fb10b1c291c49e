"""GPU: ``PL3DVNet.forward(batch, offsets, n_iters)`` (mv3d/lightningmodel.py:48-122), ``validation_step`` and ``log_metrics``
(:244-282) on one tiny scene: the ten supervised depth maps equal the same chain written out from the public stage methods bit for
bit, and every metric and loss in the returned dictionary equals the float64 checker of tests/supervision_oracle.py applied to those
depth maps within F64_RTOL (h w 2^-53 relative for a float64 sum in any order; 1e-10).

Scene: 4 reference views with a (2, 2) window = 8 images of 64 x 80; synthetic features at 16 x 20 and 32 x 40; stage 1 on an
8 x 16 grid with 8 planes (the regulariser halves the volume three times and, like the reference's, takes only multiples of 8:
the smallest grid that is not square and that both resizes to 16 x 20 really enlarge); ground truth from the analytic box room
at 64 x 80 with a block of holes and a few values below 0.5 m; offsets [0.05, 0.05, 0.025], 2 iterations = 6 sweeps, 10 supervised points."""
import numpy as np
import pytest
import torch

import supervision_oracle as oracle
from conftest import v3d

pytestmark = pytest.mark.gpu

IMG, QUARTER, HALF = (64, 80), (16, 20), (32, 40)
DEPTH_TEST = {'depth_start': .5, 'depth_interval': .6, 'n_intervals': 8, 'size': (8, 16)}
EDGE_LEN = 0.16
N_REF, WINDOW = 4, (2, 2)
OFFSETS, N_ITERS = [0.05, 0.05, 0.025], 2
N_SWEEPS = N_ITERS * len(OFFSETS)
KEYS = ['ref', 'initial', 'loss_2d', 'quarter', 'half', 'final', 'loss']
LOSS_SUM_RTOL = 16 * 2.0 ** -53          # ten float64 products and sums, each rounded once
_cache = {}


def _net(cuda, precision):
    syn, lm = v3d('synthetic'), v3d('lightningmodel')
    net = lm.PL3DVNet(None, dict(DEPTH_TEST), EDGE_LEN, feat_dim=32, img_size=IMG, precision=precision).eval()
    net.mvsnet.cnn_3d.load_state_dict(syn.costregnet_weights(seed=0, sharpen=200.0), strict=False)
    net.pointnet.load_state_dict(syn.pointnet_weights(seed=1))
    net.sparse_conv.load_state_dict(syn.sparse_unet_weights(seed=2))
    net.decoder.load_state_dict(syn.decoder_weights(seed=3, sharpen=50.0), strict=False)
    for m, seed, cin in zip((net.refine_quarter, net.refine_half, net.refine_full), (5, 6, 7), (33, 33, 4)):
        m.load_state_dict(syn.propagation_weights(cin, 32, seed), strict=False)
    return net.to(cuda)


def _batch(cuda):
    syn, Batch = v3d('synthetic'), v3d('batch').Batch
    edges, n_img = syn.make_edges(N_REF, *WINDOW)
    assert n_img == 8
    rot, tv, K = syn.make_cameras(n_img, IMG, seed=51)
    k = WINDOW[0]
    gt = syn.ray_box_depth(rot[k:k + N_REF], tv[k:k + N_REF], K[k:k + N_REF], IMG, IMG).float().contiguous()
    gt[:, 10:30, 20:50] = 0.0                               # a block of holes
    gt[0, 40, 3:9] = 0.3                                    # below 0.5 m: in the loss, not in the metrics
    gt[2, 5, 60:64] = 0.45
    b = Batch(syn.make_images(n_img, IMG, seed=53), rot, tv, K, gt, edges)
    b.features_quarter = syn.make_features(n_img, 32, *QUARTER, seed=51)
    b.features_half = syn.make_features(n_img, 32, *HALF, seed=52)
    b.images_batch = torch.zeros(n_img, dtype=torch.long)
    return b.to(cuda)


def _chain(net, b):
    """forward's ten depth maps from the public stage methods"""
    depths = []
    depth, depth_batch, feats_half, feats_quarter, _, ref_idx = net.make_initial_depth_predictions(b, net.hparams.depth_test)
    depth = depth.contiguous().float()
    depths.append(depth.clone())
    for _ in range(N_ITERS):
        xs = net.model_scene(depth, depth_batch, feats_quarter, b.rotmats, b.tvecs, b.K, b.ref_src_edges)
        for offset in OFFSETS:
            net.run_pointflow(xs, depth, depth_batch, feats_quarter, b.rotmats, b.tvecs, b.K, b.ref_src_edges, offset, 3,
                              add_to_depth=True)
            depths.append(depth.clone())
    for prop, guide in ((net.refine_quarter, feats_quarter), (net.refine_half, feats_half), (net.refine_full, b.images)):
        depth = prop.forward_resized(guide[ref_idx], depth)
        depths.append(depth.clone())
    return depths


def setup(cuda, precision):
    """net, batch, forward's result at epoch 0 with its depths, the chain's depths, the checker's records: once per precision"""
    if precision not in _cache:
        net, b = _net(cuda, precision), _batch(cuda)
        keys_before = set(net.state_dict())
        with torch.no_grad():
            out = net(b, OFFSETS, N_ITERS, return_depths=True)
            chain = _chain(net, b)
        gt = b.depth_images.cpu().numpy()
        want = [oracle.check(d.cpu().numpy(), gt, DEPTH_TEST['depth_interval']) for d in out['depths']]
        _cache[precision] = dict(net=net, batch=b, out=out, chain=chain, want=want, keys_before=keys_before)
    return _cache[precision]


def points(out):
    """the ten metric dictionaries of a result in the order of its depths, each with its loss"""
    return [dict(out['initial'], loss_2d=out['loss_2d'])] + list(out['ref']) + [out['quarter'], out['half'], out['final']]


def losses(out):
    return [float(p['loss_2d']) for p in points(out)]


@pytest.mark.parametrize('precision', ['split_bf16', 'fp32'])
def test_depths_equal_the_chain_of_the_stage_methods(cuda, precision):
    s = setup(cuda, precision)
    depths = s['out']['depths']
    assert len(depths) == 1 + N_SWEEPS + 3 == 10 and len(s['chain']) == 10
    shapes = [(N_REF,) + DEPTH_TEST['size']] * (1 + N_SWEEPS) + [(N_REF,) + QUARTER, (N_REF,) + HALF, (N_REF,) + IMG]
    assert [tuple(d.shape) for d in depths] == shapes
    for k, (a, b) in enumerate(zip(depths, s['chain'])):
        assert a.dtype == torch.float32 and torch.equal(a, b), 'depth %d' % k
    assert all(bool(torch.isfinite(d).all()) for d in depths)
    assert all(not torch.equal(depths[k], depths[k + 1]) for k in range(N_SWEEPS))          # every sweep moved the depths
    # the ground truth the scene was built with: holes, pixels below 0.5 m, and most pixels in the metrics' mask
    gt = s['batch'].depth_images
    assert bool((gt == 0).any()) and bool(((gt > 0) & (gt < 0.5)).any()) and float(((gt >= 0.5) & (gt < 65)).float().mean()) > 0.5


@pytest.mark.parametrize('precision', ['split_bf16', 'fp32'])
def test_metrics_and_losses_equal_the_checker_on_those_depths(cuda, precision):
    s = setup(cuda, precision)
    out = s['out']
    assert list(out) == KEYS + ['depths']
    assert list(out['initial']) == list(oracle.METRIC_KEYS) and len(out['ref']) == N_SWEEPS
    for k, (p, want) in enumerate(zip(points(out), s['want'])):
        if k > 0:
            assert list(p) == list(oracle.METRIC_KEYS) + ['loss_2d'], k
        for key, v in p.items():
            assert v.is_cuda and v.dim() == 0 and v.dtype == torch.float64, (k, key)
            np.testing.assert_allclose(float(v), want['mean'][oracle.COLUMNS.index(key)], rtol=oracle.F64_RTOL, atol=0,
                                       err_msg='point %d %s' % (k, key))
        assert want['counts'][:, 5].sum() > want['counts'][:, 1].sum() > 0                 # the two masks differ
    assert out['loss'].is_cuda and out['loss'].dim() == 0 and out['loss'].dtype == torch.float64
    # epoch 0: the sweeps weigh nothing
    want_losses = [w['mean'][oracle.LOSS] for w in s['want']]
    np.testing.assert_allclose(float(out['loss']), oracle.total_loss(want_losses, N_SWEEPS, 0.0), rtol=oracle.F64_RTOL, atol=0)
    np.testing.assert_allclose(float(out['loss']), oracle.total_loss(losses(out), N_SWEEPS, 0.0), rtol=LOSS_SUM_RTOL, atol=0)


@pytest.mark.parametrize('precision', ['split_bf16', 'fp32'])
def test_loss_weights_twice_the_same_bits_validation_step_and_log_metrics(cuda, precision):
    s = setup(cuda, precision)
    net, b, out = s['net'], s['batch'], s['out']
    want_losses = [w['mean'][oracle.LOSS] for w in s['want']]

    def same(a, c):
        return all(torch.equal(x[k], y[k]) for x, y in zip(points(a), points(c)) for k in x) and torch.equal(a['loss'], c['loss'])

    with torch.no_grad():
        again = net(b, OFFSETS, N_ITERS)
        assert list(again) == KEYS and same(out, again)                                    # twice: identical bits
        for epoch, lam in ((5, 0.5), (12, 1.0)):
            net.current_epoch = epoch
            o = net(b, OFFSETS, N_ITERS)
            assert losses(o) == losses(out)
            np.testing.assert_allclose(float(o['loss']), oracle.total_loss(want_losses, N_SWEEPS, lam), rtol=oracle.F64_RTOL, atol=0)
            np.testing.assert_allclose(float(o['loss']), oracle.total_loss(losses(o), N_SWEEPS, lam), rtol=LOSS_SUM_RTOL, atol=0)
        net.current_epoch = 0
        net.hparams.finetune = True
        try:
            o = net(b, OFFSETS, N_ITERS)
        finally:
            net.hparams.finetune = False
        np.testing.assert_allclose(float(o['loss']), oracle.total_loss(want_losses, N_SWEEPS, 1.0), rtol=oracle.F64_RTOL, atol=0)
        assert float(o['loss']) > float(out['loss'])
        # validation_step: forward with the reference's schedule (the test's), the record kept, the loss returned
        net.logged = None
        loss = net.validation_step(b, 0)
    assert torch.equal(loss, out['loss'])
    names = ['val/loss_2d', 'val/loss'] + ['val_2d/' + k for k in oracle.METRIC_KEYS]
    for part in ('final', 'half', 'quarter'):
        names += ['val_%s/%s' % (part, k) for k in oracle.METRIC_KEYS + ('loss_2d',)]
    for i in range(N_SWEEPS):
        names += ['val_ref%d/%s' % (i, k) for k in oracle.METRIC_KEYS + ('loss_2d',)]
    logged = net.logged
    assert list(logged) == names and all(isinstance(v, float) for v in logged.values())
    assert logged['val/loss'] == float(out['loss']) and logged['val/loss_2d'] == float(out['loss_2d'])
    assert logged['val_final/abs_rel'] == float(out['final']['abs_rel']) and logged['val_ref3/loss_2d'] == float(out['ref'][3]['loss_2d'])
    rec = net.log_metrics(out, prefix='train')
    assert rec is net.logged and list(rec) == [k.replace('val', 'train', 1) for k in names]
    assert list(rec.values()) == list(logged.values())
    assert set(net.state_dict()) == s['keys_before']
    assert s['keys_before'] == {name + '.' + k for name, m in net.named_children() if name != 'mae_loss' for k in m.state_dict()}


def test_error_cases(cuda):
    s = setup(cuda, 'split_bf16')
    net, b = s['net'], s['batch']
    Batch = v3d('batch').Batch

    def variant(**changes):
        v = Batch(b.images, b.rotmats, b.tvecs, b.K, b.depth_images, b.ref_src_edges)
        v.features_quarter, v.features_half, v.images_batch = b.features_quarter, b.features_half, b.images_batch
        for k, val in changes.items():
            setattr(v, k, val)
        return v

    with torch.no_grad():
        with pytest.raises(ValueError, match='depth_images'):
            net(variant(depth_images=None), OFFSETS, N_ITERS)
        with pytest.raises(ValueError, match='depth_images'):
            net(variant(depth_images=b.depth_images[:, :32, :40].contiguous()), OFFSETS, N_ITERS)
        with pytest.raises(ValueError, match='features_half'):
            net(variant(features_half=None), OFFSETS, N_ITERS)
        net.train()
        try:
            with pytest.raises(RuntimeError, match='BatchNorm'):
                net(b, OFFSETS, N_ITERS)
        finally:
            net.eval()
