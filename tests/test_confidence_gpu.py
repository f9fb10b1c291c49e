"""GPU: photometric confidence maps (csrc/confidence.hip; include/v3d.h: v3d_probability_map_f32, v3d_confidence_logits_f32,
v3d_costreg_depth_prob, v3d_soft_argmin_f32) against the reference-written fixtures tests/golden/P_conf_*.npz, the fp32
restatement and the float64 checker of tests/confidence_oracle.py, and through every layer up to ``prepare_preds``.

Measured on an MI355X (device error / the reference's own fp32 error, bound 4): see DESIGN.md 6."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import confidence_oracle as oracle
from conftest import v3d
from test_confidence_oracle import bits, fixture_logits, load

pytestmark = pytest.mark.gpu
DS, DI = 0.5, 0.05


def dev_gather(cuda, cv, depth, ds=DS, di=DI):
    return v3d('utils').get_propability_map(torch.from_numpy(cv).to(cuda), torch.from_numpy(depth).to(cuda), ds, di).cpu().numpy()


def dev_logits(cuda, x, depth, ds=DS, di=DI):
    return v3d('utils').confidence_from_logits(torch.from_numpy(x).to(cuda), torch.from_numpy(depth).to(cuda), ds, di).cpu().numpy()


# ---- gather kernel ----------------------------------------------------------------------------------------------------------
def test_gather_equals_the_reference_fixtures_bit_for_bit(cuda):
    g = load('P_conf_gather')
    for i, (n, D, h, w) in enumerate(g['cases']):
        cv = oracle.volume((n, D, h, w), 100 + i)
        got = dev_gather(cuda, cv, g['depth_%d' % i], float(g['depth_start']), float(g['depth_interval']))
        assert np.array_equal(bits(got), bits(g['prob_%d' % i])), (n, D, h, w)


@pytest.mark.parametrize('D', [1, 7, 8, 9, 96])
def test_gather_equals_the_restatement_at_every_shape(cuda, D):
    """h x w = 8 x 8 (one partial workgroup), 24 x 24 (crosses workgroup boundaries, no multiple of 256), 56 x 56; n = 1, 3;
    depths 0, far outside on both sides, just outside either end, on every plane, and uniform around the grid."""
    for hw in (8, 24, 56):
        for n in (1, 3):
            cv = oracle.volume((n, D, hw, hw), 1000 + D + hw + n)
            depth = oracle.special_depths(DS, DI, D, n * hw * hw, 2000 + D + hw + n).reshape(n, hw, hw)
            assert np.array_equal(bits(dev_gather(cuda, cv, depth)), bits(oracle.gather_f32(cv, depth, DS, DI))), (D, hw, n)


@pytest.mark.parametrize('mode', ['v3d_probability_map_f32', 'v3d_confidence_logits_f32'])
def test_nan_and_infinite_depths_are_pinned_to_plane_0_and_stay_in_bounds(cuda, mode):
    """NaN, +inf, -inf: finite output equal to the pinned rule (plane 0 twice), and the guard elements around the output buffer
    are untouched."""
    lib_mod = v3d('_lib')
    lib = lib_mod.load()
    n, D, h, w, G = 1, 9, 8, 8, 256
    vol = oracle.volume((n, D, h, w), 5) if 'map' in mode else oracle.logits((n, D, h, w), 1.0, 5)
    depth = oracle.special_depths(DS, DI, D, n * h * w, 6).reshape(n, h, w)
    depth.reshape(-1)[[3, 17, 40, 63]] = [np.nan, np.inf, -np.inf, np.nan]
    buf = torch.full((n * h * w + 2 * G,), -777.0, dtype=torch.float32, device=cuda)
    vol_d, depth_d = torch.from_numpy(vol).to(cuda), torch.from_numpy(depth).to(cuda)
    rc = getattr(lib, mode)(vol_d.data_ptr(), depth_d.data_ptr(), DS, DI, n, D, h, w, buf.data_ptr() + 4 * G,
                            lib_mod.stream_ptr(cuda))
    lib_mod.check(rc, mode)
    out = buf.cpu().numpy()
    assert np.all(out[:G] == -777.0) and np.all(out[-G:] == -777.0)
    got = out[G:-G].reshape(n, h, w)
    assert np.all(np.isfinite(got))
    if 'map' in mode:
        assert np.array_equal(bits(got), bits(oracle.gather_f32(vol, depth, DS, DI)))
        want0 = vol[0, 0] + vol[0, 0]
    else:
        p64 = oracle.softmax64(vol)
        want = oracle.check(p64, depth, DS, DI, indices=oracle.indices_f32(depth, DS, DI, D))['prob']
        assert oracle.max_error(got, want) <= 1e-6
        want0 = 2 * p64[0, 0]
    for k in (3, 17, 40, 63):
        np.testing.assert_allclose(got.reshape(-1)[k], want0.reshape(-1)[k], rtol=1e-6, atol=0)


# ---- given-depth mode on logits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['P_conf_a', 'P_conf_b', 'P_conf_c'])
def test_given_depth_mode_against_the_float64_checker(cuda, name):
    """The planes are those of the fp32 chain, exactly; the values within 4 x the reference's own fp32 error of the float64
    checker over ALL pixels (this mode has no uncertain set).  P_conf_c is the near-one-hot input (randn * 30)."""
    g = load(name)
    x = fixture_logits(g)
    lr = oracle.indices_f32(g['depth_given'], DS, DI, x.shape[1])
    want = oracle.check(oracle.softmax64(x), g['depth_given'], DS, DI, indices=lr)['prob']
    err = oracle.max_error(dev_logits(cuda, x, g['depth_given']), want)
    ref_err = float(g['ref_err_given'])
    print('%s given depth: device error %.3g, reference fp32 error %.3g, ratio %.2f' % (name, err, ref_err, err / ref_err))
    assert err <= oracle.RATIO * ref_err


# ---- own-depth (fused) mode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('feat_dim', [32, 16])
@pytest.mark.parametrize('shape', [(8, 8, 8), (16, 8, 24)])
def test_fused_depth_is_unchanged_and_prob_is_the_given_depth_mode(cuda, feat_dim, shape):
    """The smallest legal regulariser shapes, n = 2: the depth with return_prob has the bits of the depth without, for
    split-bf16 and exact-fp32 operands on the reference-layout entry; prob has the bits of the given-depth mode fed with that
    depth and the regularised volume."""
    mvs, syn, utils = v3d('mvsnet'), v3d('synthetic'), v3d('utils')
    D, h, w = shape
    net = mvs.CostRegNet(feat_dim, 8).eval()
    net.load_state_dict(syn.costregnet_weights(in_channels=feat_dim, seed=3, sharpen=20.0), strict=False)
    net = net.to(cuda)
    x = torch.rand((2, feat_dim, D, h, w), generator=torch.Generator().manual_seed(D + w)).to(cuda)
    ds, di = 0.5, 0.15
    vals = torch.linspace(ds, ds + di * (D - 1), D)
    for precision in ('split_bf16', 'fp32'):
        depth0, reg0 = net.regularize_depth(x, vals, return_reg=True, precision=precision)
        depth1, reg1, prob1 = net.regularize_depth(x, vals, return_reg=True, precision=precision, return_prob=True,
                                                   depth_start=ds, depth_interval=di)
        depth2, prob2 = net.regularize_depth(x, vals, precision=precision, return_prob=True, depth_start=ds, depth_interval=di)
        assert torch.equal(depth0, depth1) and torch.equal(depth0, depth2) and torch.equal(reg0, reg1), precision
        assert torch.equal(prob1, prob2)
        assert torch.equal(prob1, utils.confidence_from_logits(reg0, depth0, ds, di)), precision
        assert torch.isfinite(prob1).all() and float(prob1.min()) >= 0 and float(prob1.max()) <= 2.0
    with pytest.raises(ValueError):
        net.regularize_depth(x, vals, return_prob=True)


@pytest.mark.parametrize('name', ['P_conf_a', 'P_conf_b'])
def test_fused_mode_on_the_logit_fixtures(cuda, name):
    """The fused kernel on the fixtures' logits (v3d_soft_argmin_f32): its depth has the bits of soft_argmin_kernel's, its prob
    those of the given-depth mode fed with that depth; outside the uncertain set (at most 3 % of the pixels) prob lies within
    4 x the reference's own fp32 error of the float64 checker; ten launches give the same bits."""
    utils = v3d('utils')
    g = load(name)
    x = fixture_logits(g)
    xd, vals = torch.from_numpy(x).to(cuda), torch.from_numpy(g['depth_vals']).to(cuda)
    depth0 = utils.soft_argmin(xd, vals)
    depth, prob = utils.soft_argmin(xd, vals, return_prob=True, depth_start=DS, depth_interval=DI)
    assert torch.equal(depth0, depth)
    assert torch.equal(prob, utils.confidence_from_logits(xd, depth, DS, DI))
    p64 = oracle.softmax64(x)
    depth64 = oracle.expectation64(p64, g['depth_vals'])
    own = oracle.check(p64, depth64, DS, DI)
    share = float(own['uncertain'].mean())
    assert share <= oracle.UNCERTAIN_CAP          # the test cannot hide a failure by excluding pixels
    keep = ~own['uncertain']
    err_depth = oracle.max_error(depth.cpu().numpy(), depth64)
    err = oracle.max_error(prob.cpu().numpy(), own['prob'], keep)
    ref_err = float(g['ref_err_own'])
    print('%s own depth: device error %.3g, reference fp32 error %.3g, ratio %.2f; depth error %.3g (reference %.3g); '
          'uncertain %.2f %%' % (name, err, ref_err, err / ref_err, err_depth, float(g['ref_err_depth']), 100 * share))
    assert err <= oracle.RATIO * ref_err
    for _ in range(10):
        d, p = utils.soft_argmin(xd, vals, return_prob=True, depth_start=DS, depth_interval=DI)
        assert torch.equal(d, depth) and torch.equal(p, prob)


# ---- plumbing, on the smallest scene of the driver tests --------------------------------------------------------------------
def _net(cuda, precision='split_bf16'):
    import test_driver as td
    syn, lm = v3d('synthetic'), v3d('lightningmodel')
    cr, pn, un, dec = td.weights()
    net = lm.PL3DVNet(None, td.CFG, 0.16, feat_dim=32, img_size=td.IMG, precision=precision).eval()
    net.mvsnet.cnn_3d.load_state_dict(cr, strict=False)
    net.pointnet.load_state_dict(pn)
    net.sparse_conv.load_state_dict(un)
    net.decoder.load_state_dict(dec, strict=False)
    for m, seed, cin in zip((net.refine_quarter, net.refine_half, net.refine_full), (5, 6, 7), (33, 33, 4)):
        m.load_state_dict(syn.propagation_weights(cin, 32, seed), strict=False)
    return net.to(cuda)


def _scene(full=False):
    import test_driver as td
    syn = v3d('synthetic')
    scene = td.make_scene()
    if full:
        n_img = scene.rotmats.shape[0]
        scene.features_half = syn.make_features(n_img, 32, 2 * td.FEAT[0], 2 * td.FEAT[1], seed=42)
        scene.images = syn.make_images(n_img, td.IMG, seed=43)
    return scene


@pytest.mark.parametrize('precision', ['split_bf16', 'fp32'])
def test_forward_and_graph_return_prob(cuda, precision):
    """MVSNet.forward(return_prob=True) appends the map and leaves the depth's bits alone (split hand-off for split-bf16, the
    channel-last fp32 hand-off for exact fp32); CostVolumeGraph(return_prob=True) replays to the eager bits."""
    import test_driver as td
    mvs, utils = v3d('mvsnet'), v3d('utils')
    net = _net(cuda, precision).mvsnet
    scene = _scene().to(cuda)
    args = (td.CFG['depth_start'], td.CFG['depth_interval'], td.CFG['n_intervals'], td.CFG['size'])
    with torch.no_grad():
        out0 = net(scene, *args, n_ref=5)
        out1 = net(scene, *args, n_ref=5, return_prob=True)
        assert len(out0) == 4 and len(out1) == 5 and torch.equal(out0[0], out1[0])
        depth, prob = out1[0], out1[4]
        assert tuple(prob.shape) == (5,) + td.CFG['size'] and torch.isfinite(prob).all()
        d2, _, reg = net.cost_volume_depth(scene.features_quarter, scene, *args, return_intermediates=True)
        d3, _, reg3, prob3 = net.cost_volume_depth(scene.features_quarter, scene, *args, return_intermediates=True, return_prob=True)
        assert torch.equal(d2, d3) and torch.equal(reg, reg3)
        assert torch.equal(prob3, utils.confidence_from_logits(reg, d2, args[0], args[1]))
        graph = mvs.CostVolumeGraph(net, scene.features_quarter, scene, *args, n_ref=5, return_prob=True)
        gd, gp = graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gd, depth) and torch.equal(gp, prob)
        plain = mvs.CostVolumeGraph(net, scene.features_quarter, scene, *args, n_ref=5)
        assert torch.equal(plain.replay(), depth)


def test_process_scene_and_pred_func_with_prob(cuda, tmp_path):
    """process_scene(return_prob=True) returns the stage-1 map of every view in view order (chunks of 2 views against one call
    over the scene); pred_func_with_prob -> write_preds -> prepare_preds(prob_resize='nearest') zeroes exactly the pixels whose
    nearest-resized confidence is at most 0.2; without the keyword prepare_preds still raises."""
    import test_driver as td
    drv, res, fusion = v3d('eval_3dvnet'), v3d('results'), v3d('fusion')
    net = _net(cuda)
    scene = _scene(full=True)
    depth_plain = drv.process_scene(scene, net, 1, cuda, td.CFG, td.OFFSETS, 2, 3)
    depth, init_prob = drv.process_scene(scene, net, 1, cuda, td.CFG, td.OFFSETS, 2, 3, return_prob=True)
    assert torch.equal(depth, depth_plain)
    args = (td.CFG['depth_start'], td.CFG['depth_interval'], td.CFG['n_intervals'], td.CFG['size'])
    with torch.no_grad():
        whole = net.mvsnet(_scene().to(cuda), *args, n_ref=5, return_prob=True)[4]
    assert torch.equal(init_prob, whole)
    assert any(not torch.equal(whole[0], whole[i]) for i in range(1, 5))          # view order is observable

    dset = types.SimpleNamespace(n_src_on_either_side=1)
    plain = drv.pred_func(scene, '/data/scene0000_00', dset, net)
    assert plain[1] is None and plain[2] is None
    out = drv.pred_func_with_prob(scene, '/data/scene0000_00', dset, net)
    assert len(out) == 3 and out[2] is None and np.array_equal(out[0], plain[0])
    assert isinstance(out[1], np.ndarray) and out[1].dtype == np.float32 and out[1].shape == (5,) + td.CFG['size']
    ref_idx = torch.unique(scene.ref_src_edges[0])
    path = str(tmp_path / 'preds.npz')
    res.write_preds(path, '/data/scene0000_00', out[0], scene, ref_idx, np.arange(scene.rotmats.shape[0]), init_prob=out[1])
    with pytest.raises(ValueError):
        fusion.prepare_preds(path)
    with pytest.raises(ValueError):
        fusion.prepare_preds(path, prob_resize='lanczos')
    depths, _, _ = fusion.prepare_preds(path, prob_resize='nearest')
    big = F.interpolate(torch.from_numpy(out[1]).unsqueeze(1), td.IMG, mode='nearest').squeeze(1).numpy()
    low = big <= 0.2
    print('confidence <= 0.2 on %.1f %% of the pixels (min %.3f, max %.3f)' % (100 * low.mean(), big.min(), big.max()))
    assert 0 < low.mean() < 1
    assert np.all(out[0] > 0)
    assert np.array_equal(depths == 0, low) and np.array_equal(depths[~low], out[0][~low])


# ---- error codes ------------------------------------------------------------------------------------------------------------
def test_error_codes_of_the_entry_points():
    lib_mod = v3d('_lib')
    lib = lib_mod.load()
    BAD_SHAPE, BAD_ARG = -1, -2
    p = ctypes.c_void_p(4096)          # never dereferenced: every call below returns before any launch
    for fn in (lib.v3d_probability_map_f32, lib.v3d_confidence_logits_f32):
        assert fn(None, p, DS, DI, 1, 8, 8, 8, p, None) == BAD_ARG and b'null' in lib.v3d_last_error()
        assert fn(p, None, DS, DI, 1, 8, 8, 8, p, None) == BAD_ARG
        assert fn(p, p, DS, DI, 1, 8, 8, 8, None, None) == BAD_ARG
        assert fn(p, p, DS, 0.0, 1, 8, 8, 8, p, None) == BAD_ARG and b'depth_interval' in lib.v3d_last_error()
        assert fn(p, p, DS, float('nan'), 1, 8, 8, 8, p, None) == BAD_ARG
        assert fn(p, p, float('inf'), DI, 1, 8, 8, 8, p, None) == BAD_ARG
        assert fn(p, p, DS, DI, 1, 0, 8, 8, p, None) == BAD_SHAPE
        assert fn(p, p, DS, DI, 0, 8, 8, 8, p, None) == BAD_SHAPE
    reg = lib.v3d_costreg_depth_prob
    ok = dict(h=p, var=p, layout=0, prec=0, vals=p, ds=DS, di=DI, n=1, D=8, H=8, W=8, depth=p, reg=None, prob=p, ws=p, wsb=1 << 40)

    def call(**kw):
        a = dict(ok, **kw)
        return reg(a['h'], a['var'], a['layout'], a['prec'], a['vals'], a['ds'], a['di'], a['n'], a['D'], a['H'], a['W'],
                   a['depth'], a['reg'], a['prob'], a['ws'], a['wsb'], None)
    for name in ('h', 'var', 'vals', 'depth', 'ws'):
        assert call(**{name: None}) == BAD_ARG and b'null' in lib.v3d_last_error(), name
    assert call(D=12) == BAD_SHAPE and b'multiples of 8' in lib.v3d_last_error()
    assert call(H=9) == BAD_SHAPE and call(n=0) == BAD_SHAPE
    assert call(di=0.0) == BAD_ARG and b'depth_interval' in lib.v3d_last_error()
    assert call(layout=3) == BAD_ARG and call(prec=7) == BAD_ARG
    assert call(wsb=16) == -3
    sa = lib.v3d_soft_argmin_f32
    assert sa(None, p, DS, DI, 1, 8, 8, 8, p, p, None) == BAD_ARG
    assert sa(p, p, DS, 0.0, 1, 8, 8, 8, p, p, None) == BAD_ARG
    assert sa(p, p, DS, DI, 1, 0, 8, 8, p, p, None) == BAD_SHAPE
