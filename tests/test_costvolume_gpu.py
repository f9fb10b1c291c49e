"""GPU parity tests, rows A1-A6: the HIP path (through the C ABI) against the golden vectors
captured from the reference and against the oracle on the same seeded inputs.

Tolerances (BASELINE.json north_star: depth within 1e-4 relative):
  variance volume  : 5e-7 absolute against the reference-generated goldens and against oracle/pinned.py.  The warp
                     kernels implement the evaluation orders of the reference run that produced the goldens (sample
                     coordinates bit-exact, test_sample_positions_bit_exact_vs_pinned_oracle), so only the fused square
                     in the sum of squares is left: measured 6e-8 (cfg2), 1.2e-7 (cfg1).
                     Against oracle/costvolume.py run on THIS host the bound is 5e-5: torch.bmm's last bits depend on
                     the host BLAS (MKL on the GPU box's EPYC host does not use FMA, the build container's does), and one
                     ulp at ~160 px is 1.5e-5 px.
  regularised vol. : 5e-5 * max|x_reg| for split-bf16 operands (measured 1.1e-5), 1e-5 for exact fp32 (measured 1.3e-6)
  depth            : 1e-4 relative (measured 2.2e-5 split-bf16, 2.3e-6 exact fp32 on cfg2)
"""
import numpy as np
import pytest
import torch

from conftest import v3d
from helpers import golden_costreg_weights, load_golden, t
from oracle import costvolume as ocv

pytestmark = pytest.mark.gpu

VAR_ATOL = 5e-7          # vs goldens / the pinned oracle
VAR_ATOL_HOST = 5e-5     # vs the torch oracle on this host (BLAS-dependent last bits)
REG_RTOL = 5e-5          # of max|x_reg|, split-bf16 operands
DEPTH_RTOL = 1e-4


def _net(sd, dev, img_size):
    mvs = v3d('mvsnet')
    net = mvs.MVSNet(32, img_size).eval()
    net.cnn_3d.load_state_dict(sd, strict=False)
    return net.to(dev)


def _run_hip(net, feat, R, tv, K, edges, depth_cfg, plane_size, dev):
    Batch = v3d('batch').Batch
    b = Batch(None, R, tv, K, None, edges).to(dev)
    d0, dd, D = depth_cfg
    with torch.no_grad():
        depth, var, reg = net.cost_volume_depth(feat.to(dev), b, float(d0), float(dd), int(D),
                                                tuple(plane_size), return_intermediates=True)
        # the product path hands the variance to the regulariser in its split-bf16 input format: same numbers
        # (conv0 performs the identical hi/lo split on the fp32 volume), so the depth must be bit-identical
        depth_split = net.cost_volume_depth(feat.to(dev), b, float(d0), float(dd), int(D), tuple(plane_size))
        if feat.shape[1] == 32:
            sv = v3d('mvsnet').plane_sweep_variance(feat.to(dev), b.rotmats, b.tvecs, b.K, b.ref_src_edges,
                                                    float(d0), float(dd), int(D), net.img_size,
                                                    tuple(plane_size), split=True)
            assert torch.equal(_decode_split(sv), _split_roundtrip(var))
    torch.cuda.synchronize()
    assert torch.equal(depth_split, depth), 'split-variance path differs from the fp32-variance path'
    return depth.cpu(), var.cpu(), reg.cpu()


def _bf16_rne_bits(x):
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xffffffff
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff


def _split_roundtrip(var):
    """hi + lo of the fp32 volume, the value the split format stores (include/v3d.h)."""
    hb = _bf16_rne_bits(var)
    hi = torch.where(hb >= 0x8000, (hb << 16) - (1 << 32), hb << 16).to(torch.int32).view(torch.float32)
    lb = _bf16_rne_bits(var - hi)
    lo = torch.where(lb >= 0x8000, (lb << 16) - (1 << 32), lb << 16).to(torch.int32).view(torch.float32)
    return hi + lo


def _decode_split(sv):
    """[n][4 groups][hi, lo][D][h][w][8 bf16] -> fp32 [n, 32, D, h, w] as hi + lo."""
    n, C, D, h, w = sv.shape
    raw = sv.data.contiguous().view(torch.int16).view(n, 4, 2, D, h, w, 8)
    f = (raw.to(torch.int32) << 16).view(torch.float32)
    x = f[:, :, 0] + f[:, :, 1]                                  # [n, 4, D, h, w, 8]
    return x.permute(0, 1, 5, 2, 3, 4).reshape(n, 32, D, h, w)


@pytest.mark.parametrize('name', ['A_tiny_flat', 'A_tiny_sharp', 'A_tiny_rotated'])
def test_hip_matches_reference_golden_tiny(name, cuda):
    g = load_golden(name)
    sd = golden_costreg_weights(g)
    img_size = tuple(int(v) for v in g['img_size'])
    plane_size = tuple(int(v) for v in g['plane_size'])
    net = _net(sd, cuda, img_size)
    depth, var, reg = _run_hip(net, t(g['feat']), t(g['rotmats']), t(g['tvecs']), t(g['K']),
                               t(g['edges']), g['depth_cfg'], plane_size, cuda)
    np.testing.assert_allclose(var.numpy(), g['var'], rtol=0, atol=VAR_ATOL)
    scale = float(np.abs(g['reg']).max())
    np.testing.assert_allclose(reg.numpy(), g['reg'], rtol=0, atol=REG_RTOL * scale)
    np.testing.assert_allclose(depth.numpy(), g['depth'], rtol=DEPTH_RTOL, atol=0)


@pytest.mark.parametrize('name,cfg', [('A_cfg1', 'cfg1'), ('A_cfg2', 'cfg2')])
def test_hip_matches_reference_golden_cfg(name, cfg, cuda):
    g = load_golden(name)
    syn = v3d('synthetic')
    inp = syn.make_costvolume_inputs(cfg, n_ref=int(g['n_ref']))
    assert abs(float(inp['feat'].double().sum()) - float(g['feat_checksum'])) < 1e-6
    sd = golden_costreg_weights(g)
    net = _net(sd, cuda, inp['img_size'])
    depth, var, reg = _run_hip(net, inp['feat'], inp['rotmats'], inp['tvecs'], inp['K'],
                               inp['edges'], inp['depth'], inp['plane_size'], cuda)
    if cfg == 'cfg1':
        vs, rs = var[:, ::4, ::3, ::5, ::7], reg[:, ::3, ::5, ::7]
    else:
        vs, rs = var[:, ::4, ::5, ::7, ::7], reg[:, ::5, ::7, ::7]
    np.testing.assert_allclose(vs.numpy(), g['var_sub'], rtol=0, atol=VAR_ATOL)
    assert abs(float(var.double().sum()) - float(g['var_sum'])) < 1e-4 * abs(float(g['var_sum']))
    scale = float(np.abs(g['reg_sub']).max())
    np.testing.assert_allclose(rs.numpy(), g['reg_sub'], rtol=0, atol=REG_RTOL * scale)
    np.testing.assert_allclose(depth.numpy(), g['depth'], rtol=DEPTH_RTOL, atol=0)
    # the gate is not vacuous: the sharpened weights give a wide depth range
    assert g['depth'].max() - g['depth'].min() > 1.0


def test_hip_matches_reference_golden_cfg5(cuda):
    """BASELINE config 5 at full size (480x640, 192 planes, 120x160 plane grid) against the reference-generated golden:
    11 edges per reference (> the 8-edge LDS pass of the warp kernel: its multi-pass branch), a count that is not a power
    of two (the IEEE-division mean), D = 192 and partial 28-wide x tiles (160 = 5 x 28 + 20) in every layer."""
    g = load_golden('A_cfg5')
    syn = v3d('synthetic')
    inp = syn.make_costvolume_inputs('cfg5', n_ref=1)
    assert inp['edges'].shape[1] == 11
    assert abs(float(inp['feat'].double().sum()) - float(g['feat_checksum'])) < 1e-6
    sd = golden_costreg_weights(g)
    net = _net(sd, cuda, inp['img_size'])
    depth, var, reg = _run_hip(net, inp['feat'], inp['rotmats'], inp['tvecs'], inp['K'],
                               inp['edges'], inp['depth'], inp['plane_size'], cuda)
    np.testing.assert_allclose(var[:, ::4, ::7, ::11, ::13].numpy(), g['var_sub'], rtol=0, atol=VAR_ATOL)
    assert abs(float(var.double().sum()) - float(g['var_sum'])) < 1e-4 * abs(float(g['var_sum']))
    scale = float(np.abs(g['reg_sub']).max())
    np.testing.assert_allclose(reg[:, ::7, ::11, ::13].numpy(), g['reg_sub'], rtol=0, atol=REG_RTOL * scale)
    np.testing.assert_allclose(depth[:, ::3, ::3].numpy(), g['depth_sub'], rtol=DEPTH_RTOL, atol=0)
    assert abs(float(depth.double().sum()) - float(g['depth_sum'])) < 2e-5 * abs(float(g['depth_sum']))
    assert g['depth_sub'].max() - g['depth_sub'].min() > 1.0


def test_full_size_properties_cfg5_batch(cuda):
    """cfg5 size, 3 references per launch: batch invariance (bit-exact), zero variance for self-only edges, depth
    within the plane range -- the size-independent properties of cfg2, at the stress size."""
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    Batch = v3d('batch').Batch
    inp = syn.make_costvolume_inputs('cfg5', n_ref=3)
    sd = syn.costregnet_weights(seed=0, sharpen=200.0)
    net = _net(sd, cuda, inp['img_size'])
    d0, dd, D = inp['depth']
    b = Batch(None, inp['rotmats'], inp['tvecs'], inp['K'], None, inp['edges']).to(cuda)
    feat = inp['feat'].to(cuda)
    with torch.no_grad():
        depth = net.cost_volume_depth(feat, b, d0, dd, D, inp['plane_size'])
        assert torch.isfinite(depth).all()
        assert depth.min() >= d0 - 1e-4 and depth.max() <= d0 + dd * (D - 1) + 1e-4
        per = inp['edges'].shape[1] // 3
        bi = Batch(None, inp['rotmats'], inp['tvecs'], inp['K'], None, inp['edges'][:, per:2 * per]).to(cuda)
        assert torch.equal(net.cost_volume_depth(feat, bi, d0, dd, D, inp['plane_size'])[0], depth[1])
        self_edges = torch.tensor([[6] * 11, [6] * 11])
        v_self = mvs.plane_sweep_variance(feat, b.rotmats, b.tvecs, b.K, self_edges.to(cuda), d0, dd, D,
                                          inp['img_size'], inp['plane_size'])
        assert float(v_self.abs().max()) < 1e-6


def test_hip_matches_oracle_multi_ref(cuda):
    """Several reference views per launch (sliding window), cfg1 shape, vs the oracle."""
    syn = v3d('synthetic')
    inp = syn.make_costvolume_inputs('cfg1', n_ref=3, seed=77)
    sd = syn.costregnet_weights(seed=4, sharpen=200.0)
    d0, dd, D = inp['depth']
    with torch.no_grad():
        depth_o, var_o, reg_o = ocv.mvsnet_depth(inp['feat'], inp['rotmats'], inp['tvecs'], inp['K'],
                                                 inp['edges'], sd, d0, dd, D, inp['img_size'],
                                                 inp['plane_size'], pinned=True)
    net = _net(sd, cuda, inp['img_size'])
    depth, var, reg = _run_hip(net, inp['feat'], inp['rotmats'], inp['tvecs'], inp['K'],
                               inp['edges'], inp['depth'], inp['plane_size'], cuda)
    np.testing.assert_allclose(var.numpy(), var_o.numpy(), rtol=0, atol=VAR_ATOL)
    np.testing.assert_allclose(reg.numpy(), reg_o.numpy(), rtol=0, atol=REG_RTOL * float(reg_o.abs().max()))
    np.testing.assert_allclose(depth.numpy(), depth_o.numpy(), rtol=DEPTH_RTOL, atol=0)


def test_fused_path_partial_tiles_and_ragged_edges(cuda):
    """Whole path A on a volume whose extents are multiples of 8 (the regulariser's requirement) but of none of the
    kernels' tile sizes (24 x 24 x 40: partial 28- and 14-wide x tiles, partial z/y tiles on the coarse levels), with
    ragged, unsorted edge lists (1, 3 and 9 sources), vs the oracle."""
    syn = v3d('synthetic')
    img_size, feat_size, plane_size, D = (96, 160), (24, 40), (24, 40), 24
    R, tv, K = syn.make_cameras(12, img_size, seed=11)
    feat = syn.make_features(12, 32, *feat_size, seed=11)
    refs = [4] + [7] * 3 + [2] * 9
    srcs = [4] + [6, 7, 8] + list(range(0, 9))
    perm = torch.randperm(len(refs), generator=torch.Generator().manual_seed(1))
    edges = torch.tensor([refs, srcs])[:, perm]
    sd = syn.costregnet_weights(seed=5, sharpen=200.0)
    d0, dd = 0.5, 0.1
    with torch.no_grad():
        depth_o, var_o, reg_o = ocv.mvsnet_depth(feat, R, tv, K, edges, sd, d0, dd, D, img_size, plane_size, pinned=True)
    net = _net(sd, cuda, img_size)
    depth, var, reg = _run_hip(net, feat, R, tv, K, edges, (d0, dd, D), plane_size, cuda)
    np.testing.assert_allclose(var.numpy(), var_o.numpy(), rtol=0, atol=VAR_ATOL)
    np.testing.assert_allclose(reg.numpy(), reg_o.numpy(), rtol=0, atol=REG_RTOL * float(reg_o.abs().max()))
    np.testing.assert_allclose(depth.numpy(), depth_o.numpy(), rtol=DEPTH_RTOL, atol=0)
    assert float(depth_o.max() - depth_o.min()) > 0.5


@pytest.mark.parametrize('D', [6, 13])
def test_psv_ragged_edges_and_odd_grid(D, cuda):
    """Ragged edge lists (1, 3 and 10 sources -- more than one LDS pass), a plane grid that is not
    a multiple of the 8-pixel tile, D smaller than / not a multiple of the 8-plane chunk, unsorted edge order."""
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    img_size, feat_size, plane_size = (64, 80), (16, 20), (7, 9)
    R, tv, K = syn.make_cameras(12, img_size, seed=3)
    feat = syn.make_features(12, 32, *feat_size, seed=3)
    refs = [4] + [7] * 3 + [2] * 10
    srcs = [4] + [6, 7, 8] + list(range(0, 10))
    perm = torch.randperm(len(refs), generator=torch.Generator().manual_seed(0))
    edges = torch.tensor([refs, srcs])[:, perm]
    from oracle import pinned
    var_o = pinned.warp_variance(feat, R, tv, K, edges, 0.5, 0.3, D, img_size, plane_size)
    var = mvs.plane_sweep_variance(feat.to(cuda), R, tv, K, edges.to(cuda), 0.5, 0.3, D, img_size,
                                   plane_size)
    torch.cuda.synchronize()
    np.testing.assert_allclose(var.cpu().numpy(), var_o.numpy(), rtol=0, atol=VAR_ATOL)
    # the split hand-off format of the same volume: hi + lo of exactly these numbers
    sv = mvs.plane_sweep_variance(feat.to(cuda), R, tv, K, edges.to(cuda), 0.5, 0.3, D, img_size, plane_size,
                                  split=True)
    assert torch.equal(_decode_split(sv), _split_roundtrip(var))


def test_psv_kernel_variants_bit_identical(cuda):
    """The three warp kernels -- window (default: LDS-staged footprint windows), reuse (developer option psv_kernel = 1: footprints
    in registers, masked gathers; also the fallback for feature stacks of 2 GB or more) and the plain gather kernel (psv_kernel = 2,
    IEEE divisions; the 16-channel path) -- must produce the same bits,
    also for camera pairs whose footprints do not fit the window (zoomed / rolled / far-off sources: the out-of-window path),
    partial tiles, 13 planes, 7 edges (division path of the mean), fp32 and split output.  Each variant hashes the volumes in its
    own interpreter (scripts/psv_hash.py --option=psv_kernel=N -> v3d_set_option)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for extra in ([], ['--option=psv_kernel=1'], ['--option=psv_kernel=2']):
        r = subprocess.run([sys.executable, os.path.join(root, 'scripts', 'psv_hash.py')] + extra, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith(('cfg', '7-edge', 'exotic'))])
    assert len(outs[0]) == 6 and outs[0] == outs[1] == outs[2], outs
    assert 'nan' not in ' '.join(outs[0])


def test_conv1_conv2_depth_march_agrees_with_tile_kernels(cuda):
    """csrc/conv12z.hip (the default: conv1 + conv2 as one depth march, conv1's output never leaves LDS) against the two tile
    kernels it replaces (developer option c12_march = 0): the same products, conv2's two input-channel chunks summed in another order --
    regularised volume within 5e-6 of its range (measured 2.1e-6), depth within 1e-5, on a cfg1 batch and on a volume with partial tiles and
    ragged edges.  Each variant runs in its own interpreter (scripts/c9_dump.py --option=c12_march=0)."""
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        res = []
        for extra in ([], ['--option=c12_march=0']):
            f = os.path.join(td, 'c12_%d.npz' % len(res))
            r = subprocess.run([sys.executable, os.path.join(root, 'scripts', 'c9_dump.py'), f] + extra,
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            res.append(dict(np.load(f)))
    for k in ('a', 'b'):
        scale = float(np.abs(res[1]['reg_' + k]).max())
        np.testing.assert_allclose(res[0]['reg_' + k], res[1]['reg_' + k], rtol=0, atol=5e-6 * scale)
        np.testing.assert_allclose(res[0]['depth_' + k], res[1]['depth_' + k], rtol=1e-5, atol=0)
        assert not np.array_equal(res[0]['reg_' + k], res[1]['reg_' + k])          # another kernel really ran


def test_fp32_chain_agrees_with_split_bf16_chain(cuda):
    """precision='fp32' runs the regulariser on the exact-fp32 kernels (per-layer kernels for conv0..conv8 behind
    return_intermediates, conv9 + skip + prob fused on fp32 matrix instructions);
    the default 'split_bf16' chain runs on split-bf16 matrix cores.  Both are within 1e-4 of the oracle, hence within
    2e-4 of each other; the regularised volumes agree to 4e-4 of their range.  The choice is an argument of the C ABI
    (include/v3d.h V3D_PRECISION_*), so both run in this process."""
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    Batch = v3d('batch').Batch
    inp = syn.make_costvolume_inputs('cfg1', n_ref=2, seed=21)
    sd = syn.costregnet_weights(seed=3, sharpen=200.0)
    net = _net(sd, cuda, inp['img_size'])
    b = Batch(None, inp['rotmats'], inp['tvecs'], inp['K'], None, inp['edges']).to(cuda)
    d0, dd, D = inp['depth']
    res = {}
    with torch.no_grad():
        for pr in ('split_bf16', 'fp32'):
            depth, _, reg = net.cost_volume_depth(inp['feat'].to(cuda), b, d0, dd, D, inp['plane_size'],
                                                  return_intermediates=True, precision=pr)
            res[pr] = (depth.cpu().numpy(), reg.cpu().numpy())
        # the module-level default is the same switch
        net32 = mvs.MVSNet(32, inp['img_size'], precision='fp32').eval()
        net32.cnn_3d.load_state_dict(sd, strict=False)
        d32 = net32.to(cuda).cost_volume_depth(inp['feat'].to(cuda), b, d0, dd, D, inp['plane_size'])
        d32_kw = net.cost_volume_depth(inp['feat'].to(cuda), b, d0, dd, D, inp['plane_size'], precision='fp32')
        depth_o = ocv.mvsnet_depth(inp['feat'], inp['rotmats'], inp['tvecs'], inp['K'], inp['edges'], sd, d0, dd, D,
                                   inp['img_size'], inp['plane_size'])[0].numpy()
    # (without intermediates the exact-fp32 chain takes the channel-last volume and the depth-march conv0: the same products in
    # another summation order than the per-layer chain behind return_intermediates)
    assert torch.equal(d32, d32_kw)
    np.testing.assert_allclose(d32.cpu().numpy(), res['fp32'][0], rtol=2e-5, atol=0)
    np.testing.assert_allclose(res['split_bf16'][0], res['fp32'][0], rtol=2e-4, atol=0)
    scale = float(np.abs(res['fp32'][1]).max())
    np.testing.assert_allclose(res['split_bf16'][1], res['fp32'][1], rtol=0, atol=4e-4 * scale)
    assert not np.array_equal(res['split_bf16'][0], res['fp32'][0])      # the argument really selected another chain
    for pr in res:
        np.testing.assert_allclose(res[pr][0], depth_o, rtol=DEPTH_RTOL, atol=0)


def test_exact_fp32_fused_conv9_prob_partial_tiles_vs_oracle(cuda):
    """The exact-fp32 chain's last kernel (conv9_prob_kernel<true>: transposed conv + conv0 skip + 8 -> 1 prob conv on
    v_mfma_f32_16x16x4_f32) on a volume that is a multiple of none of its tile sizes (24 x 24 x 40: partial 4 x 8 x 28
    prob tiles on every axis): regularised volume within 1e-5 of its range of the oracle's, depth within 2e-5; the
    per-layer exact-fp32 conv9 kernel followed by the torch prob conv gives the same volume to 2e-6 of its range."""
    syn = v3d('synthetic')
    img_size, feat_size, plane_size, D = (96, 160), (24, 40), (24, 40), 24
    R, tv, K = syn.make_cameras(12, img_size, seed=13)
    feat = syn.make_features(12, 32, *feat_size, seed=13)
    refs = [4] * 2 + [7] * 3 + [2] * 5
    srcs = [3, 5] + [6, 8, 9] + [0, 1, 3, 4, 5]
    edges = torch.tensor([refs, srcs])
    sd = syn.costregnet_weights(seed=7, sharpen=200.0)
    d0, dd = 0.5, 0.1
    with torch.no_grad():
        depth_o, var_o, reg_o = ocv.mvsnet_depth(feat, R, tv, K, edges, sd, d0, dd, D, img_size, plane_size, pinned=True)
    net = _net(sd, cuda, img_size)
    Batch = v3d('batch').Batch
    b = Batch(None, R, tv, K, None, edges).to(cuda)
    with torch.no_grad():
        depth, var, reg = net.cost_volume_depth(feat.to(cuda), b, d0, dd, D, plane_size, return_intermediates=True,
                                                precision='fp32')
        # the same layers one by one: conv0..conv8 per-layer exact-fp32 kernels, conv9 per-layer, prob conv in torch
        c = net.cnn_3d
        x = var
        outs = []
        for l in range(7):
            x = c.run_layer(l, x, precision='fp32')
            outs.append(x)
        u7 = c.run_layer(7, outs[6], outs[4], precision='fp32')
        u8 = c.run_layer(8, u7, outs[2], precision='fp32')
        u9 = c.run_layer(9, u8, outs[0], precision='fp32')
        reg_layers = torch.nn.functional.conv3d(u9.cpu(), sd['prob.weight'], sd['prob.bias'], padding=1)[:, 0]
    scale = float(reg_o.abs().max())
    np.testing.assert_allclose(reg.cpu().numpy(), reg_o.numpy(), rtol=0, atol=1e-5 * scale)
    np.testing.assert_allclose(reg.cpu().numpy(), reg_layers.numpy(), rtol=0, atol=2e-6 * scale)
    np.testing.assert_allclose(depth.cpu().numpy(), depth_o.numpy(), rtol=2e-5, atol=0)
    assert float(depth_o.max() - depth_o.min()) > 0.5


def test_exact_fp32_chain_through_the_channel_last_volume(cuda):
    """precision='fp32' without intermediates: the warp kernel writes the volume as fp32 channel-last slots
    (v3d_psv_variance_cl8) and conv0 runs as the exact-fp32 depth march (v3d_costreg_depth_cl8).  (1) the slots hold the
    reference-layout volume bit for bit (ragged edges, partial tiles, 13 planes); (2) the depth is inside the 1e-4 gate of the
    oracle and within 2e-5 of the per-layer exact-fp32 chain on the reference-layout volume (same products, another
    summation order); (3) batch invariance is bit-exact."""
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    Batch = v3d('batch').Batch
    img_size, feat_size, plane_size = (64, 80), (16, 20), (7, 9)
    R, tv, K = syn.make_cameras(12, img_size, seed=3)
    feat = syn.make_features(12, 32, *feat_size, seed=3)
    refs = [4] + [7] * 3 + [2] * 10
    srcs = [4] + [6, 7, 8] + list(range(0, 10))
    edges = torch.tensor([refs, srcs])
    var = mvs.plane_sweep_variance(feat.to(cuda), R, tv, K, edges.to(cuda), 0.5, 0.3, 13, img_size, plane_size)
    cv = mvs.plane_sweep_variance(feat.to(cuda), R, tv, K, edges.to(cuda), 0.5, 0.3, 13, img_size, plane_size, cl8=True)
    n, C, D, h, w = cv.shape
    dec = cv.data.contiguous().view(n, 4, 2, D, h, w, 4).permute(0, 1, 2, 6, 3, 4, 5).reshape(n, 32, D, h, w)
    assert torch.equal(dec, var)
    inp = syn.make_costvolume_inputs('cfg1', n_ref=3, seed=21)
    sd = syn.costregnet_weights(seed=3, sharpen=200.0)
    net = _net(sd, cuda, inp['img_size'])
    b = Batch(None, inp['rotmats'], inp['tvecs'], inp['K'], None, inp['edges']).to(cuda)
    d0, dd, D = inp['depth']
    with torch.no_grad():
        d_cl8 = net.cost_volume_depth(inp['feat'].to(cuda), b, d0, dd, D, inp['plane_size'], precision='fp32')
        d_ref, _, _ = net.cost_volume_depth(inp['feat'].to(cuda), b, d0, dd, D, inp['plane_size'], precision='fp32',
                                            return_intermediates=True)
        per = inp['edges'].shape[1] // 3
        b1 = Batch(None, inp['rotmats'], inp['tvecs'], inp['K'], None, inp['edges'][:, per:2 * per]).to(cuda)
        d_one = net.cost_volume_depth(inp['feat'].to(cuda), b1, d0, dd, D, inp['plane_size'], precision='fp32')
        depth_o = ocv.mvsnet_depth(inp['feat'], inp['rotmats'], inp['tvecs'], inp['K'], inp['edges'], sd, d0, dd, D,
                                   inp['img_size'], inp['plane_size'], pinned=True)[0].numpy()
    assert torch.equal(d_one[0], d_cl8[1])
    np.testing.assert_allclose(d_cl8.cpu().numpy(), d_ref.cpu().numpy(), rtol=2e-5, atol=0)
    np.testing.assert_allclose(d_cl8.cpu().numpy(), depth_o, rtol=2e-5, atol=0)
    assert not torch.equal(d_cl8, d_ref)          # another kernel really ran


def test_psv_feat_dim_16(cuda):
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    img_size, plane_size = (64, 80), (8, 8)
    e, n_img = syn.make_edges(2, 1, 1)
    R, tv, K = syn.make_cameras(n_img, img_size, seed=9)
    feat = syn.make_features(n_img, 16, 16, 20, seed=9)
    from oracle import pinned
    var_o = pinned.warp_variance(feat, R, tv, K, e, 0.5, 0.25, 8, img_size, plane_size)
    var = mvs.plane_sweep_variance(feat.to(cuda), R, tv, K, e.to(cuda), 0.5, 0.25, 8, img_size, plane_size)
    np.testing.assert_allclose(var.cpu().numpy(), var_o.numpy(), rtol=0, atol=VAR_ATOL)


@pytest.mark.parametrize('layer', list(range(10)))
def test_costreg_single_layers(layer, cuda):
    """Each conv / stride-2 conv / transposed conv layer (+folded BN, ReLU, skip) vs torch CPU,
    on a volume whose sizes are NOT multiples of the kernel's tile (partial tiles, halos)."""
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    sd = syn.costregnet_weights(seed=5)
    net = mvs.CostRegNet(32, 8).eval()
    net.load_state_dict(sd, strict=False)
    net = net.to(cuda)
    cin = [32, 8, 16, 16, 32, 32, 64, 64, 32, 16][layer]
    g = torch.Generator().manual_seed(layer)
    shape = (2, cin, 6, 10, 12) if layer < 7 else (2, cin, 3, 5, 6)
    x = torch.randn(shape, generator=g)
    name = 'conv%d' % layer
    if layer < 7:
        ref = ocv.conv_bn_relu3d(x, sd, name, stride=2 if layer in (1, 3, 5) else 1)
        skip = None
    else:
        ref = ocv.deconv_bn_relu3d(x, sd, name)
        skip = torch.randn(ref.shape, generator=g)
        ref = skip + ref
    out = net.run_layer(layer, x.to(cuda), None if skip is None else skip.to(cuda))
    torch.cuda.synchronize()
    # conv0 runs on split-bf16 matrix cores (operands carry 16 mantissa bits): measured 7e-6 of max|out|;
    # every other layer is exact-fp32 MFMA
    tol = (4e-5 if layer == 0 else 1e-5) * max(1.0, float(ref.abs().max()))
    np.testing.assert_allclose(out.cpu().numpy(), ref.numpy(), rtol=1e-5 if layer else 0, atol=tol)
    if layer >= 7:      # output width 14: rows that are not 16-byte addressable take the direct (unstaged) epilogue
        x7 = torch.randn((1, cin, 2, 3, 7), generator=g)
        ref7 = ocv.deconv_bn_relu3d(x7, sd, name)
        skip7 = torch.randn(ref7.shape, generator=g)
        out7 = net.run_layer(layer, x7.to(cuda), skip7.to(cuda))
        np.testing.assert_allclose(out7.cpu().numpy(), (skip7 + ref7).numpy(), rtol=1e-5,
                                   atol=1e-5 * max(1.0, float(ref7.abs().max())))
    if layer == 0:      # and conv0's exact-fp32 kernel (precision='fp32'): float4 staging (width 12) ...
        out32 = net.run_layer(0, x.to(cuda), precision='fp32')
        np.testing.assert_allclose(out32.cpu().numpy(), ref.numpy(), rtol=1e-5,
                                   atol=1e-5 * max(1.0, float(ref.abs().max())))
        # ... and the one-float-per-lane staging a width that is not a multiple of 4 falls back to
        x14 = torch.randn((1, cin, 5, 9, 14), generator=g)
        ref14 = ocv.conv_bn_relu3d(x14, sd, name)
        out14 = net.run_layer(0, x14.to(cuda), precision='fp32')
        np.testing.assert_allclose(out14.cpu().numpy(), ref14.numpy(), rtol=1e-5,
                                   atol=1e-5 * max(1.0, float(ref14.abs().max())))
    if layer in (1, 2):  # the exact-fp32 kernels' direct epilogue (output rows that are not 16-byte addressable)
        x14 = torch.randn((1, cin, 5, 9, 14), generator=g)
        ref14 = ocv.conv_bn_relu3d(x14, sd, name, stride=2 if layer == 1 else 1)
        out14 = net.run_layer(layer, x14.to(cuda))
        np.testing.assert_allclose(out14.cpu().numpy(), ref14.numpy(), rtol=1e-5,
                                   atol=1e-5 * max(1.0, float(ref14.abs().max())))


@pytest.mark.parametrize('layer', list(range(1, 9)))
def test_costreg_single_layers_split_kernels(layer, cuda):
    """conv1..conv8 on the kernels of the fused path (split-bf16 matrix cores, split channel-last activations) vs
    torch CPU, on volumes that are not multiples of their tiles.  Operands carry 16 mantissa bits and K reaches 1728:
    tolerance 4e-5 of max|out| (measured <= 1e-5)."""
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    sd = syn.costregnet_weights(seed=6)
    net = mvs.CostRegNet(32, 8).eval()
    net.load_state_dict(sd, strict=False)
    net = net.to(cuda)
    cin = [32, 8, 16, 16, 32, 32, 64, 64, 32, 16][layer]
    g = torch.Generator().manual_seed(100 + layer)
    shape = (2, cin, 6, 10, 18) if layer < 7 else (2, cin, 3, 5, 9)
    x = torch.randn(shape, generator=g)
    name = 'conv%d' % layer
    if layer < 7:
        ref = ocv.conv_bn_relu3d(x, sd, name, stride=2 if layer in (1, 3, 5) else 1)
        skip = None
    else:
        ref = ocv.deconv_bn_relu3d(x, sd, name)
        skip = torch.randn(ref.shape, generator=g)
        ref = skip + ref
    out = net.run_layer(layer, x.to(cuda), None if skip is None else skip.to(cuda), split=True)
    torch.cuda.synchronize()
    err = float((out.cpu() - ref).abs().max())
    assert err <= 4e-5 * max(1.0, float(ref.abs().max())), err


def test_full_size_properties_cfg2_batch(cuda):
    """BASELINE config-2 size, several references per launch: size-independent properties.
    (1) a reference whose sources are all the reference itself has zero variance everywhere the
        samples are in range; (2) depth lies within the plane range; (3) results do not depend on
        how many references share a launch (batch of 4 == 4 single launches)."""
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    Batch = v3d('batch').Batch
    inp = syn.make_costvolume_inputs('cfg2', n_ref=4)
    sd = syn.costregnet_weights(seed=0, sharpen=200.0)
    net = _net(sd, cuda, inp['img_size'])
    d0, dd, D = inp['depth']
    b = Batch(None, inp['rotmats'], inp['tvecs'], inp['K'], None, inp['edges']).to(cuda)
    feat = inp['feat'].to(cuda)
    with torch.no_grad():
        depth, var, reg = net.cost_volume_depth(feat, b, d0, dd, D, inp['plane_size'],
                                                return_intermediates=True)
        assert torch.isfinite(var).all() and torch.isfinite(depth).all()
        assert depth.min() >= d0 - 1e-4 and depth.max() <= d0 + dd * (D - 1) + 1e-4
        per = inp['edges'].shape[1] // 4
        for i in range(4):
            bi = Batch(None, inp['rotmats'], inp['tvecs'], inp['K'], None,
                       inp['edges'][:, i * per:(i + 1) * per]).to(cuda)
            di = net.cost_volume_depth(feat, bi, d0, dd, D, inp['plane_size'])
            assert torch.equal(di[0], depth[i])
        self_edges = torch.tensor([[3] * 5, [3] * 5])
        v_self = mvs.plane_sweep_variance(feat, b.rotmats, b.tvecs, b.K, self_edges.to(cuda), d0, dd, D,
                                          inp['img_size'], inp['plane_size'])
        assert float(v_self.abs().max()) < 1e-6


@pytest.mark.parametrize('cfg', ['cfg1', 'cfg2'])
def test_sample_positions_bit_exact_vs_pinned_oracle(cfg, cuda):
    """The coordinates the warp kernels use (world points, row A1; sample positions, row A2 + grid_sample's
    un-normalisation) against oracle/pinned.py: BIT-EXACT.  oracle/pinned.py spells out the evaluation orders of the
    reference's torch-CPU run that produced the goldens (it reproduces the golden variance volumes bit for bit,
    tests/test_oracle_golden.py) and is host-independent, unlike torch.bmm itself."""
    from oracle import pinned
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    inp = syn.make_costvolume_inputs(cfg, n_ref=2, seed=5)
    d0, dd, D = inp['depth']
    Hf, Wf = inp['feat'].shape[2:]
    pos, world, csr = mvs.plane_sweep_sample_positions(inp['rotmats'], inp['tvecs'], inp['K'], inp['edges'], d0, dd, D,
                                                       inp['img_size'], (Hf, Wf), inp['plane_size'], cuda)
    ref_idx, _, edge_ofs, edge_src = csr
    assert torch.equal(edge_src.cpu().long(), inp['edges'][1])       # grouped per reference already: CSR == edge order
    K, R, t = inp['K'], inp['rotmats'], inp['tvecs']
    _, P = pinned.camera_blocks(K, R, t)
    pos, world = pos.cpu().numpy(), world.cpu().numpy()
    for r, ref in enumerate(ref_idx.cpu().tolist()):
        X = pinned.world_points(K, R, t, ref, d0, dd, D, inp['img_size'], inp['plane_size'])
        Xn = X.numpy()
        assert np.array_equal(world[r], Xn), 'world points of reference %d: %.4f bit-equal' % (ref, np.mean(world[r] == Xn))
        for e in range(int(edge_ofs[r]), int(edge_ofs[r + 1])):
            ix, iy = (a.numpy() for a in pinned.sample_positions(X, P[int(edge_src[e])], inp['img_size'], (Hf, Wf)))
            assert np.array_equal(pos[e, :, 0], ix) and np.array_equal(pos[e, :, 1], iy), \
                'edge %d: ix %.4f iy %.4f bit-equal' % (e, np.mean(pos[e, :, 0] == ix), np.mean(pos[e, :, 1] == iy))


@pytest.mark.parametrize('name', ['A_tiny_rotated', 'A_tiny_sharp'])
def test_poisoned_workspace_does_not_reach_the_variance(name, cuda):
    """The warp kernels read weight-0 taps from the zero border of the channel-last feature copy and, for samples clamped
    onto the lower border of the LAST image, from the zero row behind it.  0 x NaN is NaN: with the workspace pre-filled with
    0xFF bytes (fp32 NaN patterns, what recycled allocator memory may hold) the variance must still be finite and equal, bit
    for bit, to the one computed on a zero-filled workspace -- both kernel variants, fp32 and split output."""
    mvs = v3d('mvsnet')
    lib = v3d('_lib').load()
    g = load_golden(name)
    feat = torch.from_numpy(g['feat']).to(cuda)
    cams = [torch.from_numpy(g[k]).to(cuda) for k in ('rotmats', 'tvecs', 'K')]
    edges = torch.from_numpy(g['edges']).to(cuda)
    d0, dd, D = g['depth_cfg']
    img_size, ps = tuple(int(x) for x in g['img_size']), tuple(int(x) for x in g['plane_size'])
    nbytes = lib.v3d_psv_workspace_bytes(*[int(x) for x in (feat.shape[0], feat.shape[1], feat.shape[2], feat.shape[3])])

    class Ws:
        def __init__(self, fill):
            self.buf = torch.full((nbytes + 4096,), fill, dtype=torch.uint8, device=cuda)

        def get(self, name_, n, device):
            assert n <= self.buf.numel()
            return self.buf

    for split in (False, True):
        out = []
        for fill in (0, 255):
            v = mvs.plane_sweep_variance(feat, cams[0], cams[1], cams[2], edges, float(d0), float(dd), int(D), img_size, ps,
                                         workspace=Ws(fill), split=split)
            out.append(v.data if split else v)
        dec = _decode_split(mvs.SplitVariance(out[1], out[1].shape)) if split else out[1]
        assert torch.isfinite(dec).all()
        assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))
