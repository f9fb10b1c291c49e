"""Every element of the scene path and of the backbone at production size, against float64 references.

tests/test_full_occupancy_gpu.py does this for the regulariser and stage 3.  The same class of kernel -- matrix instructions,
self-written LDS tables, hand-placed waits -- carries everything else, and until now the suite compared those kernels with a
reference only on scenes that occupy a fraction of the machine (and with each other at larger sizes).  Here the 64-view cfg3
scene of test_full_size_scene_properties_cfg3 (seed 5, two batch elements, 4 cm voxels: 200 704 points, > 50 000 / 15 000 /
2 600 voxel rows) and the 71-image backbone step run stage by stage, and EVERY output element is compared.

Teacher forcing: each stage is checked alone.  Its float64 reference is computed from exactly the fp32 tensors the kernel under
test received -- the previous stage's KERNEL output, cast to double -- so neither a voxel-cell flip nor earlier rounding enters.
Both operand precisions of a stage receive the same input (the default route's output of the previous stage), so one reference
serves both.  References are the functions of oracle/scene.py, oracle/pinned.py and oracle/backbone.py on float64 tensors and
float64 state dicts (tests/test_oracle_scene.py exercises that evaluation on the CPU): on the CPU for the scene path, as torch
ops on the device for the backbone; no kernel of this library computes any part of them.

 1. csrc/backproject.hip: B2 and C1 (offset 0.05, n = 3, 64 views in one call): points EQUAL to oracle/pinned.py, variance
    features against the float64 `_variance_over_edges` of the kernel's own points;
 2. voxelisation: integer outputs EQUAL to oracle.scene.voxelize of the kernel's points, centres to 1e-6;
 3. csrc/sparse.hip: coordinate order of the three levels and all seven neighbour tables the convolutions consume (27-offset
    table per level, two stride-2 down maps, two transposed up maps) EQUAL to `_lookup`;
 4. PointNet (gemm_dense.hip + segment.hip) on the 200 704 x 35 input made of 1-2;
 5. single sparse convolutions on the three real coordinate maps, seeded random features (no ReLU zeros to hide a row), through
    the entry the U-Net uses (v3d_sparse_conv_f32): one layer deep, so one wrong row cannot be averaged away by a GroupNorm;
 6. the sparse U-Net from the kernel's PointNet output;
 7. the decoder from the kernel's levels, hypothesis points and variance features: fused kernel in one 64-view call, in
    16-view chunks (bit-identical), the unfused exact-fp32 chain; 320-channel input (no point features) on 16 views;
 8. ten launches of C1, PointNet, U-Net and fused decoder beside fp32 GEMMs on a second stream, each bit-identical to the first;
 9. NativeBackbone on 71 images of 256 x 320 and of 240 x 320, all five pyramid outputs, both precisions; then under load.

A failure reports how many elements fail, the worst one, and where they sit: matrices of rows are handed to `_check` transposed
([channel, row]), so its histograms read "by row % 64" (the place in a row tile) and "by channel"; per-point tensors as
[view, ..., point], backbone maps as [image, channel, y, x].

Bounds.  Split-bf16 routes: the bounds the project already states for the same outputs -- variance 5e-5 absolute, PointNet / U-Net
features 2e-4 of max|ref|, probabilities 2e-4 absolute, offsets 2e-5 m, backbone 8e-5 of each map's range.  Case 5 has no
earlier bound: 4 x 2^-16 x max|ref| (a split operand pair carries 16 mantissa bits: 2^-17 relative per operand, 2^-16 per product
of two; the terms of a row have mixed signs and |out| is well below sum|terms|, so the factor 4 is against max|ref| of the
tensor, fp32 accumulation of K <= 27 x 128 terms included).  Exact-fp32 routes: the existing bound is only the ceiling; the
bound is 4 x max|fp32 oracle - float64 oracle| of the same tensor, evaluated in the test from the REFERENCE alone (kernel and
fp32 oracle are fp32 sums of the same terms in different orders; the factor covers the maximum over 10^6-10^7 elements and the
chunking of the matrix instructions; case 5 takes 8, see F32_MARGIN_CONV).  Split-bf16 operands behind an fp32 route exceed
that (measured: PointNet 4.7 x its bound, single convolutions 1.4-2.6 x, U-Net 6 x) -- except in the unfused decoder, where the
fp32 error of the sharpened softmax itself (1e-5) is larger than what the operands add (0.5-0.7 of the bound).

Largest error measured on MI355X as a fraction of the bound, and for the fp32 routes the fp32-oracle error (of max|ref|, or
absolute where the bound is) the bound was derived from:
                               split-bf16 route      exact-fp32 route (fp32-oracle error -> worst / bound)
  1 variance B2 / C1           0.20 / 0.25           (one route)
  2 voxel centres              0.00                  (one route; integers equal)
  4 PointNet                   0.019                 2.0e-7 of max -> 0.26
  5 conv, stride 1 (3 maps)    0.079  0.072  0.076   2.4e-7 / 2.7e-7 / 2.6e-7 of max -> 0.77 / 0.98 / 0.87 (margin 8)
    conv, stride 2 (2)         0.070  0.072          2.1e-7 / 2.4e-7 -> 0.97 / 0.89
    conv, transposed (2)       0.070  0.068          3.0e-7 / 3.8e-7 -> 0.51 / 0.44
  6 U-Net, stride 4 / 2 / 1    0.10 / 0.15 / 0.17    8.3e-7 / 8.8e-7 / 9.2e-7 of max -> 0.58 / 0.73 / 0.65
  7 decoder, 64 views          prob 0.11, offset 0.17    prob 1.0e-5 -> 0.26, offset 1.3e-6 m -> 0.28
    decoder, 320 ch, 16 views  prob 0.08, offset 0.20    prob 1.2e-5 -> 0.25, offset 2.2e-6 m -> 0.26
  9 backbone 256 x 320, P1-P5  0.61 0.53 0.49 0.56 0.43  2.0 / 1.9 / 1.7 / 1.6 / 1.5 e-6 of range -> 0.30 0.23 0.25 0.24 0.25
    backbone 240 x 320, P1-P5  0.60 0.52 0.53 0.48 0.43  1.8 / 1.7 / 1.7 / 1.6 / 1.4 e-6 of range -> 0.26 0.25 0.24 0.23 0.24
  3, 8 and the chunked decoder are equalities.  The module takes 47 s on an MI355X box (16 CPU threads for the references).
"""
import functools

import pytest
import torch

from conftest import v3d
from helpers import decoder_reference, oracle_levels, state_as
from oracle import backbone as ob
from oracle import pinned as opin
from oracle import scene as osc
from test_full_occupancy_gpu import _check, _under_load

pytestmark = pytest.mark.gpu

N_REF, K_WIN, PLANE = 64, 2, (56, 56)
P = PLANE[0] * PLANE[1]
EDGE_LEN = 0.04
OFFSET, N_OFF = 0.05, 3
N_HYP = 2 * N_OFF + 1
CHUNK_VIEWS = 16                               # eval-3dvnet.py:13, the driver's offset batch size
PRECISIONS = ('split_bf16', 'fp32')
VAR_ATOL = 5e-5
FEAT_RTOL = 2e-4                               # of max|ref|
PROB_ATOL, OFFSET_ATOL = 2e-4, 2e-5
CONV_RTOL = 4 * 2.0 ** -16                     # of max|ref|, see the module docstring
BACKBONE_RTOL = {'split_bf16': 8e-5, 'fp32': 2e-5}     # of each map's range (test_native_backbone_matches_the_oracle)
F32_MARGIN = 4
# Case 5, measured with margin 4 on MI355X: 1 to 395 of 0.3-4 M elements per case outside, worst 1.95 x the bound, spread evenly over
# the 64 rows of a tile and over the channels (the tail of a rounding distribution, no pattern).  The reason: the kernel adds the
# 27 x Ci = 1 728 / 3 456 products of an output into ONE fp32 accumulator chain, the oracle adds 27 BLAS products of Ci terms each
# (several partial sums per product); a chain's rounding error grows with the square root of its length, so the kernel's is
# sqrt(3456 / ~45) ~ 9 times (1728: ~7 times) the oracle's in the worst element although both are exact fp32 -- measured 3.5 to 7.8
# times.  PointNet (K <= 256 per chain) and the U-Net (GroupNorm after every convolution) stay inside 4.  Split-bf16 operands on
# the same tensors are at 0.07 x 2^-14; run behind the fp32 route they leave this bound in all seven cases (1.4 to 2.6 x, 400 to
# 76 000 elements), the exact-fp32 kernel is at 0.44 to 0.98 of it.
F32_MARGIN_CONV = 8
N_IMAGES = 71                                  # the cfg2 step: 64 reference views + 7


def _threads():
    torch.set_num_threads(min(16, torch.get_num_threads()))


def _bound(precision, ref64, ref32, ceiling, what, margin=F32_MARGIN):
    """Absolute bound of one tensor.  split_bf16: the project's bound (`ceiling`).  fp32: `margin` x the error of the fp32
    oracle against the float64 one, never above the ceiling."""
    if precision == 'split_bf16':
        return ceiling
    e32 = float((ref32.double() - ref64).abs().max())
    scale = float(ref64.abs().max())
    print('%s: fp32 oracle vs float64 oracle %.3g absolute = %.3g of max|ref|; bound %.3g, ceiling %.3g'
          % (what, e32, e32 / scale, min(ceiling, margin * e32), ceiling))
    assert e32 > 0, what + ': the fp32 oracle equals the float64 one, no bound can be derived'
    return min(ceiling, margin * e32)


def _rows(x):
    """[rows, channels] -> [channels, rows]: `_check` then reports by row % 64 and by channel."""
    return x.t()


def _per_view(x):
    """[N_REF * P, ...] -> [view, ..., point]."""
    x = x.reshape((N_REF, P) + tuple(x.shape[1:]))
    return x.permute(0, *range(2, x.dim()), 1)


# ---- the scene, stage by stage (every stage computed on first use, once) --------------------------------------------------

class _Scene:
    def __init__(self, cuda):
        _threads()
        self.cuda = cuda
        syn = v3d('synthetic')
        cfg = syn.CONFIGS['cfg3']
        self.img_size = cfg['img_size']
        edges, n_img = syn.make_edges(N_REF, K_WIN, K_WIN)
        rot, tv, K = syn.make_cameras(n_img, cfg['img_size'], seed=5, yaw_step_deg=360.0 / n_img)
        feat = syn.make_features(n_img, 32, *cfg['feat_size'], seed=5)
        depth = syn.ray_box_depth(rot[K_WIN:K_WIN + N_REF], tv[K_WIN:K_WIN + N_REF], K[K_WIN:K_WIN + N_REF], cfg['img_size'], PLANE)
        depth = depth + 0.02 * torch.randn(depth.shape, generator=torch.Generator().manual_seed(1))
        dbatch = torch.zeros(N_REF, dtype=torch.long)
        dbatch[N_REF // 2:] = 1
        self.cpu = dict(depth=depth, dbatch=dbatch, feat=feat, rot=rot, tv=tv, K=K, edges=edges)
        self.dev = {k: v.to(cuda) for k, v in self.cpu.items()}
        self.sd = dict(pn=syn.pointnet_weights(), un=syn.sparse_unet_weights(), dec=syn.decoder_weights(sharpen=50.0),
                       dec320=syn.decoder_weights(in_dim=320, h_dim=128, seed=4, sharpen=50.0))
        self.vals = torch.linspace(-N_OFF * OFFSET, N_OFF * OFFSET, N_HYP).to(cuda)

    @functools.cached_property
    def nets(self):
        lm = v3d('lightningmodel')
        out = {}
        for pr in PRECISIONS:
            net = lm.PL3DVNet(None, {'size': PLANE}, EDGE_LEN, feat_dim=32, img_size=self.img_size, precision=pr).eval()
            net.pointnet.load_state_dict(self.sd['pn'])
            net.sparse_conv.load_state_dict(self.sd['un'])
            net.decoder.load_state_dict(self.sd['dec'], strict=False)
            out[pr] = net.to(self.cuda)
        return out

    @functools.cached_property
    def decoders320(self):
        rf = v3d('refinement')
        out = {}
        for pr in PRECISIONS:
            dec = rf.HypothesisDecoder(320, 128, 3, 1, precision=pr).eval()
            dec.load_state_dict(self.sd['dec320'], strict=False)
            out[pr] = dec.to(self.cuda)
        return out

    # -- kernels ------------------------------------------------------------------------------------------------------------
    def backproject(self, offset, n):
        d = self.dev
        with torch.no_grad():
            return v3d('lightningmodel').backproject_variance(d['depth'], d['feat'], d['rot'], d['tv'], d['K'], d['edges'],
                                                              self.img_size, offset=offset, n=n)

    @functools.cached_property
    def b2(self):
        """(pts [Np, 3], var [Np, 32], pts_batch [Np]) as PL3DVNet.construct_feature_rich_pointcloud returns them."""
        d = self.dev
        with torch.no_grad():
            out = self.nets['split_bf16'].construct_feature_rich_pointcloud(d['depth'], d['dbatch'], d['feat'], d['rot'], d['tv'],
                                                                             d['K'], d['edges'])
        assert out[0].shape == (200704, 3) and out[0].shape[0] == N_REF * P
        return out

    @functools.cached_property
    def c1(self):
        return self.backproject(OFFSET, N_OFF)

    @functools.cached_property
    def vox(self):
        pts, _, pb = self.b2
        out = v3d('utils').voxelize(pts, pb, EDGE_LEN)
        assert out[0].shape[0] > 50000, 'the scene is supposed to fill the machine: %d stride-1 rows' % out[0].shape[0]
        return out

    @functools.cached_property
    def pn_in(self):
        """The PointNet input as PL3DVNet.model_scene builds it (v3d_pointnet_input_f32) from the kernel outputs of 1-2."""
        libm = v3d('_lib')
        pts, var, _ = self.b2
        a_pts, _, _, a_edges = self.vox
        e0, e1 = a_edges[0].contiguous(), a_edges[1].contiguous()
        pts_c, anc_c, var_c = pts.contiguous(), a_pts.contiguous(), var.contiguous()
        x = torch.empty((e0.shape[0], 3 + var_c.shape[1]), dtype=torch.float32, device=self.cuda)
        libm.check(libm.load().v3d_pointnet_input_f32(libm.ptr(pts_c), libm.ptr(anc_c), libm.ptr(var_c), libm.ptr(e0), libm.ptr(e1),
                                                      e0.shape[0], var_c.shape[1], libm.ptr(x), libm.stream_ptr(self.cuda)),
                   'v3d_pointnet_input_f32')
        assert x.shape == (200704, 35)
        # plain fp32 differences and copies: the same bits as the reference's five torch ops (lightningmodel.py:180-183)
        assert torch.equal(x, torch.cat((pts[e1] - a_pts[e0], var[e1]), dim=1))
        return x

    def pointnet(self, precision):
        a_pts, _, _, a_edges = self.vox
        with torch.no_grad():
            return self.nets[precision].pointnet(self.pn_in, a_edges[0], a_pts.shape[0])

    @functools.cached_property
    def pn_out(self):
        """The default route's PointNet output: the U-Net input of both precisions."""
        return self.pointnet('split_bf16')

    def unet(self, precision):
        a_pts, a_idx, a_batch, _ = self.vox
        with torch.no_grad():
            return self.nets[precision].sparse_conv(self.pn_out, a_pts, a_idx, a_batch, EDGE_LEN, idx_min_zero=True)

    @functools.cached_property
    def xs(self):
        """The default route's levels (coarse -> fine): the decoder input of both precisions."""
        return self.unet('split_bf16')

    @functools.cached_property
    def pts_batch(self):
        return self.dev['dbatch'].unsqueeze(1).expand(N_REF, P).reshape(-1)

    @functools.cached_property
    def levels(self):
        """The three coordinate maps as SparseUNet.forward builds them, fine -> coarse."""
        sm = v3d('scenemodeling')
        _, a_idx, a_batch, _ = self.vox
        coords = torch.cat((a_batch.unsqueeze(1), a_idx), dim=1).int().contiguous()
        lv = [sm.SparseLevel(coords, 1).check()]
        for _ in range(2):
            lv.append(sm.SparseLevel(sm.SparseUNet._strided_coords(lv[-1]), 2 * lv[-1].stride).check())
        return lv

    # -- references ---------------------------------------------------------------------------------------------------------
    @functools.cached_property
    def ref_coords(self):
        """The oracle's coordinate maps, fine -> coarse, from the kernel's voxelisation (shown equal to the oracle's in 2)."""
        _, a_idx, a_batch, _ = self.vox
        c = [torch.cat((a_batch.cpu().unsqueeze(1).long(), a_idx.cpu().long()), dim=1)]
        for ts in (1, 2):
            c.append(osc.strided_coords(c[-1], ts))
        return c

    def variance_ref(self, pts):
        """float64 `_variance_over_edges` of the kernel's own points [Np, H, 3] -> [Np, H, C], 8 views at a time."""
        c = self.cpu
        H = pts.shape[1]
        pts64 = pts.cpu().double().view(N_REF, P, H, 3).permute(0, 3, 2, 1).reshape(N_REF, 3, H * P)
        feat64, rot64, tv64, K64 = (c[k].double() for k in ('feat', 'rot', 'tv', 'K'))
        out = []
        for r0 in range(0, N_REF, 8):
            e = osc.slice_edges(c['edges'], r0 + K_WIN, r0 + 8 + K_WIN, 0)
            xv = osc._variance_over_edges(feat64, pts64[r0:r0 + 8], rot64, tv64, K64, e, e[0] - (r0 + K_WIN), self.img_size)
            assert xv.dtype == torch.float64
            out.append(xv.view(8, -1, H, P).permute(0, 3, 2, 1).reshape(8 * P, H, -1))
        return torch.cat(out)

    @functools.cached_property
    def pn_ref(self):
        a_pts, _, _, a_edges = self.vox
        x, idx, n = self.pn_in.cpu(), a_edges[0].cpu(), a_pts.shape[0]
        r64 = osc.pointnet(x.double(), idx, n, state_as(self.sd['pn'], torch.float64))
        assert r64.dtype == torch.float64
        return r64, osc.pointnet(x, idx, n, self.sd['pn'])

    @functools.cached_property
    def unet_ref(self):
        a_pts, a_idx, a_batch, _ = (v.cpu() for v in self.vox)
        x = self.pn_out.cpu()
        r64 = osc.sparse_unet(x.double(), a_pts, a_idx, a_batch, EDGE_LEN, state_as(self.sd['un'], torch.float64))
        assert all(r['feats'].dtype == torch.float64 for r in r64)
        return r64, osc.sparse_unet(x, a_pts, a_idx, a_batch, EDGE_LEN, self.sd['un'])

    def decoder_ref(self, name, n_views, with_feat):
        """(probabilities float64, probabilities of the fp32 oracle) of the first n_views views from the kernel's levels,
        hypothesis points and variance features."""
        n = n_views * P
        pts, var = self.c1
        pts, var, pb = pts[:n].cpu(), var[:n].cpu() if with_feat else None, self.pts_batch[:n].cpu()
        x32, x64 = oracle_levels(self.xs, torch.float32), oracle_levels(self.xs, torch.float64)
        for x, o in zip(self.xs, x32):
            # the decoder kernels take the level's minimum point from the U-Net ('_min_pts'); the oracle reduces the voxel centres
            assert torch.equal(osc._scatter_min(o['pts'], o['batch'], int(o['batch'].max()) + 1), x['_min_pts'].cpu())
        p64 = decoder_reference(x64, pts.double(), None if var is None else var.double(), pb, state_as(self.sd[name], torch.float64))
        assert p64.dtype == torch.float64
        return p64, decoder_reference(x32, pts, var, pb, self.sd[name])

    @functools.cached_property
    def dec_ref(self):
        return self.decoder_ref('dec', N_REF, True)

    @functools.cached_property
    def dec320_ref(self):
        return self.decoder_ref('dec320', CHUNK_VIEWS, False)


@pytest.fixture(scope='module')
def scene(cuda):
    return _Scene(cuda)


# ---- 1. back-projection + variance ------------------------------------------------------------------------------------------

def test_backprojection_points_equal_pinned_oracle_and_variance_every_element(scene, cuda):
    c = scene.cpu
    ref_idx = torch.unique(c['edges'][0])
    cams = (c['K'][ref_idx], c['rot'][ref_idx], c['tv'][ref_idx])
    pts, var, _ = scene.b2
    want = opin.backproject_points(*cams, c['depth'], scene.img_size).transpose(2, 1).reshape(-1, 3)
    assert torch.equal(pts.cpu(), want), 'B2: %d point coordinates differ from oracle/pinned.py' % int((pts.cpu() != want).sum())
    _check(_per_view(var), _per_view(scene.variance_ref(pts.unsqueeze(1))[:, 0]).to(cuda), VAR_ATOL, 'B2 variance [view, ch, point]')
    hyp, hvar = scene.c1
    assert hyp.shape == (N_REF * P, N_HYP, 3) and hvar.shape == (N_REF * P, N_HYP, 32)
    want = torch.stack([opin.backproject_points(*cams, c['depth'] + i * OFFSET, scene.img_size) for i in range(-N_OFF, N_OFF + 1)], dim=2)
    want = want.permute(0, 3, 2, 1).reshape(N_REF * P, N_HYP, 3)                  # oracle.scene.pointflow_hypotheses
    assert torch.equal(hyp.cpu(), want), 'C1: %d point coordinates differ from oracle/pinned.py' % int((hyp.cpu() != want).sum())
    ref = scene.variance_ref(hyp)
    assert float(ref.abs().max()) > 1e-3
    _check(_per_view(hvar), _per_view(ref).to(cuda), VAR_ATOL, 'C1 variance [view, hyp, ch, point]')


# ---- 2. voxelisation --------------------------------------------------------------------------------------------------------

def test_voxelisation_equals_the_oracle_on_the_kernels_points(scene, cuda):
    pts, _, pb = scene.b2
    a_pts, a_idx, a_batch, a_edges = scene.vox
    r_pts, r_idx, r_batch, r_edges = osc.voxelize(pts.cpu(), pb.cpu(), EDGE_LEN)
    assert a_pts.shape[0] == r_pts.shape[0], (a_pts.shape[0], r_pts.shape[0])
    assert torch.equal(a_idx.cpu().to(r_idx.dtype), r_idx), 'anchor_idx3d'
    assert torch.equal(a_batch.cpu().to(r_batch.dtype), r_batch), 'anchor_batch'
    assert torch.equal(a_edges.cpu().to(r_edges.dtype), r_edges), 'anchor_pts_edges'
    assert set(r_batch.unique().tolist()) == {0, 1}
    _check(_rows(a_pts), _rows(r_pts.double()).to(cuda), 1e-6, 'anchor_pts [axis, row]')


# ---- 3. neighbour tables ----------------------------------------------------------------------------------------------------

def _ref_table(in_coords, out_coords, step):
    """[27, n_out]: row of out_coords[p] + step * o_k in in_coords, or -1 (oracle.scene.sparse_conv / sparse_conv_transpose)."""
    rows = []
    for o in osc.kernel_offsets():
        q = out_coords.clone()
        q[:, 1:] += o * step
        rows.append(osc._lookup(in_coords, q))
    return torch.stack(rows)


# (name, input level, output level, sign): levels fine -> coarse; the step is sign * stride of the FINER of the two maps
TABLES = [('stride-1 table, level %d' % i, i, i, 1) for i in range(3)] + \
         [('down map %d -> %d' % (i, i + 1), i, i + 1, 1) for i in range(2)] + \
         [('up map %d -> %d' % (i + 1, i), i + 1, i, -1) for i in range(2)]


def test_neighbour_tables_of_all_levels_equal_the_oracle_lookup(scene):
    levels, rc = scene.levels, scene.ref_coords
    assert [lv.stride for lv in levels] == [1, 2, 4]
    for lv, c in zip(levels, rc):
        assert torch.equal(lv.coords.cpu().long(), c), 'coordinate order of the stride-%d level' % lv.stride
    assert levels[0].n > 50000 and levels[0].n > levels[1].n > levels[2].n > 1000
    for name, i, o, sign in TABLES:
        step = sign * levels[min(i, o)].stride
        nbr = levels[i].neighbors(levels[o].coords, step).cpu().long()
        ref = _ref_table(rc[i], rc[o], step)
        bad = nbr != ref
        assert not bool(bad.any()), '%s: %d of %d entries differ; by offset: %s' \
            % (name, int(bad.sum()), bad.numel(), {k: int(n) for k, n in enumerate(bad.sum(1).tolist()) if n})
        if i == o:
            assert torch.equal(nbr[13], torch.arange(levels[i].n)), name + ': the centre offset maps a row to itself'
        assert bool((ref >= 0).any(dim=0).all()), name + ': an output row without any neighbour (itself, a child or its parent)'


# ---- 4. PointNet ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', PRECISIONS)
def test_pointnet_every_element(precision, scene, cuda):
    out = scene.pointnet(precision)
    r64, r32 = scene.pn_ref
    assert out.shape == r64.shape and out.shape[0] > 50000 and out.shape[1] == 64
    scale = float(r64.abs().max())
    assert scale > 1e-3
    bound = _bound(precision, r64, r32, FEAT_RTOL * scale, 'PointNet')
    _check(_rows(out), _rows(r64).to(cuda), bound, 'PointNet %s [channel, row]' % precision)


# ---- 5. single sparse convolutions -------------------------------------------------------------------------------------------

# (kind, input level, output level, Ci, Co): the shapes of SparseUNet's res / down / up convolutions on the real maps
CONVS = [('same', 0, 0, 64, 64), ('same', 1, 1, 128, 128), ('same', 2, 2, 128, 128), ('down', 0, 1, 64, 128), ('down', 1, 2, 128, 128),
         ('up', 2, 1, 128, 128), ('up', 1, 0, 128, 64)]


@pytest.mark.parametrize('case', CONVS, ids=['%s_L%d_L%d_%d_%d' % c for c in CONVS])
def test_single_sparse_convolution_every_element(case, scene, cuda):
    """One convolution, no norm, no ReLU, through v3d_sparse_conv_f32 (what SparseUNet._conv calls) with the neighbour table of
    SparseLevel.neighbors, against oracle.scene.sparse_conv / sparse_conv_transpose in float64."""
    kind, i, o, ci, co = case
    sm, libm = v3d('scenemodeling'), v3d('_lib')
    levels, rc = scene.levels, scene.ref_coords
    g = torch.Generator().manual_seed(100 * i + 10 * o + ci)
    kernel = torch.randn((27, ci, co), generator=g) / (27 * ci) ** 0.5
    x = torch.randn((levels[i].n, ci), generator=g)
    ts = levels[i].stride
    if kind == 'up':
        ref = lambda f, w: osc.sparse_conv_transpose(rc[i], f, ts, w, rc[o])[0]
        step = -levels[o].stride
    else:
        ref = lambda f, w: osc.sparse_conv(rc[i], f, ts, w, 1 if kind == 'same' else 2)[1]
        step = ts
    r64, r32 = ref(x.double(), kernel.double()), ref(x, kernel)
    assert r64.dtype == torch.float64 and r64.shape == (levels[o].n, co)
    # not vacuous: a reference row is all zero only where the row has no neighbour at all, and few rows are like that
    none = (_ref_table(rc[i], rc[o], step) < 0).all(dim=0)
    assert int(none.sum()) < 0.05 * levels[o].n and not bool(((r64 == 0).all(dim=1) & ~none).any())
    scale = float(r64.abs().max())
    nbr = levels[i].neighbors(levels[o].coords, step)
    pack = sm.PackedGemm(kernel, ci * co, 1, co, 27, co, ci)
    xd = x.to(cuda).contiguous()
    for pr in PRECISIONS:
        y = torch.empty((levels[o].n, co), dtype=torch.float32, device=cuda)
        libm.check(libm.load().v3d_sparse_conv_f32(pack.handle, levels[o].n, xd.data_ptr(), ci, nbr.data_ptr(), nbr.shape[1], 0, 1e-5,
                                                   None, 0, 0, y.data_ptr(), co, libm.precision_code(pr), libm.stream_ptr(cuda)),
                   'v3d_sparse_conv_f32')
        torch.cuda.synchronize()
        what = 'sparse conv %s L%d -> L%d %d -> %d %s [channel, row]' % (kind, i, o, ci, co, pr)
        _check(_rows(y), _rows(r64).to(cuda), _bound(pr, r64, r32, CONV_RTOL * scale, what, margin=F32_MARGIN_CONV), what)


# ---- 6. sparse U-Net --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', PRECISIONS)
def test_sparse_unet_every_element(precision, scene, cuda):
    xs = scene.unet(precision)
    r64, r32 = scene.unet_ref
    assert [x['stride'] for x in xs] == [4, 2, 1] == [r['stride'] for r in r64]
    for x, a, b in zip(xs, r64, r32):
        assert torch.equal(x['sparse'].coords.cpu().long(), a['coords'])
        ref = a['feats']
        scale = float(ref.abs().max())
        zeros = float((ref == 0).double().mean())
        assert scale > 1e-3 and zeros < 0.6, 'stride %d: max|ref| %.3g, %.0f %% exact zeros' % (x['stride'], scale, 100 * zeros)
        what = 'U-Net stride %d %s [channel, row]' % (x['stride'], precision)
        _check(_rows(x['feats']), _rows(ref).to(cuda), _bound(precision, ref, b['feats'], FEAT_RTOL * scale, what), what)


# ---- 7. decoder -------------------------------------------------------------------------------------------------------------

def _offsets(preds64, vals):
    return (preds64 * vals.double().cpu()[None, :]).sum(dim=1)


def _decoder_not_vacuous(p64, off64):
    assert float(off64.abs().max()) > 0.01, 'reference offsets are (nearly) zero'
    assert float((p64.max(dim=1).values > 0.5).double().mean()) > 0.25, 'reference probabilities are not peaked'


def _unfused(dec, xs, pts, var, pb, vals):
    """The 5-launch chain in the driver's 16-view chunks."""
    outs = []
    for s in range(0, pts.shape[0], CHUNK_VIEWS * P):
        e = s + CHUNK_VIEWS * P
        assert not dec.can_fuse(xs, pts[s:e], None if var is None else var[s:e])
        outs.append(dec.decode(dec.features(xs, pts[s:e], None if var is None else var[s:e], pb[s:e]), vals))
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])


def test_fused_decoder_64_views_every_element_and_chunk_invariant(scene, cuda):
    xs, (pts, var), pb, vals = scene.xs, scene.c1, scene.pts_batch, scene.vals
    dec = scene.nets['split_bf16'].decoder
    n_cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    assert pts.shape[0] == 200704 and pts.shape[0] / 32 > 2 * n_cu          # 32 points per tile: more than two tiles per CU
    p64, _ = scene.dec_ref
    off64 = _offsets(p64, vals)
    _decoder_not_vacuous(p64, off64)
    with torch.no_grad():
        assert dec.can_fuse(xs, pts, var)
        p, e = dec.decode_fused(xs, pts, var, pb, vals)
        parts = [dec.decode_fused(xs, pts[s:s + CHUNK_VIEWS * P], var[s:s + CHUNK_VIEWS * P], pb[s:s + CHUNK_VIEWS * P], vals)
                 for s in range(0, pts.shape[0], CHUNK_VIEWS * P)]
    torch.cuda.synchronize()
    _check(_per_view(p), _per_view(p64).to(cuda), PROB_ATOL, 'fused decoder probabilities [view, hyp, point]')
    _check(_per_view(e), _per_view(off64).to(cuda), OFFSET_ATOL, 'fused decoder offsets [view, point]')
    assert torch.equal(torch.cat([q[0] for q in parts]), p) and torch.equal(torch.cat([q[1] for q in parts]), e), \
        '16-view chunks differ from the 64-view call'


def test_unfused_fp32_decoder_chain_64_views_every_element(scene, cuda):
    xs, (pts, var), pb, vals = scene.xs, scene.c1, scene.pts_batch, scene.vals
    p64, p32 = scene.dec_ref
    off64 = _offsets(p64, vals)
    _decoder_not_vacuous(p64, off64)
    with torch.no_grad():
        p, e = _unfused(scene.nets['fp32'].decoder, xs, pts, var, pb, vals)
    torch.cuda.synchronize()
    _check(_per_view(p), _per_view(p64).to(cuda), _bound('fp32', p64, p32, PROB_ATOL, 'decoder probabilities'),
           'unfused fp32 decoder probabilities [view, hyp, point]')
    _check(_per_view(e), _per_view(off64).to(cuda), _bound('fp32', off64, _offsets(p32.double(), vals), OFFSET_ATOL, 'decoder offsets'),
           'unfused fp32 decoder offsets [view, point]')


def test_decoder_320_channels_16_views_every_element(scene, cuda):
    """No per-point variance features (`pts_feat=None`, refinement.py:28-41 with 320 input channels): the fused kernel and the
    exact-fp32 chain."""
    n = CHUNK_VIEWS * P
    xs, pts, pb, vals = scene.xs, scene.c1[0][:n], scene.pts_batch[:n], scene.vals
    p64, p32 = scene.dec320_ref
    off64 = _offsets(p64, vals)
    _decoder_not_vacuous(p64, off64)
    view = lambda x: x.reshape((CHUNK_VIEWS, P) + tuple(x.shape[1:])).permute(0, *range(2, x.dim() + 1), 1)
    with torch.no_grad():
        dec = scene.decoders320['split_bf16']
        assert dec.can_fuse(xs, pts, None)
        p, e = dec.decode_fused(xs, pts, None, pb, vals)
        pu, eu = _unfused(scene.decoders320['fp32'], xs, pts, None, pb, vals)
    torch.cuda.synchronize()
    _check(view(p), view(p64).to(cuda), PROB_ATOL, 'fused decoder, 320 channels, probabilities [view, hyp, point]')
    _check(view(e), view(off64).to(cuda), OFFSET_ATOL, 'fused decoder, 320 channels, offsets [view, point]')
    _check(view(pu), view(p64).to(cuda), _bound('fp32', p64, p32, PROB_ATOL, 'decoder probabilities, 320 channels'),
           'unfused fp32 decoder, 320 channels, probabilities [view, hyp, point]')
    _check(view(eu), view(off64).to(cuda), _bound('fp32', off64, _offsets(p32.double(), vals), OFFSET_ATOL, 'decoder offsets, 320 channels'),
           'unfused fp32 decoder, 320 channels, offsets [view, point]')


# ---- 8. determinism under load ----------------------------------------------------------------------------------------------

def _clone(out):
    return tuple(t.clone() for t in out) if isinstance(out, tuple) else out.clone()


def test_backproject_variance_deterministic_under_load(scene, cuda):
    launch = lambda: scene.backproject(OFFSET, N_OFF)
    _under_load(launch, _clone(launch()), 'C1 backproject_variance, 64 views', cuda)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_pointnet_deterministic_under_load(precision, scene, cuda):
    launch = lambda: scene.pointnet(precision)
    _under_load(launch, _clone(launch()), 'PointNet %s' % precision, cuda)


@pytest.mark.parametrize('precision', PRECISIONS)
def test_sparse_unet_deterministic_under_load(precision, scene, cuda):
    launch = lambda: tuple(x['feats'] for x in scene.unet(precision))
    _under_load(launch, _clone(launch()), 'sparse U-Net %s' % precision, cuda)


def test_fused_decoder_64_views_deterministic_under_load(scene, cuda):
    xs, (pts, var), pb, vals = scene.xs, scene.c1, scene.pts_batch, scene.vals
    dec = scene.nets['split_bf16'].decoder

    def launch():
        with torch.no_grad():
            return dec.decode_fused(xs, pts, var, pb, vals)
    _under_load(launch, _clone(launch()), 'fused decoder, 64 views', cuda)


# ---- 9. backbone ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('size', [(256, 320), (240, 320)], ids=['256x320', '240x320'])
def test_backbone_71_images_every_element_then_under_load(size, cuda):
    """NativeBackbone (csrc/irb.hip, fpn.hip, backbone.hip) on the cfg2 step's 71 images: all five pyramid outputs against the
    float64 `shrinker(extractor(...))` of oracle/backbone.py (torch ops on the device, 8 images at a time), both precisions."""
    _threads()
    bb, syn = v3d('backbone'), v3d('synthetic')
    fe, fs = bb.build_backbone(32)
    sd_e, sd_s = syn.backbone_weights(32, seed=6)
    assert not fe.load_state_dict(sd_e, strict=False).unexpected_keys
    fs.load_state_dict(sd_s)
    fe, fs = fe.eval().to(cuda), fs.eval().to(cuda)
    img = syn.make_images(N_IMAGES, size, seed=size[0])
    img_d = img.to(cuda)
    assert img_d.shape == (71, 3) + size
    e64, s64 = state_as(sd_e, torch.float64, cuda), state_as(sd_s, torch.float64, cuda)
    with torch.no_grad():
        parts = [ob.shrinker(s64, ob.extractor(e64, img_d[s:s + 8].double())) for s in range(0, N_IMAGES, 8)]
        r64 = [torch.cat([p[i] for p in parts]) for i in range(5)]
        parts = [ob.backbone_features(sd_e, sd_s, img[s:s + 8]) for s in range(0, N_IMAGES, 8)]
        r32 = [torch.cat([p[i] for p in parts]) for i in range(5)]
    assert all(r.dtype == torch.float64 for r in r64)
    for precision in PRECISIONS:
        nb = bb.NativeBackbone(fe, fs, precision=precision)
        assert nb.why_not(img_d) is None                        # no silent second path is measured
        with torch.no_grad():
            got = nb(img_d)
        torch.cuda.synchronize()
        assert len(got) == 5
        for i, (a, b, c) in enumerate(zip(got, r64, r32)):
            scale = float(b.abs().max())
            assert scale > 1e-3
            what = 'backbone %s P%d at %d x %d [image, channel, y, x]' % ((precision, i + 1) + size)
            _check(a, b, _bound(precision, b.cpu(), c, BACKBONE_RTOL[precision] * scale, what), what)

        def launch():
            with torch.no_grad():
                return nb(img_d)
        _under_load(launch, _clone(got), 'backbone %s at %d x %d' % ((precision,) + size), cuda)
