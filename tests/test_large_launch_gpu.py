"""Cost-volume launches past 4 GB and past 2^31 elements, every element.

The cost-volume kernels address memory as a wave-uniform 64-bit part plus a 32-bit lane offset, split block indices with magic
numbers and leave the ranges to host checks.  A truncated offset is silent: a later view is written over an earlier one, or read
from it.  Here every kernel of the cost-volume path runs ONE launch whose tensors pass 2^32 bytes (the warp kernel and the
soft-argmin also 2^33 bytes = 2^31 fp32 elements) by at least one whole view, and every element is checked without a large
reference:

  * the batch is a block of M = 7 distinct views repeated T times along the batch axis (on the device);
  * (1) every period of every output is bit-equal to period 0 (``torch.equal`` per period slice; a failure names the first
    differing period, view and element, its byte offset and that offset modulo 2^32, with the ``x % 64`` / per-view histogram);
  * (2) period 0 is bit-equal to the same call on the 7-view block alone (batch invariance);
  * (3) the 7-view result lies within the bound the existing modules use of a float64 reference built from oracle/*.py on the
    device, a view at a time (the warp kernel: oracle/pinned.py on the host).  No kernel of this library computes a reference.

Every output of a large launch is allocated here, filled with 0xFF bytes (fp32 / bf16 NaN patterns) and handed to the C entry
point directly: the wrappers allocate with ``torch.empty`` and the caching allocator may return the block that still holds the
previous, correct result.  Periods that are bit-equal to a NaN-free period 0 are NaN-free.  A byte offset wrapped at 2^32 lands
2^32 bytes lower; no period of any tensor here divides 2^32 or 2^31 (every period is 7 views), so a wrapped access meets other
data -- asserted per tensor, with the views of the block pairwise different.

Cases (device memory each needs in its docstring; printed with the workspace share from the library's ``*_workspace_bytes``):
  A   warp + variance, 231 views of cfg2 (8.90 GB), three layouts, the developer kernels; A2 the automatic reuse-kernel branch
      (feature stack of 3122 images, bordered copy >= 2^31 B); A3 the refusal at 4 GB of bordered features
  B   the fused regulariser at 231 views, six entry points; B2 the split / cl8 routes at 455 views (conv0's output and conv9's
      skip pass 2^32 B)
  C   every per-layer kernel (fp32 layout, layer 0 in both precisions; split kernels of layers 1..8)
  D   soft-argmin / confidence / probability map on a [7140, 96, 56, 56] volume (8.60 GB)
  E   stage 3 (33-channel net, 128 x 160, 1645 views: 4.31 GB of features), forward and forward_resized, both precisions

Measured on MI355X (309 GB): the module's 46 tests take 31 s, 16 s of them the host-side pinned oracle of the 7-view block; no
skip.  Peak ``torch.cuda.max_memory_allocated`` and the largest error as a fraction of its bound:
  A   10.3 GB (split layout 13.7: the decode of the block), A2 6.5, A3 10.5   variance of the block vs oracle/pinned.py  0.24
  B   17.1 GB    reg: split-bf16 0.26, fp32 reference layout 0.70, cl8 0.43; depth 0.44 / 0.10 / 0.07; prob 0.24 / 0.25
  B2  32.7 GB    as B, bit for bit
  C   5.8 .. 13.4 GB (conv2 / conv4 / conv6 on the split kernels)   fp32 layout 0.016 .. 0.12, split kernels 0.057 .. 0.12
  D   9.6 GB     depth 0.038, confidence of a given depth 0.25, of the own depth 0.22, gather bit-equal
  E   4.7 GB     split-bf16 0.015, fp32 0.10
A scratch build whose soft_argmin_kernel wraps its column base at 2^31 elements (inside the buffer) fails case D: "period 1019
differs from period 0 in 18816 elements" (the six views past the mark).
"""
import contextlib
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import confidence_oracle as conf
from conftest import v3d
from oracle import costvolume as ocv
from test_costvolume_gpu import VAR_ATOL, _decode_split, _split_roundtrip
from test_full_occupancy_gpu import (DEPTH_F32_RTOL, DEPTH_SPLIT_RTOL, PROP_RTOL, REG_F32_ATOL, REG_SPLIT_ATOL, STRIP, _check,
                                     _hist, stage3_reference)

pytestmark = pytest.mark.gpu

M = 7                                   # views of the block every launch repeats
MARKS = (('2^31 B', 2 ** 31), ('2^32 B', 2 ** 32), ('3 x 2^31 B', 3 * 2 ** 31), ('2^33 B', 2 ** 33))
BAD_SHAPE, UNSUPPORTED = -1, -5         # include/v3d.h
# single-layer tolerances of test_costreg_single_layers / test_costreg_single_layers_split_kernels (of max(1, max|ref|)):
# exact-fp32 layers 1e-5 (+ 1e-5 relative), conv0 on split-bf16 operands 4e-5, the split kernels of layers 1..8 4e-5
LAYER_F32_TOL, LAYER_C0_SPLIT_TOL, LAYER_SPLIT_TOL = 1e-5, 4e-5, 4e-5


# ---- helpers without a device (tests/test_large_launch_helpers.py) -----------------------------------------------------------

def numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def unravel(index, shape):
    out = []
    for s in reversed(shape):
        out.append(index % s)
        index //= s
    return tuple(reversed(out))


def view_bytes(shape, itemsize=4):
    return numel(shape[1:]) * itemsize


def mark_positions(shape, itemsize=4):
    """Where the byte marks fall in a contiguous tensor of `shape`: [(name, index tuple | None when the tensor ends before)]."""
    return [(name, unravel(b // itemsize, shape) if b // itemsize < numel(shape) else None) for name, b in MARKS]


def passes(shape, mark, itemsize=4):
    """The tensor passes `mark` bytes by at least one whole view."""
    return numel(shape) * itemsize >= mark + view_bytes(shape, itemsize)


def views_to_pass(one_view_bytes, mark, m=M):
    """The smallest multiple of m views whose tensor passes `mark` bytes by at least one whole view."""
    n = -(-(mark + one_view_bytes) // one_view_bytes)
    return -(-n // m) * m


def assert_no_alias(shape, m=M, itemsize=4):
    """A byte offset wrapped at 2^32 (or a signed one at 2^31) must not land on the same data one or more periods lower."""
    period = m * view_bytes(shape, itemsize)
    assert 2 ** 32 % period != 0 and 2 ** 31 % period != 0, (shape, period)
    return period


def tile_edges(edges, T, n_img):
    """The edge list of T copies of a scene of n_img images: period k refers to images k * n_img .. (k + 1) * n_img - 1."""
    return torch.cat([edges + k * n_img for k in range(T)], dim=1)


def describe(what, shape, mark=None, m=M, itemsize=4):
    """Print where the marks fall in a tensor; assert that its period does not alias and that it passes `mark`."""
    assert shape[0] % m == 0
    period = assert_no_alias(shape, m, itemsize)
    pos = ', '.join('%s: %s' % (name, 'view %d, (c, d, y, x) = %s' % (p[0], p[1:]) if p else 'beyond') for name, p in
                    mark_positions(shape, itemsize))
    print('%s %s: %.2f GB, period %d B; %s' % (what, tuple(shape), numel(shape) * itemsize / 1e9, period, pos))
    if mark is not None:
        assert passes(shape, mark, itemsize), (what, shape, mark)


# ---- device helpers ---------------------------------------------------------------------------------------------------------

def poisoned(shape, cuda):
    """An fp32 output buffer whose every byte is 0xFF (NaN patterns as fp32 and as bf16 pairs)."""
    t = torch.empty(tuple(shape), dtype=torch.float32, device=cuda)
    t.view(torch.int32).fill_(-1)
    return t


def need(cuda, nbytes, what, workspace=0):
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info(cuda)
    print('%s: needs %.1f GB of device memory (workspace %.2f GB of it); %.1f of %.1f GB free'
          % (what, nbytes / 1e9, workspace / 1e9, free / 1e9, total / 1e9))
    if free < nbytes + (2 << 30):
        pytest.skip('%s needs %.1f GB, %.1f GB of device memory are free' % (what, nbytes / 1e9, free / 1e9))
    torch.cuda.reset_peak_memory_stats(cuda)


def done(cuda, what, t0):
    torch.cuda.synchronize()
    print('%s: peak device memory %.2f GB, %.1f s' % (what, torch.cuda.max_memory_allocated(cuda) / 1e9, time.time() - t0))
    torch.cuda.empty_cache()


def bits(t):
    return t.view(torch.int32)


def assert_views_differ(t):
    """The views of the block differ pairwise (a wrapped access inside one period is seen too)."""
    for i in range(t.shape[0]):
        for j in range(i + 1, t.shape[0]):
            assert not torch.equal(bits(t[i]), bits(t[j])), 'views %d and %d of the block are equal' % (i, j)


def check_periodic(out, what, m=M):
    """Every period of `out` [T * m, ...] (fp32 storage) is bit-equal to period 0, over every element; period 0 holds no NaN."""
    b = bits(out)
    first = b[:m]
    for k in range(1, out.shape[0] // m):
        if not torch.equal(b[k * m:(k + 1) * m], first):
            d = b[k * m:(k + 1) * m] != first
            idx = torch.nonzero(d)
            pos = tuple(int(v) for v in idx[0])
            flat = (k * m + pos[0]) * numel(out.shape[1:]) + sum(p * s for p, s in zip(pos[1:], out.stride()[1:]))
            raise AssertionError('%s: period %d differs from period 0 in %d elements; first at view %d of the period, index %s: '
                                 'element %d, byte offset %d = %d mod 2^32; got 0x%08x, period 0 holds 0x%08x\n%s'
                                 % (what, k, int(d.sum()), pos[0], pos[1:], flat, 4 * flat, (4 * flat) % 2 ** 32,
                                    int(b[k * m:(k + 1) * m][pos]) & 0xffffffff, int(first[pos]) & 0xffffffff, _hist(idx, None)))
    assert not torch.isnan(out[:m]).any(), what + ': NaN (poison) in period 0'


def check_block(out, small, what, m=M):
    """Period 0 of the large launch == the same call on the block alone, bit for bit."""
    if not torch.equal(bits(out[:m]), bits(small)):
        d = bits(out[:m]) != bits(small)
        raise AssertionError('%s: period 0 of the large launch differs from the %d-view launch in %d elements\n%s'
                             % (what, m, int(d.sum()), _hist(torch.nonzero(d), None)))


@contextlib.contextmanager
def options(**kw):
    """Developer options of the library (include/v3d.h: v3d_set_option), restored on exit."""
    libm = v3d('_lib')
    old = {k: libm.set_option(k, v) for k, v in kw.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            libm.set_option(k, v)


def stream(cuda):
    return v3d('_lib').stream_ptr(cuda)


# ---- A. warp + variance -------------------------------------------------------------------------------------------------------

PSV_ENTRY = {'reference': 'v3d_psv_variance_f32', 'split': 'v3d_psv_variance_split', 'cl8': 'v3d_psv_variance_cl8'}


def decode_cl8(data, shape):
    n, C, D, h, w = shape
    return data.contiguous().view(n, 4, 2, D, h, w, 4).permute(0, 1, 2, 6, 3, 4, 5).reshape(n, 32, D, h, w)


def psv_raw(layout, feat, cams, edges, inp, out, ws, cuda, n_img=None):
    """The C entry point of the warp kernel on buffers of the caller -> return code."""
    mvs = v3d('mvsnet')
    lib = v3d('_lib').load()
    _, ref_img, edge_ofs, edge_src = mvs.edges_to_csr(edges)
    d0, dd, D = inp['depth']
    h, w = inp['plane_size']
    K, R, t = cams
    return getattr(lib, PSV_ENTRY[layout])(feat.data_ptr(), K.data_ptr(), R.data_ptr(), t.data_ptr(), ref_img.data_ptr(),
                                           edge_ofs.data_ptr(), edge_src.data_ptr(), n_img or feat.shape[0], ref_img.shape[0],
                                           edge_src.shape[0], feat.shape[1], feat.shape[2], feat.shape[3], inp['img_size'][0],
                                           inp['img_size'][1], d0, dd, D, h, w, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                           stream(cuda))


def psv_small(scene, layout):
    """The 7-view launch through the wrapper, under the developer options in force -> the raw fp32-storage tensor."""
    mvs = v3d('mvsnet')
    inp = scene['inp']
    d0, dd, D = inp['depth']
    v = mvs.plane_sweep_variance(scene['feat'], scene['R'], scene['t'], scene['K'], scene['edges'], d0, dd, D, inp['img_size'],
                                 inp['plane_size'], split=layout == 'split', cl8=layout == 'cl8')
    return v if layout == 'reference' else v.data


@pytest.fixture(scope='module')
def scene(cuda):
    """The block: 7 reference views (14 images) of cfg2 on the device, and its variance volume (default kernel)."""
    inp = v3d('synthetic').make_costvolume_inputs('cfg2', n_ref=M)
    assert inp['n_img'] == 14
    s = dict(inp=inp, feat=inp['feat'].to(cuda), K=inp['K'].to(cuda).contiguous(), R=inp['rotmats'].to(cuda).contiguous(),
             t=inp['tvecs'].to(cuda).contiguous(), edges=inp['edges'].to(cuda))
    s['var'] = psv_small(s, 'reference')
    assert_views_differ(s['var'])
    torch.cuda.synchronize()
    return s


def test_block_variance_against_the_pinned_oracle(scene):
    """(3) for case A: the 7-view reference-layout volume within VAR_ATOL of oracle/pinned.py (host, the reference's evaluation
    orders), every element; the split and cl8 layouts hold exactly these numbers (decode helpers of test_costvolume_gpu)."""
    from oracle import pinned
    inp = scene['inp']
    d0, dd, D = inp['depth']
    ref = pinned.warp_variance(inp['feat'], inp['rotmats'], inp['tvecs'], inp['K'], inp['edges'], d0, dd, D, inp['img_size'],
                               inp['plane_size'])
    var = scene['var']
    _check(var, ref.to(var.device).double(), VAR_ATOL, 'variance of the 7-view block vs oracle/pinned.py')
    mvs = v3d('mvsnet')
    assert torch.equal(_decode_split(mvs.SplitVariance(psv_small(scene, 'split'), var.shape)), _split_roundtrip(var))
    assert torch.equal(decode_cl8(psv_small(scene, 'cl8'), var.shape), var)


PSV_CASES = [('reference', {}), ('split', {}), ('cl8', {})] + [(lay, opt) for opt in ({'psv_walk': 1}, {'psv_kernel': 1},
                                                                                       {'psv_kernel': 2})
                                                               for lay in ('reference', 'split')]


@pytest.mark.parametrize('layout,opts', PSV_CASES, ids=['%s%s' % (lay, ''.join('-%s%d' % kv for kv in o.items()))
                                                         for lay, o in PSV_CASES])
def test_A_warp_variance_231_views(layout, opts, scene, cuda):
    """33 periods of the 14-image scene: 462 images, 231 views, a variance volume of 8.90 GB (past 2^33 B = 2^31 elements) in one
    launch.  Needs 9.6 GB: the volume, 0.30 GB of features and the 0.32 GB workspace (peak 10.3 GB with the 7-view launch and the
    comparison's temporaries, 13.7 GB where the split block is decoded)."""
    T = 33
    t0 = time.time()
    inp, lib = scene['inp'], v3d('_lib').load()
    d0, dd, D = inp['depth']
    h, w = inp['plane_size']
    shape = (T * M, 32, D, h, w)
    feat = scene['feat'].repeat(T, 1, 1, 1)
    wsb = lib.v3d_psv_workspace_bytes(feat.shape[0], 32, feat.shape[2], feat.shape[3])
    need(cuda, numel(shape) * 4 + feat.numel() * 4 + wsb, 'A %s %s' % (layout, opts), wsb)
    describe('A variance volume', shape, mark=2 ** 33)
    cams = tuple(scene[k].repeat(T, *([1] * (scene[k].dim() - 1))) for k in ('K', 'R', 't'))
    edges = tile_edges(scene['edges'], T, inp['n_img'])
    out, ws = poisoned(shape, cuda), torch.empty(wsb, dtype=torch.uint8, device=cuda)
    with options(**opts):
        rc = psv_raw(layout, feat, cams, edges, inp, out, ws, cuda)
        v3d('_lib').check(rc, PSV_ENTRY[layout])
        small = psv_small(scene, layout)
    torch.cuda.synchronize()
    what = 'A %s %s' % (layout, opts)
    check_periodic(out, what)
    check_block(out, small, what)
    # the 7-view launch of this layout / kernel holds the numbers of the default reference-layout launch, which
    # test_block_variance_against_the_pinned_oracle holds against the oracle
    var = scene['var']
    if layout == 'reference':
        assert torch.equal(small, var), what
    elif layout == 'split':
        assert torch.equal(_decode_split(v3d('mvsnet').SplitVariance(small, var.shape)), _split_roundtrip(var)), what
    else:
        assert torch.equal(decode_cl8(small, var.shape), var), what
    del out, ws, feat
    done(cuda, what, t0)


def big_stack(scene, n_img, cuda):
    """At least n_img images of 64 x 80 features by tiling the 14-image block; edges of the first and of the last period only."""
    T = -(-n_img // 14)
    feat = scene['feat'].repeat(T, 1, 1, 1)
    cams = tuple(scene[k].repeat(T, *([1] * (scene[k].dim() - 1))) for k in ('K', 'R', 't'))
    edges = torch.cat([scene['edges'], scene['edges'] + 14 * (T - 1)], dim=1)
    return feat, cams, edges


def test_A2_feature_stack_of_2_gb_takes_the_reuse_kernel(scene, cuda):
    """3122 images of 64 x 80 features (2.05 GB; bordered channel-last copy 2.16 GB >= 2^31 B): psv_variance_impl switches to
    the reuse kernel by itself.  References and sources come from the first and the last period only (14 views): both halves
    equal the 14-image launch bit for bit, reference and split layout; the cl8 layout is refused.  Needs 5.3 GB (workspace 2.16; peak 6.5 GB)."""
    t0 = time.time()
    inp, lib = scene['inp'], v3d('_lib').load()
    d0, dd, D = inp['depth']
    h, w = inp['plane_size']
    feat, cams, edges = big_stack(scene, 3115, cuda)      # 223 periods: the whole last period lies past 2^31 B
    n_img, Hf, Wf = feat.shape[0], feat.shape[2], feat.shape[3]
    bordered = n_img * (Hf + 2) * (Wf + 2) * 32 * 4
    assert feat.numel() * 4 < 2 ** 31 <= bordered and (n_img - 14) * (Hf + 2) * (Wf + 2) * 32 * 4 >= 2 ** 31
    wsb = lib.v3d_psv_workspace_bytes(n_img, 32, Hf, Wf)
    shape = (2 * M, 32, D, h, w)
    need(cuda, feat.numel() * 4 + wsb + 2 * numel(shape) * 4, 'A2', wsb)
    print('A2 features %s: %.2f GB, bordered copy %.3f GB = 2^31 B + %d B; the last period starts at byte %d of it'
          % (tuple(feat.shape), feat.numel() * 4 / 1e9, bordered / 1e9, bordered - 2 ** 31, (n_img - 14) * (Hf + 2) * (Wf + 2) * 128))
    assert_no_alias((n_img,) + tuple(feat.shape[1:]), m=14)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    var = scene['var']
    for layout in ('reference', 'split'):
        out = poisoned(shape, cuda)
        v3d('_lib').check(psv_raw(layout, feat, cams, edges, inp, out, ws, cuda), PSV_ENTRY[layout])
        small = psv_small(scene, layout)                              # the window kernel on the 14 images
        torch.cuda.synchronize()
        check_periodic(out, 'A2 ' + layout)
        check_block(out, small, 'A2 ' + layout)
        if layout == 'reference':
            assert torch.equal(small, var)
    out = poisoned(shape, cuda)
    assert psv_raw('cl8', feat, cams, edges, inp, out, ws, cuda) == UNSUPPORTED
    assert b'window kernel' in lib.v3d_last_error()
    torch.cuda.synchronize()
    assert int((bits(out) != -1).sum()) == 0, 'the refused call wrote to its output'
    del out, ws, feat
    done(cuda, 'A2', t0)


def test_A3_bordered_features_of_4_gb_are_refused(scene, cuda):
    """6201 images: the bordered copy would hold 2^32 B or more, beyond the 32-bit byte offsets of the tap words:
    V3D_ERR_BAD_SHAPE.  The buffers have the size the call would need (10.5 GB: 4.06 of features, 4.30 of workspace, a 14-view volume), so that a
    missing check shows as a wrong return code and never as a fault."""
    t0 = time.time()
    inp, lib = scene['inp'], v3d('_lib').load()
    d0, dd, D = inp['depth']
    h, w = inp['plane_size']
    feat, cams, edges = big_stack(scene, 6201, cuda)
    Hf, Wf = feat.shape[2], feat.shape[3]
    assert feat.shape[0] >= 6201 and 6201 * (Hf + 2) * (Wf + 2) * 128 >= 2 ** 32 > 6200 * (Hf + 2) * (Wf + 2) * 128
    wsb = lib.v3d_psv_workspace_bytes(feat.shape[0], 32, Hf, Wf)
    shape = (2 * M, 32, D, h, w)
    need(cuda, feat.numel() * 4 + wsb + numel(shape) * 4, 'A3', wsb)
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    out = poisoned(shape, cuda)
    # the references and sources of the last period lie inside the first 6201 images only up to image 6200: keep the first period
    edges = edges[:, :edges.shape[1] // 2]
    for layout in ('reference', 'split', 'cl8'):
        assert psv_raw(layout, feat, cams, edges, inp, out, ws, cuda, n_img=6201) == BAD_SHAPE, layout
        assert b'4 GB' in lib.v3d_last_error()
    torch.cuda.synchronize()
    assert int((bits(out) != -1).sum()) == 0, 'a refused call wrote to its output'
    del out, ws, feat
    done(cuda, 'A3', t0)


# ---- B. the fused regulariser -------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def regblock(scene, cuda):
    """The 7-view variance block in its three formats, the net, and the float64 CostRegNet + softmax of the fp32 volume."""
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    inp = scene['inp']
    sd = syn.costregnet_weights(sharpen=200.0)
    net = mvs.MVSNet(32, inp['img_size']).eval()
    net.cnn_3d.load_state_dict(sd, strict=False)
    net = net.to(cuda)
    d0, dd, D = inp['depth']
    var = scene['var']
    with torch.no_grad():
        vals = net.depth_values(d0, dd, D, cuda)
        sd64 = {k: v.to(cuda, torch.float64) for k, v in sd.items()}
        ref = torch.cat([ocv.costregnet(var[i:i + 1].double(), sd64).squeeze(1) for i in range(M)])
        depth = (F.softmax(-ref, dim=1) * vals.double().view(1, D, 1, 1)).sum(1)
    torch.cuda.synchronize()
    return dict(net=net, vals=vals, ref=ref, depth=depth, reference=var, split=psv_small(scene, 'split'),
                cl8=psv_small(scene, 'cl8'), shape=tuple(var.shape))


def confidence_check(reg, depth, prob, ds, di, what):
    """prob [n, h, w] against the float64 restatement (tests/confidence_oracle.py) of the confidence of `depth` under
    softmax(-reg): the planes are those of the fp32 chain on that depth (nothing uncertain), the values within RATIO x the error
    of the reference's own fp32 chain (torch's fp32 softmax, then the gather) -- the bound of test_confidence_gpu."""
    x, d = reg.cpu().numpy(), depth.cpu().numpy()
    lr = conf.indices_f32(d, ds, di, x.shape[1])
    want = conf.check(conf.softmax64(x), d, ds, di, indices=lr)['prob']
    p32 = F.softmax(-torch.from_numpy(x), dim=1).numpy()
    ref_err = conf.max_error(conf._take(p32, lr[0]) + conf._take(p32, lr[1]), want)
    err = conf.max_error(prob.cpu().numpy(), want)
    print('%s: device error %.3g, reference fp32 error %.3g: %.3f of the bound' % (what, err, ref_err, err / (conf.RATIO * ref_err)))
    assert err <= conf.RATIO * ref_err, (what, err, ref_err)
    return err / (conf.RATIO * ref_err)


# (entry point, input layout, precision)
COSTREG = [('v3d_costreg_depth_f32', 'reference', 'split_bf16'), ('v3d_costreg_depth_f32', 'reference', 'fp32'),
           ('v3d_costreg_depth_split', 'split', 'split_bf16'), ('v3d_costreg_depth_cl8', 'cl8', 'fp32'),
           ('v3d_costreg_depth_prob', 'split', 'split_bf16'), ('v3d_costreg_depth_prob', 'cl8', 'fp32')]
COSTREG_IDS = ['%s-%s-%s' % (e[12:], lay, pr) for e, lay, pr in COSTREG]


def costreg_raw(entry, layout, precision, rb, x, n, depth, reg, prob, ws, inp, cuda):
    libm = v3d('_lib')
    lib = libm.load()
    handle = rb['net'].cnn_3d.packed_handle(cuda)
    _, _, D, h, w = rb['shape']
    d0, dd, _ = inp['depth']
    vals, s = rb['vals'].data_ptr(), stream(cuda)
    if entry == 'v3d_costreg_depth_prob':
        rc = lib.v3d_costreg_depth_prob(handle, x.data_ptr(), libm.LAYOUT[layout], libm.precision_code(precision), vals, d0, dd,
                                        n, D, h, w, depth.data_ptr(), reg.data_ptr(), prob.data_ptr(), ws.data_ptr(), ws.numel(), s)
    elif entry == 'v3d_costreg_depth_f32':
        rc = lib.v3d_costreg_depth_f32(handle, x.data_ptr(), vals, n, D, h, w, depth.data_ptr(), reg.data_ptr(),
                                       libm.precision_code(precision), ws.data_ptr(), ws.numel(), s)
    else:
        rc = getattr(lib, entry)(handle, x.data_ptr(), vals, n, D, h, w, depth.data_ptr(), reg.data_ptr(), ws.data_ptr(),
                                 ws.numel(), s)
    libm.check(rc, entry)


def run_costreg_case(entry, layout, precision, T, rb, scene, cuda, tag):
    t0 = time.time()
    inp, lib = scene['inp'], v3d('_lib').load()
    _, C, D, h, w = rb['shape']
    n = T * M
    wsb = lib.v3d_costreg_workspace_bytes(rb['net'].cnn_3d.packed_handle(cuda), n, D, h, w)
    what = '%s %s %s %s, %d views' % (tag, entry, layout, precision, n)
    need(cuda, n * C * D * h * w * 4 + wsb + n * (D + 2) * h * w * 4, what, wsb)
    describe(tag + ' variance volume', (n, C, D, h, w), mark=2 ** 32)
    describe(tag + ' conv0 output / conv9 skip (workspace)', (n, 8, D, h, w), mark=2 ** 32 if tag == 'B2' else None)
    describe(tag + ' x_reg', (n, D, h, w))
    prob_out = entry == 'v3d_costreg_depth_prob'
    x7 = rb[layout]
    x = x7.repeat(T, 1, 1, 1, 1)
    depth, reg = poisoned((n, h, w), cuda), poisoned((n, D, h, w), cuda)
    prob = poisoned((n, h, w), cuda) if prob_out else None
    ws = torch.empty(wsb, dtype=torch.uint8, device=cuda)
    costreg_raw(entry, layout, precision, rb, x, n, depth, reg, prob, ws, inp, cuda)
    torch.cuda.synchronize()
    del x, ws
    # the same call on the block alone
    wsb7 = lib.v3d_costreg_workspace_bytes(rb['net'].cnn_3d.packed_handle(cuda), M, D, h, w)
    ws7 = torch.empty(wsb7, dtype=torch.uint8, device=cuda)
    depth7, reg7 = poisoned((M, h, w), cuda), poisoned((M, D, h, w), cuda)
    prob7 = poisoned((M, h, w), cuda) if prob_out else None
    costreg_raw(entry, layout, precision, rb, x7, M, depth7, reg7, prob7, ws7, inp, cuda)
    torch.cuda.synchronize()
    outs = [('depth', depth, depth7), ('reg', reg, reg7)] + ([('prob', prob, prob7)] if prob_out else [])
    for name, big, small in outs:
        check_periodic(big, '%s: %s' % (what, name))
        check_block(big, small, '%s: %s' % (what, name))
    assert_views_differ(reg7)
    ref = rb['ref']
    f32 = precision == 'fp32'
    _check(reg7, ref, (REG_F32_ATOL if f32 else REG_SPLIT_ATOL) * float(ref.abs().max()), what + ': reg of the block')
    _check(depth7, rb['depth'], (DEPTH_F32_RTOL if f32 else DEPTH_SPLIT_RTOL) * rb['depth'].abs(), what + ': depth of the block')
    if prob_out:
        confidence_check(reg7, depth7, prob7, inp['depth'][0], inp['depth'][1], what + ': prob of the block')
    del depth, reg, prob
    done(cuda, what, t0)


@pytest.mark.parametrize('entry,layout,precision', COSTREG, ids=COSTREG_IDS)
def test_B_regulariser_231_views(entry, layout, precision, regblock, scene, cuda):
    """The 8.90 GB volume of case A through every depth entry point, `reg` asked for: depth, reg (and prob) periodic, the block
    against the float64 CostRegNet + softmax.  Needs 17.1 GB: the volume, 6.89 GB of workspace (24.75 D h w floats per view and
    one view's split copy), 0.28 GB of x_reg."""
    run_costreg_case(entry, layout, precision, 33, regblock, scene, cuda, 'B')


@pytest.mark.parametrize('entry,layout,precision', [c for c in COSTREG if c[1] != 'reference'],
                         ids=[i for i, c in zip(COSTREG_IDS, COSTREG) if c[1] != 'reference'])
def test_B2_regulariser_455_views(entry, layout, precision, regblock, scene, cuda):
    """65 periods: conv0's output and conv9's skip input (8 x 96 x 56 x 56 x 4 B per view) pass 2^32 B at view 446 -- the only
    way to take conv0z, the conv12z march and conv9_prob past the mark.  Needs 32.7 GB: 17.53 of variance, 13.55 of workspace."""
    run_costreg_case(entry, layout, precision, 65, regblock, scene, cuda, 'B2')


# ---- C. the per-layer kernels -------------------------------------------------------------------------------------------------

CIN = [32, 8, 16, 16, 32, 32, 64, 64, 32, 16]
COUT = [8, 16, 16, 32, 32, 64, 64, 32, 16, 8]
# per-view input volume of each layer: 1.7 to 2.9 MB for the larger of input and output, no axis of input or output a multiple
# of the layer's tile (fp32-layout tiles: conv0 4 x 8 x 28, conv1 2 x 4 x 28, conv2 4 x 4 x 28, conv3 2 x 7 x 14, conv4
# 4 x 7 x 14, conv5 / conv6 2 x 4 x 7, outputs of conv7 4 x 8 x 14, of conv8 / conv9 4 x 8 x 28); conv0's width 44 is a
# multiple of 4 (float4 staging); the transposed layers take the half-size volumes of the coarser level their inputs live on
LAYER_IN = [(14, 36, 44), (18, 44, 60), (18, 38, 46), (18, 38, 46), (14, 30, 38), (14, 30, 38), (9, 26, 30), (7, 15, 19),
            (9, 19, 23), (9, 22, 30)]
LAYER_CASES = [(l, False, 'split_bf16') for l in range(10)] + [(0, False, 'fp32')] + [(l, True, 'split_bf16') for l in range(1, 9)]


def layer_out_shape(layer, dims):
    if layer >= 7:
        return tuple(2 * d for d in dims)
    s = 2 if layer in (1, 3, 5) else 1
    return tuple((d - 1) // s + 1 for d in dims)


def layer_raw(net, layer, split, precision, x, skip, out, ws, cuda):
    libm = v3d('_lib')
    lib = libm.load()
    n, _, Di, Hi, Wi = x.shape
    h = net.packed_handle(cuda)
    sk = None if skip is None else skip.data_ptr()
    if split:
        rc = lib.v3d_costreg_layer_split_f32(h, layer, x.data_ptr(), sk, n, Di, Hi, Wi, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                             stream(cuda))
    else:
        rc = lib.v3d_costreg_layer_f32(h, layer, x.data_ptr(), sk, n, Di, Hi, Wi, out.data_ptr(), libm.precision_code(precision),
                                       stream(cuda))
    libm.check(rc, 'v3d_costreg_layer%s_f32' % ('_split' if split else ''))


@pytest.fixture(scope='module')
def layernet(cuda):
    syn, mvs = v3d('synthetic'), v3d('mvsnet')
    sd = syn.costregnet_weights(seed=5)
    net = mvs.CostRegNet(32, 8).eval()
    net.load_state_dict(sd, strict=False)
    return net.to(cuda), {k: v.to(cuda, torch.float64) for k, v in sd.items()}


@pytest.mark.parametrize('layer,split,precision', LAYER_CASES,
                         ids=['conv%d-%s' % (l, 'split_kernel' if s else 'fp32_layout-' + p) for l, s, p in LAYER_CASES])
def test_C_single_layer_past_4_gb(layer, split, precision, layernet, cuda):
    """One layer kernel on as many periods of a 7-view block as take the larger of its input and output past 2^32 B by a view
    (skip tensors of conv7..conv9 tiled too).  Needs the input, the output, the skip and, for the split kernels, the split copy
    of the input: 5.4 GB (stride-2 layers) to 13.4 GB (conv2 / conv4 / conv6 on the split kernels: input, output and split copy of
    4.3 GB each)."""
    t0 = time.time()
    net, sd64 = layernet
    lib = v3d('_lib').load()
    dims = LAYER_IN[layer]
    odims = layer_out_shape(layer, dims)
    cin, cout = CIN[layer], COUT[layer]
    vb = max(cin * numel(dims), cout * numel(odims)) * 4
    n = views_to_pass(vb, 2 ** 32)
    T = n // M
    in_shape, out_shape = (n, cin) + dims, (n, cout) + odims
    wsb = lib.v3d_costreg_layer_split_workspace_bytes(n, cin, *dims) if split else 0
    what = 'C conv%d %s' % (layer, 'split kernel' if split else 'fp32 layout, ' + precision)
    need(cuda, (numel(in_shape) + numel(out_shape) * (2 if layer >= 7 else 1)) * 4 + wsb, what, wsb)
    describe(what + ' input', in_shape, mark=2 ** 32 if cin * numel(dims) * 4 == vb else None)
    describe(what + ' output', out_shape, mark=2 ** 32 if cout * numel(odims) * 4 == vb else None)
    g = torch.Generator(device=cuda).manual_seed(100 * layer + split)
    x7 = torch.randn((M, cin) + dims, generator=g, device=cuda)
    skip7 = torch.randn((M, cout) + odims, generator=g, device=cuda) if layer >= 7 else None
    assert_views_differ(x7)
    name = 'conv%d' % layer
    with torch.no_grad():
        if layer < 7:
            ref = torch.cat([ocv.conv_bn_relu3d(x7[i:i + 1].double(), sd64, name, stride=2 if layer in (1, 3, 5) else 1)
                             for i in range(M)])
        else:
            ref = torch.cat([skip7[i:i + 1].double() + ocv.deconv_bn_relu3d(x7[i:i + 1].double(), sd64, name) for i in range(M)])
    x = x7.repeat(T, 1, 1, 1, 1)
    skip = None if skip7 is None else skip7.repeat(T, 1, 1, 1, 1)
    out = poisoned(out_shape, cuda)
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=cuda)
    layer_raw(net, layer, split, precision, x, skip, out, ws, cuda)
    torch.cuda.synchronize()
    del x, skip, ws
    out7 = poisoned((M, cout) + odims, cuda)
    ws7 = torch.empty(max(lib.v3d_costreg_layer_split_workspace_bytes(M, cin, *dims), 256), dtype=torch.uint8, device=cuda)
    layer_raw(net, layer, split, precision, x7, skip7, out7, ws7, cuda)
    torch.cuda.synchronize()
    check_periodic(out, what)
    check_block(out, out7, what)
    scale = max(1.0, float(ref.abs().max()))
    if split:
        bound = LAYER_SPLIT_TOL * scale
    elif layer == 0 and precision == 'split_bf16':
        bound = LAYER_C0_SPLIT_TOL * scale
    else:
        bound = LAYER_F32_TOL * scale + 1e-5 * ref.abs()
    _check(out7, ref, bound, what + ': the block vs the float64 torch layer')
    del out
    done(cuda, what, t0)


# ---- D. soft-argmin and confidence alone ---------------------------------------------------------------------------------------

def test_D_soft_argmin_and_confidence_7140_views(cuda):
    """A one-channel [7140, 96, 56, 56] volume of logits (1020 periods, 8.60 GB, past 2^33 B): v3d_soft_argmin_f32 without and
    with the confidence, v3d_confidence_logits_f32 and v3d_probability_map_f32 on a given depth map.  Needs 9.6 GB."""
    t0 = time.time()
    libm = v3d('_lib')
    lib = libm.load()
    T, D, h, w = 1020, 96, 56, 56
    n = T * M
    ds, di = 0.5, 0.05
    need(cuda, n * (D + 5) * h * w * 4, 'D')
    describe('D volume', (n, D, h, w), mark=2 ** 33)
    describe('D depth / prob maps', (n, h, w))
    x7n = conf.logits((M, D, h, w), 1.0, 21)
    given7n = conf.special_depths(ds, di, D, M * h * w, 22).reshape(M, h, w)
    vals_n = conf.plane_depths(ds, di, D)
    x7, given7, vals = (torch.from_numpy(a).to(cuda) for a in (x7n, given7n, vals_n))
    assert_views_differ(x7)
    x, given = x7.repeat(T, 1, 1, 1), given7.repeat(T, 1, 1)
    s = stream(cuda)

    def launch(xv, gv, nv):
        o = {k: poisoned((nv, h, w), cuda) for k in ('depth', 'depth_p', 'prob_own', 'prob_given', 'gather')}
        libm.check(lib.v3d_soft_argmin_f32(xv.data_ptr(), vals.data_ptr(), 0., 0., nv, D, h, w, o['depth'].data_ptr(), None, s),
                   'v3d_soft_argmin_f32')
        libm.check(lib.v3d_soft_argmin_f32(xv.data_ptr(), vals.data_ptr(), ds, di, nv, D, h, w, o['depth_p'].data_ptr(),
                                           o['prob_own'].data_ptr(), s), 'v3d_soft_argmin_f32 (prob)')
        libm.check(lib.v3d_confidence_logits_f32(xv.data_ptr(), gv.data_ptr(), ds, di, nv, D, h, w, o['prob_given'].data_ptr(), s),
                   'v3d_confidence_logits_f32')
        libm.check(lib.v3d_probability_map_f32(xv.data_ptr(), gv.data_ptr(), ds, di, nv, D, h, w, o['gather'].data_ptr(), s),
                   'v3d_probability_map_f32')
        torch.cuda.synchronize()
        return o
    big, small = launch(x, given, n), launch(x7, given7, M)
    del x, given
    for k in big:
        check_periodic(big[k], 'D ' + k)
        check_block(big[k], small[k], 'D ' + k)
    # the block against float64: the expectation (the depth bound of the exact-fp32 chain, which ends with this kernel), the
    # confidence of a given depth and of the kernel's own depth, and the gather (bit for bit against the fp32 restatement)
    p64 = conf.softmax64(x7n)
    depth64 = torch.from_numpy(conf.expectation64(p64, vals_n)).to(cuda)
    assert torch.equal(small['depth'], small['depth_p'])
    _check(small['depth'], depth64, DEPTH_F32_RTOL * depth64.abs(), 'D depth of the block vs the float64 expectation')
    confidence_check(x7, given7, small['prob_given'], ds, di, 'D confidence of a given depth')
    confidence_check(x7, small['depth'], small['prob_own'], ds, di, 'D confidence of the own depth')
    assert np.array_equal(small['gather'].cpu().numpy().view(np.uint32), conf.gather_f32(x7n, given7n, ds, di).view(np.uint32))
    del big
    done(cuda, 'D', t0)


# ---- E. stage 3 -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('precision', ['split_bf16', 'fp32'])
@pytest.mark.parametrize('mode', ['forward', 'resized'])
def test_E_stage3_past_4_gb_of_features(mode, precision, cuda):
    """The 33-channel PropagationNet at 128 x 160 on 1645 views (235 periods): 4.31 GB of features, past 2^32 B by more than a
    view.  ``forward`` (depth [n, 1, 128, 160]) and ``forward_resized`` (depth [n, 64, 80]).  Needs 4.7 GB."""
    t0 = time.time()
    up, libm = v3d('upsampling'), v3d('_lib')
    lib = libm.load()
    cin, H, W = 33, 128, 160
    n = views_to_pass((cin - 1) * H * W * 4, 2 ** 32)
    T = n // M
    assert n == 1645
    what = 'E %s %s' % (mode, precision)
    need(cuda, n * (cin + 1) * H * W * 4, what)
    describe('E features', (n, cin - 1, H, W), mark=2 ** 32)
    describe('E output', (n, H, W))
    sd = v3d('synthetic').propagation_weights(cin, 32, 6)
    g = torch.Generator(device=cuda).manual_seed(33 + (mode == 'resized'))
    guide7 = torch.rand((M, cin - 1, H, W), generator=g, device=cuda)
    h0, w0 = (H, W) if mode == 'forward' else (H // 2, W // 2)
    depth7 = 1 + torch.rand((M, h0, w0), generator=g, device=cuda)
    full7 = depth7 if mode == 'forward' else F.interpolate(depth7.unsqueeze(1), (H, W), mode='nearest')[:, 0]
    assert_views_differ(guide7)
    ref = stage3_reference(sd, guide7, full7, cuda)
    net = up.PropagationNet(cin, 32, precision=precision).eval()
    net.load_state_dict(sd, strict=False)
    net = net.to(cuda)
    tables = (None, None) if mode == 'forward' else tuple(t.data_ptr() for t in up.nearest_tables((h0, w0), (H, W), cuda))

    def launch(gv, dv):
        out = poisoned((gv.shape[0], H, W), cuda)
        rc = lib.v3d_propagation_up_f32(net.packed_handle(cuda), gv.data_ptr(), dv.data_ptr(), gv.shape[0], cin - 1, H, W, h0, w0,
                                        tables[0], tables[1], out.data_ptr(), libm.precision_code(precision), stream(cuda))
        libm.check(rc, 'v3d_propagation_up_f32')
        torch.cuda.synchronize()
        return out
    guide, depth = guide7.repeat(T, 1, 1, 1), depth7.repeat(T, 1, 1)
    out, out7 = launch(guide, depth), launch(guide7, depth7)
    del guide, depth
    check_periodic(out, what)
    check_block(out, out7, what)
    assert float(((out7 - full7).abs() > 1e-3 * full7).double().mean()) > 0.5, what + ': output is (nearly) its input'
    _check(out7, ref, PROP_RTOL[precision] * ref.abs(), what + ': the block vs the float64 PropagationNet', strip=STRIP)
    del out
    done(cuda, what, t0)
