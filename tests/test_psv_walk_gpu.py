"""Depth walk of the window warp kernel (csrc/psv_window.hip): a wave keeps its 8 pixels for W consecutive 8-plane chunks
(developer option psv_walk; 0 = W chosen from the shape).  Every W must give the bits of W = 1 (the kernel variant without the
walk) and of the reuse kernel.  At these small shapes the shape rule itself gives W = 1, so 'auto' repeats that variant here: the
rule is checked on the host by tests/test_psv_walk.py, and an auto W > 1 runs in the full-size tests of
tests/test_costvolume_gpu.py (cfg2 and cfg5 goldens, batches).

The developer options are process-wide, so every variant writes its volumes in an interpreter of its own
(scripts/psv_walk_dump.py); the dumps are made once per session and shared by the tests."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VAR_ATOL = 5e-7          # vs the pinned oracle, as tests/test_costvolume_gpu.py
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = {'w1': ['--option=psv_walk=1'], 'w2': ['--option=psv_walk=2'], 'w3': ['--option=psv_walk=3'],
            'w5': ['--option=psv_walk=5'], 'auto': [], 'reuse': ['--option=psv_kernel=1']}
PLANES = ((7, 9), (8, 8))
DEPTHS = (6, 13, 24, 40)


@pytest.fixture(scope='module')
def dumps(cuda, tmp_path_factory):
    td = tmp_path_factory.mktemp('psv_walk')
    res = {}
    for name, extra in VARIANTS.items():
        f = str(td / (name + '.npz'))
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'psv_walk_dump.py'), f] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[name] = dict(np.load(f))
    return res


def _cases():
    tags = ['ragged_D%d_%dx%d' % (D, *pl) for D in DEPTHS for pl in PLANES]
    return tags + ['exotic_D13', 'exotic_D40', 'again_D40', 'leak_D40', 'leak_last8']


def test_every_walk_gives_the_bits_of_walk_1_and_of_the_reuse_kernel(dumps):
    base = dumps['w1']
    for tag in _cases():
        for kind in ('f32', 'split', 'cl8'):
            key = '%s_%s' % (tag, kind)
            assert base[key].size > 0, key
            if kind != 'split':
                assert np.isfinite(base[key].view(np.float32)).all(), key
            for name in ('w2', 'w3', 'w5', 'auto'):
                assert np.array_equal(dumps[name][key], base[key]), (name, key)
            if kind != 'cl8':
                assert np.array_equal(dumps['reuse'][key], base[key]), ('reuse', key)
    # the volumes are not trivially empty
    assert float(np.abs(base['ragged_D40_7x9_f32'].view(np.float32)).max()) > 1e-3


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


def _decode_split(raw, n, D, h, w):
    """bytes of [n][4 groups][hi, lo][D][h][w][8 bf16] -> fp32 [n, 32, D, h, w] as hi + lo."""
    r16 = torch.from_numpy(raw.view(np.int16).copy()).view(n, 4, 2, D, h, w, 8)
    f = (r16.to(torch.int32) << 16).view(torch.float32)
    x = f[:, :, 0] + f[:, :, 1]
    return x.permute(0, 1, 5, 2, 3, 4).reshape(n, 32, D, h, w)


@pytest.mark.parametrize('D', [13, 40])
def test_walk_3_against_the_pinned_oracle(D, dumps):
    sys.path.insert(0, os.path.join(ROOT, 'scripts'))
    try:
        import psv_walk_dump as pw
    finally:
        sys.path.pop(0)
    from oracle import pinned
    feat, R, tv, K, edges = pw.ragged_case()
    var_o = pinned.warp_variance(feat, R, tv, K, edges, pw.D0, pw.DD, D, pw.IMG, (7, 9))
    n = var_o.shape[0]
    var = torch.from_numpy(dumps['w3']['ragged_D%d_7x9_f32' % D].view(np.float32).copy()).view(n, 32, D, 7, 9)
    np.testing.assert_allclose(var.numpy(), var_o.numpy(), rtol=0, atol=VAR_ATOL)
    dec = _decode_split(dumps['w3']['ragged_D%d_7x9_split' % D], n, D, 7, 9)
    assert torch.equal(dec, _split_roundtrip(var))


def test_walk_state_does_not_leak_between_chunks(dumps):
    """A view with one edge and one with 10 in one launch, D = 40, W = 5: the planes of the last chunk equal a launch of only that
    chunk (depth range shifted by 32 intervals, D = 8) -- stale accumulators, stale windows or wrong store strides would show."""
    w5 = dumps['w5']
    full = w5['leak_D40_f32'].view(np.float32).reshape(2, 32, 40, 7, 9)
    last = w5['leak_last8_f32'].view(np.float32).reshape(2, 32, 8, 7, 9)
    assert np.array_equal(full[:, :, 32:].view(np.uint32), last.view(np.uint32))
    for kind in ('split', 'cl8'):      # slots [n][4][2][D][h][w][16 bytes]
        f = w5['leak_D40_' + kind].reshape(2, 4, 2, 40, 7, 9, 16)
        l = w5['leak_last8_' + kind].reshape(2, 4, 2, 8, 7, 9, 16)
        assert np.array_equal(f[:, :, :, 32:], l), kind
    assert float(np.abs(last).max()) > 1e-3


def test_two_launches_give_the_same_bits(dumps):
    a = dumps['auto']
    for kind in ('f32', 'split', 'cl8'):
        assert np.array_equal(a['ragged_D40_7x9_' + kind], a['again_D40_' + kind]), kind
