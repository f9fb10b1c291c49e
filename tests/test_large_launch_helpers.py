"""CPU: the helpers of tests/test_large_launch_gpu.py on tiny shapes -- where the byte marks fall, the no-aliasing assertion,
the number of views that passes a mark, the tiling of edge lists, and the periodic check itself (it must see one wrong
element in a late period, and poison left in period 0)."""
import pytest
import torch

import test_large_launch_gpu as ll


def test_mark_positions_and_passing():
    # one cfg2 view of the variance volume is 2^18 x 147 bytes
    shape = (231, 32, 96, 56, 56)
    assert ll.view_bytes(shape) == 2 ** 18 * 147
    pos = dict(ll.mark_positions(shape))
    v, rest = divmod(2 ** 31 // 4, 32 * 96 * 56 * 56)
    assert pos['2^31 B'] == (v,) + ll.unravel(rest, shape[1:]) and v == 55
    assert pos['2^33 B'][0] == 222 and ll.passes(shape, 2 ** 33)
    assert not ll.passes((222,) + shape[1:], 2 ** 33)           # ends inside view 222: not a whole view past the mark
    assert dict(ll.mark_positions((7, 96, 56, 56)))['2^31 B'] is None
    # a tiny tensor, by hand: 2 x 3 floats per view, itemsize 1 "byte" marks do not apply; unravel is row-major
    assert ll.unravel(7, (2, 2, 3)) == (1, 0, 1) and ll.numel((2, 2, 3)) == 12


def test_views_to_pass():
    for vb in (4, 2 ** 18 * 147, 1520640, 2621440):
        n = ll.views_to_pass(vb, 2 ** 32)
        assert n % ll.M == 0 and n * vb >= 2 ** 32 + vb and (n - ll.M) * vb < 2 ** 32 + vb
    assert ll.views_to_pass(32 * 128 * 160 * 4, 2 ** 32) == 1645


def test_no_alias_assertion():
    assert ll.assert_no_alias((231, 32, 96, 56, 56)) == 7 * 2 ** 18 * 147
    with pytest.raises(AssertionError):
        ll.assert_no_alias((8, 2, 64), m=4)                     # period 4 x 512 B divides 2^32
    with pytest.raises(AssertionError):
        ll.assert_no_alias((8, 1024), m=1)


def test_tile_edges():
    e = torch.tensor([[4, 4, 5], [3, 4, 6]])
    t = ll.tile_edges(e, 3, 14)
    assert t.shape == (2, 9)
    assert torch.equal(t[:, 3:6], e + 14) and torch.equal(t[:, 6:], e + 28) and torch.equal(t[:, :3], e)
    assert torch.equal(torch.unique(t[0]), torch.tensor([4, 5, 18, 19, 32, 33]))


def test_periodic_check_sees_one_element_and_poison():
    block = torch.arange(2 * 3 * 5, dtype=torch.float32).view(2, 3, 5)
    out = block.repeat(4, 1, 1)
    ll.check_periodic(out, 'tiny', m=2)
    ll.check_block(out, block, 'tiny', m=2)
    bad = out.clone()
    bad[7, 2, 4] = -1.0                                         # period 3, its view 1
    with pytest.raises(AssertionError) as e:
        ll.check_periodic(bad, 'tiny', m=2)
    msg = str(e.value)
    assert 'period 3 differs' in msg and 'view 1 of the period' in msg and 'element %d,' % (7 * 15 + 14) in msg
    assert 'byte offset %d' % (4 * (7 * 15 + 14)) in msg and 'failing by x % 64' in msg
    nan = out.clone()
    nan.view(torch.int32)[:] = -1                               # every period equal, all poison
    with pytest.raises(AssertionError):
        ll.check_periodic(nan, 'tiny', m=2)
    with pytest.raises(AssertionError):
        ll.check_block(bad[6:], block, 'tiny', m=2)
    with pytest.raises(AssertionError):
        ll.assert_views_differ(out[:4])
    ll.assert_views_differ(block)


def test_layer_tables_are_consistent():
    for layer, dims in enumerate(ll.LAYER_IN):
        o = ll.layer_out_shape(layer, dims)
        big = max(ll.CIN[layer] * ll.numel(dims), ll.COUT[layer] * ll.numel(o)) * 4
        assert 1.5e6 < big < 3e6, (layer, big)
        n = ll.views_to_pass(big, 2 ** 32)
        ll.assert_no_alias((n, 1, big // 4))
    assert ll.layer_out_shape(1, (18, 44, 60)) == (9, 22, 30) and ll.layer_out_shape(7, (7, 15, 19)) == (14, 30, 38)
