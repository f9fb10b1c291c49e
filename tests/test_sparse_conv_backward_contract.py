"""The workspace and output contract of v3d_sparse_conv_weight_grad_f32 (include/v3d.h) through the C ABI on caller-made buffers, as
a `Case` of the table of tests/workspace_cases.py.

The case lives in that table (`CASE` below is the table's entry), so tests/test_workspace_cases.py and
tests/test_workspace_contract_gpu.py see it however they are run.  The tests below hold the case to the same four properties with that
file's own arena and helpers, so that this file also stands alone:

  CPU   the case's inputs are seeded and built without a device; every launch of the small input has at least two workgroups, the
        last one ragged; big is at least twice small in every buffer section or in every launch; the launch lines and the chunk
        constant the groups restate are on the source lines cited;
  GPU   poison    small on 0x00-filled and on 0xFF-filled buffers and outputs: same bits, no element left unwritten;
        reuse     big, then small in the same workspace: the outputs of buffers of its own;
        canaries  buffers of exactly the bytes the size function returns, 4 KB of a fixed pattern in front and behind: all intact;
        checked   the 0xFF run of the big input meets the checker.
The 0xFF run has to meet tests/sparse_conv_backward_oracle.py at (cnt_k + 32) u S per element, so that an answer that is wrong both
times does not pass as "equal".  The source sits in rows of K + 12 floats, the gradient in rows of N + 8 floats, NaN around them and
in every source row no table entry names.
"""
import os

import numpy as np
import pytest

import sparse_conv_backward_oracle as sco
import workspace_cases as wc
from conftest import ROOT

K, N = wc.WGRAD_K, wc.WGRAD_N
SHAPES = wc.WGRAD_SHAPES                                                   # (rows, side of the two-batch grid): 2 and 4 chunks
CASE = next(c for c in wc.CASES if c.name == 'sparse_conv_weight_grad')
SIZE_FUNCTION = 'v3d_sparse_conv_weight_grad_workspace_bytes'


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_the_table_holds_the_case_and_needs_it():
    assert CASE in wc.CASES and wc.SIZED_BY[SIZE_FUNCTION] == CASE.name and (K, N) == (32, 16)
    assert SHAPES == {'small': (sco.ROWS + 37, 9), 'big': (3 * sco.ROWS + 90, 11)} and wc.WGRAD_ROWS == sco.ROWS
    rest = [c for c in wc.CASES if c is not CASE]
    assert {'v3d_sparse_conv_weight_grad_f32', SIZE_FUNCTION} <= set(wc.missing_entry_points(rest))
    assert not {'v3d_sparse_conv_weight_grad_f32', SIZE_FUNCTION} & set(wc.missing_entry_points(wc.CASES))
    fns = wc.header_functions()
    assert fns['v3d_sparse_conv_weight_grad_f32'][0] == 'src' and fns['v3d_sparse_conv_weight_grad_f32'][-3:] == ['workspace', 'workspace_bytes', 'stream']


def test_inputs_are_seeded_and_built_without_a_device():
    for size in CASE.sizes:
        a, b = CASE.make(size), CASE.make(size)
        for k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (size, k)
        assert np.isnan(a['src'][:, K:]).all() and np.isnan(a['grad_out'][:, N:]).all() and np.isfinite(a['grad_out'][:, :N]).all()
        assert a['M'] == SHAPES[size][0] and sco.chunks(a['M'])[0] == {'small': 2, 'big': 4}[size]


def test_shape_rules():
    _, lib = wc.lib_modules()
    small, big = CASE.make('small'), CASE.make('big')
    for g in CASE.groups(small):
        n, ragged = wc.workgroups(g)
        assert n >= 2 and ragged, g
    counts = [(a[0], wc.workgroups(a)[0], wc.workgroups(b)[0]) for a, b in zip(CASE.groups(small), CASE.groups(big))]
    doubled = all(nb >= 2 * na for _, na, nb in counts)
    s_small, s_big = CASE.sections(lib, small), CASE.sections(lib, big)
    for name in s_small:
        assert s_small[name] == sco.chunks(small['M'])[0] * 27 * K * N * 4 > 0
        assert s_big[name] >= 2 * s_small[name] or (s_big[name] >= s_small[name] and doubled), (name, s_small, s_big, counts)


def test_restated_constants_are_on_the_source_lines_cited():
    for text, where in CASE.constants:
        fname, line = where.rsplit(':', 1)
        lines = open(os.path.join(ROOT, '3dvnet_amd', 'csrc', fname)).read().split('\n')
        assert text in lines[int(line) - 1], '%r is not on line %s of %s: %r' % (text, line, fname, lines[int(line) - 1][:120])
    assert sco.ROWS == 512


# ---- GPU --------------------------------------------------------------------------------------------------------------------------

_own = {}


def _run_case(size, cuda, poison, canary=False, shared=None):
    inp = CASE.make(size)
    arena = wc.Arena(cuda, poison, canary=canary, shared=shared)
    res, status = wc.execute(CASE, inp, arena)
    return inp, arena, res, status


def own(size, cuda):
    """(inputs, results, status) on 0xFF-filled buffers of its own; kept, and left unchanged by the tests."""
    if size not in _own:
        inp, _, res, status = _run_case(size, cuda, 0xFF)
        _own[size] = (inp, res, status)
    return _own[size]


@pytest.mark.gpu
def test_poison_independence(cuda):
    inp, res_ff, status_ff = own('small', cuda)
    _, _, res_00, status_00 = _run_case('small', cuda, 0x00)
    for name in res_ff:
        wc.assert_written(CASE.name, 'poison', name, res_00[name], res_ff[name])
    wc.assert_same_results(CASE.name, 'poison', res_00, status_00, res_ff, status_ff)
    CASE.check(inp, res_ff, status_ff)


@pytest.mark.gpu
def test_reuse_after_a_larger_call(cuda):
    _, res_own, status_own = own('small', cuda)
    _, before, _, _ = _run_case('big', cuda, 0xFF)
    _, after, res, status = _run_case('small', cuda, 0xFF, shared=before.shared)
    assert all(before.asked[name] >= nbytes > 0 for name, nbytes in after.asked.items())
    wc.assert_same_results(CASE.name, 'reuse after big', res, status, res_own, status_own)


@pytest.mark.gpu
def test_canaries(cuda):
    _, res_own, status_own = own('small', cuda)
    _, arena, res, status = _run_case('small', cuda, 0xFF, canary=True)
    wc.assert_canaries(CASE.name, arena)
    wc.assert_same_results(CASE.name, 'canaries', res, status, res_own, status_own)


@pytest.mark.gpu
def test_the_big_input_meets_the_checker(cuda):
    inp, _, res, status = _run_case('big', cuda, 0xFF)
    CASE.check(inp, res, status)
