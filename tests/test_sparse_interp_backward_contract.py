"""The workspace and output contract of v3d_sparse_interp_backward_f32 (include/v3d.h): the chain v3d_hash_build ->
v3d_sparse_interp_backward_f32 -> v3d_hash_status through the C ABI on caller-made buffers, as a `Case` of the table of
tests/workspace_cases.py.

The case lives in that table (`CASE` below is the table's entry), so tests/test_workspace_cases.py and
tests/test_workspace_contract_gpu.py see it however they are run.  The tests below hold the case to the same four properties with that
file's own arena and helpers, so that this file also stands alone:

  CPU   the case's inputs are seeded and built without a device; every launch of the small input has at least two workgroups, the
        last one ragged; big is at least twice small in every buffer section or in every launch; the launch lines and the chunk
        constant the groups restate are on the source lines cited;
  GPU   poison    small on 0x00-filled and on 0xFF-filled buffers and outputs: same bits, same status, no element left unwritten;
        reuse     big, then small in the same buffers: the outputs of buffers of its own;
        canaries  buffers of exactly the bytes the size functions return, 4 KB of a fixed pattern in front and behind: all intact;
        paired    the table is poisoned before v3d_hash_build only; the 0xFF run of the big input meets the checker.
The 0xFF run has to meet tests/sparse_interp_backward_oracle.py at (cnt + 2) u S per element, so that an answer that is wrong both
times does not pass as "equal".  The gradient sits in rows of C + 12 floats from column 8 on, NaN around it.
"""
import os

import numpy as np
import pytest

import sparse_interp_backward_oracle as sbo
import workspace_cases as wc
from conftest import ROOT

C = wc.INTERP_BWD_C
CASE = next(c for c in wc.CASES if c.name == 'sparse_interp_backward')
SIZE_FUNCTION = 'v3d_sparse_interp_backward_workspace_bytes'


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_the_table_holds_the_case_and_needs_it():
    assert CASE in wc.CASES and wc.missing_entry_points(wc.CASES) == [] and wc.SIZED_BY[SIZE_FUNCTION] == CASE.name and C == 32
    rest = [c for c in wc.CASES if c is not CASE]
    assert set(wc.missing_entry_points(rest)) == {'v3d_sparse_interp_backward_f32', SIZE_FUNCTION}
    fns = wc.header_functions()
    assert fns['v3d_sparse_interp_backward_f32'][0] == 'table' and fns['v3d_sparse_interp_backward_f32'][-3:] == ['workspace', 'workspace_bytes', 'stream']


def test_inputs_are_seeded_and_built_without_a_device():
    for size in CASE.sizes:
        a, b = CASE.make(size), CASE.make(size)
        for k in a:
            x, y = np.asarray(a[k]), np.asarray(b[k])
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), (size, k)
        g = a['grad_out']
        assert np.isnan(g[:, :a['col0']]).all() and np.isnan(g[:, a['col0'] + C:]).all() and np.isfinite(g[:, a['col0']:a['col0'] + C]).all()


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
        assert s_small[name] > 0
        assert s_big[name] >= 2 * s_small[name] or (s_big[name] >= s_small[name] and doubled), (name, s_small, s_big, counts)


def test_restated_constants_are_on_the_source_lines_cited():
    for text, where in CASE.constants:
        fname, line = where.rsplit(':', 1)
        lines = open(os.path.join(ROOT, '3dvnet_amd', 'csrc', fname)).read().split('\n')
        assert text in lines[int(line) - 1], '%r is not on line %s of %s: %r' % (text, line, fname, lines[int(line) - 1][:120])
    assert '256' in ' '.join(t for t, _ in CASE.constants) and sbo.CHUNK == 512


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
def test_paired_calls_work_on_what_the_first_call_left(cuda):
    inp, _, res, status = _run_case('big', cuda, 0xFF)
    CASE.check(inp, res, status)
