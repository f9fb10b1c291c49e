"""The workspace and output contract of v3d_sparse_interp_backward_f32 (include/v3d.h): the chain v3d_hash_build ->
v3d_sparse_interp_backward_f32 -> v3d_hash_status through the C ABI on caller-made buffers, as a `Case` of the table of
tests/workspace_cases.py.

The case is written here and REGISTERED in that table when this module is imported (`register()` below: one `CASES.append`, one
`SIZED_BY` key), because this change adds test files only.  pytest imports every test module before it runs one, and this file's name
sorts before test_workspace_cases.py and test_workspace_contract_gpu.py, so in a run of the suite their completeness check, their
per-case checks and their GPU parametrisation all see the case.  Run alone, test_workspace_cases.py reports the two new entry
points as missing: that is the table's guard doing its work, and the cure is to move `CASE` into workspace_cases.py.  The tests
below hold the case to the same four properties with that file's own arena and helpers, so that this file also stands alone:

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
import torch

import sparse_interp_backward_oracle as sbo
import workspace_cases as wc
from conftest import ROOT
from workspace_cases import OK, p

C = 32
HASH = next(c for c in wc.CASES if c.name == 'hash_chain')


def _make(size):
    i = HASH.make(size)                                                       # the map and the queries of the forward's case
    rng = np.random.default_rng(70 + i['n'])
    ld, col0 = C + 12, 8
    grad = np.full((i['n_pts'] * i['n_hyp'], ld), np.nan, dtype=np.float32)
    grad[:, col0:col0 + C] = rng.standard_normal((grad.shape[0], C)).astype(np.float32)
    return dict(i, grad_out=grad, ld=ld, col0=col0, C=C, ts=1)


def _run(lib, a, i):
    n, n_pts, n_hyp, s = i['n'], i['n_pts'], i['n_hyp'], a.stream()
    tb, wb = lib.v3d_hash_bytes(n), lib.v3d_sparse_interp_backward_workspace_bytes(n, C, n_pts, n_hyp)
    table, ws = a.ws('table', tb), a.ws('interp_backward', wb)
    c = a.put('coords', i['coords'], torch.int32)
    assert lib.v3d_hash_build(p(c), n, p(table), tb, s) == OK
    out = a.out('grad_feats', (n, C), torch.float32)
    g, pts, pb, mn = a.put('g', i['grad_out']), a.put('pts', i['pts']), a.put('pb', i['pts_batch']), a.put('mn', i['min_pts'])
    assert lib.v3d_sparse_interp_backward_f32(p(table), n, C, 1, p(pts), p(pb), n_pts, n_hyp, p(mn), i['res'], p(g), i['ld'], i['col0'],
                                              p(out), p(ws), wb, s) == OK
    return (lib.v3d_hash_status(p(table), n, s),)


def _check(i, out, status):
    assert status == (OK,)
    orc = sbo.gradient(i)
    bad, worst, worst_zero = sbo.violations(out['grad_feats'].numpy(), orc)
    assert (orc['S'] > 0).any()
    assert bad == 0 and worst_zero == 0.0, 'grad_feats: %d elements outside (cnt + 2) u S, worst ratio %.3f' % (bad, worst)


CASE = wc.Case(
    'sparse_interp_backward', ('v3d_sparse_interp_backward_f32',), _make, _run, _check,
    bound='sparse_interp_backward_oracle.gradient within (cnt + 2) u S (tests/test_sparse_interp_backward_gpu.py::test_every_element_within_the_bound)',
    sections=lambda lib, i: {'table': lib.v3d_hash_bytes(i['n']),
                             'interp_backward': lib.v3d_sparse_interp_backward_workspace_bytes(i['n'], C, i['n_pts'], i['n_hyp'])},
    groups=lambda i: [('interp_corners / interp_backward_segment', i['n_pts'] * i['n_hyp'] * 8, 256),
                      ('interp_backward_count_kernel', i['n'] + 1, 256),
                      ('interp_backward_chunk_kernel', (i['n_pts'] * i['n_hyp'] * 8 // sbo.CHUNK + i['n']) * (C // 4), 256),
                      ('interp_backward_combine_kernel', i['n'] * (C // 4), 256)],
    constants=(('kInterpBwdChunk = 512', 'sparse.hip:200'),
               ('interp_backward_segment_kernel<<<(unsigned)((nq * 8 + 255) / 256), 256', 'sparse.hip:368'),
               ('interp_backward_count_kernel<<<(unsigned)(((long long)n_in + 256) / 256), 256', 'sparse.hip:374'),
               ('interp_backward_chunk_kernel<true><<<blocks, 256', 'sparse.hip:381'),
               ('interp_backward_combine_kernel<<<(unsigned)(((long long)n_in * tpc + 255) / 256), 256', 'sparse.hip:386')),
    paired=True)
SIZE_FUNCTION = 'v3d_sparse_interp_backward_workspace_bytes'


def register():
    """Put the case into the table of tests/workspace_cases.py, once."""
    if all(c.name != CASE.name for c in wc.CASES):
        wc.CASES.append(CASE)
        wc.SIZED_BY[SIZE_FUNCTION] = CASE.name


register()


# ---- CPU --------------------------------------------------------------------------------------------------------------------------

def test_the_table_holds_the_case_and_needs_it():
    assert CASE in wc.CASES and wc.missing_entry_points(wc.CASES) == []
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
