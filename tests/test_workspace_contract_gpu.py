"""GPU: the workspace and output contract of include/v3d.h, for every entry of tests/workspace_cases.py, through the C ABI on
caller-made buffers.  Four properties; every comparison is on bits, and the 0xFF run also has to meet the module's own CPU checker
at the module's own bound (named in the case entry), so that an answer that is wrong both times does not pass as "equal":

  poison    small on 0x00-filled and on 0xFF-filled workspaces and outputs: same bits, same status, no element left unwritten;
  reuse     big, then small (and then every other input of the case) in the same workspace: outputs and status are those of a
            workspace of its own -- and, where the entry point keeps a device status word, the rejected input of the module's
            tests, then small, which reports OK;
  canaries  workspace of exactly *_workspace_bytes bytes and every output at its documented size, 4 KB of a fixed pattern in front
            and behind: all intact;
  paired    the chains poison their buffers before the first call only (that is how every run here works); the 0xFF run of the
            big input meets the checker, back-projection's feat == NULL call equals its feat-given call.

0xFF bytes are NaN as fp32 and as bf16 pairs, -1 as counters, "error" in every status word.  The small run on 0xFF is computed once
per case and shared.  Wall time of the file on one MI355X: 3.6 s for its 91 tests.

Wrong variants of the library these tests were tried against on MI355X (none committed), and what caught each: edges_csr_kernel
clearing its rank table on the LDS path only -> test_poison_independence[edges_csr], "edges_csr (ws_path), poison: status (0,)
against (-1,)"; the same call keeping its per-reference counts one int further back than v3d_edges_csr_workspace_bytes declares ->
test_canaries[edges_csr], "4 bytes behind workspace csr (48 bytes) were written, the first at offset 48"; mesh_render_fill_kernel
not resetting the status word -> test_poison_independence[mesh_render_depth], "poison in element 0 of output status".
"""
import functools

import pytest
import torch

import workspace_cases as wc

pytestmark = pytest.mark.gpu

RUNNABLE = [c for c in wc.CASES if c.covered_by is None]


FAULT = []


def run(case, size, cuda, poison, canary=False, shared=None):
    """One run of a case.  After a HIP error (the device reports a fault) nothing more is started on it: every later run fails here."""
    if FAULT:
        pytest.fail('not run: the device reported an error in %s' % FAULT[0])
    inp = case.make(size)
    arena = wc.Arena(cuda, poison, canary=canary, shared=shared)
    try:
        res, status = wc.execute(case, inp, arena)
    except RuntimeError:
        FAULT.append('%s (%s)' % (case.name, size))
        raise
    return inp, arena, res, status


@functools.lru_cache(maxsize=None)
def _own(case_name, size):
    """(inputs, results, status) of a case on 0xFF-filled buffers of its own; kept, and left unchanged by the tests."""
    case = next(c for c in wc.CASES if c.name == case_name)
    inp, _, res, status = run(case, size, torch.device('cuda:0'), 0xFF)
    return inp, res, status


@pytest.mark.parametrize('case', RUNNABLE, ids=repr)
def test_poison_independence(case, cuda):
    for size in ('small',) + case.extra:
        inp, res_ff, status_ff = _own(case.name, size)
        _, _, res_00, status_00 = run(case, size, cuda, 0x00)
        entry = '%s (%s)' % (case.name, size)
        assert res_00.keys() == res_ff.keys()
        for name in res_ff:
            if res_00[name].shape == res_ff[name].shape:
                wc.assert_written(entry, 'poison', name, res_00[name], res_ff[name])
        wc.assert_same_results(entry, 'poison', res_00, status_00, res_ff, status_ff)
        case.check(inp, res_ff, status_ff)


@pytest.mark.parametrize('case', RUNNABLE, ids=repr)
def test_reuse_after_a_larger_call(case, cuda):
    for first, then in case.reuse:
        _, res_own, status_own = _own(case.name, then)
        _, before, _, _ = run(case, first, cuda, 0xFF)
        _, after, res, status = run(case, then, cuda, 0xFF, shared=before.shared)
        if case.sections is None and (first, then) == ('big', 'small'):
            # the size function takes a weight handle: "big is at least twice small in every section" is checked here, on the device
            for name, nbytes in after.asked.items():
                assert before.asked[name] >= 2 * nbytes > 0, '%s: workspace %s is %d bytes for big, %d for small' % (
                    case.name, name, before.asked[name], nbytes)
        wc.assert_same_results('%s (%s)' % (case.name, then), 'reuse after %s' % first, res, status, res_own, status_own)


@pytest.mark.parametrize('case', [c for c in RUNNABLE if c.rejected], ids=repr)
def test_status_word_describes_the_last_call(case, cuda):
    _, res_own, status_own = _own(case.name, 'small')
    _, bad, _, bad_status = run(case, case.rejected, cuda, 0xFF)
    assert bad_status[0] in (wc.BAD_SHAPE, wc.BAD_ARG) or bad_status[0] > 0, '%s: the rejected input was accepted: %r' % (case.name, bad_status)
    _, _, res, status = run(case, 'small', cuda, 0xFF, shared=bad.shared)
    wc.assert_same_results(case.name, 'reuse after a rejected call', res, status, res_own, status_own)


@pytest.mark.parametrize('case', RUNNABLE, ids=repr)
def test_canaries(case, cuda):
    for size in ('small',) + case.extra:
        _, res_own, status_own = _own(case.name, size)
        _, arena, res, status = run(case, size, cuda, 0xFF, canary=True)
        entry = '%s (%s)' % (case.name, size)
        wc.assert_canaries(entry, arena)
        wc.assert_same_results(entry, 'canaries', res, status, res_own, status_own)


@pytest.mark.parametrize('case', [c for c in RUNNABLE if c.paired], ids=repr)
def test_paired_calls_work_on_what_the_first_call_left(case, cuda):
    inp, _, res, status = run(case, 'big', cuda, 0xFF)
    case.check(inp, res, status)
