"""CPU: the case table of the workspace-contract tests (tests/workspace_cases.py) is complete, its inputs are built without a device and
obey the shape rules, and its comparison helpers see a single poisoned element, a single differing bit and a single touched canary byte
(as tests/test_large_launch_helpers.py does for its checker)."""
import os
import re

import numpy as np
import pytest
import torch

import workspace_cases as wc
from conftest import ROOT

CPU = torch.device('cpu')
RUNNABLE = [c for c in wc.CASES if c.covered_by is None]


# ---- completeness -------------------------------------------------------------------------------------------------------------------

def test_header_parser_finds_the_workspace_and_table_parameters():
    fns = wc.header_functions()
    assert fns['v3d_hash_build'] == ['coords', 'n', 'table', 'table_bytes', 'stream']
    assert fns['v3d_voxelize_workspace_bytes'] == [] and fns['v3d_mesh_extract_f32'][-3:] == ['workspace', 'workspace_bytes', 'stream']
    need = wc.required_entry_points()
    assert {'v3d_edges_csr_status', 'v3d_hash_status', 'v3d_sparse_neighbors', 'v3d_psv_sample_positions_f32', 'v3d_hash_bytes',
            'v3d_order_stats_workspace_bytes', 'v3d_cloud_status'} <= need
    assert 'v3d_gemm_gather_f32' not in need and len(need) >= 50


def test_every_entry_point_is_in_the_table():
    missing = wc.missing_entry_points(wc.CASES)
    assert missing == [], 'entry points of include/v3d.h without a case: %s' % missing
    declared = set(wc.header_functions())
    for c in wc.CASES:
        assert set(c.entry_points) <= declared, c                                # nothing in the table that the header does not declare
    assert set(wc.SIZED_BY) <= declared and set(wc.SIZED_BY.values()) <= {c.name for c in RUNNABLE}
    assert len({c.name for c in wc.CASES}) == len(wc.CASES)


@pytest.mark.parametrize('case', wc.CASES, ids=repr)
def test_the_table_is_incomplete_without_any_one_entry(case):
    rest = [c for c in wc.CASES if c is not case]
    gone = wc.missing_entry_points(rest)
    assert gone and set(gone) & (set(case.entry_points) | {f for f, n in wc.SIZED_BY.items() if n == case.name}), (case, gone)


def test_the_only_indirection_is_a_test_that_exists():
    pointed = [c for c in wc.CASES if c.covered_by is not None]
    assert sorted(c.entry_points[0] for c in pointed) == ['v3d_confidence_logits_f32', 'v3d_probability_map_f32', 'v3d_propagation_up_f32',
                                                          'v3d_soft_argmin_f32']
    for c in pointed:
        test, fname = c.covered_by
        src = open(os.path.join(ROOT, 'tests', fname)).read()
        body = re.search(r'^def %s\(.*?(?=^def |\Z)' % re.escape(test), src, flags=re.S | re.M)
        assert body is not None, '%s: no %s in %s' % (c.name, test, fname)
        assert 'lib.%s(' % c.entry_points[0] in body.group(0), '%s does not call %s' % (test, c.entry_points[0])
    src = open(os.path.join(ROOT, 'tests', 'test_large_launch_gpu.py')).read()
    assert 'poison' in src.lower()


def test_every_runnable_case_is_whole():
    for c in RUNNABLE:
        assert callable(c.make) and callable(c.run) and callable(c.check) and callable(c.groups) and c.bound and c.constants, c
        assert c.sizes == ('small', 'big')
    for c in RUNNABLE:
        assert all(isinstance(n, str) and ' ' not in n for n in c.inout), c          # names of arena.state buffers, not prose
        assert all(f in c.sizes + c.extra and t in c.sizes + c.extra for f, t in c.reuse) and ('big', 'small') in c.reuse
        assert {x for pair in c.reuse for x in pair} >= set(c.extra), c              # every other input shares a workspace with another too
    assert {c.name for c in RUNNABLE if c.inout} == {'decoder_fused'}
    with_status = {c.name for c in RUNNABLE if c.rejected}
    assert with_status == {'edges_csr', 'voxelize_chain', 'hash_chain', 'cloud_downsample', 'mesh_render_depth'}
    assert {c.name for c in RUNNABLE if c.paired} >= {'voxelize_chain', 'mesh_count_extract', 'hash_chain', 'edges_csr', 'cloud_downsample',
                                                      'backproject_variance', 'segment_csr_max', 'sparse_interp_backward'}
    assert {'sparse_interp_backward', 'sparse_conv_weight_grad'} <= {c.name for c in RUNNABLE} - with_status


# ---- inputs and shape rules ---------------------------------------------------------------------------------------------------------

def _arrays(x):
    if isinstance(x, dict):
        for v in x.values():
            yield from _arrays(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            yield from _arrays(v)
    elif isinstance(x, (np.ndarray, torch.Tensor)):
        yield x


@pytest.mark.parametrize('case', RUNNABLE, ids=repr)
def test_inputs_are_built_without_a_device_and_are_seeded(case):
    for size in case.sizes + case.extra + ((case.rejected,) if case.rejected else ()):
        a, b = case.make(size), case.make(size)
        arr_a, arr_b = list(_arrays(a)), list(_arrays(b))
        assert arr_a and len(arr_a) == len(arr_b)
        for x, y in zip(arr_a, arr_b):
            assert not (torch.is_tensor(x) and x.is_cuda)
            x, y = np.asarray(x), np.asarray(y)
            assert x.shape == y.shape and x.tobytes() == y.tobytes(), '%s (%s): not the same input twice' % (case, size)


@pytest.mark.parametrize('case', RUNNABLE, ids=repr)
def test_shape_rules(case):
    """Every case, whether its size function needs a device or not.  Small (big, where the issue's own shape table puts small below
    one tile): every launch has at least two workgroups, the last one ragged; a group that cannot says why in the entry.  Big: at
    least twice small in every workspace section, through the *_workspace_bytes functions; a section of fixed size is named as
    such.  Where the size function rounds small sections up to one granule, or takes a weight handle that only a device makes,
    big runs at least twice the workgroups of small in every launch instead."""
    _, lib = wc.lib_modules()
    small, big = case.make('small'), case.make('big')
    assert case.rule_on in ('small', 'big')
    groups = case.groups(case.make(case.rule_on))
    assert groups
    for g in groups:
        n, ragged = wc.workgroups(g)
        why = wc.exemption(g)
        if why is None:
            assert n >= 2 and ragged, '%s (%s): %r runs %d workgroups, ragged: %s' % (case, case.rule_on, g[0], n, ragged)
        else:
            assert isinstance(why, str) and len(why) > 10 and not (n >= 2 and ragged), (case, g)      # a reason, and one that is needed
    g_small, g_big = case.groups(small), case.groups(big)
    assert [g[0] for g in g_small] == [g[0] for g in g_big]
    counts = [(a[0], wc.workgroups(a)[0], wc.workgroups(b)[0]) for a, b in zip(g_small, g_big) if a[2] is not None]
    doubled = all(nb >= 2 * na for _, na, nb in counts)
    if case.sections is None:
        assert doubled, '%s: workgroups (kernel, small, big) %s' % (case, counts)
        # the size function takes a weight handle, which only a device makes: test_reuse_after_a_larger_call compares the bytes there
        assert any(f.startswith(('v3d_costreg_workspace', 'v3d_irb_workspace')) for f, n in wc.SIZED_BY.items()
                   if n == case.name or n == 'costreg_depth_f32' and case.name.startswith('costreg_depth_')), case
        return
    s_small, s_big = case.sections(lib, small), case.sections(lib, big)
    assert s_small.keys() == s_big.keys()
    for name in s_small:
        assert s_small[name] > 0
        if name in case.fixed:
            assert s_big[name] == s_small[name]
        else:
            assert s_big[name] >= 2 * s_small[name] or (s_big[name] >= s_small[name] and doubled), (case, name, s_small, s_big, counts)


@pytest.mark.parametrize('case', RUNNABLE, ids=repr)
def test_restated_constants_are_on_the_source_lines_the_entry_cites(case):
    assert case.constants
    for text, where in case.constants:
        fname, line = where.rsplit(':', 1)
        path = os.path.join(ROOT, fname) if '/' in fname else os.path.join(ROOT, '3dvnet_amd', 'csrc', fname)
        lines = open(path).read().split('\n')
        assert text in lines[int(line) - 1], '%s: %r is not on line %s of %s: %r' % (case, text, line, fname, lines[int(line) - 1][:120])
    per = {g[2] for size in case.sizes for g in case.groups(case.make(size)) if g[2] is not None}
    cited = ' '.join(text for text, _ in case.constants)
    for v in per:                                                               # every workgroup size the groups use is in a cited text
        assert str(v) in cited or (v == 32 and 'kDPtsWave = 4' in cited), (case, v, cited)


def test_the_two_paths_of_the_edge_kernel_are_both_in_the_table():
    case = next(c for c in wc.CASES if c.name == 'edges_csr')
    m = re.search(r'kLdsImgs = (\d+), kLdsEdges = (\d+)', case.constants[0][0])
    lds = dict(kLdsImgs=int(m.group(1)), kLdsEdges=int(m.group(2)))
    small, ws = case.make('small'), case.make('ws_path')
    assert small['n_img'] <= lds['kLdsImgs'] and small['n_edges'] <= lds['kLdsEdges']
    assert ws['n_img'] > lds['kLdsImgs'] or ws['n_edges'] > lds['kLdsEdges']


# ---- the arena and the comparison helpers -------------------------------------------------------------------------------------------

def _toy_run(arena, skip=None, overrun=0, flip=False):
    """A toy 'call': writes i * 0.5 into a 10-element output (all but element `skip`), counts into its workspace."""
    ws = arena.ws('toy', 64)
    out = arena.out('out', (10,), torch.float32)
    n = arena.out('n', (1,), torch.int32)
    vals = torch.arange(10, dtype=torch.float32) * 0.5
    if flip:
        vals.view(torch.int32)[3] ^= 1                                           # one bit
    for k in range(10):
        if k != skip:
            out[k] = vals[k]
    n[0] = 10
    ws[:] = 7
    if overrun:
        base = ws.storage_offset()
        whole = next(w for name, w, _ in arena.guards if name == 'workspace toy')
        whole[base + 64 + overrun - 1] = 0
    return arena.results()


def test_arena_poisons_what_it_hands_out_and_nothing_else():
    a = wc.Arena(CPU, 0xFF)
    assert (a.ws('w', 100) == 0xFF).all() and a.ws('w', 100).numel() == 100
    o = a.out('o', (3, 5), torch.float32)
    assert o.shape == (3, 5) and torch.isnan(o).all() and (o.view(torch.int32) == -1).all()
    assert (a.out('c', (4,), torch.int64) == -1).all() and (wc.Arena(CPU, 0).out('z', (4,), torch.float64) == 0).all()
    t = a.put('in', np.arange(5, dtype=np.int64), torch.int32)
    assert t.dtype == torch.int32 and t.tolist() == [0, 1, 2, 3, 4]              # inputs are the caller's: never poisoned
    st = a.state('acc', np.ones(3, dtype=np.float32))
    st += 1                                                                      # in/out state may change ...
    wc.assert_inputs_unchanged('toy', a)
    t[2] = 9                                                                     # ... a read-only input may not
    with pytest.raises(AssertionError, match='toy: input in was written: element 2 differs, 1 of 5 elements'):
        wc.assert_inputs_unchanged('toy', a)
    assert set(a.states) == {'acc'} and set(a.inputs) == {'in'}
    with pytest.raises(AssertionError):
        a.put('acc', np.zeros(1))
    a.length('o', 2)
    assert a.results()['o'].shape == (2, 5) and a.results()['c'].shape == (4,)
    g = wc.Arena(CPU, 0xFF, canary=True)
    w = g.ws('w', 100)
    name, whole, nbytes = g.guards[0]
    assert nbytes == 100 and whole.numel() == 100 + 2 * wc.GUARD and w.storage_offset() == wc.GUARD and wc.GUARD % 512 == 0
    assert (whole[:wc.GUARD] == wc.CANARY).all() and (whole[wc.GUARD + 100:] == wc.CANARY).all() and (w == 0xFF).all()


def test_a_reused_workspace_is_the_front_of_the_earlier_one_as_it_was_left():
    big = wc.Arena(CPU, 0xFF)
    big.ws('w', 256)[:] = 3
    small = wc.Arena(CPU, 0x00, shared=big.shared)
    w = small.ws('w', 64)
    assert small.asked == {'w': 64} and big.asked == {'w': 256}
    assert w.numel() == 64 and (w == 3).all() and w.data_ptr() == big.shared['w'].data_ptr()
    with pytest.raises(AssertionError):
        small.ws('w', 512)


def test_helpers_pass_a_clean_toy_call():
    r00, rff = _toy_run(wc.Arena(CPU, 0x00)), _toy_run(wc.Arena(CPU, 0xFF))
    for name in rff:
        wc.assert_written('toy', 'poison', name, r00[name], rff[name])
    wc.assert_same_results('toy', 'poison', r00, (0,), rff, (0,))
    g = wc.Arena(CPU, 0xFF, canary=True)
    _toy_run(g)
    wc.assert_canaries('toy', g)


def test_helpers_see_one_poisoned_element():
    r00, rff = _toy_run(wc.Arena(CPU, 0x00), skip=6), _toy_run(wc.Arena(CPU, 0xFF), skip=6)
    with pytest.raises(AssertionError, match=r'toy, poison: poison in element 6 of output out \(1 of 10 elements never written\)'):
        wc.assert_written('toy', 'poison', 'out', r00['out'], rff['out'])
    with pytest.raises(AssertionError, match='output out differs in element 6'):
        wc.assert_same_results('toy', 'poison', r00, (0,), rff, (0,))
    # element 0 is a legitimate 0.0: written both times, and not reported
    wc.assert_written('toy', 'poison', 'out', _toy_run(wc.Arena(CPU, 0x00))['out'], _toy_run(wc.Arena(CPU, 0xFF))['out'])


def test_helpers_see_one_bit_and_a_status():
    a, b = _toy_run(wc.Arena(CPU, 0xFF)), _toy_run(wc.Arena(CPU, 0xFF), flip=True)
    assert wc.first_difference(a['out'], b['out']) == (3, 1) and wc.first_difference(a['n'], b['n']) == (None, 0)
    with pytest.raises(AssertionError, match=r'toy, reuse: output out differs in element 3 \(1.5 against 1.50000\d+\), 1 of 10 elements differ'):
        wc.assert_same_results('toy', 'reuse', a, (0,), b, (0,))
    with pytest.raises(AssertionError, match='status'):
        wc.assert_same_results('toy', 'reuse', a, (0,), a, (-1,))
    nan = torch.full((4,), float('nan'))
    other = nan.clone()
    other.view(torch.int32)[2] ^= 0x10                                           # another NaN: bits differ although neither equals itself
    assert wc.first_difference(nan, nan.clone()) == (None, 0) and wc.first_difference(nan, other) == (2, 1)
    with pytest.raises(AssertionError, match='valid elements'):
        wc.assert_same_results('toy', 'reuse', {'x': torch.zeros(3)}, (), {'x': torch.zeros(4)}, ())


@pytest.mark.parametrize('overrun', [1, 300, wc.GUARD])
def test_helpers_see_one_canary_byte(overrun):
    g = wc.Arena(CPU, 0xFF, canary=True)
    _toy_run(g, overrun=overrun)
    message = r'toy, canaries: 1 bytes behind workspace toy \(64 bytes\) were written, the first at offset %d' % (64 + overrun - 1)
    with pytest.raises(AssertionError, match=message):
        wc.assert_canaries('toy', g)
    g = wc.Arena(CPU, 0xFF, canary=True)
    _toy_run(g)
    g.guards[1][1][wc.GUARD - 1] = 0                                             # the byte in front of output `out`
    with pytest.raises(AssertionError, match='in front of output out'):
        wc.assert_canaries('toy', g)
    with pytest.raises(AssertionError, match='no guarded buffer'):
        wc.assert_canaries('toy', wc.Arena(CPU, 0xFF))


def test_dropping_a_written_output_from_a_case_fires_the_poison_check():
    """The segment case's checker and the poison helper on the CPU: with the pooled output left as the arena made it, both fire."""
    case = next(c for c in wc.CASES if c.name == 'segment_csr_max')
    i = case.make('small')

    def fake(poison, with_pool):
        a = wc.Arena(CPU, poison)
        a.out('perm', (i['n'],), torch.int32)[:] = torch.from_numpy(np.argsort(i['ids'], kind='stable').astype(np.int32))
        counts = np.bincount(i['ids'], minlength=i['n_seg'])
        a.out('offsets', (i['n_seg'] + 1,), torch.int32)[:] = torch.from_numpy(np.concatenate(([0], np.cumsum(counts))).astype(np.int32))
        pool = a.out('pool', (i['n_seg'], i['N']), torch.float32)
        if with_pool:
            ref = np.full((i['n_seg'], i['N']), -np.inf, dtype=np.float32)
            np.maximum.at(ref, i['ids'], i['src'][:, :i['N']])
            pool[:] = torch.from_numpy(ref)
        return a.results()

    good00, goodff = fake(0x00, True), fake(0xFF, True)
    case.check(i, goodff, ())
    wc.assert_same_results('segment', 'poison', good00, (), goodff, ())
    bad00, badff = fake(0x00, False), fake(0xFF, False)
    with pytest.raises(AssertionError, match='poison in element 0 of output pool'):
        wc.assert_written('segment', 'poison', 'pool', bad00['pool'], badff['pool'])
    with pytest.raises(AssertionError):
        case.check(i, badff, ())
