"""The case table of tests/test_workspace_contract_gpu.py: one entry per C entry point of include/v3d.h that takes a `workspace` or
`table` pointer or writes whole output arrays, or per chain of calls that share a workspace by contract.

An entry (a `Case`) holds
  * `make(size)`      seeded inputs as NumPy arrays and plain numbers, built without a device.  Every case has 'small' and 'big';
                      some have more (`extra`: another code path, an empty side; `rejected`: the input the module's own tests use to
                      set the entry point's device status word);
  * `run(lib, arena, inp)`   the call or the chain through the C ABI (ctypes).  Every buffer comes from the `Arena`:
                      `arena.ws(name, nbytes)` a workspace of exactly the bytes the `*_workspace_bytes` function returns,
                      `arena.out(name, shape, dtype)` a pure output, `arena.put(name, array)` an input (in/out buffers the header
                      defines as accumulated or as inputs go through `put` and are never poisoned).  It returns the status: every
                      return code of a status call and every count a call hands to the host;  `arena.length(name, rows)` states the
                      valid rows of an output whose length comes back from the call (the tail is not specified);
  * `check(inp, out, status)` the module's CPU checker at the bound the module's own GPU test uses (named in `bound`);
  * `sections(lib, inp)`     the bytes of every workspace section, through the `*_workspace_bytes` functions (no GPU needed);
  * `groups(inp)`            (kernel, items, items per workgroup[, independent batches[, exemption]]) of every launch.  The shape
                      rule (two workgroups, the last one ragged) is asserted for every group; a group that cannot meet it says why
                      in its fifth field (or runs as one workgroup by design: items per workgroup None);
  * `constants`              (text, 'file:line') pairs: the launch lines and constants the groups restate.  The CPU test finds each
                      text on that line of the source;
  * `inout`                  the names of the buffers handed out through `arena.state`: in/out buffers, the caller's, never poisoned.
                      Everything handed out through `arena.put` is a read-only input and is compared with a kept copy after the run.

The arena is what the four properties are made of: it fills what it hands out with the poison byte, puts 4 KB of CANARY bytes in
front of and behind every workspace and output when asked to, and hands the workspace of an earlier run out again (reuse).  The
comparison helpers at the end work on tensors of any device; tests/test_workspace_cases.py runs them on the CPU.
"""
import ctypes
import os
import re

import numpy as np
import torch

from conftest import ROOT, v3d

OK, BAD_SHAPE, BAD_ARG = 0, -1, -2
GUARD = 4096
CANARY = 0xA5


# ---- arena ----------------------------------------------------------------------------------------------------------------------

class Arena:
    """Hands a case its device buffers.  poison: the byte every workspace and pure output is filled with before the first call.
    canary: every workspace and output lies inside a larger tensor, GUARD bytes of CANARY in front and behind (the start keeps
    the alignment torch gives: GUARD is a multiple of it).  shared: {name: buffer} of workspaces an earlier arena left behind;
    a workspace asked for under such a name is the front of that buffer, as the earlier run left it."""

    def __init__(self, device, poison, canary=False, shared=None):
        self.device, self.poison, self.canary = device, poison, canary
        self.shared = {} if shared is None else shared
        self.fresh_ws = shared is None
        self.outputs, self.lengths, self.guards, self.inputs, self.states, self.asked = {}, {}, [], {}, {}, {}

    def _region(self, name, nbytes):
        nbytes = int(nbytes)
        if not self.canary:
            return torch.full((max(nbytes, 1),), self.poison, dtype=torch.uint8, device=self.device)[:nbytes]
        whole = torch.full((2 * GUARD + nbytes,), CANARY, dtype=torch.uint8, device=self.device)
        whole[GUARD:GUARD + nbytes] = self.poison
        self.guards.append((name, whole, nbytes))
        return whole[GUARD:GUARD + nbytes]

    def ws(self, name, nbytes):
        nbytes = int(nbytes)
        self.asked[name] = nbytes
        have = self.shared.get(name)
        if have is not None and not self.fresh_ws:
            assert have.numel() >= nbytes, 'workspace %s: %d bytes kept, %d asked for' % (name, have.numel(), nbytes)
            return have[:nbytes]
        buf = self._region('workspace ' + name, nbytes)
        self.shared[name] = buf
        return buf

    def out(self, name, shape, dtype):
        shape = tuple(int(s) for s in shape)
        item = torch.empty((), dtype=dtype).element_size()
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        t = self._region('output ' + name, n * item).view(dtype).view(shape)
        self.outputs[name] = t
        return t

    def put(self, name, array, dtype=None):
        """A read-only input: never poisoned, and `assert_inputs_unchanged` finds it as it was handed out."""
        assert name not in self.inputs and name not in self.states, name
        t = torch.from_numpy(np.ascontiguousarray(array))
        t = (t if dtype is None else t.to(dtype)).to(self.device).contiguous()
        self.inputs[name] = (t, t.clone())
        return t

    def state(self, name, array, dtype=None):
        """An in/out buffer the header defines as accumulated, or as an input that an earlier call of the caller's built (a hash
        table): the caller's, never poisoned.  The case entry lists these names in `inout`."""
        assert name not in self.inputs and name not in self.states, name
        t = torch.from_numpy(np.ascontiguousarray(array))
        self.states[name] = (t if dtype is None else t.to(dtype)).to(self.device).contiguous()
        return self.states[name]

    def length(self, name, rows):
        self.lengths[name] = int(rows)

    def stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream if self.device.type == 'cuda' else None

    def results(self):
        """{name: CPU tensor cut to its valid rows}"""
        res = {}
        for name, t in self.outputs.items():
            t = t.detach().cpu()
            res[name] = t[:self.lengths[name]] if name in self.lengths else t
        return res


def p(t):
    return None if t is None else t.data_ptr()


def host_f32(values):
    a = np.ascontiguousarray(values, dtype=np.float32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


# ---- comparison helpers -----------------------------------------------------------------------------------------------------------

def as_bytes(t):
    t = t.contiguous()
    return t.view(torch.uint8).reshape(-1) if t.numel() else torch.empty(0, dtype=torch.uint8)


def first_difference(a, b):
    """(index of the first differing ELEMENT, number of differing elements) of two tensors of one shape and type, on bits."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.numel() == 0:
        return None, 0
    item = a.element_size()
    diff = (as_bytes(a).view(-1, item) != as_bytes(b).view(-1, item)).any(dim=1)
    n = int(diff.sum())
    return (int(diff.nonzero()[0]) if n else None), n


def poisoned_elements(t, poison):
    """flat bool: the elements of t whose bytes are all the poison byte"""
    if t.numel() == 0:
        return torch.zeros(0, dtype=torch.bool)
    return (as_bytes(t).view(-1, t.element_size()) == poison).all(dim=1)


def assert_written(entry, prop, name, t00, tff):
    """An element nobody stored holds 0x00 bytes after the run on a 0x00 arena AND 0xFF bytes after the run on a 0xFF arena."""
    left = poisoned_elements(t00, 0x00) & poisoned_elements(tff, 0xFF)
    n = int(left.sum())
    assert n == 0, '%s, %s: poison in element %d of output %s (%d of %d elements never written)' % (
        entry, prop, int(left.nonzero()[0]), name, n, left.numel())


def assert_same_bits(entry, prop, name, a, b):
    k, n = first_difference(a, b)
    if n:
        fa, fb = a.reshape(-1)[k], b.reshape(-1)[k]
        raise AssertionError('%s, %s: output %s differs in element %d (%r against %r), %d of %d elements differ' % (
            entry, prop, name, k, fa.item(), fb.item(), n, a.numel()))


def assert_same_results(entry, prop, res_a, status_a, res_b, status_b):
    assert status_a == status_b, '%s, %s: status %r against %r' % (entry, prop, status_a, status_b)
    assert res_a.keys() == res_b.keys()
    for name in res_a:
        assert res_a[name].shape == res_b[name].shape, '%s, %s: output %s has %s against %s valid elements' % (
            entry, prop, name, tuple(res_a[name].shape), tuple(res_b[name].shape))
        assert_same_bits(entry, prop, name, res_a[name], res_b[name])


def assert_inputs_unchanged(entry, arena):
    """No call writes a buffer the header gives it as `const`: every `arena.put` tensor holds the bits it was handed out with."""
    for name, (t, kept) in arena.inputs.items():
        k, n = first_difference(t.detach().cpu(), kept.cpu())
        assert n == 0, '%s: input %s was written: element %d differs, %d of %d elements' % (entry, name, k, n, t.numel())


def assert_canaries(entry, arena):
    assert arena.guards, '%s: the arena holds no guarded buffer' % entry
    for name, whole, nbytes in arena.guards:
        w = whole.detach().cpu()
        for side, part, base in (('in front of', w[:GUARD], -GUARD), ('behind', w[GUARD + nbytes:], nbytes)):
            bad = part != CANARY
            n = int(bad.sum())
            assert n == 0, '%s, canaries: %d bytes %s %s (%d bytes) were written, the first at offset %d' % (
                entry, n, side, name, nbytes, base + int(bad.nonzero()[0]))


# ---- the header -------------------------------------------------------------------------------------------------------------------

def header_functions():
    """{name: [parameter names]} of every function include/v3d.h declares (comments removed, as tests/test_cabi.py does)."""
    src = open(os.path.join(ROOT, 'include', 'v3d.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    out = {}
    for m in re.finditer(r'\b(v3d_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        params = [re.sub(r'\[.*?\]', '', q).strip().split()[-1].lstrip('*') for q in m.group(2).split(',') if q.strip() not in ('', 'void')]
        out[m.group(1)] = params
    return out


def required_entry_points():
    """Every function with a parameter named `workspace` or `table`, and every *_workspace_bytes / v3d_hash_bytes function."""
    fns = header_functions()
    need = {n for n, ps in fns.items() if 'workspace' in ps or 'table' in ps}
    need |= {n for n in fns if n.endswith('_workspace_bytes') or n == 'v3d_hash_bytes'}
    return need


# ---- the table --------------------------------------------------------------------------------------------------------------------

class Case:
    def __init__(self, name, entry_points, make, run=None, check=None, bound='', sections=None, groups=None, constants=(),
                 sizes=('small', 'big'), extra=(), rejected=None, inout=(), paired=False, covered_by=None, fixed=(), rule_on='small',
                 reuse=None):
        self.name, self.entry_points, self.make, self.run, self.check, self.bound = name, tuple(entry_points), make, run, check, bound
        self.sections, self.groups, self.constants = sections, groups, tuple(constants)
        self.sizes, self.extra, self.rejected, self.inout, self.paired, self.covered_by = sizes, tuple(extra), rejected, inout, paired, covered_by
        # fixed: workspace sections whose size does not depend on the shape (big == small);  rule_on: the input the two-workgroup
        # rule is checked on ('big' where the issue's shape table puts small below one tile)
        self.fixed, self.rule_on = tuple(fixed), rule_on
        # reuse: (first, then) pairs of inputs run one after the other in one workspace; `then` alone is the yardstick
        self.reuse = tuple(reuse) if reuse is not None else (('big', 'small'),) + tuple(('big', e) for e in self.extra)

    def __repr__(self):
        return self.name


CASES = []


def lib_modules():
    libm = v3d('_lib')
    return libm, libm.load()


def execute(case, inp, arena):
    """One run of a case on an arena -> (results, status); synchronises."""
    _, lib = lib_modules()
    status = case.run(lib, arena, inp)
    if arena.device.type == 'cuda':
        torch.cuda.synchronize(arena.device)
    assert_inputs_unchanged(case.name, arena)
    assert set(arena.states) == set(case.inout), '%s: in/out buffers %s, the entry names %s' % (case.name, sorted(arena.states), case.inout)
    return arena.results(), status


# ---- v3d_edges_csr -> v3d_edges_csr_status ----------------------------------------------------------------------------------------

def _edges_make(size):
    n_img, n_ref, n_edges = {'small': (5, 3, 9), 'big': (12, 7, 40), 'ws_path': (4100, 9, 300), 'rejected': (5, 3, 9)}[size]
    rng = np.random.default_rng({'small': 1, 'big': 2, 'ws_path': 3, 'rejected': 1}[size])
    refs = np.sort(rng.choice(n_img, n_ref, replace=False))
    r = np.concatenate((refs, refs[rng.integers(0, n_ref, n_edges - n_ref)]))
    edges = np.stack((r, rng.integers(0, n_img, n_edges)))[:, rng.permutation(n_edges)].astype(np.int64)
    # rejected: the wrong reference count of tests/test_driver.py (one more than the list holds)
    return dict(edges=edges, n_img=n_img, n_ref=n_ref + (size == 'rejected'), n_edges=n_edges)


def _edges_run(lib, a, i):
    nb = lib.v3d_edges_csr_workspace_bytes(i['n_img'], i['n_ref'])
    ws = a.ws('csr', nb)
    e = a.put('edges', i['edges'])
    ref_img, ofs = a.out('ref_img', (i['n_ref'],), torch.int32), a.out('edge_ofs', (i['n_ref'] + 1,), torch.int32)
    src = a.out('edge_src', (i['n_edges'],), torch.int32)
    assert lib.v3d_edges_csr(p(e), i['n_edges'], i['n_img'], i['n_ref'], p(ref_img), p(ofs), p(src), p(ws), nb, a.stream()) == OK
    return (lib.v3d_edges_csr_status(p(ws), nb, a.stream()),)


def _edges_check(i, out, status):
    assert status == (OK,)
    refs, counts = np.unique(i['edges'][0], return_counts=True)
    assert np.array_equal(out['ref_img'].numpy(), refs)
    assert np.array_equal(out['edge_ofs'].numpy(), np.concatenate(([0], np.cumsum(counts))))
    assert np.array_equal(out['edge_src'].numpy(), i['edges'][1][np.argsort(i['edges'][0], kind='stable')])


CASES.append(Case(
    'edges_csr', ('v3d_edges_csr', 'v3d_edges_csr_status'), _edges_make, _edges_run, _edges_check,
    bound='numpy.unique / stable argsort of the edge list, exact (torch.unique in tests/test_driver.py)',
    sections=lambda lib, i: {'csr': lib.v3d_edges_csr_workspace_bytes(i['n_img'], i['n_ref'])},
    groups=lambda i: [('edges_csr_kernel', i['n_edges'], None)],              # one workgroup by design (edges.hip:159)
    constants=(('kLdsImgs = 4096, kLdsEdges = 8192', 'edges.hip:24'), ('edges_csr_kernel<<<1, kThreads', 'edges.hip:159')),
    extra=('ws_path',), rejected='rejected', paired=True,
    reuse=(('big', 'small'), ('ws_path', 'small'))))                            # the LDS path after the workspace path of a larger list


# ---- v3d_segment_csr -> v3d_segment_max_f32 ---------------------------------------------------------------------------------------

def _segment_make(size):
    n, n_seg, N = {'small': (700, 300, 40), 'big': (1500, 650, 40)}[size]       # N <= 128: 8 segments per workgroup (segment.hip:178)
    rng = np.random.default_rng(10 + n)
    ids = rng.integers(0, n_seg, n)
    ids[ids % 5 == 0] += 1                                                     # every fifth segment has no rows
    ids = np.minimum(ids, n_seg - 2)                                           # ... and neither has the last one
    return dict(ids=ids.astype(np.int32), n=n, n_seg=n_seg, N=N, src=rng.standard_normal((n, N + 4)).astype(np.float32))


def _segment_run(lib, a, i):
    n, n_seg, N = i['n'], i['n_seg'], i['N']
    nb = lib.v3d_segment_csr_workspace_bytes(n)
    ws = a.ws('segcsr', nb)
    ids, src = a.put('ids', i['ids']), a.put('src', i['src'])
    perm, offs = a.out('perm', (n,), torch.int32), a.out('offsets', (n_seg + 1,), torch.int32)
    pool = a.out('pool', (n_seg, N), torch.float32)
    assert lib.v3d_segment_csr(p(ids), n, n_seg, p(perm), p(offs), p(ws), nb, a.stream()) == OK
    assert lib.v3d_segment_max_f32(p(src), N + 4, p(perm), p(offs), n_seg, N, p(pool), N, a.stream()) == OK
    return ()


def _segment_check(i, out, status):
    ids = i['ids']
    assert np.array_equal(out['perm'].numpy(), np.argsort(ids, kind='stable'))
    counts = np.bincount(ids, minlength=i['n_seg'])
    assert (counts == 0).sum() > i['n_seg'] // 8 and counts[-1] == 0           # segments with no rows, the last one among them
    assert np.array_equal(out['offsets'].numpy(), np.concatenate(([0], np.cumsum(counts))))
    ref = np.full((i['n_seg'], i['N']), -np.inf, dtype=np.float32)
    np.maximum.at(ref, ids, i['src'][:, :i['N']])
    assert np.array_equal(out['pool'].numpy(), ref)


CASES.append(Case(
    'segment_csr_max', ('v3d_segment_csr', 'v3d_segment_max_f32'), _segment_make, _segment_run, _segment_check,
    bound='stable argsort / bincount / maximum.at, exact (the scatter-max of oracle.scene.pointnet is exact too)',
    sections=lambda lib, i: {'segcsr': lib.v3d_segment_csr_workspace_bytes(i['n'])},
    groups=lambda i: [('iota_kernel', i['n'], 256), ('segment_offsets_kernel', i['n_seg'] + 1, 256), ('segment_max_kernel<32>', i['n_seg'], 8)],
    constants=(('iota_kernel<<<(n + 255) / 256, 256', 'segment.hip:212'), ('segment_offsets_kernel<<<(n_seg + 1 + 255) / 256, 256', 'segment.hip:218'),
               ('if (N <= 128) kernel32<<<(rows + 7) / 8, 256', 'segment.hip:178')), paired=True))


# ---- v3d_voxel_keys -> v3d_sort_unique_u64 -> v3d_lower_bound_u64 -> v3d_voxel_decode -> v3d_voxelize_status ------------------------

def _voxel_make(size):
    n = {'small': 600, 'big': 1300, 'rejected': 600}[size]
    rng = np.random.default_rng(20 + n)
    pts = (rng.random((n, 3)) * np.array([2.0, 1.5, 1.0]) * (1 if size == 'small' else 1.3)).astype(np.float32)
    batch = rng.integers(0, 3, n).astype(np.int64)
    if size == 'rejected':
        batch[17] = 1024                                                       # batch id out of range (voxelize.hip:23 kMaxBatch)
    return dict(pts=pts, batch=batch, n=n, edge_len=0.1)                       # > 256 occupied voxels: two workgroups in decode


def _n_voxels(i):
    from oracle import scene as osc
    return int(osc.voxelize(torch.from_numpy(i['pts']), torch.from_numpy(np.minimum(i['batch'], 2)), i['edge_len'])[0].shape[0])


def _voxel_run(lib, a, i):
    n, el, s = i['n'], i['edge_len'], a.stream()
    wb, sb = lib.v3d_voxelize_workspace_bytes(), lib.v3d_sort_unique_workspace_bytes(n)
    ws, sws = a.ws('voxelize', wb), a.ws('sort_unique', sb)
    pts, batch = a.put('pts', i['pts']), a.put('batch', i['batch'])
    keys, uniq, inv = a.out('keys', (n,), torch.int64), a.out('unique_keys', (n,), torch.int64), a.out('inverse', (n,), torch.int64)
    assert lib.v3d_voxel_keys(p(pts), p(batch), n, el, p(keys), p(ws), wb, s) == OK
    cnt = ctypes.c_int(-1)
    assert lib.v3d_sort_unique_u64(p(keys), n, p(uniq), ctypes.byref(cnt), p(sws), sb, s) == OK
    nv = cnt.value
    a.length('unique_keys', nv)
    rc = lib.v3d_voxelize_status(p(ws), wb, s)
    if rc == OK:
        assert lib.v3d_lower_bound_u64(p(uniq), nv, p(keys), n, p(inv), s) == OK
        apts, aidx, ab = a.out('anchor_pts', (n, 3), torch.float32), a.out('anchor_idx3d', (n, 3), torch.int32), a.out('anchor_batch', (n,), torch.int64)
        assert lib.v3d_voxel_decode(p(uniq), nv, el, el / 2., p(apts), p(aidx), p(ab), p(ws), wb, s) == OK
        for name in ('anchor_pts', 'anchor_idx3d', 'anchor_batch'):
            a.length(name, nv)
        rc = lib.v3d_voxelize_status(p(ws), wb, s)
    return (rc, nv)


def _voxel_check(i, out, status):
    from oracle import scene as osc
    a_pts, a_idx, a_batch, a_edges = osc.voxelize(torch.from_numpy(i['pts']), torch.from_numpy(i['batch']), i['edge_len'])
    assert status == (OK, a_pts.shape[0]) and a_pts.shape[0] > 256
    assert torch.equal(out['anchor_idx3d'].to(a_idx.dtype), a_idx) and torch.equal(out['anchor_batch'], a_batch)
    assert torch.equal(out['inverse'], a_edges[0])
    np.testing.assert_allclose(out['anchor_pts'].numpy(), a_pts.numpy(), rtol=0, atol=1e-6)


CASES.append(Case(
    'voxelize_chain', ('v3d_voxel_keys', 'v3d_sort_unique_u64', 'v3d_lower_bound_u64', 'v3d_voxel_decode', 'v3d_voxelize_status'),
    _voxel_make, _voxel_run, _voxel_check,
    bound='oracle.scene.voxelize: integer outputs exact, anchor points 1e-6 (tests/test_scene_gpu.py::test_voxelize_exact_multiple_quirk_and_multibatch)',
    sections=lambda lib, i: {'sort_unique': lib.v3d_sort_unique_workspace_bytes(i['n'])},   # the voxelize metadata block has one fixed size
    groups=lambda i: [('bbox_partial / voxel_keys / lower_bound', i['n'], 256), ('voxel_decode_kernel', _n_voxels(i), 256)],
    constants=(('voxel_keys_kernel<<<(n + 255) / 256, 256', 'voxelize.hip:288'), ('voxel_decode_kernel<<<(n_unique + 255) / 256, 256', 'voxelize.hip:317'),
               ('kMaxBatch = 1024', 'voxelize.hip:23')), rejected='rejected', paired=True))


# ---- v3d_hash_build -> v3d_sparse_neighbors / v3d_sparse_interp_f32 -> v3d_hash_status ----------------------------------------------

def _hash_make(size):
    import sparse_oracle as so                                                 # noqa: F401
    n, n_pts, n_hyp = {'small': (300, 100, 3), 'big': (1100, 220, 3), 'rejected': (300, 100, 3)}[size]
    rng = np.random.default_rng(30 + n)
    side = 8 if n <= 300 else 11
    g = np.stack(np.meshgrid(np.arange(2), np.arange(side), np.arange(side), np.arange(side), indexing='ij'), -1).reshape(-1, 4)
    coords = g[rng.choice(g.shape[0], n, replace=False)].astype(np.int64)
    coords[:, 1:] -= 2
    if size == 'rejected':
        coords[5, 2] = 65520                                                   # coordinate outside the key range [-8, 65519]
    min_pts = rng.uniform(-1, 1, (2, 3)).astype(np.float32)
    pb = rng.integers(0, 2, n_pts).astype(np.int64)
    res = 0.04
    pts = (min_pts[pb][:, None, :] + rng.uniform(-3.5, side, (n_pts, n_hyp, 3)) * res).astype(np.float32)
    return dict(coords=coords, n=n, feats=rng.standard_normal((n, 32)).astype(np.float32), min_pts=min_pts, res=res, pts=pts,
                pts_batch=pb, n_pts=n_pts, n_hyp=n_hyp)


def _hash_run(lib, a, i):
    n, n_pts, n_hyp, s = i['n'], i['n_pts'], i['n_hyp'], a.stream()
    tb, wb = lib.v3d_hash_bytes(n), lib.v3d_sparse_interp_workspace_bytes(n_pts, n_hyp)
    table, ws = a.ws('table', tb), a.ws('interp', wb)
    c = a.put('coords', i['coords'], torch.int32)
    assert lib.v3d_hash_build(p(c), n, p(table), tb, s) == OK
    nbr = a.out('nbr', (27, n), torch.int32)
    assert lib.v3d_sparse_neighbors(p(table), n, p(c), n, 1, p(nbr), s) == OK
    out = a.out('interp', (n_pts * n_hyp, 32), torch.float32)
    f, pts, pb, mn = a.put('f', i['feats']), a.put('pts', i['pts']), a.put('pb', i['pts_batch']), a.put('mn', i['min_pts'])
    assert lib.v3d_sparse_interp_f32(p(table), n, p(f), 32, 1, p(pts), p(pb), n_pts, n_hyp, p(mn), i['res'], p(out), 32, 0, p(ws), wb, s) == OK
    return (lib.v3d_hash_status(p(table), n, s),)


def _hash_check(i, out, status):
    import sparse_oracle as so
    assert status == (OK,)
    assert np.array_equal(out['nbr'].numpy().astype(np.int64), so.neighbours(i['coords'], i['coords'], 1))
    val, s = so.interp(i['coords'], i['feats'], 1, i['pts'], i['pts_batch'], i['n_hyp'], i['min_pts'], i['res'])
    got = out['interp'].numpy().astype(np.float64)
    assert np.isfinite(got).all() and (s > 0).any() and (s == 0).any()
    bad = np.abs(got - val) > so.INTERP_BOUND * s
    assert not bad.any(), 'interp: %d elements outside 9 u S, first at %s' % (bad.sum(), np.argwhere(bad)[0])


CASES.append(Case(
    'hash_chain', ('v3d_hash_build', 'v3d_sparse_neighbors', 'v3d_sparse_interp_f32', 'v3d_hash_status'),
    _hash_make, _hash_run, _hash_check,
    bound='sparse_oracle.neighbours exact, sparse_oracle.interp within 9 u S (tests/test_sparse_gpu.py::test_interp_generic_queries_within_nine_u_s)',
    sections=lambda lib, i: {'table': lib.v3d_hash_bytes(i['n']), 'interp': lib.v3d_sparse_interp_workspace_bytes(i['n_pts'], i['n_hyp'])},
    groups=lambda i: [('hash_insert / neighbors', i['n'], 256), ('interp_corners_kernel', i['n_pts'] * i['n_hyp'] * 8, 256)],
    constants=(('hash_insert_kernel<<<(n + 255) / 256, 256', 'sparse.hip:74'),
               ('interp_corners_kernel<true><<<(unsigned)((nq * 8 + 255) / 256), 256', 'sparse_interp.hip:271')), rejected='rejected',
    paired=True))


# ---- v3d_fuse_depths_f32 -> v3d_fusion_compact (one workspace, include/v3d.h) ------------------------------------------------------

def _fusion_make(size):
    import fusion_oracle as fo
    n, hw = {'small': (3, (12, 20)), 'big': (5, (24, 40))}[size]
    d, img, poses, K = fo.scene(n, hw, seed=12, yaw_step_deg=2, sigma=0.01)
    cams = v3d('fusion').camera_blocks(poses, K)
    return dict(depths=d.numpy(), images=img.numpy(), poses=poses, K=K, cams=cams.numpy(), n=n, h=hw[0], w=hw[1], z_thresh=0.1, n_thresh=2)


def _fusion_run(lib, a, i):
    n, h, w, s = i['n'], i['h'], i['w'], a.stream()
    hw = h * w
    nb = lib.v3d_fusion_workspace_bytes(n, h, w)
    ws = a.ws('fusion', nb)
    d, cams, img = a.put('d', i['depths']), a.put('cams', i['cams']), a.put('img', i['images'].reshape(n, hw, 3))
    pts, n_valid = a.out('pts', (n, hw, 3), torch.float32), a.out('n_valid', (n, hw), torch.int32)
    assert lib.v3d_fuse_depths_f32(p(d), p(cams), n, h, w, None, n, None, None, i['z_thresh'], p(pts), p(n_valid), p(ws), nb, s) == OK
    valid, vcount, vofs = a.out('all_valid', (n, h, w), torch.uint8), a.out('view_count', (n,), torch.int32), a.out('view_ofs', (n + 1,), torch.int32)
    out_pts, out_rgb, total = a.out('out_pts', (n * hw, 3), torch.float32), a.out('out_rgb', (n * hw, 3), torch.uint8), a.out('total', (1,), torch.int32)
    assert lib.v3d_fusion_compact(p(n_valid), p(pts), p(img), 3, n, h, w, i['n_thresh'], p(valid), p(vcount), p(vofs), p(out_pts), p(out_rgb),
                                  p(total), p(ws), nb, s) == OK
    torch.cuda.synchronize()
    m = int(total.item())
    a.length('out_pts', m)
    a.length('out_rgb', m)
    return (m,)


def _fusion_check(i, out, status):
    import fusion_oracle as fo
    from test_fusion_gpu import YARDSTICK, compare
    res = fo.check_scene(torch.from_numpy(i['depths']), i['poses'], i['K'], i['z_thresh'], i['n_thresh'])
    compare('workspace contract', res, out['pts'], out['n_valid'], out['all_valid'].bool().reshape(i['n'], -1), 4 * YARDSTICK)
    keep = out['n_valid'].reshape(i['n'], -1) >= i['n_thresh']
    assert torch.equal(out['all_valid'].reshape(i['n'], -1).bool(), keep) and status == (int(keep.sum()),) and status[0] > 0
    per_view = keep.sum(1)
    assert torch.equal(out['view_count'].long(), per_view)
    assert torch.equal(out['view_ofs'].long(), torch.cat((torch.zeros(1).long(), per_view.cumsum(0))))
    assert torch.equal(out['out_pts'], out['pts'][keep]) and torch.equal(out['out_rgb'], torch.from_numpy(i['images']).reshape(i['n'], -1, 3)[keep])


CASES.append(Case(
    'fusion_chain', ('v3d_fuse_depths_f32', 'v3d_fusion_compact'), _fusion_make, _fusion_run, _fusion_check,
    bound='fusion_oracle.check_scene through test_fusion_gpu.compare at 4 x the reference\'s own error; compaction exact',
    sections=lambda lib, i: {'fusion': lib.v3d_fusion_workspace_bytes(i['n'], i['h'], i['w'])},
    groups=lambda i: [('fuse_depths / compact tiles (per view)', i['h'] * i['w'], 256, i['n'])],
    constants=(('kTile = 256', 'fusion.hip:28'),), paired=True))


# ---- the cloud metrics ---------------------------------------------------------------------------------------------------------------

def _down_make(size):
    import cloud_oracle as co
    n = {'small': 700, 'big': 3000, 'rejected': 700}[size]
    rng = np.random.default_rng(40 + n)
    return dict(pts=co.room(n, 0.01, seed=n), attr=rng.random((n, 3)).astype(np.float32), n=n, voxel=-0.1 if size == 'rejected' else 0.1)


def _down_run(lib, a, i):
    n, s = i['n'], a.stream()
    nb = lib.v3d_cloud_downsample_workspace_bytes(n)
    ws = a.ws('downsample', nb)
    pts, attr = a.put('pts', i['pts']), a.put('attr', i['attr'])
    op, oa, oc = a.out('out_pts', (n, 3), torch.float32), a.out('out_attr', (n, 3), torch.float32), a.out('out_count', (1,), torch.int32)
    assert lib.v3d_cloud_downsample_f32(p(pts), p(attr), 3, n, None, i['voxel'], p(op), p(oa), p(oc), p(ws), nb, s) == OK
    m = ctypes.c_int(-7)
    rc = lib.v3d_cloud_status(p(ws), nb, ctypes.byref(m), s)
    a.length('out_pts', m.value)
    a.length('out_attr', m.value)
    return (rc, m.value)


def _down_check(i, out, status):
    import cloud_oracle as co
    from test_metrics3d_gpu import _compare_down
    ref = co.voxel_down_sample(i['pts'], i['voxel'], i['attr'])
    assert status == (OK, len(ref['keys'])) and status[1] > 256
    _compare_down('workspace contract', (out['out_pts'], out['out_attr'], out['out_count'][0]), ref)


CASES.append(Case(
    'cloud_downsample', ('v3d_cloud_downsample_f32', 'v3d_cloud_status'), _down_make, _down_run, _down_check,
    bound='cloud_oracle.voxel_down_sample within 1 ulp (test_metrics3d_gpu._compare_down)',
    sections=lambda lib, i: {'downsample': lib.v3d_cloud_downsample_workspace_bytes(i['n'])},
    groups=lambda i: [('ds_keys / ds_heads / ds_reduce', i['n'], 256)], constants=(('ds_keys_kernel<<<grid, 256', 'cloudmetrics.hip:506'),),
    rejected='rejected', paired=True))


def _nn_make(size):
    import cloud_oracle as co
    nt, nq = {'small': (700, 300), 'big': (3000, 1000), 'no_target': (0, 300), 'no_query': (700, 0)}[size]
    return dict(target=co.room(max(nt, 1), 0.01, seed=50 + nt)[:nt], query=co.room(max(nq, 1), 0.02, seed=60 + nq)[:nq], nt=nt, nq=nq)


def _nn_run(lib, a, i):
    nt, nq = i['nt'], i['nq']
    nb = lib.v3d_nn_workspace_bytes(nt, nq)
    ws = a.ws('nn', nb)
    t, q = a.put('t', i['target'].reshape(-1, 3)), a.put('q', i['query'].reshape(-1, 3))
    idx, dist = a.out('idx', (max(nq, 1),), torch.int32), a.out('dist', (max(nq, 1),), torch.float32)
    assert lib.v3d_nn_query_f32(p(t), nt, p(q), nq, p(idx), p(dist), p(ws), nb, a.stream()) == OK
    if nq:
        return ()
    # n_query == 0: nothing is done (include/v3d.h): the one-element outputs still hold the arena's bytes; no row is valid
    torch.cuda.synchronize()
    untouched = tuple(bool((as_bytes(t_).cpu() == a.poison).all()) for t_ in (idx, dist))
    a.length('idx', 0)
    a.length('dist', 0)
    return untouched


def _nn_check(i, out, status):
    import cloud_oracle as co
    if i['nq'] == 0:
        assert status == (True, True), 'n_query == 0 wrote idx / dist: %r' % (status,)
        return
    if i['nt'] == 0:
        assert (out['idx'] == -1).all() and torch.isposinf(out['dist']).all()
        return
    co.check_nn('workspace contract', i['target'], i['query'], out['idx'].numpy(), out['dist'].numpy(), co.nearest(i['target'], i['query']))


CASES.append(Case(
    'nn_query', ('v3d_nn_query_f32',), _nn_make, _nn_run, _nn_check,
    bound='cloud_oracle.check_nn: distances within 4 u, indices equal where the gap is clear',
    sections=lambda lib, i: {'nn': lib.v3d_nn_workspace_bytes(i['nt'], i['nq'])},
    groups=lambda i: [('nn_codes / nn_gather (target)', i['nt'], 256), ('nn_codes / nn_query (query)', i['nq'], 256)],
    constants=(('nn_codes_kernel<<<tgrid, 256', 'cloudmetrics.hip:573'),
               ('nn_query_kernel<<<qgrid, 256', 'cloudmetrics.hip:587')), extra=('no_target', 'no_query')))


def _cm_make(size):
    n_p, n_t = {'small': (300, 700), 'big': (1000, 3000), 'no_pred': (0, 700), 'no_target': (300, 0)}[size]
    rng = np.random.default_rng(70 + n_p + n_t)
    return dict(dp=(rng.random(n_p) * 0.1).astype(np.float32), dt=(rng.random(n_t) * 0.1).astype(np.float32), thr=0.05)


def _cm_run(lib, a, i):
    nb = lib.v3d_cloud_metrics_workspace_bytes()
    ws = a.ws('cloud_metrics', nb)
    pad = lambda x: x if x.size else np.zeros(1, np.float32)                   # noqa: E731  (an empty array still needs an address)
    dp, dt = a.put('dp', pad(i['dp'])), a.put('dt', pad(i['dt']))
    out = a.out('out', (5,), torch.float64)
    assert lib.v3d_cloud_metrics_f64(p(dp), i['dp'].size, p(dt), i['dt'].size, i['thr'], p(out), p(ws), nb, a.stream()) == OK
    return ()


def _cm_check(i, out, status):
    import cloud_oracle as co
    rec = out['out'].numpy()
    if i['dp'].size and i['dt'].size:
        co.check_metrics('workspace contract', rec.tolist(), i['dp'].astype(np.float64), i['dt'].astype(np.float64), i['thr'])
    else:                                                                      # an empty array gives NaN, as NumPy's mean does
        want = co.metrics(i['dp'], i['dt'], i['thr'])
        for k, key in enumerate(co.KEYS):
            assert np.isnan(rec[k]) == np.isnan(want[key]) and (np.isnan(rec[k]) or abs(rec[k] - want[key]) <= co.DIST_BOUND * abs(want[key])), key
        assert np.isnan(rec).any()


CASES.append(Case(
    'cloud_metrics', ('v3d_cloud_metrics_f64',), _cm_make, _cm_run, _cm_check,
    bound='cloud_oracle.check_metrics: means within 4 u, shares within the distances near the threshold',
    sections=lambda lib, i: {'cloud_metrics': lib.v3d_cloud_metrics_workspace_bytes()}, fixed=('cloud_metrics',),
    groups=lambda i: [('metrics_partial_kernel (grid-stride over 256 workgroups)', i['dp'].size, 256)],
    constants=(('kRedBlocks = 256', 'cloudmetrics.hip:33'),
               ('metrics_partial_kernel<<<dim3(kRedBlocks, 2), 256', 'cloudmetrics.hip:605')), extra=('no_pred', 'no_target')))


# ---- 2D metrics and supervision -------------------------------------------------------------------------------------------------------

_M2D_SHAPES = {'small': (2, 40, 50), 'big': (3, 97, 99)}                        # big: two slices, a partial last group of 8, gt[1:]


def _m2d_make(size):
    import metrics2d_oracle as mo
    n, H, W = _M2D_SHAPES[size]
    pred, gt = mo.scene(n, H, W, H, W, seed=80 + n)
    return dict(pred=pred, gt=gt, n=n, H=H, W=W, shift=int(size == 'big'))


def _shifted(a, name, array, shift):
    """the array on the device `shift` elements behind the alignment torch gives -> (keep-alive tensor, address)"""
    flat = np.concatenate((np.zeros(shift, array.dtype), array.reshape(-1)))
    t = a.put(name, flat)
    return t, t.data_ptr() + shift * array.itemsize


def _m2d_run(lib, a, i):
    n, H, W = i['n'], i['H'], i['W']
    nb = lib.v3d_depth_metrics_workspace_bytes(n, H, W)
    ws = a.ws('depth_metrics', nb)
    pred = a.put('pred', i['pred'])
    _, gt_p = _shifted(a, 'gt', i['gt'], i['shift'])
    counts, per, mean = a.out('counts', (n, 5), torch.int32), a.out('per_image', (n, 9), torch.float64), a.out('mean', (9,), torch.float64)
    assert lib.v3d_depth_metrics_2d(p(pred), H, W, None, None, gt_p, 0, None, 2, n, H, W, p(counts), p(per), p(mean), p(ws), nb, a.stream()) == OK
    return ()


def _m2d_check(i, out, status):
    import metrics2d_oracle as mo
    from test_metrics2d_gpu import assert_record
    assert_record({k: v.numpy() for k, v in out.items()}, mo.check(i['pred'], i['gt'], derive_valid=True), 'workspace contract')


def _slices(i, hw):
    return [('slice kernel: slices of kSlice pixels per image', hw, 8192, i['n'])]


CASES.append(Case(
    'depth_metrics_2d', ('v3d_depth_metrics_2d',), _m2d_make, _m2d_run, _m2d_check,
    bound='metrics2d_oracle.check through test_metrics2d_gpu.assert_record: counts and fp32 columns exact, float64 columns 1e-10',
    sections=lambda lib, i: {'depth_metrics': lib.v3d_depth_metrics_workspace_bytes(i['n'], i['H'], i['W'])},
    groups=lambda i: _slices(i, i['H'] * i['W']), rule_on='big',
    constants=(('kSlice = 8192', 'depth2d.h:38'), ('kGroup = 8', 'depth2d.h:39'))))


def _sup_make(size):
    import supervision_oracle as sup
    n, H, W = _M2D_SHAPES[size]
    pred, gt = sup.scene(n, H, W, H, W, seed=90 + n)
    return dict(pred=pred, gt=gt, n=n, H=H, W=W, shift=int(size == 'big'), interval=0.05)


def _sup_run(lib, a, i):
    n, H, W = i['n'], i['H'], i['W']
    nb = lib.v3d_depth_supervision_workspace_bytes(n, H, W)
    ws = a.ws('supervision', nb)
    pred = a.put('pred', i['pred'])
    _, gt_p = _shifted(a, 'gt', i['gt'], i['shift'])
    counts, per, mean = a.out('counts', (n, 6), torch.int32), a.out('per_image', (n, 10), torch.float64), a.out('mean', (10,), torch.float64)
    assert lib.v3d_depth_supervision_f32(p(pred), n, H, W, gt_p, H, W, None, None, i['interval'], p(counts), p(per), p(mean), p(ws), nb,
                                         a.stream()) == OK
    return ()


def _sup_check(i, out, status):
    import supervision_oracle as sup
    from test_supervision_gpu import assert_record
    assert_record({k: v.numpy() for k, v in out.items()}, sup.check(i['pred'], i['gt'], i['interval']), 'workspace contract')


CASES.append(Case(
    'depth_supervision', ('v3d_depth_supervision_f32',), _sup_make, _sup_run, _sup_check,
    bound='supervision_oracle.check through test_supervision_gpu.assert_record: counts and fp32 columns exact, float64 columns 1e-10',
    sections=lambda lib, i: {'supervision': lib.v3d_depth_supervision_workspace_bytes(i['n'], i['H'], i['W'])},
    groups=lambda i: _slices(i, i['H'] * i['W']), rule_on='big',
    constants=(('kSlice = 8192', 'depth2d.h:38'), ('kGroup = 8', 'depth2d.h:39'))))


# ---- order statistics -------------------------------------------------------------------------------------------------------------------

_QS = (1 - .995, .5, .995)


def _q_host():
    return (ctypes.c_double * len(_QS))(*_QS)


def _cos_make(size):
    n = {'small': 300, 'big': 5000}[size]
    rng = np.random.default_rng(100 + n)
    pts = (rng.standard_normal((n, 3)) * 3).astype(np.float32)
    pts[7, 1] = np.nan                                                          # a dropped row
    return dict(pts=pts, n=n)


def _cos_run(lib, a, i):
    nb = lib.v3d_order_stats_workspace_bytes(len(_QS))
    ws = a.ws('order_stats', nb)
    pts = a.put('pts', i['pts'])
    count, stats = a.out('count', (1,), torch.int32), a.out('stats', (len(_QS), 3, 2), torch.float32)
    assert lib.v3d_cloud_order_stats_f32(p(pts), i['n'], _q_host(), len(_QS), p(count), p(stats), p(ws), nb, a.stream()) == OK
    return ()


def _os_check(pts, out):
    import order_stats_oracle as oo
    want_n, want = oo.order_stats(pts, _QS)
    assert int(out['count'][0]) == want_n and want_n > 0 and oo.same_bits(out['stats'].numpy(), want)


CASES.append(Case(
    'cloud_order_stats', ('v3d_cloud_order_stats_f32',), _cos_make, _cos_run, lambda i, out, status: _os_check(i['pts'], out),
    bound='order_stats_oracle.order_stats, identical bits (tests/test_order_stats_gpu.py::check)',
    sections=lambda lib, i: {'order_stats': lib.v3d_order_stats_workspace_bytes(len(_QS))}, fixed=('order_stats',),
    groups=lambda i: [('order_stats_pass_kernel', i['n'], 2048)], rule_on='big',
    constants=(('kTile = kThreads * kPerThread;  // 2048 points', 'order_stats.hip:37'),)))


def _bos_make(size):
    import fusion_oracle as fo
    import order_stats_oracle as oo
    n, hw = {'small': (2, (10, 15)), 'big': (3, (37, 53))}[size]
    d, _, poses, K = fo.scene(n, hw, seed=77, yaw_step_deg=None, sigma=0.04)
    return dict(depths=d.numpy().copy(), Pi=oo.inverse_projections(K.numpy(), poses.numpy()), n=n, h=hw[0], w=hw[1])


def _bos_run(lib, a, i):
    nb = lib.v3d_order_stats_workspace_bytes(len(_QS))
    ws = a.ws('order_stats', nb)
    d, Pi = a.put('d', i['depths']), a.put('Pi', i['Pi'])
    count, stats = a.out('count', (1,), torch.int32), a.out('stats', (len(_QS), 3, 2), torch.float32)
    assert lib.v3d_backproject_order_stats_f32(p(d), p(Pi), i['n'], i['h'], i['w'], _q_host(), len(_QS), p(count), p(stats), p(ws), nb,
                                               a.stream()) == OK
    return ()


def _bos_check(i, out, status):
    import order_stats_oracle as oo
    _os_check(oo.backproject(i['depths'], i['Pi']), out)


CASES.append(Case(
    'backproject_order_stats', ('v3d_backproject_order_stats_f32',), _bos_make, _bos_run, _bos_check,
    bound='order_stats_oracle.backproject + order_stats, identical bits (tests/test_order_stats_gpu.py::check)',
    sections=lambda lib, i: {'order_stats': lib.v3d_order_stats_workspace_bytes(len(_QS))}, fixed=('order_stats',),
    groups=lambda i: [('order_stats_pass_kernel', i['n'] * i['h'] * i['w'], 2048)], rule_on='big',
    constants=(('kTile = kThreads * kPerThread;  // 2048 points', 'order_stats.hip:37'),)))


# ---- TSDF: normalise, marching cubes, rendering, resampling (no workspace but whole output arrays, or count -> extract) -------------

_VOL = {'small': (10, 9, 11), 'big': (20, 18, 22)}


def _volume(size, seed):
    from test_tsdf_transform_gpu import seeded
    return seeded(_VOL[size], seed)


def _norm_make(size):
    tsdf_vol, vols = _volume(size, 3)
    weight = vols['weight']
    return dict(tsdf=(tsdf_vol * np.maximum(weight, 1)).astype(np.float32), weight=weight, color=vols['color'] * np.maximum(weight, 1)[None],
                n_vox=int(weight.size))


def _norm_run(lib, a, i):
    n = i['n_vox']
    t, w, c = a.put('t', i['tsdf']), a.put('w', i['weight']), a.put('c', i['color'].astype(np.float32))
    to, co = a.out('tsdf_out', (n,), torch.float32), a.out('color_out', (3, n), torch.float32)
    assert lib.v3d_tsdf_normalize_f32(p(t), p(w), p(c), n, p(to), p(co), a.stream()) == OK
    return ()


def _norm_check(i, out, status):
    w = i['weight'].reshape(-1)
    seen = w > 0
    assert seen.any() and (~seen).any()
    with np.errstate(all='ignore'):
        t, c = i['tsdf'].reshape(-1), i['color'].astype(np.float32).reshape(3, -1)
        assert np.array_equal(out['tsdf_out'].numpy(), np.where(seen, t / w, t))
        assert np.array_equal(out['color_out'].numpy(), np.where(seen[None], c / w[None], c))


CASES.append(Case(
    'tsdf_normalize', ('v3d_tsdf_normalize_f32',), _norm_make, _norm_run, _norm_check,
    bound='one IEEE fp32 division per element, exact (the header\'s definition; tsdf.hip: div_rn)',
    sections=lambda lib, i: {}, groups=lambda i: [('tsdf_normalize_kernel', i['n_vox'], 256)], constants=(('kTile = 256', 'tsdf.hip:31'),)))


def _mesh_make(size):
    tsdf_vol, vols = _volume(size, 5)
    return dict(tsdf=tsdf_vol, color=vols['color'], dim=_VOL[size], voxel_size=0.04, origin=[0.25, -1.5, 3.0])


def _mesh_run(lib, a, i):
    nx, ny, nz = i['dim']
    s = a.stream()
    nb = lib.v3d_mesh_workspace_bytes(nx, ny, nz)
    ws = a.ws('mesh', nb)
    t, c = a.put('t', i['tsdf']), a.put('c', i['color'])
    counts = a.out('counts', (2,), torch.int32)
    assert lib.v3d_mesh_count_f32(p(t), nx, ny, nz, 0, p(counts), p(ws), nb, s) == OK
    torch.cuda.synchronize()
    n_v, n_f = (int(v) for v in counts.cpu())
    assert 0 <= n_v <= 3 * nx * ny * nz and 0 <= n_f <= 5 * nx * ny * nz, (n_v, n_f)
    verts, cols, tris = a.out('verts', (n_v, 3), torch.float32), a.out('colors', (n_v, 3), torch.uint8), a.out('tris', (n_f, 3), torch.int32)
    _, org = host_f32(i['origin'])
    assert lib.v3d_mesh_extract_f32(p(t), p(c), nx, ny, nz, i['voxel_size'], org, 0, p(verts), p(cols), n_v, p(tris), n_f, p(ws), nb, s) == OK
    return (n_v, n_f)


def _mesh_check(i, out, status):
    import mesh_oracle as mo
    want = mo.get_mesh(i['tsdf'], i['color'], i['voxel_size'], i['origin'])
    assert status == (want['vertices'].shape[0], want['triangles'].shape[0]) and status[1] > 256
    assert np.array_equal(out['tris'].numpy(), want['triangles']) and np.array_equal(out['colors'].numpy(), want['colors'])
    assert np.array_equal(out['verts'].numpy().view(np.uint32), want['vertices'].view(np.uint32))


CASES.append(Case(
    'mesh_count_extract', ('v3d_mesh_count_f32', 'v3d_mesh_extract_f32'), _mesh_make, _mesh_run, _mesh_check,
    bound='mesh_oracle.get_mesh: triangles and colours exact, vertices bit-equal to the fp32 restatement (test_mesh_gpu.check_positions)',
    sections=lambda lib, i: {'mesh': lib.v3d_mesh_workspace_bytes(*i['dim'])},
    groups=lambda i: [('mc_classify / mc_tricount / mc_emit', int(np.prod(i['dim'])), 256)], constants=(('kTile = 256', 'mesh.hip:42'),),
    paired=True))


def _render_make(size):
    import meshtodepth_oracle as mo
    from test_meshtodepth_oracle import projections
    n, h, w = {'small': (2, 12, 20), 'big': (3, 24, 40), 'rejected': (2, 12, 20)}[size]
    v, f = mo.icosphere(2, 1.0, (0.1, -0.05, 0.2))                              # 320 triangles
    if size == 'big':
        v, f = mo.merge((v, f), mo.icosphere(2, 0.6, (-0.9, 0.4, 0.5)))          # 640
    if size == 'rejected':
        f = np.concatenate((f[:40], [[0, 1, v.shape[0]]], f[40:])).astype(np.int32)   # a triangle index out of range
    K = np.repeat(mo.intrinsics(0.9 * w, 0.85 * w, w / 2 - 0.3, h / 2 + 0.2)[None], n, axis=0)
    return dict(verts=v, tris=f, P=projections(K, mo.orbit(n, 3.0, (0.1, -0.05, 0.2))), n=n, h=h, w=w)


def _render_run(lib, a, i):
    v, f, P = a.put('v', i['verts']), a.put('f', i['tris']), a.put('P', i['P'].astype(np.float32))
    depth, status = a.out('depth', (i['n'], i['h'], i['w']), torch.float32), a.out('status', (1,), torch.int32)
    assert lib.v3d_mesh_render_depth_f32(p(v), v.shape[0], p(f), f.shape[0], p(P), i['n'], i['h'], i['w'], .5, .05, 100., p(depth), p(status),
                                         a.stream()) == OK
    torch.cuda.synchronize()
    return (int(status.item()),)


def _render_check(i, out, status):
    import meshtodepth_oracle as mo
    from test_meshtodepth_gpu import check
    assert status == (0,)
    check('workspace contract', out['depth'].numpy(), mo.render32(i['verts'], i['tris'], i['P'], i['h'], i['w']),
          mo.render64(i['verts'], i['tris'], i['P'], i['h'], i['w']))
    assert (out['depth'] > 0).any() and (out['depth'] == 0).any()


CASES.append(Case(
    'mesh_render_depth', ('v3d_mesh_render_depth_f32',), _render_make, _render_run, _render_check,
    bound='meshtodepth_oracle.render32 bit for bit and render64 within its bound (test_meshtodepth_gpu.check)',
    sections=lambda lib, i: {}, groups=lambda i: [('mesh_render_kernel (triangles)', i['tris'].shape[0], 256),
                                                   ('fill / resolve (pixels)', i['n'] * i['h'] * i['w'], 256)],
    constants=(('kBlock = 256', 'meshrender.hip:34'),), rejected='rejected'))


def _resample_make(size):
    from test_tsdf_transform_gpu import rotation
    src = _VOL[size]
    dst = tuple(d + 1 for d in src)
    tsdf_vol, vols = _volume(size, 7)
    vox, so_, do_ = 0.04, (0.3, -1.1, 0.7), (0.24, -1.02, 0.62)
    return dict(tsdf=tsdf_vol, color=vols['color'], semseg=vols['semseg'], label16=vols['label16'], src=src, dst=dst, vox=vox, src_origin=so_,
                dst_origin=do_, M=rotation(src, vox, so_, (0.013, -0.009, 0.017)))


def _grid_args(i):
    keep = [host_f32(i['src_origin']), host_f32(np.asarray(i['M']).reshape(-1)), host_f32(i['dst_origin'])]
    return keep, (i['src'][0], i['src'][1], i['src'][2], i['vox'], keep[0][1], keep[1][1], 0, i['dst'][0], i['dst'][1], i['dst'][2], keep[2][1])


def _plan(i):
    import tsdf_transform_oracle as oracle
    return oracle, oracle.plan(i['src'], i['vox'], i['src_origin'], i['M'], False, i['dst'], i['dst_origin'], np.float32)


def _resample_run(lib, a, i):
    n = int(np.prod(i['dst']))
    t, c = a.put('t', i['tsdf']), a.put('c', i['color'])
    to, co = a.out('tsdf_dst', (n,), torch.float32), a.out('attr_dst', (3, n), torch.float32)
    keep, grid = _grid_args(i)
    assert lib.v3d_tsdf_resample_f32(p(t), p(c), 3, *grid, p(to), p(co), a.stream()) == OK
    return ()


def _resample_check(i, out, status):
    oracle, p32 = _plan(i)
    assert 0.05 < p32['outside'].mean() < 0.95
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)                     # noqa: E731
    assert np.array_equal(bits(out['tsdf_dst'].numpy()), bits(oracle.tsdf(p32, i['tsdf']).reshape(-1)))
    assert np.array_equal(bits(out['attr_dst'].numpy()), bits(oracle.trilinear(p32, i['color']).reshape(3, -1)))


CASES.append(Case(
    'tsdf_resample', ('v3d_tsdf_resample_f32',), _resample_make, _resample_run, _resample_check,
    bound='tsdf_transform_oracle fp32 restatement, bit identity (test_tsdf_transform_gpu.assert_equals_restatement)',
    sections=lambda lib, i: {}, groups=lambda i: [('tsdf_resample_kernel', int(np.prod(i['dst'])), 256)],
    constants=(('kTile = 256', 'tsdf_resample.hip:30'),)))


def _nearest_run(lib, a, i):
    n = int(np.prod(i['dst']))
    s32, s16 = a.put('semseg', i['semseg']), a.put('label16', i['label16'])
    o32, o16 = a.out('semseg', (n,), torch.int32), a.out('label16', (2, n), torch.int16)
    keep, grid = _grid_args(i)
    fill = ctypes.c_int32(-1)
    assert lib.v3d_volume_resample_nearest(p(s32), 4, 1, *grid, 1, ctypes.addressof(fill), p(o32), a.stream()) == OK
    assert lib.v3d_volume_resample_nearest(p(s16), 2, 2, *grid, 0, None, p(o16), a.stream()) == OK
    return ()


def _nearest_check(i, out, status):
    oracle, p32 = _plan(i)
    assert np.array_equal(out['semseg'].numpy(), oracle.fill_outside(p32, oracle.nearest(p32, i['semseg']), -1).reshape(-1))
    assert np.array_equal(out['label16'].numpy(), oracle.nearest(p32, i['label16']).reshape(2, -1))


CASES.append(Case(
    'volume_resample_nearest', ('v3d_volume_resample_nearest',), _resample_make, _nearest_run, _nearest_check,
    bound='tsdf_transform_oracle.nearest / fill_outside, exact', sections=lambda lib, i: {},
    groups=lambda i: [('volume_resample_nearest_kernel', int(np.prod(i['dst'])), 256)], constants=(('kTile = 256', 'tsdf_resample.hip:30'),)))


# ---- cost volume: back-projection, warp kernels, regulariser ------------------------------------------------------------------------

def _csr(edges):
    refs, counts = np.unique(edges[0], return_counts=True)
    return (refs.astype(np.int32), np.concatenate(([0], np.cumsum(counts))).astype(np.int32),
            edges[1][np.argsort(edges[0], kind='stable')].astype(np.int32))


def _views(n_ref, img_size, feat_size, seed):
    syn = v3d('synthetic')
    edges, n_img = syn.make_edges(n_ref, 1, 2)
    rot, tv, K = syn.make_cameras(n_img, img_size, seed=seed)
    feat = syn.make_features(n_img, 32, feat_size[0], feat_size[1], seed=seed)
    return dict(edges=edges.numpy(), n_img=n_img, rot=rot.numpy(), tv=tv.numpy(), K=K.numpy(), feat=feat.numpy(), img_size=img_size)


def _bp_make(size):
    syn = v3d('synthetic')
    n_ref, plane = {'small': (2, (9, 13)), 'big': (8, (13, 18))}[size]
    i = _views(n_ref, (64, 80), (16, 20), seed=9)
    rot, tv, K = (torch.from_numpy(i[k]) for k in ('rot', 'tv', 'K'))
    depth = syn.ray_box_depth(rot[1:1 + n_ref], tv[1:1 + n_ref], K[1:1 + n_ref], (64, 80), plane)
    depth = depth + 0.02 * torch.randn(depth.shape, generator=torch.Generator().manual_seed(3))
    i.update(depth=depth.numpy(), n_ref=n_ref, h=plane[0], w=plane[1], offset=0.025, n_half=1)
    return i


def _bp_run(lib, a, i):
    n_img, n_ref, h, w, nh = i['n_img'], i['n_ref'], i['h'], i['w'], 2 * i['n_half'] + 1
    nb = lib.v3d_backproject_workspace_bytes(n_img, 32, 16, 20)
    ws = a.ws('bp', nb)
    ref_img, ofs, src = (a.put(k, v) for k, v in zip(('ri', 'eo', 'es'), _csr(i['edges'])))
    d, f, K, R, t = (a.put(k, i[k]) for k in ('depth', 'feat', 'K', 'rot', 'tv'))
    for tag, feat_p in (('', p(f)), ('_kept_copy', None)):                     # feat == NULL: the copy the first call left in `ws`
        pts, var = a.out('pts' + tag, (n_ref * h * w, nh, 3), torch.float32), a.out('var' + tag, (n_ref * h * w, nh, 32), torch.float32)
        assert lib.v3d_backproject_variance_f32(p(d), feat_p, p(K), p(R), p(t), p(ref_img), p(ofs), p(src), n_img, n_ref, src.shape[0], 32, 16, 20,
                                                64, 80, h, w, i['offset'], i['n_half'], p(pts), p(var), p(ws), nb, a.stream()) == OK
    return ()


def _bp_check(i, out, status):
    from oracle import scene as osc
    T = torch.from_numpy
    pts, var, _ = osc.pointflow_hypotheses(T(i['depth']), torch.zeros(i['n_ref'], dtype=torch.long), T(i['feat']), T(i['rot']), T(i['tv']), T(i['K']),
                                           T(i['edges']), i['offset'], i['n_half'], i['img_size'], pinned=True)
    assert torch.equal(out['pts'], pts.reshape(out['pts'].shape))
    np.testing.assert_allclose(out['var'].numpy(), var.numpy().reshape(out['var'].shape), rtol=0, atol=5e-5)
    assert float(var.abs().max()) > 1e-3
    for name in ('pts', 'var'):
        assert_same_bits('backproject_variance', 'paired (feat == NULL on the kept copy)', name, out[name + '_kept_copy'], out[name])


CASES.append(Case(
    'backproject_variance', ('v3d_backproject_variance_f32',), _bp_make, _bp_run, _bp_check,
    bound='oracle.scene.pointflow_hypotheses(pinned): points bit-equal, variance 5e-5 (tests/test_scene_gpu.py)',
    sections=lambda lib, i: {'bp': lib.v3d_backproject_workspace_bytes(i['n_img'], 32, 16, 20)},
    groups=lambda i: [('backproject_variance_kernel (lanes per view)', i['h'] * i['w'] * 3 * 8, 256, i['n_ref'])],
    constants=(('dim3 grid((unsigned)((lanes + 255) / 256), n_ref)', 'backproject.hip:204'),), paired=True))


def _psv_make(size):
    if size == 'small':
        from helpers import load_golden
        g = load_golden('A_tiny_rotated')
        d0, dd, D = g['depth_cfg']
        return dict(edges=g['edges'], n_img=4, rot=g['rotmats'], tv=g['tvecs'], K=g['K'], feat=g['feat'], img_size=(64, 80), d0=float(d0),
                    dd=float(dd), D=int(D), h=8, w=8, want=g['var'])
    i = _views(6, (64, 80), (16, 20), seed=21)                                 # 9 images for 4; 13 planes on a 7 x 9 grid: ragged chunks and tiles
    i.update(d0=0.5, dd=0.15, D=13, h=7, w=9, want=None)
    return i


def _split_roundtrip(var):
    hi = var.bfloat16().float()
    return hi + (var - hi).bfloat16().float()


def _decode_split(raw, n, D, h, w):
    f = (raw.view(torch.int16).view(n, 4, 2, D, h, w, 8).to(torch.int32) << 16).view(torch.float32)
    return (f[:, :, 0] + f[:, :, 1]).permute(0, 1, 5, 2, 3, 4).reshape(n, 32, D, h, w)


def _decode_cl8(raw, n, D, h, w):
    return raw.view(n, 4, 2, D, h, w, 4).permute(0, 1, 2, 6, 3, 4, 5).reshape(n, 32, D, h, w)


def _psv_run(lib, a, i):
    n_img, D, h, w, s = i['n_img'], i['D'], i['h'], i['w'], a.stream()
    csr = _csr(i['edges'])
    n_ref, n_edges = csr[0].shape[0], csr[2].shape[0]
    ref_img, ofs, src = (a.put(k, v) for k, v in zip(('ri', 'eo', 'es'), csr))
    f, K, R, t = (a.put(k, i[k]) for k in ('feat', 'K', 'rot', 'tv'))
    nb = lib.v3d_psv_workspace_bytes(n_img, 32, 16, 20)
    for name, fn in (('var', lib.v3d_psv_variance_f32), ('var_split', lib.v3d_psv_variance_split), ('var_cl8', lib.v3d_psv_variance_cl8)):
        ws = a.ws('psv_' + name, nb)                                            # a poisoned workspace of its own for each entry point
        out = a.out(name, (n_ref, 32, D, h, w), torch.float32)
        assert fn(p(f), p(K), p(R), p(t), p(ref_img), p(ofs), p(src), n_img, n_ref, n_edges, 32, 16, 20, 64, 80, i['d0'], i['dd'], D, h, w, p(out),
                  p(ws), nb, s) == OK
    pb = n_img * 36 * 4
    ws = a.ws('positions', pb)
    pos, world = a.out('pos', (n_edges, D * h * w, 2), torch.float32), a.out('world', (n_ref, 3, D * h * w), torch.float32)
    assert lib.v3d_psv_sample_positions_f32(p(K), p(R), p(t), p(ref_img), p(ofs), p(src), n_img, n_ref, n_edges, 16, 20, 64, 80, i['d0'], i['dd'], D, h,
                                            w, p(pos), p(world), p(ws), pb, s) == OK
    return ()


def _psv_check(i, out, status):
    from oracle import pinned
    T = torch.from_numpy
    K, R, t = T(i['K']), T(i['rot']), T(i['tv'])
    want = pinned.warp_variance(T(i['feat']), R, t, K, T(i['edges']), i['d0'], i['dd'], i['D'], i['img_size'], (i['h'], i['w']))
    n, D, h, w = want.shape[0], i['D'], i['h'], i['w']
    np.testing.assert_allclose(out['var'].numpy(), want.numpy(), rtol=0, atol=5e-7)
    if i['want'] is not None:
        np.testing.assert_allclose(out['var'].numpy(), i['want'], rtol=0, atol=5e-7)
    assert float(want.max()) > 1e-3 and torch.isfinite(out['var']).all()
    assert torch.equal(_decode_split(out['var_split'], n, D, h, w), _split_roundtrip(out['var']))
    assert_same_bits('psv_variance', 'channel-last volume', 'var_cl8', _decode_cl8(out['var_cl8'], n, D, h, w).contiguous(), out['var'])
    refs, ofs, src = _csr(i['edges'])
    _, P = pinned.camera_blocks(K, R, t)
    for r, ref in enumerate(refs.tolist()):
        X = pinned.world_points(K, R, t, ref, i['d0'], i['dd'], D, i['img_size'], (h, w))
        assert np.array_equal(out['world'][r].numpy(), X.numpy())
        for e in range(int(ofs[r]), int(ofs[r + 1])):
            ix, iy = (x.numpy() for x in pinned.sample_positions(X, P[int(src[e])], i['img_size'], (16, 20)))
            assert np.array_equal(out['pos'][e, :, 0].numpy(), ix) and np.array_equal(out['pos'][e, :, 1].numpy(), iy)


CASES.append(Case(
    'psv_variance', ('v3d_psv_variance_f32', 'v3d_psv_variance_split', 'v3d_psv_variance_cl8', 'v3d_psv_sample_positions_f32'),
    _psv_make, _psv_run, _psv_check,
    bound='oracle.pinned.warp_variance and the golden volume at 5e-7; split == hi + lo of the fp32 volume, cl8 bit-equal; positions bit-equal '
          '(tests/test_costvolume_gpu.py)',
    sections=lambda lib, i: {'psv': lib.v3d_psv_workspace_bytes(i['n_img'], 32, 16, 20)},
    groups=lambda i: [('warp kernel: tiles of 8 pixels, per view and chunk of 8 planes', i['h'] * i['w'], 8,
                       np.unique(i['edges'][0]).size * -(-i['D'] // 8))],
    constants=(('kRPix = 8', 'psv_kernels.h:75'), ('8 planes x 8 pixels = 64 lanes', 'psv_window.hip:52')), rule_on='big'))


_NETS = {}


def _costreg_net(device, cin=32, seed=0, sharpen=200.0):
    """CostRegNet with seeded weights on the device -> (module, state dict); kept: the handle lives as long as the module."""
    key = (str(device), cin, seed)
    if key not in _NETS:
        syn, mvs = v3d('synthetic'), v3d('mvsnet')
        sd = syn.costregnet_weights(in_channels=cin, seed=seed, sharpen=sharpen)
        net = mvs.CostRegNet(cin, 8).eval()
        net.load_state_dict(sd, strict=False)
        _NETS[key] = (net.to(device), sd)
    return _NETS[key]


def _reg_make(size):
    if size == 'small':
        from helpers import load_golden
        g = load_golden('A_tiny_rotated')
        d0, dd, D = g['depth_cfg']
        return dict(var=g['var'], d0=float(d0), dd=float(dd), D=int(D), cin=32)
    rng = np.random.default_rng(5 if size == 'big' else 6)
    n, cin, D, h, w = {'big': (2, 32, 16, 8, 24), 'c16': (1, 16, 8, 8, 8)}[size]   # c16: in_channels / 8 = ngrp < 4 (costreg.hip:256)
    return dict(var=(rng.random((n, cin, D, h, w)) ** 2 * 0.2).astype(np.float32), d0=0.5, dd=0.125, D=D, cin=cin)


def _encode(var, layout):
    n, _, D, h, w = var.shape
    if layout == 'cl8':
        return var.view(n, 4, 2, 4, D, h, w).permute(0, 1, 2, 4, 5, 6, 3).contiguous()
    hi = var.bfloat16()
    lo = (var - hi.float()).bfloat16()
    enc = torch.stack([x.view(n, 4, 8, D, h, w).permute(0, 1, 3, 4, 5, 2) for x in (hi, lo)], dim=2).contiguous()
    return enc.view(torch.int16)


def _reg_run(entry):
    def run(lib, a, i):
        var = torch.from_numpy(i['var'])
        n, cin, D, h, w = var.shape
        net, _ = _costreg_net(a.device, cin)
        handle = net.packed_handle(a.device)
        nb = lib.v3d_costreg_workspace_bytes(handle, n, D, h, w)
        ws = a.ws('costreg', nb)
        vals = a.put('vals', torch.linspace(i['d0'], i['d0'] + i['dd'] * (D - 1), D).numpy())
        depth, reg = a.out('depth', (n, h, w), torch.float32), a.out('reg', (n, D, h, w), torch.float32)
        s = a.stream()
        if entry == 'f32':
            x = a.put('x', var.numpy())
            rc = lib.v3d_costreg_depth_f32(handle, p(x), p(vals), n, D, h, w, p(depth), p(reg), 0, p(ws), nb, s)
            assert rc == OK, lib.v3d_last_error()
            # V3D_PRECISION_FP32 on the reference layout: another layer-0 kernel and other workspace slots, on a workspace of its own
            ws = a.ws('costreg_fp32', nb)
            depth, reg = a.out('depth_fp32', (n, h, w), torch.float32), a.out('reg_fp32', (n, D, h, w), torch.float32)
            rc = lib.v3d_costreg_depth_f32(handle, p(x), p(vals), n, D, h, w, p(depth), p(reg), 1, p(ws), nb, s)
        elif entry == 'split':
            x = a.put('x', _encode(var, 'split').numpy())
            rc = lib.v3d_costreg_depth_split(handle, p(x), p(vals), n, D, h, w, p(depth), p(reg), p(ws), nb, s)
        elif entry == 'cl8':
            x = a.put('x', _encode(var, 'cl8').numpy())
            rc = lib.v3d_costreg_depth_cl8(handle, p(x), p(vals), n, D, h, w, p(depth), p(reg), p(ws), nb, s)
        else:
            x = a.put('x', var.numpy())
            prob = a.out('prob', (n, h, w), torch.float32)
            rc = lib.v3d_costreg_depth_prob(handle, p(x), 0, 0, p(vals), i['d0'], i['dd'], n, D, h, w, p(depth), p(reg), p(prob), p(ws), nb, s)
        assert rc == OK, lib.v3d_last_error()
        return ()
    return run


def _reg_check(entry):
    def check(i, out, status):
        from oracle import costvolume as ocv
        sd = v3d('synthetic').costregnet_weights(in_channels=i['cin'], seed=0, sharpen=200.0)
        with torch.no_grad():
            reg = ocv.costregnet(torch.from_numpy(i['var']), sd).squeeze(1)
            depth, _ = ocv.soft_argmin_depth(reg, i['d0'], i['dd'], i['D'])
        rtol = 1e-5 if entry == 'cl8' else 5e-5                               # of max|x_reg|: exact fp32 | split-bf16 operands
        np.testing.assert_allclose(out['reg'].numpy(), reg.numpy(), rtol=0, atol=rtol * float(reg.abs().max()))
        np.testing.assert_allclose(out['depth'].numpy(), depth.numpy(), rtol=1e-4, atol=0)
        if entry == 'f32':
            np.testing.assert_allclose(out['reg_fp32'].numpy(), reg.numpy(), rtol=0, atol=1e-5 * float(reg.abs().max()))
            np.testing.assert_allclose(out['depth_fp32'].numpy(), depth.numpy(), rtol=1e-4, atol=0)
        if entry == 'prob':
            import confidence_oracle as co
            want = co.logits_f32(out['reg'].numpy(), out['depth'].numpy(), i['d0'], i['dd'])
            assert co.max_error(out['prob'].numpy(), want.astype(np.float64)) <= 1e-6
    return check


def _reg_groups(i):
    n, _, D, h, w = i['var'].shape
    return [('soft_argmin_kernel: the pixels of all views', n * h * w, 256)]


for _entry, _sym, _extra in (('f32', 'v3d_costreg_depth_f32', ('c16',)), ('split', 'v3d_costreg_depth_split', ()), ('cl8', 'v3d_costreg_depth_cl8', ()),
                             ('prob', 'v3d_costreg_depth_prob', ())):
    CASES.append(Case(
        'costreg_depth_' + _entry, (_sym,), _reg_make, _reg_run(_entry), _reg_check(_entry),
        bound='oracle.costvolume.costregnet: x_reg within 5e-5 (split-bf16) / 1e-5 (exact fp32) of max|x_reg|, depth 1e-4 relative; prob within '
              '1e-6 of confidence_oracle.logits_f32 (tests/test_costvolume_gpu.py, tests/test_confidence_gpu.py)',
        sections=None,                                                         # v3d_costreg_workspace_bytes takes a weight handle: needs a device
        groups=_reg_groups,
        constants=(('soft_argmin_kernel<<<(unsigned)((npix + 255) / 256), 256', 'confidence.hip:147'),
                   ('(D, h, w divisible by 8)', 'include/v3d.h:201')), extra=_extra, rule_on='big'))


def _layer_make(size):
    n = {'small': 2, 'big': 4}[size]
    return dict(x=torch.randn((n, 16, 6, 10, 18), generator=torch.Generator().manual_seed(102)).numpy(), layer=2, n=n)


def _layer_run(lib, a, i):
    n, cin, D, H, W = i['x'].shape
    net, _ = _costreg_net(a.device, 32, seed=6, sharpen=1.0)
    nb = lib.v3d_costreg_layer_split_workspace_bytes(n, cin, D, H, W)
    ws = a.ws('layer_split', nb)
    x = a.put('x', i['x'])
    out = a.out('out', (n, 16, D, H, W), torch.float32)
    assert lib.v3d_costreg_layer_split_f32(net.packed_handle(a.device), i['layer'], p(x), None, n, D, H, W, p(out), p(ws), nb, a.stream()) == OK
    return ()


def _layer_check(i, out, status):
    from oracle import costvolume as ocv
    sd = v3d('synthetic').costregnet_weights(seed=6)
    with torch.no_grad():
        ref = ocv.conv_bn_relu3d(torch.from_numpy(i['x']), sd, 'conv2')
    err = float((out['out'] - ref).abs().max())
    assert err <= 4e-5 * max(1.0, float(ref.abs().max())), err


CASES.append(Case(
    'costreg_layer_split', ('v3d_costreg_layer_split_f32',), _layer_make, _layer_run, _layer_check,
    bound='oracle.costvolume.conv_bn_relu3d within 4e-5 of max|out| (tests/test_costvolume_gpu.py::test_costreg_single_layers_split_kernels)',
    sections=lambda lib, i: {'layer_split': lib.v3d_costreg_layer_split_workspace_bytes(*[int(v) for v in i['x'].shape])},
    groups=lambda i: [('re-encode + conv2 tiles: voxels per view', 6 * 10 * 18, 256, i['n'])],
    constants=(('encode_split_kernel<<<(unsigned)((total + 255) / 256), 256', 'costreg_convg.hip:579'),)))


# ---- the fused hypothesis decoder and the fused inverted-residual block ---------------------------------------------------------------

_DEC = {}


def _decoder(device):
    if str(device) not in _DEC:
        rf = v3d('refinement')
        dec = rf.HypothesisDecoder(320, 128, 3, 1).eval()
        dec.load_state_dict(_decoder_sd(), strict=False)
        _DEC[str(device)] = dec.to(device)
    return _DEC[str(device)]


def _decoder_sd():
    return v3d('synthetic').decoder_weights(in_dim=320, h_dim=128, seed=6, sharpen=100.0)


def _dec_make(size):
    import sparse_oracle as so
    n_pts, side, n_hyp = {'small': (150, 7, 3), 'big': (330, 9, 3)}[size]        # 32 points per tile (decoder.hip:101)
    rng = np.random.default_rng(120 + n_pts)
    g = np.stack(np.meshgrid(np.arange(2), np.arange(side), np.arange(side), np.arange(side), indexing='ij'), -1).reshape(-1, 4)
    fine = g[rng.random(g.shape[0]) < 0.5].astype(np.int64)
    res, min_pts = 0.0625, np.array([[-1.0, 0.5, 2.0], [3.0, -2.0, 0.25]], dtype=np.float32)
    levels = []                                                                 # finest first: strides 1, 2, 4; widths 64, 128, 128
    coords = fine
    for ts, C in ((1, 64), (2, 128), (4, 128)):
        if ts > 1:
            coords = so.strided_coords(coords, ts // 2)
        levels.append(dict(coords=coords, feats=rng.standard_normal((coords.shape[0], C)).astype(np.float32), ts=ts, res=res * ts))
    pb = rng.integers(0, 2, n_pts).astype(np.int64)
    base = min_pts[pb].astype(np.float64) + rng.uniform(-1.0, side, (n_pts, 3)) * res
    pts = (base[:, None, :] + rng.standard_normal((n_pts, 1, 3)) * 0.03 * np.arange(n_hyp)[None, :, None]).astype(np.float32)
    return dict(levels=levels, min_pts=min_pts, pts=pts, pts_batch=pb, n_pts=n_pts, n_hyp=n_hyp, vals=np.linspace(-0.1, 0.1, n_hyp).astype(np.float32))


def _dec_run(lib, a, i):
    n_pts, n_hyp, s = i['n_pts'], i['n_hyp'], a.stream()
    dec = _decoder(a.device)
    handles, w_last, b_last = dec.packed_handles(a.device)
    tabs, feats, mins = [], [], []
    for k, lv in enumerate(i['levels']):                                        # the tables are inputs of the call: built, never poisoned after
        n = lv['coords'].shape[0]
        tb = lib.v3d_hash_bytes(n)
        table = a.state('table%d' % k, np.zeros(tb, np.uint8))
        c = a.put('coords%d' % k, lv['coords'], torch.int32)
        assert lib.v3d_hash_build(p(c), n, p(table), tb, s) == OK and lib.v3d_hash_status(p(table), n, s) == OK
        tabs.append(table)
        feats.append(a.put('feats%d' % k, lv['feats']))
        mins.append(a.put('min%d' % k, i['min_pts']))
    vp = ctypes.c_void_p
    layers = (vp * 3)(*handles)
    tables, fts, mns = (vp * 3)(*[p(t) for t in tabs]), (vp * 3)(*[p(t) for t in feats]), (vp * 3)(*[p(t) for t in mins])
    n_in = (ctypes.c_int * 3)(*[lv['coords'].shape[0] for lv in i['levels']])
    chans = (ctypes.c_int * 3)(*[lv['feats'].shape[1] for lv in i['levels']])
    strides = (ctypes.c_int * 3)(*[lv['ts'] for lv in i['levels']])
    res = (ctypes.c_float * 3)(*[lv['res'] for lv in i['levels']])
    nb = lib.v3d_decoder_fused_workspace_bytes(n_pts, n_hyp)
    ws = a.ws('fused', nb)
    pts, pb, vals = a.put('pts', i['pts']), a.put('pb', i['pts_batch']), a.put('vals', i['vals'])
    preds, expect = a.out('preds', (n_pts, n_hyp), torch.float32), a.out('expect', (n_pts,), torch.float32)
    rc = lib.v3d_decoder_fused_f32(layers, p(w_last), p(b_last), tables, n_in, fts, chans, strides, mns, res, p(pts), p(pb), None, 0, n_pts, n_hyp,
                                   p(vals), p(preds), p(expect), None, p(ws), nb, s)
    assert rc == OK, lib.v3d_last_error()
    return ()


def _dec_check(i, out, status):
    from helpers import decoder_reference
    T = torch.from_numpy
    xs = []
    for lv in i['levels'][::-1]:                                                # the oracle takes coarse -> fine and prepends each level
        n = lv['coords'].shape[0]
        b = T(lv['coords'][:, 0]).long()
        xs.append(dict(feats=T(lv['feats']).double(), pts=T(i['min_pts']).double()[b], res=lv['res'], batch=b, stride=lv['ts'],
                       coords=T(lv['coords']).long()))
    sd = {k: v.double() for k, v in _decoder_sd().items() if v.dtype.is_floating_point}
    with torch.no_grad():
        want = decoder_reference(xs, T(i['pts']).double(), None, T(i['pts_batch']), sd)
    assert float(want.max()) > 0.5                                              # a peaked softmax: not vacuous
    np.testing.assert_allclose(out['preds'].numpy(), want.numpy(), rtol=0, atol=2e-4)
    own = (out['preds'].double() * T(i['vals']).double()[None]).sum(1)
    assert float((out['expect'].double() - own).abs().max()) <= 16 * 2.0 ** -24 * float(np.abs(i['vals']).max())


CASES.append(Case(
    'decoder_fused', ('v3d_decoder_fused_f32',), _dec_make, _dec_run, _dec_check,
    bound='oracle.scene decoder in float64 (helpers.decoder_reference): probabilities 2e-4 (tests/test_parity_net_gpu.py, against the golden); '
          'expectation = sum p_i v_i of its own probabilities within 16 u max|v|',
    sections=lambda lib, i: {'fused': lib.v3d_decoder_fused_workspace_bytes(i['n_pts'], i['n_hyp'])},
    groups=lambda i: [('index kernel: 8 corners x 3 levels per hypothesis point', i['n_pts'] * i['n_hyp'], 256),
                      ('decoder_fused_kernel: tiles of kDPtsTile = 32 points', i['n_pts'], 32)],
    constants=(('kDPtsWave = 4, kDPtsTile = kDPtsWave * kDWaves', 'decoder.hip:101'), ('kDWaves = 8', 'decoder.hip:100'),
               ('decoder_corner_kernel<true><<<(unsigned)((n_thr + 255) / 256), 256', 'sparse_interp.hip:286')),
    inout=('table0', 'table1', 'table2')))


_IRB = {}


def _irb_block(device=None):
    """The (192 -> 192, k 5, stride 1) block of the trunk at 1/32 resolution: few tiles, so the partial sums of the slice groups meet
    in the workspace (tests/test_backbone.py BLOCKS)."""
    bb = v3d('backbone')
    if 'blk' not in _IRB:
        torch.manual_seed(192 * 100 + 8)
        blk = bb._InvertedResidual(192, 192, 5, 1, 6).eval()
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.data.uniform_(0.5, 1.5)
                m.bias.data.normal_(0, 0.1)
        _IRB['blk'] = blk
    if device is not None and str(device) not in _IRB:
        _IRB[str(device)] = bb._Block(_IRB['blk'], device)
    return _IRB['blk'], _IRB.get(str(device))


def _irb_make(size):
    n = {'small': 3, 'big': 6}[size]
    return dict(x=torch.randn((n, 8, 10, 192), generator=torch.Generator().manual_seed(n)).numpy(), n=n)


def _irb_run(lib, a, i):
    _, fused = _irb_block(a.device)
    n = i['n']
    assert fused.supported(8, 10)
    nb = lib.v3d_irb_workspace_bytes(fused.handle, n, 8, 10)
    assert nb > 0, 'this block shape was chosen for its workspace'
    ws = a.ws('irb', nb)
    x = a.put('x', i['x'])
    out = a.out('out', (n, 8, 10, 192), torch.float32)
    assert lib.v3d_irb_nhwc_f32(fused.handle, p(x), n, 8, 10, p(out), p(ws), nb, a.stream()) == OK
    return ()


def _irb_check(i, out, status):
    blk, _ = _irb_block()
    with torch.no_grad():
        ref = blk(torch.from_numpy(i['x']).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).contiguous()
    assert torch.isfinite(out['out']).all()
    err = float((out['out'] - ref).abs().max() / ref.abs().max())
    assert err < 2e-5, 'fused block vs module: %.2e of range' % err


CASES.append(Case(
    'irb_nhwc', ('v3d_irb_nhwc_f32',), _irb_make, _irb_run, _irb_check,
    bound='the block\'s module on the CPU within 2e-5 of the range (tests/test_backbone.py::test_fused_inverted_residual_block)',
    sections=None,                                                             # v3d_irb_workspace_bytes takes a weight handle: needs a device
    # the blocks with a workspace are the 1/32-resolution ones: an 8 x 10 map of 192 channels is 15 full workgroups of the reducing launch per image
    groups=lambda i: [('irb_reduce_kernel: float4 per thread', i['n'] * 8 * 10 * 192 // 4, 256, 1,
                       'never ragged: the only maps with a workspace are the 8 x 10 ones, 80 pixels x 192 / 4 = 15 x 256 per image')],
                       constants=(('irb_reduce_kernel<<<(unsigned)((total / 4 + 255) / 256), 256', 'irb.hip:644'),),
    ))


# ---- training: v3d_hash_build -> v3d_sparse_interp_backward_f32 -> v3d_hash_status; v3d_sparse_conv_weight_grad_f32 -------------------
# (tests/test_sparse_interp_backward_contract.py and tests/test_sparse_conv_backward_contract.py hold these two cases to the four
# properties on their own as well)

INTERP_BWD_C = 32


def _ibwd_make(size):
    i = _hash_make(size)                                                       # the map and the queries of the forward's case
    rng = np.random.default_rng(70 + i['n'])
    ld, col0 = INTERP_BWD_C + 12, 8
    grad = np.full((i['n_pts'] * i['n_hyp'], ld), np.nan, dtype=np.float32)
    grad[:, col0:col0 + INTERP_BWD_C] = rng.standard_normal((grad.shape[0], INTERP_BWD_C)).astype(np.float32)
    return dict(i, grad_out=grad, ld=ld, col0=col0, C=INTERP_BWD_C, ts=1)


def _ibwd_run(lib, a, i):
    n, n_pts, n_hyp, s, C = i['n'], i['n_pts'], i['n_hyp'], a.stream(), INTERP_BWD_C
    tb, wb = lib.v3d_hash_bytes(n), lib.v3d_sparse_interp_backward_workspace_bytes(n, C, n_pts, n_hyp)
    table, ws = a.ws('table', tb), a.ws('interp_backward', wb)
    c = a.put('coords', i['coords'], torch.int32)
    assert lib.v3d_hash_build(p(c), n, p(table), tb, s) == OK
    out = a.out('grad_feats', (n, C), torch.float32)
    g, pts, pb, mn = a.put('g', i['grad_out']), a.put('pts', i['pts']), a.put('pb', i['pts_batch']), a.put('mn', i['min_pts'])
    assert lib.v3d_sparse_interp_backward_f32(p(table), n, C, 1, p(pts), p(pb), n_pts, n_hyp, p(mn), i['res'], p(g), i['ld'], i['col0'],
                                              p(out), p(ws), wb, s) == OK
    return (lib.v3d_hash_status(p(table), n, s),)


def _ibwd_check(i, out, status):
    import sparse_interp_backward_oracle as sbo
    assert status == (OK,)
    orc = sbo.gradient(i)
    bad, worst, worst_zero = sbo.violations(out['grad_feats'].numpy(), orc)
    assert (orc['S'] > 0).any()
    assert bad == 0 and worst_zero == 0.0, 'grad_feats: %d elements outside (cnt + 2) u S, worst ratio %.3f' % (bad, worst)


def _ibwd_groups(i):
    import sparse_interp_backward_oracle as sbo
    C = INTERP_BWD_C
    return [('interp_corners / interp_backward_segment', i['n_pts'] * i['n_hyp'] * 8, 256),
            ('interp_backward_count_kernel', i['n'] + 1, 256),
            ('interp_backward_chunk_kernel', (i['n_pts'] * i['n_hyp'] * 8 // sbo.CHUNK + i['n']) * (C // 4), 256),
            ('interp_backward_combine_kernel', i['n'] * (C // 4), 256)]


CASES.append(Case(
    'sparse_interp_backward', ('v3d_sparse_interp_backward_f32',), _ibwd_make, _ibwd_run, _ibwd_check,
    bound='sparse_interp_backward_oracle.gradient within (cnt + 2) u S (tests/test_sparse_interp_backward_gpu.py::test_every_element_within_the_bound)',
    sections=lambda lib, i: {'table': lib.v3d_hash_bytes(i['n']),
                             'interp_backward': lib.v3d_sparse_interp_backward_workspace_bytes(i['n'], INTERP_BWD_C, i['n_pts'], i['n_hyp'])},
    groups=_ibwd_groups,
    constants=(('kInterpBwdChunk = 512', 'sparse_interp.hip:124'),
               ('interp_backward_segment_kernel<<<(unsigned)((nq * 8 + 255) / 256), 256', 'sparse_interp.hip:347'),
               ('interp_backward_count_kernel<<<(unsigned)(((long long)n_in + 256) / 256), 256', 'sparse_interp.hip:358'),
               ('interp_backward_chunk_kernel<true><<<blocks, 256', 'sparse_interp.hip:365'),
               ('interp_backward_combine_kernel<<<(unsigned)(((long long)n_in * tpc + 255) / 256), 256', 'sparse_interp.hip:370')),
    paired=True))


WGRAD_K, WGRAD_N = 32, 16
WGRAD_ROWS = 512                                                               # sparse_conv_backward_oracle.ROWS; gemm_wgrad.hip:23, cited below
WGRAD_SHAPES = {'small': (WGRAD_ROWS + 37, 9), 'big': (3 * WGRAD_ROWS + 90, 11)}   # (rows, side of the two-batch grid): 2 and 4 chunks


def _wgrad_make(size):
    import sparse_conv_backward_oracle as sco
    m, side = WGRAD_SHAPES[size]
    nbr, _, n_in, _ = sco.table('same', sco.occupancy_map(m, side, 40 + m))
    return sco.make_case(nbr, n_in, WGRAD_K, WGRAD_N, 41 + m, pad_src=12, pad_grad=8)


def _wgrad_run(lib, a, i):
    K, N = WGRAD_K, WGRAD_N
    wb = lib.v3d_sparse_conv_weight_grad_workspace_bytes(i['M'], 27, K, N)
    ws = a.ws('weight_grad', wb)
    src, nbr, g = a.put('src', i['src']), a.put('nbr', i['nbr']), a.put('grad_out', i['grad_out'])
    out = a.out('grad_w', (27, K, N), torch.float32)
    return (lib.v3d_sparse_conv_weight_grad_f32(p(src), i['ld_src'], p(nbr), i['M'], 27, p(g), i['ld_grad'], i['M'], K, N, p(out), p(ws), wb,
                                                a.stream()),)


def _wgrad_check(i, out, status):
    import sparse_conv_backward_oracle as sco
    assert status == (OK,)
    orc = sco.weight_grad(i['x'], i['nbr'].astype(np.int64), i['g'])
    got = out['grad_w'].numpy()
    assert np.isfinite(got).all() and (orc['S'] > 0).any()
    bad, worst, worst_zero = sco.violations(got, orc)
    assert bad == 0 and worst_zero == 0.0, 'grad_w: %d elements outside (cnt + 32) u S, worst ratio %.3f' % (bad, worst)


CASES.append(Case(
    'sparse_conv_weight_grad', ('v3d_sparse_conv_weight_grad_f32',), _wgrad_make, _wgrad_run, _wgrad_check,
    bound='sparse_conv_backward_oracle.weight_grad within (cnt_k + 32) u S (tests/test_sparse_conv_weight_grad_gpu.py::test_sizes_and_channel_pairs)',
    sections=lambda lib, i: {'weight_grad': lib.v3d_sparse_conv_weight_grad_workspace_bytes(i['M'], 27, WGRAD_K, WGRAD_N)},
    # one workgroup per (chunk of 512 rows, offset): 27 independent batches of chunks; the reduction walks 27 K N / 4 float4
    groups=lambda i: [('sparse_conv_wgrad_kernel', i['M'], WGRAD_ROWS, 27),
                      ('sparse_conv_wgrad_reduce_kernel', 27 * WGRAD_K * WGRAD_N // 4, 256)],
    constants=(('constexpr int kWgradRows = 512;', 'gemm_wgrad.hip:23'),
               ('kern<<<dim3((unsigned)ch.n, (unsigned)n_seg), 256', 'gemm_wgrad.hip:239'),
               ('sparse_conv_wgrad_reduce_kernel<<<(unsigned)((slab4 + 255) / 256), 256', 'gemm_wgrad.hip:243'))))


# ---- entry points whose outputs are poisoned elsewhere -------------------------------------------------------------------------------------

for _sym, _test in (('v3d_propagation_up_f32', 'test_E_stage3_past_4_gb_of_features'),
                    ('v3d_soft_argmin_f32', 'test_D_soft_argmin_and_confidence_7140_views'),
                    ('v3d_confidence_logits_f32', 'test_D_soft_argmin_and_confidence_7140_views'),
                    ('v3d_probability_map_f32', 'test_D_soft_argmin_and_confidence_7140_views')):
    CASES.append(Case(_sym[4:], (_sym,), None, covered_by=(_test, 'test_large_launch_gpu.py')))


# the size functions, with the entry points they size
SIZED_BY = {
    'v3d_edges_csr_workspace_bytes': 'edges_csr', 'v3d_psv_workspace_bytes': 'psv_variance', 'v3d_costreg_workspace_bytes': 'costreg_depth_f32',
    'v3d_costreg_layer_split_workspace_bytes': 'costreg_layer_split', 'v3d_backproject_workspace_bytes': 'backproject_variance',
    'v3d_hash_bytes': 'hash_chain', 'v3d_sparse_interp_workspace_bytes': 'hash_chain', 'v3d_segment_csr_workspace_bytes': 'segment_csr_max',
    'v3d_sort_unique_workspace_bytes': 'voxelize_chain', 'v3d_voxelize_workspace_bytes': 'voxelize_chain',
    'v3d_decoder_fused_workspace_bytes': 'decoder_fused', 'v3d_irb_workspace_bytes': 'irb_nhwc', 'v3d_fusion_workspace_bytes': 'fusion_chain',
    'v3d_cloud_downsample_workspace_bytes': 'cloud_downsample', 'v3d_nn_workspace_bytes': 'nn_query',
    'v3d_cloud_metrics_workspace_bytes': 'cloud_metrics', 'v3d_mesh_workspace_bytes': 'mesh_count_extract',
    'v3d_depth_metrics_workspace_bytes': 'depth_metrics_2d', 'v3d_depth_supervision_workspace_bytes': 'depth_supervision',
    'v3d_order_stats_workspace_bytes': 'cloud_order_stats',
    'v3d_sparse_interp_backward_workspace_bytes': 'sparse_interp_backward',
    'v3d_sparse_conv_weight_grad_workspace_bytes': 'sparse_conv_weight_grad'}


# what the issue puts in scope besides the functions with a `workspace` / `table` parameter: workspace-free calls that write whole arrays
WHOLE_ARRAY_ENTRY_POINTS = ('v3d_tsdf_normalize_f32', 'v3d_mesh_render_depth_f32', 'v3d_tsdf_resample_f32', 'v3d_volume_resample_nearest',
                            'v3d_segment_max_f32', 'v3d_lower_bound_u64', 'v3d_propagation_up_f32', 'v3d_soft_argmin_f32',
                            'v3d_confidence_logits_f32', 'v3d_probability_map_f32')


def missing_entry_points(cases, sized_by=None):
    """The entry points the table has to hold and does not: every function of the header with a `workspace` or `table` parameter, every
    size function (through SIZED_BY: it must name a case of the table), and the workspace-free ones above."""
    sized_by = SIZED_BY if sized_by is None else sized_by
    names = {c.name for c in cases}
    have = {e for c in cases for e in c.entry_points}
    have |= {f for f, case in sized_by.items() if case in names}
    return sorted((required_entry_points() | set(WHOLE_ARRAY_ENTRY_POINTS)) - have)


def workgroups(group):
    """(number of workgroups, ragged) of a groups() entry (kernel, items, items per workgroup[, independent batches])"""
    _, items, per = group[:3]
    if per is None:                                                            # one workgroup by design
        return 1, True
    batches = group[3] if len(group) > 3 else 1
    return batches * -(-items // per), items % per != 0


def exemption(group):
    """why a group is not held to the two-workgroup rule, or None"""
    if group[2] is None:
        return 'one workgroup by design'
    return group[4] if len(group) > 4 else None
