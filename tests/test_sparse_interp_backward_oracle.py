"""CPU: the float64 oracle of the sparse interpolation's backward (tests/sparse_interp_backward_oracle.py) is right, its bound
is not vacuous on the inputs of tests/test_sparse_interp_backward_gpu.py and rejects wrong backward passes; the training module's new
functions refuse CPU tensors.  Every figure is printed before it is asserted."""
import os
import re

import numpy as np
import pytest
import torch

import sparse_interp_backward_oracle as sbo
from conftest import ROOT, v3d

# share of the elements a wrong backward pass can affect that it must push outside the bound (or to NaN); below the smallest share
# measured over all cases (reversed_bits on exact-C128-ts4-h7: 97.8 %)
FLOOR = 0.90


@pytest.fixture(scope='module', params=sbo.CASES, ids=sbo.case_id)
def case_orc(request):
    case = sbo.build(request.param)
    return request.param, case, sbo.gradient(case)


def test_chunk_constant_is_the_kernels():
    src = open(os.path.join(ROOT, '3dvnet_amd', 'csrc', 'sparse_interp.hip')).read()
    assert int(re.search(r'constexpr int kInterpBwdChunk = (\d+);', src).group(1)) == sbo.CHUNK
    assert sbo.N_HOT > 3 * sbo.CHUNK and sbo.N_HOT % sbo.CHUNK != 0


def test_inputs_hold_what_they_are_for(case_orc):
    """About 200 shuffled rows from -8 upward in two batch elements; queries inside, on the rim (1 .. 7 corners present), outside
    (none), on lattice points (a weight of exactly 1); rows with lists of 0; the hot cases a list of more than three chunks beside
    lists of 0 and 1; the strided cases NaN wherever the gradient is not."""
    param, case, orc = case_orc
    coords, rows, w, cnt = case['coords'], orc['rows'], orc['w'], orc['cnt']
    assert 170 <= coords.shape[0] <= 230 and coords[:, 1:].min() == -8 and set(coords[:, 0].tolist()) == {0, 1}
    assert not np.array_equal(coords, coords[np.lexsort(coords.T[::-1])])                    # shuffled
    nq = case['n_pts'] * case['n_hyp']
    assert rows.shape == (nq, 8) and 2000 <= nq <= 7000
    present = (rows >= 0).sum(axis=1).reshape(case['n_pts'], case['n_hyp'])[:, 0]
    kinds = case['kinds']
    assert (present[kinds == 'inside'] == 8).any() and set(range(1, 8)) & set(present[kinds == 'rim'].tolist())
    assert (present[kinds == 'outside'] == 0).all() and (kinds == 'outside').sum() >= 50
    far = np.abs(case['lattice_units'][:, 0]).max(axis=1) * case['ts'] > so_max()
    assert far.sum() >= 10                                                                   # beyond the 60000 range guard
    assert (w[np.repeat(kinds == 'lattice', case['n_hyp'])] == 1).any()                       # exactly on a lattice point
    assert (rows[(case['lattice_units'].reshape(-1, 3) < -8 / case['ts'] + 1).any(axis=1)] >= 0).any()
    assert (cnt == 0).sum() >= 1 and (cnt == 1).sum() >= 1 and cnt.max() < 2000
    print('%s: %d rows, %d queries, list length median %d max %d, rows with cnt == 0: %d'
          % (sbo.case_id(param), coords.shape[0], nq, int(np.median(cnt)), cnt.max(), (cnt == 0).sum()))
    if param[0].startswith('hot'):
        assert (cnt > 3 * sbo.CHUNK).sum() == 8 and ((cnt % sbo.CHUNK) != 0)[cnt > sbo.CHUNK].all()
        assert (cnt == 0).any() and (cnt == 1).any()
    if param[0].startswith('strided'):
        g = case['grad_out']
        assert case['ld'] > case['C'] and case['col0'] > 0 and np.isnan(g[:, :case['col0']]).all() \
            and np.isnan(g[:, case['col0'] + case['C']:]).all() and np.isfinite(g[:, case['col0']:case['col0'] + case['C']]).all()
        assert (case['col0'] % 4 == 0 and case['ld'] % 4 == 0) == (param[0] == 'strided_vec')
    if case['exact']:
        assert np.array_equal(case['pts'].astype(np.float64), case['min_pts'][case['pts_batch']].astype(np.float64)[:, None, :]
                              + case['lattice_units'] * case['res'])
        assert np.array_equal(np.round(w.astype(np.float64) * 64), w.astype(np.float64) * 64)  # multiples of 1/64
        assert np.array_equal(orc['g64'].astype(np.float32).astype(np.float64), orc['g64']) and np.abs(orc['g64']).max() < 2 ** 15


def so_max():
    import sparse_oracle as so
    return so.INTERP_MAX


def test_oracle_matches_float64_autograd(case_orc):
    """g64 against float64 autograd of the dense stock formulation (gather feats[rows] -> weight -> sum).  Seen 0: np.add.at and
    index_put's backward add the same float64 terms in the same order."""
    param, case, orc = case_orc
    rows, w = torch.from_numpy(orc['rows']), torch.from_numpy(orc['w']).double()
    feats = torch.zeros(case['coords'].shape[0], case['C'], dtype=torch.float64, requires_grad=True)
    gathered = feats[rows.clamp(min=0)] * (rows >= 0).double().unsqueeze(-1)                  # [nq, 8, C]
    out = (gathered * w.unsqueeze(-1)).sum(dim=1)
    g = torch.from_numpy(case['grad_out'][:, case['col0']:case['col0'] + case['C']]).double()
    out.backward(g)
    scale = float(np.abs(orc['g64']).max())
    err = float((feats.grad - torch.from_numpy(orc['g64'])).abs().max())
    print('%s: max|g64 - autograd| = %.3g at max|g64| = %.3g' % (sbo.case_id(param), err, scale))
    assert scale > 0 and err <= 1e-11 * scale
    assert np.isfinite(orc['g64']).all() and np.isfinite(orc['S']).all()
    assert not orc['g64'][orc['cnt'] == 0].any() and not orc['S'][orc['cnt'] == 0].any()


def test_bound_is_not_vacuous_and_holds_a_float32_evaluation(case_orc):
    """max(bound) / max|g64| < 1e-2 (seen 1.4e-5 .. 4.1e-5, the hot rows 1.2e-3 and 1.7e-3: cnt = 1838 and
    S / |g64| of the order of sqrt(cnt)); the oracle is inside its own bound; the same terms summed
    in float32 by np.add.at lie inside it (seen worst ratio <= 0.20)."""
    param, case, orc = case_orc
    b, scale = sbo.bound(orc), float(np.abs(orc['g64']).max())
    print('%s: max bound / max|g64| = %.3g' % (sbo.case_id(param), float(b.max()) / scale))
    assert float(b.max()) / scale < 1e-2
    assert sbo.violations(orc['g64'], orc)[0] == 0
    rows, w = orc['rows'].reshape(-1), orc['w'].reshape(-1)
    g = case['grad_out'][:, case['col0']:case['col0'] + case['C']]
    keep = rows >= 0
    g32 = np.zeros(orc['g64'].shape, dtype=np.float32)
    np.add.at(g32, rows[keep], w[keep][:, None] * g[np.nonzero(keep)[0] >> 3])
    assert g32.dtype == np.float32
    bad, worst, worst_zero = sbo.violations(g32, orc)
    print('   float32 on the CPU: worst |g32 - g64| / bound = %.3f, outside: %d' % (worst, bad))
    assert bad == 0 and worst_zero == 0.0
    if case['exact']:
        assert np.array_equal(g32.astype(np.float64), orc['g64'])


def _affected(case, orc, wrong, variant):
    """The elements a variant can change."""
    touched = (orc['S'] > 0) | (wrong['S'] > 0) | np.isnan(wrong['S'])
    if variant == 'clamp_absent':
        touched = touched & (np.arange(orc['cnt'].shape[0]) == 0)[:, None]
    if variant == 'drop_last_chunk':
        touched = touched & (orc['cnt'] > sbo.CHUNK)[:, None]
    return touched


def test_wrong_backward_passes_leave_the_bound(case_orc):
    """1 - w weights, reversed corner bits, absent corners clamped to row 0, pts_batch indexed by query, col0 ignored, the last
    chunk of the hot rows dropped: the share of the affected elements outside the bound.  Seen: one_minus_w 99.9 .. 100 %,
    reversed_bits 97.8 .. 99.5 %, clamp_absent 100 %, batch_by_query 99.3 .. 100 %, col0_ignored 100 % (NaN), drop_last_chunk
    99.6 .. 100 %."""
    param, case, orc = case_orc
    for variant in sbo.VARIANTS:
        if variant == 'batch_by_query' and param[3] == 1:
            continue                                             # one hypothesis: the two indexings agree
        if variant == 'col0_ignored' and case['col0'] == 0:
            continue
        if variant == 'drop_last_chunk' and not param[0].startswith('hot'):
            continue
        wrong = sbo.gradient(case, variant)
        where = _affected(case, orc, wrong, variant)
        assert int(where.sum()) >= case['C'], variant
        bad = ~(np.abs(wrong['g64'] - orc['g64']) <= sbo.bound(orc)) & where
        frac = float(bad.sum()) / float(where.sum())
        print('%s %s: outside the bound on %.1f %% of %d affected elements' % (sbo.case_id(param), variant, 100 * frac, where.sum()))
        assert frac >= FLOOR, variant


def test_training_functions_refuse_the_cpu():
    tr, lib = v3d('training'), v3d('_lib')
    x = dict(feats=torch.zeros(3, 4, requires_grad=True), sparse=None, stride=1, res=0.1, pts=torch.zeros(3, 3),
             batch=torch.zeros(3, dtype=torch.long))
    with pytest.raises(lib.V3DLibraryError):
        tr.sparse_interpolate(x, torch.zeros(5, 2, 3), torch.zeros(5, dtype=torch.long))
    with pytest.raises(lib.V3DLibraryError):
        tr.decoder_features([x], torch.zeros(5, 2, 3), None, torch.zeros(5, dtype=torch.long))
