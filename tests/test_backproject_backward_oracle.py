"""CPU: the float64 oracle of the back-projected variance's gradients (tests/backproject_backward_oracle.py) is right, its
acceptance bounds are not vacuous on the inputs of tests/test_backproject_backward_gpu.py and reject wrong gradients; the training
module's new functions refuse CPU tensors.  Every figure is printed before it is asserted."""
import pytest
import torch

import backproject_backward_oracle as bbo
from conftest import v3d

FLOOR = 0.70            # share of the non-zero elements (of the images a bug can change) that a wrong gradient must push outside


@pytest.fixture(scope='module', params=bbo.ALL_CASES, ids=bbo.case_id)
def case_orc(request):
    case = bbo.build(request.param)
    return request.param, case, bbo.gradient(case)


def test_inputs_hold_the_special_pixels():
    case = bbo.make_case(32, 'rotated', 3)
    d = case['depth_map']
    assert d.shape == (3, 7, 9) and float(d[-1, 0, 0]) == pytest.approx(0.1) and float(d[-1, 0, 1]) == 0.0 and torch.isnan(d[-1, 0, 2])
    assert float(d[-1, 0, 0]) - 3 * case['offset'] < 0                        # hypotheses behind the camera
    assert case['gvar'].shape == (3 * 63, 7, 32) and case['gpts'].shape == (3 * 63, 1, 3)
    assert torch.bincount(case['edges'][0]).tolist() == [1, 3, 4] and 4 not in case['edges'].flatten().tolist()
    pos = bbo.positions(case)
    assert any(bool(torch.isnan(ix).any()) for _, _, ix, _ in pos)
    chunk = bbo.make_chunk_case(16, 'dense', 4)
    assert torch.bincount(chunk['edges'][0]).tolist() == [8, 9, 17] and chunk['unused'] == 18
    assert chunk['depth_map'].shape == (3, 5, 7) and chunk['gvar'].shape == (105, 9, 16)
    assert sorted(2 * p[3] + 1 for p in bbo.SEGMENT_CASES) == [1, 3, 7, 15, 17, 33]


def test_oracle_matches_float64_autograd(case_orc):
    """g64 against float64 autograd through F.grid_sample on the float64 grid of the pinned positions.  Seen <= 3.2e-15."""
    param, case, orc = case_orc
    ref = bbo.autograd_reference(case)
    err = float((orc['g64'] - ref).abs().max())
    print('%s: max|g64 - autograd| = %.3g at max|g64| = %.3g' % (bbo.case_id(param), err, float(orc['g64'].abs().max())))
    assert err <= 1e-12
    assert torch.isfinite(orc['g64']).all() and torch.isfinite(orc['M']).all()
    assert not orc['g64'][case['unused']].any() and not orc['N'][case['unused']].any()


def test_bound_is_not_vacuous_and_holds_a_float32_evaluation(case_orc):
    """max(bound) / max|g64| < 1e-3 (seen 4.9e-6 .. 5.1e-5); the oracle is inside its own bound; the same taps and weights in
    float32 torch ops on the CPU lie inside it (seen worst ratio 0.037 .. 0.079)."""
    param, case, orc = case_orc
    b, scale = bbo.bound(orc), float(orc['g64'].abs().max())
    print('%s: max bound / max|g64| = %.3g' % (bbo.case_id(param), float(b.max()) / scale))
    assert scale > 0 and float(b.max()) / scale < 1e-3
    assert bbo.violations(orc['g64'], orc)[0] == 0
    g32 = bbo.gradient(case, dtype=torch.float32)['g64']
    assert g32.dtype == torch.float32
    bad, worst, worst_zero = bbo.violations(g32, orc)
    print('   float32 on the CPU: worst |g32 - g64| / bound = %.3f, outside: %d' % (worst, bad))
    assert bad == 0 and worst_zero == 0.0


def _share_outside(case, orc, variant):
    wrong = bbo.gradient(case, variant=variant)['g64']
    where = (orc['g64'] != 0) & bbo.affected_images(case, variant)[:, None, None, None]
    assert int(where.sum()) > 1000, variant
    bad = ((wrong - orc['g64']).abs() > bbo.bound(orc)) & where
    return float(bad.sum()) / float(where.sum()), int(where.sum())


@pytest.mark.parametrize('param', [p for p in bbo.CASES if p[2] == 3], ids=bbo.case_id)
def test_wrong_gradients_leave_the_bound(param):
    """no_avg, global_cnt, swap_ne_sw, tail_hyp, centre_only on every base case of n = 3; reversed_hyp on the 'sliding' cameras (on
    'rotated' most samples are outside the image and it reaches only about a third: it is judged where the samples are inside, the
    floor is not lowered for it).  Seen 76.1 .. 100 %."""
    case = bbo.build(param)
    orc = bbo.gradient(case)
    for variant in bbo.BASE_VARIANTS:
        frac, n = _share_outside(case, orc, variant)
        judged = variant != 'reversed_hyp' or param[1] != 'rotated'
        print('%s %s: outside the bound on %.1f %% of %d non-zero elements%s' % (bbo.case_id(param), variant, 100 * frac, n,
                                                                                  '' if judged else ' (not judged on these cameras)'))
        if judged:
            assert frac >= FLOOR, variant


@pytest.mark.parametrize('param', bbo.CHUNK_CASES, ids=bbo.case_id)
def test_chunk_bugs_leave_the_bound(param):
    """avg_first_chunk, drop_later_chunks, stale_records, tail_hyp, first_segment (n = 4: nine hypotheses, one past the segment of
    8) over the images each can change.  Seen 84.5 / 76.1 / 84.5 / 98.6 / 98.6 % on 'rotated', >= 96.3 % on 'dense';
    reversed_hyp is judged on 'dense'."""
    case = bbo.build(param)
    orc = bbo.gradient(case)
    assert orc['cnt_max'] == 17
    for variant in bbo.CHUNK_VARIANTS + (('reversed_hyp',) if param[2] == 'dense' else ()):
        frac, n = _share_outside(case, orc, variant)
        print('%s %s: outside the bound on %.1f %% of %d non-zero elements' % (bbo.case_id(param), variant, 100 * frac, n))
        assert frac >= FLOOR, variant


def test_depth_oracle():
    """The depth oracle equals float64 autograd through R^T (Kinv p d - t) (seen 9e-16); its bound 16 * 2^-24 * M_d is small
    against the gradient (seen 2e-6), holds a float32 evaluation of the chains (seen 0.097) and rejects R for R^T and a dropped z
    term on every pixel (seen 100 %)."""
    for param in ((32, 'rotated', 0), (32, 'sliding', 0), ('chunk', 32, 'dense', 0)):
        case = bbo.build(param)
        g64, M = bbo.depth_gradient(case)
        err = float((g64 - bbo.depth_autograd_reference(case)).abs().max())
        b = bbo.depth_bound(M)
        print('%s: max|g64 - autograd| = %.3g, max bound / max|g64| = %.3g' % (bbo.case_id(param), err, float(b.max() / g64.abs().max())))
        assert err <= 1e-12 and torch.isfinite(g64).all()
        assert float(b.max() / g64.abs().max()) < 1e-3
        # float32: the kernel's three nested chains with plain float32 torch ops (no FMA: one more rounding per term)
        Kinv, R, p = (x.float() for x in bbo._rays(case))
        c = [Kinv[:, i, 0:1] * p[0] + Kinv[:, i, 1:2] * p[1] + Kinv[:, i, 2:3] * p[2] for i in range(3)]
        ray = [R[:, 0, j:j + 1] * c[0] + R[:, 1, j:j + 1] * c[1] + R[:, 2, j:j + 1] * c[2] for j in range(3)]
        gp = case['gpts'].reshape(g64.shape[0], -1, 3)
        g32 = (gp[..., 0] * ray[0] + gp[..., 1] * ray[1] + gp[..., 2] * ray[2]).reshape(g64.shape)
        bad, worst = bbo.depth_violations(g32, g64, M)
        print('   float32 on the CPU: worst |g32 - g64| / bound = %.3f, outside: %d' % (worst, bad))
        assert bad == 0
        for variant in bbo.DEPTH_VARIANTS:
            wrong, _ = bbo.depth_gradient(case, variant=variant)
            frac = float(((wrong - g64).abs() > b).double().mean())
            print('   %s: outside the bound on %.1f %% of the pixels' % (variant, 100 * frac))
            assert frac >= FLOOR, variant


def test_training_functions_refuse_the_cpu():
    tr, lib = v3d('training'), v3d('_lib')
    case = bbo.make_case(32, 'rotated', 3)
    args = (case['depth_map'], case['feat'].requires_grad_(True), case['rotmats'], case['tvecs'], case['K'], case['edges'],
            case['img_size'])
    with pytest.raises(lib.V3DLibraryError):
        tr.backproject_variance(*args, offset=0.05, n=3)
    batch = torch.zeros(3, dtype=torch.long)
    with pytest.raises(lib.V3DLibraryError):
        tr.feature_rich_pointcloud(args[0], batch, *args[1:])
    with pytest.raises(lib.V3DLibraryError):
        tr.pointflow_hypotheses(args[0], batch, *args[1:6], 0.05, 3, case['img_size'])
