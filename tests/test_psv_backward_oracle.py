"""CPU: the float64 oracle of the plane-sweep variance gradient (tests/psv_backward_oracle.py) is right and its acceptance bound
is not vacuous on the inputs of tests/test_psv_backward_gpu.py; the training module imports, refuses CPU tensors, and its
functional regulariser equals the oracle's."""
import pytest
import torch

import psv_backward_oracle as pbo
from conftest import v3d
from oracle import costvolume as cv


@pytest.fixture(scope='module', params=pbo.CASES, ids=lambda p: '%d-%s' % p)
def case_orc(request):
    case = pbo.make_case(*request.param)
    return case, pbo.gradient(case)


def test_inputs_exercise_the_edge_cases():
    """Mirrored samples, samples partly outside, sources wholly outside on some planes but not on all; the 1-edge reference;
    the unused image."""
    case = pbo.make_case(32)
    K, R, t = case['K'], case['rotmats'], case['tvecs']
    _, P = pbo.pin.camera_blocks(K, R, t)
    Hf, Wf = case['feat'].shape[2:]
    D, n_pix = case['depth'][2], case['plane_size'][0] * case['plane_size'][1]
    mirrored = partly = 0
    wholly_some_planes = False
    for r, src, ix, iy in pbo.positions(case):
        ref = torch.unique(case['edges'][0]).tolist()[r]
        X = pbo.pin.world_points(K, R, t, ref, *case['depth'], case['img_size'], case['plane_size'])
        qz = P[src, 2, 0] * X[0] + P[src, 2, 1] * X[1] + P[src, 2, 2] * X[2] + P[src, 2, 3]
        mirrored += int((qz < 0).sum())
        inside = [ok for _, _, ok in pbo._taps(ix, iy, Hf, Wf)]
        n_in = sum(o.long() for o in inside)
        partly += int(((n_in > 0) & (n_in < 4)).sum())
        out_plane = (n_in == 0).view(D, n_pix).all(dim=1)
        wholly_some_planes |= bool(out_plane.any() and not out_plane.all())
    assert mirrored > 0 and partly > 0 and wholly_some_planes
    counts = torch.bincount(case['edges'][0]).tolist()
    assert counts == [1, 3, 4] and 4 not in case['edges'].flatten().tolist()


def test_oracle_matches_autograd(case_orc):
    """(a) g64 against torch.autograd through oracle.costvolume's chain (features in float64): the two differ only through
    the fp32 rounding of the positions (~1e-6 relative); an indexing or sign mistake is O(1)."""
    case, orc = case_orc
    ref = pbo.autograd_reference(case)
    scale = float(orc['g64'].abs().max())
    err = float((orc['g64'] - ref).abs().max())
    print('max|g64 - autograd| / max|g64| = %.3g' % (err / scale))
    assert err <= 1e-4 * scale


def test_bound_is_tight_and_rejects_wrong_gradients(case_orc):
    """(b) the acceptance bound (N + 32) 2^-24 M is at most 1e-3 max|g64| on at least 99 % of the elements, and three wrong
    gradients each violate it on at least half of the non-zero elements."""
    case, orc = case_orc
    b, scale = pbo.bound(orc), float(orc['g64'].abs().max())
    tight = float((b <= 1e-3 * scale).double().mean())
    print('bound <= 1e-3 max|g64| on %.2f %% of the elements; max bound / max|g64| = %.3g' % (100 * tight, float(b.max()) / scale))
    assert tight >= 0.99
    nonzero = orc['g64'] != 0
    assert int(nonzero.sum()) > 1000
    for variant in ('no_avg', 'global_cnt', 'swap_ne_sw'):
        wrong = pbo.gradient(case, variant=variant)['g64']
        bad = ((wrong - orc['g64']).abs() > b) & nonzero
        frac = float(bad.sum()) / float(nonzero.sum())
        print('%s: outside the bound on %.1f %% of the non-zero elements' % (variant, 100 * frac))
        assert frac >= 0.5, variant
    # the oracle itself is inside its bound, and the 1-edge reference and the unused image contribute exactly nothing
    assert pbo.violations(orc['g64'], orc)[0] == 0
    assert not orc['g64'][4].any() and not orc['N'][4].any()
    only_ref0 = torch.zeros_like(case['gvar'])
    only_ref0[0] = case['gvar'][0]
    assert not pbo.gradient(case, gvar=only_ref0)['g64'].any()


def test_training_module_on_the_cpu():
    """(c) the module imports, the autograd function refuses CPU tensors, and the functional regulariser with running
    statistics equals oracle.costvolume.costregnet."""
    tr, mvs, syn, lib = v3d('training'), v3d('mvsnet'), v3d('synthetic'), v3d('_lib')
    case = pbo.make_case(32)
    with pytest.raises(lib.V3DLibraryError):
        tr.plane_sweep_variance(case['feat'].requires_grad_(True), case['rotmats'], case['tvecs'], case['K'], case['edges'],
                                *case['depth'], case['img_size'], case['plane_size'])
    csr = mvs.edges_to_csr(case['edges'])
    with pytest.raises(lib.V3DLibraryError):
        tr.PlaneSweepVariance.apply(case['feat'], case['K'], case['rotmats'], case['tvecs'], csr[1], csr[2], csr[3],
                                    case['depth'] + (case['img_size'], case['plane_size']))
    sd = syn.costregnet_weights(seed=0, sharpen=200.0)
    net = mvs.CostRegNet(32, 8).eval()
    keys = set(net.state_dict())
    net.load_state_dict(sd, strict=False)
    x = torch.rand((2, 32, 8, 8, 8), generator=torch.Generator().manual_seed(1)) * 0.1
    with torch.no_grad():
        got, want = tr.costregnet(net, x), cv.costregnet(x, sd)
    assert got.shape == (2, 1, 8, 8, 8) and torch.equal(got, want)
    assert set(net.state_dict()) == keys
    # batch statistics: another result, and the running buffers move
    before = net.conv0.bn.running_mean.clone()
    with torch.no_grad():
        trained = tr.costregnet(net, x, bn_training=True)
    assert not torch.equal(trained, got) and not torch.equal(net.conv0.bn.running_mean, before)
