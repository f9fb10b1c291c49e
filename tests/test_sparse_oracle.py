"""CPU tests that pin tests/sparse_oracle.py, the checker of the sparse-structure GPU tests (tests/test_sparse_gpu.py): against
the torch oracle of the scene path (oracle/scene.py: sorted-key lookup, kernel offsets, strided coordinates, fp32 interpolation),
against a dense grid_sample, against closed forms, and -- the restated hash, which only chooses inputs -- against pairs worked out
by hand."""
import numpy as np
import torch
import torch.nn.functional as F

import sparse_oracle as so
from oracle import scene as osc


def _random_map(n=600, extent=9, seed=0, ts=1, lo=0):
    rng = np.random.default_rng(seed)
    c = np.concatenate((rng.integers(0, 2, (n, 1)), (rng.integers(0, extent, (n, 3)) + lo) * ts), axis=1)
    c = np.unique(c, axis=0)
    return c[rng.permutation(c.shape[0])]                       # row order is not the sorted order


def test_lookup_and_neighbours_equal_the_scene_oracle():
    coords = _random_map(seed=1)
    rng = np.random.default_rng(2)
    q = np.concatenate((rng.integers(0, 2, (500, 1)), rng.integers(-2, 11, (500, 3))), axis=1)
    q[:100] = coords[:100]
    got = so.lookup(coords, q)
    ref = osc._lookup(torch.from_numpy(coords), torch.from_numpy(q)).numpy()
    assert np.array_equal(got, ref)
    assert (got >= 0).sum() >= 100 and (got < 0).sum() > 50     # both outcomes occur
    assert np.array_equal(so.offsets(), osc.kernel_offsets().numpy())
    for step in (1, -1, 2):
        nbr = so.neighbours(coords, coords, step)
        assert nbr.shape == (27, coords.shape[0])
        cc = torch.from_numpy(coords)
        for k, o in enumerate(osc.kernel_offsets()):
            qq = cc.clone()
            qq[:, 1:] += step * o
            assert np.array_equal(nbr[k], osc._lookup(cc, qq).numpy()), (step, k)
        assert np.array_equal(nbr[13], np.arange(coords.shape[0]))


def test_strided_coords_floor_on_negative_inputs():
    coords = np.array([[0, -8, -7, -1], [0, -5, 0, 1], [0, -6, -2, 3], [1, -1, -1, -1], [1, 2, 3, -8], [0, -7, -8, -2]])
    assert so.strided_coords(coords, 1).tolist() == [[0, -8, -8, -2], [0, -6, -2, 2], [0, -6, 0, 0], [1, -2, -2, -2], [1, 2, 2, -8]]
    assert so.strided_coords(coords, 2).tolist() == [[0, -8, -8, -4], [0, -8, -4, 0], [0, -8, 0, 0], [1, -4, -4, -4], [1, 0, 0, -8]]
    assert so.strided_coords(coords, 4).tolist() == [[0, -8, -8, -8], [0, -8, -8, 0], [0, -8, 0, 0], [1, -8, -8, -8], [1, 0, 0, -8]]
    # and the scene oracle's floor division on a random map that reaches below zero
    c = _random_map(seed=3, extent=14, lo=-8)
    assert c[:, 1:].min() == -8
    for ts in (1, 2, 4):
        assert np.array_equal(so.strided_coords(c, ts), osc.strided_coords(torch.from_numpy(c), ts).numpy())


def _interp_case(seed, ts, n_q=400, c=6):
    rng = np.random.default_rng(seed)
    coords = _random_map(seed=seed, ts=ts)
    feats = rng.standard_normal((coords.shape[0], c)).astype(np.float32)
    res = 0.04 * ts
    min_pts = rng.uniform(-2, 2, (2, 3)).astype(np.float32)
    pts_batch = rng.integers(0, 2, n_q)
    pts = (min_pts[pts_batch] + rng.uniform(-1.5, 10.5, (n_q, 3)) * res).astype(np.float32)
    return coords, feats, res, min_pts, pts, pts_batch


def test_interp_agrees_with_the_scene_oracle_within_the_bound():
    """oracle.scene.sparse_interpolate is the same sum in fp32 (torch): 8 products and 8 additions, each rounded once, on weights
    that may differ from the checker's in the last place (torch.prod fixes no order) -- the 9 u S of the GPU tests covers the first,
    the weights are compared on their own."""
    worst = 0.0
    for seed, ts in ((10, 1), (11, 2), (12, 4)):
        coords, feats, res, min_pts, pts, pts_batch = _interp_case(seed, ts)
        val, s = so.interp(coords, feats, ts, pts, pts_batch, 1, min_pts, res)
        b, qc = so.query_coords(pts, pts_batch, 1, min_pts, res, ts)
        q = torch.cat((torch.from_numpy(b).float()[:, None], torch.from_numpy(qc)), dim=1)
        ref = osc.sparse_interpolate(torch.from_numpy(coords), torch.from_numpy(feats), ts, q).numpy()
        assert (s > 0).any(axis=1).sum() > 150 and (s == 0).all(axis=1).sum() > 5       # inside and outside both occur
        err = np.abs(ref - val)
        assert (err <= so.INTERP_BOUND * s).all()
        worst = max(worst, float((err[s > 0] / (so.INTERP_BOUND * s[s > 0])).max()))
    print('interp vs scene oracle: worst |diff| / (9 u S) = %.3f' % worst)


def test_interp_equals_dense_grid_sample_on_a_full_block():
    n, ts, c = 6, 2, 5
    rng = np.random.default_rng(20)
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing='ij'), -1).reshape(-1, 3)
    coords = np.concatenate((np.zeros((g.shape[0], 1), dtype=np.int64), g * ts), axis=1)
    perm = rng.permutation(coords.shape[0])
    coords = coords[perm]
    feats = rng.standard_normal((coords.shape[0], c)).astype(np.float32)
    res = 0.5                                                     # power of two: p -> lattice coordinate without rounding surprises
    u = rng.uniform(0, n - 1, (300, 3))                           # lattice units, inside the block
    pts = (u * res).astype(np.float32)
    val, s = so.interp(coords, feats, ts, pts, np.zeros(300, dtype=np.int64), 1, np.zeros((1, 3), np.float32), res)
    vol = torch.zeros((1, c, n, n, n), dtype=torch.float64)
    vol[0][:, coords[:, 1] // ts, coords[:, 2] // ts, coords[:, 3] // ts] = torch.from_numpy(feats).double().T
    grid = torch.from_numpy(pts.astype(np.float64) / res) / (n - 1) * 2 - 1
    samp = F.grid_sample(vol, grid[None, None, None][..., [2, 1, 0]], mode='bilinear', padding_mode='zeros', align_corners=True)
    # res and ts are powers of two and min_pts is 0: qc, c, qc - c and the quotient by ts are exact, so a weight carries the
    # roundings of its three (1 - .) factors and of two products, 5 u relative; the float64 grid_sample adds ~1e-16
    assert (np.abs(val - samp[0, :, 0, 0].T.numpy()) <= 6 * so.U * s + 1e-13).all()
    assert (s > 0).all()


def test_interp_closed_forms():
    rng = np.random.default_rng(30)
    for ts in (1, 2, 4):
        coords = _random_map(seed=31 + ts, ts=ts, extent=5, n=400)
        feats = rng.standard_normal((coords.shape[0], 8)).astype(np.float32)
        res = 0.125 * ts
        min_pts = np.array([[-1.5, 0.25, 3.0], [2.0, -4.0, 0.5]], dtype=np.float32)
        # on a lattice point: that row's features, exactly
        pts = (min_pts[coords[:, 0]] + (coords[:, 1:] // ts) * res).astype(np.float32)
        val, _ = so.interp(coords, feats, ts, pts, coords[:, 0], 1, min_pts, res)
        assert np.array_equal(val, feats.astype(np.float64))
        # at the centre of a cell whose 8 corners are present: their mean
        table = {tuple(r): i for i, r in enumerate(coords.tolist())}
        cells = [(r, [table.get((r[0], r[1] + dx, r[2] + dy, r[3] + dz)) for dz in (0, ts) for dy in (0, ts) for dx in (0, ts)])
                 for r in coords.tolist()]
        cells = [(r, k) for r, k in cells if None not in k]
        assert len(cells) >= 5
        base = np.array([r for r, _ in cells])
        pts = (min_pts[base[:, 0]] + (base[:, 1:] // ts + 0.5) * res).astype(np.float32)
        val, _ = so.interp(coords, feats, ts, pts, base[:, 0], 1, min_pts, res)
        mean = np.stack([feats[k].astype(np.float64).mean(axis=0) for _, k in cells])
        assert np.array_equal(val, mean)                                      # weights 1/8: exact in float64
        # every corner absent: below the minimum, beyond the range guard, another batch's empty space, far away
        far = np.array([[-3, 1, 1], [1, 1, -9.5], [70000, 1, 1], [1e6 / res, 0, 0], [200, 200, 200]]) * res
        pts = (min_pts[0] + far).astype(np.float32)
        val, s = so.interp(coords, feats, ts, pts, np.zeros(5, dtype=np.int64), 1, min_pts, res)
        assert (val == 0).all() and (s == 0).all()


def test_interp_range_guard_and_hypothesis_layout():
    """Rows at -8 and 60000 are found, rows the table may hold beyond 60000 are not looked up; n_hyp repeats the batch id."""
    coords = np.array([[0, -8, -8, -8], [0, 60000, 0, 0], [0, 60001, 0, 0], [1, 0, 0, 0]])
    feats = np.array([[1.], [2.], [4.], [8.]], dtype=np.float32)
    min_pts = np.zeros((2, 3), dtype=np.float32)
    pts = np.array([[[-8, -8, -8], [-8.5, -8, -8]], [[60000.5, 0, 0], [60001, 0, 0]], [[0, 0, 0], [0.5, 0, 0]]], dtype=np.float32)
    rows, w, _ = so.corner_table(coords, 1, pts, [0, 0, 1], 2, min_pts, 1.0)
    val, _ = so.interp(coords, feats, 1, pts, [0, 0, 1], 2, min_pts, 1.0)
    assert val[:, 0].tolist() == [1.0, 0.5, 1.0, 0.0, 8.0, 4.0]
    assert rows[1].tolist() == [-1, 0, -1, -1, -1, -1, -1, -1]                 # lower x corner is -9: outside the guard
    assert rows[2, 1] == -1 and rows[3, 0] == -1                               # 60001 is in the map and still absent


def test_restated_hash_reproduces_hand_computed_slots():
    """(coordinate -> packed key -> 32-bit hash -> slot of a 256-slot table), worked out with exact integer arithmetic from the
    formulas of sparse_hash.h."""
    pairs = [((0, 0, 0, 0), 0x800080008, 0x23fa54ce, 206),
             ((1, 2, 3, 4), 0x1000a000b000c, 0x95d852d4, 212),
             ((65535, -8, 65519, -8), 0xffff0000fff70000, 0x42d6bc74, 116),
             ((0, 65519, 0, 0), 0xfff700080008, 0xe47c483c, 60),
             ((3, -1, -1, -1), 0x3000700070007, 0x0d4c753e, 62),
             ((1, 100, 200, 300), 0x1006c00d00134, 0x6ec3d622, 34)]
    c = np.array([p[0] for p in pairs])
    keys = so.pack_key(c[:, 0], c[:, 1], c[:, 2], c[:, 3])
    assert [int(k) for k in keys] == [p[1] for p in pairs]
    assert [int(h) for h in so.hash_u64(keys)] == [p[2] for p in pairs]
    assert so.table_capacity(40) == 256 and so.table_capacity(64) == 256 and so.table_capacity(65) == 512
    assert so.home_slot(c, 40).tolist() == [p[3] for p in pairs]
    assert [so.table_capacity(n) for n in (1, 15, 16, 17, 4096, 4097, 20000)] == [64, 64, 64, 128, 16384, 32768, 131072]
