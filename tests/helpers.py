"""Shared helpers for the parity tests."""
import os

import numpy as np
import torch

from conftest import v3d

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load_golden(name):
    d = np.load(os.path.join(GOLDEN, name + '.npz'))
    return {k: d[k] for k in d.files}


def weights_checksum(sd):
    return float(sum(v.double().abs().sum().item() * (i + 1)
                     for i, (k, v) in enumerate(sorted(sd.items()))))


def golden_costreg_weights(g):
    """Re-create the seeded weights a fixture was generated with and verify their checksum."""
    syn = v3d('synthetic')
    sd = syn.costregnet_weights(seed=int(g['weights_seed']), sharpen=float(g['sharpen']))
    cs = weights_checksum(sd)
    assert abs(cs - float(g['weights_checksum'])) <= 1e-9 * abs(cs), \
        'seeded weights drifted from the ones the golden fixture was generated with'
    return sd


def t(x):
    return torch.from_numpy(np.asarray(x))


def state_as(sd, dtype, device=None):
    """The floating-point entries of a state dict in `dtype` (on `device`): what the functional oracles take as weights."""
    return {k: v.detach().to(device=device, dtype=dtype) for k, v in sd.items() if v.dtype.is_floating_point}


def decoder_reference(xs, pts, pts_feat, pts_batch, sd, chunk=8 * 3136):
    """oracle.scene.decoder_net(decoder_features(...)) a chunk of query points at a time (the [Nq, 7, 352] feature tensor of
    a 64-view scene is 4 GB in float64).  The result has the dtype of its inputs."""
    from oracle import scene as osc
    out = []
    for s in range(0, pts.shape[0], chunk):
        f = osc.decoder_features(xs, pts[s:s + chunk], None if pts_feat is None else pts_feat[s:s + chunk], pts_batch[s:s + chunk])
        out.append(osc.decoder_net(f, sd))
    return torch.cat(out)


def oracle_levels(xs, dtype):
    """Level dicts as oracle.scene consumes them, made from the ones a sparse U-Net returned (the oracle's or the HIP
    module's): the same features and voxel centres, cast to `dtype`, on the CPU."""
    out = []
    for x in xs:
        coords = x['sparse'].coords if 'sparse' in x else x['coords']
        out.append({'feats': x['feats'].detach().cpu().to(dtype), 'pts': x['pts'].detach().cpu().to(dtype), 'res': float(x['res']),
                    'batch': x['batch'].detach().cpu().long(), 'stride': int(x['stride']), 'coords': coords.detach().cpu().long()})
    return out


def pinned_project_to_grid(pts_ref, rotmats, tvecs, K, src_idx, img_size):
    """oracle.costvolume.project_to_grid with the host-independent evaluation orders of oracle/pinned.py (P = K [R|t] and
    P [X;1] spelled out with elementwise ops) instead of this host's torch.bmm, whose last bits depend on the host BLAS
    (MKL with and without FMA differ by one ulp in ~35 % of the coordinates): the goldens' projection on any host."""
    from oracle import pinned
    _, P = pinned.camera_blocks(K, rotmats, tvecs)
    Ps = P[src_idx]                                                       # [E, 3, 4]
    X = pts_ref.float()                                                   # [E, 3, n_pts]
    q = [pinned.dot3_chain(Ps[:, i, 0:1], X[:, 0], Ps[:, i, 1:2], X[:, 1], Ps[:, i, 2:3], X[:, 2]) + Ps[:, i, 3:4]
         for i in range(3)]
    zb = q[2].abs() + 1e-8
    gx = ((q[0] / zb) / float(img_size[1] - 1)) * 2 - 1.0
    gy = ((q[1] / zb) / float(img_size[0] - 1)) * 2 - 1.0
    return torch.stack((gx, gy), dim=-1).unsqueeze(2)                     # [E, n_pts, 1, 2]
