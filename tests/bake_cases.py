"""Shared constructions of the texture-bake tests (tests/test_bake_cpu.py, tests/test_bake_gpu.py): the meshes, seeded query sets that
visit the places where an atlas goes wrong (corners, edges, the hypotenuse, the last cell of a row and of the atlas, misses), an affine
field, texel values around the byte ties, and the stage-2 models.  Everything is numpy / CPU torch and deterministic; the definition's
results are computed once per case and handed out read-only."""
import functools

import numpy as np
import torch

from tests import inside_cases, raycast_cases as rc
from psnerf_amd import meshbake as mb

SIZES = (16, 17, 64, 256)


# ------------------------------------------------------------------------------------------------ meshes
@functools.lru_cache(maxsize=None)
def meshes():
    """name -> (vertices, faces, vertex normals or None)."""
    out = {}
    out['a single triangle'] = (np.array([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.5, 0.9]]), np.array([[0, 1, 2]], dtype=np.int64), None)
    tv = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) * 0.37
    tf = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int64)
    tn = tv / np.linalg.norm(tv, axis=1, keepdims=True)
    tn[3] = 0.0                                                          # a zero vertex normal, and with it rows whose sum is short
    out['a tetrahedron'] = (tv, tf, tn)
    v1, f1 = rc.icosphere(1)
    out['icosphere(1)'] = (v1, f1, v1.copy())                             # 80 faces; the vertices of a unit sphere are its normals
    v2, f2 = rc.icosphere(2)
    out['icosphere(2)'] = (v2, f2, None)
    sv, sf = inside_cases.mc_sphere_small()[:2]
    out['mc sphere'] = (np.asarray(sv, dtype=np.float64), np.asarray(sf, dtype=np.int64), None)
    zero = np.array([[f1[3, 0], f1[3, 1], f1[3, 1]], [f1[5, 2], f1[5, 2], f1[5, 2]]], dtype=np.int64)     # a repeated corner; a point
    mid = np.concatenate([v1, 0.5 * (v1[f1[7, 0]] + v1[f1[7, 1]])[None]])                                # a collinear triple
    coll = np.array([[f1[7, 0], len(v1), f1[7, 1]]], dtype=np.int64)
    out['zero-area faces'] = (mid, np.concatenate([f1[:10], zero, coll, f1[10:20]]), None)
    out['an odd face count'] = (v1, f1[:79].copy(), v1.copy())            # the last cell holds one face
    for v, f, n in out.values():
        for a in (v, f) + (() if n is None else (n,)):
            a.setflags(write=False)
    return out


def fits(T, F):
    """Whether F faces fit a T x T atlas at all (cells of 4 texels); what does not fit must raise."""
    g = min(g for g in range(1, F + 2) if g * g >= (F + 1) // 2)       # the fewest cells per side
    return T // g >= 4, 4 * g


def face_ranges(F):
    """Face ranges that start and end mid-cell (odd f0, odd f1), next to the whole and the ends."""
    r = [(0, F)]
    if F >= 4:
        r += [(1, F - (F % 2 == 0)), (1, 3), (F - 1, F), (0, 1)]
    if F >= 40:
        r += [(17, 33), (F // 2 | 1, (F // 2 | 1) + 2)]
    return [(a, b) for a, b in dict.fromkeys(r) if 0 <= a < b <= F]


# ------------------------------------------------------------------------------------------------ queries
def queries(atlas, Q, seed=0, misses=True):
    """(face int64 [Q], bary float64 [Q, 3]): corners, edge midpoints, hypotenuse and interior points (b >= 0), on random faces and on
    the faces in the last cell of the first cell row and of the atlas, with misses (-1, NaN barycentrics) and faces beyond F between."""
    g = np.random.RandomState(seed)
    F = atlas.F
    special = np.unique(np.clip(np.array([0, 1, 2 * atlas.G - 2, 2 * atlas.G - 1, 2 * atlas.G, F - 2, F - 1]), 0, F - 1))
    face = g.randint(0, F, Q).astype(np.int64)
    face[::3] = special[np.arange(len(face[::3])) % len(special)]
    bary = g.dirichlet(np.ones(3), Q)
    kind = np.arange(Q) % 8
    eye = np.eye(3)
    bary[kind == 0] = eye[g.randint(0, 3, int((kind == 0).sum()))]                      # corners
    mids = np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]])
    bary[kind == 1] = mids[g.randint(0, 3, int((kind == 1).sum()))]                     # edge midpoints
    t = g.random_sample(int((kind == 2).sum()))
    bary[kind == 2] = np.stack([np.zeros_like(t), t, 1.0 - t], axis=1)                  # on the hypotenuse
    t = g.random_sample(int((kind == 3).sum()))
    bary[kind == 3] = np.stack([1.0 - t, t, np.zeros_like(t)], axis=1)                  # on a leg
    if misses and Q >= 8:
        miss = kind == 5
        face[miss] = np.where(np.arange(int(miss.sum())) % 4 == 3, F + 5, -1)
        bary[miss & (face == -1)] = np.nan
    return face, np.ascontiguousarray(bary)


def surface_points(v, f, face, bary):
    a, b, c = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    return bary[:, 0:1] * a + bary[:, 1:2] * b + bary[:, 2:3] * c


# ------------------------------------------------------------------------------------------------ fields and values
AFFINE_A = np.array([[0.83, -0.41, 0.27], [-0.19, 0.66, 0.52], [0.31, 0.48, -0.77], [0.05, -0.92, 0.14]])     # [C = 4, 3]
AFFINE_B = np.array([0.3, -1.1, 0.45, 2.0])


def affine(p):
    """f(p) = A p + b -> [..., 4], float64."""
    return np.asarray(p, dtype=np.float64) @ AFFINE_A.T + AFFINE_B


def bake_affine(atlas, v, f):
    """The affine field baked through the definition: points -> float32 rows -> texture.  -> (texture float32 [T, T, 4], max |f| over
    the rows)."""
    p = mb.host_atlas_points(atlas, v, f)[0]
    rows = affine(p)
    return mb.host_atlas_scatter(atlas, rows.astype(np.float32)), float(np.abs(rows).max())


def tie_values():
    """float32 texel values on the .5 ties of x * 255, just beside them, below 0, above 1, infinite and NaN."""
    k = np.arange(0, 255, dtype=np.float64)
    ties = ((k + 0.5) / 255.0).astype(np.float32)
    vals = [ties, np.nextafter(ties, np.float32(2.0)), np.nextafter(ties, np.float32(-1.0)), (k / 255.0).astype(np.float32),
            np.array([-0.0, -1e-30, -0.3, -7.0, 1.0, 1.0000001, 1.7, 1e30, np.inf, -np.inf, np.nan, 0.5, 0.49999997, 0.50000006], dtype=np.float32)]
    # the products that land EXACTLY on k + 0.5 in float32: x = (k + 0.5) / 255 rounded may or may not; search next to each tie
    exact = []
    for x in ties:
        for y in (x, np.nextafter(x, np.float32(2.0)), np.nextafter(x, np.float32(-1.0))):
            p = np.float32(y) * np.float32(255.0)
            if p - np.floor(p) == np.float32(0.5):
                exact.append(y)
    assert len(exact) >= 20
    return np.concatenate(vals + [np.array(exact, dtype=np.float32)])


def rows_for(n_rows, C, seed):
    """float32 rows [n_rows, C]: mostly values in [-0.2, 1.2], the tie values and NaN / infinities sprinkled in."""
    g = np.random.RandomState(seed)
    rows = (g.random_sample((n_rows, C)) * 1.4 - 0.2).astype(np.float32)
    t = tie_values()
    at = g.randint(0, rows.size, min(rows.size // 3 + 1, 4 * len(t)))
    rows.reshape(-1)[at] = t[g.randint(0, len(t), len(at))]
    return rows


# ------------------------------------------------------------------------------------------------ the stage-2 models
MODEL_CASES = {'sgbasis, normal net': {}, 'sgbasis, geometric normals': {'train.normal_mlp': False},
               'microfacet, normal net': {'train.render_model': 'microfacet'},
               'microfacet, geometric normals': {'train.render_model': 'microfacet', 'train.normal_mlp': False}}


def make_models(case, seed=3):
    """(the product's PSNetwork, the oracle's PSNetwork with the same state_dict), both on the CPU."""
    import psnerf_amd.stage2 as s2
    from oracle import stage2 as o2
    torch.manual_seed(seed)
    onet = o2.PSNetwork(o2.bear_conf(**MODEL_CASES[case]))
    net = s2.PSNetwork(s2.bear_conf(**MODEL_CASES[case]))
    net.load_state_dict(onet.state_dict())
    return net, onet


def view(H, W, fx=30.0, distance=4.0):
    """A camera on the +z axis looking at the origin (the dataset's OpenCV pose) -> (camera_mat [1, 4, 4], world_mat [1, 4, 4])."""
    K = torch.eye(4, dtype=torch.float64)
    K[0, 0] = K[1, 1] = fx
    K[0, 2], K[1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    c2w = torch.eye(4, dtype=torch.float64)
    c2w[1, 1] = c2w[2, 2] = -1.0
    c2w[2, 3] = distance
    return K[None], c2w[None]
