"""Shared inputs of the registration tests (tests/test_align_cpu.py, tests/test_align_gpu.py): the deformed icosphere, the known
transforms, the error measures and host-made row sets.  Everything is numpy float64 and deterministic."""
import numpy as np

from tests import raycast_cases as rc

_CACHE = {}

# (rotation in degrees about AXIS, translation as a fraction of the target's diagonal along SHIFT, scale): the starts of the issue's table
STARTS = ((5.0, 0.02, 1.0), (8.0, 0.03, 1.04), (15.0, 0.05, 1.08))
AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
SHIFT = np.array([0.6, 0.64, -0.48])


def deformed_icosphere(level):
    """The icosphere of ``level`` deformed to have no symmetry: v (1 + 0.25 x + 0.15 y^2 - 0.2 x z + 0.1 z) (1, 0.8, 0.65) ->
    (vertices, faces), read-only; level 2 has 162 vertices and 320 faces."""
    if level not in _CACHE:
        v, f = rc.icosphere(level)
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        w = (v * (1.0 + 0.25 * x + 0.15 * y * y - 0.2 * x * z + 0.1 * z)[:, None]) * np.array([1.0, 0.8, 0.65])
        w, f = np.ascontiguousarray(w), np.array(f, dtype=np.int64)
        w.setflags(write=False)
        f.setflags(write=False)
        _CACHE[level] = (w, f)
    return _CACHE[level]


def diagonal(v):
    return float(np.sqrt(((v.max(axis=0) - v.min(axis=0)) ** 2).sum()))


def rotation(axis, degrees):
    """Rodrigues' formula, written out here so that the tests do not lean on the module under test."""
    k = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    a = np.radians(degrees)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def known(start, diag, axis=AXIS):
    """The 4 x 4 matrix of a start of the table: x -> s R x + t with |t| = fraction x diag."""
    degrees, fraction, scale = start
    m = np.eye(4)
    m[:3, :3] = scale * rotation(axis, degrees)
    m[:3, 3] = fraction * diag * SHIFT / np.linalg.norm(SHIFT)
    return m


def move(matrix, v):
    return np.ascontiguousarray(v @ matrix[:3, :3].T + matrix[:3, 3])


def errors(found, moved_by, diag):
    """The error of ``found`` (the registration's 4 x 4) as the inverse of ``moved_by``: E = found . moved_by should be the identity ->
    (rotation error in degrees, translation error / diag, scale error).  The angle is asin(|E_R - E_R^T|_F / (2 sqrt 2)), which resolves
    angles far below the 1e-8 rad at which arccos((trace - 1) / 2) goes blind."""
    E = np.asarray(found) @ np.asarray(moved_by)
    s = np.linalg.det(E[:3, :3]) ** (1.0 / 3.0)
    R = E[:3, :3] / s
    sine = np.linalg.norm(R - R.T) / (2.0 * np.sqrt(2.0))
    angle = np.degrees(np.arcsin(min(1.0, sine))) if np.trace(R) > 1.0 else 180.0 - np.degrees(np.arcsin(min(1.0, sine)))
    return float(angle), float(np.linalg.norm(E[:3, 3]) / diag), float(abs(s - 1.0))


def without_a_third(v, f):
    """The mesh without the third of its faces whose centroids lie lowest along (1, 1, 1): a partial scan -> (vertices, faces)."""
    c = v[f].mean(axis=1) @ np.ones(3)
    keep = np.argsort(c, kind='stable')[len(f) // 3:]
    return v, np.ascontiguousarray(f[np.sort(keep)])


def row_set(n, seed, level=1, special=False):
    """Host-made rows for the teacher-forced sums tests: P = points near the level-``level`` deformed icosphere, Y and tri = their
    closest points on it -> dict(P, Y, tri, vertices, faces).  ``special``: the mesh gains a zero-area triangle, and rows are planted
    (when n allows) with tri = -1, tri = F (beyond the last), a NaN coordinate in P, an infinite one in Y and the zero-area triangle."""
    from psnerf_amd import meshdist
    v, f = deformed_icosphere(level)
    v, f = np.array(v), np.array(f)
    rng = np.random.RandomState(seed)
    pts, _ = meshdist.host_sample_surface(v, f, n, rng)
    P = pts + 0.05 * rng.standard_normal((n, 3))
    Y, _, tri = meshdist.host_closest_point(v, f, P)
    planted = {}
    if special:
        f = np.concatenate([f, [[3, 3, 7]]])                    # zero area: a repeated corner
        spots = {'no_triangle': 0, 'beyond_last': 1, 'nan_P': 2, 'inf_Y': 3, 'zero_area': 4}
        for name, i in spots.items():
            if i >= n:
                continue
            planted[name] = i
            if name == 'no_triangle':
                tri[i] = -1
            elif name == 'beyond_last':
                tri[i] = len(f)
            elif name == 'nan_P':
                P[i, 1] = np.nan
            elif name == 'inf_Y':
                Y[i, 2] = np.inf
            else:
                tri[i] = len(f) - 1
    return {'P': np.ascontiguousarray(P), 'Y': np.ascontiguousarray(Y), 'tri': tri.astype(np.int64), 'vertices': v, 'faces': f,
            'planted': planted}
