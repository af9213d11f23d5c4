"""Shared constructions of the occlusion tests (tests/test_occlusion_cpu.py, tests/test_occlusion_gpu.py): rows on the meshes of
tests/raycast_cases.py, direction tables, and the cases the device is held to with the definition's answer computed once and handed
out read-only.  Everything is numpy float64 and deterministic.

Cost.  The definition is a brute force over rows x K x faces ray-triangle pairs; every case stays below about 1e8 of them (the
largest: 65 rows x 65 directions x 5 728 faces = 2.4e7), so a test takes seconds."""
import functools

import numpy as np

from tests import raycast_cases as rc
from psnerf_amd import meshdist as md
from psnerf_amd import meshocclude as mo


def unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def geometric_normals(v, f, face):
    a = v[f[face, 0]]
    return unit(np.cross(v[f[face, 1]] - a, v[f[face, 2]] - a))


def surface_rows(v, f, count, seed, faces=None, on_edges=False, face=None):
    """``count`` points on the faces ``faces`` (default: those with an area) with the faces' geometric normals, ordered by face as
    the rows of an atlas are -> (points [count, 3], normals [count, 3], face [count]).  ``on_edges``: every fourth point lies on an
    edge and every eighth on a corner of its face.  ``face`` [count]: the face of every row, given instead of drawn."""
    g = np.random.RandomState(seed)
    if faces is None:
        area = np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
        faces = np.nonzero(area > 0)[0]
    face = np.sort(np.asarray(faces)[g.randint(0, len(faces), count)]) if face is None else np.asarray(face)
    u, w = g.random_sample(count), g.random_sample(count)
    flip = u + w > 1.0
    u, w = np.where(flip, 1.0 - u, u), np.where(flip, 1.0 - w, w)
    if on_edges:
        w[::4] = 0.0
        u[::8] = 0.0
    a, b, c = v[f[face, 0]], v[f[face, 1]], v[f[face, 2]]
    return a + u[:, None] * (b - a) + w[:, None] * (c - a), geometric_normals(v, f, face), face


def world_table(K, seed, axes=False):
    """K unit directions all around the sphere (a world-frame table: light directions); ``axes``: the six axis directions among them,
    which are exactly perpendicular to the normals of an axis-aligned face."""
    d = unit(np.random.RandomState(seed).standard_normal((K, 3)))
    if axes:
        six = np.concatenate([np.eye(3), -np.eye(3)])
        d[:min(K, 6)] = six[:min(K, 6)]
    return d


def degenerate_rows(p, n):
    """Rows that cast nothing, written over copies of (p, n) at rows 3, 7, 11, 15, 19 (as far as they exist) -> (p, n, bool [R])."""
    p, n = p.copy(), n.copy()
    dead = np.zeros(len(p), dtype=bool)
    for row, (what, value) in zip(range(3, len(p), 4), (('n', 0.0), ('n', np.nan), ('n', np.inf), ('p', np.nan), ('p', -np.inf))):
        if what == 'n' and value == 0.0:
            n[row] = 0.0
        elif what == 'n':
            n[row, row % 3] = value
        else:
            p[row, row % 3] = value
        dead[row] = True
    return p, n, dead


def corner_mesh():
    """A floor z = 0 and a wall x = 0, each a square of 100 units of two triangles, meeting in the line x = z = 0."""
    v = np.array([[-50.0, -50.0, 0.0], [50.0, -50.0, 0.0], [50.0, 50.0, 0.0], [-50.0, 50.0, 0.0],
                  [0.0, -50.0, 0.0], [0.0, 50.0, 0.0], [0.0, 50.0, 100.0], [0.0, -50.0, 100.0]])
    return v, np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the device's cases
# name -> (mesh, rows R, directions K, local, bias (None: the default), t_max).  Between them: K in {1, 31, 32, 33, 64, 65, 1024},
# R in {1, 63, 64, 65, 257}, both modes, bias 0 / > 0 / default, a finite t_max, every mesh.
CASES = {
    'icosphere, R 257, K 64': ('icosphere(2)', 257, 64, True, None, np.inf),
    'icosphere, R 64, K 1024, no bias': ('icosphere(2)', 64, 1024, True, 0.0, np.inf),
    'icosphere, one row, one direction': ('icosphere(2)', 1, 1, True, 1e-3, np.inf),
    'icosphere, one row, world': ('icosphere(2)', 1, 1, False, 1e-3, np.inf),
    'icosphere inward, R 65, K 33, short rays': ('icosphere(2) inward', 65, 33, True, None, 0.05),
    'icosphere inward, R 63, K 32, world': ('icosphere(2) inward', 63, 32, False, 1e-3, 0.8),
    'snapped cube, R 257, K 32, no bias': ('snapped cube', 257, 32, True, 0.0, np.inf),
    'snapped cube, R 64, K 65, world': ('snapped cube', 64, 65, False, 2.0 ** -20, np.inf),
    'marching cubes, R 65, K 65': ('marching cubes', 65, 65, True, None, np.inf),
    'marching cubes, R 63, K 31, world': ('marching cubes', 63, 31, False, None, 1.5),
    'two oversize triangles, R 64, K 31': ('two oversize triangles', 64, 31, True, None, np.inf),
    'degenerate triangles, R 65, K 33, world': ('degenerate triangles', 65, 33, False, 0.0, np.inf),
    'every face oversize, R 63, K 64': ('icosphere(1), every face oversize', 63, 64, True, None, np.inf),
}
ALL_OVERSIZE_CELL = 0.05          # the grid of the last case: cells of this edge with max_span = 1, so that every face is oversize


def case_mesh(mesh):
    if mesh.startswith('icosphere(2)'):
        return rc.icosphere(2)
    if mesh.startswith('icosphere(1)'):
        return rc.icosphere(1)
    if mesh == 'snapped cube':
        return rc.snapped_cube(6)[:2]
    if mesh == 'marching cubes':
        return rc.mc_mesh()
    return rc.awkward_meshes()[mesh]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: v, f, points, normals, table, local, bias (a float), t_max, dead (the rows that cast nothing) and ``want`` = the
    definition's (hits, visible, ao, bent, words); all read-only."""
    mesh, R, K, local, bias, t_max = CASES[name]
    v, f = case_mesh(mesh)
    seed = len(name)
    if mesh == 'snapped cube':                                   # rows ON the cube's faces, whose vertices sit on the grid's corners
        p, n, _ = surface_rows(v, f, R, seed, faces=np.arange(6 * 2 * 36), on_edges=True)
    else:
        p, n, _ = surface_rows(v, f, R, seed)
    if mesh.endswith('inward'):
        n = -n
    if R >= 63:
        if mesh.startswith('icosphere'):                         # rows outside the grid's box, looking away from it and back at it
            p[5], n[5] = 3.0 * p[5], unit(p[5])
            p[9], n[9] = 3.0 * p[9], -unit(p[9])
        p, n, dead = degenerate_rows(p, n)
    else:
        dead = np.zeros(R, dtype=bool)
    table = mo.hemisphere_table(K) if local else world_table(K, seed, axes=mesh == 'snapped cube')
    if bias is None:
        bias = mo.default_bias(md._HostMesh(v, f))
    want = mo.host_occlusion_rows(v, f, p, n, table, local, bias, t_max, bits=True)
    out = dict(v=v, f=f, points=p, normals=n, table=table, local=local, bias=float(bias), t_max=float(t_max), dead=dead, want=want)
    for x in (p, n, table, dead) + tuple(want):
        x.setflags(write=False)
    return out


def rays_of(c):
    """The rays of a case as the definition forms them, row by row and direction by direction -> (origins [R K, 3], directions
    [R K, 3], cast bool [R, K]); rows that cast nothing have no cast direction."""
    p, n, table = c['points'], c['normals'], c['table']
    with np.errstate(all='ignore'):
        o = p + c['bias'] * n
        if c['local']:
            t, b = mo.frame(n)
            d = (table[None, :, 0, None] * t[:, None, :] + table[None, :, 1, None] * b[:, None, :]) + table[None, :, 2, None] * n[:, None, :]
            cast = np.ones((len(p), len(table)), dtype=bool)
        else:
            d = np.broadcast_to(table[None], (len(p), len(table), 3))
            cast = (n[:, None, 0] * d[..., 0] + n[:, None, 1] * d[..., 1]) + n[:, None, 2] * d[..., 2] > 0.0
    cast = cast & ~c['dead'][:, None]
    o = np.broadcast_to(o[:, None, :], d.shape)
    return np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(d.reshape(-1, 3)), cast
