"""The meshes of tests/test_simplify_*.py, built once per process and read-only: the smallest set that still reaches every way the
clustering, the quadric solve and the duplicate pass can go wrong.  RUNS lists (case, size argument) as both test files walk them."""
import functools

import numpy as np


def _grid_sheet(n, origin, du, dv):
    """(n + 1)^2 points origin + i du + j dv (i-major) and the 2 n^2 triangles of the n x n quads, normal du x dv."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    p = np.asarray(origin, dtype=np.float64)[None, :] + i.reshape(-1, 1) * np.asarray(du, dtype=np.float64)[None, :] \
        + j.reshape(-1, 1) * np.asarray(dv, dtype=np.float64)[None, :]
    q = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    a, b, c, d = q, q + (n + 1), q + (n + 1) + 1, q + 1
    return p, np.concatenate([np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)]).astype(np.int64)


def _weld(v, f):
    """Merge vertices with equal coordinates (they are formed from small integers times one step: equal points have equal bits)."""
    _, first, inverse = np.unique(np.round(v * 4096.0).astype(np.int64), axis=0, return_index=True, return_inverse=True)
    return v[first], inverse.reshape(-1)[f]


def cube(n=16):
    """The surface of [-1, 1]^3, n x n quads per side, shared vertices, outward normals: 6 n^2 + 2 vertices, 12 n^2 faces."""
    s = 2.0 / n
    sides = []
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for sign in (-1.0, 1.0):
            origin = np.full(3, -1.0)
            origin[axis] = sign
            du, dv = np.zeros(3), np.zeros(3)
            du[u], dv[w] = s, s
            if sign < 0:
                du, dv = dv, du
            sides.append(_grid_sheet(n, origin, du, dv))
    v = np.concatenate([p for p, _ in sides])
    f = np.concatenate([t + k * (n + 1) ** 2 for k, (_, t) in enumerate(sides)])
    return _weld(v, f)


def rotation(seed=3):
    q, r = np.linalg.qr(np.random.RandomState(seed).randn(3, 3))
    q = q * np.sign(np.diag(r))[None, :]
    return q if np.linalg.det(q) > 0 else q[:, ::-1]


def messy_cube():
    """cube16 with its vertex ids and face order shuffled, three duplicated faces, a face with a repeated index and four unreferenced
    vertices (inside the cube): "first in face order" and "ascending by key" are not the order of appearance."""
    v, f = cube(16)
    g = np.random.RandomState(11)
    extra = g.rand(4, 3) - 0.5
    v = np.concatenate([v, extra])
    new_id = g.permutation(len(v))
    out_v = np.empty_like(v)
    out_v[new_id] = v
    f = new_id[f]
    f = np.concatenate([f, f[[5, 700, 2001]], np.array([[f[9, 0], f[9, 0], f[9, 1]]])])
    return out_v, f[g.permutation(len(f))]


SLAB_H = 0.25


def slab():
    """Two thin closed slabs stacked: each is two 8 x 8 sheets over [0, 2]^2, 0.01 SLAB_H apart and joined at the rim, the second slab
    0.03 SLAB_H above the first.  At cell edge SLAB_H all four sheets fall into the same layer of cells: every top face has a bottom
    face over the same clusters in the OPPOSITE orientation (both stay), the second slab's faces are exact duplicates of the first's
    (they go), and the rim faces are degenerate.  (One slab alone has no exact duplicates: on a regular sheet no two faces of one
    orientation share their three cells.)"""
    n, gap = 8, 0.01 * SLAB_H
    m = (n + 1) ** 2
    ring = [(i, 0) for i in range(n)] + [(n, j) for j in range(n)] + [(i, n) for i in range(n, 0, -1)] + [(0, j) for j in range(n, 0, -1)]
    vs, fs = [], []
    for k, z in enumerate((0.0, 3.0 * gap)):
        top, tf = _grid_sheet(n, (0.0, 0.0, z + gap), (SLAB_H, 0, 0), (0, SLAB_H, 0))
        bottom, bf = _grid_sheet(n, (0.0, 0.0, z), (0, SLAB_H, 0), (SLAB_H, 0, 0))    # (j-major: point (i, j) at index j (n + 1) + i)
        rim = []
        for (i0, j0), (i1, j1) in zip(ring, ring[1:] + ring[:1]):
            t0, t1 = i0 * (n + 1) + j0, i1 * (n + 1) + j1
            b0, b1 = m + j0 * (n + 1) + i0, m + j1 * (n + 1) + i1
            rim += [[t0, b0, b1], [t0, b1, t1]]
        vs += [top, bottom]
        fs.append(np.concatenate([tf, bf + m, np.asarray(rim, dtype=np.int64)]) + 2 * m * k)
    return np.concatenate(vs), np.concatenate(fs)


def sphere(n_lat=100, n_lon=100):
    """A UV sphere of radius 1: 2 n_lon (n_lat - 1) faces (19 800)."""
    theta = np.pi * np.arange(1, n_lat) / n_lat
    phi = 2.0 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(theta), np.cos(phi)), np.outer(np.sin(theta), np.sin(phi)), np.outer(np.cos(theta), np.ones(n_lon))], axis=2)
    v = np.concatenate([[[0.0, 0.0, 1.0]], ring.reshape(-1, 3), [[0.0, 0.0, -1.0]]])
    at = lambda i, j: 1 + i * n_lon + (j % n_lon)
    f = []
    for j in range(n_lon):
        f.append([0, at(0, j), at(0, j + 1)])
        f.append([len(v) - 1, at(n_lat - 2, j + 1), at(n_lat - 2, j)])
    i, j = np.meshgrid(np.arange(n_lat - 2), np.arange(n_lon), indexing='ij')
    a, b, c, d = at(i, j).reshape(-1), at(i + 1, j).reshape(-1), at(i + 1, j + 1).reshape(-1), at(i, j + 1).reshape(-1)
    return v, np.concatenate([np.asarray(f, dtype=np.int64), np.stack([a, b, c], axis=1), np.stack([a, c, d], axis=1)])


@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'empty':
        v, f = np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    elif name == 'five_points':
        v, f = np.random.RandomState(0).rand(5, 3), np.zeros((0, 3), dtype=np.int64)
    elif name == 'one_triangle':
        v, f = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.5]]), np.array([[0, 1, 2]])
    elif name == 'cube16':
        v, f = cube(16)
    elif name == 'cube16_rotated':
        v, f = cube(16)
        v = v @ rotation().T
    elif name == 'cube16_messy':
        v, f = messy_cube()
    elif name == 'slab':
        v, f = slab()
    elif name == 'sphere':
        v, f = sphere()
    else:
        raise KeyError(name)
    v, f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
    v.flags.writeable = f.flags.writeable = False
    return v, f


ROTATED_RESOLUTIONS = (2, 3, 4, 5, 9, 17, 34)
# (case, size argument): one triangle in one cell (nothing survives) and across three cells; the cube coarse (corner runs of over a
# thousand entries per cluster), at the corner gate's two resolutions and with almost no merging; rotated, so that clamping happens;
# shuffled with duplicates; the slab collapsed
RUNS = [('five_points', dict(resolution=2)), ('one_triangle', dict(cell=4.0)), ('one_triangle', dict(resolution=2)),
        ('cube16', dict(resolution=2)), ('cube16', dict(resolution=4)), ('cube16', dict(resolution=5)), ('cube16', dict(resolution=34))] + \
       [('cube16_rotated', dict(resolution=n)) for n in ROTATED_RESOLUTIONS] + \
       [('cube16_messy', dict(resolution=4)), ('cube16_messy', dict(resolution=5)), ('cube16_messy', dict(resolution=34)),
        ('cube16_messy', dict(cell=0.3)),
        ('slab', dict(cell=SLAB_H)), ('sphere', dict(resolution=12))]


def run_id(run):
    return '%s-%s' % (run[0], '-'.join('%s%g' % (k[0], v) for k, v in sorted(run[1].items())))


@functools.lru_cache(maxsize=None)
def host_result(index):
    """host_simplify of RUNS[index], computed once and shared."""
    from psnerf_amd import meshsimplify as ms
    name, kw = RUNS[index]
    v, f = case(name)
    out_v, out_f, report = ms.host_simplify(v, f, **kw)
    out_v.flags.writeable = out_f.flags.writeable = False
    return out_v, out_f, report
