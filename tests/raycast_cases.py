"""Shared constructions of the ray-casting tests (tests/test_raycast_cpu.py, tests/test_raycast_gpu.py): meshes, among them the ones
built to sit badly in the triangle grid, and seeded ray sets, among them the ones built to run along the grid's planes, edges and
corners.  Everything is numpy float64 and deterministic."""
import numpy as np

from tests import mesh_fields as mf

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ meshes
def icosphere(level):
    """A subdivided icosahedron, vertices normalised to radius 1: 20 x 4^level faces, closed, oriented outward, convex, around 0."""
    def make():
        p = (1.0 + 5.0 ** 0.5) / 2.0
        v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p), (p, 0, -1), (p, 0, 1),
             (-p, 0, -1), (-p, 0, 1)]
        f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
        v = [np.asarray(x, dtype=np.float64) / np.linalg.norm(x) for x in v]
        for _ in range(level):
            mid, nf = {}, []

            def midpoint(i, j):
                key = (min(i, j), max(i, j))
                if key not in mid:
                    m = v[i] + v[j]
                    v.append(m / np.linalg.norm(m))
                    mid[key] = len(v) - 1
                return mid[key]
            for a, b, c in f:
                ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
                nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
            f = nf
        v, f = np.stack(v), np.asarray(f, dtype=np.int64)
        assert len(f) == 20 * 4 ** level and mf.is_closed_oriented(f)
        return v, f
    return _cached(('icosphere', level), make)


def inner_radius(v, f):
    """The smallest distance from the origin to a face plane of a convex mesh around the origin."""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.cross(b - a, c - a)
    return float(np.abs((n * a).sum(1) / np.linalg.norm(n, axis=1)).min())


def _grid_square(origin, eu, ev, n):
    """The square origin + [0, n] eu + [0, n] ev as 2 n^2 triangles -> (vertices [(n + 1)^2, 3], faces)."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    v = origin + i.reshape(-1, 1) * eu + j.reshape(-1, 1) * ev
    q = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).ravel()
    f = np.concatenate([np.stack([q, q + n + 1, q + n + 2], 1), np.stack([q, q + n + 2, q + 1], 1)])
    return v, f


SNAP_CELL = 2.0 ** -8            # the cell MeshIndex must arrive at for snapped_cube: 0.75 / 192
SNAP_LO = -0.375
SNAP_FIRST = 93                  # the cube occupies the cells SNAP_FIRST .. SNAP_FIRST + n - 1 on every axis


def snapped_cube(n=6):
    """The surface of a cube of n cells per side, triangulated n x n per side, EVERY vertex exactly on a corner lo + k cell of the
    grid MeshIndex builds for the mesh (the caller asserts that from the index).  How the grid is pinned: MeshIndex takes cell =
    max(mean triangle edge, largest extent / 192).  Two small patches of fine triangles (edge cell / 8) in opposite corners of
    [-0.375, 0.375]^3 stretch the bounding box to 0.75 = 192 x 2^-8 per axis and pull the mean edge under one cell, so the second term
    governs and cell = 2^-8 exactly; all coordinates are multiples of 2^-11, exact in float64.
    -> (vertices, faces, number of cube vertices: the cube's come first)."""
    def make():
        c, e = SNAP_CELL, np.eye(3)
        base = SNAP_LO + SNAP_FIRST * c
        vs, fs, at = [], [], 0
        for axis in range(3):
            eu, ev = e[(axis + 1) % 3] * c, e[(axis + 2) % 3] * c
            for side in (0, 1):
                v, f = _grid_square(np.full(3, base) + side * n * c * e[axis], eu, ev, n)
                vs.append(v)
                fs.append(f + at)
                at += len(v)
        n_cube = at
        for corner, sign in ((np.full(3, SNAP_LO), 1.0), (np.full(3, -SNAP_LO), -1.0)):
            v, f = _grid_square(corner, sign * e[0] * c / 8, sign * e[1] * c / 8, 6)
            vs.append(v)
            fs.append(f + at)
            at += len(v)
        return np.concatenate(vs), np.concatenate(fs), n_cube
    return _cached(('snapped_cube', n), make)


def mc_mesh():
    """The marching-cubes mesh of the sphere + rod + torus field at resolution 32 in world units: 5 728 faces."""
    def make():
        from psnerf_amd.stage1.extracting import host_marching_cubes, to_world
        v, f = host_marching_cubes(mf.sphere_rod_torus(32), 0.0)
        assert len(f) == 5728
        return to_world(v, 33, mf.BOX_SIZE), f
    return _cached('mc', make)


def awkward_meshes():
    """name -> (vertices, faces): meshes that sit badly in the grid, on the icosphere(3) (1 280 faces)."""
    def make():
        v, f = icosphere(3)
        lo, hi = v.min(0), v.max(0)
        out = {}
        big = 10.0 * np.array([[lo[0], lo[1], lo[2]], [hi[0], lo[1], hi[2]], [lo[0], hi[1], hi[2]], [hi[0], hi[1], lo[2]]])
        out['two oversize triangles'] = (np.concatenate([v, big]), np.concatenate([f, len(v) + np.array([[0, 1, 2], [1, 3, 2]])]))
        g = np.random.RandomState(11)
        dup = f[g.choice(len(f), 60, replace=False)]
        zero = np.stack([dup[:, 0], dup[:, 1], dup[:, 1]], axis=1)                       # a repeated corner
        point = np.repeat(f[:30, :1], 3, axis=1)                                        # three equal corners
        mid = np.concatenate([v, 0.5 * (v[f[:40, 0]] + v[f[:40, 1]])])                  # a collinear triple: a, midpoint, b
        coll = np.stack([f[:40, 0], len(v) + np.arange(40), f[:40, 1]], axis=1)
        out['degenerate triangles'] = (mid, np.concatenate([zero, point, coll, f]))     # (the degenerate ones get the LOW ids)
        out['a single triangle'] = (np.array([[0.1, 0.2, 0.3], [1.3, 0.1, -0.2], [0.4, 1.5, 0.9]]), np.array([[0, 1, 2]]))
        flat = v.copy()
        flat[:, 2] = 0.25
        out['flat bounding box'] = (flat, f)
        return out
    return _cached('awkward', make)


# The leading faces of 'degenerate triangles' with a repeated corner.  For those the test's det is 0 in floating point too (two of
# the sheared corners are the same numbers, so U = 0 and V = -W exactly) and they can never be returned.  The 40 collinear triples
# behind them have a ROUNDED midpoint: slivers of area ~1e-17 that the definition may legitimately hit.
N_REPEATED = 60 + 30


# ------------------------------------------------------------------------------------------------ ray sets
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def ray_sets(v, f, lo, cell, n, count, seed=0, focus=None):
    """name -> (origins [Q, 3], directions [Q, 3], t_min, t_max), Q <= count, for the mesh (v, f) whose grid has the lower corner lo,
    the cell edge ``cell`` and n cells per axis (what MeshIndex reports; the grid-aligned sets run along ITS planes, edges and
    corners).  ``focus`` = (lower, upper corner) of the part of the mesh the rays are aimed at (default: its bounding box).
    Directions are not normalised unless the set says so."""
    g = np.random.RandomState(seed)
    lo, n = np.asarray(lo, dtype=np.float64), np.asarray(n)
    blo, bhi = (v.min(0), v.max(0)) if focus is None else (np.asarray(focus[0], dtype=np.float64), np.asarray(focus[1], dtype=np.float64))
    k_lo = np.clip(np.floor((blo - lo) / cell).astype(np.int64) - 1, 0, n)
    k_hi = np.clip(np.ceil((bhi - lo) / cell).astype(np.int64) + 1, 0, n)
    centre, diag = 0.5 * (blo + bhi), float(np.linalg.norm(bhi - blo))
    area = np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)
    solid = np.nonzero(area > 0)[0]
    inf = np.inf
    out = {}

    # camera-like bundles from outside: a few eyes, each with a fan of rays toward points of the box
    eyes = centre + 2.0 * diag * _unit(g.standard_normal((4, 3)))
    eye = eyes[g.randint(0, 4, count)]
    target = blo + g.random_sample((count, 3)) * (bhi - blo) * 1.3 - 0.15 * (bhi - blo)
    out['camera bundles'] = (eye, target - eye, 0.0, inf)

    inside = blo + g.random_sample((count, 3)) * (bhi - blo)
    out['origins in the box'] = (inside, g.standard_normal((count, 3)), 0.0, inf)

    # origins on the surface, offset along the normal
    pick = solid[g.randint(0, len(solid), count)]
    w = g.dirichlet(np.ones(3), count)
    a, b, c = v[f[pick, 0]], v[f[pick, 1]], v[f[pick, 2]]
    on = w[:, 0:1] * a + w[:, 1:2] * b + w[:, 2:3] * c
    nrm = _unit(np.cross(b - a, c - a))
    out['surface points, offset'] = (on + 1e-3 * diag * nrm * np.where(g.rand(count, 1) < 0.5, -1.0, 1.0), g.standard_normal((count, 3)), 0.0, inf)

    # axis-parallel rays from outside the box, through it
    axis = g.randint(0, 3, count)
    sign = np.where(g.rand(count) < 0.5, -1.0, 1.0)
    o = blo + g.random_sample((count, 3)) * (bhi - blo)
    d = np.zeros((count, 3))
    d[np.arange(count), axis] = sign * (0.5 + g.rand(count))
    o[np.arange(count), axis] = np.where(sign > 0, blo[axis] - 0.3 * diag, bhi[axis] + 0.3 * diag)
    out['axis-parallel'] = (o, d, 0.0, inf)

    # rays lying exactly in cell-boundary planes (one coordinate on the lattice, no motion along it)
    k = np.stack([g.randint(k_lo[i], k_hi[i] + 1, count) for i in range(3)], axis=1)
    lattice = lo + k * cell
    axis = g.randint(0, 3, count)
    o = blo + g.random_sample((count, 3)) * (bhi - blo)
    d = g.standard_normal((count, 3))
    o[np.arange(count), axis] = lattice[np.arange(count), axis]
    d[np.arange(count), axis] = 0.0
    axis_parallel = g.rand(count) < 0.3                       # some of them also parallel to a second axis
    second = (axis + 1 + g.randint(0, 2, count)) % 3
    d[axis_parallel, second[axis_parallel]] = 0.0
    out['in cell-boundary planes'] = (o - 0.7 * diag * _unit(d), d, 0.0, inf)

    # rays running along cell edges (two coordinates on the lattice)
    axis = g.randint(0, 3, count)
    o = lattice.copy()
    d = np.zeros((count, 3))
    d[np.arange(count), axis] = np.where(g.rand(count) < 0.5, -1.0, 1.0) * (0.25 + g.rand(count))
    o[np.arange(count), axis] = np.where(d[np.arange(count), axis] > 0, lo[axis] - 2.5 * cell, lo[axis] + (n[axis] + 2.5) * cell)
    out['along cell edges'] = (o, d, 0.0, inf)

    # rays through cell corners along a space diagonal: exact for a power-of-two cell, to rounding otherwise
    signs = np.where(g.rand(count, 3) < 0.5, -1.0, 1.0)
    steps = g.randint(1, 40, count)[:, None]
    out['through cell corners'] = (lattice - steps * cell * signs, signs * (0.5 + g.randint(0, 3, count)[:, None]), 0.0, inf)

    # rays aimed at vertices and at edge midpoints
    used = np.unique(f[solid])
    tv = v[used[g.randint(0, len(used), count // 2)]]
    e = f[solid[g.randint(0, len(solid), count - count // 2)]]
    side = g.randint(0, 3, len(e))
    tm = 0.5 * (v[e[np.arange(len(e)), side]] + v[e[np.arange(len(e)), (side + 1) % 3]])
    target = np.concatenate([tv, tm])
    o = centre + 1.5 * diag * _unit(g.standard_normal((count, 3)))
    out['at vertices and edge midpoints'] = (o, target - o, 0.0, inf)

    # rays that miss the box, touch a box face, or start beyond the mesh pointing away
    third = count // 3
    o1 = centre + 3.0 * diag * _unit(g.standard_normal((third, 3)))
    d1 = np.cross(o1 - centre, g.standard_normal((third, 3)))                    # tangential: far from the box
    o2 = blo + g.random_sample((third, 3)) * (bhi - blo)                         # in a face plane of the box, moving within it
    ax2 = g.randint(0, 3, third)
    o2[np.arange(third), ax2] = np.where(g.rand(third) < 0.5, blo[ax2], bhi[ax2])
    d2 = g.standard_normal((third, 3))
    d2[np.arange(third), ax2] = 0.0
    o2 = o2 - 0.8 * diag * _unit(d2)
    o3 = centre + 1.2 * diag * _unit(g.standard_normal((count - 2 * third, 3)))
    d3 = (o3 - centre) * (0.5 + g.rand(len(o3), 1))
    out['missing, touching, pointing away'] = (np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, d3]), 0.0, inf)

    # directions with one and with two zero components, origins anywhere around
    o = centre + (g.random_sample((count, 3)) - 0.5) * 1.6 * (bhi - blo + 0.1 * diag)
    d = g.standard_normal((count, 3))
    d[np.arange(count), g.randint(0, 3, count)] = 0.0
    two = g.rand(count) < 0.5
    keep = g.randint(0, 3, count)
    for i in range(3):
        d[two & (keep != i), i] = 0.0
    d[two, keep[two]] = np.where(g.rand(int(two.sum())) < 0.5, -1.5, 0.75)
    out['zero components'] = (o, d, 0.0, inf)

    # rays with a NaN, an infinity or a zero direction, between healthy ones
    m = min(count, 256)
    o, d = inside[:m].copy(), g.standard_normal((m, 3))
    o[0::8, 1] = np.nan
    d[1::8, 2] = np.nan
    d[2::8] = 0.0
    d[3::8, 0] = np.inf
    o[4::8, 2] = -np.inf
    out['NaN, infinite and zero rays'] = (o, d, 0.0, inf)

    # windows on t that cut off the first hit: the window opens behind it
    o = centre + 1.5 * diag * _unit(g.standard_normal((count, 3)))
    target = blo + (0.2 + 0.6 * g.random_sample((count, 3))) * (bhi - blo)
    out['window behind the first hit'] = (o, _unit(target - o), 1.5 * diag, 1.5 * diag + 0.6 * diag)
    out['window that ends early'] = (o, _unit(target - o), -inf, 1.5 * diag)
    return out
