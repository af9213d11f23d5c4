"""The meshes of tests/test_meshtopo_*.py and tests/test_meshsmooth_*.py, built once per process and read-only: the smallest
constructed meshes that reach every branch of the edge table, the rings, the corner runs and the smoothing step, with what each must
report, and three of tests/meshclean_cases.py with the values computed on the CPU with the definition.  KNOWN holds, per case, the
report entries that are known by construction."""
import functools

import numpy as np

TET_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
TET_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)


def _grid_faces(n, m, wrap):
    """Two triangles per cell of an n x m grid of cells; vertex (i, j) = i * cols + j; ``wrap``: both directions closed (a torus)."""
    rows, cols = (n, m) if wrap else (n + 1, m + 1)
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing='ij')
    i, j = i.reshape(-1), j.reshape(-1)
    a, b = i * cols + j, i * cols + (j + 1) % cols
    c, d = ((i + 1) % rows) * cols + j, ((i + 1) % rows) * cols + (j + 1) % cols
    return np.concatenate([np.stack([a, d, b], axis=1), np.stack([a, c, d], axis=1)]).astype(np.int64)


def torus(n, m):
    u, w = np.meshgrid(2 * np.pi * np.arange(n) / n, 2 * np.pi * np.arange(m) / m, indexing='ij')
    r = 2.0 + np.cos(w)
    return np.stack([r * np.cos(u), r * np.sin(u), np.sin(w)], axis=-1).reshape(-1, 3), _grid_faces(n, m, True)


def patch(n, m):
    """An open planar patch of n x m cells with integer coordinates, cut like the lattice of equilateral triangles sheared to a square
    grid: every interior vertex has the six neighbours (+-1, 0), (0, +-1), (1, 1), (-1, -1), which sum to six times the vertex."""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(m + 1), indexing='ij')
    v = np.stack([i, j, np.zeros_like(i)], axis=-1).reshape(-1, 3).astype(np.float64)
    return v, _grid_faces(n, m, False)


def moebius(n):
    """A strip of n cells whose ends are glued with a half turn: one side, one rim."""
    t = 2 * np.pi * np.arange(n) / n
    ring = lambda s: np.stack([(2 + s * np.cos(t / 2)) * np.cos(t), (2 + s * np.cos(t / 2)) * np.sin(t), s * np.sin(t / 2)], axis=1)
    v = np.concatenate([ring(-0.5), ring(0.5)])
    faces = []
    for i in range(n):
        a, b = i, n + i
        c, d = (i + 1, n + i + 1) if i + 1 < n else (n, 0)        # the last cell meets the first one upside down
        faces += [[a, c, d], [a, d, b]]
    return v, np.array(faces, dtype=np.int64)


def fan(n):
    """n triangles about vertex 0: its ring has n + 1 neighbours and its corner run n entries."""
    t = 2 * np.pi * np.arange(n + 1) / (n + 7)
    v = np.concatenate([np.array([[0.0, 0.0, 0.25]]), np.stack([np.cos(t), np.sin(t), 0.1 * np.sin(5 * t)], axis=1)])
    k = np.arange(n)
    return v, np.stack([np.zeros(n, dtype=np.int64), 1 + k, 2 + k], axis=1).astype(np.int64)


def _with_oddities(v, f, seed):
    """A degenerate face, a duplicated face, a face with zero area and two unreferenced vertices on top of a mesh; coordinates with a
    -0.0 and a denormal among them."""
    g = np.random.RandomState(seed)
    extra = np.array([[-0.0, 5e-324, 1.0], [3.0, -0.0, 2.5e-310]])
    n = len(v)
    v = np.concatenate([v, extra, v[:1]])                       # (the last one coincides with vertex 0: a zero-area face below)
    f = np.concatenate([f, [[1, 1, 2]], f[3:4], [[0, n + 2, 0]], [[0, 1, n + 2]]]).astype(np.int64)
    return v, f[g.permutation(len(f))]


BUILDERS = {
    'empty': lambda: (np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)),
    'points': lambda: (np.random.RandomState(0).rand(5, 3), np.zeros((0, 3), dtype=np.int64)),
    'triangle': lambda: (np.random.RandomState(1).rand(5, 3), np.array([[4, 2, 3]], dtype=np.int64)),
    'tet': lambda: (TET_V, TET_F),
    'tet_flipped': lambda: (TET_V, np.concatenate([TET_F[:3], TET_F[3:, ::-1]])),
    'tet_doubled': lambda: (TET_V, np.concatenate([TET_F, TET_F[:1]])),
    'three_on_an_edge': lambda: (np.random.RandomState(2).rand(5, 3), np.array([[0, 1, 2], [0, 1, 3], [1, 0, 4]], dtype=np.int64)),
    'torus': lambda: torus(7, 5),
    'patch': lambda: patch(6, 4),
    'moebius': lambda: moebius(9),
    'fan300': lambda: fan(300),
    'torus_wide': lambda: torus(37, 7),                          # 259 vertices: just over one workgroup's worth
    'oddities': lambda: _with_oddities(*torus(6, 5), seed=3),
}

# what is known by construction (report keys)
KNOWN = {
    'empty': dict(n_edges=0, euler=0, is_watertight=False, is_oriented=False, n_vertices_unreferenced=0),
    'points': dict(n_edges=0, euler=0, is_watertight=False, n_vertices_unreferenced=5),
    'triangle': dict(n_edges=3, n_boundary_edges=3, euler=1, is_watertight=False, n_vertices_unreferenced=2),
    'tet': dict(n_edges=6, euler=2, is_watertight=True, is_oriented=True, n_boundary_edges=0, n_nonmanifold_edges=0, n_inconsistent_edges=0),
    'tet_flipped': dict(n_edges=6, euler=2, is_watertight=True, is_oriented=False, n_inconsistent_edges=3),
    'tet_doubled': dict(n_edges=6, n_nonmanifold_edges=3, is_watertight=False, is_oriented=False),
    'three_on_an_edge': dict(n_edges=7, n_nonmanifold_edges=1, n_boundary_edges=6, is_watertight=False),
    'torus': dict(n_edges=105, euler=0, is_watertight=True, is_oriented=True),
    'patch': dict(n_boundary_edges=2 * (6 + 4), euler=1, is_watertight=False, n_nonmanifold_edges=0, n_inconsistent_edges=0),
    'moebius': dict(is_watertight=False, is_oriented=False, euler=0, n_edges=36, n_boundary_edges=18, n_nonmanifold_edges=0),
    'fan300': dict(n_edges=601, n_boundary_edges=302, euler=1, is_watertight=False),
    'torus_wide': dict(n_vertices=259, euler=0, is_watertight=True, is_oriented=True),
    'oddities': dict(n_faces_degenerate=2, n_vertices_unreferenced=2, is_watertight=False),
}

# tests/meshclean_cases.py, computed on the CPU with the definition: E, boundary, non-manifold, inconsistent, degenerate, euler
MEASURED = {
    'ribbon': (8204, 4104, 2, 4098, 1, 3),
    'sphere_rod_torus': (34224, 0, 0, 0, 0, 2),
    'checker16': (24798, 0, 0, 0, 0, -458),
    'checker16_shuffled': (24798, 0, 0, 0, 0, -458),
}
MEASURED_KEYS = ('n_edges', 'n_boundary_edges', 'n_nonmanifold_edges', 'n_inconsistent_edges', 'n_faces_degenerate', 'euler')

OUT_OF_RANGE = (TET_V, np.array([[0, 2, 1], [0, 1, 4], [0, 3, 2], [-1, 2, 3]], dtype=np.int64))
NAMES = sorted(BUILDERS) + sorted(MEASURED)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in MEASURED:
        from tests.meshclean_cases import case as clean_case
        return clean_case(name)
    v, f = BUILDERS[name]()
    v, f = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3), np.ascontiguousarray(f, dtype=np.int64).reshape(-1, 3)
    v.flags.writeable = f.flags.writeable = False
    return v, f


@functools.lru_cache(maxsize=None)
def host(name):
    """Everything the definition gives for a case, computed once: (edge table, (ring_start, ring), (corner_start, corner), report)."""
    from psnerf_amd import meshtopo as mt
    v, f = case(name)
    table = mt.host_edges(f, len(v))
    return table, mt.host_rings(table['edges'], len(v)), mt.host_corner_runs(f, len(v)), mt.host_report(v, f, table)
