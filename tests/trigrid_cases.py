"""Shared constructions of the triangle-grid tests (tests/test_trigrid_cpu.py, tests/test_trigrid_gpu.py): meshes with the grid
each is indexed in, built to exercise the index itself -- a triangle's cell range on and off cell boundaries, the oversize threshold
from both sides, the per-wave compaction of the oversize list lane by lane, grids of one cell and of one layer, a cell that is no
power of two, a grid that stops short of the bounding box -- and the default grids of meshes the suite already has.

A case is (vertices, faces, the grid's arguments, max_span).  ``case(name)`` builds it once; the arrays are read-only.  Where the
mesh is constructed in integer cell units the case carries that construction (c0, c1, span per triangle), which was never passed
through a floor.  CASES pins what psnerf_amd.meshdist.host_tri_grid counted on each.  Everything is numpy float64 and deterministic."""
import numpy as np

from tests import raycast_cases as rc
from psnerf_amd import meshdist as md

# name -> (faces, n, n_over, n_entries, occupied cells): what the host definition counted
CASES = {
    'lattice soup': (703, [16, 16, 16], 313, 2574, 1888),
    'oversize by lane': (650, [16, 16, 16], 70, 1016, 896),
    'oversize by lane, none oversize': (650, [16, 16, 16], 0, 5751, 4096),
    'one triangle': (1, [3, 3, 3], 0, 27, 27),
    'one triangle, oversize': (1, [3, 3, 3], 1, 0, 0),
    'flat box': (1280, [17, 17, 1], 0, 4746, 257),
    'mesh in one point': (4, [1, 1, 1], 0, 4, 1),
    'cell 0.1': (240, [13, 13, 13], 2, 3099, 1419),
    'truncated grid': (320, [192, 192, 192], 46, 221858, 91000),
    'snapped cube': (576, [192, 192, 192], 0, 1872, 220),
    'marching cubes': (5728, [30, 20, 28], 0, 27478, 3985),
    'two oversize triangles': (1282, [103, 103, 103], 2, 5144, 665),
    'degenerate triangles': (1410, [14, 14, 14], 0, 7074, 1144),
}
EXPLICIT_CELL = ['lattice soup', 'oversize by lane', 'oversize by lane, none oversize', 'one triangle', 'one triangle, oversize',
                 'mesh in one point', 'cell 0.1', 'truncated grid', 'snapped cube']   # the cell does not depend on a rounded mean edge
QUERY_CASES = ['lattice soup', 'oversize by lane', 'truncated grid']

SOUP_CELL = 2.0 ** -4
SOUP_LO = -0.5
SOUP_N = 16
SOUP_MAX_SPAN = 8
SOUP_SHAPES = [(2, 2, 2), (3, 3, 1), (1, 1, 8), (1, 1, 9), (1, 1, 1), (2, 4, 1), (3, 1, 3), (8, 1, 1), (9, 1, 1)]
LANE_FACES = 650
LANE_OVERSIZE = [0, 63] + list(range(64, 128)) + [192 + 31, 192 + 32, 256, LANE_FACES - 1]
TRUNCATED_MAX_SPAN = 4096

_CACHE = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------------ boxes in integer cell units
def _quarter_box(first, shape, snap_lo, snap_hi):
    """A bounding box that covers exactly the cells first .. first + shape - 1 per axis of the 16^3 grid, in QUARTERS of a cell from
    lo -> (q0 [3], q1 [3]).  An interior corner lies at k + 0.25 (lower) or k + 0.75 (upper); a snapped lower corner lies on the
    grid corner k and belongs to cell k; a snapped upper corner lies on the lower boundary of the last cell (it belongs to the upper
    cell), or at hi when the box ends in the last cell of the grid (hi clamps into n - 1); a box of one cell keeps its upper
    corner inside."""
    q0, q1 = [], []
    for a in range(3):
        last = first[a] + shape[a] - 1
        assert 0 <= first[a] and last <= SOUP_N - 1
        q0.append(4 * first[a] + (0 if snap_lo[a] else 1))
        if snap_hi[a] and last == SOUP_N - 1:
            q1.append(4 * SOUP_N)
        elif snap_hi[a] and shape[a] > 1:
            q1.append(4 * last)
        else:
            q1.append(4 * last + 3)
    return q0, q1


def _box_triangle(q0, q1, g):
    """Three corners whose per-axis minimum and maximum are q0 and q1: two opposite corners of the box and a third one that is neither."""
    q0, q1 = np.asarray(q0), np.asarray(q1)
    pick = g.randint(0, 2, 3).astype(bool)
    if pick.all() or not pick.any():
        pick[g.randint(0, 3)] ^= True
    tri = np.stack([q0, q1, np.where(pick, q1, q0)])
    return tri[g.permutation(3)]


def _soup_mesh(boxes, seed):
    """boxes: per triangle (first cell [3], shape [3], snap_lo [3], snap_hi [3]) -> (vertices, faces, c0, c1, span); three vertices
    of its own per triangle, coordinates lo + q / 4 cell with integer q: exact in float64."""
    g = np.random.RandomState(seed)
    q = np.stack([_box_triangle(*_quarter_box(*b), g) for b in boxes])                       # [F, 3, 3] quarters
    c0 = np.asarray([b[0] for b in boxes], dtype=np.int64)
    c1 = c0 + np.asarray([b[1] for b in boxes], dtype=np.int64) - 1
    v = SOUP_LO + q.reshape(-1, 3) * (SOUP_CELL / 4.0)
    assert np.array_equal((v - SOUP_LO) * (4.0 / SOUP_CELL), q.reshape(-1, 3))
    f = np.arange(3 * len(boxes), dtype=np.int64).reshape(-1, 3)
    return _frozen(v, f, c0, c1, np.prod(c1 - c0 + 1, axis=1))


def _whole_box():
    return ([0, 0, 0], [SOUP_N] * 3, [True] * 3, [True] * 3)


def _lattice_soup():
    g = np.random.RandomState(2024)
    boxes = []
    for t in range(78 * len(SOUP_SHAPES)):
        shape = SOUP_SHAPES[t % len(SOUP_SHAPES)]
        first = [g.randint(0, SOUP_N - shape[a] + 1) for a in range(3)]
        if t % 13 == 0:                                             # some end in the grid's last cell, so that a corner sits at hi
            first[t % 3] = SOUP_N - shape[t % 3]
        snap = [bool((t >> b) & 1) for b in range(6)]
        boxes.append((first, shape, snap[0:3], snap[3:6]))
    boxes.append(_whole_box())                                      # pins lo and hi
    return _soup_mesh(boxes, 1)


def _by_lane():
    g = np.random.RandomState(650)
    tiny = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2)]
    large = [(3, 3, 1), (9, 1, 1), (1, 3, 3), (2, 5, 1)]               # spans 9, 9, 9, 10 > 8
    boxes = []
    for t in range(LANE_FACES):
        shape = large[t % 4] if t in LANE_OVERSIZE else tiny[t % 4]
        first = [g.randint(0, SOUP_N - shape[a] + 1) for a in range(3)]
        snap = [bool((t >> b) & 1) for b in range(6)]
        boxes.append((first, shape, snap[0:3], snap[3:6]))
    boxes[0] = _whole_box()
    return _soup_mesh(boxes, 2)


# ------------------------------------------------------------------------------------------------ the other meshes
def _lattice_01():
    """240 triangles with every vertex at lo + k * 0.1 as floating point computes it, k < 12: here nothing is exact, and the test
    demands only that host and device floor alike."""
    g = np.random.RandomState(3)
    lo = np.array([0.3, -0.7, 1.1])
    k = g.randint(0, 11, (240, 1, 3)) + g.randint(0, 3, (240, 3, 3))
    k[0], k[1] = [[0, 0, 0], [12, 0, 12], [0, 12, 12]], [[12, 12, 12], [0, 12, 0], [12, 0, 0]]
    v = lo + np.minimum(k, 12).reshape(-1, 3) * 0.1
    return _frozen(v, np.arange(720, dtype=np.int64).reshape(-1, 3))


def mean_edge(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float((np.linalg.norm(b - a, axis=1) + np.linalg.norm(c - b, axis=1) + np.linalg.norm(a - c, axis=1)).mean() / 3.0)


def _make(name):
    construction, cell, max_span = None, None, md.MAX_SPAN
    if name == 'lattice soup':
        v, f, c0, c1, span = _lattice_soup()
        construction, cell, max_span = (c0, c1, span), SOUP_CELL, SOUP_MAX_SPAN
    elif name.startswith('oversize by lane'):
        v, f, c0, c1, span = _cached('by lane', _by_lane)
        construction, cell = (c0, c1, span), SOUP_CELL
        max_span = SOUP_MAX_SPAN if name == 'oversize by lane' else SOUP_N ** 3
    elif name.startswith('one triangle'):
        v, f = rc.awkward_meshes()['a single triangle']
        cell, max_span = 0.5, 1 if name.endswith('oversize') else md.MAX_SPAN      # (its default grid is one cell: nothing spans more)
    elif name == 'flat box':
        v, f = rc.awkward_meshes()['flat bounding box']
    elif name == 'mesh in one point':
        v, f = np.full((5, 3), 0.3) * [1.0, -2.0, 3.0], np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4], [4, 4, 4]])
    elif name == 'cell 0.1':
        (v, f), cell = _lattice_01(), 0.1
    elif name == 'truncated grid':
        v, f = rc.icosphere(2)
        cell, max_span = float((v.max(0) - v.min(0)).max()) / 400.0, TRUNCATED_MAX_SPAN
    elif name == 'snapped cube':
        v, f = rc.snapped_cube(6)[:2]
    elif name == 'marching cubes':
        v, f = rc.mc_mesh()
    else:
        v, f = rc.awkward_meshes()[name]
    v, f = np.ascontiguousarray(v, dtype=np.float64), np.ascontiguousarray(f, dtype=np.int64)
    lo, hi = [float(x) for x in v.min(0)], [float(x) for x in v.max(0)]
    grid_cell, n = md.grid_shape(lo, hi, mean_edge(v, f), cell)
    return dict(name=name, vertices=v, faces=f, lo=lo, hi=hi, cell=grid_cell, n=n, max_span=max_span, cell_arg=cell, construction=construction)


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case(name):
    """-> dict(name, vertices, faces, lo, hi, cell, n, max_span: the grid as MeshIndex lays it with cell=cell_arg, max_span=max_span;
    construction: (c0, c1, span) in integer cell units, or None)."""
    return _cached(('case', name), lambda: _make(name))


def definition(name, cell=None):
    """host_tri_grid of a case, computed once (``cell``: the cell the device arrived at, where it chose one itself: a mean edge may
    differ from numpy's in the last bit)."""
    c = case(name)
    cell = c['cell'] if cell is None else cell

    def make():
        d = md.host_tri_grid(c['vertices'], c['faces'], c['lo'], c['hi'], cell, c['n'], c['max_span'])
        _frozen(*d.values())
        return d
    return _cached(('definition', name, cell), make)


# ------------------------------------------------------------------------------------------------ queries
def query_points(c, count, seed):
    """About ``count`` points for a case's grid: uniform in the box and around it, on cell boundaries (one, two and three coordinates
    on the lattice), at lo and hi, far outside."""
    g = np.random.RandomState(seed)
    lo, hi, cell, n = np.asarray(c['lo']), np.asarray(c['hi']), c['cell'], np.asarray(c['n'])
    m = count // 5
    inside = lo + g.random_sample((m, 3)) * (hi - lo)
    around = lo - 0.25 * (hi - lo) + g.random_sample((m, 3)) * 1.5 * (hi - lo)
    k = np.stack([g.randint(0, n[a] + 1, 2 * m) for a in range(3)], axis=1)
    lattice = lo + k * cell
    on = lo + g.random_sample((2 * m, 3)) * (hi - lo)
    keep = g.randint(1, 8, 2 * m)                                   # which coordinates sit on the lattice: 1 .. 7 as three bits
    for a in range(3):
        sel = (keep >> a) & 1 == 1
        on[sel, a] = lattice[sel, a]
    corners = np.array([[lo[a] if (i >> a) & 1 == 0 else hi[a] for a in range(3)] for i in range(8)])
    faces = lo + g.random_sample((m - 8, 3)) * (hi - lo)            # on the faces of the box
    ax = g.randint(0, 3, m - 8)
    faces[np.arange(m - 8), ax] = np.where(g.rand(m - 8) < 0.5, lo[ax], hi[ax])
    far = 0.5 * (lo + hi) + (g.random_sample((8, 3)) - 0.5) * 12.0 * (hi - lo)
    return np.concatenate([inside, around, on, corners, faces, far])[:count + 8]


def query_rays(c, count, seed):
    """About ``count`` rays for a case's grid -> (origins, directions): origins of ``query_points`` (in and around the box, on cell
    boundaries, at lo and hi, far outside) with directions toward a point of the box, and axis-parallel ones for a third of them."""
    g = np.random.RandomState(seed + 1000)
    lo, hi = np.asarray(c['lo']), np.asarray(c['hi'])
    o = query_points(c, count, seed + 500)
    target = lo + g.random_sample(o.shape) * (hi - lo)
    d = target - o
    axial = np.arange(len(o)) % 3 == 0
    keep = g.randint(0, 3, len(o))
    for a in range(3):
        d[axial & (keep != a), a] = 0.0
    d[axial & (np.abs(d).sum(axis=1) == 0.0)] = [0.0, 0.0, 1.0]
    return o, d


def home_cells(c, points, cell=None):
    """The (clamped) cell of each of points [Q, 3], as csrc/trigrid.h:md_cell forms it -> int64 [Q, 3]."""
    cell = c['cell'] if cell is None else cell
    t = np.floor((points - np.asarray(c['lo'])) * (1.0 / cell))
    return np.minimum(np.where(t >= 0.0, t, 0.0), np.asarray(c['n']) - 1.0).astype(np.int64)


def cell_centres(c, count, seed, axis):
    """``count`` points at centres of cells (a margin of 1e-9 cell can not reach a second column from there) -> (points, their cells
    [count, 3]); a fifth of them moved outside the box in the plane across ``axis`` by whole extents.  Where the grid stops short of
    the box on an axis, a seventh lie halfway between the grid's end and hi: in the box, and in the last cell."""
    g = np.random.RandomState(seed)
    lo, hi, cell, n = np.asarray(c['lo']), np.asarray(c['hi']), c['cell'], np.asarray(c['n'])
    k = np.stack([g.randint(0, n[a], count) for a in range(3)], axis=1)
    p = lo + (k + 0.5) * cell
    for a in range(3):
        if lo[a] + n[a] * cell < hi[a]:
            beyond = np.arange(count) % 7 == a
            k[beyond, a] = n[a] - 1
            p[beyond, a] = 0.5 * (lo[a] + n[a] * cell + hi[a])
    out = np.arange(count) % 5 == 4
    side = (axis + 1 + g.randint(0, 2, count)) % 3
    shift = np.where(g.rand(count) < 0.5, -1.0, 1.0) * (hi - lo + cell)[side] * (1 + g.randint(0, 2, count))
    p[out, side[out]] += shift[out]
    return p, k
