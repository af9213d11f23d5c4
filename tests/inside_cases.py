"""Shared constructions of the inside-test and mesh-evaluation tests (tests/test_inside_*.py, tests/test_mesheval_*.py): closed, open
and nested meshes whose inside is known without the code under test, and seeded point sets, among them the ones laid exactly on the
triangle grid's column boundaries and on the mesh's own vertices and edges, where a crossing count has to break ties.  Everything is
numpy float64 and deterministic."""
import numpy as np

from tests import raycast_cases as rc

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ meshes
BOX_LO = np.array([0.25, -0.5, 0.125])       # binary fractions: every lattice point below is exact
BOX_HI = np.array([1.0, 0.75, 0.875])


def box(seed=0):
    """The surface of the axis-aligned box [BOX_LO, BOX_HI] as 12 triangles, each randomly flipped and rotated, in random order: the
    crossing counts may depend on neither orientation nor order."""
    def make():
        corner = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)
        v = BOX_LO + corner * (BOX_HI - BOX_LO)
        quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
        f = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], dtype=np.int64)
        g = np.random.RandomState(seed)
        for t in range(len(f)):
            if g.rand() < 0.5:
                f[t] = f[t][::-1]
            f[t] = np.roll(f[t], g.randint(3))
        return v, f[g.permutation(len(f))]
    return _cached(('box', seed), make)


def box_lattice():
    """17^3 points lo + (i - 4) (hi - lo) / 8, i = 0 .. 16 per axis: every face, edge and corner of the box carries lattice points, and
    four layers lie outside on every side."""
    ax = [BOX_LO[a] + (np.arange(17) - 4) * (BOX_HI[a] - BOX_LO[a]) / 8 for a in range(3)]
    return np.stack(np.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3)


def _lattice_field(fn, offset):
    ax = 2.0 * (np.arange(17, dtype=np.float64) / 16 - 0.5)
    return fn(ax[:, None, None] - offset[0], ax[None, :, None] - offset[1], ax[None, None, :] - offset[2]).astype(np.float32)


def _mc(field):
    from psnerf_amd.stage1.extracting import host_marching_cubes
    v, f = host_marching_cubes(field, 0.0)
    padded = np.pad(field.astype(np.float64), 1, 'constant', constant_values=-1e6)     # (what marching cubes saw)
    n = padded.shape[0]
    lattice = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing='ij'), -1).reshape(-1, 3)
    return v, f, padded.reshape(-1), lattice


def mc_sphere():
    """host_marching_cubes of a sphere in general position (centre (0.013, -0.007, 0.003), radius 0.6131 in [-1, 1]^3, float32 field on
    the 17^3 lattice, positive inside) -> (vertices in units of the padded lattice, faces, the padded field [19^3], the padded
    lattice's points [19^3, 3]).  Every vertex lies on a lattice line, so the line through EVERY lattice point runs through vertices."""
    return _cached('mc sphere', lambda: _mc(_lattice_field(lambda x, y, z: 0.6131 - np.sqrt(x * x + y * y + z * z), (0.013, -0.007, 0.003))))


def mc_sphere_small():
    """The same sphere with radius 0.4517: a second marching-cubes mesh to evaluate the first against."""
    return _cached('mc sphere small', lambda: _mc(_lattice_field(lambda x, y, z: 0.4517 - np.sqrt(x * x + y * y + z * z), (0.013, -0.007, 0.003))))


def mc_torus():
    """Likewise a torus around z (radii 0.55 and 0.27) with the offset (0.011, 0.006, -0.009)."""
    return _cached('mc torus', lambda: _mc(_lattice_field(lambda x, y, z: 0.27 - np.sqrt((np.sqrt(x * x + y * y) - 0.55) ** 2 + z * z),
                                                        (0.011, 0.006, -0.009))))


def hemisphere(level=2):
    """The icosphere with every face removed whose centroid has z < 0: a dome open downward."""
    v, f = rc.icosphere(level)
    return v, f[v[f].mean(axis=1)[:, 2] >= 0.0]


def nested(level=2, inner=0.5):
    """Two concentric icospheres of radius 1 and ``inner``, both oriented outward."""
    v, f = rc.icosphere(level)
    return np.concatenate([v, inner * v]), np.concatenate([f, f + len(v)])


def volume(v, f):
    """The exact volume a closed oriented mesh encloses: the sum of a . (b x c) / 6."""
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return float((a * np.cross(b, c)).sum() / 6.0)


def five_sigma(share, n, box_volume):
    """The gap allowed between a Monte-Carlo volume from n uniform points and the true one: 5 standard deviations of the binomial
    share, sqrt(p (1 - p) / n), times the box's volume (p = the true share)."""
    return 5.0 * np.sqrt(share * (1.0 - share) / n) * box_volume


# ------------------------------------------------------------------------------------------------ point sets
def margin(lo, cell, n, points):
    """The walk's margin (csrc/meshinside.hip) for the largest coordinate of the set."""
    scale = max(float(np.abs(points[np.isfinite(points)]).max()), float(np.abs(lo).max()), float(np.abs(lo + n * cell).max()))
    return 1e-9 * cell + 1e-12 * scale


def point_sets(v, f, lo, cell, n, axis, count, seed=0, focus=None):
    """name -> points [Q, 3], Q <= count, for the mesh (v, f) whose grid has the lower corner lo, the cell edge ``cell`` and n cells
    per axis (what MeshIndex reports), for lines along ``axis``.  ``focus`` = (lower, upper corner) of the part of the mesh the
    points are laid around (default: its bounding box)."""
    g = np.random.RandomState(seed)
    lo, n = np.asarray(lo, dtype=np.float64), np.asarray(n)
    kx, ky, kz = (axis + 1) % 3, (axis + 2) % 3, axis
    blo, bhi = (v.min(0), v.max(0)) if focus is None else (np.asarray(focus[0], dtype=np.float64), np.asarray(focus[1], dtype=np.float64))
    ext = np.maximum(bhi - blo, cell)
    uniform = lambda m: blo - 0.1 * ext + g.random_sample((m, 3)) * 1.2 * ext
    k_lo = np.clip(np.floor((blo - lo) / cell).astype(np.int64) - 1, 0, n)
    k_hi = np.clip(np.ceil((bhi - lo) / cell).astype(np.int64) + 1, 0, n)
    plane = lambda a, m: lo[a] + g.randint(k_lo[a], k_hi[a] + 1, m) * cell
    out = {'uniform, box + 10 %': uniform(count)}

    p = uniform(count)
    third = count // 3
    p[:third, kx] = plane(kx, third)
    p[third:2 * third, ky] = plane(ky, third)
    p[2 * third:, kx], p[2 * third:, ky] = plane(kx, count - 2 * third), plane(ky, count - 2 * third)
    out['on column boundaries'] = p

    q = p.copy()
    m = margin(lo, cell, n, q)
    q[:, kx] += np.where(np.arange(count) < third, 1.0, 0.0) * (g.random_sample(count) - 0.5) * m
    q[:, ky] += np.where((np.arange(count) >= third) & (np.arange(count) < 2 * third), 1.0, 0.0) * (g.random_sample(count) - 0.5) * m
    q[2 * third:, kx] += (g.random_sample(count - 2 * third) - 0.5) * m
    q[2 * third:, ky] += (g.random_sample(count - 2 * third) - 0.5) * m
    out['within half a margin of column boundaries'] = q

    used = np.unique(f)
    p = v[used[g.randint(0, len(used), count)]].copy()
    p[:, kz] = uniform(count)[:, kz]
    out['under and over vertices'] = p

    e = f[g.randint(0, len(f), count)]
    side = g.randint(0, 3, count)
    mid = 0.5 * (v[e[np.arange(count), side]] + v[e[np.arange(count), (side + 1) % 3]])
    p = mid.copy()
    p[:, kz] = uniform(count)[:, kz]
    out['under and over edge midpoints'] = p

    half = count // 2
    out['vertices and face centroids'] = np.concatenate([v[used[g.randint(0, len(used), half)]], v[f[g.randint(0, len(f), count - half)]].mean(axis=1)])

    p = uniform(count)
    a = g.randint(0, 3, count)
    far = np.where(g.rand(count) < 0.5, v.min(0)[a] - (0.01 + g.rand(count)) * ext[a], v.max(0)[a] + (0.01 + g.rand(count)) * ext[a])
    p[np.arange(count), a] = far
    out['outside the box'] = p

    m = min(count, 256)
    p = uniform(m)
    p[0::8, 0] = np.nan
    p[1::8, 1] = np.inf
    p[2::8, 2] = -np.inf
    p[3::8] = np.nan
    out['NaN and infinite rows'] = p
    return out
