"""Analytic test fields for the mesh extraction, computed in numpy float64 FROM THE INTEGER LATTICE with + - * sqrt abs min max
only and rounded to float32 once, so that every path (reference libraries, numpy host path, device kernels) sees the same bits
through a look-up "model".  Used by tools/gen_golden_mesh.py and by tests/test_mesh_*.py."""
import numpy as np
import torch

BOX_SIZE = 2.4  # 2 + padding 0.4, the extractor's default


def _norm(*c):
    return np.sqrt(sum(x * x for x in c))


def sphere_rod_torus(R):
    """8 max(sphere, thin rod, thin torus) on the (R + 1)^3 lattice, x, y, z = i / R - 0.5 -> float32 [R + 1] * 3 (x-major).
    Positive inside.  The rod and the torus are thinner than a coarse voxel: refinement reaches them only through points that
    neighbouring subdivisions put on a coarse voxel's faces."""
    ax = np.arange(R + 1, dtype=np.float64) / R - 0.5
    x, y, z = ax[:, None, None], ax[None, :, None], ax[None, None, :]
    sphere = 0.30 - _norm(x + 0.08, y - 0.05, z + 0.02)
    rod = np.minimum(0.035 - _norm(y - 0.11, z + 0.13), 0.45 - np.abs(x))
    torus = 0.05 - _norm(_norm(x, z) - 0.36, y + 0.2)
    f = 8.0 * np.maximum(sphere, np.maximum(rod, torus))
    return np.broadcast_to(f, (R + 1,) * 3).astype(np.float32)


def checker(R, seed=0):
    """Seeded +-(1 + u) values: a second pattern that visits the ambiguous-face configurations smooth fields leave out."""
    g = np.random.RandomState(seed)
    sign = np.where(g.rand(R + 1, R + 1, R + 1) < 0.5, -1.0, 1.0)
    return (sign * (1.0 + g.rand(R + 1, R + 1, R + 1))).astype(np.float32)


class LookupModel(object):
    """A "model" with the reference's call signature that looks its values up in a lattice field:
    model(p[None], None, return_logits=True) -> [1, Q, 1], index = round((p / box_size + 0.5) * R) per axis.  ``calls`` counts
    the points asked for and ``seen`` marks them (to check that no point is evaluated twice)."""

    def __init__(self, field, box_size=BOX_SIZE):
        self.field = torch.as_tensor(np.ascontiguousarray(field))
        self.R = field.shape[0] - 1
        self.box_size = box_size
        self.n_points = 0
        self.seen = torch.zeros(field.shape, dtype=torch.int32)

    def to(self, device):
        if device is not None:
            self.field = self.field.to(device)
            self.seen = self.seen.to(device)
        return self

    def eval(self):
        return self

    def __call__(self, p, ray_d=None, return_logits=False, **kwargs):
        assert return_logits and p.dim() == 3 and p.shape[0] == 1
        q = p[0].to(torch.float64)
        idx = torch.round((q / self.box_size + 0.5) * self.R).long()
        assert bool(((idx >= 0) & (idx <= self.R)).all())
        self.n_points += idx.shape[0]
        self.seen.index_put_((idx[:, 0], idx[:, 1], idx[:, 2]), torch.ones(idx.shape[0], dtype=torch.int32, device=idx.device),
                             accumulate=True)
        return self.field[idx[:, 0], idx[:, 1], idx[:, 2]].reshape(1, -1, 1)


# ---------------------------------------------------------------------------------------------- mesh comparison ("same surface")
def lattice_edges(vertices):
    """Marching-cubes vertices in lattice units [V, 3] -> int64 [V, 4] (i, j, k, axis): the lattice edge each vertex lies on (the
    one non-integer coordinate names the axis).  A vertex that sits exactly on a lattice point is ambiguous and refused."""
    v = np.asarray(vertices, dtype=np.float64)
    r = np.round(v)
    frac = np.abs(v - r) > 1e-9
    assert (frac.sum(axis=1) == 1).all(), 'a vertex lies on a lattice point or off the lattice edges'
    axis = frac.argmax(axis=1)
    base = r.astype(np.int64)
    rows = np.arange(v.shape[0])
    base[rows, axis] = np.floor(v[rows, axis]).astype(np.int64)
    return np.concatenate([base, axis[:, None]], axis=1)


def _edge_keys(le):
    return [tuple(int(x) for x in e) for e in le]


def share_cell_face(e1, e2):
    """Do two lattice edges (i, j, k, axis) lie in one unit square of the lattice?"""
    a1, a2 = e1[3], e2[3]
    d = [e2[c] - e1[c] for c in range(3)]
    if a1 == a2:
        return d[a1] == 0 and sorted(abs(x) for x in d) == [0, 0, 1]
    third = 3 - a1 - a2
    if d[third] != 0:
        return False
    return (d[a1], d[a2]) in ((0, 0), (1, 0), (0, -1), (1, -1))


def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)


def is_closed_oriented(faces):
    """(b): every undirected mesh edge is used by exactly two triangles, once in each direction."""
    d = directed_edges(faces)
    if d.shape[0] == 0:
        return True
    if (d[:, 0] == d[:, 1]).any():
        return False
    big = int(d.max()) + 1
    fwd = d[:, 0] * big + d[:, 1]
    if np.unique(fwd).shape[0] != fwd.shape[0]:
        return False  # a directed edge twice
    rev = d[:, 1] * big + d[:, 0]
    return bool(np.array_equal(np.sort(fwd), np.sort(rev)))


def face_segments(vertices, faces):
    """(c): the directed mesh edges whose two lattice edges share a cell face, as a set of (lattice edge, lattice edge)."""
    keys = _edge_keys(lattice_edges(vertices))
    out = set()
    for a, b in directed_edges(faces):
        ka, kb = keys[a], keys[b]
        if share_cell_face(ka, kb):
            assert (ka, kb) not in out
            out.add((ka, kb))
    return out


def area_volume(vertices, faces):
    v, f = np.asarray(vertices, dtype=np.float64), np.asarray(faces, dtype=np.int64)
    if f.shape[0] == 0:
        return 0.0, 0.0
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(axis=1)).sum()
    volume = (a * np.cross(b, c)).sum() / 6.0
    return float(area), float(volume)


def assert_same_surface(v1, f1, v2, f2, what=''):
    """(a) - (e) of the mesh contract, both meshes in lattice units: same vertex-carrying lattice edges with vertices equal to
    1e-9; closed and consistently oriented; same directed face segments; same triangle count; signed volumes of one sign within
    (cells with triangles) x (cell volume), areas within that count x (cell face area)."""
    e1, e2 = lattice_edges(v1), lattice_edges(v2)
    k1, k2 = _edge_keys(e1), _edge_keys(e2)
    assert len(set(k1)) == len(k1) and len(set(k2)) == len(k2), what + ': a lattice edge carries two vertices'
    assert set(k1) == set(k2), what + ': different vertex-carrying lattice edges'
    pos2 = dict((k, i) for i, k in enumerate(k2))
    match = np.array([pos2[k] for k in k1], dtype=np.int64)
    err = np.abs(np.asarray(v1) - np.asarray(v2)[match]).max() if len(k1) else 0.0
    print('%s: %d vertices, %d / %d faces, max vertex difference %.3e lattice units' % (what, len(k1), len(f1), len(f2), err))
    assert err < 1e-9, what + ': vertices differ by %g' % err
    assert is_closed_oriented(f1) and is_closed_oriented(f2), what + ': not closed / consistently oriented'
    assert face_segments(v1, f1) == face_segments(v2, f2), what + ': different face segments'
    assert len(f1) == len(f2), what + ': %d vs %d triangles' % (len(f1), len(f2))
    (a1, w1), (a2, w2) = area_volume(v1, f1), area_volume(v2, f2)
    n_cells = len(set(tuple(c) for c in np.floor(np.asarray(v2)[np.asarray(f2)].mean(axis=1) + 1e-12).astype(np.int64))) if len(f2) else 0
    print('%s: area %.6f / %.6f, volume %.6f / %.6f, %d cells' % (what, a1, a2, w1, w2, n_cells))
    assert w1 * w2 > 0 or (w1 == 0 and w2 == 0), what + ': volumes of different sign'
    assert abs(w1 - w2) < max(n_cells, 1) * 1.0 and abs(a1 - a2) < max(n_cells, 1) * 1.0, what + ': area / volume'


def edges_digest(vertices):
    """sha256 of the sorted int64 list of vertex-carrying lattice edges."""
    import hashlib
    e = lattice_edges(vertices)
    e = e[np.lexsort((e[:, 3], e[:, 2], e[:, 1], e[:, 0]))]
    return hashlib.sha256(np.ascontiguousarray(e.astype('<i8')).tobytes()).hexdigest()
