"""Mesh simplification: quadric vertex clustering on a uniform grid, to a cell size, a resolution or a face budget.  The shipped
extraction (resolution 64, upsampling_steps 3) returns several hundred thousand faces per object; the lineage of the extractor
(Occupancy Networks' ``Generator3D(simplify_nfaces=)``) had a simplification step behind a native library, which UNISURF and the
reference dropped with that library.  This one needs no library: all vertices of one grid cell become one vertex, placed at the
minimiser of the cell's regularised quadric error (after Lindstrom, "Out-of-core simplification of large polygonal models", 2000).

Two implementations of one definition, as in meshclean.py and meshdist.py:
  * CPU inputs -> the numpy functions below (``host_*``), float64 / int64; they are the definition, and what the device path is
    tested against, bit for bit.
  * device tensors (or ``device='cuda'``) -> csrc/meshsimplify.hip: psn_vc_cell_keys, a stable torch.sort + head flags + cumsum (the
    clusters and their vertex runs), psn_vc_face_keys, one torch.sort of the corner keys (each cluster's run of (face, corner)
    pairs) and one stable sort of the face keys (the duplicates), psn_vc_solve (a wave per cluster), psn_vc_face_flags, two
    torch.cumsum scans and meshclean's psn_cc_compact.  Host reads: the bounding box, one row (status, clusters, faces,
    degenerate faces) per grid tried, and the final totals.  No floating-point atomics: two runs give the same bits.

Definition.
  Inputs.  vertices float64 [V, 3], non-finite values raise ValueError; faces int64 [F, 3], an index outside 0 .. V - 1 raises
    ValueError.  Duplicated faces, faces with a repeated index and unreferenced vertices are legal.
  Grid.  origin = the per-axis minimum of all vertices, extent = the maximum minus the origin.  Either the cell edge h = ``cell`` > 0
    is given, or ``resolution`` = n with 1 <= n <= MAX_RESOLUTION (4096) and h = max(extent) / n (h = 1 when the extent is zero on
    every axis: one cell).  dims_a = floor(extent_a / h) + 1; a ``cell`` that gives more than MAX_RESOLUTION + 1 cells along an axis
    raises ValueError.  origin, h and dims are Python floats / ints on the host in both paths.  A vertex's cell is
    c_a = min(max(floor((v_a - origin_a) / h), 0), dims_a - 1), its key (c_z dims_y + c_y) dims_x + c_x.
  Clusters.  The occupied cells ascending by key; cluster[v] = the rank of v's cell.  More than MAX_CLUSTERS = 2^21 - 1 clusters
    raise ValueError on both paths (three cluster ids share one 63-bit face key).
  Centroid.  x0[k] = (the sum of the cluster's vertices, added one after the other in ascending vertex index, starting from 0) /
    count.  Every vertex counts, referenced by a face or not.
  Quadric.  Per face n = (b - a) x (c - a), unnormalised (the weight is area^2):
        nx = ab_y ac_z - ab_z ac_y,  ny = ab_z ac_x - ab_x ac_z,  nz = ab_x ac_y - ab_y ac_x.
    Every (face, corner) pair contributes to the cluster k of that corner (a face with two corners in one cluster contributes twice),
    in ascending (face, corner), each sum starting from 0:
        A00 += nx nx, A01 += nx ny, A02 += nx nz, A11 += ny ny, A12 += ny nz, A22 += nz nz
        d = (nx (a_x - x0_x) + ny (a_y - x0_y)) + nz (a_z - x0_z);   r_x += nx d, r_y += ny d, r_z += nz d
    with a the face's FIRST vertex and x0 = x0[k]: r is formed relative to the centroid, which avoids the cancellation in b - A x0.
  Position.  t = (A00 + A11) + A22.  t == 0: x = x0.  Otherwise lam = regularisation t (default 1e-3; must be > 0),
    m00 = A00 + lam, m11 = A11 + lam, m22 = A22 + lam, and (A + lam I) delta = r is solved by this LDL^T sequence, verbatim on both paths:
        l10 = A01 / m00;  l20 = A02 / m00;  d1 = m11 - l10 A01;  e21 = A12 - l20 A01;  l21 = e21 / d1
        d2 = (m22 - l20 A02) - l21 e21
        y1 = r_y - l10 r_x;  y2 = (r_z - l20 r_x) - l21 y1
        dz = y2 / d2;  dy = y1 / d1 - l21 dz;  dx = (r_x / m00 - l10 dy) - l20 dz;   x = x0 + (dx, dy, dz)
    The matrix is symmetric positive definite with condition number <= (1 + regularisation) / regularisation, so the pivots are
    positive and a direct method is safe in float64; no iterative eigen-solver (none would match numpy's bits).  The regularisation
    pulls the directions the faces do not determine (flat regions, straight edges) to the centroid: a parameter of the definition,
    not a tolerance.  x is then clamped per axis into [origin_a + c_a h, origin_a + (c_a + 1) h] (x < lo ? lo : x, then
    x > hi ? hi : x); n_clamped counts the clusters (all of them) where the clamp moved a coordinate.
  Faces.  Re-index through ``cluster``; drop a face that names a cluster twice (n_faces_degenerate); rotate the rest so that the
    smallest id comes first, orientation kept, and give it the key (g0 2^21 + g1) 2^21 + g2; of equal keys keep the first in face
    order (n_faces_duplicate).  Two faces over the same three clusters with OPPOSITE orientation have different keys and both stay:
    a thin sheet collapsed onto itself keeps its two sides.  n_faces_flipped counts the surviving faces whose new normal
    m = (x[g1] - x[g0]) x (x[g2] - x[g0]) (corner order as in the input face, the cross product as above) has
    (nx mx + ny my) + nz mz < 0 with their old normal n: a report value only.
  Output.  The surviving faces in their original order and with their original corner order (the rotation only serves the
    comparison); exactly the clusters a surviving face names, ascending by key; faces re-indexed.  Normals do not ride along:
    positions move, and the extractor estimates normals after this step.
  target_faces = N.  F <= N: the mesh is returned untouched, report {'unchanged': True}.  Otherwise count(n) = the number of output
    faces at resolution n, +inf where the cluster limit is exceeded.  count(MAX_RESOLUTION) <= N: use MAX_RESOLUTION.  Else
    count(1) > N: use 1, report 'target_missed': True.  Else bisect: lo = 1, hi = MAX_RESOLUTION; while hi - lo > 1:
    mid = (lo + hi) // 2, lo = mid if count(mid) <= N else hi = mid; use lo.  count is nearly but not strictly monotone: the contract
    is n_faces <= N and that both paths choose the same n, not optimality.  The report lists the probes as (n, count) in the order
    they were made.  A probe runs the key kernels, the sorts and the count only, never the solve.
  Report.  resolution (None when ``cell`` was given), cell, dims, n_clusters, n_vertices, n_faces, n_clamped, n_faces_degenerate,
    n_faces_duplicate, n_faces_flipped, probes (and unchanged / target_missed when they apply).
"""
import math

import numpy as np
import torch

from .meshcore import Mesh, Phase, device_mesh, face_cross, host_mesh, mesh_parts, on_device, to_numpy

MAX_RESOLUTION = 4096          # == PSN_VC_MAX_RESOLUTION
MAX_CLUSTERS = (1 << 21) - 1   # == PSN_VC_MAX_CLUSTERS
ID_BITS = 21


# ------------------------------------------------------------------------------------------------ arguments and the grid
def _check_sizes(target_faces, cell, resolution, regularisation):
    if sum(x is not None for x in (target_faces, cell, resolution)) != 1:
        raise ValueError('simplify: exactly one of target_faces, cell and resolution must be given')
    if not (float(regularisation) > 0.0 and math.isfinite(float(regularisation))):
        raise ValueError('simplify: regularisation=%r (must be > 0)' % (regularisation,))
    if cell is not None and not (float(cell) > 0.0 and math.isfinite(float(cell))):
        raise ValueError('simplify: cell=%r (must be > 0)' % (cell,))
    if resolution is not None and not 1 <= int(resolution) <= MAX_RESOLUTION:
        raise ValueError('simplify: resolution=%r (1 .. %d)' % (resolution, MAX_RESOLUTION))
    if target_faces is not None and int(target_faces) < 1:
        raise ValueError('simplify: target_faces=%r (at least 1)' % (target_faces,))


def make_grid(lo, hi, cell=None, resolution=None):
    """(origin, h, dims) in Python floats / ints from the bounding box, as the definition states; the same function on both paths."""
    lo, hi = [float(x) for x in lo], [float(x) for x in hi]
    if not all(math.isfinite(x) for x in lo + hi):
        raise ValueError('simplify: a vertex coordinate is not finite')
    extent = [hi[a] - lo[a] for a in range(3)]
    if cell is not None:
        h = float(cell)
    else:
        h = max(extent) / int(resolution)
        if max(extent) == 0.0:
            h = 1.0
    if not (h > 0.0 and math.isfinite(h)):
        raise ValueError('simplify: cell edge %r' % h)
    dims = []
    for a in range(3):
        q = math.floor(extent[a] / h)
        if not q <= MAX_RESOLUTION:
            raise ValueError('simplify: cell=%r gives more than %d cells along an axis; use a coarser cell' % (h, MAX_RESOLUTION + 1))
        dims.append(int(q) + 1)
    return tuple(lo), h, tuple(dims)


def _too_many(n_clusters):
    return ValueError('simplify: %d clusters (at most %d); use a coarser cell' % (n_clusters, MAX_CLUSTERS))


# ------------------------------------------------------------------------------------------------ host path: the definition
def host_cell_keys(v, grid):
    origin, h, dims = grid
    c = [np.minimum(np.maximum(np.floor((v[:, a] - origin[a]) / h), 0.0), float(dims[a] - 1)).astype(np.int64) for a in range(3)]
    return (c[2] * dims[1] + c[1]) * dims[0] + c[0]


def host_clusters(vertices, grid):
    """-> (cluster int64 [V], keys of the clusters int64 [C], ascending)."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    cell_key, cluster = np.unique(host_cell_keys(v, grid), return_inverse=True)
    return cluster.reshape(-1).astype(np.int64), cell_key.astype(np.int64)


def host_face_keys(f, cluster):
    """-> (g int64 [F, 3]: the faces re-indexed; key int64 [F]: the rotated triple in 3 x 21 bits, -1 for a degenerate face)."""
    g = cluster[f].reshape(-1, 3)
    g0, g1, g2 = g[:, 0], g[:, 1], g[:, 2]
    degenerate = (g0 == g1) | (g1 == g2) | (g0 == g2)
    first = np.where((g0 < g1) & (g0 < g2), 0, np.where(g1 < g2, 1, 2))    # (ids differ where it matters)
    rows = np.arange(g.shape[0])
    r0, r1, r2 = g[rows, first], g[rows, (first + 1) % 3], g[rows, (first + 2) % 3]
    key = (((r0 << ID_BITS) + r1) << ID_BITS) + r2
    return g, np.where(degenerate, -1, key)


def host_keep_faces(key):
    """-> bool [F]: not degenerate and the first of its key in face order."""
    order = np.argsort(key, kind='stable')
    s = key[order]
    head = s >= 0
    head[1:] &= s[1:] != s[:-1]
    keep = np.zeros(key.shape[0], dtype=bool)
    keep[order] = head
    return keep


def _host_count(v, f, grid):
    """(n_clusters, n output faces) of one grid: what a target_faces probe computes."""
    cluster, cell_key = host_clusters(v, grid)
    if cell_key.shape[0] > MAX_CLUSTERS:
        return cell_key.shape[0], math.inf
    return cell_key.shape[0], int(host_keep_faces(host_face_keys(f, cluster)[1]).sum())


def solve_positions(x0, A, r, regularisation):
    """The definition's LDL^T sequence on arrays ([C, 3] centroids, [C, 6] A00 A01 A02 A11 A12 A22, [C, 3] r) -> x [C, 3]."""
    A00, A01, A02, A11, A12, A22 = (A[:, i] for i in range(6))
    t = (A00 + A11) + A22
    live = t != 0.0
    lam = regularisation * t
    one = np.ones_like(t)
    m00, m11, m22 = np.where(live, A00 + lam, one), np.where(live, A11 + lam, one), np.where(live, A22 + lam, one)
    l10 = A01 / m00
    l20 = A02 / m00
    d1 = m11 - l10 * A01
    e21 = A12 - l20 * A01
    l21 = e21 / d1
    d2 = (m22 - l20 * A02) - l21 * e21
    y1 = r[:, 1] - l10 * r[:, 0]
    y2 = (r[:, 2] - l20 * r[:, 0]) - l21 * y1
    dz = y2 / d2
    dy = y1 / d1 - l21 * dz
    dx = (r[:, 0] / m00 - l10 * dy) - l20 * dz
    delta = np.stack([dx, dy, dz], axis=1)
    return np.where(live[:, None], x0 + delta, x0)


def host_quadrics(v, f, cluster, n_clusters):
    """-> (x0 [C, 3], A [C, 6], r [C, 3], count int64 [C]) by the definition's sums (np.bincount adds one weight after the other in
    index order, each bin starting from 0)."""
    count = np.bincount(cluster, minlength=n_clusters)
    x0 = np.stack([np.bincount(cluster, weights=v[:, a], minlength=n_clusters) for a in range(3)], axis=1) / count[:, None]
    a = v[f[:, 0]]
    n = face_cross(v, f)
    k = cluster[f].reshape(-1)                                   # ascending (face, corner)
    n3 = [np.repeat(x, 3) for x in n]
    a3 = np.repeat(a, 3, axis=0)
    rel = a3 - x0[k]
    d = (n3[0] * rel[:, 0] + n3[1] * rel[:, 1]) + n3[2] * rel[:, 2]
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    A = np.stack([np.bincount(k, weights=n3[i] * n3[j], minlength=n_clusters) for i, j in pairs], axis=1)
    r = np.stack([np.bincount(k, weights=n3[i] * d, minlength=n_clusters) for i in range(3)], axis=1)
    return x0, A, r, count


def host_positions(v, f, cluster, cell_key, grid, regularisation=1e-3, clamp=True, minimiser=True):
    """-> (x float64 [C, 3], clamped bool [C]).  ``clamp=False`` / ``minimiser=False`` (the centroid) are the wrong formulations the
    tests show to fail."""
    origin, h, dims = grid
    x0, A, r, _ = host_quadrics(v, f, cluster, cell_key.shape[0])
    x = solve_positions(x0, A, r, float(regularisation)) if minimiser else x0
    cx, rest = cell_key % dims[0], cell_key // dims[0]
    cells = np.stack([cx, rest % dims[1], rest // dims[1]], axis=1).astype(np.float64)
    lo = np.asarray(origin)[None, :] + cells * h
    hi = np.asarray(origin)[None, :] + (cells + 1.0) * h
    y = np.where(x < lo, lo, x)
    y = np.where(y > hi, hi, y)
    clamped = (y != x).any(axis=1)
    return (y if clamp else x), clamped


def _host_at(v, f, grid, regularisation, resolution, probes, deduplicate=True, clamp=True, minimiser=True):
    origin, h, dims = grid
    cluster, cell_key = host_clusters(v, grid)
    n_clusters = cell_key.shape[0]
    if n_clusters > MAX_CLUSTERS:
        raise _too_many(n_clusters)
    report = {'resolution': resolution, 'cell': h, 'dims': dims, 'n_clusters': n_clusters, 'probes': probes}
    if f.shape[0] == 0:
        report.update(n_vertices=0, n_faces=0, n_clamped=0, n_faces_degenerate=0, n_faces_duplicate=0, n_faces_flipped=0)
        return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64), report
    g, key = host_face_keys(f, cluster)
    keep = host_keep_faces(key) if deduplicate else key >= 0
    x, clamped = host_positions(v, f, cluster, cell_key, grid, regularisation, clamp, minimiser)
    out_g = g[keep]
    old, new = face_cross(v, f[keep]), face_cross(x, out_g)
    flipped = ((old[0] * new[0] + old[1] * new[1]) + old[2] * new[2]) < 0.0
    used = np.zeros(n_clusters, dtype=bool)
    used[out_g.reshape(-1)] = True
    new_index = np.cumsum(used) - 1
    n_degenerate = int((key < 0).sum())
    report.update(n_vertices=int(used.sum()), n_faces=int(out_g.shape[0]), n_clamped=int(clamped.sum()), n_faces_degenerate=n_degenerate,
                  n_faces_duplicate=int(f.shape[0] - n_degenerate - out_g.shape[0]), n_faces_flipped=int(flipped.sum()))
    return x[used], new_index[out_g].astype(np.int64).reshape(-1, 3), report


def choose_resolution(target, count):
    """The definition's search: ``count(n)`` -> the number of output faces at resolution n (math.inf beyond the cluster limit)
    -> (n, probes, target_missed).  The same function drives both paths."""
    probes = []

    def probe(n):
        probes.append((n, count(n)))
        return probes[-1][1]
    if probe(MAX_RESOLUTION) <= target:
        return MAX_RESOLUTION, probes, False
    if probe(1) > target:
        return 1, probes, True
    lo, hi = 1, MAX_RESOLUTION
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if probe(mid) <= target:
            lo = mid
        else:
            hi = mid
    return lo, probes, False


def _unchanged_report(n_vertices, n_faces):
    return {'unchanged': True, 'resolution': None, 'cell': None, 'dims': None, 'n_clusters': int(n_vertices), 'n_vertices': int(n_vertices),
            'n_faces': int(n_faces), 'n_clamped': 0, 'n_faces_degenerate': 0, 'n_faces_duplicate': 0, 'n_faces_flipped': 0, 'probes': []}


def _empty_report(cell, resolution):
    return {'resolution': resolution, 'cell': cell, 'dims': (1, 1, 1), 'n_clusters': 0, 'n_vertices': 0, 'n_faces': 0, 'n_clamped': 0,
            'n_faces_degenerate': 0, 'n_faces_duplicate': 0, 'n_faces_flipped': 0, 'probes': []}


def host_simplify(vertices, faces, target_faces=None, cell=None, resolution=None, regularisation=1e-3, **wrong):
    """-> (vertices float64 [V', 3], faces int64 [F', 3], report).  ``wrong``: deduplicate / clamp / minimiser = False switch one
    rule of the definition off (tests only)."""
    _check_sizes(target_faces, cell, resolution, regularisation)
    v, f, _ = host_mesh(vertices, faces, finite='simplify')
    if target_faces is not None and f.shape[0] <= int(target_faces):
        return v, f, _unchanged_report(v.shape[0], f.shape[0])
    if v.shape[0] == 0:
        return v, f, _empty_report(cell, resolution)
    lo, hi = v.min(axis=0), v.max(axis=0)
    probes, missed = [], False
    if target_faces is not None:
        resolution, probes, missed = choose_resolution(int(target_faces),
                                                       lambda n: _host_count(v, f, make_grid(lo, hi, None, n))[1])
    out_v, out_f, report = _host_at(v, f, make_grid(lo, hi, cell, resolution), regularisation, None if cell is not None else int(resolution),
                                    probes, **wrong)
    if missed:
        report['target_missed'] = True
    return out_v, out_f, report


# ------------------------------------------------------------------------------------------------ device path
def _raise_status(status, n_vertices, n_clusters):
    """An out-of-range index is the caller's error whatever else happened.  More clusters than the limit is the caller's error too,
    and is raised (or counted as +inf by a probe) where the definition does so: the kernel then could not pack some ids and says so,
    which is not a fault of its own.  The cluster bit WITHIN the limit would be one."""
    from . import hip
    if status & hip.VC_E_INDEX:
        raise ValueError('mesh: a face refers to a vertex outside 0 .. %d' % (n_vertices - 1))
    if status & hip.VC_E_CLUSTER and n_clusters <= min(MAX_CLUSTERS, hip.VC_MAX_CLUSTERS):
        raise RuntimeError('meshsimplify: a cluster id outside 0 .. %d reached the face keys (status %d)' % (MAX_CLUSTERS - 1, status))


class _DeviceGrid(object):
    """Everything one grid needs before the solve: the clusters, the face keys, their sorts and the one host read."""

    def __init__(self, v, f, grid, full, events=None):
        from . import hip
        n_v, n_f = v.shape[0], f.shape[0]
        dev = v.device
        self.grid = grid
        with Phase(events, 'clusters'):
            keys = hip.vc_cell_keys(v, grid)
            self.cell_key_sorted, self.vertex_order = torch.sort(keys, stable=True)
            head = torch.ones(n_v, dtype=torch.bool, device=dev)
            head[1:] = self.cell_key_sorted[1:] != self.cell_key_sorted[:-1]
            self.rank_sorted = torch.cumsum(head, dim=0, dtype=torch.int64) - 1          # the cluster of each sorted vertex
            self.cluster = torch.empty(n_v, dtype=torch.int64, device=dev)
            self.cluster[self.vertex_order] = self.rank_sorted
        with Phase(events, 'face keys'):
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            self.corner_keys, face_keys, self.g = hip.vc_face_keys(f, self.cluster, status, want_corners=full)
            self.face_key_sorted, self.face_order = torch.sort(face_keys, stable=True)
            self.face_head = self.face_key_sorted >= 0
            self.face_head[1:] &= self.face_key_sorted[1:] != self.face_key_sorted[:-1]
            row = torch.stack([status[0].to(torch.int64), self.rank_sorted[-1] + 1, self.face_head.sum(), (self.face_key_sorted < 0).sum()])
        status, self.n_clusters, self.n_faces, self.n_degenerate = (int(x) for x in row.tolist())      # the one host read
        _raise_status(status, n_v, self.n_clusters)


def _device_at(v, f, grid, regularisation, resolution, probes, events=None):
    from . import hip
    origin, h, dims = grid
    n_v, n_f = v.shape[0], f.shape[0]
    dev = v.device
    report = {'resolution': resolution, 'cell': h, 'dims': dims, 'probes': probes}
    if n_f == 0:
        keys = hip.vc_cell_keys(v, grid)
        report.update(n_clusters=int(torch.unique(keys).numel()), n_vertices=0, n_faces=0, n_clamped=0, n_faces_degenerate=0,
                      n_faces_duplicate=0, n_faces_flipped=0)
        if report['n_clusters'] > MAX_CLUSTERS:
            raise _too_many(report['n_clusters'])
        return v.new_zeros((0, 3)), f.new_zeros((0, 3)), report
    d = _DeviceGrid(v, f, grid, True, events)
    n_c = d.n_clusters
    if n_c > MAX_CLUSTERS:
        raise _too_many(n_c)
    with Phase(events, 'runs'):
        bounds = torch.arange(n_c + 1, dtype=torch.int64, device=dev)
        vertex_start = torch.searchsorted(d.rank_sorted, bounds)
        corner_sorted = torch.sort(d.corner_keys).values
        corner_start = torch.searchsorted(corner_sorted, bounds * (3 * n_f))
        face_keep = torch.zeros(n_f, dtype=torch.uint8, device=dev)
        face_keep[d.face_order] = d.face_head.to(torch.uint8)
    with Phase(events, 'solve'):
        x, clamped = hip.vc_solve(v, f, d.vertex_order, vertex_start, d.cell_key_sorted, corner_sorted, corner_start, n_c, grid,
                                  float(regularisation))
    with Phase(events, 'compaction'):
        vertex_keep, flipped = hip.vc_face_flags(v, f, d.g, x, face_keep)
        face_incl, vertex_incl = torch.cumsum(face_keep, dim=0, dtype=torch.int64), torch.cumsum(vertex_keep, dim=0, dtype=torch.int64)
        totals = torch.stack([face_incl[-1], vertex_incl[-1], clamped.sum(), flipped.sum()]).tolist()
        n_out_f, n_out_v = int(totals[0]), int(totals[1])
        out_v, out_f, _ = hip.cc_compact(x, d.g, None, face_keep, vertex_keep, face_incl - face_keep, vertex_incl - vertex_keep, n_out_f,
                                         n_out_v)
    assert n_out_f == d.n_faces
    report.update(n_clusters=n_c, n_vertices=n_out_v, n_faces=n_out_f, n_clamped=int(totals[2]), n_faces_degenerate=d.n_degenerate,
                  n_faces_duplicate=n_f - d.n_degenerate - n_out_f, n_faces_flipped=int(totals[3]))
    return out_v, out_f, report


def _device_bounds(v):
    """The six bounding-box values, read back once (min / max propagate a NaN, so one non-finite coordinate shows here)."""
    box = torch.cat([v.amin(dim=0), v.amax(dim=0)]).tolist()
    return box[:3], box[3:]


def _device_clusters(v, grid):
    """-> cluster int64 [V] on the device (tests)."""
    return _DeviceGrid(v, v.new_zeros((0, 3), dtype=torch.int64), grid, False).cluster


def _device_simplify(v, f, target_faces=None, cell=None, resolution=None, regularisation=1e-3, events=None):
    """host_simplify on device tensors (float64 [V, 3], int64 [F, 3], contiguous) -> (vertices, faces: device tensors, report)."""
    from . import ops
    _check_sizes(target_faces, cell, resolution, regularisation)
    ops._hit('MeshSimplify')
    if target_faces is not None and f.shape[0] <= int(target_faces):
        return v, f, _unchanged_report(v.shape[0], f.shape[0])
    if v.shape[0] == 0:
        if f.shape[0]:
            raise ValueError('mesh: a face refers to a vertex outside 0 .. -1')
        return v, f, _empty_report(cell, resolution)
    lo, hi = _device_bounds(v)
    make_grid(lo, hi, cell, 1 if cell is None else None)      # (raises for a non-finite coordinate before anything is launched)
    probes, missed = [], False
    if target_faces is not None:
        def count(n):
            with Phase(events, 'probes'):
                d = _DeviceGrid(v, f, make_grid(lo, hi, None, n), False)
            return math.inf if d.n_clusters > MAX_CLUSTERS else d.n_faces
        resolution, probes, missed = choose_resolution(int(target_faces), count)
    out_v, out_f, report = _device_at(v, f, make_grid(lo, hi, cell, resolution), regularisation, None if cell is not None else int(resolution),
                                      probes, events)
    if missed:
        report['target_missed'] = True
    return out_v, out_f, report


# ------------------------------------------------------------------------------------------------ public surface
def simplify_mesh(mesh, target_faces=None, cell=None, resolution=None, regularisation=1e-3, device=None):
    """``mesh``: anything with .vertices and .faces, or a tuple (vertices, faces[, normals]) -> (Mesh, report); exactly one of
    ``target_faces``, ``cell`` and ``resolution``.  Device tensors, or ``device='cuda'``, take the device path (only the result is
    copied back); otherwise the host path.  Normals do not ride along (an untouched mesh keeps its own)."""
    vertices, faces, normals = mesh_parts(mesh)
    if on_device(vertices, device):
        v, f, _ = device_mesh(vertices, faces, None, device)
        v, f, report = _device_simplify(v, f, target_faces, cell, resolution, regularisation)
        v, f = v.cpu().numpy(), f.cpu().numpy()
    else:
        v, f, report = host_simplify(to_numpy(vertices), to_numpy(faces), target_faces, cell, resolution, regularisation)
    keep_normals = report.get('unchanged') and normals is not None
    return Mesh(v, f, vertex_normals=to_numpy(normals) if keep_normals else None), report
