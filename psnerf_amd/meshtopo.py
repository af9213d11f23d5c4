"""Mesh connectivity: the edge table of a triangle mesh and what follows from it -- a report that says whether the surface is closed
and consistently wound (and why not), the vertex rings, the per-vertex corner runs and vertex normals formed on the device.  Every
other mesh module treats the mesh as a bag of triangles; ``contains``, ``bake_occlusion`` and the volume IoU assume a closed,
consistently wound surface, and this is the module that can tell.  The reference has nothing of the kind (users take trimesh).

Two implementations of one definition, as in meshclean.py / meshsimplify.py:
  * CPU inputs -> the numpy functions below (``host_*``), float64 / int64; they are the definition, and what the device path is
    tested against, bit for bit (all but ``area`` and ``volume``, whose summation order is the device's own).
  * device tensors (or ``device='cuda'``) -> csrc/meshtopo.hip: key kernels, a stable torch.sort, run bounds, then a kernel that walks
    each run in a fixed order.  No floating-point atomics: two runs give the same bits.

Definition.
  Inputs.  vertices float64 [V, 3]; faces int64 [F, 3], an index outside 0 .. V - 1 raises ValueError.  A face with a repeated index is
    *degenerate*: legal, counted, and it contributes no half-edge.  Duplicated faces and unreferenced vertices are legal.
  Edge table.  Half-edge h = 3 f + k of a non-degenerate face runs from a = f[k] to b = f[(k + 1) % 3]; its undirected key is
    min(a, b) V + max(a, b) (63 bits: V <= 2^31 - 2), a degenerate face's three keys are a sentinel that sorts last.  A stable sort of
    the keys gives the unique edges ascending by key and every edge its run of half-edges in ascending h.  ``edges`` int64 [E, 2] =
    (lo, hi); ``count`` int32 [E] = the half-edges of the run; ``forward`` int32 [E] = those with a < b; ``halfedge_edge`` int64 [3 F] =
    the rank of each half-edge's edge, -1 for a sentinel; ``counters`` int64 [4] = boundary edges (count == 1), non-manifold edges
    (count > 2), inconsistent edges (count == 2 and forward != 1: the two faces run along the edge in the same direction) and
    degenerate faces; ``vertex_used`` / ``vertex_open`` bool [V] = the vertices of an edge / of an edge with count != 2.
  Report.  n_vertices, n_faces, n_faces_degenerate, n_vertices_unreferenced (named by no non-degenerate face), n_edges,
    n_boundary_edges, n_nonmanifold_edges, n_inconsistent_edges, euler = (V - unreferenced) - E + (F - degenerate),
    is_watertight = F - degenerate > 0 and no boundary and no non-manifold edge, is_oriented = is_watertight and no inconsistent edge,
    area = the sum of 0.5 |(b - a) x (c - a)| (meshcore.face_cross), volume = the sum of (a . (b x c)) / 6, signed, meaningful only
    when is_oriented.  Python ints, bools and floats.
  Rings.  The directed pairs (lo -> hi) and (hi -> lo) of the unique edges, keyed u V + w and sorted: ``ring_start`` int64 [V + 1],
    ``ring`` int64 [2 E]; each vertex's neighbours once and ascending, however many faces share the edge.
  Corner runs.  The corners laid out corner-major (j = k F + f), their vertex ids stably sorted: ``corner_start`` int64 [V + 1],
    ``corner`` int64 [3 F] (values j: k = j // F, f = j % F): per vertex its (corner, face) pairs in ascending (k, f), which is the order
    in which meshocclude.area_weighted_normals' three np.add.at passes add.  Corners of degenerate faces stay in the runs.
  Vertex normals.  Per vertex, from +0.0, over its corner run in order: += (b - a) x (c - a) of the face (weight='area'), or that
    divided by its length sqrt((nx nx + ny ny) + nz nz), a face without length adding nothing (weight='uniform'); then divided by
    the sum's length, formed the same way; zero where that is not > 0.  'area' is area_weighted_normals, bit for bit.  Angle
    weighting needs atan2, which is not bit-reproducible between numpy and the device: not built.
"""
import numpy as np
import torch

from .meshcore import Phase, device_mesh, face_cross, host_mesh, mesh_parts, on_device, to_numpy

SENTINEL = np.iinfo(np.int64).max
WEIGHTS = ('area', 'uniform')
COUNTERS = ('n_boundary_edges', 'n_nonmanifold_edges', 'n_inconsistent_edges', 'n_faces_degenerate')


def _check_weight(weight):
    if weight not in WEIGHTS:
        raise ValueError("vertex normals: weight=%r ('area' or 'uniform')" % (weight,))


# ------------------------------------------------------------------------------------------------ host path: the definition
def host_edge_keys(faces, n_vertices):
    """-> keys int64 [3 F], key of half-edge h = 3 f + k at position h."""
    n_v, f, _ = host_mesh(None, faces, n_vertices=n_vertices)
    a, b = f, np.roll(f, -1, axis=1)
    degenerate = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    keys = np.minimum(a, b) * n_v + np.maximum(a, b)
    return np.where(degenerate[:, None], SENTINEL, keys).reshape(-1).astype(np.int64)


def host_edges(faces, n_vertices):
    """-> {'edges', 'count', 'forward', 'halfedge_edge', 'counters', 'vertex_used', 'vertex_open'} (module docstring)."""
    n_v, f, _ = host_mesh(None, faces, n_vertices=n_vertices)
    keys = host_edge_keys(f, n_v)
    order = np.argsort(keys, kind='stable')
    s = keys[order]
    live = s != SENTINEL
    head = live.copy()
    head[1:] &= s[1:] != s[:-1]
    rank = np.cumsum(head) - 1
    n_e = int(head.sum())
    edge_key = s[head]
    edges = np.stack([edge_key // max(n_v, 1), edge_key % max(n_v, 1)], axis=1).astype(np.int64).reshape(-1, 2)
    is_forward = (f < np.roll(f, -1, axis=1)).reshape(-1)[order]
    count = np.bincount(rank[live], minlength=n_e).astype(np.int32)
    forward = np.bincount(rank[live], weights=is_forward[live], minlength=n_e).astype(np.int32)
    halfedge_edge = np.empty(keys.shape[0], dtype=np.int64)
    halfedge_edge[order] = np.where(live, rank, -1)
    counters = np.array([(count == 1).sum(), (count > 2).sum(), ((count == 2) & (forward != 1)).sum(), (~live).sum() // 3], dtype=np.int64)
    used, is_open = np.zeros(n_v, dtype=bool), np.zeros(n_v, dtype=bool)
    used[edges.reshape(-1)] = True
    is_open[edges[count != 2].reshape(-1)] = True
    return {'edges': edges, 'count': count, 'forward': forward, 'halfedge_edge': halfedge_edge, 'counters': counters, 'vertex_used': used,
            'vertex_open': is_open}


def host_measure_terms(vertices, faces):
    """-> (area terms float64 [F], volume terms float64 [F]): what ``area`` and ``volume`` are the sums of."""
    v, f, _ = host_mesh(vertices, faces)
    nx, ny, nz = face_cross(v, f)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    volume = ((a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]))
              + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])) / 6.0
    return area, volume


def _report(n_v, n_f, n_e, counters, n_used, area, volume):
    boundary, nonmanifold, inconsistent, degenerate = (int(x) for x in counters)
    watertight = n_f - degenerate > 0 and boundary == 0 and nonmanifold == 0
    return {'n_vertices': int(n_v), 'n_faces': int(n_f), 'n_faces_degenerate': degenerate, 'n_vertices_unreferenced': int(n_v - n_used),
            'n_edges': int(n_e), 'n_boundary_edges': boundary, 'n_nonmanifold_edges': nonmanifold, 'n_inconsistent_edges': inconsistent,
            'euler': int((n_v - (n_v - n_used)) - n_e + (n_f - degenerate)), 'is_watertight': bool(watertight),
            'is_oriented': bool(watertight and inconsistent == 0), 'area': float(area), 'volume': float(volume)}


def report_line(r):
    """One line of text for a report (the command-line tools)."""
    state = 'watertight and oriented' if r['is_oriented'] else ('watertight, NOT consistently oriented' if r['is_watertight'] else 'NOT watertight')
    return ('%s: %d vertices (%d unreferenced), %d edges, %d faces (%d degenerate), Euler characteristic %d; %d boundary, %d non-manifold, '
            '%d inconsistent edges; area %.6g, volume %.6g' % (state, r['n_vertices'], r['n_vertices_unreferenced'], r['n_edges'], r['n_faces'],
                                                              r['n_faces_degenerate'], r['euler'], r['n_boundary_edges'],
                                                              r['n_nonmanifold_edges'], r['n_inconsistent_edges'], r['area'], r['volume']))


def host_report(vertices, faces, table=None):
    """-> the report dict.  ``table``: host_edges of the same mesh, where the caller has it."""
    v, f, _ = host_mesh(vertices, faces)
    table = host_edges(f, v.shape[0]) if table is None else table
    area, volume = host_measure_terms(v, f)
    return _report(v.shape[0], f.shape[0], table['edges'].shape[0], table['counters'], int(table['vertex_used'].sum()), area.sum(), volume.sum())


def host_rings(edges, n_vertices):
    """edges int64 [E, 2] (unique, as host_edges returns them) -> (ring_start int64 [V + 1], ring int64 [2 E])."""
    n_v = int(n_vertices)
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    keys = np.sort(np.stack([e[:, 0] * n_v + e[:, 1], e[:, 1] * n_v + e[:, 0]], axis=1).reshape(-1))
    ring_start = np.searchsorted(keys // max(n_v, 1), np.arange(n_v + 1)).astype(np.int64)
    return ring_start, (keys % max(n_v, 1)).astype(np.int64)


def host_corner_runs(faces, n_vertices):
    """-> (corner_start int64 [V + 1], corner int64 [3 F] with values j = k F + f)."""
    n_v, f, _ = host_mesh(None, faces, n_vertices=n_vertices)
    ids = f.T.reshape(-1)
    corner = np.argsort(ids, kind='stable').astype(np.int64)
    return np.searchsorted(ids[corner], np.arange(n_v + 1)).astype(np.int64), corner


def host_vertex_normals(vertices, faces, weight='area'):
    """-> normals float64 [V, 3] (module docstring).  np.add.at adds one row after the other in index order, each sum from +0.0."""
    _check_weight(weight)
    v, f, _ = host_mesh(vertices, faces)
    m = np.zeros_like(v)
    with np.errstate(all='ignore'):
        cross = np.stack(face_cross(v, f), axis=1).reshape(-1, 3)
        if weight == 'uniform':
            size = np.sqrt((cross[:, 0] * cross[:, 0] + cross[:, 1] * cross[:, 1]) + cross[:, 2] * cross[:, 2])
            has = size > 0.0
            cross = np.where(has[:, None], cross / np.where(has, size, 1.0)[:, None], 0.0)   # (+0.0 added to a sum from +0.0: nothing)
        for c in range(3):
            np.add.at(m, f[:, c], cross)
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        long = length > 0.0
        return np.where(long[:, None], m / np.where(long, length, 1.0)[:, None], 0.0)


# ------------------------------------------------------------------------------------------------ device path
def _raise_status(status, n_vertices):
    from . import hip
    if status & hip.TOPO_E_INDEX:
        raise ValueError('mesh: a face refers to a vertex outside 0 .. %d' % (n_vertices - 1))


def _device_edges(f, n_vertices, events=None, out=None):
    """host_edges on a device tensor of faces -> the same dict of device tensors, and 'n_edges'.  One host read: the number of edges
    with the status word.  ``out``: the seven output buffers of hip.topo_edges (tests)."""
    from . import hip, ops
    ops._hit('MeshEdges')
    n_v, n_half = int(n_vertices), 3 * f.shape[0]
    dev = f.device
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with Phase(events, 'edge keys'):
        keys = hip.topo_edge_keys(f, n_v, status)
    with Phase(events, 'edge sort'):
        sorted_keys, order = torch.sort(keys, stable=True)
        head = sorted_keys != SENTINEL
        head[1:] &= sorted_keys[1:] != sorted_keys[:-1]
        rank_incl = torch.cumsum(head, dim=0, dtype=torch.int64)
        n_e = rank_incl[-1] if n_half else rank_incl.new_zeros(())
        row = torch.stack([status[0].to(torch.int64), n_e]).tolist()                   # the one host read
    _raise_status(int(row[0]), n_v)
    with Phase(events, 'edge table'):
        edges, count, forward, halfedge_edge, used, is_open, counters = hip.topo_edges(sorted_keys, order, rank_incl, f, n_v, int(row[1]), out)
    return {'edges': edges, 'count': count, 'forward': forward, 'halfedge_edge': halfedge_edge, 'counters': counters, 'vertex_used': used,
            'vertex_open': is_open, 'n_edges': int(row[1])}


def _device_rings(edges, n_vertices, events=None, out=None):
    """host_rings on a device edge table -> (ring_start, ring), device tensors.  No host read."""
    from . import hip
    with Phase(events, 'rings'):
        keys = torch.sort(hip.topo_ring_keys(edges, n_vertices)).values
        return hip.topo_runs(keys, max(int(n_vertices), 1), n_vertices, want_rem=True, out=out)


def _device_corner_runs(f, n_vertices, events=None, out_start=None, check=True):
    """host_corner_runs on device faces -> (corner_start, corner), device tensors.  ``check``: read the status word and raise for an
    index out of range (one host read); callers that have checked the faces already pass False."""
    from . import hip
    with Phase(events, 'corner runs'):
        status = torch.zeros(1, dtype=torch.int32, device=f.device)
        ids, corner = torch.sort(hip.topo_corner_keys(f, n_vertices, status), stable=True)
        corner_start, _ = hip.topo_runs(ids, 1, n_vertices, out=None if out_start is None else (out_start, None))
    if check:
        _raise_status(int(status.item()), int(n_vertices))
    return corner_start, corner


def _device_vertex_normals(v, f, weight='area', events=None, out=None, check=True):
    """host_vertex_normals on device tensors -> normals float64 [V, 3] on the device."""
    from . import hip, ops
    _check_weight(weight)
    ops._hit('MeshVertexNormals')
    corner_start, corner = _device_corner_runs(f, v.shape[0], events, check=check)
    with Phase(events, 'normals'):
        return hip.topo_vertex_normals(v, f, corner_start, corner, weight, out=out)


def _device_measures(v, f, out=None):
    from . import hip
    return hip.topo_measures(v, f, out=out)


def _device_report(v, f, table=None, events=None):
    """host_report on device tensors.  Host reads: the edge table's one, and one row of counters and sums."""
    table = _device_edges(f, v.shape[0], events) if table is None else table
    with Phase(events, 'report'):
        sums = _device_measures(v, f)
        counts = torch.cat([table['counters'], table['vertex_used'].sum(dtype=torch.int64).reshape(1)]).tolist()
        area, volume = sums.tolist()
    return _report(v.shape[0], f.shape[0], table['n_edges'], counts[:4], counts[4], area, volume)


# ------------------------------------------------------------------------------------------------ public surface
def edges(mesh, device=None):
    """``mesh``: anything with .vertices and .faces, or a tuple (vertices, faces) -> the edge table (module docstring) as a dict.
    Device tensors, or ``device='cuda'``, take the kernels (device tensors out; the two vertex flags uint8); otherwise numpy."""
    vertices, faces, _ = mesh_parts(mesh)
    if on_device(vertices, device):
        v, f, _ = device_mesh(vertices, faces, None, device)
        return _device_edges(f, v.shape[0])
    v, f, _ = host_mesh(to_numpy(vertices), to_numpy(faces))
    return host_edges(f, v.shape[0])


def mesh_report(mesh, device=None):
    """-> the report dict of Python ints, bools and floats, on either path."""
    vertices, faces, _ = mesh_parts(mesh)
    if on_device(vertices, device):
        v, f, _ = device_mesh(vertices, faces, None, device)
        return _device_report(v, f)
    return host_report(to_numpy(vertices), to_numpy(faces))


def rings(mesh, device=None):
    """-> (ring_start [V + 1], ring [2 E]): numpy on the host path, device tensors on the device path."""
    vertices, faces, _ = mesh_parts(mesh)
    if on_device(vertices, device):
        v, f, _ = device_mesh(vertices, faces, None, device)
        return _device_rings(_device_edges(f, v.shape[0])['edges'], v.shape[0])
    v, f, _ = host_mesh(to_numpy(vertices), to_numpy(faces))
    return host_rings(host_edges(f, v.shape[0])['edges'], v.shape[0])


def corner_runs(mesh, device=None):
    """-> (corner_start [V + 1], corner [3 F]): numpy on the host path, device tensors on the device path."""
    vertices, faces, _ = mesh_parts(mesh)
    if on_device(vertices, device):
        v, f, _ = device_mesh(vertices, faces, None, device)
        return _device_corner_runs(f, v.shape[0])
    v, f, _ = host_mesh(to_numpy(vertices), to_numpy(faces))
    return host_corner_runs(f, v.shape[0])


def vertex_normals(mesh, weight='area', device=None):
    """-> normals float64 [V, 3]: numpy on the host path, a device tensor on the device path (same bits)."""
    vertices, faces, _ = mesh_parts(mesh)
    if on_device(vertices, device):
        v, f, _ = device_mesh(vertices, faces, None, device)
        return _device_vertex_normals(v, f, weight)
    return host_vertex_normals(to_numpy(vertices), to_numpy(faces), weight)
