"""Mesh clean-up: connected components of a triangle mesh, per-component statistics, selection and compaction -- separating the
object from the detached floaters and closed inner shells that marching cubes also returns for an occupancy field trained from few
views.  ``get_chamfer_dist`` samples the predicted mesh by area, so every such piece adds to the pred -> gt term.  The reference has
no such step (its only answer is ``--clip``, stage1/model/extracting.py:130-132, which cuts everything below z = -1); users of the
pipeline take trimesh's ``split()`` on the host and keep the largest piece.  trimesh is not needed here.

Two implementations of one definition, as in meshdist.py:
  * CPU inputs -> the numpy functions below (``host_*``), float64 / int64; they are the definition, and what the device path is
    tested against.
  * device tensors (or ``device='cuda'``) -> csrc/meshclean.hip: psn_cc_label (a lock-free union-find in one pass over the faces and a
    flatten launch), psn_cc_stats (one pass over the vertices, one over the faces), then the small per-component table on the host
    (``select`` is the same function for both paths), psn_cc_flag, two torch.cumsum scans and psn_cc_compact.  Two host reads: the
    table (which carries the kernels' status word) and the two totals of the scans.

Definition.  Two vertices are adjacent when one face names both; labels[v] = the smallest vertex index reachable from v, so an
unreferenced vertex keeps its own index.  Duplicated faces and faces with a repeated index are legal; an index outside 0 .. V - 1
raises ValueError.  A face belongs to the component of its first index.  The table has one row per component that owns at least one
face, ascending by label: label, n_vertices, n_faces, area (the sum of 0.5 |(b - a) x (c - a)| in float64).  ``select`` first drops
the components with fewer than ``min_faces`` faces, then (``keep = K``) takes the K largest by face count or area, ties to the smaller
label.  Cleaning keeps the faces of the selected components in their original order and exactly the vertices a kept face names
(unreferenced vertices always go), in their original order with their bits untouched; faces are re-indexed, normals ride along.
"""
import numpy as np
import torch

from .meshcore import Mesh, Phase, device_mesh, face_areas, host_mesh, mesh_parts, on_device, to_numpy


# ------------------------------------------------------------------------------------------------ host path: the definition
def host_components(faces, n_vertices, return_rounds=False):
    """labels int64 [V]: the smallest vertex index reachable from each vertex.  Rounds of (hook: the larger of the two labels an
    edge sees takes the smallest label offered to it; jump: labels[v] = labels[labels[v]] until nothing moves), repeated until no
    edge sees two labels.  labels[v] <= v throughout and every label is a fixed point after the jump, so the label a component ends
    with is its smallest index."""
    n_v, f, _ = host_mesh(None, faces, n_vertices=n_vertices)
    labels = np.arange(n_v, dtype=np.int64)
    e0, e1 = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
    rounds = 0
    while True:
        a, b = labels[e0], labels[e1]
        differ = a != b
        if not differ.any():
            break
        lo, hi = np.minimum(a, b)[differ], np.maximum(a, b)[differ]
        order = np.lexsort((lo, hi))                       # per larger label, the smallest offer first
        hi, lo = hi[order], lo[order]
        first = np.ones(hi.shape[0], dtype=bool)
        first[1:] = hi[1:] != hi[:-1]
        labels[hi[first]] = np.minimum(labels[hi[first]], lo[first])
        while True:
            jumped = labels[labels]
            if np.array_equal(jumped, labels):
                break
            labels = jumped
        rounds += 1
    return (labels, rounds) if return_rounds else labels


def host_component_table(vertices, faces, labels):
    """-> {'label', 'n_vertices', 'n_faces' (int64 [C]), 'area' (float64 [C])}: one row per component that owns at least one face,
    ascending by label."""
    v, f, _ = host_mesh(vertices, faces)
    n_v = v.shape[0]
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    if labels.shape[0] != n_v:
        raise ValueError('mesh: %d labels for %d vertices' % (labels.shape[0], n_v))
    label, row = np.unique(labels[f[:, 0]], return_inverse=True)
    n_rows = label.shape[0]
    n_faces = np.bincount(row.reshape(-1), minlength=n_rows).astype(np.int64)
    area = np.bincount(row.reshape(-1), weights=face_areas(v, f), minlength=n_rows).astype(np.float64)
    at = np.minimum(np.searchsorted(label, labels), max(n_rows - 1, 0))
    owned = label[at] == labels if n_rows else np.zeros(n_v, dtype=bool)
    n_vertices = np.bincount(at[owned], minlength=n_rows).astype(np.int64)
    return {'label': label.astype(np.int64), 'n_vertices': n_vertices, 'n_faces': n_faces, 'area': area}


def select(table, keep=None, min_faces=0, by='faces'):
    """The labels of the components to keep, ascending: drop those with n_faces < min_faces, then (keep = K >= 1) take the K largest by
    ``by`` ('faces' or 'area'), ties to the smaller label; keep=None keeps all that pass min_faces."""
    if by not in ('faces', 'area'):
        raise ValueError("select: by=%r ('faces' or 'area')" % (by,))
    if keep is not None and int(keep) < 1:
        raise ValueError('select: keep=%r (None, or at least 1)' % (keep,))
    rows = np.nonzero(table['n_faces'] >= int(min_faces))[0]
    if keep is not None:
        size = table['n_faces' if by == 'faces' else 'area'][rows]
        order = np.lexsort((table['label'][rows], -size))   # descending by size, then ascending by label
        rows = rows[order[:int(keep)]]
    return np.sort(table['label'][rows]).astype(np.int64)


def _report(table, kept, n_faces, n_vertices, n_out_faces, n_out_vertices):
    return {'n_components': int(table['label'].shape[0]), 'n_kept': int(len(kept)), 'n_faces_removed': int(n_faces - n_out_faces),
            'n_vertices_removed': int(n_vertices - n_out_vertices), 'table': table}


def host_clean(vertices, faces, vertex_normals=None, keep=None, min_faces=0, by='faces'):
    """-> (vertices, faces, normals or None, report).  report: n_components (rows of the table: the components that own a face),
    n_kept, n_faces_removed, n_vertices_removed (unreferenced vertices included) and the table."""
    v, f, normals = host_mesh(vertices, faces, vertex_normals)
    n_v = v.shape[0]
    labels = host_components(f, n_v)
    table = host_component_table(v, f, labels)
    kept = select(table, keep, min_faces, by)
    out_f = f[np.isin(labels[f[:, 0]], kept)]
    vertex_keep = np.zeros(n_v, dtype=bool)
    vertex_keep[out_f.reshape(-1)] = True
    new_index = np.cumsum(vertex_keep) - 1
    out_v = v[vertex_keep]
    return out_v, new_index[out_f].astype(np.int64).reshape(-1, 3), None if normals is None else normals[vertex_keep], \
        _report(table, kept, f.shape[0], n_v, out_f.shape[0], out_v.shape[0])


# ------------------------------------------------------------------------------------------------ device path
def _raise_status(status, n_vertices):
    from . import hip
    if status & hip.CC_E_INDEX:
        raise ValueError('mesh: a face refers to a vertex outside 0 .. %d' % (n_vertices - 1))
    if status & hip.CC_E_BOUND:
        raise RuntimeError('meshclean: the labelling kernel ran into its static loop bound (status %d)' % status)


def _device_table(v, f, events=None):
    """-> (labels int32 [V] on the device, table as numpy arrays).  One host read: the table rows, with the status word in front."""
    from . import hip, ops
    ops._hit('MeshComponents')
    n_v = v.shape[0]
    status = torch.empty(1, dtype=torch.int32, device=v.device)
    with Phase(events, 'labelling'):
        labels = hip.cc_label(f, n_v, status)
    with Phase(events, 'table'):
        counts, area = hip.cc_stats(v, f, labels, status)
        rows = torch.nonzero(counts[1]).reshape(-1)
        head = torch.cat([status.to(torch.int64), rows, counts[0][rows], counts[1][rows]]).cpu().numpy()
        area = area[rows].cpu().numpy()
    _raise_status(int(head[0]), n_v)
    n = rows.shape[0]
    table = {'label': head[1:1 + n].copy(), 'n_vertices': head[1 + n:1 + 2 * n].copy(), 'n_faces': head[1 + 2 * n:1 + 3 * n].copy(),
             'area': area}
    return labels, table


def _device_clean(v, f, normals, keep, min_faces, by, events=None):
    """host_clean on device tensors -> (vertices, faces, normals or None: device tensors, report)."""
    from . import hip
    labels, table = _device_table(v, f, events)
    kept = select(table, keep, min_faces, by)
    with Phase(events, 'compaction'):
        keep_label = torch.zeros(v.shape[0], dtype=torch.uint8, device=v.device)
        if len(kept):
            keep_label[torch.from_numpy(kept).to(v.device)] = 1
        face_keep, vertex_keep = hip.cc_flag(f, labels, keep_label)
        face_incl, vertex_incl = torch.cumsum(face_keep, dim=0, dtype=torch.int64), torch.cumsum(vertex_keep, dim=0, dtype=torch.int64)
        totals = torch.stack([face_incl[-1] if f.shape[0] else face_incl.new_zeros(()),
                              vertex_incl[-1] if v.shape[0] else vertex_incl.new_zeros(())]).tolist()
        n_out_f, n_out_v = int(totals[0]), int(totals[1])
        out_v, out_f, out_n = hip.cc_compact(v, f, normals, face_keep, vertex_keep, face_incl - face_keep, vertex_incl - vertex_keep,
                                             n_out_f, n_out_v)
    return out_v, out_f, out_n, _report(table, kept, f.shape[0], v.shape[0], n_out_f, n_out_v)


# ------------------------------------------------------------------------------------------------ public surface
def components(vertices, faces, device=None):
    """-> (labels, table).  Device tensors, or ``device='cuda'``, take the device path (labels: int32 device tensor); otherwise the
    host path (labels: int64 numpy array).  The table is numpy arrays on both paths."""
    if on_device(vertices, device):
        v, f, _ = device_mesh(vertices, faces, None, device)
        return _device_table(v, f)
    v, f = to_numpy(vertices), to_numpy(faces)
    labels = host_components(f, np.asarray(v).reshape(-1, 3).shape[0])
    return labels, host_component_table(v, f, labels)


def clean_mesh(mesh, keep=1, min_faces=0, by='faces', device=None):
    """``mesh``: anything with .vertices and .faces (and optionally .vertex_normals), or a tuple (vertices, faces[, normals]) ->
    (Mesh, report): the ``keep`` largest components (None: all) among those with at least ``min_faces`` faces.  Device tensors, or
    ``device='cuda'``, take the device path (only the cleaned mesh is copied back); otherwise the host path."""
    vertices, faces, normals = mesh_parts(mesh)
    if on_device(vertices, device):
        v, f, n = device_mesh(vertices, faces, normals, device)
        v, f, n, report = _device_clean(v, f, n, keep, min_faces, by)
        return Mesh(v.cpu().numpy(), f.cpu().numpy(), vertex_normals=to_numpy(n)), report
    v, f, n, report = host_clean(to_numpy(vertices), to_numpy(faces), to_numpy(normals), keep, min_faces, by)
    return Mesh(v, f, vertex_normals=n), report
