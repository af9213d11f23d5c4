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

from .stage1.extracting import Mesh


# ------------------------------------------------------------------------------------------------ host path: the definition
def _faces_array(faces, n_vertices):
    f = np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    n_v = int(n_vertices)
    if n_v < 0:
        raise ValueError('mesh: %d vertices' % n_v)
    if f.shape[0] and (f.min() < 0 or f.max() >= n_v):
        raise ValueError('mesh: a face refers to vertex %d of %d' % (int(f.max() if f.max() >= n_v else f.min()), n_v))
    return f, n_v


def host_components(faces, n_vertices, return_rounds=False):
    """labels int64 [V]: the smallest vertex index reachable from each vertex.  Rounds of (hook: the larger of the two labels an
    edge sees takes the smallest label offered to it; jump: labels[v] = labels[labels[v]] until nothing moves), repeated until no
    edge sees two labels.  labels[v] <= v throughout and every label is a fixed point after the jump, so the label a component ends
    with is its smallest index."""
    f, n_v = _faces_array(faces, n_vertices)
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


def _face_areas(v, f):
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    ab, ac = b - a, c - a
    nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    return 0.5 * np.sqrt(nx * nx + ny * ny + nz * nz)


def host_component_table(vertices, faces, labels):
    """-> {'label', 'n_vertices', 'n_faces' (int64 [C]), 'area' (float64 [C])}: one row per component that owns at least one face,
    ascending by label."""
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float64).reshape(-1, 3))
    f, n_v = _faces_array(faces, v.shape[0])
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    if labels.shape[0] != n_v:
        raise ValueError('mesh: %d labels for %d vertices' % (labels.shape[0], n_v))
    label, row = np.unique(labels[f[:, 0]], return_inverse=True)
    n_rows = label.shape[0]
    n_faces = np.bincount(row.reshape(-1), minlength=n_rows).astype(np.int64)
    area = np.bincount(row.reshape(-1), weights=_face_areas(v, f), minlength=n_rows).astype(np.float64)
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
    v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float64).reshape(-1, 3))
    f, n_v = _faces_array(faces, v.shape[0])
    normals = None if vertex_normals is None else np.asarray(vertex_normals).reshape(-1, 3)
    if normals is not None and normals.shape[0] != n_v:
        raise ValueError('mesh: %d normals for %d vertices' % (normals.shape[0], n_v))
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
def _to_device(vertices, faces, normals, device):
    """The mesh as contiguous device tensors (float64 [V, 3], int64 [F, 3], normals float32 / float64 [V, 3] or None)."""
    def tensor(x, dtype):
        if not torch.is_tensor(x):
            x = np.ascontiguousarray(np.asarray(x) if dtype is None else np.asarray(x, dtype=dtype))
            x = torch.from_numpy(x if x.flags.writeable else x.copy())
        return x
    v, f = tensor(vertices, np.float64), tensor(faces, np.int64)
    device = v.device if v.is_cuda else torch.device('cuda' if device is None else device)
    v = v.to(device=device, dtype=torch.float64).reshape(-1, 3).contiguous()
    f = f.to(device=device, dtype=torch.int64).reshape(-1, 3).contiguous()
    n = None
    if normals is not None:
        n = tensor(normals, None)
        if n.dtype not in (torch.float32, torch.float64):
            n = n.to(torch.float64)
        n = n.to(device).reshape(-1, 3).contiguous()
        if n.shape[0] != v.shape[0]:
            raise ValueError('mesh: %d normals for %d vertices' % (n.shape[0], v.shape[0]))
    return v, f, n


def _raise_status(status, n_vertices):
    from . import hip
    if status & hip.CC_E_INDEX:
        raise ValueError('mesh: a face refers to a vertex outside 0 .. %d' % (n_vertices - 1))
    if status & hip.CC_E_BOUND:
        raise RuntimeError('meshclean: the labelling kernel ran into its static loop bound (status %d)' % status)


def _device_table(v, f, events=None):
    """-> (labels int32 [V] on the device, table as numpy arrays).  One host read: the table rows, with the status word in front."""
    from . import hip, ops
    from .stage1.extracting import _Phase
    ops._hit('MeshComponents')
    n_v = v.shape[0]
    status = torch.empty(1, dtype=torch.int32, device=v.device)
    with _Phase(events, 'labelling'):
        labels = hip.cc_label(f, n_v, status)
    with _Phase(events, 'table'):
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
    from .stage1.extracting import _Phase
    labels, table = _device_table(v, f, events)
    kept = select(table, keep, min_faces, by)
    with _Phase(events, 'compaction'):
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


def _on_device(vertices, device):
    if device is not None:
        return torch.device(device).type == 'cuda'
    return torch.is_tensor(vertices) and vertices.is_cuda


def _numpy(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else x


# ------------------------------------------------------------------------------------------------ public surface
def components(vertices, faces, device=None):
    """-> (labels, table).  Device tensors, or ``device='cuda'``, take the device path (labels: int32 device tensor); otherwise the
    host path (labels: int64 numpy array).  The table is numpy arrays on both paths."""
    if _on_device(vertices, device):
        v, f, _ = _to_device(vertices, faces, None, device)
        return _device_table(v, f)
    v, f = _numpy(vertices), _numpy(faces)
    labels = host_components(f, np.asarray(v).reshape(-1, 3).shape[0])
    return labels, host_component_table(v, f, labels)


def clean_mesh(mesh, keep=1, min_faces=0, by='faces', device=None):
    """``mesh``: anything with .vertices and .faces (and optionally .vertex_normals), or a tuple (vertices, faces[, normals]) ->
    (Mesh, report): the ``keep`` largest components (None: all) among those with at least ``min_faces`` faces.  Device tensors, or
    ``device='cuda'``, take the device path (only the cleaned mesh is copied back); otherwise the host path."""
    if isinstance(mesh, (tuple, list)):
        vertices, faces = mesh[0], mesh[1]
        normals = mesh[2] if len(mesh) > 2 else None
    else:
        vertices, faces, normals = mesh.vertices, mesh.faces, getattr(mesh, 'vertex_normals', None)
    if _on_device(vertices, device):
        v, f, n = _to_device(vertices, faces, normals, device)
        v, f, n, report = _device_clean(v, f, n, keep, min_faces, by)
        return Mesh(v.cpu().numpy(), f.cpu().numpy(), vertex_normals=None if n is None else n.cpu().numpy()), report
    v, f, n, report = host_clean(_numpy(vertices), _numpy(faces), None if normals is None else _numpy(normals), keep, min_faces, by)
    return Mesh(v, f, vertex_normals=n), report
