"""What every mesh module shares: the ``Mesh`` container with its writer and reader, the unpacking of the forms a mesh is handed
over in, the one host validator and the one device mover of a (vertices, faces[, normals]) triple, the triangle cross product and
the HIP-event bracket of the measurement runs.  Nothing here imports from ``stage1`` or from another ``mesh*`` module.

Conventions.  vertices float64 [V, 3], faces int64 [F, 3], both contiguous; a face index outside 0 .. V - 1 is the caller's error.
On the host it raises ValueError here; on the device the kernels report it in their status word (or the caller folds the range
into a host read it makes anyway), so the mover spends no host read of its own.
"""
import os

import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ the container and its writer
class Mesh(object):
    """What the extraction returns: vertices float64 [V, 3], faces int64 [F, 3], optional vertex normals.  Stands in for
    trimesh.Trimesh(vertices, faces, vertex_normals=normals, process=False) as far as extract_mesh.py uses it."""

    def __init__(self, vertices, faces, vertex_normals=None):
        self.vertices = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
        self.vertex_normals = None if vertex_normals is None else np.asarray(vertex_normals).reshape(-1, 3)

    @property
    def is_empty(self):
        return self.vertices.shape[0] == 0

    def export(self, path):
        ext = os.path.splitext(path)[1].lower()
        if ext == '.obj':
            with open(path, 'w') as f:
                for v in self.vertices:
                    f.write('v %.17g %.17g %.17g\n' % tuple(v))
                if self.vertex_normals is not None:
                    for v in self.vertex_normals:
                        f.write('vn %.9g %.9g %.9g\n' % tuple(v))
                for t in self.faces + 1:
                    if self.vertex_normals is not None:
                        f.write('f %d//%d %d//%d %d//%d\n' % (t[0], t[0], t[1], t[1], t[2], t[2]))
                    else:
                        f.write('f %d %d %d\n' % tuple(t))
        elif ext == '.ply':
            props = ['x', 'y', 'z'] + (['nx', 'ny', 'nz'] if self.vertex_normals is not None else [])
            head = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % self.vertices.shape[0]]
            head += ['property float %s' % p for p in props]
            head += ['element face %d' % self.faces.shape[0], 'property list uchar int vertex_indices', 'end_header']
            vert = self.vertices.astype('<f4')
            if self.vertex_normals is not None:
                vert = np.concatenate([vert, self.vertex_normals.astype('<f4')], axis=1)
            rec = np.empty(self.faces.shape[0], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
            rec['n'] = 3
            rec['i'] = self.faces
            with open(path, 'wb') as f:
                f.write(('\n'.join(head) + '\n').encode('ascii'))
                f.write(np.ascontiguousarray(vert).tobytes())
                f.write(rec.tobytes())
        else:
            raise NotImplementedError('Mesh.export: %r (supported: .obj, .ply)' % ext)
        return path


# ------------------------------------------------------------------------------------------------ the reader
_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2', 'uint16': 'u2',
              'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4', 'double': 'f8', 'float64': 'f8'}


def _fan(polygons):
    """Polygons (lists of vertex indices) -> triangles, a fan around the first corner."""
    out = []
    for p in polygons:
        if len(p) < 3:
            raise ValueError('a face with %d corners' % len(p))
        out.extend((p[0], p[k], p[k + 1]) for k in range(1, len(p) - 1))
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)


def _load_obj(path):
    vertices, normals, polygons = [], [], []
    with open(path, 'r') as fh:
        for line in fh:
            tok = line.split()
            if not tok or tok[0].startswith('#'):
                continue
            if tok[0] == 'v':
                vertices.append([float(x) for x in tok[1:4]])
            elif tok[0] == 'vn':
                normals.append([float(x) for x in tok[1:4]])
            elif tok[0] == 'f':
                idx = [int(t.split('/')[0]) for t in tok[1:]]
                polygons.append([i - 1 if i > 0 else len(vertices) + i for i in idx])   # (negative: relative to the end)
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    vn = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    return Mesh(v, _fan(polygons), vertex_normals=vn if len(vn) == len(v) and len(v) else None)


def _load_ply(path):
    with open(path, 'rb') as fh:
        data = fh.read()
    end = data.find(b'end_header')
    if not data.startswith(b'ply') or end < 0:
        raise ValueError('no PLY header')
    body = data.index(b'\n', end) + 1
    fmt, elements = None, []
    for line in data[:end].decode('ascii', 'replace').splitlines()[1:]:
        tok = line.split()
        if not tok or tok[0] in ('comment', 'obj_info'):
            continue
        if tok[0] == 'format':
            fmt = tok[1]
        elif tok[0] == 'element':
            elements.append((tok[1], int(tok[2]), []))
        elif tok[0] == 'property':
            if not elements:
                raise ValueError('a property before any element')
            elements[-1][2].append((tok[-1], (tok[2], tok[3])) if tok[1] == 'list' else (tok[-1], tok[1]))
    if fmt not in ('ascii', 'binary_little_endian'):
        raise ValueError('format %r (supported: ascii, binary_little_endian)' % fmt)
    vertices, polygons, normals = None, [], None
    tokens, tpos = (data[body:].split(), 0) if fmt == 'ascii' else (None, 0)
    pos = body
    for name, count, props in elements:
        has_list = any(isinstance(t, tuple) for _, t in props)
        if any((t if not isinstance(t, tuple) else t[0]) not in _PLY_TYPES or (isinstance(t, tuple) and t[1] not in _PLY_TYPES)
               for _, t in props):
            raise ValueError('element %s: unknown property type' % name)
        if not has_list:
            if fmt == 'ascii':
                rows = np.asarray(tokens[tpos:tpos + count * len(props)], dtype=np.float64).reshape(count, len(props))
                tpos += count * len(props)
                cols = dict((p, rows[:, i]) for i, (p, _) in enumerate(props))
            else:
                dt = np.dtype([(p, '<' + _PLY_TYPES[t]) for p, t in props])
                rec = np.frombuffer(data, dtype=dt, count=count, offset=pos)
                pos += count * dt.itemsize
                cols = dict((p, rec[p]) for p, _ in props)
            if name == 'vertex':
                vertices = np.stack([cols['x'], cols['y'], cols['z']], axis=1).astype(np.float64)
                if all(k in cols for k in ('nx', 'ny', 'nz')):
                    normals = np.stack([cols['nx'], cols['ny'], cols['nz']], axis=1).astype(np.float64)
            continue
        is_face = name == 'face'
        if fmt == 'binary_little_endian' and len(props) == 1 and count > 0:
            # the common case (and what Mesh.export writes): one list property, every face with as many corners as the first
            ct, it = _PLY_TYPES[props[0][1][0]], _PLY_TYPES[props[0][1][1]]
            k = int(np.frombuffer(data, dtype='<' + ct, count=1, offset=pos)[0])
            dt = np.dtype([('n', '<' + ct), ('i', '<' + it, (k,))])
            if pos + count * dt.itemsize <= len(data):
                rec = np.frombuffer(data, dtype=dt, count=count, offset=pos)
                if (rec['n'] == k).all():
                    pos += count * dt.itemsize
                    if is_face:
                        polygons = rec['i'].astype(np.int64).reshape(count, k)
                    continue
        rows = []
        for _ in range(count):
            row = None
            for pname, t in props:
                if isinstance(t, tuple):
                    if fmt == 'ascii':
                        k = int(tokens[tpos])
                        idx = [int(x) for x in tokens[tpos + 1:tpos + 1 + k]]
                        tpos += 1 + k
                    else:
                        ct, it = np.dtype('<' + _PLY_TYPES[t[0]]), np.dtype('<' + _PLY_TYPES[t[1]])
                        k = int(np.frombuffer(data, dtype=ct, count=1, offset=pos)[0])
                        idx = np.frombuffer(data, dtype=it, count=k, offset=pos + ct.itemsize).astype(np.int64).tolist()
                        pos += ct.itemsize + k * it.itemsize
                    if pname in ('vertex_indices', 'vertex_index'):
                        row = idx
                elif fmt == 'ascii':
                    tpos += 1
                else:
                    pos += np.dtype(_PLY_TYPES[t]).itemsize
            if is_face and row is not None:
                rows.append(row)
        if is_face:
            polygons = rows
    if vertices is None:
        raise ValueError('no vertex element')
    faces = _fan([list(p) for p in polygons]) if len(polygons) else np.zeros((0, 3), dtype=np.int64)
    return Mesh(vertices, faces, vertex_normals=normals)


def load_mesh(path):
    """Read what ``Mesh.export`` writes, and ground-truth scans of the same kinds: Wavefront .obj (v / vn / f with a, a/b, a/b/c or
    a//n corners) and .ply (ascii or binary little-endian).  Polygons with more than three corners are fan-triangulated.
    Anything else raises a ValueError that names the file."""
    ext = os.path.splitext(path)[1].lower()
    if ext not in ('.obj', '.ply'):
        raise ValueError('load_mesh: %s: unsupported extension %r (supported: .obj, .ply)' % (path, ext))
    try:
        mesh = _load_obj(path) if ext == '.obj' else _load_ply(path)
    except (ValueError, KeyError, IndexError) as e:
        raise ValueError('load_mesh: %s: %s' % (path, e))
    if len(mesh.faces) and (mesh.faces.min() < 0 or mesh.faces.max() >= len(mesh.vertices)):
        raise ValueError('load_mesh: %s: a face refers to a vertex that does not exist' % path)
    return mesh


# ------------------------------------------------------------------------------------------------ the forms a mesh comes in
def mesh_parts(mesh):
    """A Mesh, anything with .vertices / .faces (/ .vertex_normals), or a (vertices, faces[, normals]) tuple ->
    (vertices, faces, normals or None), as they are."""
    if isinstance(mesh, (tuple, list)):
        return mesh[0], mesh[1], (mesh[2] if len(mesh) > 2 else None)
    return mesh.vertices, mesh.faces, getattr(mesh, 'vertex_normals', None)


def to_numpy(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else x


def on_device(vertices, device=None):
    """Does this call take the device path: ``device`` decides where it is given, otherwise where the vertices are."""
    if device is not None:
        return torch.device(device).type == 'cuda'
    return torch.is_tensor(vertices) and vertices.is_cuda


def host_mesh(vertices, faces, normals=None, n_vertices=None, prefix='mesh', finite=False, widen_normals=False):
    """The one host validator -> (vertices float64 [V, 3] contiguous, faces int64 [F, 3] contiguous, normals [V, 3] or None).
    ``vertices`` = None with ``n_vertices`` = V: only the faces are checked, against that count, and V is returned in the vertices'
    place.  ``prefix`` opens every message.  ``finite``: a coordinate that is not finite raises; a string is the prefix of that one
    message.  ``widen_normals``: the normals become float64 (False: their bits stay untouched).  Every error is a ValueError."""
    if vertices is None:
        v, n_v = None, int(n_vertices)
        if n_v < 0:
            raise ValueError('%s: %d vertices' % (prefix, n_v))
    else:
        v = np.ascontiguousarray(np.asarray(vertices, dtype=np.float64).reshape(-1, 3))
        n_v = v.shape[0]
        if finite and not np.isfinite(v).all():
            raise ValueError('%s: a vertex coordinate is not finite' % (finite if isinstance(finite, str) else prefix))
    f = np.ascontiguousarray(np.asarray(faces, dtype=np.int64).reshape(-1, 3))
    if f.shape[0] and (f.min() < 0 or f.max() >= n_v):
        raise ValueError('%s: a face refers to vertex %d of %d' % (prefix, int(f.max() if f.max() >= n_v else f.min()), n_v))
    if normals is not None:
        normals = np.ascontiguousarray(np.asarray(normals, dtype=np.float64 if widen_normals else None).reshape(-1, 3))
        if normals.shape[0] != n_v:
            raise ValueError('%s: %d normals for %d vertices' % (prefix, normals.shape[0], n_v))
    return (n_v if v is None else v), f, normals


def device_mesh(vertices, faces, normals=None, device=None, prefix='mesh', widen_normals=False):
    """The one device mover -> (vertices float64 [V, 3], faces int64 [F, 3], normals [V, 3] or None), contiguous device tensors, from
    numpy arrays (read-only ones are copied first), CPU tensors or device tensors; what is already in place is returned as it is.
    Vertices on a device stay there; otherwise everything goes to ``device`` (default 'cuda').  Normals keep float32 / float64
    (anything else, and everything with ``widen_normals``, becomes float64); their count is checked against V.  No host read."""
    def tensor(x, dtype):
        if not torch.is_tensor(x):
            x = np.ascontiguousarray(np.asarray(x, dtype=dtype))
            x = torch.from_numpy(x if x.flags.writeable else x.copy())
        return x
    v, f = tensor(vertices, np.float64), tensor(faces, np.int64)
    device = v.device if v.is_cuda else torch.device('cuda' if device is None else device)
    v = v.to(device=device, dtype=torch.float64).reshape(-1, 3).contiguous()
    f = f.to(device=device, dtype=torch.int64).reshape(-1, 3).contiguous()
    if normals is not None:
        normals = tensor(normals, None)
        wide = widen_normals or normals.dtype not in (torch.float32, torch.float64)
        normals = normals.to(device=device, dtype=torch.float64 if wide else normals.dtype).reshape(-1, 3).contiguous()
        if normals.shape[0] != v.shape[0]:
            raise ValueError('%s: %d normals for %d vertices' % (prefix, normals.shape[0], v.shape[0]))
    return v, f, normals


# ------------------------------------------------------------------------------------------------ the triangle cross product
def face_cross(v, f):
    """(b - a) x (c - a) of the faces f of vertices v, unnormalised -> (nx, ny, nz); numpy arrays or torch tensors alike.  The
    operation order is part of the definitions built on it (host and device results are compared bit for bit)."""
    a = v[f[:, 0]]
    ab, ac = v[f[:, 1]] - a, v[f[:, 2]] - a
    nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    return nx, ny, nz


def face_areas(v, f):
    nx, ny, nz = face_cross(v, f)
    return 0.5 * (torch if torch.is_tensor(nx) else np).sqrt(nx * nx + ny * ny + nz * nz)


# ------------------------------------------------------------------------------------------------ measurement
class Phase(object):
    """``with Phase(log, name):`` brackets device work with HIP events when ``log`` is a list, to which (name, start event,
    end event) is appended; with ``log`` = None it does nothing."""

    def __init__(self, log, name):
        self.log, self.name = log, name

    def __enter__(self):
        if self.log is not None:
            self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if self.log is not None and exc[0] is None:
            self.e1.record()
            self.log.append((self.name, self.e0, self.e1))
        return False
