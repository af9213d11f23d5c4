"""Occlusion of surface points by the mesh itself: ambient occlusion, bent normals and one visibility bit per direction, per row of
(point, normal).  The reference has nothing of the kind; what this shows is the EXPORTED ASSET -- binary occlusion by the mesh, not the
network's transmittance (the caveat of meshrender.mesh_light_visibility applies).

Two implementations of one definition, as in every mesh module:
  * numpy inputs -> ``host_occlusion_rows`` below, float64 with every operation order written out: it IS the definition.
  * a ``MeshIndex`` / device tensors -> csrc/meshocclude.hip (psn_occlusion_rows), which forms each row's rays in registers in that
    order and walks them with psn_ray_cast's own any-hit walk: every output equal bit for bit.

Definition.  ``hemisphere_table(K)``: K cosine-weighted unit directions about +z, so that a plain count estimates the cosine-weighted
occlusion integral: u = (k + 0.5) / K, phi = 2 pi ((k g) mod 1) with g = (sqrt 5 - 1) / 2, r = sqrt u, row k = (r cos phi, r sin phi,
sqrt(1 - u)).  It is computed on the host and handed to the kernel as data.
``frame(n)``: the branchless orthonormal basis of Duff et al. (JCGT 2017): s = 1 if n_z >= 0 else -1, a = -1 / (s + n_z),
q = (n_x n_y) a, t = (1 + (s (n_x n_x)) a, s q, (-s) n_x), b = (q, s + (n_y n_y) a, -n_y).
A row: a row whose point or normal has a non-finite component, or whose normal is zero, casts nothing (hits -1, ao NaN, bent 0,
visible 0, words 0).  Origin o = p + bias n (the three products, then the three sums).  Direction k, (x, y, z) = table[k]:
local: d = (x t + y b) + z n per component, every direction cast; world: d = table[k], cast iff (n0 d0 + n1 d1) + n2 d2 > 0.
Blocked = meshdist.host_ray_cast(v, f, o, d, 0.0, t_max, any_hit=True) reports a hit.  hits / visible = the cast directions that are /
are not blocked; ao = 1 - hits / K' (K' = the number cast; 1 when K' = 0); bent = the sum over k in index order of the unblocked cast
d, divided by sqrt((m0 m0 + m1 m1) + m2 m2), zero where that is not > 0; words: bit k % 32 of word k // 32 <=> k cast and not blocked."""
import numpy as np
import torch

from . import meshdist as md
from .meshcore import face_cross, mesh_parts, to_numpy

MAX_DIRS = 1024              # PSN_OCC_MAX_DIRS: the device's limit; the definition has none
BIAS_SCALE = 1e-4            # bias=None: this times the bounding-box diagonal of the mesh


# ------------------------------------------------------------------------------------------------ host path: the definition
def hemisphere_table(K):
    """K cosine-weighted unit directions about +z (module docstring) -> float64 [K, 3]."""
    K = int(K)
    if K < 1:
        raise ValueError('hemisphere_table: K = %d' % K)
    k = np.arange(K, dtype=np.float64)
    u = (k + 0.5) / K
    phi = 2.0 * np.pi * np.mod(k * ((np.sqrt(5.0) - 1.0) / 2.0), 1.0)
    r = np.sqrt(u)
    return np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(1.0 - u)], axis=1)


def frame(n):
    """The basis (t, b) of Duff et al. about the unit normals n [..., 3] -> (t [..., 3], b [..., 3]), float64."""
    n = np.asarray(n, dtype=np.float64)
    nx, ny, nz = n[..., 0], n[..., 1], n[..., 2]
    with np.errstate(all='ignore'):
        s = np.where(nz >= 0.0, 1.0, -1.0)
        a = -1.0 / (s + nz)
        q = (nx * ny) * a
        t = np.stack([1.0 + (s * (nx * nx)) * a, s * q, (-s) * nx], axis=-1)
        b = np.stack([q, s + (ny * ny) * a, -ny], axis=-1)
    return t, b


def _check(table, bias, t_max, what):
    table = np.ascontiguousarray(np.asarray(table, dtype=np.float64))
    if table.ndim != 2 or table.shape[1] != 3 or table.shape[0] < 1:
        raise ValueError('%s: a direction table [K >= 1, 3] expected, got %s' % (what, table.shape))
    if not np.isfinite(bias):
        raise ValueError('%s: bias = %r is not finite' % (what, bias))
    if not t_max >= 0.0:
        raise ValueError('%s: t_max = %r < 0 (or a NaN)' % (what, t_max))
    return table


def host_occlusion_rows(vertices, faces, points, normals, table, local=True, bias=0.0, t_max=np.inf, bits=False):
    """The definition (module docstring): points / normals [R, 3], table [K, 3] -> (hits int32 [R], visible int32 [R], ao float64 [R],
    bent float64 [R, 3], words int32 [R, ceil(K / 32)] or None)."""
    table = _check(table, bias, t_max, 'host_occlusion_rows')
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    if p.shape != n.shape:
        raise ValueError('host_occlusion_rows: %d points and %d normals' % (p.shape[0], n.shape[0]))
    R, K = p.shape[0], table.shape[0]
    ok = np.isfinite(p).all(axis=1) & np.isfinite(n).all(axis=1) & (n != 0.0).any(axis=1)
    rows = np.nonzero(ok)[0]
    p, n = p[rows], n[rows]
    with np.errstate(all='ignore'):
        o = p + bias * n
        x, y, z = (table[None, :, i, None] for i in range(3))                          # [1, K, 1]
        if local:
            t, b = frame(n)
            d = (x * t[:, None, :] + y * b[:, None, :]) + z * n[:, None, :]            # [r, K, 3]
            cast = np.ones((len(rows), K), dtype=bool)
        else:
            d = np.broadcast_to(table[None], (len(rows), K, 3))
            cast = (n[:, None, 0] * d[..., 0] + n[:, None, 1] * d[..., 1]) + n[:, None, 2] * d[..., 2] > 0.0
        blocked = np.zeros((len(rows), K), dtype=bool)
        if cast.any():
            ri, ki = np.nonzero(cast)
            blocked[ri, ki] = md.host_ray_cast(vertices, faces, o[ri], d[ri, ki], 0.0, t_max, any_hit=True)[3]
        seen = cast & ~blocked
        m = np.zeros((len(rows), 3))
        for k in range(K):                                                             # (sequential, in index order)
            m = np.where(seen[:, k, None], m + d[:, k, :], m)
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        long = length > 0.0
        unit = np.where(long[:, None], m / np.where(long, length, 1.0)[:, None], 0.0)
        n_hits = (cast & blocked).sum(axis=1).astype(np.int32)
        n_cast = cast.sum(axis=1)
        row_ao = np.where(n_cast > 0, 1.0 - n_hits / np.where(n_cast > 0, n_cast, 1), 1.0)
    hits = np.full(R, -1, dtype=np.int32)
    visible = np.zeros(R, dtype=np.int32)
    ao = np.full(R, np.nan)
    bent = np.zeros((R, 3))
    hits[rows], visible[rows], ao[rows], bent[rows] = n_hits, seen.sum(axis=1).astype(np.int32), row_ao, unit
    words = None
    if bits:
        n_words = (K + 31) // 32
        padded = np.zeros((len(rows), n_words * 32), dtype=np.uint32)
        padded[:, :K] = seen
        packed = (padded.reshape(len(rows), n_words, 32) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint32)
        words = np.zeros((R, n_words), dtype=np.int32)
        words[rows] = packed.view(np.int32)
    return hits, visible, ao, bent, words


def unpack_bits(words, K):
    """words int32 [R, ceil(K / 32)] (numpy or tensor) -> bool [R, K] numpy: direction k was cast and not blocked."""
    w = to_numpy(words).astype(np.int32).view(np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(w.shape[0], -1)[:, :K]


def default_bias(index):
    """1e-4 x the bounding-box diagonal of the mesh of a MeshIndex / _HostMesh, in float64 on the host -> float."""
    if isinstance(index, md.MeshIndex):
        lo, hi = np.asarray(index.lo, dtype=np.float64), np.asarray(index.hi, dtype=np.float64)     # (the exact extremes, read at the build)
    else:
        lo, hi = index.vertices.min(axis=0), index.vertices.max(axis=0)
    e = hi - lo
    return float(BIAS_SCALE * np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]))


# ------------------------------------------------------------------------------------------------ one code path over both
def occlusion_rows(mesh_or_index, points, normals, table=None, K=64, local=True, bias=None, t_max=float('inf'), bits=False, n_tests=None):
    """host_occlusion_rows for a numpy mesh (numpy out); for a ``MeshIndex`` or device tensors the same through psn_occlusion_rows
    (device tensors out, bit for bit).  ``table`` = None: hemisphere_table(K).  ``bias`` = None: 1e-4 x the bounding-box diagonal of
    the mesh, computed on the host in float64.  -> (hits, visible, ao, bent, words or None)."""
    if isinstance(mesh_or_index, (md.MeshIndex, md._HostMesh)):
        index = mesh_or_index
    else:
        v = mesh_parts(mesh_or_index)[0]
        if torch.is_tensor(v) and not v.is_cuda:
            raise RuntimeError('occlusion_rows: a HIP device mesh (the kernel) or a numpy mesh (the host definition) expected, got CPU tensors')
        index = md._prepare(mesh_or_index, None, 'mesh')
    if table is None:
        table = hemisphere_table(K)
    if bias is None:
        bias = default_bias(index)
    return index.occlusion(points, normals, table, local=local, bias=float(bias), t_max=float(t_max), bits=bits, n_tests=n_tests)


def area_weighted_normals(vertices, faces):
    """Per vertex the normalised sum of the (b - a) x (c - a) of its faces (area-weighted face normals); numpy in, numpy float64 out;
    a vertex of no face, or whose sum has no length, gets zero (and so casts nothing)."""
    v, f = to_numpy(vertices).astype(np.float64).reshape(-1, 3), to_numpy(faces).astype(np.int64).reshape(-1, 3)
    m = np.zeros_like(v)
    cross = np.stack(face_cross(v, f), axis=1)
    for c in range(3):
        np.add.at(m, f[:, c], cross)
    with np.errstate(all='ignore'):
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        long = length > 0.0
        return np.where(long[:, None], m / np.where(long, length, 1.0)[:, None], 0.0)


def vertex_occlusion(mesh, vertex_normals=None, table=None, K=64, local=True, bias=None, t_max=float('inf'), bits=False, device=None):
    """occlusion_rows at the vertices of ``mesh`` (a Mesh, a (vertices, faces[, normals]) tuple, a MeshIndex): the rows are the
    vertices with ``vertex_normals`` (default: the mesh's own, else area-weighted face normals: area_weighted_normals on the host path,
    meshtopo's vertex-normal kernel, which gives the same bits, on the device).  A mesh on the device, or ``device='cuda'``, takes the
    kernels."""
    if isinstance(mesh, (md.MeshIndex, md._HostMesh)):
        index, vn = mesh, vertex_normals
    else:
        v, f, own = mesh_parts(mesh)
        vn = own if vertex_normals is None else vertex_normals
        index = md._prepare((v, f), device, 'mesh')
    if vn is None and isinstance(index, md.MeshIndex):      # on the device: the same bits without the copy-back (the index checked the faces)
        from . import meshtopo
        vn = meshtopo._device_vertex_normals(index.vertices, index.faces, 'area', check=False)
    elif vn is None:
        vn = area_weighted_normals(index.vertices, index.faces)
    if isinstance(index, md.MeshIndex):
        vn = torch.as_tensor(to_numpy(vn) if not (torch.is_tensor(vn) and vn.is_cuda) else vn).to(index.vertices.device)
    else:
        vn = to_numpy(vn)
    return occlusion_rows(index, index.vertices, vn, table, K, local, bias, t_max, bits)
