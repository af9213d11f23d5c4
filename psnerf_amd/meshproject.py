"""The views projected onto the mesh: per surface row (point, normal) which of V cameras see it and what their images show there --
the way back from the images to the surface, which meshrender (pixels -> triangles), meshbake (networks -> atlas) and meshocclude
(hemispheres) do not give.  On it rest the photographic texture (meshbake.bake_views), photometric-stereo normals fused per vertex
(``vertex_views(..., frame='camera_normal')`` and ``fused_normals``), photo-consistency (``spread``) and visible-surface evaluation
(mesheval.evaluate_mesh(visible_from=...)).  The reference has nothing of the kind.

Two implementations of one definition, as in every mesh module:
  * numpy inputs -> ``host_project_rows`` below, float64 with every operation order written out: it IS the definition.
  * a ``MeshIndex`` / device tensors -> csrc/meshproject.hip (psn_project_rows), one thread per row over all views in ascending order,
    the segment to each camera formed in registers and walked with psn_ray_cast's own any-hit walk: every output equal bit for bit.

Definition.  Inputs: a mesh, rows points / normals [R, 3], images [V, H, W, C] uint8 (a byte u is the double u / 255.0) or float32
(widened exactly), 1 <= C <= 4 -- or no images and ``hw`` = (H, W): visibility only --, the cameras as hull._views takes them (its
[V, 16] table: R row-major, o, K00, K02, K12), optional masks [V, H, W] (non-zero = set), bias (None: meshocclude.default_bias),
cos_min, weight 'cosine' | 'uniform', frame 'raw' | 'camera_normal', bits.
A row whose point or normal has a non-finite component, or whose normal is zero, sees nothing: n_seen 0, best_view -1, every sum,
weight and word 0.  For every other row the views are taken in ascending order, and view v SEES the row iff all of
  1. projection (hull._project_uv, the one statement of it): d = p - o, x_c = (d0 R[0, c] + d1 R[1, c]) + d2 R[2, c], front = x_2 > 0,
     u = K02 + K00 (x_0 / x_2), v = K12 + K00 (x_1 / x_2);
  2. footprint: front, 0 <= u <= W - 1 and 0 <= v <= H - 1 in float64 (a NaN is outside); then x0 = floor u, x1 = min(x0 + 1, W - 1),
     fx = u - x0, likewise y0, y1, fy (meshbake.host_atlas_sample's rule);
  3. facing: e = o - p, c = ((n0 e0 + n1 e1) + n2 e2) / sqrt((e0 e0 + e1 e1) + e2 e2), and c > cos_min strictly;
  4. mask: with masks, the four pixels (y0 | y1, x0 | x1) of view v are all non-zero (a sample that would blend object and
     background is not taken);
  5. not blocked: q = p + bias n (three products, then three sums), r = o - q, and
     meshdist.host_ray_cast(vertices, faces, q, r, t_min=0.0, t_max=1.0, any_hit=True) reports no hit (r is not normalised: t = 1 is the
     camera; a q or r that is not a ray the cast takes at all -- a non-finite component, r = 0 -- misses, as there).
The sample of a seeing view, per channel: val = (1 - fy)((1 - fx) t00 + fx t10) + fy ((1 - fx) t01 + fx t11), t_ab the pixel (y_b, x_a).
frame 'camera_normal' (C = 3): val is then taken to the world by the trainer's rule (stage1/training.py:_targets_torch),
w_i = (R[i, 0] val0 + R[i, 1] (-val1)) + R[i, 2] (-val2), and that vector is what is accumulated and reported.
Weight: w = c ('cosine') or 1 ('uniform').  Accumulated in view order from 0: sum[ch] += w val[ch]; sum_sq[ch] += w (val[ch] val[ch]);
weight += w; n_seen += 1; best_view = the seeing view with the largest w, a tie to the lowest index; best_value = its val; with
``bits``, bit v % 32 of word v // 32 is set.
Outputs (``Projection``): sum, sum_sq [R, C], weight [R] float64; n_seen, best_view [R] int32; best_value [R, C] float64; words int32
[R, ceil(V / 32)] or None.  Without images sum, sum_sq and best_value are None.

Not built: blending across seams, colour correction between views, soft visibility."""
import collections

import numpy as np
import torch

from . import hull
from . import meshdist as md
from .meshcore import Mesh, device_mesh, face_cross, host_mesh, mesh_parts, on_device, to_numpy

MAX_VIEWS = 256              # PSN_PROJECT_MAX_VIEWS: the device's limit; the definition has none
MAX_EXTENT = 32768           # PSN_PROJECT_MAX_EXTENT
MAX_CHANNELS = 4             # PSN_PROJECT_MAX_CHANNELS

Projection = collections.namedtuple('Projection', 'sum sum_sq weight n_seen best_view best_value words')


def check_modes(weight, frame, what):
    """-> (uniform, camera_normal); ValueError for anything else."""
    if weight not in ('cosine', 'uniform'):
        raise ValueError('%s: weight=%r (\'cosine\' or \'uniform\')' % (what, weight))
    if frame not in ('raw', 'camera_normal'):
        raise ValueError('%s: frame=%r (\'raw\' or \'camera_normal\')' % (what, frame))
    return weight == 'uniform', frame == 'camera_normal'


def _check_images(images, hw, masks, V, camera_normal, what):
    """-> (H, W, C) after the shape and type rules of the definition (images / masks: numpy arrays or tensors, or None)."""
    if images is None:
        if hw is None:
            raise ValueError('%s: without images, hw = (H, W) is required' % what)
        H, W, C = int(hw[0]), int(hw[1]), 0
    else:
        dtype = str(images.dtype).replace('torch.', '')
        if len(images.shape) != 4 or dtype not in ('uint8', 'float32'):
            raise ValueError('%s: images uint8 or float32 [V, H, W, C] expected, got %s %s' % (what, dtype, tuple(images.shape)))
        H, W, C = (int(x) for x in images.shape[1:])
        if images.shape[0] != V or not 1 <= C <= MAX_CHANNELS:
            raise ValueError('%s: images %s for %d views (1 <= C <= %d)' % (what, tuple(images.shape), V, MAX_CHANNELS))
        if hw is not None and (int(hw[0]), int(hw[1])) != (H, W):
            raise ValueError('%s: hw = %r, the images are %d x %d' % (what, tuple(hw), H, W))
    if not (1 <= H <= MAX_EXTENT and 1 <= W <= MAX_EXTENT):
        raise ValueError('%s: images of %d x %d (1 .. %d)' % (what, H, W, MAX_EXTENT))
    if masks is not None and tuple(masks.shape) != (V, H, W):
        raise ValueError('%s: masks [%d, %d, %d] expected, got %s' % (what, V, H, W, tuple(masks.shape)))
    if camera_normal and C != 3:
        raise ValueError('%s: frame=\'camera_normal\' needs C = 3, got %d' % (what, C))
    return H, W, C


def _check_scalars(bias, cos_min, what):
    if not np.isfinite(bias):
        raise ValueError('%s: bias = %r is not finite' % (what, bias))
    if not np.isfinite(cos_min):
        raise ValueError('%s: cos_min = %r is not finite' % (what, cos_min))


# ------------------------------------------------------------------------------------------------ host path: the definition
def host_project_table(vertices, faces, points, normals, images, table, hw=None, masks=None, bias=0.0, cos_min=0.0, weight='cosine',
                       frame='raw', bits=False):
    """The definition (module docstring) over the view table ``table`` [V, 16] of hull._views -> Projection of numpy arrays."""
    what = 'host_project_rows'
    uniform, camera_normal = check_modes(weight, frame, what)
    _check_scalars(bias, cos_min, what)
    table = np.asarray(table, dtype=np.float64)
    V = table.shape[0]
    images = None if images is None else np.asarray(images)
    masks = None if masks is None else np.asarray(masks) != 0
    H, W, C = _check_images(images, hw, masks, V, camera_normal, what)
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = np.asarray(normals, dtype=np.float64).reshape(-1, 3)
    if p.shape != n.shape:
        raise ValueError('%s: %d points and %d normals' % (what, p.shape[0], n.shape[0]))
    R = p.shape[0]
    ok = np.isfinite(p).all(axis=1) & np.isfinite(n).all(axis=1) & (n != 0.0).any(axis=1)
    rows = np.nonzero(ok)[0]
    p, n = p[rows], n[rows]
    r = len(rows)
    total, total_sq, best_value = np.zeros((r, C)), np.zeros((r, C)), np.zeros((r, C))
    w_sum, best_w = np.zeros(r), np.zeros(r)
    n_seen, best_view = np.zeros(r, dtype=np.int32), np.full(r, -1, dtype=np.int32)
    seen_bits = np.zeros((r, V), dtype=bool)
    with np.errstate(all='ignore'):
        q = p + bias * n
        for v in range(V):                                                             # (sequential, in view order)
            view = table[v]
            Rm, o = view[0:9].reshape(3, 3), view[9:12]
            pu, pv, front = hull._project_uv(p, view)
            inside = front & (pu >= 0.0) & (pu <= float(W - 1)) & (pv >= 0.0) & (pv <= float(H - 1))
            e0, e1, e2 = o[0] - p[:, 0], o[1] - p[:, 1], o[2] - p[:, 2]
            c = ((n[:, 0] * e0 + n[:, 1] * e1) + n[:, 2] * e2) / np.sqrt((e0 * e0 + e1 * e1) + e2 * e2)
            sees = inside & (c > cos_min)
            at = np.nonzero(sees)[0]
            flx, fly = np.floor(pu[at]), np.floor(pv[at])
            x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
            fx, fy = pu[at] - flx, pv[at] - fly
            if masks is not None:
                m = masks[v]
                keep = m[y0, x0] & m[y0, x1] & m[y1, x0] & m[y1, x1]
                at, x0, x1, y0, y1, fx, fy = (a[keep] for a in (at, x0, x1, y0, y1, fx, fy))
            if len(at):
                blocked = md.host_ray_cast(vertices, faces, q[at], o[None, :] - q[at], 0.0, 1.0, any_hit=True)[3]
                at, x0, x1, y0, y1, fx, fy = (a[~blocked] for a in (at, x0, x1, y0, y1, fx, fy))
            if not len(at):
                continue
            w = np.ones(len(at)) if uniform else c[at]
            val = np.zeros((len(at), C))
            if C:
                img = images[v]
                wide = (lambda t: t / 255.0) if img.dtype == np.uint8 else (lambda t: t)
                t00, t10 = wide(img[y0, x0].astype(np.float64)), wide(img[y0, x1].astype(np.float64))
                t01, t11 = wide(img[y1, x0].astype(np.float64)), wide(img[y1, x1].astype(np.float64))
                fx, fy = fx[:, None], fy[:, None]
                val = (1.0 - fy) * ((1.0 - fx) * t00 + fx * t10) + fy * ((1.0 - fx) * t01 + fx * t11)
                if camera_normal:
                    a, b, g = val[:, 0], -val[:, 1], -val[:, 2]
                    val = np.stack([(Rm[i, 0] * a + Rm[i, 1] * b) + Rm[i, 2] * g for i in range(3)], axis=1)
                total[at] += w[:, None] * val
                total_sq[at] += w[:, None] * (val * val)
            better = (n_seen[at] == 0) | (w > best_w[at])                              # (a tie stays with the lower view)
            best_w[at[better]], best_view[at[better]], best_value[at[better]] = w[better], v, val[better]
            w_sum[at] += w
            n_seen[at] += 1
            seen_bits[at, v] = True
    out = [np.zeros((R, C)), np.zeros((R, C)), np.zeros(R), np.zeros(R, dtype=np.int32), np.full(R, -1, dtype=np.int32), np.zeros((R, C))]
    for full, part in zip(out, (total, total_sq, w_sum, n_seen, best_view, best_value)):
        full[rows] = part
    words = None
    if bits:
        n_words = (V + 31) // 32
        padded = np.zeros((r, n_words * 32), dtype=np.uint32)
        padded[:, :V] = seen_bits
        packed = (padded.reshape(r, n_words, 32) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint32)
        words = np.zeros((R, n_words), dtype=np.int32)
        words[rows] = packed.view(np.int32)
    if C == 0:
        out[0] = out[1] = out[5] = None
    return Projection(*out, words)


def host_project_rows(vertices, faces, points, normals, images, camera_mats, world_mats, masks=None, bias=None, cos_min=0.0,
                      weight='cosine', frame='raw', bits=False, hw=None):
    """The definition (module docstring) -> Projection of numpy arrays.  ``images`` None with ``hw`` = (H, W): visibility only."""
    if bias is None:
        from .meshocclude import default_bias
        bias = default_bias(md._HostMesh(vertices, faces))
    return host_project_table(vertices, faces, points, normals, images, hull._views(camera_mats, world_mats), hw, masks, float(bias),
                              float(cos_min), weight, frame, bits)


def unpack_bits(words, V):
    """words int32 [R, ceil(V / 32)] (numpy or tensor) -> bool [R, V] numpy: view v sees the row."""
    from .meshocclude import unpack_bits as unpack
    return unpack(words, V)


# ------------------------------------------------------------------------------------------------ what the sums give
def _xp(x):
    return torch if torch.is_tensor(x) else np


def mean(result):
    """sum / weight per row [R, C]; 0 where the weight is 0."""
    xp = _xp(result.weight)
    has = (result.weight != 0.0)[:, None]
    return xp.where(has, result.sum / xp.where(has, result.weight[:, None], xp.ones_like(result.weight[:, None])), xp.zeros_like(result.sum))


def spread(result):
    """The weighted standard deviation of what the views show, sqrt(max(sum_sq / weight - mean^2, 0)) [R, C]; 0 where the weight is 0."""
    xp = _xp(result.weight)
    has = (result.weight != 0.0)[:, None]
    m = mean(result)
    second = xp.where(has, result.sum_sq / xp.where(has, result.weight[:, None], xp.ones_like(result.weight[:, None])), xp.zeros_like(m))
    var = second - m * m
    return xp.sqrt(xp.where(var > 0.0, var, xp.zeros_like(var)))


def fused_normals(result):
    """``sum`` normalised per row [R, 3] (the fused normal of a frame='camera_normal' projection); a zero stays zero."""
    xp = _xp(result.weight)
    m = result.sum
    length = xp.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
    long = (length > 0.0)[:, None]
    return xp.where(long, m / xp.where(long, length[:, None], xp.ones_like(length[:, None])), xp.zeros_like(m))


# ------------------------------------------------------------------------------------------------ one code path over both
def _index_of(mesh_or_index, device, what):
    if isinstance(mesh_or_index, (md.MeshIndex, md._HostMesh)):
        return mesh_or_index
    v = mesh_parts(mesh_or_index)[0]
    if device is None and torch.is_tensor(v) and not v.is_cuda:
        raise RuntimeError('%s: a HIP device mesh (the kernel) or a numpy mesh (the host definition) expected, got CPU tensors' % what)
    return md._prepare(mesh_or_index, device, 'mesh')


def project_rows(mesh_or_index, points, normals, images, camera_mats, world_mats, masks=None, bias=None, cos_min=0.0, weight='cosine',
                 frame='raw', bits=False, hw=None, n_tests=None, out=None, device=None):
    """host_project_rows for a numpy mesh (numpy out); for a ``MeshIndex`` or device tensors (or ``device='cuda'``) the same through
    psn_project_rows (device tensors out, bit for bit).  ``bias`` = None: 1e-4 x the bounding-box diagonal of the mesh, computed on
    the host in float64.  ``images`` None with ``hw`` = (H, W): visibility only.  -> Projection."""
    what = 'project_rows'
    index = _index_of(mesh_or_index, device, what)
    uniform, camera_normal = check_modes(weight, frame, what)
    views = hull._views(camera_mats, world_mats)
    V = views.shape[0]
    _check_images(images, hw, masks, V, camera_normal, what)
    if bias is None:
        from .meshocclude import default_bias
        bias = default_bias(index)
    _check_scalars(bias, cos_min, what)
    if isinstance(index, md.MeshIndex):
        if V > MAX_VIEWS:
            raise ValueError('%s: %d views, the kernel takes %d' % (what, V, MAX_VIEWS))
        dev = index.vertices.device
        place = lambda x: x if torch.is_tensor(x) and x.is_cuda else torch.from_numpy(np.array(to_numpy(x))).to(dev)
        return index.project_rows(place(points), place(normals), images, views, hw=hw, masks=masks, bias=float(bias), cos_min=float(cos_min),
                                  weight=weight, frame=frame, bits=bits, n_tests=n_tests, out=out)
    return index.project_rows(points, normals, images, views, hw=hw, masks=masks, bias=float(bias), cos_min=float(cos_min), weight=weight,
                              frame=frame, bits=bits)


def vertex_views(mesh, images, camera_mats, world_mats, vertex_normals=None, device=None, **options):
    """project_rows at the vertices of ``mesh`` (a Mesh, a (vertices, faces[, normals]) tuple, a MeshIndex): the rows are the vertices
    with ``vertex_normals`` (default: meshtopo.vertex_normals, area-weighted; the same bits on both paths) -> Projection per vertex.
    A mesh on the device, or ``device='cuda'``, takes the kernels.  ``options``: project_rows' other arguments."""
    from . import meshtopo
    index = _index_of(mesh, device, 'vertex_views')
    vn = vertex_normals
    if vn is None:
        vn = meshtopo.vertex_normals((index.vertices, index.faces))
    return project_rows(index, index.vertices, vn, images, camera_mats, world_mats, **options)


def face_rows(vertices, faces):
    """The rows of the faces: centroid ((a + b) + c) x t, t = the double nearest 1 / 3 (a product, not a quotient: torch divides a
    device tensor by a scalar through the reciprocal, so only the product has the same bits on both paths), and the geometric unit normal (b - a) x (c - a) / |.|, |m| = sqrt((m0 m0 +
    m1 m1) + m2 m2), zero where that is not > 0 (such a face sees nothing); numpy arrays or tensors alike, the same bits."""
    xp = _xp(vertices)
    a, b, c = vertices[faces[:, 0]], vertices[faces[:, 1]], vertices[faces[:, 2]]
    centroid = ((a + b) + c) * (1.0 / 3.0)
    m0, m1, m2 = face_cross(vertices, faces)
    m = xp.stack([m0, m1, m2], 1)
    if xp is np:
        with np.errstate(all='ignore'):
            length = np.sqrt((m0 * m0 + m1 * m1) + m2 * m2)
            long = (length > 0.0)[:, None]
            return centroid, np.where(long, m / np.where(long, length[:, None], 1.0), 0.0)
    length = torch.sqrt((m0 * m0 + m1 * m1) + m2 * m2)
    long = (length > 0.0)[:, None]
    return centroid, torch.where(long, m / torch.where(long, length[:, None], torch.ones_like(length[:, None])), torch.zeros_like(m))


def face_visibility(mesh, camera_mats, world_mats, H, W, masks=None, device=None, **options):
    """The number of views that see each face of ``mesh`` -> n_seen int32 [F]: project_rows without images at the face centroids with
    the faces' geometric normals (``face_rows``).  ``options``: bias, cos_min, and ``result=True`` for the whole Projection (``bits``
    then gives the words)."""
    whole = options.pop('result', False)
    index = _index_of(mesh, device, 'face_visibility')
    p, n = face_rows(index.vertices, index.faces)
    res = project_rows(index, p, n, None, camera_mats, world_mats, masks=masks, hw=(H, W), **options)
    return res if whole else res.n_seen


def trim_unseen(mesh, camera_mats, world_mats, H, W, masks=None, device=None, **options):
    """``mesh`` without the faces no view sees (face_visibility == 0), compacted as meshclean compacts: the kept faces in their order,
    re-indexed, and the vertices they use in their order, with their normals -> (Mesh, n_seen per ORIGINAL face).  Device tensors, or
    ``device='cuda'``, take the device path (the trimmed mesh is copied back); otherwise the host path."""
    vertices, faces, normals = mesh_parts(mesh) if not isinstance(mesh, (md.MeshIndex, md._HostMesh)) else (mesh.vertices, mesh.faces, None)
    index = _index_of(mesh, device, 'trim_unseen')
    n_seen = face_visibility(index, camera_mats, world_mats, H, W, masks=masks, **options)
    if isinstance(index, md.MeshIndex):
        from . import hip
        v, f, nrm = device_mesh(index.vertices, index.faces, normals, index.vertices.device)
        face_keep = (n_seen > 0).view(torch.uint8).contiguous()
        vertex_keep = torch.zeros(v.shape[0], dtype=torch.uint8, device=v.device)
        vertex_keep[f[n_seen > 0].reshape(-1)] = 1
        face_incl, vertex_incl = torch.cumsum(face_keep, dim=0, dtype=torch.int64), torch.cumsum(vertex_keep, dim=0, dtype=torch.int64)
        n_out_f, n_out_v = (int(x) for x in torch.stack([face_incl[-1], vertex_incl[-1]]).tolist())
        if n_out_f == 0:
            return Mesh(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)), n_seen
        out_v, out_f, out_n = hip.cc_compact(v, f, nrm, face_keep, vertex_keep, face_incl - face_keep, vertex_incl - vertex_keep, n_out_f, n_out_v)
        return Mesh(out_v.cpu().numpy(), out_f.cpu().numpy(), vertex_normals=to_numpy(out_n)), n_seen
    v, f, nrm = host_mesh(index.vertices, index.faces, to_numpy(normals))
    out_f = f[n_seen > 0]
    vertex_keep = np.zeros(v.shape[0], dtype=bool)
    vertex_keep[out_f.reshape(-1)] = True
    new_index = np.cumsum(vertex_keep) - 1
    return Mesh(v[vertex_keep], new_index[out_f].astype(np.int64).reshape(-1, 3), vertex_normals=None if nrm is None else nrm[vertex_keep]), n_seen
