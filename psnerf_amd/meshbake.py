"""Baking the stage-2 materials onto the exported mesh: a texture atlas of the mesh, the albedo / specular / normal textures of a trained
``stage2.PSNetwork`` on it, and the textured OBJ + MTL another renderer can load.  The reference has nothing of the kind: its albedo,
specular weights and normals exist only as per-view images.

Two implementations of one definition, as in photostereo.py / mesheval.py:
  * numpy inputs -> the functions below (``Atlas``, ``host_atlas_points``, ``host_atlas_scatter``, ``host_atlas_sample``), which ARE the
    definition: integer layout, float64 geometry with every operation order written out.
  * device tensors -> csrc/meshbake.hip (psn_atlas_points, psn_atlas_scatter, psn_atlas_fill, psn_atlas_sample), the same operations in
    the same order: equal bit for bit.

The atlas.  Two faces share one square cell of c x c texels of a T x T texture; no chart packing, no area weighting (marching-cubes and
vertex-clustered faces are near-uniform in size) -- the layout is exact and reproducible.  With F faces:
  c = the largest integer with (T // c)^2 >= ceil(F / 2) (or the ``cell`` given); c < 4 is refused.  G = T // c, n = c - 3,
  K = (n + 2)(n + 3) / 2 rows per face.
  Face f: cell q = f // 2, origin (X0, Y0) = ((q % G) c, (q // G) c), half h = f % 2.  Texel coordinates are texel-centre indices (x, y);
  y is the row of the image array, row 0 the top of the PNG.
  h = 0: corner 0 -> (X0, Y0), corner 1 -> (X0 + n, Y0), corner 2 -> (X0, Y0 + n); local texel (i, j), i, j >= 0, i + j <= n + 1, sits
  at (X0 + i, Y0 + j).  h = 1: the same reflected through the cell centre, (X0 + c - 1 - i, Y0 + c - 1 - j) -- both halves keep their
  orientation.  The row of local (i, j) of face f is r = f K + k, k = j (n + 2) - j (j - 1) / 2 + i.
  The line i + j = n + 1 is the face's GUTTER: the corners lie on texel centres, so a bilinear lookup anywhere inside the UV triangle
  reads only texels the face owns -- the two legs need no gutter, the hypotenuse needs exactly this line.  The cell diagonal
  x + y - X0 - Y0 = c - 1, the free half of a last cell that holds one face, the cells behind it and the margin beyond G c belong to no
  face and hold ``fill``.
  Surface point of a row: p = (v0 + (i / n) e1) + (j / n) e2, e1 = v1 - v0, e2 = v2 - v0, float64.  Gutter rows lie up to 1 / n of an edge
  BEYOND the hypotenuse, in the face's plane, and are deliberately not clamped: the baked texture of an affine field is then affine over
  the whole owned set, and the bilinear lookup reproduces it.
  Normal of a row: normalise((b0 n0 + b1 n1) + b2 n2), b = (1 - (i + j) / n, i / n, j / n), with vertex normals; normalise(e1 x e2)
  without; |m| = sqrt((m0 m0 + m1 m1) + m2 m2), and a vector whose length is not > 0 becomes zero, never NaN.
  OBJ coordinates of a corner at (x, y): u = (x + 0.5) / T, v = 1 - (y + 0.5) / T; every face gets three ``vt`` of its own.
The lookup (``host_atlas_sample``): (x, y) = (b0 (x0, y0) + b1 (x1, y1)) + b2 (x2, y2) over the corner texels, barycentrics in the corner
  order MeshIndex.ray_cast / host_ray_triangle return; x0 = clamp(floor x, 0, T - 1), x1 = min(x0 + 1, T - 1), fx = x - floor x, likewise y;
  value = (1 - fy)((1 - fx) t00 + fx t10) + fy ((1 - fx) t01 + fx t11) in float64.  A face outside 0 .. F - 1 (a miss is -1) or a
  position that is not finite gives a NaN row.
Bytes (``to_img``, the rule of imgmetrics.to_img in float32): clip to [0, 1], x 255, round half to even; NaN -> 0.
Baked visibility (``bake_occlusion``, or ``bake_materials(..., occlusion=K)``): the rows' points and normals go through
  meshocclude.occlusion_rows (K cosine-weighted directions about the row's normal, any-hit against the mesh itself) and the ambient
  occlusion and the bent normal of each row are scattered like any other map; a row that casts nothing (a zero normal) bakes ``fill``.
Baked photographs (``bake_views``): the rows' points and normals go through meshproject.project_rows (which views see the row, and the
  weighted sums of what their images show there); the mean, the best view's sample, the number of seeing views and the weighted spread
  of each row are scattered like any other map; a row no view sees bakes ``fill``.
"""
import math
import os

import numpy as np
import torch

from .meshcore import Phase, device_mesh, face_cross, host_mesh, mesh_parts, on_device, to_numpy

MIN_CELL = 4                 # PSN_ATLAS_MIN_CELL
MAX_SIZE = 32768             # PSN_ATLAS_MAX_SIZE
MAX_CHANNELS = 32            # PSN_ATLAS_MAX_CHANNELS
CHUNK_ROWS = 1 << 20         # bake_materials: rows per chunk of faces unless chunk_faces is given
MAPS = ('albedo', 'specular', 'normal')


# ------------------------------------------------------------------------------------------------ the atlas: integers only
class Atlas(object):
    """The layout of F faces in a T x T texture (module docstring).  T, F, c, G, n, K are plain ints."""

    def __init__(self, T, F, cell=None):
        T, F = int(T), int(F)
        if F < 1 or not 1 <= T <= MAX_SIZE:
            raise ValueError('Atlas: %d faces in a texture of %d x %d (at least one face; 1 .. %d texels a side)' % (F, T, T, MAX_SIZE))
        cells = (F + 1) // 2
        g = math.isqrt(cells - 1) + 1                    # the fewest cells per side: the smallest g with g g >= cells
        c = T // g if cell is None else int(cell)        # T // c >= g  <=>  c <= T // g
        if c < MIN_CELL or c > T or (T // c) ** 2 < cells:
            raise ValueError('Atlas: F = %d faces need %d x %d cells of at least %d texels: T >= %d (T = %d%s)' % (
                F, g, g, MIN_CELL, MIN_CELL * g, T, '' if cell is None else ', cell = %d' % c))
        self.T, self.F, self.c, self.G, self.n = T, F, c, T // c, c - 3
        self.K = (self.n + 2) * (self.n + 3) // 2

    def __repr__(self):
        return 'Atlas(T=%d, F=%d, cell=%d)' % (self.T, self.F, self.c)

    def local(self):
        """The local texels in row order -> (i [K], j [K]) int64: k = j (n + 2) - j (j - 1) / 2 + i."""
        n = self.n
        j = np.repeat(np.arange(n + 2, dtype=np.int64), np.arange(n + 2, 0, -1))
        i = np.arange(self.K, dtype=np.int64) - (j * (n + 2) - j * (j - 1) // 2)
        return i, j

    def _place(self, f, i, j):
        """Local (i, j) of the faces f (broadcast together) -> texel (x, y), int64."""
        f = np.asarray(f, dtype=np.int64)
        q, h = f // 2, f % 2
        X0, Y0 = (q % self.G) * self.c, (q // self.G) * self.c
        return np.where(h == 0, X0 + i, X0 + self.c - 1 - i), np.where(h == 0, Y0 + j, Y0 + self.c - 1 - j)

    def texels(self, f0=0, f1=None):
        """The texels of the rows of the faces f0 <= f < f1, in row order -> (x, y) int64 [(f1 - f0) K]."""
        f0, f1 = self._range(f0, f1)
        i, j = self.local()
        x, y = self._place(np.arange(f0, f1, dtype=np.int64)[:, None], i[None, :], j[None, :])
        return x.reshape(-1), y.reshape(-1)

    def corners(self, f=None):
        """The corner texels of the faces f (default: all) -> int64 [..., 3, 2], (x, y) of corner 0, 1, 2."""
        f = np.arange(self.F, dtype=np.int64) if f is None else np.asarray(f, dtype=np.int64)
        n = self.n
        x, y = self._place(f[..., None], np.array([0, n, 0], dtype=np.int64), np.array([0, 0, n], dtype=np.int64))
        return np.stack([x, y], axis=-1)

    def owner(self):
        """Per texel the face that owns it (-1: none) and its row k within the face -> (face [T, T], k [T, T]) int64, indexed [y, x]."""
        face = np.full((self.T, self.T), -1, dtype=np.int64)
        k = np.full((self.T, self.T), -1, dtype=np.int64)
        x, y = self.texels()
        face[y, x] = np.repeat(np.arange(self.F, dtype=np.int64), self.K)
        k[y, x] = np.tile(np.arange(self.K, dtype=np.int64), self.F)
        return face, k

    def _range(self, f0, f1):
        f0, f1 = int(f0), self.F if f1 is None else int(f1)
        if not 0 <= f0 <= f1 <= self.F:
            raise ValueError('Atlas: face range [%d, %d) of %d faces' % (f0, f1, self.F))
        return f0, f1


def atlas_uv(atlas, f=None):
    """OBJ texture coordinates of the corners of the faces f (default: all) -> float64 [..., 3, 2]: u = (x + 0.5) / T,
    v = 1 - (y + 0.5) / T."""
    xy = atlas.corners(f).astype(np.float64)
    return np.stack([(xy[..., 0] + 0.5) / atlas.T, 1.0 - (xy[..., 1] + 0.5) / atlas.T], axis=-1)


def to_img(x):
    """The byte of a texel, in float32: clip to [0, 1], x 255, round half to even; NaN -> 0 (a NaN has no byte: it is MADE 0 here
    instead of being left to the conversion)."""
    x = np.asarray(x).astype(np.float32)
    x = np.where(np.isnan(x), np.float32(0.0), x)
    return (x.clip(0, 1) * np.float32(255.0)).round().astype(np.uint8)


# ------------------------------------------------------------------------------------------------ host path: the definition
def _unit(m):
    """m / |m| with |m| = sqrt((m0 m0 + m1 m1) + m2 m2); a vector whose length is not > 0 becomes zero."""
    with np.errstate(all='ignore'):
        length = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        ok = length > 0.0
        return np.where(ok[:, None], m / np.where(ok, length, 1.0)[:, None], 0.0)


def host_atlas_points(atlas, vertices, faces, vertex_normals=None, f0=0, f1=None):
    """The surface points and normals of the rows of the faces f0 <= f < f1 -> (points float64 [R, 3], points_f32 float32 [R, 3] = the
    points rounded once, normals float64 [R, 3]), R = (f1 - f0) K."""
    v, f, vn = host_mesh(vertices, faces, vertex_normals, prefix='atlas', widen_normals=True)
    if f.shape[0] != atlas.F:
        raise ValueError('atlas: %d faces, the atlas was laid out for %d' % (f.shape[0], atlas.F))
    f0, f1 = atlas._range(f0, f1)
    i, j = atlas.local()
    nd = float(atlas.n)
    u, w = (i.astype(np.float64) / nd)[None, :, None], (j.astype(np.float64) / nd)[None, :, None]
    tri = f[f0:f1]
    v0 = v[tri[:, 0]][:, None, :]
    e1, e2 = v[tri[:, 1]][:, None, :] - v0, v[tri[:, 2]][:, None, :] - v0
    with np.errstate(all='ignore'):
        p = ((v0 + u * e1) + w * e2).reshape(-1, 3)
        if vn is not None:
            b0 = (1.0 - (i + j).astype(np.float64) / nd)[None, :, None]
            m = (b0 * vn[tri[:, 0]][:, None, :] + u * vn[tri[:, 1]][:, None, :]) + w * vn[tri[:, 2]][:, None, :]
        else:
            m = np.stack(face_cross(v, tri), axis=-1)
            m = np.broadcast_to(m[:, None, :], (f1 - f0, atlas.K, 3))
        return p, p.astype(np.float32), _unit(m.reshape(-1, 3))


def _new_texture(atlas, C, fill, u8):
    if not 1 <= C <= MAX_CHANNELS:
        raise ValueError('atlas: %d channels (1 .. %d)' % (C, MAX_CHANNELS))
    fill = np.float32(0.0 if fill is None else fill)
    return np.full((atlas.T, atlas.T, C), to_img(fill) if u8 else fill, dtype=np.uint8 if u8 else np.float32)


def host_atlas_scatter(atlas, rows, f0=0, f1=None, out=None, fill=None, u8=False):
    """rows float32 [(f1 - f0) K, C] -> the texels of the faces f0 <= f < f1 of a [T, T, C] texture, float32 or (``u8``) bytes by
    ``to_img``.  ``out`` = None: a new texture, ``fill`` (default 0) everywhere else.  ``out`` given: written in place, only the texels
    of those faces -- and, with a ``fill``, the texels that NO face owns; so chunks of faces compose into one texture."""
    f0, f1 = atlas._range(f0, f1)
    rows = np.asarray(rows)
    if rows.dtype != np.float32 or rows.ndim != 2 or rows.shape[0] != (f1 - f0) * atlas.K:
        raise ValueError('atlas: rows float32 [%d, C] expected, got %s %s' % ((f1 - f0) * atlas.K, rows.dtype, rows.shape))
    if out is None:
        out = _new_texture(atlas, rows.shape[1], fill, u8)
    else:
        if out.shape != (atlas.T, atlas.T, rows.shape[1]) or out.dtype not in (np.float32, np.uint8):
            raise ValueError('atlas: texture [%d, %d, %d] float32 or uint8 expected, got %s %s' % (atlas.T, atlas.T, rows.shape[1], out.dtype, out.shape))
        if fill is not None:
            host_atlas_fill(atlas, out, fill)
    x, y = atlas.texels(f0, f1)
    out[y, x] = to_img(rows) if out.dtype == np.uint8 else rows
    return out


def host_atlas_fill(atlas, texture, fill=0.0):
    """The texels no face owns := fill (bytes by ``to_img``), in place."""
    free = atlas.owner()[0] < 0
    texture[free] = to_img(np.float32(fill)) if texture.dtype == np.uint8 else np.float32(fill)
    return texture


def host_atlas_sample(atlas, face, bary, texture):
    """The bilinear lookup of the module docstring: face int64 [Q], bary float64 [Q, 3], texture float32 [T, T, C] -> float64 [Q, C]."""
    face = np.asarray(face, dtype=np.int64).reshape(-1)
    bary = np.asarray(bary, dtype=np.float64).reshape(-1, 3)
    tex = np.asarray(texture)
    if tex.dtype != np.float32 or tex.ndim != 3 or tex.shape[:2] != (atlas.T, atlas.T) or bary.shape[0] != face.shape[0]:
        raise ValueError('atlas: face [Q], bary [Q, 3] and a float32 texture [%d, %d, C] expected' % (atlas.T, atlas.T))
    inside = (face >= 0) & (face < atlas.F)
    xy = atlas.corners(np.where(inside, face, 0)).astype(np.float64)              # [Q, 3, 2]
    with np.errstate(all='ignore'):
        x = (bary[:, 0] * xy[:, 0, 0] + bary[:, 1] * xy[:, 1, 0]) + bary[:, 2] * xy[:, 2, 0]
        y = (bary[:, 0] * xy[:, 0, 1] + bary[:, 1] * xy[:, 1, 1]) + bary[:, 2] * xy[:, 2, 1]
        ok = inside & np.isfinite(x) & np.isfinite(y)
        x, y = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
        flx, fly = np.floor(x), np.floor(y)
        top = float(atlas.T - 1)
        x0, y0 = np.clip(flx, 0.0, top).astype(np.int64), np.clip(fly, 0.0, top).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, atlas.T - 1), np.minimum(y0 + 1, atlas.T - 1)
        fx, fy = (x - flx)[:, None], (y - fly)[:, None]
        t00, t10 = tex[y0, x0].astype(np.float64), tex[y0, x1].astype(np.float64)
        t01, t11 = tex[y1, x0].astype(np.float64), tex[y1, x1].astype(np.float64)
        val = (1.0 - fy) * ((1.0 - fx) * t00 + fx * t10) + fy * ((1.0 - fx) * t01 + fx * t11)
    return np.where(ok[:, None], val, np.nan)


# ------------------------------------------------------------------------------------------------ one code path over both
def _no_cpu_tensor(x, what):
    if torch.is_tensor(x) and not x.is_cuda:
        raise RuntimeError('%s: a HIP device tensor (the kernels) or a numpy array (the host definition) expected, got a CPU tensor' % what)


def atlas_points(atlas, vertices, faces, vertex_normals=None, f0=0, f1=None):
    """host_atlas_points for numpy arrays; for device tensors the same through psn_atlas_points (bit for bit), device tensors out."""
    _no_cpu_tensor(vertices, 'atlas_points')
    if not on_device(vertices):
        return host_atlas_points(atlas, vertices, faces, vertex_normals, f0, f1)
    from . import hip
    if faces.shape[0] != atlas.F:
        raise RuntimeError('atlas: %d faces, the atlas was laid out for %d' % (faces.shape[0], atlas.F))
    return hip.atlas_points(vertices, faces, vertex_normals, atlas.T, atlas.c, f0, f1)


def atlas_scatter(atlas, rows, f0=0, f1=None, out=None, fill=None, u8=False):
    """host_atlas_scatter for numpy arrays; for device tensors the same through psn_atlas_scatter / psn_atlas_fill."""
    _no_cpu_tensor(rows, 'atlas_scatter')
    if not on_device(rows):
        return host_atlas_scatter(atlas, rows, f0, f1, out, fill, u8)
    from . import hip
    if out is None:
        if rows.dim() != 2 or not 1 <= rows.shape[1] <= MAX_CHANNELS:
            raise RuntimeError('atlas: rows [R, 1 .. %d] expected, got %s' % (MAX_CHANNELS, tuple(rows.shape)))
        start = np.float32(0.0 if fill is None else fill)
        out = torch.full((atlas.T, atlas.T, rows.shape[1]), int(to_img(start)) if u8 else float(start), dtype=torch.uint8 if u8 else torch.float32,
                         device=rows.device)
    elif fill is not None:
        hip.atlas_fill(out, atlas.c, atlas.F, fill)
    return hip.atlas_scatter(rows.contiguous(), out, atlas.c, atlas.F, f0, f1)


def atlas_sample(atlas, face, bary, texture):
    """host_atlas_sample for numpy arrays; for device tensors the same through psn_atlas_sample."""
    _no_cpu_tensor(texture, 'atlas_sample')
    if not on_device(texture):
        return host_atlas_sample(atlas, face, bary, texture)
    from . import hip
    return hip.atlas_sample(face.contiguous(), bary.contiguous(), texture, atlas.c, atlas.F)


# ------------------------------------------------------------------------------------------------ the bake
def host_embed(x, n_freqs):
    """[x, sin(2^k x), cos(2^k x)]_{k < n_freqs} of CPU points [R, 3] in float32 (the columns psn_pe_encode writes on the device)."""
    out = [x]
    for k in range(n_freqs):
        out += [torch.sin(x * float(2 ** k)), torch.cos(x * float(2 ** k))]
    return torch.cat(out, dim=-1)


def eval_network(model, net, x, n_freqs, cache=None):
    """One of the small stage-2 networks (``model.albedo_net``, ``rough_net``, ``normal_net``) on points x float32 [R, 3] -> [R, C].
    Device points: the encoding kernel and the network's own forward, i.e. the fused engine (under ops.STRICT anything else raises).
    CPU points: the same layers in torch on the host (the stage-2 model has no host forward of its own).
    ``cache``: a dict in which the encoding of x is kept per n_freqs (networks on the same points share it)."""
    emb = None if cache is None else cache.get(n_freqs)
    if emb is None:
        emb = model._pe(x, n_freqs) if x.is_cuda else host_embed(x, n_freqs)
        if cache is not None:
            cache[n_freqs] = emb
    if x.is_cuda:
        return net(emb, model._cols(n_freqs, x.device))
    y = emb
    last = len(net.linears) - 1
    for li, layer in enumerate(net.linears):
        y = torch.nn.functional.linear(y, layer.weight, layer.bias)
        if li != last:
            y = torch.relu(y)
            if li in net.skip_at:
                y = torch.cat([y, emb], dim=-1)
        elif net.final == 'sigmoid':
            y = torch.sigmoid(y)
    return y


def material_rows(model, x, row_normals, maps=MAPS, cache=None):
    """The material maps at points x float32 [R, 3] -> {name: float32 [R, C]}: albedo [R, 3]; specular = relu(rough_net) [R, nbasis]
    (sgbasis: the SG weights) or rough_net [R, 1] (microfacet: the roughness); normal = normalize(normal_net) with train.normal_mlp,
    else ``row_normals`` (the geometric normals of the rows) in float32.  ``cache``: see eval_network."""
    from . import ops
    out = {}
    if 'albedo' in maps:
        out['albedo'] = eval_network(model, model.albedo_net, x, model.n_freqs, cache)
    if 'specular' in maps:
        r = eval_network(model, model.rough_net, x, model.n_freqs, cache)
        out['specular'] = torch.relu(r) if model.render_model == 'sgbasis' else r
    if 'normal' in maps:
        if model.normal_mlp:
            out['normal'] = ops.normalize_rows(eval_network(model, model.normal_net, x, model.n_freqs_n, cache))
        else:
            out['normal'] = row_normals.to(torch.float32)
    return out


# When set to a list (tools/bench_bake.py), bake_materials appends (phase, start_event, end_event) recorded on the stream: 'points',
# one phase per map (encoding + network + its output glue) and 'scatter'.
PHASE_EVENTS = None


@torch.no_grad()
def bake_materials(model, mesh, size=2048, maps=MAPS, chunk_faces=None, fill=0.0, device=None, occlusion=None, occlusion_bias=None,
                   occlusion_distance=float('inf')):
    """The material textures of a stage-2 ``PSNetwork`` on ``mesh`` -> {'atlas': Atlas, 'albedo': [T, T, 3], 'specular': [T, T, nbasis]
    (sgbasis) or [T, T, 1] (microfacet), 'normal': [T, T, 3]}, float32, T = ``size``; texels no face owns hold ``fill``.
    The model is put in eval mode for the call and nothing is jittered.  Chunk of faces by chunk of faces (``chunk_faces``; default:
    about a million rows): rows -> points -> networks -> texels, so that no more than one chunk of rows ever exists.
    One code path: a model on the device (or ``device='cuda'``: the mesh is moved there) runs the kernels and returns device tensors;
    a CPU model with a numpy mesh runs the definition and returns numpy arrays.
    ``occlusion`` = K: also 'occlusion' [T, T, 1] and 'bent' [T, T, 3] of ``bake_occlusion`` on the same atlas, from the same rows, with
    K directions, ``occlusion_bias`` (None: 1e-4 x the bounding-box diagonal) and ``occlusion_distance`` (the rays' t_max)."""
    maps = tuple(maps)
    if not maps or any(m not in MAPS for m in maps):
        raise ValueError('bake_materials: maps %r (any of %s)' % (maps, ', '.join(MAPS)))
    param = next(model.parameters())
    dev = param.device if device is None else torch.device(device)
    if dev.type == 'cuda' and dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    if dev != param.device:
        raise ValueError('bake_materials: the model is on %s, device = %s' % (param.device, dev))
    on_dev = dev.type == 'cuda'
    v, f, vn = mesh_parts(mesh)
    if on_dev:
        v, f, vn = device_mesh(v, f, vn, dev, prefix='atlas', widen_normals=True)
        if f.shape[0] and (int(f.min()) < 0 or int(f.max()) >= v.shape[0]):   # (two host reads: the atlas kernels have no status word)
            raise ValueError('atlas: a face refers to a vertex outside 0 .. %d' % (v.shape[0] - 1))
    else:
        v, f, vn = host_mesh(to_numpy(v), to_numpy(f), to_numpy(vn), prefix='atlas', widen_normals=True)
    atlas = Atlas(size, f.shape[0])
    step = max(1, CHUNK_ROWS // atlas.K) if chunk_faces is None else int(chunk_faces)
    if step < 1:
        raise ValueError('bake_materials: chunk_faces = %d' % step)
    occluder = None if occlusion is None else _Occluder(v, f, int(occlusion), occlusion_bias, occlusion_distance)
    was_training = model.training
    model.eval()
    out = {'atlas': atlas}
    try:
        for f0 in range(0, atlas.F, step):
            f1 = min(f0 + step, atlas.F)
            with Phase(PHASE_EVENTS, 'points'):
                p, x, nrm = atlas_points(atlas, v, f, vn, f0, f1)
            if occluder is not None:
                occluder.bake(atlas, p, nrm, f0, f1, out, fill)
            if not on_dev:
                x, nrm = torch.from_numpy(x), torch.from_numpy(nrm)
            cache = {}                                                   # the encodings of this chunk's points
            for name in maps:
                with Phase(PHASE_EVENTS, name):
                    rows = material_rows(model, x, nrm, (name,), cache)[name].float().contiguous()
                with Phase(PHASE_EVENTS, 'scatter'):
                    out[name] = atlas_scatter(atlas, rows if on_dev else rows.numpy(), f0, f1, out.get(name), fill if name not in out else None)
    finally:
        model.train(was_training)
    return out


# ------------------------------------------------------------------------------------------------ baked visibility
class _Occluder(object):
    """The mesh as its own occluder for a bake: the index (a MeshIndex for device tensors, the host twin for numpy arrays), the
    direction table and the bias, made once; ``bake`` turns one chunk of rows into texels of 'occlusion' and 'bent'."""

    def __init__(self, v, f, K, bias, t_max):
        from . import meshdist as md, meshocclude as mo
        self.index = md._prepare((v, f), None, 'mesh')
        self.table = mo.hemisphere_table(K)
        self.bias = mo.default_bias(self.index) if bias is None else float(bias)
        self.t_max = float(t_max)

    def bake(self, atlas, points, normals, f0, f1, out, fill):
        from . import meshocclude as mo
        with Phase(PHASE_EVENTS, 'occlusion'):
            hits, _, ao, bent, _ = mo.occlusion_rows(self.index, points, normals, self.table, bias=self.bias, t_max=self.t_max)
            if torch.is_tensor(ao):
                dead = (hits < 0)[:, None]
                rows = {'occlusion': torch.where(dead, float(fill), ao[:, None].float()), 'bent': torch.where(dead, float(fill), bent.float())}
            else:
                dead = (hits < 0)[:, None]
                rows = {'occlusion': np.where(dead, np.float32(fill), ao[:, None].astype(np.float32)),
                        'bent': np.where(dead, np.float32(fill), bent.astype(np.float32))}
        with Phase(PHASE_EVENTS, 'scatter'):
            for name, r in rows.items():
                out[name] = atlas_scatter(atlas, r.contiguous() if torch.is_tensor(r) else np.ascontiguousarray(r), f0, f1, out.get(name),
                                          fill if name not in out else None)


def bake_occlusion(mesh, size=2048, atlas=None, K=64, bias=None, t_max=float('inf'), chunk_faces=None, fill=0.0, device=None):
    """Ambient occlusion and bent normals of ``mesh`` under its own shadow, on its atlas -> {'atlas': Atlas, 'occlusion': float32
    [T, T, 1] = 1 - the cosine-weighted share of the hemisphere about the row's normal that the mesh blocks within ``t_max``,
    'bent': float32 [T, T, 3] = the normalised sum of the unblocked directions (object space)}; texels no face owns, and rows that cast
    nothing (a zero normal), hold ``fill``.  ``atlas``: an Atlas laid out for the mesh (default: Atlas(size, F)); K directions of
    meshocclude.hemisphere_table; ``bias`` = None: 1e-4 x the bounding-box diagonal.  Row normals are the ones atlas_points returns
    (the mesh's vertex normals interpolated, else the face's own).  Chunk of faces by chunk of faces as bake_materials; a bake in
    chunks equals a bake in one call bit for bit.  One code path: device tensors (or ``device='cuda'``: the mesh is moved there) run
    the kernels and return device tensors; a numpy mesh runs the definition and returns numpy arrays."""
    v, f, vn = mesh_parts(mesh)
    _no_cpu_tensor(v, 'bake_occlusion')
    if on_device(v, device):
        v, f, vn = device_mesh(v, f, vn, device, prefix='atlas', widen_normals=True)
    else:
        v, f, vn = host_mesh(to_numpy(v), to_numpy(f), to_numpy(vn), prefix='atlas', widen_normals=True)
    atlas = Atlas(size, f.shape[0]) if atlas is None else atlas
    if atlas.F != f.shape[0]:
        raise ValueError('bake_occlusion: %d faces, the atlas was laid out for %d' % (f.shape[0], atlas.F))
    step = max(1, CHUNK_ROWS // atlas.K) if chunk_faces is None else int(chunk_faces)
    if step < 1:
        raise ValueError('bake_occlusion: chunk_faces = %d' % step)
    occluder = _Occluder(v, f, int(K), bias, t_max)          # (building the index also checks the faces' vertex indices)
    out = {'atlas': atlas}
    for f0 in range(0, atlas.F, step):
        f1 = min(f0 + step, atlas.F)
        with Phase(PHASE_EVENTS, 'points'):
            p, _, nrm = atlas_points(atlas, v, f, vn, f0, f1)
        occluder.bake(atlas, p, nrm, f0, f1, out, fill)
    return out


# ------------------------------------------------------------------------------------------------ the photographs on the atlas
class _Projector(object):
    """The views of a bake: the index (a MeshIndex for device tensors, the host twin for numpy arrays), the images, masks and bias, made
    (and, on the device, uploaded) once; ``bake`` turns one chunk of rows into texels of 'photo', 'photo_best', 'seen' and 'spread'."""

    def __init__(self, v, f, images, camera_mats, world_mats, masks, options):
        from . import meshdist as md, meshocclude as mo
        self.index = md._prepare((v, f), None, 'mesh')
        if isinstance(self.index, md.MeshIndex):
            dev = self.index.vertices.device
            place = lambda x: x if x is None or (torch.is_tensor(x) and x.is_cuda) else torch.from_numpy(np.array(to_numpy(x))).to(dev)
            images, masks = place(images), place(masks)
        else:
            images, masks = to_numpy(images), to_numpy(masks)
        self.images, self.masks, self.cameras = images, masks, (camera_mats, world_mats)
        self.options = dict(options)
        if self.options.get('bias') is None:
            self.options['bias'] = mo.default_bias(self.index)

    def bake(self, atlas, points, normals, f0, f1, out, fill):
        from . import meshproject as mp
        with Phase(PHASE_EVENTS, 'project'):
            res = mp.project_rows(self.index, points, normals, self.images, self.cameras[0], self.cameras[1], masks=self.masks, **self.options)
            maps = {'photo': mp.mean(res), 'photo_best': res.best_value, 'seen': res.n_seen[:, None], 'spread': mp.spread(res)}
            unseen = (res.n_seen == 0)[:, None]
            if torch.is_tensor(res.weight):
                rows = {k: torch.where(unseen, float(fill), m.float()) for k, m in maps.items()}
            else:
                rows = {k: np.where(unseen, np.float32(fill), m.astype(np.float32)) for k, m in maps.items()}
        with Phase(PHASE_EVENTS, 'scatter'):
            for name, r in rows.items():
                out[name] = atlas_scatter(atlas, r.contiguous() if torch.is_tensor(r) else np.ascontiguousarray(r), f0, f1, out.get(name),
                                          fill if name not in out else None)


def bake_views(mesh, images, camera_mats, world_mats, size=2048, atlas=None, masks=None, chunk_faces=None, fill=0.0, device=None, **options):
    """The photographs on the atlas of ``mesh``: per texel row, meshproject.project_rows over ``images`` [V, H, W, C] (uint8 or float32)
    of the cameras (camera_mats, world_mats) -> {'atlas': Atlas, 'photo': float32 [T, T, C] = the weighted mean of what the seeing views
    show, 'photo_best': [T, T, C] = the view of the largest weight alone, 'seen': [T, T, 1] = the number of seeing views as a float,
    'spread': [T, T, C] = the weighted standard deviation over the seeing views (photo-consistency)}; texels no face owns, and rows no
    view sees, hold ``fill``.  ``options``: project_rows' bias, cos_min, weight and frame.  Row normals are the ones atlas_points
    returns.  Chunk of faces by chunk of faces as bake_occlusion; a bake in chunks equals a bake in one call bit for bit.  One code
    path: device tensors (or ``device='cuda'``: the mesh is moved there) run the kernels and return device tensors; a numpy mesh
    runs the definition and returns numpy arrays."""
    if images is None:
        raise ValueError('bake_views: images are required (visibility alone: meshproject.face_visibility)')
    v, f, vn = mesh_parts(mesh)
    _no_cpu_tensor(v, 'bake_views')
    if on_device(v, device):
        v, f, vn = device_mesh(v, f, vn, device, prefix='atlas', widen_normals=True)
    else:
        v, f, vn = host_mesh(to_numpy(v), to_numpy(f), to_numpy(vn), prefix='atlas', widen_normals=True)
    atlas = Atlas(size, f.shape[0]) if atlas is None else atlas
    if atlas.F != f.shape[0]:
        raise ValueError('bake_views: %d faces, the atlas was laid out for %d' % (f.shape[0], atlas.F))
    step = max(1, CHUNK_ROWS // atlas.K) if chunk_faces is None else int(chunk_faces)
    if step < 1:
        raise ValueError('bake_views: chunk_faces = %d' % step)
    projector = _Projector(v, f, images, camera_mats, world_mats, masks, options)      # (building the index also checks the faces)
    out = {'atlas': atlas}
    for f0 in range(0, atlas.F, step):
        f1 = min(f0 + step, atlas.F)
        with Phase(PHASE_EVENTS, 'points'):
            p, _, nrm = atlas_points(atlas, v, f, vn, f0, f1)
        projector.bake(atlas, p, nrm, f0, f1, out, fill)
    return out


# ------------------------------------------------------------------------------------------------ the writer
def export_textured(path, mesh, baked, gamma=1.0):
    """Write the textured asset: ``name.obj`` (v, vt, f v/vt; vn and f v/vt/vn when the mesh has vertex normals), ``name.mtl``
    (map_Kd name_albedo.png; norm name_normal.png), the PNGs (bytes by ``to_img``; the albedo raised to 1 / gamma first, the normals
    stored as n / 2 + 0.5 -- OBJECT space, not tangent space) and ``name_specular.npy`` (float32 [T, T, C]: the SG weights have more
    than three channels and are not an image); with 'occlusion' / 'bent' (bake_occlusion) also ``name_ao.png`` (one channel, map_Ka) and
    ``name_bent.png`` (stored as n / 2 + 0.5 like the normals); with 'photo' and 'seen' (bake_views) also ``name_photo.png`` (C = 1, 3 or 4)
    and ``name_seen.png`` (one channel, the number of seeing views as a byte, 255 at most), named in one comment line.  ``path``: name.obj, or the name without an extension; ``baked``: bake_materials'
    result (only the maps it holds are written) -> {what: file path}."""
    from PIL import Image
    base = path[:-4] if path.lower().endswith('.obj') else path
    folder, name = os.path.dirname(os.path.abspath(base)), os.path.basename(base)
    os.makedirs(folder, exist_ok=True)
    atlas = baked['atlas']
    v, f, vn = host_mesh(*(to_numpy(x) for x in mesh_parts(mesh)), prefix='atlas', widen_normals=True)
    if f.shape[0] != atlas.F:
        raise ValueError('export_textured: %d faces, the atlas was laid out for %d' % (f.shape[0], atlas.F))
    files = {'obj': os.path.join(folder, name + '.obj'), 'mtl': os.path.join(folder, name + '.mtl')}
    mtl = ['newmtl %s' % name, 'Ka 0 0 0', 'Kd 1 1 1', 'Ks 0 0 0', 'illum 1']
    if 'albedo' in baked:
        a = to_numpy(baked['albedo']).astype(np.float32)
        if gamma != 1.0:
            a = np.power(a.clip(0, 1), np.float32(1.0 / gamma)).astype(np.float32)
        files['albedo'] = os.path.join(folder, name + '_albedo.png')
        Image.fromarray(to_img(a)).save(files['albedo'])
        mtl.append('map_Kd %s_albedo.png' % name)
    if 'normal' in baked:
        files['normal'] = os.path.join(folder, name + '_normal.png')
        Image.fromarray(to_img(to_numpy(baked['normal']).astype(np.float32) / np.float32(2.0) + np.float32(0.5))).save(files['normal'])
        mtl += ['# object-space normals, stored as n / 2 + 0.5', 'norm %s_normal.png' % name]
    if 'specular' in baked:
        files['specular'] = os.path.join(folder, name + '_specular.npy')
        np.save(files['specular'], to_numpy(baked['specular']).astype(np.float32))
        mtl.append('# specular: %s_specular.npy, float32 [T, T, C]' % name)
    if 'occlusion' in baked:
        files['ao'] = os.path.join(folder, name + '_ao.png')
        Image.fromarray(to_img(to_numpy(baked['occlusion']).astype(np.float32))[:, :, 0]).save(files['ao'])
        mtl += ['# ambient occlusion by the mesh itself, 1 = open', 'map_Ka %s_ao.png' % name]
    if 'bent' in baked:
        files['bent'] = os.path.join(folder, name + '_bent.png')
        Image.fromarray(to_img(to_numpy(baked['bent']).astype(np.float32) / np.float32(2.0) + np.float32(0.5))).save(files['bent'])
        mtl.append('# bent normals: %s_bent.png, object space, stored as n / 2 + 0.5' % name)
    if 'photo' in baked and 'seen' in baked:
        photo = to_img(to_numpy(baked['photo']).astype(np.float32))
        files['photo'] = os.path.join(folder, name + '_photo.png')
        Image.fromarray(photo[:, :, 0] if photo.shape[2] == 1 else photo).save(files['photo'])
        files['seen'] = os.path.join(folder, name + '_seen.png')
        Image.fromarray(np.clip(to_numpy(baked['seen']).astype(np.float32)[:, :, 0], 0.0, 255.0).astype(np.uint8)).save(files['seen'])
        mtl.append('# the photographs on the atlas: %s_photo.png (the mean over the seeing views), %s_seen.png (their number, 255 at most)'
                   % (name, name))
    with open(files['mtl'], 'w') as out:
        out.write('\n'.join(mtl) + '\n')
    uv = atlas_uv(atlas).reshape(-1, 2)
    with open(files['obj'], 'w') as out:
        out.write('mtllib %s.mtl\nusemtl %s\n' % (name, name))
        out.write(''.join('v %.17g %.17g %.17g\n' % tuple(p) for p in v))
        out.write(''.join('vt %.17g %.17g\n' % tuple(t) for t in uv))
        if vn is not None:
            out.write(''.join('vn %.9g %.9g %.9g\n' % tuple(m) for m in vn))
        corner = '%d/%d' if vn is None else '%d/%d/%d'
        for i, t in enumerate(f + 1):
            ids = [(t[k], 3 * i + k + 1) + ((t[k],) if vn is not None else ()) for k in range(3)]
            out.write('f %s\n' % ' '.join(corner % c for c in ids))
    return files
