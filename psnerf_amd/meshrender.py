"""Looking at a mesh from a camera: depth, normal and silhouette maps of a dataset view and binary shadow maps, by casting rays
against the triangles (meshdist.MeshIndex.ray_cast -> csrc/meshray.hip on the device, meshdist.host_ray_cast on the host).  The
reference has nothing of the kind: all of its maps come from marching the occupancy network (stage1/model/rendering.py:297-408),
so what these functions show is the EXPORTED ASSET, not the network.

The camera convention is the reference's, through the very functions ``Renderer.shape_extract`` uses: the origin is
``stage1.rendering.camera_origin`` (the translation of world_mat) and the directions are ``stage1.rendering.pixel_rays``, which
divides both pixel axes by fx (the reference's quirk, stage1/model/common.py:220) and does not normalise.  They are formed in the
dtype of the inputs and then converted to float64, in which all the geometry runs.

As everywhere in meshdist: a mesh on the device (a MeshIndex, device tensors, or ``device='cuda'``) takes the device path and
returns device tensors; anything else takes the numpy definition and returns CPU tensors."""
import functools

import numpy as np
import torch

from . import meshdist as md
from .meshcore import to_numpy


def _index(mesh, device):
    """A Mesh, a (vertices, faces) pair, a MeshIndex or a _HostMesh -> MeshIndex or _HostMesh."""
    return md._prepare(mesh, device, 'mesh')


def _cast(index, origins, directions, t_min, t_max, any_hit=False, sort=True, n_tests=None):
    """index.ray_cast with torch tensors out on either path (the host path computes in numpy)."""
    if isinstance(index, md.MeshIndex):
        dev = index.vertices.device
        return index.ray_cast(origins.to(dev), directions.to(dev), t_min, t_max, any_hit=any_hit, n_tests=n_tests, sort=sort)
    out = index.ray_cast(origins, directions, t_min, t_max, any_hit=any_hit)
    return tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in out)


def _mesh_tensors(index):
    if isinstance(index, md.MeshIndex):
        return index.vertices, index.faces
    return torch.from_numpy(index.vertices), torch.from_numpy(index.faces)


@torch.no_grad()
def render_mesh(mesh, pixels, camera_mat, world_mat, scale_mat=None, vertex_normals=None, device=None, sort_rays=True, textures=None,
                atlas=None):
    """The mesh as the camera of a dataset view sees it.  pixels [1, N, 2] (or [N, 2]) in the units of camera_mat, camera_mat
    [1, 3|4, 3|4], world_mat [1, 4, 4] (camera to world, the dataset's 'img.camera_mat' / 'img.world_mat').  ``scale_mat`` is taken for
    the signature's sake and, exactly as in ``Renderer.shape_extract`` (and stage1/model/common.py:205-207), not used.
    -> dict of [N] / [N, 3] float64 tensors (bool / int64 where noted), zeros wherever the ray misses, as shape_extract gives them:
        mask     bool, the silhouette
        t        the ray parameter along the unnormalised direction
        depth    t |d|, the Euclidean distance from the camera
        points   origin + t d
        tri      int64, the triangle hit (-1 on a miss)
        normals  unit length and turned to face the camera: the geometric normal of the triangle, or with ``vertex_normals``
                 [V, 3] (e.g. Extractor3D.estimate_normals) their barycentric interpolation, normalised
    ``mesh``: a Mesh, a (vertices, faces) pair or a ready MeshIndex (one index serves every view).
    ``textures`` ({name: float32 [T, T, C]}, e.g. the maps of meshbake.bake_materials) with their ``atlas`` (a meshbake.Atlas): the
    dict also holds, under each name, the texture looked up bilinearly at the first hits (meshbake.atlas_sample) -> float64 [N, C],
    NaN wherever the ray misses.  Without them the dict is what it always was."""
    from .stage1.rendering import camera_origin, pixel_rays
    index = _index(mesh, device)
    if pixels.dim() == 2:
        pixels = pixels[None]
    n = pixels.shape[1]
    o = camera_origin(n, world_mat)[0].to(torch.float64)
    d = pixel_rays(pixels, camera_mat, world_mat)[0].to(torch.float64)
    t, tri, bary, hit = _cast(index, o, d, 0.0, float('inf'), sort=sort_rays)
    o, d = o.to(t.device), d.to(t.device)
    zero = torch.zeros((), dtype=torch.float64, device=t.device)
    t = torch.where(hit, t, zero)
    v, f = _mesh_tensors(index)
    corners = f[tri.clamp(min=0)]
    if vertex_normals is None:
        a = v[corners[:, 0]]
        nrm = torch.linalg.cross(v[corners[:, 1]] - a, v[corners[:, 2]] - a)
    else:
        vn = torch.as_tensor(vertex_normals).to(device=t.device, dtype=torch.float64).reshape(-1, 3)
        if vn.shape[0] != v.shape[0]:
            raise ValueError('render_mesh: %d vertex normals for %d vertices' % (vn.shape[0], v.shape[0]))
        w = torch.where(hit[:, None], bary, zero)
        nrm = w[:, 0:1] * vn[corners[:, 0]] + w[:, 1:2] * vn[corners[:, 1]] + w[:, 2:3] * vn[corners[:, 2]]
    length = nrm.norm(dim=1, keepdim=True)
    nrm = torch.where(length > 0, nrm / torch.where(length > 0, length, torch.ones_like(length)), zero)
    away = (nrm * d).sum(dim=1, keepdim=True) > 0
    nrm = torch.where(hit[:, None], torch.where(away, -nrm, nrm), zero)
    out = {'mask': hit, 't': t, 'depth': t * d.norm(dim=1), 'points': torch.where(hit[:, None], o + t[:, None] * d, zero),
           'tri': tri, 'normals': nrm}
    if textures:
        out.update(_sample_textures(textures, atlas, tri, bary, out))
    return out


def _sample_textures(textures, atlas, tri, bary, out):
    """Each texture at the first hits, on the path the cast took: device tensors through the kernel, otherwise the numpy definition."""
    from . import meshbake
    if atlas is None:
        raise ValueError('render_mesh: textures need the atlas they were baked on')
    sampled = {}
    for name, tex in textures.items():
        if name in out:
            raise ValueError('render_mesh: the texture name %r is a key of the result' % name)
        if tri.is_cuda:
            tex = torch.as_tensor(tex).to(device=tri.device, dtype=torch.float32).contiguous()
            sampled[name] = meshbake.atlas_sample(atlas, tri, bary, tex)
        else:
            tex = np.asarray(to_numpy(tex))
            sampled[name] = torch.from_numpy(meshbake.host_atlas_sample(atlas, tri.numpy(), bary.numpy(), tex.astype(np.float32, copy=False)))
    return sampled


@functools.lru_cache(maxsize=8)
def tile_pixels(H, W, tile=8):
    """The pixels (x, y) of an H x W image in tile order: tiles row by row, the pixels of a tile row by row -> int64 [H W, 2] (kept
    per image size: not to be written to).  A wave's 64 rays are then one 8 x 8 patch of the image and walk neighbouring cells."""
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    key = ((ys // tile) * ((W + tile - 1) // tile) + xs // tile) * (tile * tile) + (ys % tile) * tile + xs % tile
    order = np.argsort(key.ravel(), kind='stable')
    return torch.from_numpy(np.stack([xs.ravel()[order], ys.ravel()[order]], axis=1))


@torch.no_grad()
def render_view(mesh, camera_mat, world_mat, H, W, scale_mat=None, vertex_normals=None, device=None, textures=None, atlas=None):
    """render_mesh over the whole H x W pixel grid (integer pixel coordinates, as handoff.arange_pixels makes them), handed over
    in 8 x 8 tiles -> the same dict with [H, W] / [H, W, 3] maps (and [H, W, C] per texture of ``textures``)."""
    px = tile_pixels(H, W)
    out = render_mesh(mesh, px[None].to(device=camera_mat.device, dtype=camera_mat.dtype), camera_mat, world_mat, scale_mat, vertex_normals,
                      device, sort_rays=False, textures=textures, atlas=atlas)
    maps = {}
    for key, val in out.items():
        full = torch.zeros((H, W) + tuple(val.shape[1:]), dtype=val.dtype, device=val.device)
        full[px[:, 1].to(val.device), px[:, 0].to(val.device)] = val
        maps[key] = full
    return maps


@torch.no_grad()
def mesh_light_visibility(mesh, points, light_dir, lnear=0.1, lfar=3.5, device=None, n_tests=None):
    """Is the light visible from the point, going by the MESH: bool [L, Ns], False where the segment from points[s] + lnear l to
    points[s] + lfar l along the unit light direction l = light_dir[L] meets a triangle (any-hit rays).  points [Ns, 3], light_dir
    [L, 3] (normalised here); the defaults and the [L, Ns] layout are those of ``Renderer.light_visibility``.
    This is BINARY OCCLUSION BY THE MESH.  It is not the network's transmittance (``Renderer.light_visibility`` composites the
    occupancy along the shadow ray and returns a value in [0, 1]), and nothing in training or in shape_extract uses it."""
    index = _index(mesh, device)
    p = torch.as_tensor(points).to(torch.float64).reshape(-1, 3)
    l = torch.as_tensor(light_dir).to(torch.float64).reshape(-1, 3)
    l = l / l.norm(dim=1, keepdim=True)
    n_l, n_s = l.shape[0], p.shape[0]
    o = p.to(l.device)[None].expand(n_l, n_s, 3).reshape(-1, 3)
    d = l[:, None].expand(n_l, n_s, 3).reshape(-1, 3)
    _, _, _, hit = _cast(index, o, d, float(lnear), float(lfar), any_hit=True, n_tests=n_tests)
    return ~hit.reshape(n_l, n_s)
