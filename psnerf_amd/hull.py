"""Silhouette carving: dilated object masks, the visual hull of a set of views, and the carved value grid -- the step between "dense value
grid" and "marching cubes" that the reference's ``Extractor3D.generate_mesh(mask_loader=...)`` takes (stage1/model/extracting.py:120-127,
326-377): a lattice point is set to -30 when it lies in no image, or when some image that contains it shows background there after
the masks were dilated by ``disk(12)``.

The RULE is the reference's; the PROJECTION is not.  Its ``filter_points`` multiplies camera_mat @ world_mat @ scale_mat as if they
were UNISURF's world -> NDC matrices, while its own loader hands out camera-to-world poses and a pixel-unit K
(stage1/dataloading/dataset.py:125-127), so a faithful port would carve with the wrong projection on this project's data.  The
projection here is the inverse of the camera every other part of the project uses, ``stage1.rendering.pixel_rays`` and
``camera_origin`` (what shape_extract and meshrender render with), quirk included: both pixel axes are scaled by fx = K[0, 0].

Two implementations of one definition, as in meshclean.py and meshbake.py:
  * numpy arrays -> the ``host_*`` functions below, float64 / integer; they are the definition, and what the device path is tested
    against, byte for byte.
  * device tensors -> csrc/hull.hip: psn_mask_dilate (bit-packed rows, shift-OR doubling), psn_hull_points, psn_hull_grid.

Definition.
  Footprint: an int32 table of 2 r + 1 half-widths w[dy] >= 0, dy = -r .. r: the pixels (dx, dy) with |dx| <= w[dy], a row-convex
    shape symmetric in x.  ``disk_footprint(r)``: w = floor(sqrt(r^2 - dy^2)), skimage's disk(r); ``diamond_footprint(r)``:
    w = r - |dy|, what ndimage.binary_dilation(mask, iterations=r) with the default cross gives.  No half-width exceeds r.
  Dilation: masks [V, H, W] (non-zero = set) -> uint8 0 / 1, out[v, y, x] = OR over dy, |dx| <= w[dy] of m[v, y + dy, x + dx], where a
    pixel outside the image has the value ``border`` (0 or 1).  Erosion = NOT dilate(NOT m, border=1) (scipy's border_value=0 erosion).
    ``mask_valid`` = ~(dilate XOR erode) with the diamond: the loader's training.mask_valid rule (dataset.py:88-91).
  Projection of p through (camera_mat K, world_mat), float64, every product and sum a separate operation, in this order:
    d = p - o, o = world_mat[:3, 3];  x_c = (d0 R[0, c] + d1 R[1, c]) + d2 R[2, c], R = world_mat[:3, :3];  front = x_2 > 0;
    u = K[0, 2] + K[0, 0] (x_0 / x_2);  v = K[1, 2] + K[0, 0] (x_1 / x_2);  ix = floor(u + 0.5), iy = floor(v + 0.5) (integer pixel
    coordinates are pixel centres, as handoff.arange_pixels makes them);  in_image = front and 0 <= ix < W and 0 <= iy < H (the
    comparisons in float64, so a u or v that is not finite is not in the image).  ``scale_mat`` is accepted and ignored, exactly as
    meshrender.render_mesh documents.
  Carving: views in ascending order; carved_by = the lowest view whose image contains the point and whose mask is 0 there; -2 if no
    image contains the point; -1 if the point is kept; keep = carved_by == -1.  A view that does not see a point does not carve it,
    but some view must see it.
  Grid: value_grid float32 [n, n, n], x-major as ``_make_3d_grid``; ``axis`` [n] = the lattice coordinates of all three axes (the caller
    forms box_size * torch.linspace(-0.5, 0.5, n), exactly as the ``clip`` branch of the extractor does); ``value`` is written where
    keep is false, every other element keeps its bits; the number carved is returned.

Not built: carving inside the MISE rounds (the points are evaluated as before; only the dense grid is carved), and soft masks (a mask
pixel is set or not).
"""
import json

import numpy as np
import torch

from .meshcore import Mesh, to_numpy

CARVE_VALUE = -30.0


# ------------------------------------------------------------------------------------------------ footprints
def disk_footprint(r):
    """Half-widths of skimage.morphology.disk(r): dx^2 + dy^2 <= r^2."""
    r = _radius(r)
    dy = np.arange(-r, r + 1, dtype=np.int64)
    w = np.floor(np.sqrt((r * r - dy * dy).astype(np.float64))).astype(np.int64)
    w += ((w + 1) ** 2 + dy * dy <= r * r)      # (the square root of an integer, made exact)
    w -= (w * w + dy * dy > r * r)
    return w.astype(np.int32)


def diamond_footprint(r):
    """Half-widths of ``r`` iterations of the 4-neighbour cross: |dx| + |dy| <= r."""
    r = _radius(r)
    return (r - np.abs(np.arange(-r, r + 1))).astype(np.int32)


def _radius(r):
    if int(r) != r or int(r) < 0:
        raise ValueError('hull: footprint radius %r (an integer >= 0)' % (r,))
    return int(r)


def check_footprint(footprint):
    """-> (half-widths int32 [2 r + 1], r); ValueError for anything that is not a footprint."""
    w = np.asarray(footprint)
    if w.ndim != 1 or w.shape[0] % 2 != 1 or not np.issubdtype(w.dtype, np.integer):
        raise ValueError('hull: a footprint is an integer table of 2 r + 1 half-widths, got %s %s' % (w.dtype, w.shape))
    r = (w.shape[0] - 1) // 2
    if (w < 0).any() or (w > r).any():
        raise ValueError('hull: half-widths must lie in 0 .. r = %d, got %d .. %d' % (r, int(w.min()), int(w.max())))
    return np.ascontiguousarray(w, dtype=np.int32), r


def footprint_pixels(footprint):
    """The footprint as a bool image [2 r + 1, 2 r + 1]."""
    w, r = check_footprint(footprint)
    return np.abs(np.arange(-r, r + 1))[None, :] <= w[:, None]


# ------------------------------------------------------------------------------------------------ host path: the definition
def _host_masks(masks):
    m = np.asarray(masks)
    if m.ndim != 3 or m.shape[1] < 1 or m.shape[2] < 1:
        raise ValueError('hull: masks [V, H, W] expected, got %s' % (m.shape,))
    return m != 0


def host_dilate(masks, footprint, border=0):
    """masks [V, H, W] (non-zero = set) -> uint8 0 / 1 [V, H, W]."""
    w, r = check_footprint(footprint)
    if border not in (0, 1):
        raise ValueError('hull: border=%r (0 or 1)' % (border,))
    m = _host_masks(masks)
    V, H, W = m.shape
    padded = np.pad(m, ((0, 0), (r, r), (r, r)), 'constant', constant_values=bool(border)).astype(np.int64)
    run = np.concatenate([np.zeros((V, H + 2 * r, 1), dtype=np.int64), np.cumsum(padded, axis=2)], axis=2)   # run[x] = sum of [0, x)
    out = np.zeros((V, H, W), dtype=bool)
    for i in range(2 * r + 1):                               # row y + dy of the image is row y + i of the padded one
        k = int(w[i])
        rows = run[:, i:i + H]
        out |= (rows[:, :, r + k + 1:r + k + 1 + W] - rows[:, :, r - k:r - k + W]) > 0
    return out.astype(np.uint8)


def host_erode(masks, footprint):
    return (1 - host_dilate(~_host_masks(masks), footprint, border=1)).astype(np.uint8)


def _views(camera_mats, world_mats, n_views=None):
    """-> float64 [V, 16]: R row-major (9), o (3), K[0, 0], K[0, 2], K[1, 2], 0.  camera_mats [3, 3] / [4, 4] (one K for every view) or
    [V, 3 | 4, 3 | 4]; world_mats [V, 3 | 4, 4] (or one matrix).  float32 matrices are widened exactly."""
    k = np.asarray(to_numpy(camera_mats), dtype=np.float64)
    p = np.asarray(to_numpy(world_mats), dtype=np.float64)
    p = p[None] if p.ndim == 2 else p
    if p.ndim != 3 or p.shape[1] not in (3, 4) or p.shape[2] != 4:
        raise ValueError('hull: world_mats [V, 4, 4] (camera to world) expected, got %s' % (p.shape,))
    V = p.shape[0] if n_views is None else int(n_views)
    k = k[None] if k.ndim == 2 else k
    if k.ndim != 3 or k.shape[1] < 3 or k.shape[2] < 3 or k.shape[0] not in (1, V) or p.shape[0] != V or V < 1:
        raise ValueError('hull: camera_mats %s and world_mats %s do not describe %d views' % (k.shape, p.shape, V))
    k = np.broadcast_to(k, (V,) + k.shape[1:])
    table = np.zeros((V, 16), dtype=np.float64)
    table[:, 0:9] = p[:, :3, :3].reshape(V, 9)
    table[:, 9:12] = p[:, :3, 3]
    table[:, 12], table[:, 13], table[:, 14] = k[:, 0, 0], k[:, 0, 2], k[:, 1, 2]
    return table


def _host_points(points):
    p = np.asarray(points)
    if p.ndim != 2 or p.shape[1] != 3 or p.dtype not in (np.float32, np.float64):
        raise ValueError('hull: points float32 or float64 [Q, 3] expected, got %s %s' % (p.dtype, p.shape))
    return p.astype(np.float64)


def _project_uv(p, view):
    """The definition's arithmetic for float64 points [Q, 3] and one row of the view table, up to the image-plane position
    -> (u, v, front).  The one statement of the projection: ``_project`` below and meshproject.host_project_rows both go through it."""
    R, o, fx, cx, cy = view[0:9].reshape(3, 3), view[9:12], view[12], view[13], view[14]
    with np.errstate(all='ignore'):
        d0, d1, d2 = p[:, 0] - o[0], p[:, 1] - o[1], p[:, 2] - o[2]
        x0 = (d0 * R[0, 0] + d1 * R[1, 0]) + d2 * R[2, 0]
        x1 = (d0 * R[0, 1] + d1 * R[1, 1]) + d2 * R[2, 1]
        x2 = (d0 * R[0, 2] + d1 * R[1, 2]) + d2 * R[2, 2]
        u = cx + fx * (x0 / x2)
        v = cy + fx * (x1 / x2)
        return u, v, x2 > 0


def _project(p, view):
    """_project_uv rounded to the nearest pixel centre -> (floor(u + 0.5), floor(v + 0.5), front)."""
    u, v, front = _project_uv(p, view)
    with np.errstate(all='ignore'):
        return np.floor(u + 0.5), np.floor(v + 0.5), front


def host_project(points, camera_mat, world_mat, hw=None, scale_mat=None):
    """points [Q, 3] -> (ix int64 [Q], iy int64 [Q], in_image bool [Q]); ``hw`` = (H, W), or None for an unbounded image plane.  Where
    in_image is false, ix = iy = -1.  ``scale_mat`` is accepted and ignored."""
    del scale_mat
    fu, fv, front = _project(_host_points(points), _views(camera_mat, world_mat, 1)[0])
    H, W = (2.0 ** 31, 2.0 ** 31) if hw is None else (float(hw[0]), float(hw[1]))
    lo = -2.0 ** 31 if hw is None else 0.0
    with np.errstate(invalid='ignore'):
        inside = front & (fu >= lo) & (fu < W) & (fv >= lo) & (fv < H)
    ix = np.where(inside, fu, -1.0).astype(np.int64)
    iy = np.where(inside, fv, -1.0).astype(np.int64)
    return ix, iy, inside


def _host_carve(p, m, table):
    V, H, W = m.shape
    carved_by = np.full(p.shape[0], -2, dtype=np.int32)
    for v in range(V):
        fu, fv, front = _project(p, table[v])
        with np.errstate(invalid='ignore'):
            inside = front & (fu >= 0.0) & (fu < float(W)) & (fv >= 0.0) & (fv < float(H))
        at = np.nonzero(inside & (carved_by < 0))[0]          # (a point a lower view carved is settled)
        seen = m[v, fv[at].astype(np.int64), fu[at].astype(np.int64)]
        carved_by[at] = np.where(seen, -1, v)
    return carved_by == -1, carved_by


def host_carve_points(points, masks, camera_mats, world_mats):
    """-> (keep bool [Q], carved_by int32 [Q])."""
    m = _host_masks(masks)
    return _host_carve(_host_points(points), m, _views(camera_mats, world_mats, m.shape[0]))


def _host_axis(axis, n):
    a = np.asarray(to_numpy(axis))
    if a.shape != (n,) or a.dtype not in (np.float32, np.float64):
        raise ValueError('hull: axis float [%d] expected, got %s %s' % (n, a.dtype, a.shape))
    return a.astype(np.float64)


def _check_grid(grid):
    n = grid.shape[0] if grid.ndim == 3 else 0
    if tuple(grid.shape) != (n, n, n) or n < 2:
        raise ValueError('hull: a cubic value grid [n, n, n], n >= 2, expected, got %s' % (tuple(grid.shape),))
    return n


def lattice_points(axis):
    """The [n^3, 3] float64 points of the lattice, x-major."""
    a = np.asarray(axis, dtype=np.float64)
    n = a.shape[0]
    return np.stack([np.repeat(a, n * n), np.tile(np.repeat(a, n), n), np.tile(a, n * n)], axis=1)


def host_carve_grid(value_grid, axis, masks, camera_mats, world_mats, value=CARVE_VALUE):
    """In place on a float32 numpy grid [n, n, n] -> the number of lattice points carved."""
    if not isinstance(value_grid, np.ndarray) or value_grid.dtype != np.float32:
        raise ValueError('hull: a float32 numpy value grid expected')
    n = _check_grid(value_grid)
    keep, _ = host_carve_points(lattice_points(_host_axis(axis, n)), masks, camera_mats, world_mats)
    carved = ~keep.reshape(n, n, n)
    value_grid[carved] = np.float32(value)
    return int(carved.sum())


# ------------------------------------------------------------------------------------------------ device path
def _device_masks(masks, device=None):
    """uint8 [V, H, W] on ``device`` (default: where the masks are) from a uint8 / bool device tensor, a CPU tensor or a numpy array."""
    if not torch.is_tensor(masks):
        masks = torch.from_numpy(np.ascontiguousarray(_host_masks(masks)))
    if masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.bool):
        raise ValueError('hull: masks uint8 or bool [V, H, W] expected, got %s %s' % (masks.dtype, tuple(masks.shape)))
    return masks.to(masks.device if device is None else device).contiguous().view(torch.uint8)


def _device_views(camera_mats, world_mats, n_views, device):
    return torch.from_numpy(_views(camera_mats, world_mats, n_views)).to(device)


# ------------------------------------------------------------------------------------------------ public surface
def dilate_masks(masks, footprint, border=0):
    """Device tensor -> psn_mask_dilate (uint8 device tensor); numpy array -> host_dilate."""
    if torch.is_tensor(masks) and masks.is_cuda:
        from . import hip
        return hip.mask_dilate(_device_masks(masks), check_footprint(footprint)[0], border)
    return host_dilate(to_numpy(masks), footprint, border)


def erode_masks(masks, footprint):
    if torch.is_tensor(masks) and masks.is_cuda:
        from . import hip
        return hip.mask_dilate(_device_masks(masks), check_footprint(footprint)[0], 1, invert=True)
    return host_erode(to_numpy(masks), footprint)


def mask_valid(mask, iterations=2):
    """~(dilate XOR erode) with the diamond of ``iterations``: bool, of the mask's shape ([H, W] or [V, H, W])."""
    fp = diamond_footprint(iterations)
    m = mask if mask.ndim == 3 else mask[None]
    valid = dilate_masks(m, fp) == erode_masks(m, fp)
    return valid if mask.ndim == 3 else valid[0]


def carve_points(points, masks, camera_mats, world_mats):
    """-> (keep bool [Q], carved_by int32 [Q]): device tensors for device points (psn_hull_points), numpy arrays otherwise."""
    if torch.is_tensor(points) and points.is_cuda:
        from . import hip
        m = _device_masks(masks, points.device)
        keep, carved_by = hip.hull_points(points.contiguous(), _device_views(camera_mats, world_mats, m.shape[0], points.device), m)
        return keep.view(torch.bool), carved_by
    return host_carve_points(to_numpy(points), to_numpy(masks), camera_mats, world_mats)


def carve_grid(value_grid, axis, masks, camera_mats, world_mats, value=CARVE_VALUE):
    """In place -> the number carved: a float32 device grid goes through psn_hull_grid, a numpy grid through the definition."""
    if torch.is_tensor(value_grid) and value_grid.is_cuda:
        from . import hip
        n = _check_grid(value_grid)
        dev = value_grid.device
        m = _device_masks(masks, dev)
        ax = torch.as_tensor(_host_axis(axis, n) if not (torch.is_tensor(axis) and axis.is_cuda) else axis.to(torch.float64)).to(dev)
        count = hip.hull_grid(value_grid, ax.contiguous(), _device_views(camera_mats, world_mats, m.shape[0], dev), m, value)
        return int(count.item())
    if torch.is_tensor(value_grid):
        raise ValueError('hull: a device tensor or a numpy array expected for the value grid')
    return host_carve_grid(value_grid, axis, to_numpy(masks), camera_mats, world_mats, value)


class VisualHull(object):
    """The dilated masks and cameras of a set of views: ``masks`` [V, H, W] (non-zero = object; a numpy array stays on the host, a
    device tensor on its device), ``camera_mats`` [3, 3] or [V, 3, 3] (pixel-unit K), ``world_mats`` [V, 4, 4] (camera to world, OpenCV
    axes: what the loader hands out as 'img.world_mat').  The masks are dilated once, here."""

    def __init__(self, masks, camera_mats, world_mats, footprint=None):
        self.footprint = check_footprint(disk_footprint(12) if footprint is None else footprint)[0]
        if torch.is_tensor(masks) and not masks.is_cuda:
            masks = masks.numpy()
        masks = masks if masks.ndim == 3 else masks[None]
        self.views = _views(camera_mats, world_mats, masks.shape[0])      # (checks the matrices against the number of masks)
        self.camera_mats, self.world_mats = to_numpy(camera_mats), to_numpy(world_mats)
        self.masks = dilate_masks(masks if torch.is_tensor(masks) else (np.asarray(masks) != 0), self.footprint)

    @property
    def device(self):
        return self.masks.device if torch.is_tensor(self.masks) else torch.device('cpu')

    @classmethod
    def from_loader(cls, loader, footprint=None, device=None):
        """``loader``: an iterable of the data loader's dicts ('img.mask', 'img.camera_mat', 'img.world_mat'; with or without the batch
        dimension of 1 a DataLoader adds).  ``device``: where the dilated masks are to live (None: the host)."""
        masks, ks, poses = [], [], []
        for data in loader:
            m, k, p = (np.asarray(to_numpy(data[key])) for key in ('img.mask', 'img.camera_mat', 'img.world_mat'))
            masks.append(m.reshape(m.shape[-2:]) != 0)
            ks.append(k.reshape(k.shape[-2:]))
            poses.append(p.reshape(p.shape[-2:]))
        if not masks:
            raise ValueError('VisualHull.from_loader: the loader is empty')
        return cls(_place(np.stack(masks), device), np.stack(ks), np.stack(poses), footprint)

    @classmethod
    def from_params(cls, params_json, mask_dir, views=None, footprint=None, device=None):
        """The dataset's params.json ('K', 'pose_c2w' in OpenGL axes, 'n_view'), read as tools/render_mesh.py reads it, and
        mask_dir/view_VV.png (imgmetrics.load_image).  ``views``: view numbers from 1 (default: all)."""
        K, poses, views, _ = cameras_from_params(params_json, views, 'VisualHull.from_params')
        return cls(_place(masks_from_dir(mask_dir, views), device), K, poses, footprint)

    def _on(self, device):
        """The dilated masks where ``device`` is (moved once and kept when that is not where they were given)."""
        device = torch.device(device)
        if device.type != 'cuda':
            return to_numpy(self.masks)
        if not (torch.is_tensor(self.masks) and self.masks.device == device):
            self.masks = torch.as_tensor(to_numpy(self.masks)).to(device)
        return self.masks

    def carve_points(self, points):
        dev = points.device if torch.is_tensor(points) else 'cpu'
        return carve_points(points, self._on(dev), self.camera_mats, self.world_mats)

    def contains(self, points):
        """keep [Q] of points [Q, 3] (float32 or float64; device tensor or numpy array, answered where the points are)."""
        return self.carve_points(points)[0]

    def carve_grid(self, grid, axis, value=CARVE_VALUE):
        dev = grid.device if torch.is_tensor(grid) else 'cpu'
        return carve_grid(grid, axis, self._on(dev), self.camera_mats, self.world_mats, value)

    def indicator(self, resolution, box_size, device=None):
        """-> (grid float32 [n, n, n], n = resolution + 1: +1 inside the hull, -1 outside and on the outermost lattice layer; axis)."""
        n = int(resolution) + 1
        axis = box_size * torch.linspace(-0.5, 0.5, n)
        device = self.device if device is None else torch.device(device)
        grid = torch.ones((n, n, n), dtype=torch.float32, device=device) if device.type == 'cuda' else np.ones((n, n, n), dtype=np.float32)
        self.carve_grid(grid, axis, value=-1.0)
        for face in (0, n - 1):
            grid[face], grid[:, face], grid[:, :, face] = -1.0, -1.0, -1.0
        return grid, axis

    def mesh(self, resolution, box_size, device=None):
        """The visual hull as a mesh: marching cubes at iso 0 on ``indicator`` (the empty outer layer closes a hull that reaches the
        box).  On the masks' device (or ``device``) through the device kernels, otherwise through the numpy definitions."""
        from .stage1.extracting import host_marching_cubes, to_world
        grid, _ = self.indicator(resolution, box_size, device)
        if torch.is_tensor(grid):
            from . import hip
            v, f = hip.marching_cubes(grid, 0.0, box_size)
            return Mesh(v.cpu().numpy(), f.cpu().numpy())
        v, f = host_marching_cubes(grid, 0.0)
        return Mesh(to_world(v, grid.shape[0], box_size), f)


def cameras_from_params(params_json, views=None, what='cameras_from_params'):
    """The dataset's params.json ('K', 'pose_c2w' in OpenGL axes, 'n_view', optionally 'imhw'), read as tools/render_mesh.py reads it
    -> (K float32 [3, 3], world_mats float32 [n, 4, 4] in OpenCV axes, the view numbers from 1, (H, W) or None).  ``views``: view
    numbers from 1 (default: all)."""
    with open(params_json) as f:
        para = json.load(f)
    K = np.array(para['K']).astype(np.float32)
    pose = np.array(para['pose_c2w']).astype(np.float32).copy()
    pose[:, :3, 1:3] *= -1.0                                          # OpenGL -> OpenCV, stage1/dataloading/dataset.py:56
    views = list(views) if views else list(range(1, int(para.get('n_view', len(pose))) + 1))
    for vi in views:
        if not 1 <= vi <= len(pose):
            raise ValueError('%s: view %d of %d' % (what, vi, len(pose)))
    hw = tuple(int(x) for x in para['imhw']) if 'imhw' in para else None
    return K, pose[[vi - 1 for vi in views]], views, hw


def masks_from_dir(mask_dir, views):
    """mask_dir/view_VV.png (imgmetrics.load_image) of the view numbers ``views`` -> bool [n, H, W]."""
    import os
    from .imgmetrics import load_image
    masks = []
    for vi in views:
        m = load_image(os.path.join(mask_dir, 'view_%02d.png' % vi))
        masks.append((m.reshape(m.shape[0], m.shape[1], -1)[..., 0]) != 0)
    return np.stack(masks)


def _place(masks, device):
    return masks if device is None or torch.device(device).type != 'cuda' else torch.from_numpy(masks).to(device)
