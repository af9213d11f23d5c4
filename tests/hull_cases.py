"""Inputs of the silhouette-carving tests (tests/test_hull_cpu.py, tests/test_hull_gpu.py): mask patterns, footprints, random and
constructed cameras, the analytic sphere rigs and the analytic sphere "model".  numpy only; every result is cached and must be
left unchanged by its users."""
import functools

import numpy as np
import torch

from psnerf_amd import hull

RADII = (0, 1, 2, 12)
SHAPES = {'disk': hull.disk_footprint, 'diamond': hull.diamond_footprint}
PATTERNS = ('empty', 'full', 'corners', 'centre', 'random', 'checker')
SPHERE_RADIUS = 0.5
BOX_SIZE = 2.4


# ------------------------------------------------------------------------------------------------ masks
def pattern(name, V, H, W, seed=0):
    """uint8 [V, H, W] with values 0 and 255 (a non-zero byte is a set pixel, whatever its value)."""
    m = np.zeros((V, H, W), dtype=np.uint8)
    if name == 'full':
        m[:] = 255
    elif name == 'corners':
        m[:, 0, 0] = m[:, 0, -1] = m[:, -1, 0] = m[:, -1, -1] = 255
    elif name == 'centre':
        m[:, H // 2, W // 2] = 255
    elif name == 'random':
        m[np.random.RandomState(seed + 7 * H + W).rand(V, H, W) < 0.02] = 1
    elif name == 'checker':
        m[:, (np.arange(H)[:, None] + np.arange(W)[None, :]) % 2 == 0] = 255
    elif name != 'empty':
        raise KeyError(name)
    if V > 1 and name in ('corners', 'centre'):
        m[1] = np.roll(m[1], (H // 3, W // 3), axis=(0, 1))        # (the views differ)
    return m


def brute_dilate(masks, footprint, border):
    """The definition of the dilation as a loop over the offsets of the footprint."""
    w = np.asarray(footprint)
    r = (len(w) - 1) // 2
    m = np.pad(np.asarray(masks) != 0, ((0, 0), (r, r), (r, r)), 'constant', constant_values=bool(border))
    V, H, W = np.asarray(masks).shape
    out = np.zeros((V, H, W), dtype=bool)
    for dy in range(-r, r + 1):
        for dx in range(-int(w[dy + r]), int(w[dy + r]) + 1):
            out |= m[:, r + dy:r + dy + H, r + dx:r + dx + W]
    return out.astype(np.uint8)


# ------------------------------------------------------------------------------------------------ cameras
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """Camera-to-world [4, 4] float32, OpenCV axes (x right, y down, z forward): the columns of R are the camera axes in the world."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m.astype(np.float32)


def intrinsics(fx, H, W, fy=None):
    """Pixel-unit K [3, 3] float32 with the principal point at the centre of the pixel grid.  fy is carried but unused by the project's
    camera (both axes are scaled by fx)."""
    return np.array([[fx, 0.0, (W - 1) / 2.0], [0.0, fx if fy is None else fy, (H - 1) / 2.0], [0.0, 0.0, 1.0]], dtype=np.float32)


def random_camera(seed, H, W):
    g = np.random.RandomState(seed)
    eye = g.randn(3)
    eye *= (1.5 + g.rand()) / np.linalg.norm(eye)
    up = g.randn(3)
    K = intrinsics(60.0 + 80.0 * g.rand(), H, W, fy=33.0)          # (an fy that would be noticed if it were used)
    K[0, 2] += np.float32(g.rand() * 3.0)
    K[1, 2] -= np.float32(g.rand() * 3.0)
    return K, look_at(eye, g.randn(3) * 0.1, up)


def axis_camera(H, W, fx=64.0):
    """An axis-aligned camera at (0, 0, -2) looking along +z with power-of-two intrinsics: every product of the projection is exact."""
    K = np.array([[fx, 0.0, 16.0], [0.0, fx, 8.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    c2w = np.eye(4, dtype=np.float32)
    c2w[2, 3] = -2.0
    return K, c2w


def edge_points(H, W, fx=64.0):
    """For axis_camera: float64 points whose u + 0.5 is exactly 0, just below 0, exactly W and just below W (v in the image), then
    the same for v and H -> (points [8, 3], in_image bool [8])."""
    K, c2w = axis_camera(H, W, fx)
    depth = 2.0                                                     # x_2 of the points (z = 0)
    def at(u, v):
        return [(u - 16.0) / fx * depth, (v - 8.0) / fx * depth, 0.0]
    eps = 2.0 ** -20
    p = [at(-0.5, 3.0), at(-0.5 - eps, 3.0), at(W - 0.5, 3.0), at(W - 0.5 - eps, 3.0),
         at(5.0, -0.5), at(5.0, -0.5 - eps), at(5.0, H - 0.5), at(5.0, H - 0.5 - eps)]
    return np.array(p, dtype=np.float64), np.array([True, False, False, True, True, False, False, True])


def odd_points(world_mat):
    """Constructed points for a camera: behind it, at its centre, NaN, and far in front of it on the axis."""
    o, zax = world_mat[:3, 3].astype(np.float64), world_mat[:3, 2].astype(np.float64)
    return np.stack([o - 1.5 * zax, o, np.array([np.nan, 0.0, 0.0]), o + np.array([0.0, np.nan, 0.0]), o + 1.0 * zax])


# ------------------------------------------------------------------------------------------------ the sphere rigs
RIG_H, RIG_W, RIG_FX, RIG_DISTANCE = 80, 64, 90.0, 2.0


@functools.lru_cache(maxsize=None)
def sphere_rig(V):
    """V cameras on a ring of radius 2 in the z = 0 plane looking at the centre, image x along the ring; images 64 wide and 80 high,
    fx = 90; the analytic silhouettes of the sphere of radius 0.5 at the pixel centres -> (masks uint8 [V, H, W] 0 / 255, K [3, 3],
    world_mats [V, 4, 4]).  The silhouette's radius is 23 pixels: dilated by 12 it is wider than the image (32 pixels to either side of
    the centre) and narrower than it is high, so the 8-view hull is one piece that the top and bottom of the images cut off."""
    K = intrinsics(RIG_FX, RIG_H, RIG_W)
    poses = np.stack([look_at((RIG_DISTANCE * np.cos(a), RIG_DISTANCE * np.sin(a), 0.0)) for a in 2.0 * np.pi * (np.arange(V) + 0.25) / V])
    ys, xs = np.meshgrid(np.arange(RIG_H, dtype=np.float64), np.arange(RIG_W, dtype=np.float64), indexing='ij')
    # the ray through a pixel centre in camera axes is (qx, qy, 1); it meets the sphere iff its distance to the centre (0, 0, D) is <= r
    q = np.stack([(xs - float(K[0, 2])) / RIG_FX, (ys - float(K[1, 2])) / RIG_FX, np.ones_like(xs)], axis=-1)
    along = q[..., 2] * RIG_DISTANCE / np.linalg.norm(q, axis=-1)
    dist2 = RIG_DISTANCE ** 2 - along ** 2
    one = (dist2 <= SPHERE_RADIUS ** 2).astype(np.uint8) * 255
    masks = np.repeat(one[None], V, axis=0)
    for a in (masks, K, poses):
        a.setflags(write=False)
    return masks, K, poses


@functools.lru_cache(maxsize=None)
def lattice(n=33, box_size=BOX_SIZE):
    """(axis float32-exact float64 [n], points float64 [n^3, 3] x-major): what the extractor's grid uses."""
    axis = (box_size * torch.linspace(-0.5, 0.5, n)).numpy().astype(np.float64)
    p = hull.lattice_points(axis)
    p.setflags(write=False)
    return axis, p


@functools.lru_cache(maxsize=None)
def sphere_carve(V, radius, n=33):
    """The definition on the sphere rig -> (keep, carved_by) over lattice(n)."""
    masks, K, poses = sphere_rig(V)
    dil = hull.host_dilate(masks, hull.disk_footprint(radius))
    keep, by = hull.host_carve_points(lattice(n)[1], dil, K, poses)
    keep.setflags(write=False)
    by.setflags(write=False)
    return keep, by


class SphereModel(object):
    """A "model" with the reference's call signature: -logit = 8 (radius - |p|) (positive inside, as the extractor's values are)."""

    def __init__(self, radius=SPHERE_RADIUS):
        self.radius = radius

    def to(self, device):
        return self

    def eval(self):
        return self

    def __call__(self, p, ray_d=None, return_logits=False, **kwargs):
        assert return_logits
        return (8.0 * (self.radius - p.to(torch.float32).norm(dim=-1))).unsqueeze(-1)


def sphere_field(n, box_size=BOX_SIZE):
    axis = (box_size * torch.linspace(-0.5, 0.5, n)).numpy().astype(np.float64)
    p = hull.lattice_points(axis)
    return (8.0 * (SPHERE_RADIUS - np.linalg.norm(p, axis=1))).astype(np.float32).reshape(n, n, n)


def write_dataset(folder, V):
    """The sphere rig as the dataset's files: folder/params.json ('K', 'pose_c2w' in OpenGL axes, 'n_view', 'imhw') and
    folder/mask/view_VV.png -> (params path, mask directory)."""
    import json
    import os
    from PIL import Image
    masks, K, poses = sphere_rig(V)
    gl = poses.copy()
    gl[:, :3, 1:3] *= -1.0
    mask_dir = os.path.join(str(folder), 'mask')
    os.makedirs(mask_dir)
    for v in range(V):
        Image.fromarray(np.ascontiguousarray(masks[v])).save(os.path.join(mask_dir, 'view_%02d.png' % (v + 1)))
    params = os.path.join(str(folder), 'params.json')
    with open(params, 'w') as f:
        json.dump({'K': K.tolist(), 'pose_c2w': gl.tolist(), 'n_view': V, 'imhw': [RIG_H, RIG_W]}, f)
    return params, mask_dir
