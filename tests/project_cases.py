"""Shared constructions of the view-projection tests (tests/test_project_cpu.py, tests/test_project_gpu.py): camera rings around the
meshes of tests/raycast_cases.py and tests/occlusion_cases.py, images, masks, and the cases the device is held to with the
definition's answer computed once and handed out read-only.  Everything is numpy and deterministic.

Cost.  The definition is a brute force over rows x views x faces segment-triangle pairs for the pairs that pass the four cheap
tests; every case stays below about 3e7 of them, so a test takes seconds."""
import functools

import numpy as np

from tests import hull_cases as hc, occlusion_cases as oc, raycast_cases as rc
from psnerf_amd import hull
from psnerf_amd import meshdist as md
from psnerf_amd import meshocclude as mo
from psnerf_amd import meshproject as mp

SPHERE_SCALE = hc.SPHERE_RADIUS                    # rc.icosphere is a unit sphere; hull_cases.sphere_rig looks at one of radius 0.5


def sphere(level=2):
    v, f = rc.icosphere(level)
    return v * SPHERE_SCALE, f


def cameras(v, V, H, W, seed=0):
    """V cameras on a spiral around the bounding box of the vertices ``v``, between 55 degrees below and above its equator, looking at
    points near its centre, the object filling most of the image -> (K float32 [3, 3], world_mats float32 [V, 4, 4])."""
    g = np.random.RandomState(1000 + seed)
    lo, hi = v.min(axis=0), v.max(axis=0)
    centre, half = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)
    distance = 2.5 * half
    k = np.arange(V)
    azimuth = 2.0 * np.pi * ((k * 0.6180339887498949) % 1.0) + 0.3
    elevation = np.deg2rad(55.0) * (2.0 * (k + 0.5) / V - 1.0)
    eyes = centre + distance * np.stack([np.cos(elevation) * np.cos(azimuth), np.cos(elevation) * np.sin(azimuth), np.sin(elevation)], axis=1)
    poses = np.stack([hc.look_at(e, centre + 0.1 * half * g.randn(3)) for e in eyes])
    K = hc.intrinsics(0.42 * min(H, W) * distance / half, H, W, fy=33.0)
    K[0, 2] += np.float32(0.37)
    K[1, 2] -= np.float32(0.21)
    return K, poses


def images(V, H, W, C, dtype, seed=0):
    g = np.random.RandomState(2000 + seed)
    if dtype == np.uint8:
        return g.randint(0, 256, (V, H, W, C)).astype(np.uint8)
    return (g.random_sample((V, H, W, C)) * 2.0 - 0.5).astype(np.float32)


def masks_for(V, H, W, seed=0):
    """uint8 [V, H, W], about a tenth of the pixels cleared, set pixels of several non-zero values."""
    g = np.random.RandomState(3000 + seed)
    return (g.randint(1, 256, (V, H, W)) * (g.random_sample((V, H, W)) > 0.1)).astype(np.uint8)


def closed_form_convex(p, n, K, poses, H, W, cos_min=0.0):
    """For a convex mesh with outward row normals and a positive bias nothing blocks: view v sees a row iff the row is in front of the
    camera, inside the footprint and faces it -> bool [R, V], written directly (matrix products, not the definition's statement)."""
    K, poses = np.asarray(K, dtype=np.float64), np.asarray(poses, dtype=np.float64)
    out = np.zeros((len(p), len(poses)), dtype=bool)
    for v, pose in enumerate(poses):
        x = (p - pose[:3, 3]) @ pose[:3, :3]
        with np.errstate(all='ignore'):
            pu, pv = K[0, 2] + K[0, 0] * x[:, 0] / x[:, 2], K[1, 2] + K[0, 0] * x[:, 1] / x[:, 2]
        e = pose[:3, 3] - p
        c = (n * e).sum(axis=1) / np.linalg.norm(e, axis=1)
        out[:, v] = (x[:, 2] > 0) & (pu >= 0) & (pu <= W - 1) & (pv >= 0) & (pv <= H - 1) & (c > cos_min)
    return out


# ------------------------------------------------------------------------------------------------ the device's cases
# name -> (mesh, rows R, views V, image dtype (None: no images), C, masks, weight, frame, bias (None: the default), rows on edges).
# Between them: R in {1, 63, 64, 65, 255, 257, 513 (one above two workgroups)}, V in {1, 2, 32, 33, 256}, uint8 and float32, C in
# {0, 1, 3, 4}, with and without masks, both weights, both frames, bias 0 and the default, every mesh.
CASES = {
    'icosphere, R 257, V 33, u8 C3, masks': ('icosphere(2)', 257, 33, np.uint8, 3, True, 'cosine', 'raw', None, False),
    'icosphere, R 513, V 2, f32 C4, uniform, no bias': ('icosphere(2)', 513, 2, np.float32, 4, False, 'uniform', 'raw', 0.0, True),
    'icosphere, one row, one view, f32 C1': ('icosphere(2)', 1, 1, np.float32, 1, False, 'cosine', 'raw', 1e-3, False),
    'icosphere, R 64, V 256, u8 C1, masks': ('icosphere(2)', 64, 256, np.uint8, 1, True, 'cosine', 'raw', None, False),
    'icosphere, R 255, V 32, f32 C3, camera normals': ('icosphere(2)', 255, 32, np.float32, 3, False, 'cosine', 'camera_normal', None, False),
    'icosphere in and out, R 65, V 33, no images, masks': ('icosphere(2) inward', 65, 33, None, 0, True, 'cosine', 'raw', None, False),
    'snapped cube, R 257, V 32, u8 C4, on edges, no bias': ('snapped cube', 257, 32, np.uint8, 4, False, 'cosine', 'raw', 0.0, True),
    'marching cubes, R 63, V 33, f32 C3, camera normals, uniform': ('marching cubes', 63, 33, np.float32, 3, True, 'uniform', 'camera_normal', None,
                                                                   False),
    'two oversize triangles, R 64, V 32, u8 C3': ('two oversize triangles', 64, 32, np.uint8, 3, False, 'uniform', 'raw', None, False),
    'degenerate triangles, R 65, V 1, no images': ('degenerate triangles', 65, 1, None, 0, False, 'cosine', 'raw', 0.0, False),
    'every face oversize, R 63, V 2, f32 C1': ('icosphere(1), every face oversize', 63, 2, np.float32, 1, True, 'cosine', 'raw', None, True),
    'corner, R 65, V 33, f32 C3': ('corner', 65, 33, np.float32, 3, False, 'cosine', 'raw', None, True),
}
H, W = 37, 29


def case_mesh(mesh):
    return oc.corner_mesh() if mesh == 'corner' else oc.case_mesh(mesh)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: v, f, points, normals, images, masks, K, poses, views (the [V, 16] table), hw, weight, frame, bias (a float), cos_min, dead (the
    rows that see nothing by rule) and ``want`` = the definition's Projection with bits; all read-only."""
    mesh, R, V, dtype, C, masked, weight, frame, bias, on_edges = CASES[name]
    v, f = case_mesh(mesh)
    seed = len(name)
    faces = np.arange(6 * 2 * 36) if mesh == 'snapped cube' else None
    p, n, _ = oc.surface_rows(v, f, R, seed, faces=faces, on_edges=on_edges)
    cos_min = 0.0
    if mesh.endswith('inward'):                                  # every other row looks inward, and no view is turned away by the facing test:
        n[::2] = -n[::2]                                         # whatever is unseen in this case is outside a footprint, masked or BLOCKED
        cos_min = -2.0
    if R >= 63:
        p, n, dead = oc.degenerate_rows(p, n)
    else:
        dead = np.zeros(R, dtype=bool)
    K, poses = cameras(v, V, H, W, seed)
    if R == 1 and V == 1:                                        # the one view looks at the one row from along its normal
        poses = hc.look_at(p[0] + 2.0 * n[0], p[0])[None]
    img = None if dtype is None else images(V, H, W, C, dtype, seed)
    masks = masks_for(V, H, W, seed) if masked else None
    if bias is None:
        bias = mo.default_bias(md._HostMesh(v, f))
    want = mp.host_project_rows(v, f, p, n, img, K, poses, masks=masks, bias=bias, cos_min=cos_min, weight=weight, frame=frame, bits=True,
                                hw=(H, W))
    out = dict(v=v, f=f, points=p, normals=n, images=img, masks=masks, K=K, poses=poses, views=hull._views(K, poses), hw=(H, W), weight=weight,
               frame=frame, bias=float(bias), cos_min=cos_min, dead=dead, want=want, C=C, V=V)
    for x in (p, n, dead, img, masks, K, poses) + tuple(want):
        if x is not None:
            x.setflags(write=False)
    return out
