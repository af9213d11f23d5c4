"""Inputs of the photometric-stereo tests (tests/test_ps_cpu.py, tests/test_ps_gpu.py): a Lambertian sphere with analytic normals,
random views of any pixel count, and a row of constructed pixels with expectations that follow by hand from the definition
(psnerf_amd/photostereo.py)."""
import functools

import numpy as np


def random_lights(L, seed, spread=0.6):
    """normalize((0, 0, 1) + spread * randn) -> float64 [L, 3]."""
    rs = np.random.RandomState(seed)
    l = np.array([0.0, 0.0, 1.0])[None] + spread * rs.randn(L, 3)
    return l / np.linalg.norm(l, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def sphere(H, W, L, seed, highlight=0.0):
    """Orthographic unit sphere seen along -z: the mask is the disc of radius 0.6 (normals up to 37 degrees off the axis, so that
    every masked pixel is lit by most of the lights), I = rho * max(n . l, 0) (+ highlight * max(n . h, 0)^60, h the half vector
    with the view direction (0, 0, 1)) -> dict(images float32 [L, H, W, 3], mask bool [H, W], normal float64 [H, W, 3] (0 outside),
    albedo float64 [H, W, 3], light_dir float64 [L, 3]).  Cached: the arrays are shared, do not write to them."""
    ys, xs = np.meshgrid((np.arange(H) + 0.5) / H * 2.0 - 1.0, (np.arange(W) + 0.5) / W * 2.0 - 1.0, indexing='ij')
    r2 = xs * xs + ys * ys
    mask = r2 < 0.36
    n = np.stack([xs, ys, np.sqrt(np.clip(1.0 - r2, 0.0, None))], -1)
    n = np.where(mask[..., None], n, 0.0)
    rho = np.stack([0.5 + 0.2 * np.sin(3.0 * xs), 0.4 + 0.2 * np.cos(2.0 * ys), 0.3 + 0.1 * xs * ys], -1)
    ld = random_lights(L, seed)
    cos = np.clip(np.einsum('hwc,lc->lhw', n, ld), 0.0, None)
    img = rho[None] * cos[..., None]
    if highlight:
        half = ld + np.array([0.0, 0.0, 1.0])[None]
        half = half / np.linalg.norm(half, axis=1, keepdims=True)
        img = img + highlight * (np.clip(np.einsum('hwc,lc->lhw', n, half), 0.0, None) ** 60)[..., None]
    img = np.where(mask[None, ..., None], img, 0.0).astype(np.float32)
    for a in (img, mask, n, rho, ld):
        a.setflags(write=False)
    return {'images': img, 'mask': mask, 'normal': n, 'albedo': rho, 'light_dir': ld}


def to_u8(images):
    return np.round(np.clip(images, 0.0, 1.0) * 255.0).astype(np.uint8)


def angular_error_deg(a, b, mask):
    cos = np.clip((a * b).sum(-1)[mask], -1.0, 1.0)
    return np.degrees(np.arccos(cos))


def random_view(L, H, W, seed, dtype=np.uint8, ties=False):
    """A view of any size: a smooth random normal field under random lights with noise, a third of the values dark, a mask with
    holes -> (images [L, H, W, 3] of ``dtype``, mask bool [H, W], light_dir float64 [L, 3]).  ``ties``: uint8 values from a set of
    four levels, so that most of a pixel's lights tie in g."""
    rs = np.random.RandomState(seed)
    ld = random_lights(L, seed + 1, spread=0.8)
    n = np.array([0.0, 0.0, 1.0])[None, None] + 0.5 * rs.randn(H, W, 3)
    n = n / np.linalg.norm(n, axis=-1, keepdims=True)
    rho = 0.2 + 0.7 * rs.rand(H, W, 3)
    img = rho[None] * np.clip(np.einsum('hwc,lc->lhw', n, ld), 0.0, None)[..., None] * (1.0 + 0.1 * rs.randn(L, H, W, 3))
    img = np.where(rs.rand(L, H, W, 1) < 0.3, 0.0, img)                 # shadows
    img = np.clip(img, 0.0, 1.2)
    mask = rs.rand(H, W) > 0.15
    if H * W == 1:
        mask[:] = True
    if ties:
        return (np.round(np.clip(img, 0.0, 1.0) * 3.0) * 60.0).astype(np.uint8), mask, ld
    return (to_u8(img) if dtype == np.uint8 else img.astype(np.float32)), mask, ld


# eight small-integer lights: 0 .. 3 lie in the plane z = 0, so a pixel that only they light has det A == 0 exactly
CONSTRUCTED_LIGHTS = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 2]], dtype=np.float64)


def constructed(dtype=np.uint8):
    """One row of six pixels under CONSTRUCTED_LIGHTS -> (images [8, 1, 6, 3], mask [1, 6]):
       0  two lit lights only                      1  lit by the four coplanar lights only
       2  outside the mask (with bright values)     3  the same byte in every light and channel: the tie rule decides the kept set
       4  Lambertian, normal (0, 0, 1) scaled       5  Lambertian, normal (1, 2, 2) / 3 scaled
    What each must give is worked out in tests/test_ps_cpu.py::test_constructed_pixels."""
    L = 8
    img = np.zeros((L, 1, 6, 3), np.float64)
    img[4, 0, 0] = img[6, 0, 0] = 100
    img[0:4, 0, 1] = 50
    img[:, 0, 2] = 200
    img[:, 0, 3] = 77
    for px, nrm in ((4, np.array([0.0, 0.0, 30.0])), (5, np.array([10.0, 20.0, 20.0]))):
        img[:, 0, px, :] = np.clip(CONSTRUCTED_LIGHTS @ nrm, 0.0, None)[:, None] * np.array([1.0, 2.0, 0.5])[None]
    mask = np.ones((1, 6), bool)
    mask[0, 2] = False
    assert img.max() <= 255 and np.all(img == np.round(img))
    return (img.astype(np.uint8) if dtype == np.uint8 else (img / 256.0).astype(np.float32)), mask
