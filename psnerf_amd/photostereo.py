"""Calibrated photometric stereo: the per-view normal map that stage 1 is regularised with (``training.normal_loss``, ``img.normal``,
``img.norm_mask``), the per-light intensities that ``inten_normalize`` needs and light_avg.py's light-averaged training image, from one
view's images under L known directional lights.

The lights are the dataset's CALIBRATED ones (``params.json: light_direction``, in the view's OpenGL camera frame, which is the frame
``img.normal`` is defined in).  This replaces SDPS-Net's NORMAL estimate, which the reference reads from ``sdps_out*/outnpy``; it does
not replace SDPS-Net's light estimate: with uncalibrated data there is nothing here to run.

Two implementations of one definition, as in imgmetrics.py / mesheval.py:
  * numpy inputs -> the float64 functions below (``host_*``): explicit loops over the lights, so the summation order is stated.
  * device tensors -> csrc/photostereo.hip (psn_ps_normals, psn_ps_light_intensity, psn_ps_light_average), float64 arithmetic in the
    definition's order: normals, albedo, validity and kept counts equal the definition bit for bit.

The definition, per masked pixel (``host_photometric_stereo``):
  1. v[l, c] = I[l, c] / e[l, c] (e = light_int, 1 without it; a byte u is the double u / 255.0), g[l] = (v[l,0] + v[l,1]) + v[l,2].
  2. light l is LIT if g[l] > dark; n_lit = their number.
  3. rank[i] = #{lit j : g[j] < g[i] or (g[j] == g[i] and j < i)}: ascending in g, ties by light index.
  4. light i is KEPT if it is lit and floor(low * n_lit) <= rank[i] < n_lit - floor(high * n_lit): shadows go by ``dark``, penumbra and
     highlights by the trim.
  5. over the kept lights in ascending index: A = sum l l^T (six entries, each product formed and then added), b = sum l * g[l].
  6. m = adj(A) b with
         c00 = a11 a22 - a12 a12   c01 = a02 a12 - a01 a22   c02 = a01 a12 - a02 a11
         c11 = a00 a22 - a02 a02   c12 = a01 a02 - a00 a12   c22 = a00 a11 - a01 a01
         det = (a00 c00 + a01 c01) + a02 c02
         m0 = (c00 b0 + c01 b1) + c02 b2   m1 = (c01 b0 + c11 b1) + c12 b2   m2 = (c02 b0 + c12 b1) + c22 b2
     (the solution is m / det; only its direction is used, and det > 0 for a valid pixel).
  7. valid: kept >= min_lights, det > cond * t^3 with t = ((a00 + a11) + a22) / 3 and t^3 = (t t) t, and |m| > 0,
     |m| = sqrt((m0 m0 + m1 m1) + m2 m2).
  8. n = m / |m|.
  9. albedo[c] = sum v[l, c] s[l] / sum s[l]^2 with s[l] = max((n0 lx + n1 ly) + n2 lz, 0) over the kept lights in index order; 0 if
     the denominator is 0.
 10. invalid or unmasked pixels: normal 0, albedo 0, valid 0.  ``kept`` is the kept count of every masked pixel (0 outside the mask).
``light_dir`` is used as given and NOT normalised.
"""
import numpy as np
import torch

MAX_LIGHTS = 256     # PSN_PS_MAX_LIGHTS
MIN_LIGHTS = 3       # PSN_PS_MIN_LIGHTS
DEFAULTS = dict(low=0.1, high=0.25, dark=0.0, min_lights=3, cond=1e-4)


# ------------------------------------------------------------------------------------------------ host path: the definition
def _check_params(L, low, high, min_lights):
    if not MIN_LIGHTS <= L <= MAX_LIGHTS:
        raise ValueError('photometric stereo: L = %d lights (%d .. %d)' % (L, MIN_LIGHTS, MAX_LIGHTS))
    if not (0.0 <= low < 1.0 and 0.0 <= high < 1.0 and low + high < 1.0):
        raise ValueError('photometric stereo: low = %r, high = %r (both in [0, 1), low + high < 1)' % (low, high))
    if min_lights < MIN_LIGHTS:
        raise ValueError('photometric stereo: min_lights = %d (at least %d)' % (min_lights, MIN_LIGHTS))


def _as_double_images(images):
    """[L, H, W, 3] uint8 or float32 -> float64: a byte u is u / 255.0, a float is converted exactly."""
    images = np.asarray(images)
    if images.ndim != 4 or images.shape[3] != 3:
        raise ValueError('photometric stereo: images [L, H, W, 3] expected, got %s' % (images.shape,))
    if images.dtype == np.uint8:
        return images.astype(np.float64) / 255.0
    if images.dtype == np.float32:
        return images.astype(np.float64)
    raise ValueError('photometric stereo: images must be uint8 or float32, got %s' % images.dtype)


def _light_table(t, L, name):
    """None, [L] or [L, 3] -> None or float64 [L, 3]."""
    if t is None:
        return None
    t = np.asarray(t, dtype=np.float64)
    if t.shape == (L,):
        t = np.repeat(t[:, None], 3, axis=1)
    if t.shape != (L, 3):
        raise ValueError('photometric stereo: %s [%d] or [%d, 3] expected, got %s' % (name, L, L, t.shape))
    return np.ascontiguousarray(t)


def _pos(x):
    return np.where(x > 0.0, x, 0.0)


def host_photometric_stereo(images, mask, light_dir, light_int=None, low=0.1, high=0.25, dark=0.0, min_lights=3, cond=1e-4):
    """The definition (module docstring) -> (normal [H, W, 3] float64, albedo [H, W, 3] float64, valid [H, W] uint8, kept [H, W] int32)."""
    I = _as_double_images(images)
    L, H, W = I.shape[:3]
    _check_params(L, low, high, min_lights)
    ld = np.asarray(light_dir, dtype=np.float64)
    if ld.shape != (L, 3):
        raise ValueError('photometric stereo: light_dir [%d, 3] expected, got %s' % (L, ld.shape))
    e = _light_table(light_int, L, 'light_int')
    inside = (np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0).reshape(-1)
    N = H * W
    I = I.reshape(L, N, 3)
    with np.errstate(all='ignore'):
        v = I if e is None else I / e[:, None, :]
        g = (v[:, :, 0] + v[:, :, 1]) + v[:, :, 2]                       # [L, N]
        lit = g > dark
        n_lit = lit.sum(0).astype(np.int64)
        rank = np.zeros((L, N), dtype=np.int64)
        j_index = np.arange(L)[:, None]
        for i in range(L):      # (a count of integers: its order does not matter)
            before = (g < g[i][None]) | ((g == g[i][None]) & (j_index < i))
            rank[i] = (lit & before).sum(0)
        lo = np.floor(low * n_lit.astype(np.float64)).astype(np.int64)
        hi = n_lit - np.floor(high * n_lit.astype(np.float64)).astype(np.int64)
        keep = lit & (rank >= lo[None]) & (rank < hi[None])
        kept = keep.sum(0).astype(np.int32)
        z = np.zeros(N)
        a00, a01, a02, a11, a12, a22, b0, b1, b2 = (z.copy() for _ in range(9))
        for l in range(L):
            k = keep[l]
            lx, ly, lz = ld[l]
            a00 = np.where(k, a00 + lx * lx, a00)
            a01 = np.where(k, a01 + lx * ly, a01)
            a02 = np.where(k, a02 + lx * lz, a02)
            a11 = np.where(k, a11 + ly * ly, a11)
            a12 = np.where(k, a12 + ly * lz, a12)
            a22 = np.where(k, a22 + lz * lz, a22)
            b0 = np.where(k, b0 + lx * g[l], b0)
            b1 = np.where(k, b1 + ly * g[l], b1)
            b2 = np.where(k, b2 + lz * g[l], b2)
        c00 = a11 * a22 - a12 * a12
        c01 = a02 * a12 - a01 * a22
        c02 = a01 * a12 - a02 * a11
        c11 = a00 * a22 - a02 * a02
        c12 = a01 * a02 - a00 * a12
        c22 = a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        m0 = (c00 * b0 + c01 * b1) + c02 * b2
        m1 = (c01 * b0 + c11 * b1) + c12 * b2
        m2 = (c02 * b0 + c12 * b1) + c22 * b2
        t = ((a00 + a11) + a22) / 3.0
        norm = np.sqrt((m0 * m0 + m1 * m1) + m2 * m2)
        valid = inside & (kept >= min_lights) & (det > cond * ((t * t) * t)) & (norm > 0.0)
        n0, n1, n2 = m0 / norm, m1 / norm, m2 / norm
        num = [z.copy() for _ in range(3)]
        den = z.copy()
        for l in range(L):
            k = keep[l]
            lx, ly, lz = ld[l]
            s = _pos((n0 * lx + n1 * ly) + n2 * lz)
            for c in range(3):
                num[c] = np.where(k, num[c] + v[l, :, c] * s, num[c])
            den = np.where(k, den + s * s, den)
        rho = [np.where(den == 0.0, 0.0, num[c] / den) for c in range(3)]
    normal = np.where(valid[:, None], np.stack([n0, n1, n2], -1), 0.0)
    albedo = np.where(valid[:, None], np.stack(rho, -1), 0.0)
    kept = np.where(inside, kept, 0).astype(np.int32)
    return normal.reshape(H, W, 3), albedo.reshape(H, W, 3), valid.astype(np.uint8).reshape(H, W), kept.reshape(H, W)


def host_light_intensity(images, mask, normal, albedo, valid, light_dir, dark=0.0, bright=1.0, relative_to=None):
    """Per light and channel e[l, c] = sum_p I m / sum_p m^2 with m = albedo[p, c] * max((n0 lx + n1 ly) + n2 lz, 0), over the valid
    pixels whose I[l, p, c] lies in the open interval (dark, bright); 0 where the denominator is 0 -> float64 [L, 3].  ``mask`` only
    restricts ``valid`` further (None: no restriction).  ``relative_to``: divide every row by that row (light_avg.py:55)."""
    I = _as_double_images(images)
    L = I.shape[0]
    I = I.reshape(L, -1, 3)
    ld = np.asarray(light_dir, dtype=np.float64)
    n = np.asarray(normal, dtype=np.float64).reshape(-1, 3)
    rho = np.asarray(albedo, dtype=np.float64).reshape(-1, 3)
    ok = np.asarray(valid).reshape(-1) != 0
    if mask is not None:
        ok = ok & (np.asarray(mask).reshape(-1) != 0)
    e = np.zeros((L, 3))
    for l in range(L):
        s = _pos((n[:, 0] * ld[l, 0] + n[:, 1] * ld[l, 1]) + n[:, 2] * ld[l, 2])
        for c in range(3):
            use = ok & (I[l, :, c] > dark) & (I[l, :, c] < bright)
            m = rho[:, c] * s
            num, den = float(np.sum((I[l, :, c] * m)[use])), float(np.sum((m * m)[use]))
            e[l, c] = 0.0 if den == 0.0 else num / den
    return _relative(e, relative_to)


def _relative(e, relative_to):
    if relative_to is None:
        return e
    with np.errstate(all='ignore'):
        return e / e[relative_to][None, :]


def round_u8(x):
    """light_avg.py:64,67: (x.clip(0, 1) * 255).round().astype(uint8), half to even."""
    return np.round(np.clip(x, 0.0, 1.0) * 255.0).astype(np.uint8)


def host_light_average(images, mask, relat_int=None):
    """light_avg.py:58-67: limg[l] = (u / 255.0) * mask, divided by relat_int[l] ([L] or [L, 3]) when given; the mean is the sequential
    sum over l in index order divided by L (what np.mean(list, axis=0) does) -> (mean float64 [H, W, 3], mean_u8 [H, W, 3], the
    normalised images uint8 [L, H, W, 3] or None without relat_int)."""
    I = _as_double_images(images)
    L, H, W = I.shape[:3]
    r = _light_table(relat_int, L, 'relat_int')
    m = (np.ones((H, W)) if mask is None else (np.asarray(mask) != 0).astype(np.float64))[..., None]
    norm = np.zeros((L, H, W, 3), np.uint8) if r is not None else None
    acc = None
    with np.errstate(all='ignore'):
        for l in range(L):
            limg = I[l] * m
            if r is not None:
                limg = limg / r[l][None, None, :]
                norm[l] = round_u8(limg)
            acc = limg if acc is None else acc + limg
        mean = acc / float(L)
    return mean, round_u8(mean), norm


def feedback_intensity(e):
    """The intensities as the next iteration divides by them: an entry that is not positive (a light that no valid pixel saw) is 1."""
    if torch.is_tensor(e):
        return torch.where(e > 0.0, e, torch.ones_like(e))
    return np.where(e > 0.0, e, 1.0)


def host_estimate(images, mask, light_dir, n_iter=1, low=0.1, high=0.25, dark=0.0, min_lights=3, cond=1e-4, bright=1.0, light_int=None):
    """Alternates the two: normals with the current intensities (none at first, unless ``light_int`` is given), then intensities from
    them, ``n_iter`` times -> dict(normal, albedo, valid, kept, light_int [L, 3])."""
    out = None
    for _ in range(max(1, int(n_iter))):
        normal, albedo, valid, kept = host_photometric_stereo(images, mask, light_dir, light_int, low, high, dark, min_lights, cond)
        e = host_light_intensity(images, mask, normal, albedo, valid, light_dir, dark, bright)
        out = {'normal': normal, 'albedo': albedo, 'valid': valid, 'kept': kept, 'light_int': e}
        light_int = feedback_intensity(e)
    return out


# ------------------------------------------------------------------------------------------------ one code path over both
def _is_host(images):
    return not torch.is_tensor(images)


def _dev_table(t, L, name, device):
    """None, or a [L] / [L, 3] tensor or array -> None or a contiguous float64 [L, 3] device tensor."""
    if t is None:
        return None
    t = torch.as_tensor(t, dtype=torch.float64).to(device)
    if tuple(t.shape) == (L,):
        t = t[:, None].expand(L, 3)
    if tuple(t.shape) != (L, 3):
        raise RuntimeError('photometric stereo: %s [%d] or [%d, 3] expected, got %s' % (name, L, L, tuple(t.shape)))
    return t.contiguous()


def _dev_images(images, mask):
    if not images.is_cuda:
        raise RuntimeError('photometric stereo: images must be a HIP device tensor (host arrays: pass numpy arrays for the host_* definition)')
    if images.dim() != 4 or images.shape[3] != 3:
        raise RuntimeError('photometric stereo: images [L, H, W, 3] expected, got %s' % (tuple(images.shape),))
    L, H, W = (int(x) for x in images.shape[:3])
    if mask is not None:
        mask = torch.as_tensor(mask).to(images.device)
        if tuple(mask.shape) != (H, W):
            raise RuntimeError('photometric stereo: mask [%d, %d] expected, got %s' % (H, W, tuple(mask.shape)))
        mask = (mask != 0).contiguous()
    return images.contiguous(), mask, L, H, W


def photometric_stereo(images, mask, light_dir, light_int=None, low=0.1, high=0.25, dark=0.0, min_lights=3, cond=1e-4, path='auto'):
    """host_photometric_stereo for numpy arrays; for device tensors the same through psn_ps_normals (bit for bit) ->
    (normal [H, W, 3] float64, albedo [H, W, 3] float64, valid [H, W] uint8, kept [H, W] int32), arrays or device tensors as the input.
    ``path`` (device only): 'auto', 'tile' (g in LDS, L <= hip.PS_TILE_LIGHTS) or 'reform' (g re-formed from the images)."""
    if _is_host(images):
        return host_photometric_stereo(images, mask, light_dir, light_int, low, high, dark, min_lights, cond)
    from . import hip
    images, mask, L, H, W = _dev_images(images, mask)
    ld = _dev_table(light_dir, L, 'light_dir', images.device)
    e = _dev_table(light_int, L, 'light_int', images.device)
    n, a, v, k = hip.ps_normals(images.reshape(L, H * W, 3), None if mask is None else mask.reshape(-1), ld, e, low, high, dark, min_lights,
                                cond, path=path)
    return n.reshape(H, W, 3), a.reshape(H, W, 3), v.reshape(H, W), k.reshape(H, W)


def light_intensity(images, mask, normal, albedo, valid, light_dir, dark=0.0, bright=1.0, relative_to=None):
    """host_light_intensity for numpy arrays; for device tensors psn_ps_light_intensity (fixed-order partial sums: two runs give the
    same bits) -> float64 [L, 3]."""
    if _is_host(images):
        return host_light_intensity(images, mask, normal, albedo, valid, light_dir, dark, bright, relative_to)
    from . import hip
    images, mask, L, H, W = _dev_images(images, mask)
    dev = images.device
    ok = torch.as_tensor(valid).to(dev).reshape(-1) != 0
    if mask is not None:
        ok = ok & mask.reshape(-1)
    n = torch.as_tensor(normal, dtype=torch.float64).to(dev).reshape(H * W, 3).contiguous()
    a = torch.as_tensor(albedo, dtype=torch.float64).to(dev).reshape(H * W, 3).contiguous()
    e = hip.ps_light_intensity(images.reshape(L, H * W, 3), n, a, ok.contiguous(), _dev_table(light_dir, L, 'light_dir', dev), dark, bright)[0]
    return e if relative_to is None else e / e[relative_to][None, :]


def light_average(images, mask, relat_int=None):
    """host_light_average for numpy arrays; for device tensors psn_ps_light_average (bit for bit, byte for byte) ->
    (mean float64 [H, W, 3], mean_u8 [H, W, 3], normalised images uint8 [L, H, W, 3] or None)."""
    if _is_host(images):
        return host_light_average(images, mask, relat_int)
    from . import hip
    images, mask, L, H, W = _dev_images(images, mask)
    r = _dev_table(relat_int, L, 'relat_int', images.device)
    mean, mean_u8, norm = hip.ps_light_average(images.reshape(L, H * W, 3), None if mask is None else mask.reshape(-1), r)
    return mean.reshape(H, W, 3), mean_u8.reshape(H, W, 3), None if norm is None else norm.reshape(L, H, W, 3)


def estimate(images, mask, light_dir, n_iter=1, low=0.1, high=0.25, dark=0.0, min_lights=3, cond=1e-4, bright=1.0, light_int=None):
    """host_estimate over either kind of input -> dict(normal, albedo, valid, kept, light_int)."""
    if _is_host(images):
        return host_estimate(images, mask, light_dir, n_iter, low, high, dark, min_lights, cond, bright, light_int)
    out = None
    for _ in range(max(1, int(n_iter))):
        normal, albedo, valid, kept = photometric_stereo(images, mask, light_dir, light_int, low, high, dark, min_lights, cond)
        e = light_intensity(images, mask, normal, albedo, valid, light_dir, dark, bright)
        out = {'normal': normal, 'albedo': albedo, 'valid': valid, 'kept': kept, 'light_int': e}
        light_int = feedback_intensity(e)
    return out


def stage1_normals(result):
    """What the stage-1 data dictionary carries for the normal loss (the reference's dataset.py:129-131), from estimate()'s or
    photometric_stereo()'s result (a dict with 'normal' and 'valid', or the 4-tuple): {'img.normal': float32 [3, H, W],
    'img.norm_mask': float32 [H, W]}, in the camera frame of the light directions -- the frame the trainer maps to the world."""
    normal, valid = (result['normal'], result['valid']) if isinstance(result, dict) else (result[0], result[2])
    if torch.is_tensor(normal):
        return {'img.normal': normal.to(torch.float32).permute(2, 0, 1).contiguous(), 'img.norm_mask': (valid != 0).to(torch.float32)}
    return {'img.normal': np.ascontiguousarray(np.asarray(normal).astype(np.float32).transpose(2, 0, 1)),
            'img.norm_mask': (np.asarray(valid) != 0).astype(np.float32)}
