"""Calibrated photometric stereo on the GPU (csrc/photostereo.hip through psnerf_amd/hip.py and psnerf_amd/photostereo.py) against the
float64 numpy definition in the same module.  Outputs land in guarded buffers (NaN / 0xFF), so a pixel the kernel skips shows.

Gates, with where they come from:
  psn_ps_normals        normal, albedo, valid, kept: EQUAL, bit for bit, on both paths (LDS tile / g re-formed).  The kernel does the
                        definition's float64 operations in the definition's order with contraction off; division and square root are
                        correctly rounded on both sides; the ranking is integer counting.
  psn_ps_light_intensity  within n_pixels * 2^-50 relative of the definition: numerator and denominator are sums of at most n_pixels
                        non-negative float64 terms added in another order than numpy's (each within n_pixels * 2^-53 of the exact
                        sum on either side), the quotient adds one rounding.  Two runs equal bit for bit.
  psn_ps_light_average  mean bit for bit, both uint8 outputs byte for byte (a sequential sum in the definition's order).
"""
import functools

import numpy as np
import pytest
import torch

from tests import ps_cases
from psnerf_amd import photostereo as ps

pytestmark = pytest.mark.gpu
SETTINGS = (dict(low=0.1, high=0.25, dark=0.0), dict(low=0.0, high=0.3, dark=0.05))


@functools.lru_cache(maxsize=None)
def host_normals(L, H, W, dtype_name, ties, with_int, setting):
    """The inputs of one case and the definition's result, computed once -> (images, mask, light_dir, light_int or None, result)."""
    images, mask, ld = ps_cases.random_view(L, H, W, seed=L * 1000 + H * W, dtype=np.dtype(dtype_name).type, ties=ties)
    e = None
    if with_int:
        e = 0.5 + np.random.RandomState(L).rand(L, 3)
    res = ps.host_photometric_stereo(images, mask, ld, e, **SETTINGS[setting])
    for a in (images, mask, ld) + tuple(res):
        a.setflags(write=False)
    return images, mask, ld, e, res


def dev(a, cuda):
    return None if a is None else torch.from_numpy(np.array(a)).to(cuda)


def guarded(N, cuda):
    return (torch.full((N, 3), float('nan'), dtype=torch.float64, device=cuda), torch.full((N, 3), float('nan'), dtype=torch.float64, device=cuda),
            torch.full((N,), 255, dtype=torch.uint8, device=cuda), torch.full((N,), -7, dtype=torch.int32, device=cuda))


def same_bits(t, a):
    """A device tensor and a numpy array of the same dtype hold the same bytes (NaN-safe, -0.0 is not +0.0)."""
    return np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(a).view(np.uint8))


def check_normals(cuda, images, mask, ld, e, res, setting, what):
    from psnerf_amd import hip
    L, H, W = images.shape[:3]
    N = H * W
    d_img, d_mask, d_ld = dev(images, cuda).reshape(L, N, 3), dev(mask, cuda).reshape(N), dev(ld, cuda)
    d_e = dev(e, cuda)
    paths = ('auto', 'reform') + (('tile',) if L <= hip.PS_TILE_LIGHTS else ())
    for path in paths:
        out = hip.ps_normals(d_img, d_mask, d_ld, d_e, path=path, out=guarded(N, cuda), **SETTINGS[setting])
        for name, t, a in zip(('normal', 'albedo', 'valid', 'kept'), out, res):
            assert same_bits(t, a.reshape(t.shape)), '%s, path %s: %s differs from the definition in %d of %d elements' % (
                what, path, name, int((t.cpu().numpy() != a.reshape(t.shape)).sum()), a.size)
    return int(res[2].sum())


@pytest.mark.parametrize('L', [3, 4, 8, 64, 65, 96, 97, 256])
def test_normals_equal_the_definition_bit_for_bit(cuda, L):
    """Every light count at which something changes (the minimum, the 8-light ranking block and its remainders, the LDS tile's last
    size 96 and the first size beyond it, the maximum) x the pixel counts around a wave (1, 63, 64, 65) and two images with several
    workgroups, uint8 and float32, with and without light_int, two settings of (low, high, dark) -- on every path that L admits."""
    sizes = [(1, 1), (1, 63), (1, 64), (1, 65), (24, 20)] + ([(48, 40)] if L <= 96 else [])
    n_valid = 0
    for i, (H, W) in enumerate(sizes):
        for dtype_name in ('uint8', 'float32'):
            with_int, setting = (i + (dtype_name == 'uint8')) % 2 == 1, (i // 2 + (dtype_name == 'float32')) % 2
            if (H, W) == (24, 20):          # the image with every combination
                combos = [(w, s) for w in (False, True) for s in (0, 1)]
            else:
                combos = [(with_int, setting)]
            for w, s in combos:
                images, mask, ld, e, res = host_normals(L, H, W, dtype_name, False, w, s)
                n_valid += check_normals(cuda, images, mask, ld, e, res, s, 'L=%d %dx%d %s light_int=%s setting %d' % (L, H, W, dtype_name, w, s))
    print('L=%d: %d valid pixels compared bit for bit' % (L, n_valid))
    assert n_valid > (100 if L > 3 else 0)


@pytest.mark.parametrize('L', [8, 96, 130])
def test_heavy_ties_follow_the_tie_rule(cuda, L):
    """uint8 images with four grey levels: most of a pixel's lights tie in g, and the light index decides the kept set."""
    for setting in (0, 1):
        images, mask, ld, e, res = host_normals(L, 24, 20, 'uint8', True, False, setting)
        n_valid = check_normals(cuda, images, mask, ld, e, res, setting, 'ties L=%d setting %d' % (L, setting))
    assert n_valid > 50


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_constructed_pixels_among_valid_ones(cuda, dtype):
    """The constructed pixels of tests/test_ps_cpu.py (two lit lights, coplanar lit lights with det == 0, unmasked, all-equal bytes,
    trims that leave fewer than min_lights) in one row with valid sphere pixels, so that lanes of one wave take every branch."""
    from psnerf_amd import hip
    cons, cmask = ps_cases.constructed(dtype)
    ld = ps_cases.CONSTRUCTED_LIGHTS
    rs = np.random.RandomState(1)
    n = np.array([0.0, 0.0, 1.0])[None] + 0.4 * rs.randn(70, 3)
    lamb = np.clip(n @ ld.T, 0.0, None).T[:, None, :, None] * np.array([40.0, 25.0, 10.0])[None, None, None, :]      # [8, 1, 70, 3], < 255
    lamb = np.round(lamb)
    lamb = lamb.astype(np.uint8) if dtype == np.uint8 else (lamb / 256.0).astype(np.float32)
    images = np.concatenate([lamb[:, :, :30], cons, lamb[:, :, 30:]], axis=2)
    mask = np.concatenate([np.ones((1, 30), bool), cmask, np.ones((1, 40), bool)], axis=1)
    N = images.shape[2]
    d_img, d_mask, d_ld = dev(images, cuda).reshape(8, N, 3), dev(mask, cuda).reshape(N), dev(ld, cuda)
    for kw in (dict(low=0.0, high=0.0), dict(low=0.25, high=0.25), dict(low=0.4, high=0.4), dict(low=0.0, high=0.0, min_lights=5)):
        res = ps.host_photometric_stereo(images, mask, ld, **kw)
        for path in ('tile', 'reform'):
            out = hip.ps_normals(d_img, d_mask, d_ld, None, path=path, out=guarded(N, cuda), **kw)
            for name, t, a in zip(('normal', 'albedo', 'valid', 'kept'), out, res):
                assert same_bits(t, a.reshape(t.shape)), '%r path %s: %s' % (kw, path, name)
        if kw == dict(low=0.0, high=0.0):
            assert res[2][0, 30:36].tolist() == [0, 0, 0, 1, 1, 1] and res[3][0, 30:36].tolist() == [2, 4, 0, 8, 4, 8] and res[2].sum() > 40
    flat = ld.copy()
    flat[:, 2] = 0.0
    out = hip.ps_normals(d_img, d_mask, dev(flat, cuda), None, low=0.0, high=0.0, out=guarded(N, cuda))
    assert not out[2].any() and not out[0].any() and not out[1].any() and same_bits(out[3], ps.host_photometric_stereo(images, mask, flat, low=0.0, high=0.0)[3].reshape(N))


@pytest.mark.parametrize('H,W,L,dtype', [(24, 20, 8, np.float32), (48, 40, 12, np.uint8), (53, 41, 5, np.uint8), (1, 2049, 3, np.float32)])
def test_light_intensity_against_the_definition(cuda, H, W, L, dtype):
    """Pixel counts that leave a partial last workgroup (480, 1920, 2173 = one chunk of 2048 + 125, 2049 = + 1)."""
    from psnerf_amd import hip
    images, mask, ld = ps_cases.random_view(L, H, W, seed=H + L, dtype=dtype)
    normal, albedo, valid, _ = ps.host_photometric_stereo(images, mask, ld)
    N = H * W
    d_img, d_ld = dev(images, cuda).reshape(L, N, 3), dev(ld, cuda)
    d_n, d_a, d_v = dev(normal, cuda).reshape(N, 3), dev(albedo, cuda).reshape(N, 3), dev(valid, cuda).reshape(N)
    gate = N * 2.0 ** -50
    for dark, bright in ((0.0, 1.0), (0.1, 0.8)):
        want = ps.host_light_intensity(images, mask, normal, albedo, valid, ld, dark, bright)
        nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float64, device=cuda)
        a = hip.ps_light_intensity(d_img, d_n, d_a, d_v, d_ld, dark, bright, out=(nan(L, 3), nan(L, 6)))
        b = hip.ps_light_intensity(d_img.clone(), d_n.clone(), d_a.clone(), d_v.clone(), d_ld.clone(), dark, bright)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), 'two runs differ'
        got = a[0].cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got == 0.0, want == 0.0)
        rel = float(np.abs(got[want != 0.0] / want[want != 0.0] - 1.0).max()) if (want != 0.0).any() else 0.0
        print('light intensity %dx%d L=%d %s window (%.1f, %.1f): max relative error %.3e (gate %.3e), %d valid pixels'
              % (H, W, L, np.dtype(dtype).name, dark, bright, rel, gate, int(valid.sum())))
        assert rel <= gate
        assert (want != 0.0).sum() >= L
        pub = ps.light_intensity(dev(images, cuda), dev(mask, cuda), d_n.reshape(H, W, 3), d_a.reshape(H, W, 3), d_v.reshape(H, W), d_ld, dark, bright,
                                 relative_to=0)
        assert torch.equal(pub, a[0] / a[0][0][None])


def test_light_average_bit_for_bit(cuda):
    """The mean bit for bit, both uint8 outputs byte for byte; values chosen to hit the .5 rounding ties: pixel row 0 holds, over four
    lights, bytes (255, 255, 0, 0) -> mean 0.5 -> 127.5 -> 128, and (255, 255, 255, 0) -> 191.25; with relat_int = 2 the normalised
    byte of 255 is 127.5 -> 128."""
    from psnerf_amd import hip
    for L, H, W, dtype in ((4, 13, 17, np.uint8), (7, 1, 300, np.uint8), (5, 9, 31, np.float32)):
        images, mask, _ = ps_cases.random_view(L, H, W, seed=L, dtype=dtype)
        images = images.copy()
        if dtype == np.uint8 and L == 4:
            images[:, 0, 0] = np.array([255, 255, 0, 0], np.uint8)[:, None]
            images[:, 0, 1] = np.array([255, 255, 255, 0], np.uint8)[:, None]
            images[:, 0, 2] = np.array([1, 3, 5, 255], np.uint8)[:, None]
            mask = mask.copy()
            mask[0, :3] = True
        N = H * W
        d_img, d_mask = dev(images, cuda), dev(mask, cuda)
        relats = (None, np.full(L, 2.0), np.stack([np.linspace(0.6, 1.7, L), np.linspace(1.2, 0.4, L), np.full(L, 2.0)], 1))
        for relat in relats:
            want = ps.host_light_average(images, mask, relat)
            guard = (torch.full((N, 3), float('nan'), dtype=torch.float64, device=cuda), torch.full((N, 3), 99, dtype=torch.uint8, device=cuda),
                     torch.full((L, N, 3), 99, dtype=torch.uint8, device=cuda) if relat is not None else None)
            r = None if relat is None else dev(relat if relat.ndim == 2 else np.repeat(relat[:, None], 3, 1), cuda)
            raw = hip.ps_light_average(d_img.reshape(L, N, 3), d_mask.reshape(N), r, out=guard)
            got = ps.light_average(d_img, d_mask, None if relat is None else dev(relat, cuda))
            assert same_bits(raw[0], want[0].reshape(N, 3)) and same_bits(raw[1], want[1].reshape(N, 3))
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
            assert (want[2] is None and raw[2] is None and got[2] is None) or (same_bits(raw[2], want[2].reshape(L, N, 3)) and same_bits(got[2], want[2]))
        if dtype == np.uint8 and L == 4:
            assert want[1][0, 0, 2] == 64 and ps.host_light_average(images, mask, None)[1][0, 0].tolist() == [128, 128, 128]
            assert want[2][0, 0, 0, 2] == 128                                                              # 127.5 -> 128
    # without a mask
    got = ps.light_average(d_img, None)
    want = ps.host_light_average(images, None)
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])


def test_estimate_through_the_public_functions(cuda):
    """estimate(n_iter=1) on the 48 x 40 sphere equals host_estimate bit for bit in normal, albedo, valid, kept, and within the
    intensity gate in light_int.  n_iter=2 feeds the device's own intensities back; their rounding differs from the host's by the gate,
    which can move a kept set at a tie, so the second round is compared teacher-forced: the device normals given the HOST's first-round
    intensities equal the host's second round bit for bit."""
    s = ps_cases.sphere(48, 40, 12, seed=12)
    images, mask, ld = ps_cases.to_u8(s['images']), np.array(s['mask']), np.array(s['light_dir'])
    d_img, d_mask, d_ld = dev(images, cuda), dev(mask, cuda), dev(ld, cuda)
    h1 = ps.host_estimate(images, mask, ld, n_iter=1)
    d1 = ps.estimate(d_img, d_mask, d_ld, n_iter=1)
    assert all(torch.is_tensor(v) and v.is_cuda for v in d1.values())
    for k in ('normal', 'albedo', 'valid', 'kept'):
        assert same_bits(d1[k], h1[k]), k
    gate = images.shape[1] * images.shape[2] * 2.0 ** -50
    e_d, e_h = d1['light_int'].cpu().numpy(), h1['light_int']
    assert np.all(e_h > 0.0) and float(np.abs(e_d / e_h - 1.0).max()) <= gate
    h2 = ps.host_estimate(images, mask, ld, n_iter=2)
    forced = ps.photometric_stereo(d_img, d_mask, d_ld, light_int=dev(ps.feedback_intensity(e_h), cuda))
    for t, k in zip(forced, ('normal', 'albedo', 'valid', 'kept')):
        assert same_bits(t, h2[k]), 'teacher-forced second round: ' + k
    d2 = ps.estimate(d_img, d_mask, d_ld, n_iter=2)
    moved = int((d2['kept'].cpu().numpy() != h2['kept']).sum())
    err = ps_cases.angular_error_deg(d2['normal'].cpu().numpy(), h2['normal'], h2['valid'] != 0).max()
    print('estimate(n_iter=2) with the device\'s own intensities: %d kept counts differ from the host\'s, max angle to the host\'s normals %.3e degrees'
          % (moved, err))
    assert d2['normal'].shape == (48, 40, 3) and err < 1.0


def test_bindings_reject_bad_arguments(cuda):
    from psnerf_amd import hip
    img = torch.zeros(8, 50, 3, dtype=torch.uint8, device=cuda)
    ld = torch.ones(8, 3, dtype=torch.float64, device=cuda)
    with pytest.raises(RuntimeError, match='float32 or uint8'):
        hip.ps_normals(img.double(), None, ld)
    with pytest.raises(RuntimeError, match='lights'):
        hip.ps_normals(img[:2].contiguous(), None, ld[:2].contiguous())
    with pytest.raises(RuntimeError, match='light_dir'):
        hip.ps_normals(img, None, ld.float())
    with pytest.raises(RuntimeError, match='light_dir'):
        hip.ps_normals(img, None, ld[:5].contiguous())
    with pytest.raises(RuntimeError, match='mask'):
        hip.ps_normals(img, torch.ones(49, dtype=torch.bool, device=cuda), ld)
    with pytest.raises(RuntimeError, match='path'):
        hip.ps_normals(img, None, ld, path='fast')
    with pytest.raises(RuntimeError, match='low'):
        hip.ps_normals(img, None, ld, low=0.6, high=0.6)
    with pytest.raises(RuntimeError, match='LDS tile'):
        hip.ps_normals(torch.zeros(100, 5, 3, dtype=torch.uint8, device=cuda), None, torch.ones(100, 3, dtype=torch.float64, device=cuda), path='tile')
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        hip.ps_light_average(img.cpu(), None)


def test_stage1_normals_feed_a_trainer_step_under_strict(cuda):
    """The maps of stage1_normals() in the stage-1 data dictionary: one Trainer step with normal_loss on, past normal_after, under
    ops.STRICT (no fallback off the fused paths), at a tiny synthetic batch."""
    from psnerf_amd import ops
    from psnerf_amd.stage1 import NeuralNetwork, Renderer, Trainer
    from psnerf_amd.synthetic import stage1_batch, stage1_cfg
    h, w, L = 48, 40, 8
    s = ps_cases.sphere(h, w, L, seed=L)
    res = ps.estimate(dev(ps_cases.to_u8(s['images']), cuda), dev(s['mask'], cuda), dev(s['light_dir'], cuda))
    maps = ps.stage1_normals(res)
    assert maps['img.normal'].shape == (3, h, w) and maps['img.normal'].dtype == torch.float32 and maps['img.normal'].is_cuda
    assert maps['img.norm_mask'].shape == (h, w) and maps['img.norm_mask'].dtype == torch.float32
    assert int(maps['img.norm_mask'].sum()) == int(s['mask'].sum())
    cfg = stage1_cfg('bunny', **{'training.n_training_points': 256, 'training.normal_loss': True, 'training.normal_after': 0})
    torch.manual_seed(0)
    net = NeuralNetwork(cfg)
    tr = Trainer(Renderer(net, cfg, device=cuda), torch.optim.Adam(net.parameters(), lr=1e-4), cfg, device=cuda)
    batch = stage1_batch(cfg, h=h, w=w, seed=2)
    batch['img.mask'] = torch.from_numpy(np.array(s['mask'])).float()[None]
    batch['img.normal'] = maps['img.normal'][None]
    batch['img.norm_mask'] = maps['img.norm_mask'][None]
    ops.reset_hits()
    with ops.strict():
        terms = tr.train_step(batch, it=10)
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    assert 'normal_loss' in terms and all(bool(torch.isfinite(v.detach()).all()) for v in terms.values() if torch.is_tensor(v))
