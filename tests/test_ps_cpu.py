"""The host definition of the calibrated photometric stereo (psnerf_amd/photostereo.py:host_*): the Lambertian sphere against its
analytic normals, the kept set against numpy's least squares, constructed pixels with expectations worked out by hand, the light average
against a literal transcription of light_avg.py:58-67, the recovered light intensities, and the C ABI's argument checks through the built
library (no device needed: every check fails before a launch)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import ROOT
from tests import ps_cases
from psnerf_amd import photostereo as ps


@pytest.mark.parametrize('H,W,L', [(24, 20, 8), (48, 40, 12)])
def test_lambertian_sphere(H, W, L):
    """Gate: every masked pixel valid, mean angular error < 1e-3 degrees (float32 images: the rounding alone is around 1e-6
    degrees; the gate has three decades of room on purpose -- it catches a wrong frame, sign or trim)."""
    s = ps_cases.sphere(H, W, L, seed=L)
    normal, albedo, valid, kept = ps.host_photometric_stereo(s['images'], s['mask'], s['light_dir'])
    assert normal.shape == (H, W, 3) and normal.dtype == np.float64 and albedo.shape == (H, W, 3) and albedo.dtype == np.float64
    assert valid.shape == (H, W) and valid.dtype == np.uint8 and kept.shape == (H, W) and kept.dtype == np.int32
    m = s['mask']
    assert m.sum() > 40 and np.array_equal(valid != 0, m)
    err = ps_cases.angular_error_deg(normal, s['normal'], m)
    e_alb = float(np.abs(albedo - s['albedo'])[m].max())
    print('sphere %dx%d L=%d: %d pixels, angular error mean %.3e max %.3e degrees (gate 1e-3 on the mean), albedo max %.3e, kept %d .. %d'
          % (H, W, L, m.sum(), err.mean(), err.max(), e_alb, kept[m].min(), kept[m].max()))
    assert err.mean() < 1e-3
    assert e_alb < 1e-5
    assert np.all(normal[~m] == 0.0) and np.all(albedo[~m] == 0.0) and np.all(kept[~m] == 0)
    # the public function on numpy arrays IS the definition; estimate() adds the intensities
    again = ps.photometric_stereo(s['images'], s['mask'], s['light_dir'])
    assert all(np.array_equal(a, b) for a, b in zip(again, (normal, albedo, valid, kept)))
    maps = ps.stage1_normals(ps.estimate(s['images'], s['mask'], s['light_dir']))
    assert maps['img.normal'].shape == (3, H, W) and maps['img.normal'].dtype == np.float32
    assert maps['img.norm_mask'].shape == (H, W) and maps['img.norm_mask'].dtype == np.float32
    assert np.array_equal(maps['img.normal'], normal.astype(np.float32).transpose(2, 0, 1)) and np.array_equal(maps['img.norm_mask'] != 0, m)


def kept_set(images, light_dir, low, high, dark):
    """The kept set of every pixel straight from steps 1 - 4 of the definition, one pixel at a time with a stable sort."""
    L = images.shape[0]
    v = images.reshape(L, -1, 3).astype(np.float64) / (255.0 if images.dtype == np.uint8 else 1.0)
    g = (v[:, :, 0] + v[:, :, 1]) + v[:, :, 2]
    keep = np.zeros(g.shape, bool)
    for p in range(g.shape[1]):
        lit = [l for l in range(L) if g[l, p] > dark]
        order = sorted(lit, key=lambda l: (g[l, p], l))
        n = len(lit)
        for l in order[int(np.floor(low * n)):n - int(np.floor(high * n))]:
            keep[l, p] = True
    return keep, g


@pytest.mark.parametrize('low,high,dark', [(0.1, 0.25, 0.0), (0.0, 0.3, 0.05)])
def test_normal_is_the_least_squares_solution_over_the_kept_set(low, high, dark):
    """Over the same kept lights the normal agrees with np.linalg.lstsq within 1e-9 per component (cond = 1e-4 bounds the
    amplification of 2^-53 far below that)."""
    images, mask, ld = ps_cases.random_view(10, 9, 11, seed=3, dtype=np.float32)
    normal, _, valid, kept = ps.host_photometric_stereo(images, mask, ld, low=low, high=high, dark=dark)
    keep, g = kept_set(images, ld, low, high, dark)
    assert np.array_equal(kept.reshape(-1)[mask.reshape(-1)], keep.sum(0)[mask.reshape(-1)])
    worst, n_valid = 0.0, 0
    for p in np.flatnonzero(valid.reshape(-1)):
        x = np.linalg.lstsq(ld[keep[:, p]], g[keep[:, p], p], rcond=None)[0]
        worst = max(worst, float(np.abs(x / np.linalg.norm(x) - normal.reshape(-1, 3)[p]).max()))
        n_valid += 1
    print('low %.2f high %.2f dark %.2f: %d valid pixels, max |n - lstsq| = %.3e (gate 1e-9)' % (low, high, dark, n_valid, worst))
    assert n_valid > 30 and worst <= 1e-9


@pytest.mark.parametrize('dtype', [np.uint8, np.float32])
def test_constructed_pixels(dtype):
    images, mask = ps_cases.constructed(dtype)
    ld = ps_cases.CONSTRUCTED_LIGHTS
    scale = 255.0 if dtype == np.uint8 else 256.0
    normal, albedo, valid, kept = ps.host_photometric_stereo(images, mask, ld, low=0.0, high=0.0)
    assert valid[0].tolist() == [0, 0, 0, 1, 1, 1]
    assert kept[0].tolist() == [2, 4, 0, 8, 4, 8]          # two lit; four coplanar lit (det == 0 exactly); unmasked; all; z > 0 only; all
    assert np.all(normal[0, :3] == 0.0) and np.all(albedo[0, :3] == 0.0)
    assert np.abs(normal[0, 4] - [0.0, 0.0, 1.0]).max() < 1e-12 and np.abs(normal[0, 5] - np.array([1.0, 2.0, 2.0]) / 3.0).max() < 1e-12
    for px in (4, 5):
        assert np.abs(albedo[0, px] - 30.0 * np.array([1.0, 2.0, 0.5]) / scale).max() < 1e-12
    # the tie rule: pixel 3 has one g for all eight lights, so ranks are the light indices and low = high = 0.25 keeps lights 2 .. 5
    normal, albedo, valid, kept = ps.host_photometric_stereo(images, mask, ld, low=0.25, high=0.25)
    assert kept[0, 3] == 4 and valid[0, 3] == 1
    x = np.linalg.lstsq(ld[2:6], np.ones(4), rcond=None)[0]
    assert np.abs(normal[0, 3] - x / np.linalg.norm(x)).max() < 1e-12
    assert kept[0].tolist() == [2, 2, 0, 4, 2, 4] and valid[0].tolist() == [0, 0, 0, 1, 0, 1]
    # low, high that leave fewer than min_lights: 8 lit, floor(3.2) = 3 off either end leaves 2
    normal, albedo, valid, kept = ps.host_photometric_stereo(images, mask, ld, low=0.4, high=0.4)
    assert kept[0].tolist() == [2, 2, 0, 2, 2, 2] and not valid.any() and not normal.any() and not albedo.any()
    assert ps.host_photometric_stereo(images, mask, ld, low=0.0, high=0.0, min_lights=5)[2][0].tolist() == [0, 0, 0, 1, 0, 1]
    # every light in the plane z = 0: det == 0 exactly for every pixel
    flat = ld.copy()
    flat[:, 2] = 0.0
    normal, _, valid, kept = ps.host_photometric_stereo(images, mask, flat, low=0.0, high=0.0)
    assert not valid.any() and not normal.any() and kept[0, 5] == 8


def test_light_int_per_light_and_per_channel():
    """Images scaled by powers of two and light_int = those factors give the unscaled result bit for bit, as [L] and as [L, 3]."""
    s = ps_cases.sphere(24, 20, 8, seed=8)
    base = ps.host_photometric_stereo(s['images'], s['mask'], s['light_dir'])
    e1 = np.array([0.5, 1.0, 2.0, 4.0, 1.0, 0.25, 2.0, 8.0])
    e3 = np.stack([e1, e1[::-1], np.roll(e1, 3)], 1)
    for e in (e1, e3):
        scaled = (s['images'] * (e[:, None, None, None] if e.ndim == 1 else e[:, None, None, :])).astype(np.float32)
        got = ps.host_photometric_stereo(scaled, s['mask'], s['light_dir'], light_int=e)
        assert all(np.array_equal(a, b) for a, b in zip(got, base))
    assert not np.array_equal(ps.host_photometric_stereo(scaled, s['mask'], s['light_dir'])[0], base[0])
    with pytest.raises(ValueError):
        ps.host_photometric_stereo(s['images'], s['mask'], s['light_dir'], light_int=np.ones((8, 2)))


def test_parameter_errors():
    s = ps_cases.sphere(24, 20, 8, seed=8)
    for kw in (dict(low=-0.1), dict(high=1.0), dict(low=0.5, high=0.5), dict(min_lights=2)):
        with pytest.raises(ValueError):
            ps.host_photometric_stereo(s['images'], s['mask'], s['light_dir'], **kw)
    with pytest.raises(ValueError):
        ps.host_photometric_stereo(s['images'][:2], s['mask'], s['light_dir'][:2])
    with pytest.raises(ValueError):
        ps.host_photometric_stereo(s['images'].astype(np.float64), s['mask'], s['light_dir'])
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        ps.photometric_stereo(torch.from_numpy(s['images'].copy()), torch.from_numpy(s['mask'].copy()), s['light_dir'])


def test_quantisation_and_highlight_report():
    """Report only, no gate beyond sanity: what 8-bit quantisation and a strong cos^60 highlight cost at the defaults."""
    for L in (8, 12, 32):
        s = ps_cases.sphere(48, 40, L, seed=L)
        n8, _, v8, _ = ps.host_photometric_stereo(ps_cases.to_u8(s['images']), s['mask'], s['light_dir'])
        h = ps_cases.sphere(48, 40, L, seed=L, highlight=0.8)
        nh, _, vh, _ = ps.host_photometric_stereo(ps_cases.to_u8(h['images']), h['mask'], h['light_dir'])
        e8 = ps_cases.angular_error_deg(n8, s['normal'], v8 != 0)
        eh = ps_cases.angular_error_deg(nh, h['normal'], vh != 0)
        print('uint8 sphere 48x40 L=%d: mean angular error %.3f degrees (max %.3f); with a 0.8 cos^60 highlight %.3f (max %.3f)'
              % (L, e8.mean(), e8.max(), eh.mean(), eh.max()))
        assert e8.mean() < 5.0 and eh.mean() < 20.0


def transcribed_light_average(u8, mask, relat_int):
    """light_avg.py:58-67 with the file reads and writes replaced by arrays -> (mean, mean_u8, [normalised images])."""
    light_img, written = [], []
    for idx in range(u8.shape[0]):
        limg = np.array(u8[idx]) / 255.
        limg = limg * mask[..., None]
        if relat_int is not None:
            limg = limg / relat_int[idx]
            written.append((limg.clip(0, 1) * 255).round().astype(np.uint8))
        light_img.append(limg)
    light_img_mean = np.mean(light_img, axis=0)
    return light_img_mean, (light_img_mean.clip(0, 1) * 255).round().astype(np.uint8), written


def test_light_average_is_the_transcription():
    images, mask, _ = ps_cases.random_view(7, 13, 17, seed=5)
    images[:, 0, 0] = [[0, 0, 0], [1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]]
    mask[0, 0] = True
    for relat in (None, np.linspace(0.6, 1.7, 7), np.stack([np.linspace(0.6, 1.7, 7), np.linspace(1.2, 0.4, 7), np.ones(7)], 1)):
        mean, mean_u8, norm = ps.host_light_average(images, mask, relat)
        r_mean, r_u8, r_norm = transcribed_light_average(images, mask, relat)
        assert mean.dtype == np.float64 and np.array_equal(mean, r_mean) and np.array_equal(mean_u8, r_u8)
        assert (norm is None and not r_norm) or np.array_equal(norm, np.stack(r_norm))
    # rounding ties: four lights with bytes 255, 255, 0, 0 have the mean 0.5 exactly, and 127.5 rounds half to even = 128
    pair = np.zeros((4, 1, 1, 3), np.uint8)
    pair[0] = pair[1] = 255
    mean, mean_u8, _ = ps.host_light_average(pair, None)
    assert mean[0, 0, 0] == 0.5 and mean_u8[0, 0, 0] == 128
    pair[2] = 255                                                      # 0.75 -> 191.25 -> 191
    assert ps.host_light_average(pair, None)[1][0, 0, 0] == 191
    assert ps.round_u8(np.array([0.5 / 255.0, 1.5 / 255.0, 2.5 / 255.0, -1.0, 7.0])).tolist()[-2:] == [0, 255]


def test_light_intensity_recovers_the_scales():
    """Images of the Lambertian sphere scaled per light and channel: the estimate relative to light 0 is the scale relative to light
    0 within the float32 rounding of the images (gate 1e-6 relative)."""
    s = ps_cases.sphere(48, 40, 12, seed=12)
    rs = np.random.RandomState(0)
    k = 0.5 + rs.rand(12, 3)
    scaled = (s['images'].astype(np.float64) * k[:, None, None, :]).astype(np.float32)
    valid = s['mask'].astype(np.uint8)
    e = ps.host_light_intensity(scaled, s['mask'], s['normal'], s['albedo'], valid, s['light_dir'], dark=0.0, bright=np.inf, relative_to=0)
    err = float(np.abs(e / (k / k[0][None]) - 1.0).max())
    print('light intensities of 12 lights x 3 channels relative to light 0: max relative error %.3e (gate 1e-6)' % err)
    assert e.shape == (12, 3) and err <= 1e-6
    # the window (dark, bright) is open and per channel; nothing inside -> 0
    assert np.all(ps.host_light_intensity(scaled, s['mask'], s['normal'], s['albedo'], valid, s['light_dir'], dark=5.0, bright=6.0) == 0.0)
    # host_estimate alternates the two, starting without intensities, and feeds back feedback_intensity(e)
    out = ps.host_estimate(scaled, s['mask'], s['light_dir'], n_iter=2, bright=np.inf)
    first = ps.host_photometric_stereo(scaled, s['mask'], s['light_dir'])
    e1 = ps.host_light_intensity(scaled, s['mask'], first[0], first[1], first[2], s['light_dir'], 0.0, np.inf)
    second = ps.host_photometric_stereo(scaled, s['mask'], s['light_dir'], ps.feedback_intensity(e1))
    e2 = ps.host_light_intensity(scaled, s['mask'], second[0], second[1], second[2], s['light_dir'], 0.0, np.inf)
    assert np.array_equal(out['normal'], second[0]) and np.array_equal(out['valid'], second[2]) and np.array_equal(out['light_int'], e2)
    assert np.array_equal(ps.feedback_intensity(np.array([0.0, 2.0, -1.0])), [1.0, 2.0, 1.0])
    err1 = ps_cases.angular_error_deg(first[0], s['normal'], first[2] != 0).mean()
    err2 = ps_cases.angular_error_deg(second[0], s['normal'], second[2] != 0).mean()
    print('unknown intensities 0.5 .. 1.5: mean angular error %.3f degrees without them, %.3f after one round of estimates' % (err1, err2))


def test_c_entries_check_their_arguments_on_the_host():
    from psnerf_amd import hip
    lib = hip._lib
    d = 64   # a non-null pointer that is never dereferenced: every check below fails before a launch
    err = lambda: lib.psn_last_error()
    normals = lambda images=d, ty=1, ld=d, L=8, n=100, low=0.1, high=0.25, min_lights=3, path=0, out=d: lib.psn_ps_normals(
        images, ty, None, ld, None, L, n, low, high, 0.0, min_lights, 1e-4, path, out, d, d, d, None)
    assert normals(images=None) == -1 and b'null' in err()
    assert normals(ld=None) == -1 and b'null' in err()
    assert normals(out=None) == -1 and b'null' in err()
    assert normals(ty=2) == -1 and b'image_type' in err()
    assert normals(L=2) == -1 and b'lights' in err()
    assert normals(L=hip.PS_MAX_LIGHTS + 1) == -1 and b'lights' in err()
    assert normals(n=0) == -1 and b'n_pixels' in err()
    assert normals(low=-0.5) == -1 and b'low' in err()
    assert normals(high=1.0) == -1 and b'low' in err()
    assert normals(low=0.5, high=0.5) == -1 and b'low' in err()
    assert normals(low=float('nan')) == -1 and b'low' in err()
    assert normals(min_lights=2) == -1 and b'min_lights' in err()
    assert normals(path=3) == -1 and b'path' in err()
    assert normals(L=hip.PS_TILE_LIGHTS + 1, path=hip.PS_PATH_TILE) == -1 and b'LDS tile' in err()
    inten = lambda images=d, ty=0, L=8, n=100, partial=d: lib.psn_ps_light_intensity(images, ty, d, d, d, d, L, n, 0.0, 1.0, partial, d, d, None)
    assert inten(images=None) == -1 and b'null' in err()
    assert inten(partial=None) == -1 and b'null' in err()
    assert inten(ty=7) == -1 and b'image_type' in err()
    assert inten(L=1) == -1 and b'lights' in err()
    assert inten(n=-4) == -1 and b'n_pixels' in err()
    avg = lambda images=d, ty=1, L=8, n=100, mean=d: lib.psn_ps_light_average(images, ty, None, None, L, n, mean, d, None, None)
    assert avg(images=None) == -1 and b'null' in err()
    assert avg(mean=None) == -1 and b'null' in err()
    assert avg(ty=-1) == -1 and b'image_type' in err()
    assert avg(L=300) == -1 and b'lights' in err()
    assert avg(n=0) == -1 and b'n_pixels' in err()
    # one row of six per 2048-pixel chunk and light
    assert lib.psn_ps_workspace(96, 512 * 612) == 96 * 153 * 6 and lib.psn_ps_workspace(3, 2049) == 3 * 2 * 6
    assert lib.psn_ps_workspace(2, 100) == -1 and lib.psn_ps_workspace(8, 0) == -1
    assert (hip.PS_MAX_LIGHTS, hip.PS_MIN_LIGHTS) == (ps.MAX_LIGHTS, ps.MIN_LIGHTS) and hip.PS_TILE_LIGHTS <= hip.PS_MAX_LIGHTS


def write_dataset(root, n_view=2, L=8, H=24, W=20):
    """A small dataset directory in the reference's layout, from the Lambertian sphere."""
    from PIL import Image
    s = ps_cases.sphere(H, W, L, seed=L)
    os.makedirs(os.path.join(root, 'mask'))
    for vi in range(n_view):
        os.makedirs(os.path.join(root, 'img', 'view_%02d' % (vi + 1)))
        for li in range(L):
            Image.fromarray(ps_cases.to_u8(s['images'][li])).save(os.path.join(root, 'img', 'view_%02d' % (vi + 1), '%03d.png' % (li + 1)))
        Image.fromarray((s['mask'] * 255).astype(np.uint8)).save(os.path.join(root, 'mask', 'view_%02d.png' % (vi + 1)))
    with open(os.path.join(root, 'params.json'), 'w') as f:
        json.dump({'n_view': n_view, 'light_is_same': True, 'light_direction': s['light_dir'].tolist()}, f)
    return s


def test_tool_writes_what_the_reference_loaders_read(tmp_path):
    """tools/photometric_stereo.py --host on a dataset directory: the files the reference's stage-1 dataset and light_avg.py's
    consumers read, with the definition's contents."""
    from psnerf_amd.imgmetrics import load_image
    spec = importlib.util.spec_from_file_location('psn_tools_photometric_stereo', os.path.join(ROOT, 'tools', 'photometric_stereo.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    root = str(tmp_path / 'obj')
    L = 8
    s = write_dataset(root, L=L)
    report = tool.main(['--path', str(tmp_path), '--obj', 'obj', '--host', '--light-avg', '--light-intnorm'])
    u8 = np.stack([ps_cases.to_u8(s['images'][li]) for li in range(L)])
    out = ps.host_estimate(u8, s['mask'], s['light_dir'])
    for vi in (1, 2):
        n = np.load(os.path.join(root, 'sdps_out_l%d' % L, 'outnpy', 'view_%02d.npy' % vi))
        assert n.dtype == np.float32 and n.shape == (24, 20, 3) and np.array_equal(n, out['normal'].astype(np.float32))
        assert np.array_equal(load_image(os.path.join(root, 'norm_mask', 'view_%02d.png' % vi)), out['valid'] * 255)
        relat = out['light_int'] / out['light_int'][3][None]          # light_avg.py:55: shared lights are relative to light 4
        mean, mean_u8, norm = ps.host_light_average(u8, s['mask'], relat)
        assert np.array_equal(load_image(os.path.join(root, 'img_intnorm_sdps_l%d' % L, 'avg', 'view_%02d.png' % vi)), mean_u8)
        assert np.array_equal(load_image(os.path.join(root, 'img_intnorm_sdps_l%d' % L, 'view_%02d' % vi, '003.png')), norm[2])
        assert np.array_equal(load_image(os.path.join(root, 'img', 'avg_l%d' % L, 'view_%02d.png' % vi)), ps.host_light_average(u8, s['mask'])[1])
    e = np.load(os.path.join(root, 'sdps_out_l%d' % L, 'light_intensity_pred.npy'))
    assert e.shape == (2, L, 3) and np.array_equal(e[0], out['light_int'])
    assert report['views'] == 2 and report['lights'] == L and 0.0 <= report['valid_fraction'] <= 1.0
