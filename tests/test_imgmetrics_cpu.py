"""The host definition of the image evaluation (psnerf_amd/imgmetrics.py:host_*, psnerf_amd.metrics.SSIM): SSIM against an
independent evaluation of the same formula through scipy.ndimage.gaussian_filter -- the function skimage calls; skimage itself is
not a dependency --, its exact properties, the evaluation.py sequence against a literal transcription, the 8-bit quantisation, and
the refusal of CPU tensors on the device path."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests.helpers import ROOT
from tests.imgmetrics_data import image_batch
from psnerf_amd import imgmetrics as im
from psnerf_amd import metrics


def scipy_ssim(x, y):
    """structural_similarity(data_range=1, channel_axis=2, gaussian_weights=True, sigma=1.5, use_sample_covariance=False) in float64
    through scipy's own filter -> (mean, map)."""
    from scipy.ndimage import gaussian_filter
    x, y = x.astype(np.float64), y.astype(np.float64)
    f = lambda a: np.stack([gaussian_filter(a[..., c], 1.5, truncate=3.5, mode='reflect') for c in range(a.shape[2])], axis=-1)
    ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    S = ((2 * ux * uy + 1e-4) * (2 * vxy + 9e-4)) / ((ux ** 2 + uy ** 2 + 1e-4) * (vx + vy + 9e-4))
    crop = S[5:S.shape[0] - 5, 5:S.shape[1] - 5]
    return float(np.mean([crop[..., c].mean() for c in range(S.shape[2])])), S


@pytest.mark.parametrize('h,w', [(11, 11), (37, 53), (512, 612)])
def test_host_ssim_against_scipy_filter(h, w):
    pred, gt, _ = image_batch(h + w, 1, h, w)
    x, y = pred[0].astype(np.float32) / 255., gt[0].astype(np.float32) / 255.
    got, got_map = im.host_ssim(x, y, full=True)
    ref, ref_map = scipy_ssim(x, y)
    err_map = float(np.abs(got_map - ref_map).max())
    print('%d x %d: ssim %.6f, |mean - scipy| = %.3e, map max %.3e (gate 1e-12)' % (h, w, got, abs(got - ref), err_map))
    assert got_map.shape == (h, w, 3) and got_map.dtype == np.float64
    assert abs(got - ref) <= 1e-12 and err_map <= 1e-12
    assert metrics.SSIM(x, y) == got
    if (h, w) == (512, 612):
        assert 0.80 < got < 0.92          # the test images are meant to land around 0.86


def test_weights_match_the_kernel_table():
    """csrc/imgmetrics.hip carries the window as hexadecimal float64 constants: they are the definition's weights bit for bit."""
    text = open(os.path.join(ROOT, 'psnerf_amd', 'csrc', 'imgmetrics.hip')).read()
    table = re.search(r'#define IM_WEIGHTS(.*?)\}', text, flags=re.S).group(1)
    consts = [float.fromhex(t) for t in re.findall(r'0x1\.[0-9a-f]+p-?\d+', table)]
    assert len(consts) == 11 and consts == [float(v) for v in im.WEIGHTS]
    assert abs(im.WEIGHTS.sum() - 1.0) < 1e-15 and im.RADIUS == 5 and im.WIN == 11


def test_ssim_exact_properties():
    pred, gt, mask = image_batch(3, 1, 40, 48)
    x, y = pred[0].astype(np.float32) / 255., gt[0].astype(np.float32) / 255.
    assert metrics.SSIM(x, x) == 1.0
    assert metrics.SSIM(x, y) == metrics.SSIM(y, x)
    assert metrics.SSIM(x, y, mask[0]) == metrics.SSIM(x, y) == metrics.SSIM(x, y, np.zeros_like(mask[0]))     # the mask is ignored
    for a, b in ((0.2, 0.7), (0.0, 1.0), (0.5, 0.5)):
        got = metrics.SSIM(np.full((20, 31, 3), a, np.float32), np.full((20, 31, 3), b, np.float32))
        a64, b64 = float(np.float32(a)), float(np.float32(b))
        assert abs(got - (2 * a64 * b64 + 1e-4) / (a64 ** 2 + b64 ** 2 + 1e-4)) <= 1e-12
    for shape in ((10, 40, 3), (40, 10, 3)):
        with pytest.raises(ValueError):
            metrics.SSIM(np.zeros(shape, np.float32), np.zeros(shape, np.float32))
    with pytest.raises(ValueError):
        metrics.SSIM(x, y, sigma=2.0)


def reference_sequence(img_pred, img_gt, mask, inten_normalize):
    """evaluation.py:15-26,81-89 transcribed, with float64 dot products -> (psnr, ssim, scale)."""
    bg = lambda x, m: x * m[..., None] + 1 * ~m[..., None]
    img_gt = img_gt.astype(np.float32) / 255.
    img_gt = bg(img_gt.astype(np.float64), mask)
    img_pred = (img_pred.astype(np.float32) / 255.).astype(np.float64)
    scale = 1.0
    if inten_normalize:
        opt_scale = []
        for i in range(3):
            x_hat = img_pred[:, :, i][mask]
            x = img_gt[:, :, i][mask]
            opt_scale.append(x_hat.dot(x) / x_hat.dot(x_hat))
        scale = np.array(opt_scale).mean()
        img_pred = (img_pred * scale).clip(0, 1)
    a, b = bg(img_pred, mask), bg(img_gt, mask)
    mse = np.mean((a[mask] - b[mask]) ** 2)
    psnr = 100 if mse == 0 else -10.0 * math.log10(mse)
    return psnr, scipy_ssim(a, b)[0], scale


@pytest.mark.parametrize('inten_normalize', [False, True])
@pytest.mark.parametrize('per_image_masks', [False, True])
def test_host_evaluate_images_against_the_transcription(inten_normalize, per_image_masks):
    B = 3
    pred, gt, mask = image_batch(11, B, 45, 60, per_image_masks=per_image_masks, gain=0.8 if inten_normalize else 1.0)
    assert mask.shape[0] == (B if per_image_masks else 1)
    psnr, ssim, scale = im.host_evaluate_images(pred, gt, mask, inten_normalize=inten_normalize)
    assert psnr.shape == ssim.shape == scale.shape == (B,) and psnr.dtype == np.float64
    for b in range(B):
        p, s, k = reference_sequence(pred[b], gt[b], mask[b if per_image_masks else 0], inten_normalize)
        assert abs(psnr[b] - p) <= 1e-12 and abs(ssim[b] - s) <= 1e-12 and abs(scale[b] - k) <= 1e-14 * k
    if inten_normalize:
        assert np.all(np.abs(scale - 1.25) < 0.02)          # the gain 0.8 is undone
    else:
        assert np.all(scale == 1.0)
    # float32 input = the same values; a single [H, W, 3] pair with a [H, W] mask
    p2, s2, k2 = im.host_evaluate_images(pred[0].astype(np.float32) / 255., gt[0].astype(np.float32) / 255., mask[0], inten_normalize)
    assert p2[0] == psnr[0] and s2[0] == ssim[0] and k2[0] == scale[0]
    with pytest.raises(ValueError):
        im.host_evaluate_images(pred, gt, np.concatenate([mask[:1], mask[:1]]), inten_normalize)


def test_white_bg_and_scale_img():
    pred, gt, mask = image_batch(5, 1, 30, 30, gain=0.5)
    x, m = pred[0].astype(np.float32) / 255., mask[0]
    w = im.host_white_bg(x, m)
    assert w.dtype == np.float64 and np.all(w[~m] == 1.0) and np.array_equal(w[m], x.astype(np.float64)[m])
    scaled, k = im.host_scale_img(x, gt[0].astype(np.float32) / 255., m)
    assert abs(k - 2.0) < 0.05 and scaled.min() >= 0.0 and scaled.max() <= 1.0


def test_to_img_rounds_half_to_even_on_both_paths():
    v = np.array([0.5, 1.5, 2.5, 3.5, 254.5, -3.0, 300.0, 127.49, 127.51], dtype=np.float32) / np.float32(255.0)
    # only values whose product with 255 is again exactly k + 0.5 exercise the tie rule; build those from the product side
    ties = np.array([k + 0.5 for k in (0, 1, 2, 3, 100, 253)], dtype=np.float32)
    x = np.concatenate([v, (ties / np.float32(255.0)).astype(np.float32)])
    prod = (x.astype(np.float32).clip(0, 1) * 255)
    want = np.round(prod).astype(np.uint8)          # np.round: half to even
    got = im.to_img(x)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    is_tie = prod - np.floor(prod) == 0.5
    assert is_tie.sum() >= 3 and np.all(got[is_tie] % 2 == 0)
    t = im.to_img(torch.from_numpy(x))
    assert t.dtype == torch.uint8 and np.array_equal(t.numpy(), got)
    assert np.array_equal(im.to_img(x.astype(np.float64).reshape(3, 5)), got.reshape(3, 5))
    assert im.to_img(np.array([-1.0, 2.0])).tolist() == [0, 255]


def test_load_image_reads_what_was_written(tmp_path):
    from PIL import Image
    pred, _, mask = image_batch(1, 1, 12, 17)
    Image.fromarray(pred[0]).save(str(tmp_path / 'a.png'))
    Image.fromarray((mask[0] * 255).astype(np.uint8)).save(str(tmp_path / 'm.png'))
    assert np.array_equal(im.load_image(str(tmp_path / 'a.png')), pred[0])
    assert np.array_equal(im.load_image(str(tmp_path / 'm.png')).astype(bool), mask[0])


def test_device_path_rejects_cpu_tensors():
    x = torch.rand(1, 16, 16, 3)
    m = torch.ones(1, 16, 16, dtype=torch.bool)
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        im.evaluate_images(x, x, m)
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        im.evaluate_normals(x, x, m)
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        metrics.SSIM(x[0], x[0])
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        metrics.PSNR(x[0], x[0])
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        metrics.MAE(x[0], x[0])
    with pytest.raises(RuntimeError):
        im.evaluate_images(x.numpy(), x.numpy(), m.numpy())


def test_c_entries_check_their_arguments_on_the_host():
    from psnerf_amd import hip
    lib = hip._lib
    d = 64   # a non-null pointer that is never dereferenced: every check below fails before a launch
    assert lib.psn_img_metrics(None, None, 0, None, 1, None, 1, 16, 16, d, d, d, d, None, None) == -1 and b'null' in lib.psn_last_error()
    assert lib.psn_img_metrics(d, d, 2, None, 1, None, 1, 16, 16, d, d, d, d, None, None) == -1 and b'image_type' in lib.psn_last_error()
    assert lib.psn_img_metrics(d, d, 0, None, 1, None, 1, 10, 16, d, d, d, d, None, None) == -1 and b'11-tap' in lib.psn_last_error()
    assert lib.psn_img_metrics(d, d, 1, d, 2, None, 3, 16, 16, d, d, d, d, None, None) == -1 and b'mask batch' in lib.psn_last_error()
    assert lib.psn_img_scale_sums(d, d, 0, None, 1, 1, 16, 5, d, d, None) == -1 and b'11-tap' in lib.psn_last_error()
    assert lib.psn_img_scale_sums(d, d, 0, None, 1, 1, 16, 16, None, d, None) == -1 and b'null' in lib.psn_last_error()
    assert lib.psn_normal_mae(d, d, d, 2, 1, 3, 100, d, d, None, None) == -1 and b'mask batch' in lib.psn_last_error()
    assert lib.psn_normal_mae(d, d, None, 1, 1, 1, 0, d, d, None, None) == -1 and b'n_pixels' in lib.psn_last_error()
    # one row of 7 per 16 x 32 tile / per 2048-pixel chunk; 2 per chunk for the normals
    assert lib.psn_img_workspace(hip.IMG_WS_METRICS, 8, 512, 612) == 8 * 32 * 20 * 7
    assert lib.psn_img_workspace(hip.IMG_WS_SCALE_SUMS, 8, 512, 612) == 8 * 153 * 7
    assert lib.psn_img_workspace(hip.IMG_WS_NORMAL_MAE, 2, 1, 4097) == 2 * 3 * 2
    assert lib.psn_img_workspace(9, 1, 16, 16) == -1 and lib.psn_img_workspace(0, 0, 16, 16) == -1


@pytest.mark.parametrize('inten_normalize', [False, True])
def test_evaluate_tool_walks_the_reference_layout(tmp_path, capsys, inten_normalize):
    """tools/evaluate.py --host on a small experiment written in the reference's directory layout: its three numbers are those of
    a direct evaluation of the same files' contents, and it prints the reference's lines plus the LPIPS note."""
    import importlib.util
    from tests.imgmetrics_data import write_experiment
    spec = importlib.util.spec_from_file_location('psn_tools_evaluate', os.path.join(ROOT, 'tools', 'evaluate.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    test_out, obj, exp, expected = write_experiment(tmp_path, inten_normalize=inten_normalize)
    out = tool.main(['--obj_name', obj, '--expname', exp, '--test_out_dir', test_out, '--host'])
    text = capsys.readouterr().out
    psnr, ssim, mae = [], [], []
    for pred, gt, mask, npred, ngt in expected:
        p, s, _ = im.host_evaluate_images(pred, gt, mask[None], inten_normalize=inten_normalize)
        psnr.append(p); ssim.append(s)
        mae.append(metrics.MAE(npred, ngt, mask)[0])
    assert abs(out['psnr'] - np.concatenate(psnr).mean()) <= 1e-12 and abs(out['ssim'] - np.concatenate(ssim).mean()) <= 1e-12
    assert abs(out['normal_mae'] - np.mean(mae)) <= 1e-9
    assert 'evaluation_view: 2 , light is same,  evaluation_light: 4' in text
    assert 'PSNR Error:  %.2f' % out['psnr'] in text and 'SSIM Error:  %.4f' % out['ssim'] in text
    assert 'Normal MAE Error:  %.2f' % out['normal_mae'] in text and 'LPIPS: not computed' in text
