"""Image evaluation on the GPU (csrc/imgmetrics.hip through psnerf_amd/imgmetrics.py and psnerf_amd/metrics.py) against the float64
numpy definition in the same modules.  Every pixel of every map and every image of every batch is compared.

Gates, with where they come from (the device arithmetic is float64 with contraction off and follows the definition's order):
  SSIM    each filtered moment is a 22-term float64 sum of values <= 1: error about 3e-15; the variances inherit about 1e-14; divided
          by the smallest denominators C2 = 9e-4 and C1 = 1e-4 that is at most about 2e-10 per map pixel.  Gate 1e-9 absolute on
          every map pixel and on every per-image SSIM.
  PSNR    the masked mean square is a float64 sum in another order, relative error far below 1e-10; PSNR moves by 4.34 x that.
          Gate 1e-9 dB.
  scale   1e-12 relative.
  MAE     the dot products can match to the last bit, acos may differ by an ulp or two; one ulp at a dot product next to +-1 moves
          the angle by at most sqrt(2 x 2.2e-16) rad = 1.2e-6 degrees.  Gate 1e-5 degrees per pixel and on the mean.
"""
import numpy as np
import pytest
import torch

from tests.imgmetrics_data import image_batch, normal_batch
from psnerf_amd import imgmetrics as im
from psnerf_amd import metrics

pytestmark = pytest.mark.gpu
GATE_SSIM, GATE_PSNR, GATE_SCALE, GATE_MAE = 1e-9, 1e-9, 1e-12, 1e-5


def host_maps(pred, gt, mask, inten_normalize):
    """The definition per image, with the SSIM map: -> (psnr [B], ssim [B], scale [B], map [B, H, W, 3])."""
    B = pred.shape[0]
    psnr, ssim, scale, maps = np.zeros(B), np.zeros(B), np.ones(B), []
    for b in range(B):      # host_evaluate_images's own sequence, keeping the map (tests/test_imgmetrics_cpu.py ties the two together)
        m = mask[0 if mask.shape[0] == 1 else b]
        p = pred[b].astype(np.float32) / 255. if pred.dtype == np.uint8 else pred[b]
        g = gt[b].astype(np.float32) / 255. if gt.dtype == np.uint8 else gt[b]
        g = im.host_white_bg(g, m)
        if inten_normalize:
            p, scale[b] = im.host_scale_img(p, g, m)
        p = im.host_white_bg(p, m)
        psnr[b] = metrics.PSNR(p, g, m)
        ssim[b], smap = im.host_ssim(p, g, full=True)
        maps.append(smap)
    if B <= 3:
        again = im.host_evaluate_images(pred, gt, mask, inten_normalize=inten_normalize)
        assert np.array_equal(again[0], psnr) and np.array_equal(again[1], ssim) and np.array_equal(again[2], scale)
    return psnr, ssim, scale, np.stack(maps)


def check_batch(cuda, pred, gt, mask, inten_normalize, what, images=None):
    """evaluate_images(full=True) against the definition (``images``: the indices the host evaluates; default all), and two runs
    bit-identical in the partial sums, the outputs and the map."""
    from psnerf_amd import hip
    d_pred, d_gt, d_mask = torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda), torch.from_numpy(mask).to(cuda)
    psnr, ssim, scale, smap = im.evaluate_images(d_pred, d_gt, d_mask, inten_normalize=inten_normalize, full=True)
    assert all(t.is_cuda and t.dtype == torch.float64 for t in (psnr, ssim, scale, smap)) and smap.shape == pred.shape
    # bit-identity: the raw entries twice, on fresh buffers
    k = scale.contiguous() if inten_normalize else None
    runs = [hip.img_metrics(d_pred.clone(), d_gt.clone(), d_mask.clone(), scale=k, full=True) for _ in range(2)]
    for key in ('partial', 'sums', 'ssim', 'psnr', 'map'):
        assert torch.equal(runs[0][key], runs[1][key]), '%s: two runs differ in %s' % (what, key)
    assert torch.equal(runs[0]['ssim'], ssim) and torch.equal(runs[0]['psnr'], psnr) and torch.equal(runs[0]['map'], smap)
    if inten_normalize:
        s1, s2 = hip.img_scale_sums(d_pred, d_gt, d_mask), hip.img_scale_sums(d_pred.clone(), d_gt.clone(), d_mask.clone())
        assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1]), what + ': two runs of the scale sums differ'
    pick = list(range(pred.shape[0])) if images is None else list(images)
    h_mask = mask if mask.shape[0] == 1 else mask[pick]
    h_psnr, h_ssim, h_scale, h_map = host_maps(pred[pick], gt[pick], h_mask, inten_normalize)
    psnr, ssim, scale, smap = psnr.cpu().numpy()[pick], ssim.cpu().numpy()[pick], scale.cpu().numpy()[pick], smap.cpu().numpy()[pick]
    e_map, e_ssim = float(np.abs(smap - h_map).max()), float(np.abs(ssim - h_ssim).max())
    e_psnr, e_scale = float(np.abs(psnr - h_psnr).max()), float(np.abs(scale / h_scale - 1.0).max())
    print('%s: B=%d %dx%d %s mask %s scale=%s | max |S - S_host| = %.3e, per image %.3e (gate %.0e); PSNR %.3e dB (gate %.0e); scale rel %.3e '
          '(gate %.0e); ssim[0] = %.6f psnr[0] = %.4f scale[0] = %.6f' % (what, pred.shape[0], pred.shape[1], pred.shape[2], pred.dtype, mask.shape[0],
                                                                    inten_normalize, e_map, e_ssim, GATE_SSIM, e_psnr, GATE_PSNR, e_scale,
                                                                    GATE_SCALE, ssim[0], psnr[0], scale[0]))
    assert e_map <= GATE_SSIM and e_ssim <= GATE_SSIM, what
    assert e_psnr <= GATE_PSNR, what
    assert e_scale <= GATE_SCALE, what


@pytest.mark.parametrize('h,w,B', [(11, 11, 2), (37, 53, 3), (64, 64, 2), (130, 70, 3), (512, 612, 8)])
def test_evaluate_images_against_the_definition(cuda, h, w, B):
    for per_image_masks in (False, True):
        for inten_normalize in (False, True):
            pred, gt, mask = image_batch(h * 7 + w, B, h, w, per_image_masks=per_image_masks, gain=0.8 if inten_normalize else 1.0)
            if h == 11:
                mask[:, 5, 5] = True        # (the disc of an 11 x 11 image must not be empty)
            what = '%dx%d' % (h, w)
            check_batch(cuda, pred, gt, mask, inten_normalize, what + ' uint8')
            as_float = lambda a: (a.astype(np.float32) / 255. + np.float32(0.001) * (a % 7).astype(np.float32)).astype(np.float32)
            check_batch(cuda, as_float(pred), as_float(gt), mask, inten_normalize, what + ' float32')


def test_uint8_and_float32_inputs_agree_bit_for_bit(cuda):
    """A byte u is read as the float32 value (float)u / 255.0f: the same images as uint8 and as float32 give the same bits."""
    pred, gt, mask = image_batch(2, 2, 48, 80)
    dm = torch.from_numpy(mask).to(cuda)
    a = im.evaluate_images(torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda), dm, inten_normalize=True, full=True)
    f = lambda x: torch.from_numpy(x.astype(np.float32) / 255.).to(cuda)
    b = im.evaluate_images(f(pred), f(gt), dm, inten_normalize=True, full=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_normal_mae_against_the_definition(cuda):
    from psnerf_amd import hip
    for B, h, w, per_image in ((1, 11, 13, False), (3, 64, 50, True), (2, 130, 70, False)):
        pred, gt = normal_batch(h + w, B, h, w)
        _, _, mask = image_batch(1, B, h, w, per_image_masks=per_image)
        mask[:, :9, :] = True             # the zero vectors and the identical rows take part
        dp, dg, dm = torch.from_numpy(pred).to(cuda), torch.from_numpy(gt).to(cuda), torch.from_numpy(mask).to(cuda)
        mae, err = im.evaluate_normals(dp, dg, dm, full=True)
        again = hip.normal_mae(dp.reshape(B, -1, 3).clone(), dg.reshape(B, -1, 3).clone(), dm.reshape(mask.shape[0], -1), full=True)
        first = hip.normal_mae(dp.reshape(B, -1, 3), dg.reshape(B, -1, 3), dm.reshape(mask.shape[0], -1), full=True)
        assert all(torch.equal(x, y) for x, y in zip(first, again)) and torch.equal(first[2].reshape(B, h, w), err)
        assert mae.is_cuda and mae.dtype == torch.float64 and mae.shape == (B,) and err.shape == (B, h, w)
        mae, err = mae.cpu().numpy(), err.cpu().numpy()
        worst_px, worst_mean = 0.0, 0.0
        for b in range(B):
            m = mask[b if per_image else 0]
            h_mean, h_err = metrics.MAE(pred[b], gt[b], m)
            _, h_all = metrics.MAE(pred[b], gt[b])
            worst_px = max(worst_px, float(np.abs(err[b] - h_all).max()), float(np.abs(err[b][m] - h_err).max()))
            worst_mean = max(worst_mean, abs(mae[b] - h_mean))
            assert np.all(np.abs(err[b, :3, :4] - 90.0) <= GATE_MAE) and np.all(np.abs(err[b, 2:5, 2:6] - 90.0) <= GATE_MAE)   # zero vectors
        print('normals B=%d %dx%d: max per-pixel |err - host| = %.3e deg, per-view mean %.3e deg (gate %.0e); mae[0] = %.4f'
              % (B, h, w, worst_px, worst_mean, GATE_MAE, mae[0]))
        assert worst_px <= GATE_MAE and worst_mean <= GATE_MAE
    # identical maps: the worst case of the bound (every dot product next to 1); the definition's own value is not 0 but
    # acos(1 / (1 + 1e-5)^2) = 0.36 degrees for unit vectors, because of the + 1e-5 in the normalisation
    n, _ = normal_batch(3, 1, 40, 40)
    n[:, :3, :4] = 1.0
    dn = torch.from_numpy(n).to(cuda)
    mae, err = im.evaluate_normals(dn, dn.clone(), None, full=True)
    h_mean, h_err = metrics.MAE(n[0], n[0])
    e = float(np.abs(err.cpu().numpy()[0] - h_err).max())
    print('identical normal maps: max per-pixel |err - host| = %.3e deg, mean %.3e deg (gate %.0e); host mean %.6f'
          % (e, abs(float(mae[0]) - h_mean), GATE_MAE, h_mean))
    assert e <= GATE_MAE and abs(float(mae[0]) - h_mean) <= GATE_MAE
    # without the normalisation identical unit vectors are at 0 up to the rounding of |v|^2
    u = n[0] / np.linalg.norm(n[0].astype(np.float64), axis=-1, keepdims=True)
    u = u.astype(np.float32)
    d_mean, _ = metrics.MAE(torch.from_numpy(u).to(cuda), torch.from_numpy(u).to(cuda), normalize=False)
    h_mean, _ = metrics.MAE(u, u, normalize=False)
    assert abs(d_mean - h_mean) <= GATE_MAE


def test_metrics_module_on_device_tensors(cuda):
    pred, gt, mask = image_batch(9, 1, 96, 75)
    x, y, m = pred[0].astype(np.float32) / 255., gt[0].astype(np.float32) / 255., mask[0]
    dx, dy, dm = torch.from_numpy(x).to(cuda), torch.from_numpy(y).to(cuda), torch.from_numpy(m).to(cuda)
    s_d, s_h = metrics.SSIM(dx, dy), metrics.SSIM(x, y)
    p_d, p_h = metrics.PSNR(dx, dy, dm), metrics.PSNR(x, y, m)
    q_d, q_h = metrics.PSNR(dx, dy), metrics.PSNR(x, y)
    u_d = metrics.SSIM(torch.from_numpy(pred[0]).to(cuda), torch.from_numpy(gt[0]).to(cuda), dm)       # uint8, mask ignored
    print('metrics on device tensors: SSIM %.3e, PSNR masked %.3e dB, unmasked %.3e dB off the numpy paths' % (abs(s_d - s_h), abs(p_d - p_h), abs(q_d - q_h)))
    assert isinstance(s_d, float) and isinstance(p_d, float)
    assert abs(s_d - s_h) <= GATE_SSIM and abs(u_d - s_h) <= GATE_SSIM
    assert abs(p_d - p_h) <= GATE_PSNR and abs(q_d - q_h) <= GATE_PSNR
    assert abs(metrics.SSIM(dx, dx.clone()) - 1.0) <= GATE_SSIM
    assert metrics.PSNR(dx, dx.clone()) == 100 and metrics.PSNR(dx, dx.clone(), dm) == 100
    pn, gn = normal_batch(4, 1, 96, 75)
    dpn, dgn = torch.from_numpy(pn[0]).to(cuda), torch.from_numpy(gn[0]).to(cuda)
    for mk, dmk in ((None, None), (m, dm)):
        mean_d, err_d = metrics.MAE(dpn, dgn, dmk)
        mean_h, err_h = metrics.MAE(pn[0], gn[0], mk)
        assert isinstance(mean_d, float) and err_d.is_cuda and err_d.shape == err_h.shape
        assert abs(mean_d - mean_h) <= GATE_MAE and float(np.abs(err_d.cpu().numpy() - err_h).max()) <= GATE_MAE
    mean_d, _ = metrics.MAE(dpn.reshape(-1, 3), dgn.reshape(-1, 3), dm.reshape(-1))       # the [N, 3] form
    assert abs(mean_d - metrics.MAE(pn[0], gn[0], m)[0]) <= GATE_MAE


def test_bindings_reject_bad_arguments(cuda):
    x = torch.zeros(2, 16, 16, 3, device=cuda)
    m = torch.ones(2, 16, 16, dtype=torch.bool, device=cuda)
    with pytest.raises(RuntimeError, match='float32 or uint8'):
        im.evaluate_images(x.double(), x.double(), m)
    with pytest.raises(RuntimeError, match='one dtype'):
        im.evaluate_images(x, x.to(torch.uint8), m)
    with pytest.raises(RuntimeError, match='shape mismatch'):
        im.evaluate_images(x, x[:, :, :12].contiguous(), m)
    with pytest.raises(RuntimeError, match='11-tap'):
        im.evaluate_images(x[:, :10].contiguous(), x[:, :10].contiguous(), m[:, :10].contiguous())
    with pytest.raises(RuntimeError, match='neither 1 nor B'):
        im.evaluate_images(torch.cat([x, x[:1]]), torch.cat([x, x[:1]]), m)
    with pytest.raises(RuntimeError, match='uint8 or bool'):
        im.evaluate_images(x, x, m.float())
    with pytest.raises(RuntimeError, match='HIP device tensor'):
        im.evaluate_images(x, x.cpu(), m)
    with pytest.raises(RuntimeError, match='float32'):
        im.evaluate_normals(x.double(), x.double(), m)
    with pytest.raises(RuntimeError, match='neither 1 nor B'):
        im.evaluate_normals(torch.cat([x, x[:1]]), torch.cat([x, x[:1]]), m)


def test_one_view_of_96_lights_under_strict(cuda):
    """One view's 96 lights at the stated size of configs[4] (512 x 612) in one call under ops.strict(), one [1, H, W] mask for all of
    them, with the intensity scale.  The host definition runs on the images 0, 47 and 95, chosen here by index before anything is
    computed (all 96 would cost the suite about a minute); those three are checked in full, map included."""
    from psnerf_amd import ops
    pred, gt, mask = image_batch(96, 96, 512, 612, gain=0.7)
    assert mask.shape == (1, 512, 612)
    ops.reset_hits()
    with ops.strict():
        check_batch(cuda, pred, gt, mask, True, '96 lights', images=(0, 47, 95))
        pn, gn = normal_batch(5, 1, 512, 612)
        mae = im.evaluate_normals(torch.from_numpy(pn).to(cuda), torch.from_numpy(gn).to(cuda), torch.from_numpy(mask).to(cuda))
    assert not ops.FALLBACKS, dict(ops.FALLBACKS)
    assert abs(float(mae[0]) - metrics.MAE(pn[0], gn[0], mask[0])[0]) <= GATE_MAE


@pytest.mark.parametrize('inten_normalize', [False, True])
def test_evaluate_tool_on_the_device(cuda, tmp_path, capsys, inten_normalize):
    """tools/evaluate.py on a small experiment in the reference's layout: the device run against its own --host run."""
    import importlib.util
    import os
    from tests.helpers import ROOT
    from tests.imgmetrics_data import write_experiment
    spec = importlib.util.spec_from_file_location('psn_tools_evaluate', os.path.join(ROOT, 'tools', 'evaluate.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    test_out, obj, exp, _ = write_experiment(tmp_path, inten_normalize=inten_normalize)
    argv = ['--obj_name', obj, '--expname', exp, '--test_out_dir', test_out]
    dev = tool.main(argv)
    text = capsys.readouterr().out
    host = tool.main(argv + ['--host'])
    print('tools/evaluate.py device %r host %r' % (dev, host))
    assert abs(dev['psnr'] - host['psnr']) <= GATE_PSNR and abs(dev['ssim'] - host['ssim']) <= GATE_SSIM
    assert abs(dev['normal_mae'] - host['normal_mae']) <= GATE_MAE
    assert 'PSNR Error:' in text and 'SSIM Error:' in text and 'Normal MAE Error:' in text and 'LPIPS: not computed' in text
