"""Final image / normal metrics of the stage-2 evaluation under the reference's names and signatures
(stage2/utils/metrics.py:17-62): MAE, PSNR, SSIM.  numpy inputs take the host path, float64 numpy as in the reference (SSIM:
psnerf_amd.imgmetrics.host_ssim, skimage's structural_similarity written out); device tensors take csrc/imgmetrics.hip through
psnerf_amd.hip (float64 on the device, one image per call here -- whole batches: psnerf_amd.imgmetrics.evaluate_images /
evaluate_normals) and return Python floats like the host path.  LPIPS is not provided: it needs pretrained AlexNet weights."""
import math

import numpy as np
import torch


def _device_image(x, name):
    if not torch.is_tensor(x) or x.dim() != 3:
        raise RuntimeError('%s: a [H, W, 3] device tensor expected next to a tensor argument, got %s' % (name, type(x).__name__ if not torch.is_tensor(x) else tuple(x.shape)))
    return x[None].contiguous()


def _device_mask(mask, shape):
    if mask is None:
        return None
    if not torch.is_tensor(mask):
        raise RuntimeError('mask: a device tensor expected next to device images')
    if mask.dtype not in (torch.bool, torch.uint8):
        mask = mask != 0
    return mask.reshape((1,) + tuple(shape)).contiguous()


def MAE(vec1, vec2, mask=None, normalize=True):
    """Mean angular error in degrees between two normal maps [N,3] or [H,W,3] (metrics.py:17-37).
    Returns (mean, per-pixel errors of the masked pixels).  Zero vectors stay zero (=> 90 degrees)."""
    if torch.is_tensor(vec1) or torch.is_tensor(vec2):
        from . import hip
        if not (torch.is_tensor(vec1) and torch.is_tensor(vec2)):
            raise RuntimeError('MAE: a tensor and a numpy array (both device tensors, or both numpy arrays)')
        m = _device_mask(mask, (vec1.numel() // 3,))
        sums, _, err = hip.normal_mae(vec1.reshape(1, -1, 3).contiguous(), vec2.reshape(1, -1, 3).contiguous(), m, normalize=normalize, full=True)
        total, count = sums[0].tolist()
        return total / count, (err[0].reshape(vec1.shape[:-1]) if m is None else err[0][m[0] != 0])
    a = np.array(vec1, dtype=np.float64, copy=True)
    b = np.array(vec2, dtype=np.float64, copy=True)
    if normalize:
        na = np.linalg.norm(a, axis=-1)
        nb = np.linalg.norm(b, axis=-1)
        a = a / (na[..., None] + 1e-5)
        b = b / (nb[..., None] + 1e-5)
        a[na == 0] = 0
        b[nb == 0] = 0
    dots = np.clip((a * b).sum(-1), -1.0, 1.0)
    if mask is not None:
        dots = dots[np.asarray(mask).astype(bool)]
    err = np.degrees(np.arccos(dots))
    return err.mean(), err


def PSNR(img1, img2, mask=None):
    """-10 log10(mean squared error) over the masked pixels of two [H,W,3] images in [0,1]; 100 when identical
    (metrics.py:39-51)."""
    if torch.is_tensor(img1) or torch.is_tensor(img2):
        from . import hip
        a, b = _device_image(img1, 'PSNR'), _device_image(img2, 'PSNR')
        return float(hip.img_metrics(a, b, _device_mask(mask, a.shape[1:3]))['psnr'][0])
    a = np.asarray(img1, dtype=np.float64)
    b = np.asarray(img2, dtype=np.float64)
    if mask is not None:
        m = np.asarray(mask).astype(bool)
        a, b = a[m], b[m]
    mse = np.mean((a - b) ** 2)
    return 100 if mse == 0 else -10.0 * math.log10(mse)


def SSIM(img1, img2, mask=None, data_range=1, channel_axis=2, gaussian_weights=True, sigma=1.5, use_sample_covariance=False):
    """SSIM of two [H, W, 3] images in [0, 1] (metrics.py:53-62: skimage's structural_similarity with exactly these settings; any
    other setting raises).  The mask is accepted and ignored, as in the reference.  numpy -> imgmetrics.host_ssim; device tensors
    (float32 or uint8) -> psn_img_metrics.  At least 11 pixels per extent."""
    if (data_range, channel_axis, gaussian_weights, sigma, use_sample_covariance) != (1, 2, True, 1.5, False):
        raise ValueError('SSIM: only the reference\'s settings are implemented (data_range=1, channel_axis=2, gaussian_weights=True, '
                         'sigma=1.5, use_sample_covariance=False)')
    if torch.is_tensor(img1) or torch.is_tensor(img2):
        from . import hip
        return float(hip.img_metrics(_device_image(img1, 'SSIM'), _device_image(img2, 'SSIM'), None)['ssim'][0])
    from .imgmetrics import host_ssim
    return host_ssim(img1, img2)


def get_chamfer_dist(src_mesh, tgt_mesh, num_samples=10000, rng=None, device=None):
    """Chamfer distance between two meshes -> (chamfer, raw) (metrics.py:79-101): psnerf_amd.meshdist, on the host for numpy
    meshes and on the device for device tensors or ``device='cuda'``."""
    from .meshdist import get_chamfer_dist as f
    return f(src_mesh, tgt_mesh, num_samples, rng=rng, device=device)


def get_surface_dist(src_mesh, tgt_mesh, num_samples=10000, rng=None, device=None):
    """One-sided mean distance of src_mesh's surface samples to tgt_mesh (metrics.py:103-113): psnerf_amd.meshdist."""
    from .meshdist import get_surface_dist as f
    return f(src_mesh, tgt_mesh, num_samples, rng=rng, device=device)


def evaluate_mesh(pred, gt, num_samples=10000, thresholds=None, iou_points=100000, rng=None, device=None, vote=False, report=False,
                  align=None, align_options=None):
    """Accuracy / completeness, F-score, normal consistency and volume IoU of a mesh against the ground truth -> dict:
    psnerf_amd.mesheval (the reference reports the Chamfer distance only).  ``align``: 'rigid' or 'similarity' registers ``pred`` to
    ``gt`` first (psnerf_amd.meshalign)."""
    from .mesheval import evaluate_mesh as f
    return f(pred, gt, num_samples, thresholds=thresholds, iou_points=iou_points, rng=rng, device=device, vote=vote, report=report, align=align,
             align_options=align_options)
