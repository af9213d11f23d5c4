"""Image evaluation: what the reference's evaluation.py computes for every test view and light -- the white-background compositing
under ``mask_pred & mask_gt``, the optional least-squares intensity scale (``scale_img``), PSNR over the masked pixels and SSIM over
the composited image -- and, per view, the normal MAE.  LPIPS is NOT computed: it needs the pretrained AlexNet weights of the
``lpips`` package, which this project neither ships nor downloads.

Two implementations of one definition, as in meshdist.py:
  * numpy inputs -> the float64 functions below (``host_*``); they are the definition, and what the device path is tested against.
  * device tensors -> csrc/imgmetrics.hip (psn_img_scale_sums, psn_img_metrics, psn_normal_mae) through ``evaluate_images`` /
    ``evaluate_normals``: a whole batch of image pairs per call ([B, H, W, 3] uint8 or float32, one mask per image or one for all),
    float64 arithmetic on the device, results left on the device.

SSIM is skimage.metrics.structural_similarity as stage2/utils/metrics.py:53-62 calls it (data_range=1, channel_axis=2,
gaussian_weights=True, sigma=1.5, use_sample_covariance=False), written out: an 11-tap Gaussian window (radius int(3.5 * 1.5 + 0.5) =
5, weights exp(-x^2 / (2 sigma^2)) normalised to sum 1), applied along axis 0 and then along axis 1 with scipy's 'reflect' border
(d c b a | a b c d | d c b a), to the five planes x, y, x x, y y, x y; S from the filtered planes; the mean of S with a 5-pixel border
cropped, per channel, then the mean of the three channel values.  The taps are added in a fixed order (tap 0 first:
acc = w[0] p[0]; acc = acc + w[k] p[k]), which csrc/imgmetrics.hip follows.
Stated differences from the reference: (1) skimage keeps float32 inputs in float32; the definition here widens to float64 first.
On a 512 x 612 x 3 pair the float32 evaluation is 3.0e-7 away from this one, so the reference's own number sits that far from the
definition.  (2) scale_img's two dot products are float32 BLAS calls of unspecified order in the reference; here they accumulate in
float64 (numpy's float64 dot), and the scaled image stays float64.
"""
import numpy as np
import torch

SIGMA = 1.5
RADIUS = int(3.5 * SIGMA + 0.5)            # 5: skimage's truncate = 3.5
WIN = 2 * RADIUS + 1                       # 11
C1, C2 = (0.01 * 1.0) ** 2, (0.03 * 1.0) ** 2   # (K1 data_range)^2, (K2 data_range)^2
_X = np.arange(-RADIUS, RADIUS + 1).astype(np.float64)
WEIGHTS = np.exp(-0.5 / (SIGMA * SIGMA) * _X ** 2)
WEIGHTS = WEIGHTS / WEIGHTS.sum()          # (the table IM_WEIGHTS of csrc/imgmetrics.hip, bit for bit)


# ------------------------------------------------------------------------------------------------ host path: the definition
def _filter_axis(p, axis):
    """The 11-tap window along ``axis`` of a float64 array, 'reflect' border (np.pad: symmetric), taps added in order 0 .. 10."""
    pad = [(0, 0)] * p.ndim
    pad[axis] = (RADIUS, RADIUS)
    q = np.pad(p, pad, mode='symmetric')
    n = p.shape[axis]
    take = lambda k: q[(slice(None),) * axis + (slice(k, k + n),)]
    acc = WEIGHTS[0] * take(0)
    for k in range(1, WIN):
        acc = acc + WEIGHTS[k] * take(k)
    return acc


def _window(p):
    return _filter_axis(_filter_axis(p, 0), 1)


def host_ssim(img1, img2, full=False):
    """SSIM of two [H, W, 3] images in [0, 1] (see the module docstring) -> float, or (float, map float64 [H, W, 3]) with
    ``full``.  Inputs are taken as they are and widened to float64.  ValueError below 11 pixels in either extent, as skimage."""
    x = np.asarray(img1).astype(np.float64)
    y = np.asarray(img2).astype(np.float64)
    if x.shape != y.shape or x.ndim != 3:
        raise ValueError('host_ssim: two [H, W, C] images of one shape expected, got %s and %s' % (x.shape, y.shape))
    if x.shape[0] < WIN or x.shape[1] < WIN:
        raise ValueError('host_ssim: win_size %d exceeds image extent %s' % (WIN, x.shape[:2]))
    ux, uy = _window(x), _window(y)
    uxx, uyy, uxy = _window(x * x), _window(y * y), _window(x * y)
    vx = uxx - ux * ux
    vy = uyy - uy * uy
    vxy = uxy - ux * uy
    a1, a2 = 2 * ux * uy + C1, 2 * vxy + C2
    b1, b2 = ux ** 2 + uy ** 2 + C1, vx + vy + C2
    S = (a1 * a2) / (b1 * b2)
    crop = S[RADIUS:S.shape[0] - RADIUS, RADIUS:S.shape[1] - RADIUS]
    per_channel = np.array([crop[..., c].mean() for c in range(S.shape[2])])
    mssim = float(per_channel.mean())
    return (mssim, S) if full else mssim


def host_white_bg(x, mask):
    """evaluation.py:26: ``x * mask[..., None] + 1 * ~mask[..., None]`` in float64 (x inside the mask, 1 outside)."""
    m = np.asarray(mask).astype(bool)
    return np.asarray(x).astype(np.float64) * m[..., None] + 1 * ~m[..., None]


def host_scale_img(img, gt, mask):
    """evaluation.py:15-24 -> (scaled image float64, scale): scale = the mean over the channels of x^ . x / x^ . x^ over the mask
    (x^ the prediction, x the ground truth), the image (img * scale).clip(0, 1).  The dot products accumulate in float64 (the
    reference's are float32 BLAS calls of unspecified order)."""
    m = np.asarray(mask).astype(bool)
    img = np.asarray(img).astype(np.float64)
    gt = np.asarray(gt).astype(np.float64)
    opt_scale = []
    for i in range(3):
        x_hat = img[:, :, i][m]
        x = gt[:, :, i][m]
        opt_scale.append(x_hat.dot(x) / x_hat.dot(x_hat))
    opt_scale = np.array(opt_scale).mean()
    return (img * opt_scale).clip(0, 1), float(opt_scale)


def _as_float_images(a):
    a = np.asarray(a)
    if a.dtype == np.uint8:
        a = a.astype(np.float32) / 255.           # evaluation.py:82,85
    return a[None] if a.ndim == 3 else a


def host_evaluate_images(pred, gt, mask, inten_normalize=False):
    """evaluation.py:81-89 for a batch: pred / gt [B, H, W, 3] (or one [H, W, 3]) uint8 or float, mask [B, H, W] or [1, H, W] (what the
    script calls mask_pred & mask_gt) -> (psnr [B], ssim [B], scale [B]) float64.  The ground truth is the image inside the mask and
    1 outside; the prediction is optionally scaled (host_scale_img; scale = 1 otherwise) and composited the same way; PSNR runs over
    the masked pixels, SSIM over the whole composited image."""
    from .metrics import PSNR
    pred, gt = _as_float_images(pred), _as_float_images(gt)
    mask = np.asarray(mask).astype(bool)
    mask = mask[None] if mask.ndim == 2 else mask
    B = pred.shape[0]
    if mask.shape[0] not in (1, B):
        raise ValueError('host_evaluate_images: mask batch %d is neither 1 nor B = %d' % (mask.shape[0], B))
    psnr, ssim, scale = np.zeros(B), np.zeros(B), np.ones(B)
    for b in range(B):
        m = mask[0 if mask.shape[0] == 1 else b]
        g = host_white_bg(gt[b], m)
        p = pred[b]
        if inten_normalize:
            p, scale[b] = host_scale_img(p, g, m)
        p = host_white_bg(p, m)
        psnr[b] = PSNR(p, g, m)
        ssim[b] = host_ssim(p, g)
    return psnr, ssim, scale


def to_img(x):
    """stage2/eval.py:17, the reference's 8-bit quantisation: clip to [0, 1], x 255, round half to even, uint8 -- numpy arrays and
    tensors alike, so that a device render is evaluated at the precision at which the reference reads it back from its PNG."""
    if torch.is_tensor(x):
        return (x.to(torch.float32).clamp(0, 1) * 255).round().to(torch.uint8)
    return (np.asarray(x).astype(np.float32).clip(0, 1) * 255).round().astype(np.uint8)


def load_image(path):
    """An image file as the array the reference gets from imageio.imread (uint8 [H, W, 3], [H, W] for a single-channel mask), read
    with PIL."""
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


# ------------------------------------------------------------------------------------------------ device path
def _batched(t, dims, name):
    if not torch.is_tensor(t):
        raise RuntimeError('%s must be a HIP device tensor (host arrays: psnerf_amd.imgmetrics.host_evaluate_images)' % name)
    return (t[None] if t.dim() == dims - 1 else t).contiguous()


def evaluate_images(pred, gt, mask, inten_normalize=False, full=False):
    """host_evaluate_images on the device for a whole batch: pred / gt [B, H, W, 3] device tensors, both uint8 or both float32;
    mask [B, H, W] or [1, H, W] (uint8 / bool; one view's mask serves all of its lights) -> (psnr [B], ssim [B], scale [B]) float64
    device tensors, with ``full`` also the SSIM map [B, H, W, 3].  Nothing is copied back."""
    from . import hip
    pred, gt = _batched(pred, 4, 'pred'), _batched(gt, 4, 'gt')
    if mask is not None:
        mask = _batched(mask, 3, 'mask')
    if inten_normalize:
        sums, _ = hip.img_scale_sums(pred, gt, mask)
        q = sums[:, 0:3] / sums[:, 3:6]
        scale = (((q[:, 0] + q[:, 1]) + q[:, 2]) / 3.0).contiguous()       # np.mean of the three quotients, in its order
    else:
        scale = None
    out = hip.img_metrics(pred, gt, mask, scale=scale, full=full)
    if scale is None:
        scale = torch.ones(pred.shape[0], dtype=torch.float64, device=pred.device)
    return (out['psnr'], out['ssim'], scale, out['map']) if full else (out['psnr'], out['ssim'], scale)


def evaluate_normals(pred, gt, mask, full=False):
    """metrics.MAE per view on the device: pred / gt float32 [B, H, W, 3] (or one [H, W, 3]) normal maps, mask [B, H, W] or
    [1, H, W] -> the mean angular error in degrees per view, float64 [B] on the device (with ``full`` also the per-pixel errors
    [B, H, W])."""
    from . import hip
    pred, gt = _batched(pred, 4, 'pred'), _batched(gt, 4, 'gt')
    B, H, W = pred.shape[:3]
    if mask is not None:
        mask = _batched(mask, 3, 'mask')
        mask = mask.reshape(mask.shape[0], -1)
    sums, _, err = hip.normal_mae(pred.reshape(B, -1, 3), gt.reshape(B, -1, 3), mask, normalize=True, full=full)
    mae = sums[:, 0] / sums[:, 1]
    return (mae, err.reshape(B, H, W)) if full else mae
