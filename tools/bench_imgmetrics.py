#!/usr/bin/env python
"""Measure the device image evaluation at the stated size of configs[4] and write profiles/img_metrics.json.

Synthetic 512 x 612 views, uint8, one [1, H, W] mask per batch (one view's mask for all of its lights); batch sizes 1, 96 (one view's
lights) and 480 (a whole evaluation set).  For each: HIP events around psnerf_amd.imgmetrics.evaluate_images with and without the
intensity scale, and around evaluate_normals; --warmup warm-ups, then median / min / max of --repeats.  Reported next to the times:
the compulsory bytes (two images and one mask read once) and the fraction of the box's streaming rate they amount to -- the kernel is
bound by float64 arithmetic, not by memory, so this fraction is small by construction; it is written down, not promised.  Also the
host definition's time for one image pair on this machine's CPU.

    python tools/bench_imgmetrics.py [--repeats 7] [--warmup 2] [--out profiles/img_metrics.json]
"""
import argparse
import os
import socket
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 512, 612
STREAM_BYTES_PER_S = 6.29e12     # measured float4 copy rate of an MI355X (79 % of the 8 TB/s of the data sheet)


from benchlib import stat as _stat, write_profile  # noqa: E402


def synthetic(B, dev, seed=0):
    """uint8 [B, H, W, 3] pairs on the device: a smooth texture in a disc, white outside; prediction = ground truth + 0.03 x noise."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32) / W, torch.arange(W, dtype=torch.float32) / W, indexing='ij')
    mask = (((yy * W - H / 2.0) / (0.42 * H)) ** 2 + ((xx * W - W / 2.0) / (0.42 * W)) ** 2) <= 1.0
    f = (torch.rand(3, 4, 3, generator=g) * 40.0 - 20.0)
    tex = 0.5 + 0.1 * sum(torch.cos(2 * np.pi * (f[:, k, 0, None, None] * yy + f[:, k, 1, None, None] * xx) + f[:, k, 2, None, None]) for k in range(4))
    tex = tex.permute(1, 2, 0).to(dev)
    m = mask.to(dev)
    gt = torch.where(m[..., None], tex, torch.ones_like(tex))
    gen = torch.Generator(device=dev).manual_seed(seed)
    pred = gt[None] + 0.03 * torch.randn(B, H, W, 3, device=dev, generator=gen) * m[None, ..., None]
    q = lambda x: (x.clamp(0, 1) * 255).round().to(torch.uint8)
    return q(pred).contiguous(), q(gt[None].expand(B, H, W, 3)).contiguous(), m[None].contiguous()


def timed(fn, warmup, repeats):
    out = []
    for it in range(warmup + repeats):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1))
    return _stat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'img_metrics.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_imgmetrics: no GPU (this is a measurement; there is no host fall-back)')
    from psnerf_amd import imgmetrics as im, ops
    dev = torch.device('cuda:0')
    out = {'device': torch.cuda.get_device_name(0), 'box': socket.gethostname(), 'repeats': args.repeats, 'warmup': args.warmup,
           'image': [H, W, 3], 'dtype': 'uint8', 'stream_bytes_per_s_used_for_the_fraction': STREAM_BYTES_PER_S, 'batches': {}}
    with ops.strict():
        for B in (1, 96, 480):
            pred, gt, mask = synthetic(B, dev)
            normals = torch.nn.functional.normalize(torch.randn(B, H, W, 3, device=dev), dim=-1)
            normals2 = (normals + 0.1 * torch.randn_like(normals)).contiguous()
            nbytes = B * H * W * 7          # two uint8 images and one mask byte per pixel (the shared mask is read once per image)
            rec = {'compulsory_bytes': nbytes}
            for name, fn in (('evaluate_images', lambda: im.evaluate_images(pred, gt, mask)),
                             ('evaluate_images_inten_normalize', lambda: im.evaluate_images(pred, gt, mask, inten_normalize=True)),
                             ('evaluate_images_full_map', lambda: im.evaluate_images(pred, gt, mask, full=True)),
                             ('evaluate_normals', lambda: im.evaluate_normals(normals, normals2, mask))):
                rec[name] = timed(fn, args.warmup, args.repeats)
            ms = rec['evaluate_images']['median_ms']
            rec['ms_per_image_pair'] = ms / B
            rec['fraction_of_streaming_rate'] = nbytes / (ms * 1e-3) / STREAM_BYTES_PER_S
            psnr, ssim, _ = im.evaluate_images(pred, gt, mask)
            rec['mean_psnr_db'], rec['mean_ssim'] = float(psnr.mean()), float(ssim.mean())
            out['batches'][str(B)] = rec
            if B == 1:
                p, g, m = pred.cpu().numpy(), gt.cpu().numpy(), mask.cpu().numpy()
                t = []
                for _ in range(3):
                    t0 = time.time()
                    h = im.host_evaluate_images(p, g, m)
                    t.append(time.time() - t0)
                out['host_definition_one_pair'] = {'seconds_median_of_3': float(np.median(t)), 'cpu_threads': torch.get_num_threads(),
                                                   'ssim': float(h[1][0]), 'device_minus_host_ssim': float(ssim[0]) - float(h[1][0]),
                                                   'device_minus_host_psnr_db': float(psnr[0]) - float(h[0][0])}
            del pred, gt, normals, normals2
    out['note'] = ('HIP events on the stream around the whole call (kernel launches and the allocation of the outputs); '
                   'evaluate_images = psn_img_metrics + its fixed-order reduce; inten_normalize adds psn_img_scale_sums; full_map also '
                   'writes the float64 [B, H, W, 3] SSIM map')
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
