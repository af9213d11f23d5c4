#!/usr/bin/env python
"""Measure the device photometric stereo at the stated size of configs[4] and write profiles/ps_normals.json.

One synthetic 512 x 612 view under 96 lights, uint8 (90 MB).  HIP events around psn_ps_normals on both of its paths (the g tile in LDS;
g re-formed from the image bytes), with and without light_int, around the intensity pass and the light average; --warmup warm-ups,
then median / min / max of --repeats.  Next to them, in the same run: a device-to-device copy of the same 90 MB, and the numpy
definition on this machine's CPU (once; --no-host skips it), whose result is also compared with the device's bit for bit.

    python tools/bench_ps.py [--repeats 7] [--warmup 2] [--out profiles/ps_normals.json]
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

H, W, L = 512, 612, 96


from benchlib import stat as _stat, write_profile  # noqa: E402


def synthetic(dev, seed=0):
    """uint8 [L, H, W, 3] on the device: a bumpy Lambertian surface in a disc under lights normalize((0, 0, 1) + 0.6 randn), cast
    shadows as random dark patches, 8-bit noise -> (images, mask bool [H, W], light_dir float64 [L, 3])."""
    g = torch.Generator(device='cpu').manual_seed(seed)
    ld = torch.nn.functional.normalize(torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)[None] + 0.6 * torch.randn(L, 3, generator=g, dtype=torch.float64), dim=-1)
    yy, xx = torch.meshgrid((torch.arange(H, dtype=torch.float32, device=dev) + 0.5) / H * 2 - 1, (torch.arange(W, dtype=torch.float32, device=dev) + 0.5) / W * 2 - 1,
                            indexing='ij')
    r2 = xx * xx + yy * yy
    mask = r2 < 0.81
    n = torch.stack([xx + 0.1 * torch.sin(25 * yy), yy + 0.1 * torch.cos(31 * xx), torch.sqrt((1.0 - r2).clamp(min=0.05))], -1)
    n = torch.nn.functional.normalize(n, dim=-1)
    rho = torch.stack([0.5 + 0.3 * torch.sin(9 * xx), 0.5 + 0.3 * torch.cos(7 * yy), 0.4 + 0.2 * xx * yy], -1)
    gen = torch.Generator(device=dev).manual_seed(seed)
    images = torch.empty(L, H, W, 3, dtype=torch.uint8, device=dev)
    for l in range(L):
        cos = (n * ld[l].float().to(dev)).sum(-1).clamp(min=0)
        img = rho * cos[..., None] * (1.0 + 0.02 * torch.randn(H, W, 3, device=dev, generator=gen))
        shadow = torch.rand(H // 16, W // 17 + 1, device=dev, generator=gen) < 0.1
        shadow = shadow.repeat_interleave(16, 0).repeat_interleave(17, 1)[:H, :W]
        img = torch.where(shadow[..., None] | ~mask[..., None], torch.zeros_like(img), img)
        images[l] = (img.clamp(0, 1) * 255).round().to(torch.uint8)
    return images, mask, ld.to(dev)


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
    ap.add_argument('--no-host', action='store_true', help='skip the numpy definition (about a minute of CPU time)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ps_normals.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ps: no GPU (this is a measurement; there is no host fall-back)')
    from psnerf_amd import hip, photostereo as ps
    dev = torch.device('cuda:0')
    images, mask, ld = synthetic(dev)
    N = H * W
    flat, fmask = images.reshape(L, N, 3), mask.reshape(N).contiguous()
    e = (0.5 + torch.rand(L, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))).to(dev)
    nbytes = L * N * 3
    out = {'device': torch.cuda.get_device_name(0), 'box': socket.gethostname(), 'repeats': args.repeats, 'warmup': args.warmup,
           'view': [L, H, W, 3], 'dtype': 'uint8', 'image_bytes': nbytes, 'masked_pixels': int(mask.sum()),
           'ranking_comparisons': int(mask.sum()) * L * L}
    bufs = tuple(torch.empty(s, dtype=d, device=dev) for s, d in (((N, 3), torch.float64), ((N, 3), torch.float64), ((N,), torch.uint8), ((N,), torch.int32)))
    for name, kw in (('ps_normals_tile', dict(path='tile')), ('ps_normals_reform', dict(path='reform')),
                     ('ps_normals_tile_light_int', dict(path='tile', light_int=e)), ('ps_normals_reform_light_int', dict(path='reform', light_int=e)),
                     ('ps_normals_tile_no_trim', dict(path='tile', low=0.0, high=0.0))):
        out[name] = timed(lambda: hip.ps_normals(flat, fmask, ld, out=bufs, **kw), args.warmup, args.repeats)
    normal, albedo, valid, kept = hip.ps_normals(flat, fmask, ld)
    out['valid_pixels'] = int(valid.sum())
    out['kept_lights_mean'] = float(kept[fmask].double().mean())
    out['ps_light_intensity'] = timed(lambda: hip.ps_light_intensity(flat, normal, albedo, valid, ld), args.warmup, args.repeats)
    out['ps_light_average'] = timed(lambda: hip.ps_light_average(flat, fmask), args.warmup, args.repeats)
    out['ps_light_average_normalised'] = timed(lambda: hip.ps_light_average(flat, fmask, e), args.warmup, args.repeats)
    out['estimate_one_round'] = timed(lambda: ps.estimate(images, mask, ld), args.warmup, args.repeats)
    dst = torch.empty_like(images)
    out['device_to_device_copy_of_the_images'] = timed(lambda: dst.copy_(images), args.warmup, args.repeats)
    ms = out['ps_normals_tile']['median_ms']
    out['ps_normals_tile_over_copy'] = ms / out['device_to_device_copy_of_the_images']['median_ms']
    out['ps_normals_tile_comparisons_per_s'] = out['ranking_comparisons'] / (ms * 1e-3)
    out['ps_normals_tile_image_bytes_per_s'] = nbytes / (ms * 1e-3)
    if not args.no_host:
        h_img, h_mask, h_ld = images.cpu().numpy(), mask.cpu().numpy(), ld.cpu().numpy()
        t0 = time.time()
        h = ps.host_photometric_stereo(h_img, h_mask, h_ld)
        t_n = time.time() - t0
        t0 = time.time()
        h_e = ps.host_light_intensity(h_img, h_mask, h[0], h[1], h[2], h_ld)
        t_e = time.time() - t0
        t0 = time.time()
        h_avg = ps.host_light_average(h_img, h_mask)
        t_a = time.time() - t0
        same = lambda t, a: bool(np.array_equal(t.cpu().numpy().view(np.uint8), np.ascontiguousarray(a).view(np.uint8)))
        d_e = hip.ps_light_intensity(flat, normal, albedo, valid, ld)[0].cpu().numpy()
        d_avg = hip.ps_light_average(flat, fmask)
        out['host_definition'] = {
            'photometric_stereo_seconds': t_n, 'light_intensity_seconds': t_e, 'light_average_seconds': t_a, 'cpu_threads': torch.get_num_threads(),
            'device_equals_host_bit_for_bit': {'normal': same(normal, h[0].reshape(N, 3)), 'albedo': same(albedo, h[1].reshape(N, 3)),
                                               'valid': same(valid, h[2].reshape(N)), 'kept': same(kept, h[3].reshape(N)),
                                               'light_average_mean': same(d_avg[0], h_avg[0].reshape(N, 3)),
                                               'light_average_u8': same(d_avg[1], h_avg[1].reshape(N, 3))},
            'light_intensity_max_relative_difference': float(np.abs(d_e / h_e - 1.0).max()), 'light_intensity_gate': N * 2.0 ** -50}
    out['note'] = ('HIP events on the stream around the whole call; ps_normals writes into preallocated outputs, the other entries allocate '
                   'theirs; estimate_one_round = normals + intensities through psnerf_amd.photostereo.estimate')
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
