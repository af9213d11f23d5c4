#!/usr/bin/env python3
"""Calibrated photometric stereo over a dataset directory in the reference's layout: the per-view normal maps that stage 1 is
regularised with, the per-light intensities and light_avg.py's averaged / intensity-normalised images.

    python tools/photometric_stereo.py --path dataset --obj bunny [--light-avg] [--light-intnorm] [--host]

Reads   <path>/<obj>/params.json (n_view, light_is_same, light_direction: the CALIBRATED lights, in each view's camera frame),
        img/view_XX/NNN.png, mask/view_XX.png.
Writes  sdps_out_l<L>/outnpy/view_XX.npy   float32 [H, W, 3], what stage1/dataloading/dataset.py:101 loads as the estimated normal
        norm_mask/view_XX.png              255 where the estimate is valid (dataset.py:87)
        sdps_out_l<L>/light_intensity_pred.npy   [n_view, L, 3], what light_avg.py --sdps loads
        (sdps_out/ without the suffix when the views have their own lights)
  --light-avg       img/avg_l<L>/view_XX.png (img/avg/ for per-view lights): light_avg.py without --light_intnorm
  --light-intnorm   img_intnorm_sdps_l<L>/view_XX/NNN.png and img_intnorm_sdps_l<L>/avg/view_XX.png: light_avg.py --light_intnorm --sdps,
                    with its choice of the light the intensities are relative to (light 4 for shared lights, light 1 otherwise)
The directory names are the reference's, so its loaders find the files; the normals are this project's estimate from the calibrated
lights, not SDPS-Net's.  --host runs the float64 numpy definition instead of the device kernels.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--obj', required=True)
    ap.add_argument('--path', default='dataset')
    ap.add_argument('--host', action='store_true', help='the numpy definition instead of the device kernels')
    ap.add_argument('--light-avg', action='store_true')
    ap.add_argument('--light-intnorm', action='store_true')
    ap.add_argument('--n-iter', type=int, default=1, help='rounds of normals <-> intensities')
    ap.add_argument('--low', type=float, default=0.1)
    ap.add_argument('--high', type=float, default=0.25)
    ap.add_argument('--dark', type=float, default=0.0)
    args = ap.parse_args(argv)

    import numpy as np
    import torch
    from PIL import Image
    from psnerf_amd import photostereo as ps
    from psnerf_amd.imgmetrics import load_image

    base = os.path.join(args.path, args.obj)
    with open(os.path.join(base, 'params.json')) as f:
        para = json.load(f)
    n_view, same = para['n_view'], para['light_is_same']
    suffix = '_l%d' % len(para['light_direction']) if same else ''
    est_dir = os.path.join(base, 'sdps_out' + suffix)
    norm_dir = os.path.join(base, 'img_intnorm_sdps' + suffix)
    os.makedirs(os.path.join(est_dir, 'outnpy'), exist_ok=True)
    os.makedirs(os.path.join(base, 'norm_mask'), exist_ok=True)
    on_device = not args.host
    put = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if on_device else (lambda a: a)
    get = (lambda t: t.cpu().numpy()) if on_device else (lambda a: a)
    save = lambda a, *path: Image.fromarray(a).save(os.path.join(*path))

    intensities, n_valid, n_masked = [], 0, 0
    for vi in range(n_view):
        view = 'view_%02d' % (vi + 1)
        ld = np.asarray(para['light_direction'] if same else para['light_direction'][vi], dtype=np.float64)
        mask = load_image(os.path.join(base, 'mask', view + '.png')).astype(bool)
        if mask.ndim == 3:
            mask = mask[..., 0]
        images = np.stack([load_image(os.path.join(base, 'img', view, '%03d.png' % (li + 1)))[..., :3] for li in range(ld.shape[0])])
        d_images, d_mask = put(images), put(mask)
        out = ps.estimate(d_images, d_mask, put(ld), n_iter=args.n_iter, low=args.low, high=args.high, dark=args.dark)
        np.save(os.path.join(est_dir, 'outnpy', view + '.npy'), get(out['normal']).astype(np.float32))
        valid = get(out['valid'])
        save(valid * np.uint8(255), base, 'norm_mask', view + '.png')
        e = get(out['light_int'])
        intensities.append(e)
        n_valid += int(valid.sum())
        n_masked += int(mask.sum())
        if args.light_avg:
            avg_dir = os.path.join(base, 'img', 'avg' + suffix)
            os.makedirs(avg_dir, exist_ok=True)
            save(get(ps.light_average(d_images, d_mask)[1]), avg_dir, view + '.png')
        if args.light_intnorm:
            relat = e / e[3 if same else 0][None]          # light_avg.py:55
            _, mean_u8, norm = ps.light_average(d_images, d_mask, put(relat))
            os.makedirs(os.path.join(norm_dir, 'avg'), exist_ok=True)
            os.makedirs(os.path.join(norm_dir, view), exist_ok=True)
            save(get(mean_u8), norm_dir, 'avg', view + '.png')
            norm = get(norm)
            for li in range(ld.shape[0]):
                save(norm[li], norm_dir, view, '%03d.png' % (li + 1))
    np.save(os.path.join(est_dir, 'light_intensity_pred.npy'), np.array(intensities) if same else np.array(intensities, dtype=object),
            allow_pickle=True)
    report = {'views': n_view, 'lights': int(len(para['light_direction'])) if same else [len(l) for l in para['light_direction']],
              'valid_fraction': n_valid / max(n_masked, 1), 'normals': est_dir, 'device': on_device}
    print(json.dumps(report))
    return report


if __name__ == '__main__':
    main()
