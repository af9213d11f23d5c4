#!/usr/bin/env python
"""The counterpart of the reference's evaluation.py: image PSNR / SSIM over every test view and light and the normal MAE over
every test view of one experiment, on the GPU.

    python tools/evaluate.py --obj_name bear --expname test_1 [--test_out_dir stage2/test_out] [--host]

Same arguments, same directory layout (evaluation.py:37-89):
    <test_out_dir>/<obj_name>/<expname>/runconf.conf               dataset.data_dir, dataset.all_view, dataset.inten_normalize, ...
    <test_out_dir>/<obj_name>/<expname>/rgb/img/view_VV/LLL.png    rendered images
    <test_out_dir>/<obj_name>/<expname>/mask/img/view_VV.png       rendered mask
    <test_out_dir>/<obj_name>/<expname>/normal/npy/view_VV.npy     rendered normals
    <data_dir>/params.json, norm_mask/view_VV.png, normal/npy/view_VV.npy, img | img_intnorm_gt /view_VV/LLL.png
runconf.conf is read with psnerf_amd.stage2.conf (pyhocon is not a dependency), images with PIL.  A view's images are uploaded once
and all of its lights are evaluated in one call (psnerf_amd.imgmetrics.evaluate_images, one [1, H, W] mask for the view); only the
per-image results come back.  ``--host`` runs the float64 numpy definition instead (no GPU needed; minutes, not seconds).
LPIPS is not computed: it needs the pretrained AlexNet weights of the lpips package, which are not part of this project.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description='Evaluation')
    ap.add_argument('--obj_name', type=str, default='bear')
    ap.add_argument('--expname', type=str, default='test_1')
    ap.add_argument('--test_out_dir', type=str, default='stage2/test_out')
    ap.add_argument('--host', action='store_true', help='run the float64 numpy definition on the CPU instead of the device kernels')
    args = ap.parse_args(argv)

    import torch
    from psnerf_amd import imgmetrics as im
    from psnerf_amd import metrics
    from psnerf_amd.stage2.conf import load_conf
    if not args.host and not torch.cuda.is_available():
        raise SystemExit('evaluate: no GPU visible (the device path has no fall-back; --host runs the numpy definition)')
    dev = None if args.host else torch.device('cuda:0')

    test_out_path = os.path.join(args.test_out_dir, args.obj_name, args.expname)
    conf = load_conf(os.path.join(test_out_path, 'runconf.conf'))
    data_path = conf.get_string('dataset.data_dir')
    train_all_view = conf.get_bool('dataset.all_view', default=False)
    inten_normalize = conf.get_string('dataset.inten_normalize', default=None)
    im_sub = 'img_intnorm_gt' if inten_normalize is not None else 'img'
    if data_path.startswith('../'):
        data_path = data_path[3:]
    with open(os.path.join(data_path, 'params.json')) as f:
        para = json.load(f)

    n_view = para['n_view']
    test_slt = np.arange(n_view) if train_all_view else np.array(para['view_test'])
    poses = np.array(para['pose_c2w']).astype(np.float32)
    if para['light_is_same']:
        n_light = len(para['light_direction'])
        if train_all_view:
            n_light = conf.get_int('dataset.train_light', default=n_light)
        light_slt = [np.arange(n_light)] * len(test_slt)
        print('evaluation_view: %d , light is same,  evaluation_light: %d' % (len(test_slt), n_light))
    else:
        light_slt = [np.arange(len(ll)) for li, ll in enumerate(para['light_direction']) if li in test_slt]
        print('evaluation_view: %d , evaluation_light: %s' % (len(test_slt), [len(li) for li in light_slt]))

    scale_on = inten_normalize == 'sdps'
    psnr_all, ssim_all, normal_data = [], [], []
    for vidx, vi in enumerate(test_slt):
        view = 'view_%02d' % (vi + 1)
        mask_gt = im.load_image(os.path.join(data_path, 'norm_mask', view + '.png')).astype(bool)
        mask_pred = im.load_image(os.path.join(test_out_path, 'mask/img', view + '.png')).astype(bool)
        mask = mask_pred & mask_gt
        if os.path.exists(os.path.join(data_path, 'normal')):
            normal_gt = np.load(os.path.join(data_path, 'normal/npy', view + '.npy'))
            if not para['gt_normal_world']:
                normal_gt = np.einsum('ij,hwj->hwi', poses[vi, :3, :3], normal_gt)
            normal_pred = np.load(os.path.join(test_out_path, 'normal/npy', view + '.npy'))
            if args.host:
                normal_data.append(metrics.MAE(normal_pred, normal_gt, mask)[0])
            else:
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
                normal_data.append(im.evaluate_normals(up(normal_pred), up(normal_gt), torch.from_numpy(mask).to(dev))[0])
        # a view's images: loaded, uploaded once, all lights in one call
        gts = np.stack([im.load_image(os.path.join(data_path, im_sub, view, '%03d.png' % (li + 1)))[..., :3] for li in light_slt[vidx]])
        preds = np.stack([im.load_image(os.path.join(test_out_path, 'rgb/img', view, '%03d.png' % (li + 1)))[..., :3] for li in light_slt[vidx]])
        if args.host:
            psnr, ssim, _ = im.host_evaluate_images(preds, gts, mask[None], inten_normalize=scale_on)
        else:
            psnr, ssim, _ = im.evaluate_images(torch.from_numpy(preds).to(dev), torch.from_numpy(gts).to(dev), torch.from_numpy(mask[None]).to(dev),
                                               inten_normalize=scale_on)
        psnr_all.append(psnr)
        ssim_all.append(ssim)
        print('\rview: %d/%d, lights: %02d' % (vidx + 1, len(test_slt), len(light_slt[vidx])), end='')
    print()
    if not args.host:       # one copy back: the per-image results
        psnr_all = [p.cpu().numpy() for p in psnr_all]
        ssim_all = [s.cpu().numpy() for s in ssim_all]
        normal_data = [float(x) for x in normal_data]
    out = {'psnr': float(np.concatenate(psnr_all).mean()), 'ssim': float(np.concatenate(ssim_all).mean())}
    print('PSNR Error:  %.2f' % out['psnr'])
    print('SSIM Error:  %.4f' % out['ssim'])
    print('LPIPS: not computed (it needs the pretrained AlexNet weights of the lpips package, which this project does not ship)')
    if len(normal_data) > 0:
        out['normal_mae'] = float(np.array(normal_data).mean())
        print('Normal MAE Error:  %.2f' % out['normal_mae'])
    return out


if __name__ == '__main__':
    main()
