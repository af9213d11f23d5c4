"""Synthetic, deterministic image pairs for the image-evaluation tests: a smooth random texture inside a disc mask and white
outside; the prediction is the ground truth + 0.03 x noise, quantised to 8 bits (SSIM lands around 0.86)."""
import numpy as np


def smooth_texture(g, h, w):
    """[h, w, 3] in [0.1, 0.9]: four random cosines per channel, up to 20 cycles across the longer extent."""
    yy, xx = np.meshgrid(np.arange(h) / float(max(h, w)), np.arange(w) / float(max(h, w)), indexing='ij')
    out = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(4):
            fy, fx, ph = g.uniform(-20, 20), g.uniform(-20, 20), g.uniform(0, 2 * np.pi)
            out[..., c] += np.cos(2 * np.pi * (fy * yy + fx * xx) + ph)
    return 0.5 + 0.1 * out


def disc_mask(h, w, shift=0.0):
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    return ((yy - h / 2.0 - shift) ** 2 / (0.42 * h) ** 2 + (xx - w / 2.0 + shift) ** 2 / (0.42 * w) ** 2) <= 1.0


def image_batch(seed, B, h, w, per_image_masks=False, gain=1.0):
    """-> (pred uint8 [B, h, w, 3], gt uint8 [B, h, w, 3], mask bool [B or 1, h, w]).  gain: the prediction's intensity relative to
    the ground truth's (what scale_img undoes)."""
    g = np.random.RandomState(seed)
    nm = B if per_image_masks else 1
    mask = np.stack([disc_mask(h, w, shift=0.04 * min(h, w) * i) for i in range(nm)])
    pred, gt = [], []
    for b in range(B):
        m = mask[b if per_image_masks else 0][..., None]
        t = smooth_texture(g, h, w) * m + 1.0 * ~m
        p = (t * gain + 0.03 * g.standard_normal(t.shape)) * m + 1.0 * ~m
        gt.append((np.clip(t, 0, 1) * 255).round().astype(np.uint8))
        pred.append((np.clip(p, 0, 1) * 255).round().astype(np.uint8))
    return np.stack(pred), np.stack(gt), mask


def normal_batch(seed, B, h, w):
    """-> (pred float32 [B, h, w, 3], gt float32 [B, h, w, 3]): unit-ish normals, the prediction perturbed; a block of zero vectors
    in each, and a block where both agree exactly."""
    g = np.random.RandomState(seed)
    gt = g.standard_normal((B, h, w, 3))
    gt /= np.linalg.norm(gt, axis=-1, keepdims=True)
    pred = gt * g.uniform(0.5, 2.0, (B, h, w, 1)) + 0.1 * g.standard_normal((B, h, w, 3))
    pred[:, :3, :4] = 0.0
    gt[:, 2:5, 2:6] = 0.0
    pred[:, 6:9, :] = gt[:, 6:9, :]
    return pred.astype(np.float32), gt.astype(np.float32)


def write_experiment(root, h=40, w=52, n_view=3, view_test=(1, 2), n_light=4, inten_normalize=False, seed=0):
    """A small experiment in the directory layout tools/evaluate.py (the reference's evaluation.py) walks, built from the synthetic
    images above -> (test_out_dir, obj_name, expname, expected) with expected = the per-image inputs for a direct evaluation:
    a list over the test views of (pred uint8 [L, h, w, 3], gt uint8 [L, h, w, 3], mask bool [h, w], normal_pred, normal_gt_world)."""
    import json
    import os
    from PIL import Image
    data = os.path.join(str(root), 'dataset', 'toy')
    out = os.path.join(str(root), 'test_out', 'toy', 'exp')
    sub = 'img_intnorm_gt' if inten_normalize else 'img'
    g = np.random.RandomState(seed)
    poses = []
    for v in range(n_view):
        q, _ = np.linalg.qr(g.standard_normal((3, 3)))
        pose = np.eye(4)
        pose[:3, :3] = q
        poses.append(pose.tolist())
    params = {'n_view': n_view, 'view_test': list(view_test), 'light_is_same': True, 'gt_normal_world': False, 'pose_c2w': poses,
              'light_direction': g.standard_normal((n_light, 3)).tolist()}
    os.makedirs(data)
    with open(os.path.join(data, 'params.json'), 'w') as f:
        json.dump(params, f)
    os.makedirs(out)
    with open(os.path.join(out, 'runconf.conf'), 'w') as f:
        f.write('train{\n    expname = exp\n}\ndataset{\n    data_dir = %s\n    all_view = False\n%s}\n'
                % (data, '    inten_normalize = sdps\n' if inten_normalize else ''))
    expected = []
    for vi in view_test:
        view = 'view_%02d' % (vi + 1)
        pred, gt, _ = image_batch(seed + 10 * vi, n_light, h, w, gain=0.8 if inten_normalize else 1.0)
        mask_gt, mask_pred = disc_mask(h, w), disc_mask(h, w, shift=1.5)
        for d, name in ((os.path.join(data, 'norm_mask'), mask_gt), (os.path.join(out, 'mask', 'img'), mask_pred)):
            os.makedirs(d, exist_ok=True)
            Image.fromarray((name * 255).astype(np.uint8)).save(os.path.join(d, view + '.png'))
        for d, imgs in ((os.path.join(data, sub, view), gt), (os.path.join(out, 'rgb', 'img', view), pred)):
            os.makedirs(d)
            for li in range(n_light):
                Image.fromarray(imgs[li]).save(os.path.join(d, '%03d.png' % (li + 1)))
        npred, ngt = normal_batch(seed + vi, 1, h, w)
        for d, n in ((os.path.join(data, 'normal', 'npy'), ngt[0]), (os.path.join(out, 'normal', 'npy'), npred[0])):
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, view + '.npy'), n)
        world = np.einsum('ij,hwj->hwi', np.array(poses[vi], dtype=np.float32)[:3, :3], ngt[0])
        expected.append((pred, gt, mask_gt & mask_pred, npred[0], world))
    return os.path.join(str(root), 'test_out'), 'toy', 'exp', expected
