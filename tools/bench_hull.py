#!/usr/bin/env python
"""Measure silhouette carving on the device (psnerf_amd/hull.py, csrc/hull.hip) and write profiles/hull_carve.json.

The rig: 20 views of 512 x 612 (the dataset's size) on a ring around a sphere of radius 0.5, fx = 700, analytic silhouettes.  HIP events
on the stream, median / min / max of --repeats after --warmup warm-ups:
  * the dilation of the 20 masks by disk(12) (psn_mask_dilate: pack + dilate), and by the diamond of 2 for context;
  * ``carve_grid`` on a 513^3 grid (the shipped extraction size) with the 20 dilated masks, lattice points per second, the number carved;
  * ``carve_points`` on 1 M uniform points of the box, float32 and float64.
Beside them, in the same run: a device-to-device copy of the 513^3 grid (the yardstick: the grid kernel reads no grid element and
writes only the carved ones, so it is bound by the projections, not by the grid's bytes), and the numpy definition's time on a
sub-sample (one mask for the dilation, 100 000 points for the carving), scaled to the full size.

    python tools/bench_hull.py [--repeats 7] [--warmup 2] [--out profiles/hull_carve.json]
"""
import argparse
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import stat as _stat, write_profile  # noqa: E402

H, W, FX, DISTANCE, RADIUS = 512, 612, 700.0, 2.0, 0.5


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


def look_at(eye):
    z = -eye / np.linalg.norm(eye)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x /= np.linalg.norm(x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, np.cross(z, x), z, eye
    return m.astype(np.float32)


def rig(V):
    K = np.array([[FX, 0.0, (W - 1) / 2.0], [0.0, FX, (H - 1) / 2.0], [0.0, 0.0, 1.0]], dtype=np.float32)
    ang = 2.0 * np.pi * (np.arange(V) + 0.25) / V
    poses = np.stack([look_at(np.array([DISTANCE * np.cos(a), DISTANCE * np.sin(a), 0.4 * np.sin(3.0 * a)])) for a in ang])
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    q = np.stack([(xs - float(K[0, 2])) / FX, (ys - float(K[1, 2])) / FX, np.ones_like(xs)], axis=-1)
    masks = []
    for p in poses:
        depth = float(np.linalg.norm(p[:3, 3]))
        along = depth / np.linalg.norm(q, axis=-1)
        masks.append(((depth * depth - along * along) <= RADIUS ** 2).astype(np.uint8) * 255)
    return np.stack(masks), K, poses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--views', type=int, default=20)
    ap.add_argument('--n', type=int, default=513, help='lattice points per axis')
    ap.add_argument('--points', type=int, default=1000000)
    ap.add_argument('--commit', default=None, help='the commit the tree stands on (default: git rev-parse, where there is a .git)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hull_carve.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_hull: no GPU (this is a measurement; there is no host fall-back)')
    from psnerf_amd import hip, hull
    dev = torch.device('cuda:0')
    commit = args.commit
    if commit is None:
        try:
            commit = subprocess.check_output(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            pass
    V, n, Q = args.views, args.n, args.points
    masks, K, poses = rig(V)
    d_masks = torch.from_numpy(masks).to(dev)
    disk, diamond = hull.disk_footprint(12), hull.diamond_footprint(2)
    out = {'device': torch.cuda.get_device_name(0), 'box': socket.gethostname(), 'parent_commit': commit, 'repeats': args.repeats,
           'warmup': args.warmup, 'views': V, 'image': [H, W], 'grid': '%d^3' % n}

    # dilation
    dilated = hip.mask_dilate(d_masks, disk)
    out['dilate_disk12_ms'] = timed(lambda: hip.mask_dilate(d_masks, disk, out=dilated), args.warmup, args.repeats)
    scratch = torch.empty_like(dilated)
    out['dilate_diamond2_ms'] = timed(lambda: hip.mask_dilate(d_masks, diamond, out=scratch), args.warmup, args.repeats)
    out['dilate_disk12_pixels_per_s'] = V * H * W / (out['dilate_disk12_ms']['median_ms'] * 1e-3)
    t0 = time.time()
    host_one = hull.host_dilate(masks[:1], disk)
    host_dilate_ms = 1e3 * (time.time() - t0)
    out['dilate_disk12_equals_the_definition_on_view_0'] = bool(np.array_equal(dilated[0].cpu().numpy(), host_one[0]))
    out['host_definition'] = {'dilate_disk12_one_mask_ms': host_dilate_ms, 'dilate_disk12_scaled_to_all_masks_ms': host_dilate_ms * V}

    # the grid
    views = torch.from_numpy(hull._views(K, poses, V)).to(dev)
    axis = (2.4 * torch.linspace(-0.5, 0.5, n)).to(torch.float64).to(dev)
    grid = torch.zeros((n, n, n), dtype=torch.float32, device=dev)
    count = int(hip.hull_grid(grid, axis, views, dilated).item())
    out['carve_grid_ms'] = timed(lambda: hip.hull_grid(grid, axis, views, dilated), args.warmup, args.repeats)
    out['carve_grid_points_carved'], out['carve_grid_fraction_carved'] = count, count / float(n ** 3)
    out['carve_grid_lattice_points_per_s'] = n ** 3 / (out['carve_grid_ms']['median_ms'] * 1e-3)
    other = torch.empty_like(grid)
    out['grid_copy_ms'] = timed(lambda: other.copy_(grid), args.warmup, args.repeats)
    out['carve_grid_over_grid_copy'] = out['carve_grid_ms']['median_ms'] / out['grid_copy_ms']['median_ms']
    del other

    # points
    g = torch.Generator(device='cpu').manual_seed(0)
    p64 = ((torch.rand(Q, 3, generator=g, dtype=torch.float64) - 0.5) * 2.4)
    d64 = p64.to(dev)
    d32 = d64.to(torch.float32)
    keep, by = hip.hull_points(d64, views, dilated)
    out['carve_points_f64_ms'] = timed(lambda: hip.hull_points(d64, views, dilated, out=(keep, by)), args.warmup, args.repeats)
    out['carve_points_f32_ms'] = timed(lambda: hip.hull_points(d32, views, dilated, out=(keep, by)), args.warmup, args.repeats)
    out['carve_points'] = Q
    out['carve_points_per_s'] = Q / (out['carve_points_f64_ms']['median_ms'] * 1e-3)
    sub = 100000
    hd = dilated.cpu().numpy()
    t0 = time.time()
    _, hby = hull.host_carve_points(p64[:sub].numpy(), hd, K, poses)
    host_ms = 1e3 * (time.time() - t0)
    keep, by = hip.hull_points(d64, views, dilated)
    out['carve_points_equal_the_definition_on_the_subsample'] = bool(np.array_equal(by[:sub].cpu().numpy(), hby))
    out['host_definition'].update({'carve_points_subsample': sub, 'carve_points_subsample_ms': host_ms,
                                   'carve_points_scaled_to_all_points_ms': host_ms * Q / sub,
                                   'carve_grid_scaled_from_the_subsample_ms': host_ms * n ** 3 / sub})
    out['note'] = ('HIP events on the stream around the single C-ABI calls (psn_mask_dilate is two launches: pack and dilate).  The rig: '
                   'views on a ring at distance 2 around a sphere of radius 0.5, 512 x 612, fx = 700, analytic silhouettes dilated by disk(12).  '
                   'grid_copy = a device-to-device copy of the float32 grid, the yardstick.  host_definition = the numpy definition on the same '
                   'box: one mask for the dilation, a sub-sample of the points for the carving, scaled linearly to the full sizes.  No time gate.')
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
