#!/usr/bin/env python
"""Measure ray casting against the mesh at the shipped extraction size and write profiles/mesh_raycast.json.

Mesh: the sphere-initialised BEAR network of tools/bench_mesh.py extracted at (resolution 64, upsampling_steps 3), kept on the
device, as the other mesh benches use it.  Two workloads, HIP events around each, --warmup warm-ups, then median / min / max of
--repeats:
  * one 512 x 612 view of primary rays through meshrender.render_view (synthetic.stage1_camera: the object fills ~70 % of the
    image height): the whole call (rays, kernel, maps) and the kernel alone;
  * 20 000 surface points x 96 lights of any-hit shadow rays through meshrender.mesh_light_visibility (lnear 0.1, lfar 3.5): the
    whole call (including the sort by entry cell) and the kernel alone on the sorted order.
From the kernel's counter: ray-triangle tests per ray for both.  For context, the numpy definition's time on a sub-sample of each
ray set, scaled to nothing: it is reported as seconds per 1 000 rays.  Nothing gates on these numbers.

    python tools/bench_raycast.py [--repeats 7] [--warmup 2] [--out profiles/mesh_raycast.json]
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

from benchlib import extracted_mesh, stat as _stat, write_profile  # noqa: E402


def timed(fn, warmup, repeats):
    """fn() bracketed by HIP events -> (stat over the repeats, last result)."""
    ms, out = [], None
    for it in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return _stat(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--host-rays', type=int, default=200, help='rays of each set given to the numpy definition')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_raycast.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_raycast: no GPU (this is a measurement; there is no host fall-back)')
    from psnerf_amd import hip, meshdist as md, meshrender as mr, ops
    import psnerf_amd.stage1 as s1
    from psnerf_amd.stage1.rendering import camera_origin, pixel_rays
    from psnerf_amd.synthetic import stage1_camera, stage1_cfg
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    cfg = stage1_cfg('bear')
    net = s1.NeuralNetwork(cfg).to(dev)
    H, W, n_points, n_lights = 512, 612, 20000, 96
    out = {'device': torch.cuda.get_device_name(0), 'box': socket.gethostname(), 'repeats': args.repeats, 'warmup': args.warmup}
    with ops.strict():
        v, f = extracted_mesh(net, dev, 64, 3)
        index = md.MeshIndex(v, f)
        raw = lambda o, d, t_min, t_max, order, any_hit, n_tests=None: hip.ray_cast(index.index, o, d, t_min, t_max, order=order, any_hit=any_hit,
                                                                                    n_tests=n_tests)
        counter = torch.zeros(1, dtype=torch.int64, device=dev)

        # ---- primary rays: one view
        K, c2w, _ = stage1_camera(cfg, H, W)
        K, c2w = K.to(dev), c2w.to(dev)
        px = mr.tile_pixels(H, W).to(dev)
        o = camera_origin(H * W, c2w)[0].to(torch.float64).contiguous()
        d = pixel_rays(px[None].float(), K, c2w)[0].to(torch.float64).contiguous()
        whole, maps = timed(lambda: mr.render_view(index, K, c2w, H, W), args.warmup, args.repeats)
        kernel, _ = timed(lambda: raw(o, d, 0.0, float('inf'), None, False), args.warmup, args.repeats)
        row_major = torch.argsort(px[:, 1] * W + px[:, 0])          # the same rays, handed over row by row instead of in 8 x 8 tiles
        kernel_rows, _ = timed(lambda: raw(o[row_major].contiguous(), d[row_major].contiguous(), 0.0, float('inf'), None, False), args.warmup, args.repeats)
        counter.zero_()
        hit = raw(o, d, 0.0, float('inf'), None, False, counter)[3]
        view = {'rays': H * W, 'pixels_on_the_mesh': int(maps['mask'].sum()), 'whole_call_ms': whole, 'kernel_ms': kernel,
                'kernel_row_major_pixels_ms': kernel_rows, 'triangle_tests_per_ray': counter.item() / float(H * W),
                'rays_per_s_kernel': H * W / (kernel['median_ms'] * 1e-3)}
        assert int(hit.sum()) == view['pixels_on_the_mesh']

        # ---- any-hit shadow rays: 20 k surface points x 96 lights
        pts, face = index.sample_surface(n_points, np.random.RandomState(0))
        g = np.random.RandomState(1)
        lights = g.standard_normal((n_lights, 3))
        lights[:, 1] = np.abs(lights[:, 1])
        lights = torch.from_numpy(lights / np.linalg.norm(lights, axis=1, keepdims=True)).to(dev)
        whole_s, vis = timed(lambda: mr.mesh_light_visibility(index, pts, lights), args.warmup, args.repeats)
        so = pts[None].expand(n_lights, n_points, 3).reshape(-1, 3).contiguous()
        sd = lights[:, None].expand(n_lights, n_points, 3).reshape(-1, 3).contiguous()
        order = index.entry_order(so, sd, 0.1)
        kernel_s, _ = timed(lambda: raw(so, sd, 0.1, 3.5, order, True), args.warmup, args.repeats)
        kernel_s_unsorted, _ = timed(lambda: raw(so, sd, 0.1, 3.5, None, True), args.warmup, args.repeats)
        first_s, _ = timed(lambda: raw(so, sd, 0.1, 3.5, order, False), args.warmup, args.repeats)
        counter.zero_()
        raw(so, sd, 0.1, 3.5, order, True, counter)
        n_rays = n_points * n_lights
        shadow = {'rays': n_rays, 'points': n_points, 'lights': n_lights, 'hidden_share': float((~vis).double().mean()),
                  'whole_call_ms': whole_s, 'kernel_ms': kernel_s, 'kernel_unsorted_ms': kernel_s_unsorted, 'kernel_first_hit_mode_ms': first_s,
                  'triangle_tests_per_ray': counter.item() / float(n_rays), 'rays_per_s_kernel': n_rays / (kernel_s['median_ms'] * 1e-3)}
    out['mesh'] = {'faces': int(index.faces.shape[0]), 'vertices': int(index.vertices.shape[0]), 'cells': list(index.n), 'cell_edge': index.cell,
                   'list_entries': index.n_entries, 'oversize_list': index.n_over, 'index_bytes': index.index_bytes}

    # ---- the numpy definition on a sub-sample, for context
    hv, hf = index.vertices.cpu().numpy(), index.faces.cpu().numpy()
    host = {}
    for name, (ro, rd, t_min, t_max, any_hit, dev_hit) in (('view', (o, d, 0.0, np.inf, False, hit)),
                                                            ('shadow', (so, sd, 0.1, 3.5, True, (~vis).reshape(-1)))):
        pick = torch.linspace(0, ro.shape[0] - 1, args.host_rays, device=dev).long()
        t0 = time.time()
        h_hit = md.host_ray_cast(hv, hf, ro[pick].cpu().numpy(), rd[pick].cpu().numpy(), t_min, t_max, any_hit=any_hit)[3]
        host[name] = {'rays': int(len(pick)), 'seconds_per_1000_rays': (time.time() - t0) / len(pick) * 1000.0,
                      'hit_equal_to_the_device': bool(np.array_equal(h_hit, dev_hit[pick].bool().cpu().numpy()))}
    out.update({'view_512x612': view, 'shadow_20k_x_96': shadow, 'numpy_definition': host})
    out['note'] = ('HIP events on the stream; "whole_call" = the public function (ray set-up, the sort by entry cell where there is one, the '
                   'kernel, the maps); "kernel" = psn_ray_cast alone on prepared rays in the order the public function uses')
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
