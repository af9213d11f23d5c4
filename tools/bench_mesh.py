#!/usr/bin/env python
"""Measure the device mesh extraction at the shipped size (extraction: resolution 64, upsampling_steps 3 -> a 513^3 grid) on a
sphere-initialised stage-1 network and write profiles/mesh_extract.json: HIP-event time per phase over the repeats (median, min,
max), rounds, points evaluated, vertices / faces, peak device memory; achieved bytes/s of the fill and count kernels from their
compulsory traffic (one read + one write, resp. one read, of the 4-byte grid); rows/s of the scattered evaluation next to a plain
on_points call over the same number of contiguous points timed in the same run.

    python tools/bench_mesh.py [--repeats 7] [--warmup 2] [--resolution 64] [--upsampling-steps 3] [--out profiles/mesh_extract.json]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import stat as _stat, sum_kernels, sum_phases, write_profile  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--upsampling-steps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_extract.json'))
    args = ap.parse_args()
    from psnerf_amd import hip, ops
    import psnerf_amd.stage1 as s1
    from psnerf_amd.synthetic import stage1_cfg
    from psnerf_amd.stage1.extracting import Extractor3D
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = s1.NeuralNetwork(stage1_cfg('bear')).to(dev)
    n = (args.resolution << args.upsampling_steps) + 1
    runs = []
    with ops.strict():
        for it in range(args.warmup + args.repeats):
            ex = Extractor3D(net, device=dev, resolution0=args.resolution, upsampling_steps=args.upsampling_steps)
            ex.phase_events = []
            hip.PROFILE_EVENTS = []
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.time()
            mesh, stats = ex.generate_mesh()
            torch.cuda.synchronize()
            wall = time.time() - t0
            kern, hip.PROFILE_EVENTS = hip.PROFILE_EVENTS, None
            if it < args.warmup:
                continue
            phases = sum_phases(ex.phase_events)
            phases.update(('kernel ' + name, ms) for name, ms in sum_kernels(kern).items())
            runs.append(dict(phases=phases, wall_ms=1e3 * wall, stats=stats, n_vertices=len(mesh.vertices), n_faces=len(mesh.faces),
                             peak_mib=torch.cuda.max_memory_allocated() / 2.0 ** 20))
        # the yardstick: the same pack over the same number of CONTIGUOUS points, gathered outputs
        n_pts = runs[-1]['stats']['n_points_evaluated']
        pack = net._logit_packed()
        pts = (torch.rand(n_pts, 3, device=dev) - 0.5) * 2.4
        plain = []
        for it in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            pack.on_points(pts, net.octaves_pe, 1.0 / net.rescale)
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                plain.append(e0.elapsed_time(e1))
    names = sorted(runs[0]['phases'])
    phases = dict((k, _stat([r['phases'].get(k, 0.0) for r in runs])) for k in names)
    grid_bytes = 4.0 * n ** 3
    fill, count, ev = phases['kernel grid_ffill']['median_ms'], phases['kernel mc_count']['median_ms'], phases['kernel mlp_infer']['median_ms']
    out = {
        'device': torch.cuda.get_device_name(0), 'grid': '%d^3' % n, 'resolution0': args.resolution, 'upsampling_steps': args.upsampling_steps,
        'repeats': args.repeats, 'warmup': args.warmup,
        'phases_ms': phases, 'wall_ms': _stat([r['wall_ms'] for r in runs]),
        'device_total_ms': _stat([sum(v for k, v in r['phases'].items() if not k.startswith('kernel ')) for r in runs]),
        'rounds': runs[-1]['stats']['n_rounds'], 'points_evaluated': n_pts, 'points_of_grid': n ** 3,
        'vertices': runs[-1]['n_vertices'], 'faces': runs[-1]['n_faces'], 'peak_device_memory_mib': max(r['peak_mib'] for r in runs),
        'fill_tb_per_s': 2.0 * grid_bytes / (fill * 1e-3) / 1e12, 'count_tb_per_s': grid_bytes / (count * 1e-3) / 1e12,
        'evaluation': {'scattered_list_ms': phases['kernel mlp_infer'], 'scattered_rows_per_s': n_pts / (ev * 1e-3),
                       'plain_on_points_ms': _stat(plain), 'plain_rows_per_s': n_pts / (float(np.median(plain)) * 1e-3),
                       'ratio_scattered_over_plain': float(np.median(plain)) / ev},
        'note': 'phases without the "kernel" prefix partition the device work of one extraction (HIP events on the stream); "kernel *" '
                'entries are the brackets around single C-ABI launches inside them (mlp_infer = all rounds summed)',
    }
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
