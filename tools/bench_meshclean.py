#!/usr/bin/env python
"""Measure the device mesh clean-up (psnerf_amd/meshclean.py, csrc/meshclean.hip) on the mesh of the shipped extraction setting
(resolution 64, upsampling_steps 3 -> a 513^3 grid) of a sphere-initialised stage-1 network, and on the same mesh with a few thousand
small closed pieces appended so that there is something to remove, and write profiles/mesh_clean.json: HIP-event time per phase
(labelling, table, compaction) and wall time of keep=1 over the repeats (median, min, max), the brackets around the single C-ABI
launches with their algorithmic bytes against a device-to-device copy timed in the same run, the numpy definition's time on the same
box, and the extraction's own time from profiles/mesh_extract.json.  The labelling is a single pass: it has no rounds to report.

    python tools/bench_meshclean.py [--repeats 7] [--warmup 2] [--pieces 4096] [--out profiles/mesh_clean.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import extracted_mesh, stat as _stat, sum_phases, write_profile  # noqa: E402


def octahedra(count, seed=0, radius=0.004, box=1.1):
    """``count`` closed pieces of 6 vertices and 8 outward-oriented faces at seeded positions in [-box, box]^3."""
    g = np.random.RandomState(seed)
    corner = radius * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    tri = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int64)
    centre = (g.rand(count, 3) * 2.0 - 1.0) * box
    v = (centre[:, None, :] + corner[None, :, :]).reshape(-1, 3)
    f = (tri[None, :, :] + 6 * np.arange(count)[:, None, None]).reshape(-1, 3)
    return v, f


def measure(v, f, repeats, warmup, copy_gb_per_s):
    from psnerf_amd import hip, meshclean
    runs = []
    for it in range(warmup + repeats):
        events, hip.PROFILE_EVENTS = [], []
        torch.cuda.synchronize()
        t0 = time.time()
        out_v, out_f, _n, report = meshclean._device_clean(v, f, None, 1, 0, 'faces', events=events)
        torch.cuda.synchronize()
        wall = time.time() - t0
        kern, hip.PROFILE_EVENTS = hip.PROFILE_EVENTS, None
        if it < warmup:
            continue
        kernels = dict((name, (e0.elapsed_time(e1), units)) for name, units, e0, e1, _fl in kern)
        runs.append(dict(phases=sum_phases(events), kernels=kernels, wall_ms=1e3 * wall))
    kernels = {}
    for name in sorted(runs[0]['kernels']):
        ms, nbytes = _stat([r['kernels'][name][0] for r in runs]), runs[0]['kernels'][name][1]
        rate = nbytes / (ms['median_ms'] * 1e-3) / 1e9
        kernels[name] = dict(ms, algorithmic_bytes=int(nbytes), gb_per_s=rate, fraction_of_copy_rate=rate / copy_gb_per_s)
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    host = []
    for _ in range(3):
        t0 = time.time()
        meshclean.host_clean(hv, hf, keep=1)
        host.append(1e3 * (time.time() - t0))
    return {'vertices': int(v.shape[0]), 'faces': int(f.shape[0]), 'components': report['n_components'],
            'faces_removed': report['n_faces_removed'], 'vertices_removed': report['n_vertices_removed'],
            'vertices_kept': int(out_v.shape[0]), 'faces_kept': int(out_f.shape[0]),
            'phases_ms': dict((k, _stat([r['phases'][k] for r in runs])) for k in sorted(runs[0]['phases'])),
            'device_total_ms': _stat([sum(r['phases'].values()) for r in runs]), 'wall_ms': _stat([r['wall_ms'] for r in runs]),
            'kernels': kernels, 'host_definition_ms': _stat(host)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--upsampling-steps', type=int, default=3)
    ap.add_argument('--pieces', type=int, default=4096)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_clean.json'))
    args = ap.parse_args()
    from psnerf_amd import ops
    import psnerf_amd.stage1 as s1
    from psnerf_amd.synthetic import stage1_cfg
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = s1.NeuralNetwork(stage1_cfg('bear')).to(dev)
    with ops.strict():
        v, f = extracted_mesh(net, dev, args.resolution, args.upsampling_steps)
        # the yardstick of the byte counts: a device-to-device copy of 256 MiB (read + write), timed here
        src = torch.empty(1 << 28, dtype=torch.uint8, device=dev)
        copies = []
        for it in range(args.warmup + args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            src.clone()
            e1.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                copies.append(e0.elapsed_time(e1))
        copy_gb_per_s = 2.0 * src.numel() / (float(np.median(copies)) * 1e-3) / 1e9
        pv, pf = octahedra(args.pieces)
        v2 = torch.cat([v, torch.from_numpy(pv).to(dev)])
        f2 = torch.cat([f, torch.from_numpy(pf).to(dev) + v.shape[0]])
        out = {'device': torch.cuda.get_device_name(0), 'grid': '%d^3' % ((args.resolution << args.upsampling_steps) + 1),
               'repeats': args.repeats, 'warmup': args.warmup, 'copy_gb_per_s': copy_gb_per_s,
               'extracted': measure(v, f, args.repeats, args.warmup, copy_gb_per_s),
               'extracted_plus_pieces': dict(measure(v2, f2, args.repeats, args.warmup, copy_gb_per_s), pieces=args.pieces)}
    extract = os.path.join(ROOT, 'profiles', 'mesh_extract.json')
    if os.path.exists(extract):
        with open(extract) as fh:
            out['extraction_device_total_ms_from_mesh_extract_json'] = json.load(fh)['device_total_ms']['median_ms']
    out['note'] = ('clean_mesh(keep=1) on device tensors; phases partition its device work (HIP events on the stream; "table" and "compaction" '
                   'each contain one host read); kernels = the brackets around single C-ABI calls with the bytes they must move '
                   '(psnerf_amd/hip.py), against a 256 MiB device-to-device copy timed in the same run; labelling is one pass, no rounds; '
                   'host_definition_ms = meshclean.host_clean (numpy) on the same box, 3 runs')
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
