#!/usr/bin/env python
"""Measure the device mesh simplification (psnerf_amd/meshsimplify.py, csrc/meshsimplify.hip) on the mesh of the shipped extraction
setting (resolution 64, upsampling_steps 3 -> a 513^3 grid) of a sphere-initialised stage-1 network, and write
profiles/mesh_simplify.json, by the protocol of tools/bench_meshclean.py: HIP-event time per phase and wall time over the repeats
(median of 7 after 2 warm-ups), the brackets around the single C-ABI launches, and the numpy definition's time on the same box, for
  * target_faces = a tenth of the faces (the probes of the bisection are a phase of their own), and
  * one fixed resolution (no probes), and
  * a coarse grid (resolution 2: a few clusters whose corner runs hold hundreds of thousands of entries each).
A quality figure is recorded beside the times (a record, not a gate): get_surface_dist in both directions between the fine mesh and
its simplification to a quarter of its faces, and the same two distances between the fine mesh and the (64, 2) extraction, which has
about that many faces -- "why not extract coarser?" as a number.

    python tools/bench_simplify.py [--repeats 7] [--warmup 2] [--resolution-fixed 128] [--resolution-coarse 2] [--out profiles/mesh_simplify.json]
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

from benchlib import extracted_mesh, stat as _stat, sum_kernels, sum_phases, write_profile  # noqa: E402


def measure(v, f, repeats, warmup, host_runs, **size):
    from psnerf_amd import hip, meshsimplify
    runs = []
    for it in range(warmup + repeats):
        events, hip.PROFILE_EVENTS = [], []
        torch.cuda.synchronize()
        t0 = time.time()
        out_v, out_f, report = meshsimplify._device_simplify(v, f, events=events, **size)
        torch.cuda.synchronize()
        wall = time.time() - t0
        kern, hip.PROFILE_EVENTS = hip.PROFILE_EVENTS, None
        if it < warmup:
            continue
        runs.append(dict(phases=sum_phases(events), kernels=sum_kernels(kern), wall_ms=1e3 * wall))
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    host = []
    for _ in range(host_runs):
        t0 = time.time()
        host_v, host_f, _ = meshsimplify.host_simplify(hv, hf, **size)
        host.append(1e3 * (time.time() - t0))
    same = host_v.tobytes() == out_v.cpu().numpy().tobytes() and np.array_equal(host_f, out_f.cpu().numpy())
    report = dict(report, probes=[[n, c if c != float('inf') else None] for n, c in report['probes']])
    total = _stat([sum(r['phases'].values()) for r in runs])
    out = {'vertices': int(v.shape[0]), 'faces': int(f.shape[0]), 'report': report, 'equals_the_numpy_definition_bit_for_bit': bool(same),
           'phases_ms': dict((k, _stat([r['phases'].get(k, 0.0) for r in runs])) for k in sorted(runs[0]['phases'])),
           'kernel_launches_ms_summed_over_the_call': dict((k, _stat([r['kernels'][k] for r in runs])) for k in sorted(runs[0]['kernels'])),
           'device_total_ms': total, 'wall_ms': _stat([r['wall_ms'] for r in runs]), 'host_definition_ms': _stat(host)}
    if 'probes' in out['phases_ms']:
        out['probes_fraction_of_device_total'] = out['phases_ms']['probes']['median_ms'] / total['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--upsampling-steps', type=int, default=3)
    ap.add_argument('--resolution-fixed', type=int, default=128)
    ap.add_argument('--resolution-coarse', type=int, default=2)
    ap.add_argument('--samples', type=int, default=100000)
    ap.add_argument('--host-runs', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_simplify.json'))
    args = ap.parse_args()
    from psnerf_amd import meshsimplify, ops
    from psnerf_amd.meshdist import MeshIndex, get_surface_dist
    import psnerf_amd.stage1 as s1
    from psnerf_amd.synthetic import stage1_cfg
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = s1.NeuralNetwork(stage1_cfg('bear')).to(dev)
    with ops.strict():
        v, f = extracted_mesh(net, dev, args.resolution, args.upsampling_steps)
        tenth = f.shape[0] // 10
        out = {'device': torch.cuda.get_device_name(0), 'grid': '%d^3' % ((args.resolution << args.upsampling_steps) + 1),
               'repeats': args.repeats, 'warmup': args.warmup,
               'target_faces_a_tenth': measure(v, f, args.repeats, args.warmup, args.host_runs, target_faces=tenth),
               'fixed_resolution': measure(v, f, args.repeats, args.warmup, args.host_runs, resolution=args.resolution_fixed),
               'coarse_resolution': measure(v, f, args.repeats, args.warmup, args.host_runs, resolution=args.resolution_coarse)}
        # quality: the fine mesh against its simplification to a quarter of its faces, and against the extraction one step coarser
        coarse_v, coarse_f = extracted_mesh(net, dev, args.resolution, args.upsampling_steps - 1)
        quarter = f.shape[0] // 4
        simple_v, simple_f, report = meshsimplify._device_simplify(v, f, target_faces=quarter)
        fine, simple, coarse = MeshIndex(v, f), MeshIndex(simple_v, simple_f), MeshIndex(coarse_v, coarse_f)
        rng = np.random.RandomState(0)
        out['quality'] = {
            'samples': args.samples, 'fine_faces': int(f.shape[0]), 'target_faces': int(quarter),
            'simplified': {'faces': int(simple_f.shape[0]), 'vertices': int(simple_v.shape[0]), 'resolution': report['resolution'],
                           'cell': report['cell'], 'n_faces_flipped': report['n_faces_flipped'],
                           'fine_to_simplified': get_surface_dist(fine, simple, args.samples, rng),
                           'simplified_to_fine': get_surface_dist(simple, fine, args.samples, rng)},
            'extracted_one_step_coarser': {'faces': int(coarse_f.shape[0]), 'vertices': int(coarse_v.shape[0]),
                                           'grid': '%d^3' % ((args.resolution << (args.upsampling_steps - 1)) + 1),
                                           'fine_to_coarse': get_surface_dist(fine, coarse, args.samples, rng),
                                           'coarse_to_fine': get_surface_dist(coarse, fine, args.samples, rng)}}
    for name, key in (('mesh_extract.json', 'extraction_device_total_ms_from_mesh_extract_json'),
                      ('mesh_clean.json', 'clean_device_total_ms_from_mesh_clean_json')):
        path = os.path.join(ROOT, 'profiles', name)
        if os.path.exists(path):
            with open(path) as fh:
                data = json.load(fh)
            out[key] = (data['extracted'] if 'extracted' in data else data)['device_total_ms']['median_ms']
    out['note'] = ('_device_simplify on device tensors; phases partition its device work (HIP events on the stream): "probes" = every grid the '
                   'bisection of target_faces tries (key kernels, sorts, count, one host read each), then for the chosen grid "clusters", '
                   '"face keys" (with the host read), "runs" (the corner-key sort, run bounds, keep flags), "solve" (psn_vc_solve) and '
                   '"compaction" (psn_vc_face_flags, two scans, the totals read, psn_cc_compact); kernel_launches = the brackets around '
                   'single C-ABI calls summed over the call (probes included); host_definition_ms = meshsimplify.host_simplify (numpy) on '
                   'the same box; quality = mean distance of surface samples (meshdist.get_surface_dist), world units, box edge 2.4')
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
