#!/usr/bin/env python
"""Measure the device Chamfer distance at the shipped extraction size and write profiles/mesh_chamfer.json.

Meshes: the sphere-initialised BEAR network of tools/bench_mesh.py extracted at (resolution 64, upsampling_steps 3) and (64, 2),
kept on the device.  For N = 10 000 and N = 1 000 000 samples per side, HIP events around each phase, --warmup warm-ups, then
median / min / max of --repeats: sampler (both meshes), index build (count / scan / fill, both meshes), the two query launches
(with the sort by home cell, which is part of the path).  Per mesh: faces, cells, list entries, oversize-list length, index bytes.
From the kernel's counter: triangle tests per query and their ratio to the F tests of a brute force; queries/s; peak device memory.
Lane mapping: the shipped thread-per-query kernel with and without the home-cell sort, measured here; the wave-per-query variant
was measured by the run that still had it and removed -- its record in the output file is carried over, marked as such.

    python tools/bench_chamfer.py [--repeats 7] [--warmup 2] [--out profiles/mesh_chamfer.json]
"""
import argparse
import json
import os
import socket
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import extracted_mesh, stat as _stat, sum_phases, write_profile  # noqa: E402


def one_pass(md, meshes, n, seed, events, sort=True, counters=None):
    """One Chamfer evaluation with every phase bracketed (appended to ``events``) -> (chamfer, indices)."""
    from psnerf_amd.meshcore import Phase
    idx = []
    for v, f in meshes:
        index = md.MeshIndex(v, f, profile=True)
        events.extend(('index ' + name, e0, e1) for name, e0, e1 in index.build_events)
        idx.append(index)
    rng = np.random.RandomState(seed)
    with Phase(events, 'sampler'):
        pts = [index.sample_surface(n, rng)[0] for index in idx]
    def query(index, p, n_tests):
        if sort:
            return index.closest_point(p, n_tests=n_tests)[1]
        from psnerf_amd import hip   # the same kernel on the points as they come: the binding below MeshIndex
        return hip.closest_point(index.index, p, order=None, n_tests=n_tests)[1]
    with Phase(events, 'query'):
        d01 = query(idx[1], pts[0], None if counters is None else counters[1:2])
        d10 = query(idx[0], pts[1], None if counters is None else counters[0:1])
    return float((d01.mean() + d10.mean()) / 2), idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_chamfer.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_chamfer: no GPU (this is a measurement; there is no host fall-back)')
    from psnerf_amd import meshdist as md, ops
    import psnerf_amd.stage1 as s1
    from psnerf_amd.synthetic import stage1_cfg
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = s1.NeuralNetwork(stage1_cfg('bear')).to(dev)
    out = {'device': torch.cuda.get_device_name(0), 'box': socket.gethostname(), 'repeats': args.repeats, 'warmup': args.warmup, 'sizes': {}}
    with ops.strict():
        meshes = [extracted_mesh(net, dev, 64, 3), extracted_mesh(net, dev, 64, 2)]
        for n in (10000, 1000000):
            runs = {'sorted': [], 'unsorted': []}
            counters = torch.zeros(2, dtype=torch.int64, device=dev)
            chamfer = None
            for mapping in ('sorted', 'unsorted'):
                for it in range(args.warmup + args.repeats):
                    torch.cuda.synchronize()
                    torch.cuda.reset_peak_memory_stats()
                    counters.zero_()
                    events = []
                    ch, idx = one_pass(md, meshes, n, 0, events, sort=mapping == 'sorted', counters=counters)
                    torch.cuda.synchronize()
                    phases = sum_phases(events)
                    assert chamfer is None or ch == chamfer, 'the result depends on the run'
                    chamfer = ch
                    if it >= args.warmup:
                        runs[mapping].append(dict(phases=phases, peak_mib=torch.cuda.max_memory_allocated() / 2.0 ** 20))
            tests = [int(x) for x in counters.tolist()]
            faces = [int(i.faces.shape[0]) for i in idx]
            names = sorted(runs['sorted'][0]['phases'])
            phases = dict((k, _stat([r['phases'][k] for r in runs['sorted']])) for k in names)
            q_ms = phases['query']['median_ms']
            out['sizes'][str(n)] = {
                'samples_per_side': n, 'chamfer': chamfer, 'phases_ms': phases,
                'total_ms': _stat([sum(r['phases'].values()) for r in runs['sorted']]),
                'queries_per_s': 2.0 * n / (q_ms * 1e-3),
                'triangle_tests_per_query': {'against_fine_mesh': tests[0] / float(n), 'against_coarse_mesh': tests[1] / float(n)},
                'ratio_to_brute_force': {'against_fine_mesh': tests[0] / float(n) / faces[0], 'against_coarse_mesh': tests[1] / float(n) / faces[1]},
                'bound_F_over_100': {'fine_mesh': faces[0] / 100.0, 'met': tests[0] / float(n) < faces[0] / 100.0},
                'lane_mapping_query_ms': {'thread_per_query_sorted_by_home_cell (shipped; the sort is inside the bracket)': phases['query'],
                                          'thread_per_query_unsorted': _stat([r['phases']['query'] for r in runs['unsorted']])},
                'peak_device_memory_mib': max(r['peak_mib'] for r in runs['sorted']),
            }
        out['meshes'] = dict((name, {'faces': int(i.faces.shape[0]), 'vertices': int(i.vertices.shape[0]), 'cells': list(i.n),
                                     'cell_edge': i.cell, 'list_entries': i.n_entries, 'oversize_list': i.n_over, 'index_bytes': i.index_bytes})
                             for name, i in zip(('fine (64, 3)', 'coarse (64, 2)'), idx))
    if os.path.exists(args.out):   # the record of the removed variant travels with the file
        try:
            old = json.load(open(args.out))
            if 'wave_per_query_variant_removed' in old:
                out['wave_per_query_variant_removed'] = old['wave_per_query_variant_removed']
        except ValueError:
            pass
    out['note'] = ('HIP events on the stream; "index *" = both meshes; "query" = both directions incl. the sort by home cell; memory peak '
                   'includes the two meshes')
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
