#!/usr/bin/env python
"""Measure the device mesh connectivity and smoothing (psnerf_amd/meshtopo.py, psnerf_amd/meshsmooth.py, csrc/meshtopo.hip) on the mesh
of the shipped extraction setting (resolution 64, upsampling_steps 3 -> a 513^3 grid) of a sphere-initialised stage-1 network, and
write profiles/mesh_smooth.json, by the protocol of tools/bench_simplify.py: HIP-event time per phase (median of 7 after 2 warm-ups):
the edge keys, the sort with its head-flag scan and host read, the edge kernel, the rings, the corner runs and the vertex normals, one
smoothing step, ten lambda | mu pairs (the whole _device_smooth call, report included); beside them a device-to-device copy of the
vertex array (what one step cannot beat) and the numpy definition's time on the same box.  A record: there is no time gate.

    python tools/bench_smooth.py [--repeats 7] [--warmup 2] [--host-runs 1] [--out profiles/mesh_smooth.json]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from benchlib import extracted_mesh, stat as _stat, sum_kernels, sum_phases, write_profile  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--resolution', type=int, default=64)
    ap.add_argument('--upsampling-steps', type=int, default=3)
    ap.add_argument('--host-runs', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_smooth.json'))
    args = ap.parse_args()
    from psnerf_amd import hip, meshsmooth, meshtopo, ops
    from psnerf_amd.meshcore import Phase
    import psnerf_amd.stage1 as s1
    from psnerf_amd.synthetic import stage1_cfg
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    net = s1.NeuralNetwork(stage1_cfg('bear')).to(dev)
    runs = []
    with ops.strict():
        v, f = extracted_mesh(net, dev, args.resolution, args.upsampling_steps)
        n_v = v.shape[0]
        for it in range(args.warmup + args.repeats):
            events, hip.PROFILE_EVENTS = [], []
            torch.cuda.synchronize()
            table = meshtopo._device_edges(f, n_v, events)                                 # 'edge keys', 'edge sort', 'edge table'
            ring_start, ring = meshtopo._device_rings(table['edges'], n_v, events)         # 'rings'
            normals = meshtopo._device_vertex_normals(v, f, 'area', events, check=False)   # 'corner runs', 'normals'
            with Phase(events, 'report'):
                report = meshtopo._device_report(v, f, table)
            with Phase(events, 'one smoothing step'):
                stepped = hip.topo_smooth_step(v, ring_start, ring, table['vertex_open'], 0.5)
            with Phase(events, 'vertex array copy'):
                copied = v.clone()
            torch.cuda.synchronize()
            t0 = time.time()
            inner = []
            with Phase(events, 'ten Taubin pairs'):
                smooth, smooth_report = meshsmooth._device_smooth(v, f, 10, events=inner)
            torch.cuda.synchronize()
            wall = 1e3 * (time.time() - t0)
            events.append(('ten Taubin pairs: the twenty steps',) + [(e0, e1) for name, e0, e1 in inner if name == 'steps'][0])
            kern, hip.PROFILE_EVENTS = hip.PROFILE_EVENTS, None
            if it >= args.warmup:
                runs.append(dict(phases=sum_phases(events), kernels=sum_kernels(kern), wall_ms=wall))
    hv, hf = v.cpu().numpy(), f.cpu().numpy()
    host = {'edges': [], 'rings': [], 'normals': [], 'ten Taubin pairs': []}
    for _ in range(args.host_runs):
        t0 = time.time()
        host_table = meshtopo.host_edges(hf, n_v)
        t1 = time.time()
        host_ring = meshtopo.host_rings(host_table['edges'], n_v)
        t2 = time.time()
        host_normals = meshtopo.host_vertex_normals(hv, hf, 'area')
        t3 = time.time()
        host_smooth, _ = meshsmooth.host_smooth(hv, hf, 10)
        t4 = time.time()
        for key, ms in zip(('edges', 'rings', 'normals', 'ten Taubin pairs'), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            host[key].append(1e3 * ms)
    same = (all(table[k].cpu().numpy().tobytes() == host_table[k].tobytes() for k in ('edges', 'count', 'forward', 'halfedge_edge', 'counters'))
            and ring.cpu().numpy().tobytes() == host_ring[1].tobytes() and ring_start.cpu().numpy().tobytes() == host_ring[0].tobytes()
            and normals.cpu().numpy().tobytes() == host_normals.tobytes() and smooth.cpu().numpy().tobytes() == host_smooth.tobytes())
    out = {'device': torch.cuda.get_device_name(0), 'grid': '%d^3' % ((args.resolution << args.upsampling_steps) + 1), 'repeats': args.repeats,
           'warmup': args.warmup, 'vertices': int(n_v), 'faces': int(f.shape[0]), 'edges': int(table['n_edges']), 'topology': report,
           'smoothing_report': smooth_report, 'equals_the_numpy_definition_bit_for_bit': bool(same),
           'phases_ms': dict((k, _stat([r['phases'][k] for r in runs])) for k in sorted(runs[0]['phases'])),
           'kernel_launches_ms_summed_over_the_run': dict((k, _stat([r['kernels'][k] for r in runs])) for k in sorted(runs[0]['kernels'])),
           'ten_taubin_pairs_wall_ms': _stat([r['wall_ms'] for r in runs]),
           'host_definition_ms': dict((k, _stat(x)) for k, x in host.items()),
           'vertex_array_bytes': int(24 * n_v), 'ring_entries': int(ring.numel()),
           'note': ('phases = HIP events on the stream: "edge keys" (psn_topo_edge_keys), "edge sort" (the stable torch.sort, head flags, scan and '
                    'the one host read), "edge table" (psn_topo_edges), "rings" (psn_topo_ring_keys, torch.sort, psn_topo_runs), "corner runs" '
                    '(psn_topo_corner_keys, the stable torch.sort, psn_topo_runs), "normals" (psn_topo_vertex_normals), "report" '
                    '(psn_topo_measures and the row of counters read back), "one smoothing step" (psn_topo_smooth_step with the boundary '
                    'pinned), "vertex array copy" (a device-to-device copy of the [V, 3] float64 array: the floor of a step), "ten Taubin '
                    'pairs" (the whole meshsmooth._device_smooth call: edge table, rings, 20 steps, both measures, the report row) and '
                    'its twenty launches of psn_topo_smooth_step alone; kernel_launches = the brackets around single '
                    'C-ABI calls summed over one run of all of the above; host_definition_ms = the numpy definition on the same box')}
    write_profile(args.out, out)


if __name__ == '__main__':
    main()
